"""What the Moran stages share on the host (spadot_amd/moran.py), the parts that work on device tensors: the CSR of a call's edge
lists against the numpy restatement of tests/hotspots_ref.py with the refusal of edge ends out of range, and the centre and
spread of a DeviceCounts against those of the same matrix given as dense columns."""
import numpy as np
import pytest
import torch

import hotspots_ref as href
import modules_cases as mcases
from spadot_amd import moran

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _edges(n, rng):
    """An unsorted edge list over n spots with duplicates (none for n = 1): (src, dst) int64."""
    if n == 1:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    src, dst = rng.integers(0, n, 5 * n), rng.integers(0, n, 5 * n)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    src, dst = np.concatenate([src, src[:7], src[:3]]), np.concatenate([dst, dst[:7], dst[:3]])    # duplicates, some twice
    order = rng.permutation(src.size)
    assert np.any(np.diff(src[order]) < 0) or src.size < 2
    return src[order], dst[order]


@pytest.mark.parametrize("dtype", (torch.int32, torch.int64), ids=("int32", "int64"))
@pytest.mark.parametrize("sizes", ((1, 37), (2, 37)), ids=("n1_n37", "n2_n37"))
def test_edge_csr_is_the_stable_sort_by_source_of_every_time_point(sizes, dtype):
    rng = np.random.default_rng(100 * sizes[0] + 7)
    lists = [_edges(n, rng) for n in sizes]
    pairs = [(torch.as_tensor(s, dtype=dtype, device=DEV), torch.as_tensor(d, dtype=dtype, device=DEV)) for s, d in lists]
    rowptr, col, desc = moran.edge_csr(pairs, np.asarray(sizes), torch.device(DEV))
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and rowptr.is_contiguous() and col.is_contiguous()
    assert desc.dtype == np.int64 and desc.shape == (2, 8)
    rowptr, col = rowptr.cpu().numpy(), col.cpu().numpy()
    assert rowptr.shape == (sum(sizes) + 2,) and col.shape == (sum(s.size for s, _ in lists),)
    eoff = roff = row0 = 0
    for t, ((src, dst), n) in enumerate(zip(lists, sizes)):
        want_rp, want_col = href.csr(src, dst, n)
        E = src.size
        assert desc[t].tolist() == [eoff, n, E, row0, t, roff, 0, 0]
        np.testing.assert_array_equal(rowptr[roff:roff + n + 1], want_rp)
        np.testing.assert_array_equal(col[eoff:eoff + E], want_col)
        eoff, roff, row0 = eoff + E, roff + n + 1, row0 + n


def test_edge_ends_out_of_range_are_refused_before_they_are_narrowed():
    rng = np.random.default_rng(5)
    src, dst = _edges(37, rng)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)

    def pairs(d, dtype):
        return [(none, none), (torch.as_tensor(src, dtype=dtype, device=DEV), torch.as_tensor(d, dtype=dtype, device=DEV))]

    sizes = np.asarray([1, 37])
    bad = dst.copy()
    bad[4] = 37
    for dtype in (torch.int32, torch.int64):
        with pytest.raises(ValueError, match=r"time point 1 has edge ends 0 \.\. 37: they must lie in 0 \.\. 36"):
            moran.edge_csr(pairs(bad, dtype), sizes, torch.device(DEV))
    bad[4] = -1
    with pytest.raises(ValueError, match=r"time point 1 has edge ends -1 \.\. 36: they must lie in 0 \.\. 36"):
        moran.edge_csr(pairs(bad, torch.int32), sizes, torch.device(DEV))
    bad[4] = 2 ** 32 + 5                                                             # 5 once narrowed to int32
    with pytest.raises(ValueError, match=r"edge ends 0 \.\. 4294967301: they must lie in 0 \.\. 36"):
        moran.edge_csr(pairs(bad, torch.int64), sizes, torch.device(DEV))
    with pytest.raises(ValueError, match=r"edge ends 0 \.\. 4294967301: they must lie in 0 \.\. 36"):
        moran.refuse_edge_ends(pairs(bad, torch.int64), sizes, wide_only=True)
    bad[4] = 37
    moran.refuse_edge_ends(pairs(bad, torch.int32), sizes, wide_only=True)           # int32 ends: left to autocorr_check
    moran.refuse_edge_ends(pairs(dst, torch.int64), sizes)


def test_centre_and_spread_of_a_device_counts_and_of_the_same_dense_columns_have_equal_bits():
    import scipy.sparse as sp
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.utils._preprocess_utils import RawCounts
    _, _, V = mcases.tile_case(37, 3)                                                # fp32 [37, 3], zeros not stored
    assert V.shape == (37, 3) and V.dtype == np.float32 and (V == 0).any()
    raw = RawCounts(sp.csr_matrix(V), np.zeros(37, dtype=np.int64), np.zeros((37, 2)), np.arange(3).astype(str))
    dc = DeviceCounts(raw, DEV)
    assert dc.perm.tolist() == list(range(37)) and int(dc.cval.numel()) == int((V != 0).sum())
    a = moran.columns(dc, dc.cval)
    b = moran.columns([torch.as_tensor(V, device=DEV)])
    assert a.dense is None and a.counts is dc and b.counts is None and (a.T, a.G, a.n) == (b.T, b.G, b.n) == (1, 3, 37)
    got_a, got_b = moran.centre_spread(a), moran.centre_spread(b)
    for name, x, y in zip(("S0", "centre", "m2", "sumsq"), got_a, got_b):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert x.shape == y.shape == (1, 3) and x.dtype == y.dtype == np.float64
        print(name, x.tolist(), y.tolist())
        if name == "S0":                                                             # the stored count: the dense columns store all
            np.testing.assert_array_equal(x[0], (V != 0).sum(0))
            np.testing.assert_array_equal(y[0], [37, 37, 37])
        else:
            assert x.tobytes() == y.tobytes(), name
    V64 = V.astype(np.float64)
    np.testing.assert_allclose(got_a[1].cpu().numpy()[0], V64.mean(0), rtol=4 * 37 * 2.0 ** -53)
    np.testing.assert_allclose(got_a[3].cpu().numpy()[0], (V64 * V64).sum(0), rtol=4 * 37 * 2.0 ** -53)
