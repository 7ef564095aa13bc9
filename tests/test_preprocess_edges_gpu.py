"""The kernels of csrc/preprocess.hip at their tile and segment edges, on the crafted cases of tests/pre_cases.py (what each
case holds is checked in tests/test_preprocess_edges_cpu.py), against plain fp64 numpy and tests/preprocess_ref.py:

    segments      column segments of 0, 1, 5, 63, 64, 65, N-1 and N entries around the 64-lane butterfly, a time point of one
                  spot, zero-total spots, interleaved input rows, and the t= slices of lognorm_stats / scale_write
    scale tiles   k_pre_scale_write with one, two and three column tiles (S = 15360, 15361, 30721)
    p-values      every branch of k_sparkx_pvals and of its ACAT on crafted moments

Tolerances.  Counts are integers, so counts and sums of counts are exact in fp64.  The log-normalised mean is a sum of at most
131 non-negative terms: relative error (n + 2) u < 1e-13 on either side.  The std comes from a two-pass sum of squares around
that mean: relative error (n + 2) u max|v| / std, and max|v| / std <= 16 on these columns (asserted in the CPU test), so
133 * 2.2e-16 * 16 < 5e-13 per side, 1e-12 in all.  The float32 block keeps the stage test's rtol 2e-6, atol 2e-6; moments,
p-values and ACAT keep the stage test's 1e-10 (1e-15 absolute where ACAT's 1 - cdf cancels)."""
import numpy as np
import pytest
import torch

import pre_cases as pc
import preprocess_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = (1e4, 1e-4)          # the clustering input's target and the output's


def _dc(case):
    from spadot_amd.preprocess import DeviceCounts
    return DeviceCounts(pc.raw_counts(case), DEV)


def _d(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def seg():
    return pc.segments()


@pytest.fixture(scope="module")
def dc(seg):
    return _dc(seg)


def test_rows_are_permuted_into_time_point_blocks(seg, dc):
    np.testing.assert_array_equal(dc.perm, seg.perm)
    assert list(dc.tps) == seg.labels
    np.testing.assert_array_equal(dc.tp_off_host, seg.tp_off)
    assert (dc.X != seg.B).nnz == 0


@pytest.mark.parametrize("thr", [0.01, 3.0, 60000.0])
def test_gene_detect_counts_and_sums_are_exact(seg, dc, thr):
    cnt, colsum = dc.gene_detect(thr)
    D = np.asarray(seg.B.todense())
    for t in range(3):
        blk = D[seg.tp_off[t]:seg.tp_off[t + 1]]
        np.testing.assert_array_equal(cnt[t].cpu().numpy(), (blk >= thr).sum(0))
        np.testing.assert_array_equal(colsum[t].cpu().numpy(), blk.sum(0))


def test_row_total_with_a_mask_per_time_point_is_exact(seg, dc):
    rng = np.random.default_rng(1)
    mask = rng.uniform(size=(3, pc.SEG_G)) < 0.5
    mask[1, pc.SEG_MIDDLE_ONLY] = True
    mask[:, 0], mask[:, pc.SEG_G - 1] = (True, False, True), (False, True, True)
    got = dc.row_total(mask).cpu().numpy()
    D = np.asarray(seg.B.todense())
    want = np.concatenate([(D[seg.tp_off[t]:seg.tp_off[t + 1]] * mask[t]).sum(1) for t in range(3)])
    np.testing.assert_array_equal(got, want)
    assert np.all(got[list(pc.SEG_ZERO_ROWS)] == 0)


def _total(dc, cols):
    mask = np.zeros((dc.T, dc.G), dtype=bool)
    mask[:, np.asarray(cols)] = True
    return dc.row_total(mask)


@pytest.mark.parametrize("target", TARGETS)
def test_lognorm_stats_whole_and_sliced(seg, dc, target):
    cols = np.asarray(pc.SEG_COLS)
    total = _total(dc, cols)
    mean, std = dc.lognorm_stats(cols, total, target)
    assert mean.shape == std.shape == (3, cols.size)
    for t in range(3):
        _, mu, sd = ref.log_stats(seg.B[seg.tp_off[t]:seg.tp_off[t + 1]][:, cols], target)
        np.testing.assert_allclose(mean[t].cpu().numpy(), mu, rtol=1e-13, atol=0)
        np.testing.assert_allclose(std[t].cpu().numpy(), sd, rtol=1e-12, atol=0)
        m1, s1 = dc.lognorm_stats(cols, total, target, t=t)
        assert m1.shape == (1, cols.size)
        assert torch.equal(m1[0], mean[t]) and torch.equal(s1[0], std[t])
    assert torch.all(std[1] == 1)                                      # one spot: std 0 -> 1
    k = pc.SEG_COLS.index(pc.SEG_ALL_ZERO)
    assert torch.all(mean[:, k] == 0) and torch.all(std[:, k] == 1)    # an empty column: mean 0, std 0 -> 1


@pytest.mark.parametrize("clip", [0.0, 1.5])
@pytest.mark.parametrize("target", TARGETS)
def test_scale_write_whole_and_sliced(seg, dc, target, clip):
    cols = np.asarray(pc.SEG_COLS)
    total = _total(dc, cols)
    mean, std = dc.lognorm_stats(cols, total, target)
    Z = dc.scale_write(cols, total, target, mean, std, clip=clip)
    assert Z.shape == (202, cols.size) and Z.dtype == torch.float32
    for t in range(3):
        lo, hi = int(seg.tp_off[t]), int(seg.tp_off[t + 1])
        want = ref.normalize_log_scale(seg.B[lo:hi][:, cols], target, clip or None)
        np.testing.assert_allclose(Z[lo:hi].cpu().numpy(), want.astype(np.float32), rtol=2e-6, atol=2e-6)
        Zt = dc.scale_write(cols, total, target, mean[t:t + 1], std[t:t + 1], clip=clip, t=t)
        assert Zt.shape == (hi - lo, cols.size) and torch.equal(Zt, Z[lo:hi])
    if clip:
        assert float(Z.abs().max()) == clip and 0 < float((Z.abs() == clip).float().mean()) < 0.9
    assert torch.all(Z[70] == 0)                                       # the single spot of the middle time point


def _close(got, want, rtol):
    scale = np.abs(want).max() if want.size else 1.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * scale)


def test_sparkx_moments_on_short_segments(seg, dc):
    from spadot_amd._lib import model_lib
    rng = np.random.default_rng(2)
    rowmap = np.full(202, -1, dtype=np.int32)
    xts, pairs, want = [], [], {}
    off = 0
    for t in (0, 2):
        rows = pc.kept_rows(seg, t)
        loc = seg.spatial_block[rows]
        sets = [loc] + [ref.transloc_func_vec(loc, k, "gaussian") for k in range(5)] + \
            [ref.transloc_func_vec(loc, k, "cosine") for k in range(5)]
        xts.append(np.concatenate([s - s.mean(0, keepdims=True) for s in sets], axis=1))
        rowmap[rows] = off + np.arange(rows.size)
        off += rows.size
        genes = np.flatnonzero(np.asarray(seg.B[rows].sum(0)).ravel() > 0)
        C = seg.B[rows][:, genes].tocsc()
        want[t] = (genes, [ref.sparkx_sk(C, s) for s in sets])
        pairs += [(t, g) for g in genes]
    assert np.all(rowmap[list(pc.SEG_ZERO_ROWS)] == -1)
    pairs = np.asarray(pairs, dtype=np.int32)[rng.permutation(len(pairs))]     # the pair list mixes the time points
    assert np.any(np.diff(pairs[:, 0]) < 0)
    P = pairs.shape[0]
    pt, pg, rm, xt = _d(pairs[:, 0], torch.int32), _d(pairs[:, 1], torch.int32), _d(rowmap, torch.int32), _d(np.concatenate(xts))
    mom = torch.empty((P, 24), dtype=torch.float64, device=DEV)
    rc = model_lib().spadot_sparkx_moments(*dc._csc(), dc.tp_off.data_ptr(), P, pt.data_ptr(), pg.data_ptr(), rm.data_ptr(),
                                           xt.data_ptr(), mom.data_ptr(), _stream())
    assert rc == 0
    mom = mom.cpu().numpy()
    for t, (genes, res) in want.items():
        sel = np.flatnonzero(pairs[:, 0] == t)
        got = mom[sel[np.argsort(pairs[sel, 1])]]                      # in gene order, as `genes`
        np.testing.assert_array_equal(got[:, 0], res[0]["sy"])        # sums of integers below 2^53
        np.testing.assert_array_equal(got[:, 1], res[0]["syy"])
        for k in range(11):
            _close(got[:, 2 + 2 * k:4 + 2 * k], res[k]["ehl"], 1e-10)


# ---------------------------------------------------------------- tiles of k_pre_scale_write
@pytest.mark.parametrize("S", pc.ST_S)
def test_scale_write_across_column_tiles(S):
    from spadot_amd.preprocess import CLUSTER_TARGET, TARGET_SUM, scale_output
    case = pc.scale_tiles(S)
    cols = case.facts["cols"]
    dc = _dc(case)
    assert dc.G == S + pc.ST_EXTRA
    ntile, w = pc.tile_rule(S, pc.PRE_TILE)
    edges = pc.st_edges(S)
    M = case.B[:, cols]
    # the stage's own step 4
    X = scale_output(dc, cols).cpu().numpy()
    want = np.concatenate([ref.normalize_log_scale(M[3 * t:3 * t + 3], TARGET_SUM) for t in range(2)])
    assert X.shape == (6, S)
    np.testing.assert_allclose(X, want.astype(np.float32), rtol=2e-6, atol=2e-6)
    assert np.all(X[0, edges] > X[1, edges]) and np.all(X[4, edges] > X[3, edges])     # a count there, against a row without
    # with a clip, whole and per time point
    total = _total(dc, cols)
    mean, std = dc.lognorm_stats(cols, total, CLUSTER_TARGET)
    Z = dc.scale_write(cols, total, CLUSTER_TARGET, mean, std, clip=1.0)
    want = np.concatenate([ref.normalize_log_scale(M[3 * t:3 * t + 3], CLUSTER_TARGET, 1.0) for t in range(2)])
    np.testing.assert_allclose(Z.cpu().numpy(), want.astype(np.float32), rtol=2e-6, atol=2e-6)
    for t in range(2):
        Zt = dc.scale_write(cols, total, CLUSTER_TARGET, mean[t:t + 1], std[t:t + 1], clip=1.0, t=t)
        assert torch.equal(Zt, Z[3 * t:3 * t + 3])
    # the rows without counts over `cols` are the zero entries' value everywhere
    for r in (pc.ST_EMPTY_ROW, pc.ST_ZERO_TOTAL_ROW):
        t = r // 3
        np.testing.assert_array_equal(Z[r].cpu().numpy(), (-mean[t] / std[t]).clamp(-1.0, 1.0).float().cpu().numpy())


# ---------------------------------------------------------------- k_sparkx_pvals, branch by branch
def _trapezoid_sf(q, l1, l2, nodes):
    """The kernel's documented rule: 1 for q <= 0, the closed form for equal weights, else the trapezoid on `nodes` points."""
    if not q > 0:
        return 1.0
    if l1 == l2:
        return float(np.exp(-q / (2 * l1)))
    th = np.pi * np.arange(nodes) / nodes
    return float(np.mean(np.exp(-q / (2 * (l1 * np.cos(th) ** 2 + l2 * np.sin(th) ** 2)))))


@pytest.mark.parametrize("nodes", [1, 256])
def test_pvalue_kernel_branch_by_branch(nodes):
    from spadot_amd._lib import model_lib
    from spadot_amd.preprocess import PVAL_NODES
    assert PVAL_NODES == 256
    mom, pt, names = pc.pvalue_rows()
    P, n = mom.shape[0], pc.PV_N
    inv = np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (2, 11, 1))
    mom_d, pt_d, nk_d, inv_d, lam_d = _d(mom), _d(pt, torch.int32), _d([n, n], torch.int32), _d(inv), _d(pc.PV_LAM)
    stat = torch.empty((P, 11), dtype=torch.float64, device=DEV)
    pval = torch.empty((P, 11), dtype=torch.float64, device=DEV)
    comb = torch.empty(P, dtype=torch.float64, device=DEV)
    rc = model_lib().spadot_sparkx_pvals(mom_d.data_ptr(), P, pt_d.data_ptr(), nk_d.data_ptr(), inv_d.data_ptr(),
                                         lam_d.data_ptr(), nodes, stat.data_ptr(), pval.data_ptr(), comb.data_ptr(), _stream())
    assert rc == 0
    stat, pval, comb = stat.cpu().numpy(), pval.cpu().numpy(), comb.cpu().numpy()
    assert not np.isnan(pval).any() and not np.isnan(comb).any()
    for i, name in enumerate(names):
        if name in ("ylam_zero", "all_zero"):                          # no null distribution: the kernel's documented p = 1
            assert np.all(pval[i] == 1) and comb[i] == 1, name
            continue
        lam = pc.PV_LAM[pt[i]]
        ylam = 1 - n * (mom[i, 0] / n) ** 2 / mom[i, 1]
        q = (mom[i, 2::2] ** 2 + mom[i, 3::2] ** 2) * n / mom[i, 1]
        np.testing.assert_allclose(stat[i], q, rtol=1e-13, atol=0, err_msg=name)
        if nodes == 1:
            want = [_trapezoid_sf(q[k], ylam * lam[k, 0], ylam * lam[k, 1], 1) for k in range(11)]
        else:
            want = [ref.sf_two_term(q[k], ylam * lam[k, 0], ylam * lam[k, 1]) for k in range(11)]
        np.testing.assert_allclose(pval[i], want, rtol=1e-10, atol=0, err_msg=name)
        assert comb[i] == pytest.approx(ref.acat(pval[i]), rel=1e-10, abs=1e-15), name
        if name in ("q_zero", "one_only"):
            assert comb[i] == 1 and (pval[i] == 1).sum() == (11 if name == "q_zero" else 1)
        elif name in ("underflow", "zero_and_one"):
            assert comb[i] == 0 and pval[i, 0] == 0 and (name == "underflow" or pval[i, 1] == 1)
        elif name in ("one_small_cct", "three_small", "all_small", "small_among_unequal"):
            # cct > 1e15: the combined p is 1 / (pi cct), below the absolute floor of the comparison above, so it is
            # compared here in relative terms with the same formula on the device's own p-values
            small = pval[i][pval[i] < 1e-16]
            assert small.size == {"one_small_cct": 1, "three_small": 3, "all_small": 11, "small_among_unequal": 1}[name]
            rest = np.tan((0.5 - pval[i][pval[i] >= 1e-16]) * np.pi).sum() / 11
            np.testing.assert_allclose(comb[i], 1.0 / (np.pi * (np.sum(1.0 / (11 * np.pi * small)) + rest)), rtol=1e-12, atol=0,
                                       err_msg=name)
        elif name == "one_small_atan":
            assert 0 <= comb[i] < 2e-15 and (pval[i] < 1e-16).sum() == 1
