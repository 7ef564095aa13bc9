"""The co-occurrence kernel on the MI355X against the numpy restatement of its definition (tests/cooccur_ref.py, held to its own
conditions by tests/test_cooccurrence_cpu.py): the edge call, sets that straddle the 256-wide tile, the integer lattice, the
set whose thresholds are its own squared distances (a contracted distance would lose pairs there), repeatability, the saturated
counts, the statistics, the refusals and the stage.

Everything the device computes is an integer, so every comparison of counts is assert_array_equal.  The host statistics are
fp64 arithmetic on the same integers: within 1e-12 relative, NaN in the same places."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cooccur_cases as cases
import cooccur_ref as ref
import nhood_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


def _counts(problems, **kw):
    """cooccurrence_counts of [(xy, labels, r2, K)] by squared thresholds."""
    from spadot_amd.cooccurrence import cooccurrence_counts
    return cooccurrence_counts([_dev(p[0]) for p in problems], [p[1] for p in problems], radii_sq=[p[2] for p in problems],
                               n_clusters=[p[3] for p in problems], **kw)


def test_edge_call_matches_the_restatement():
    call = cases.edge_call()
    got = _counts(call)                                                              # B = 1, 16, 17 and 64 in one call
    assert [g.shape for g in got] == [(1, 1, 1), (2, 2, 16), (3, 3, 17), (32, 32, 64)]
    for i, g in enumerate(got):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, cases.want(f"edge{i}"), err_msg=f"problem {i}")
    assert not got[0].any()                                                          # n = 1: no pairs
    np.testing.assert_array_equal(got[1], np.broadcast_to(np.array([[0, 1], [1, 0]])[:, :, None], (2, 2, 16)))
    assert not got[2][1].any() and not got[2][:, 1].any() and got[2][0, 2].any()     # the label value without spots
    assert got[3][:, :, -1].sum() > got[3][:, :, 0].sum()


@pytest.mark.parametrize("n", cases.TILE_SIZES)
def test_sets_that_straddle_the_tile_match_the_restatement(n):
    np.testing.assert_array_equal(_counts([cases.tile_case(n)])[0], cases.want(f"tile{n}"))


def test_the_integer_lattice_matches_the_restatement():
    got = _counts([cases.lattice()])[0]
    np.testing.assert_array_equal(got, cases.want("lattice"))
    np.testing.assert_array_equal(got.sum(axis=(0, 1))[:3], [0, 528, 528 + 484])


def test_pairs_on_their_threshold_count():
    """The thresholds are the set's own unfused squared distances: test_cooccurrence_cpu shows that a contracted distance
    would lose at least three of the 64 pairs that lie on them."""
    xy, lab, r2, K, pairs = cases.on_threshold()
    got = _counts([(xy, lab, r2, K)])[0]
    want = cases.want("on_threshold")
    print("ordered pairs that differ from the restatement, per threshold:", np.abs(got - want).sum(axis=(0, 1)).tolist())
    np.testing.assert_array_equal(got, want)


def test_a_problem_alone_in_a_batch_and_run_twice_gives_the_same_integers():
    call = cases.edge_call()
    prob = cases.tile_case(257)
    alone = _counts([prob])[0]
    np.testing.assert_array_equal(alone, cases.want("tile257"))
    batch = _counts([call[3], cases.tile_case(513), prob, call[1], cases.lattice()])  # other n, K and B around it
    np.testing.assert_array_equal(batch[2], alone)
    np.testing.assert_array_equal(batch[0], cases.want("edge3"))
    np.testing.assert_array_equal(batch[1], cases.want("tile513"))
    np.testing.assert_array_equal(_counts([prob])[0], alone)                          # called twice
    wide = _counts([(prob[0], prob[1], prob[2], 9)])[0]                                # a larger K: the same corner, zeros around
    np.testing.assert_array_equal(wide[:5, :5], alone)
    assert wide.shape == (9, 9, 7) and wide[5:].sum() == 0 and wide[:, 5:].sum() == 0
    many = np.concatenate([prob[2], prob[2][-1] + 1.0 + np.arange(33.0)])             # a larger B: the same leading thresholds
    more = _counts([(prob[0], prob[1], many, 5)])[0]
    assert more.shape == (5, 5, 40)
    np.testing.assert_array_equal(more[:, :, :7], alone)
    out = torch.full((2, 32, 32, 64), -77, dtype=torch.int64, device=DEV)             # every element of the output is written
    both = _counts([prob, call[3]], out=out)
    np.testing.assert_array_equal(both[0], alone)
    res = out.cpu().numpy()
    np.testing.assert_array_equal(res[0, :5, :5, :7], alone)
    assert res[0].sum() == alone.sum() and res.min() == 0


def test_the_device_result_is_symmetric():
    for g in _counts([cases.edge_call()[3], cases.tile_case(513)]):
        np.testing.assert_array_equal(g, g.transpose(1, 0, 2))


@pytest.fixture(scope="module")
def planted():
    from spadot_amd.cooccurrence import cooccurrence
    xy, lab, K = cases.planted_xy()
    return xy, lab, K, cooccurrence([_dev(xy)], [lab], n_clusters=[K])[0]


def test_at_the_diameter_the_device_counts_every_pair(planted):
    from spadot_amd.cooccurrence import cooccurrence_counts
    xy, lab, K, _ = planted
    diameter = np.sqrt(ref.d2_matrix(xy).max())
    got = cooccurrence_counts([_dev(xy)], [_dev(lab)], radii=[[diameter, 2 * diameter]], n_clusters=[K])[0]
    sizes = np.bincount(lab, minlength=K)
    full = np.outer(sizes, sizes) - np.diag(sizes)
    np.testing.assert_array_equal(got[:, :, 1], full)
    assert got[:, :, 0].sum() >= full.sum() - 2                      # the squared root may round below the farthest pair
    far = cooccurrence_counts([_dev(xy)], [lab], radii_sq=[[ref.d2_matrix(xy).max()]], n_clusters=[K])[0]
    np.testing.assert_array_equal(far[:, :, 0], full)


def test_cooccurrence_on_the_planted_set(planted):
    """Counts, statistics and rings of the 45 x 45 planted set under the default radii, and the compactness of its domains:
    ratio[a, a, t] > 1 at every radius that holds pairs (in the restatement 4.49 at the least at index 1, 2.07 at index 49)."""
    from spadot_amd.cooccurrence import cooccurrence
    xy, lab, K, r = planted
    np.testing.assert_array_equal(r.radii, ref.default_radii(xy, 50))
    np.testing.assert_array_equal(r.counts, cases.want("planted"))
    np.testing.assert_array_equal(r.sizes, np.bincount(lab, minlength=K))
    assert r.counts.shape == (K, K, 50) and r.ring is False
    for ring, got in ((False, r), (True, cooccurrence([_dev(xy)], [_dev(lab)], ring=True, n_clusters=[K])[0])):
        want = ref.stats(cases.want("planted"), ring=ring)
        for name in ("ratio", "cond", "marg"):
            np.testing.assert_array_equal(np.isnan(getattr(got, name)), np.isnan(want[name]), err_msg=name)
            np.testing.assert_allclose(getattr(got, name), want[name], rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
    # Planted Voronoi domains are compact: every domain is over-represented around itself at the smallest scale.  The first
    # default radius of this set (0.315) lies below its smallest spot distance (0.409), so no pair exists there and the
    # definition gives NaN; the smallest scale with pairs is index 1.  Asserted there and at every larger radius.
    own = r.ratio[np.arange(K), np.arange(K), :]
    print("ratio[a, a, 1]", np.round(own[:, 1], 2), "smallest over t >= 1", np.round(own[:, 1:].min(), 2))
    assert cases.want("planted")[:, :, 0].sum() == 0 and np.all(np.isnan(own[:, 0]))
    assert np.all(own[:, 1:] > 1)


SENTINEL = -77


def _desc(n=37, K=3, B=17, sizes=(20, 0, 17)):
    d = np.zeros((1, 40), dtype=np.int64)
    d[0, :4] = (0, n, K, B)
    d[0, 5:5 + len(sizes)] = np.cumsum(sizes)
    return d


def test_refusals_come_before_any_launch():
    from spadot_amd import stage_ops as ops
    from spadot_amd.cooccurrence import cooccurrence_counts
    xy, lab, r2, K = cases.edge_call()[2]
    x = _dev(xy)
    out = torch.full((1, 3, 3, 17), SENTINEL, dtype=torch.int64, device=DEV)
    kw = dict(n_clusters=[3], out=out)
    for n_clusters in ([33], [0]):
        with pytest.raises(ValueError, match="1 to 32"):
            cooccurrence_counts([x], [lab], radii_sq=[r2], n_clusters=n_clusters, out=out)
    with pytest.raises(ValueError, match=r"labels must lie in 0 \.\. 1"):
        cooccurrence_counts([x], [lab], radii_sq=[r2], n_clusters=[2], out=out)      # a label >= K
    with pytest.raises(ValueError, match="labels must lie in"):
        cooccurrence_counts([x], [lab - 1], radii_sq=[r2], **kw)                     # a negative label
    with pytest.raises(ValueError, match="1 to 64"):
        cooccurrence_counts([x], [lab], radii_sq=[np.arange(65.0)], **kw)
    with pytest.raises(ValueError, match="1 to 64"):
        cooccurrence_counts([x], [lab], radii_sq=[[]], **kw)
    for bad in ([-1.0, 2.0], [1.0, np.inf], [1.0, np.nan], [1.0, 1.0], [2.0, 1.0]):
        with pytest.raises(ValueError, match="finite, >= 0 and strictly increasing"):
            cooccurrence_counts([x], [lab], radii_sq=[bad], **kw)
        with pytest.raises(ValueError, match="finite, >= 0 and strictly increasing"):
            cooccurrence_counts([x], [lab], radii=[bad], **kw)
    for where, value in ((5, np.nan), (40, np.inf)):
        broken = xy.copy()
        broken.reshape(-1)[where] = value
        with pytest.raises(ValueError, match="not finite"):
            cooccurrence_counts([_dev(broken)], [lab], radii_sq=[r2], **kw)
    with pytest.raises(ValueError, match="at most 65535"):
        cooccurrence_counts([x] * 65536, [lab] * 65536, radii_sq=[r2] * 65536, out=out)
    with pytest.raises(RuntimeError, match="MI355X only.*no CPU path"):
        cooccurrence_counts([torch.as_tensor(xy)], [lab], radii_sq=[r2], **kw)
    with pytest.raises(ValueError, match="a labeling of shape"):
        cooccurrence_counts([x], [lab[:-1]], radii_sq=[r2], **kw)
    for desc, k_max, b_max, what in ((_desc(n=2147483392, sizes=(2147483392, 0, 0)), 3, 17, "spots"), (_desc(K=33), 33, 17, "label values"),
                                     (_desc(B=65), 3, 65, "thresholds"), (_desc(K=4), 3, 17, "label values"),
                                     (_desc(B=18), 3, 17, "thresholds"), (_desc(sizes=(20, 0, 16)), 3, 17, "inconsistent")):
        with pytest.raises(ValueError, match=what):
            ops.cooccur_counts(x, desc, [r2], k_max, b_max, out=out)
    with pytest.raises(ValueError, match="at most 65535"):
        ops.cooccur_counts(x, np.zeros((65536, 40), dtype=np.int64), [r2] * 65536, 3, 17, out=out)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.cooccur_counts(torch.as_tensor(xy), _desc(), [r2], 3, 17)
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)                                                # nothing was launched
    lib = ops.model_lib()                                                            # the library's own checks, from the host copies
    pad = np.full((1, 32), -1.0)
    pad[0, :17] = r2

    def call(desc, thresholds, P=1, k_max=3, b_max=17):
        return lib.spadot_cooccur_counts(x.data_ptr(), ctypes.c_void_p(desc.ctypes.data), _dev(desc).data_ptr(),
                                         ctypes.c_void_p(thresholds.ctypes.data), _dev(thresholds).data_ptr(), P, k_max, b_max,
                                         out.data_ptr(), None)

    for desc in (_desc(n=2147483392, sizes=(2147483392, 0, 0)), _desc(K=4), _desc(K=0), _desc(B=18), _desc(B=0)):
        assert call(desc, pad) == -7, desc[0, :8].tolist()
    assert call(_desc(), pad, k_max=33) == -7 and call(_desc(), pad, b_max=65) == -7 and call(_desc(), pad, b_max=0) == -7
    assert call(_desc(), pad, P=65536) == -7
    for t, value in ((0, -0.5), (3, np.inf), (4, np.nan), (5, pad[0, 4]), (16, pad[0, 2])):
        broken = pad.copy()
        broken[0, t] = value
        assert call(_desc(), broken) == -7, (t, value)
    assert call(_desc(sizes=(20, 0, 16)), pad) == -22
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)
    got = cooccurrence_counts([x], [lab], radii_sq=[r2], **kw)[0]                    # and the same tensor is written by a valid call
    np.testing.assert_array_equal(got, cases.want("edge2"))
    np.testing.assert_array_equal(out.cpu().numpy()[0], got)


STAGE_FILES = ["s_cooccurrence.npz"] + [f"s_cooccurrence_{tp}.csv" for tp in ("E10", "E12", "E14")]


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from spadot_amd.cooccurrence import cooccur
    out = tmp_path_factory.mktemp("cooccurrence")
    df = nhood_cases.stage_table()
    path = os.path.join(out, "domains.csv")
    df.to_csv(path, index=False)
    res = cooccur(argparse.Namespace(domains=path, output_dir=str(out), prefix="s_", bins=50, radius=None, ring=False, device=DEV))
    return df, path, str(out), res


def test_the_stage_writes_its_files(stage):
    import pandas as pd
    from spadot_amd.cooccurrence import TABLE_COLUMNS
    from spadot_amd.utils._analyze_utils import have_matplotlib
    df, path, out, res = stage
    tps = ["E10", "E12", "E14"]
    want = cases.stage_want()
    assert res["timepoints"] == tps and set(res["timings"]) == {"read_s", "device_s", "write_s", "total_s"}
    z = np.load(os.path.join(out, "s_cooccurrence.npz"))
    assert set(z.files) == {"timepoints", "bins", "ring"} | {f"{tp}_{name}" for tp in tps for name in ("counts", "ratio", "radii", "sizes")}
    assert z["timepoints"].tolist() == tps and int(z["bins"]) == 50 and not bool(z["ring"])
    for tp in tps:
        N, radii, K = want[tp]
        np.testing.assert_array_equal(z[f"{tp}_counts"], N, err_msg=tp)
        assert z[f"{tp}_counts"].dtype == np.int64 and z[f"{tp}_counts"].shape == (K, K, 50)
        np.testing.assert_array_equal(z[f"{tp}_radii"], radii)
        m = np.asarray(df["timepoint"]) == tp
        np.testing.assert_array_equal(z[f"{tp}_sizes"], np.bincount(np.asarray(df["kmeans"])[m], minlength=K))
        np.testing.assert_allclose(z[f"{tp}_ratio"], ref.stats(N)["ratio"], rtol=1e-12, atol=0, equal_nan=True)
        tab = pd.read_csv(os.path.join(out, f"s_cooccurrence_{tp}.csv"), float_precision="round_trip")
        assert tuple(tab.columns) == TABLE_COLUMNS == ("domain", "neighbor", "radius", "count", "ratio") and len(tab) == K * K * 50
        np.testing.assert_array_equal((tab["domain"] * K + tab["neighbor"]) * 50 + np.tile(np.arange(50), K * K), np.arange(K * K * 50))
        np.testing.assert_array_equal(tab["radius"], np.tile(radii, K * K))
        np.testing.assert_array_equal(tab["count"], N.reshape(-1))
        np.testing.assert_array_equal(np.asarray(tab["ratio"]), z[f"{tp}_ratio"].reshape(-1))
        png = os.path.join(out, f"s_{tp}_cooccurrence.png")
        assert os.path.exists(png) == have_matplotlib() and (not os.path.exists(png) or os.path.getsize(png) > 0)


def test_a_second_run_and_the_sub_command_write_the_same_bytes(stage, tmp_path):
    from spadot_amd.cooccurrence import cooccur
    df, path, out, res = stage
    cooccur(argparse.Namespace(domains=path, output_dir=str(tmp_path), prefix="s_", device=DEV))       # the defaults
    for name in STAGE_FILES:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(tmp_path, name), "rb").read(), name
    sub = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "spadot_amd", "cooccurrence", "--domains", path, "-o", str(sub), "--prefix", "s_",
                        "--device", DEV], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in STAGE_FILES:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(sub, name), "rb").read(), name
    other = cooccur(argparse.Namespace(domains=path, output_dir=str(tmp_path / "ring"), prefix="", bins=8, radius=6.0, ring=True,
                                       device=DEV))
    r12 = other["results"]["E12"]
    np.testing.assert_array_equal(r12.radii, 6.0 * np.arange(1, 9) / 8)
    m = np.asarray(df["timepoint"]) == "E12"
    xy = np.stack([df["pixel_x"][m], df["pixel_y"][m]], axis=1)
    lab = np.asarray(df["kmeans"])[m]
    N = ref.counts(xy, lab, r12.radii ** 2, int(lab.max()) + 1)
    np.testing.assert_array_equal(r12.counts, N)
    np.testing.assert_allclose(r12.ratio, ref.stats(N, ring=True)["ratio"], rtol=1e-12, atol=0, equal_nan=True)
    assert bool(np.load(os.path.join(tmp_path / "ring", "cooccurrence.npz"))["ring"])
