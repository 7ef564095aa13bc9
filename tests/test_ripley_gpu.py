"""The ripley kernel on the MI355X against the numpy restatement of its definition (tests/ripley_ref.py, held to its own
conditions by tests/test_ripley_cpu.py): the generator's bits, the edge call, domains that straddle the 256-wide tile, the integer
lattice, nearest neighbours on their thresholds, the agreement with the cooccurrence stage, repeatability and isolation, the
refusals and the stage.

Everything the device returns is an integer (or, from ripley_points, the bits of a generated point), so every comparison of counts
is assert_array_equal.  The host statistics are fp64 arithmetic on the same integers: within 1e-12 relative, NaN in the same
places."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cooccur_cases
import nhood_cases
import ripley_cases as cases
import ripley_ref as ref
import spadot_amd.ripley  # noqa: F401  (the stage under test)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = cases.SEED


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


def _counts(problems, seed=SEED, **kw):
    """ripley_counts of a list of ripley_cases problems by squared thresholds, each drawing under its own g."""
    from spadot_amd.ripley import ripley_counts
    kw.setdefault("problem_ids", [p["g"] for p in problems])
    kw.setdefault("n_clusters", [p["K"] for p in problems])
    return ripley_counts([_dev(p["xy"]) for p in problems], [p["lab"] for p in problems], radii_sq=[p["r2"] for p in problems],
                         n_sim=[p["S"] for p in problems], n_probes=[p["M"] for p in problems], null=[p["null"] for p in problems],
                         seed=seed, **kw)


@pytest.mark.parametrize("name", sorted(cases.windows()))
def test_generated_points_have_the_bits_of_the_restatement(name):
    from spadot_amd.ripley import ripley_points
    v = cases.windows()[name]
    cum, _ = ref.fan(v)
    for stream in (0, 1 + 3 * 19 + 4):                                           # the probe set, and simulation 4 of domain 3
        for count in (1, 256, 257):
            got = ripley_points(v, seed=SEED, g=2, stream=stream, count=count, device=DEV)
            assert got.dtype == torch.float64 and tuple(got.shape) == (count, 2)
            np.testing.assert_array_equal(got.cpu().numpy(), ref.points(v, cum, SEED, 2, stream, count), err_msg=f"{stream} {count}")
    far = ripley_points(v, seed=-1, g=2147483647, stream=1 + 32 * 9999, count=300, device=DEV).cpu().numpy()
    np.testing.assert_array_equal(far, ref.points(v, cum, -1, 2147483647, 1 + 32 * 9999, 300))


def test_edge_call_matches_the_restatement():
    call = cases.edge_call()
    got = _counts(call)                                                          # B = 1, 16, 17, 64; S = 1, 19; M = 1, 257; both nulls
    assert [g.shape for g in got] == [(1, 2, 3, 1), (1, 20, 3, 16), (3, 20, 3, 17), (32, 2, 3, 64)]
    for i, g in enumerate(got):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, cases.want(f"edge{i}"), err_msg=f"problem {i}")
    assert not got[0][:, :, :2].any()                                            # n = 1: no pair, G never counts
    np.testing.assert_array_equal(got[1][0, 0, :2], np.full((2, 16), 2))         # two coincident spots: neighbours at 0
    assert not got[2][1].any() and got[2][0].any() and got[2][2].any()           # the label value without spots
    assert got[3][:, :, 2].any() and got[3][:, 1, 0].any()


@pytest.mark.parametrize("m", cases.TILE_SIZES)
def test_domains_that_straddle_the_tile_match_the_restatement(m):
    got = _counts([cases.tile_case(m, "labels"), cases.tile_case(m, "csr")])
    np.testing.assert_array_equal(got[0], cases.want(f"tile{m}_labels"))
    np.testing.assert_array_equal(got[1], cases.want(f"tile{m}_csr"))
    np.testing.assert_array_equal(got[0][:, 0], got[1][:, 0])                    # the observed pattern does not see the null


def test_the_integer_lattice_matches_the_restatement():
    got = _counts([cases.lattice("labels"), cases.lattice("csr")])
    np.testing.assert_array_equal(got[0], cases.want("lattice_labels"))
    np.testing.assert_array_equal(got[1], cases.want("lattice_csr"))
    sizes = np.bincount(cases.lattice()["lab"], minlength=3)
    assert not got[0][:, :, :2, 0].any()                                         # threshold 0: no two spots of a lattice coincide
    np.testing.assert_array_equal(got[0][:, 0, 1, 5], sizes)                     # within 5 every spot has a neighbour of its domain
    np.testing.assert_array_equal(got[0][:, 1:, 1, 5], np.broadcast_to(sizes[:, None], (3, 3)))


def test_nearest_neighbours_on_their_threshold_count():
    """The thresholds are the set's own unfused squared nearest-neighbour distances: test_ripley_cpu shows that a contracted
    distance would lose 10 of the 64 spots that lie on them."""
    p, pairs = cases.on_threshold()
    got = _counts([p])[0]
    want = cases.want("on_threshold")
    print("counts that differ from the restatement, per threshold:", np.abs(got - want).sum(axis=(0, 1, 2)).tolist())
    np.testing.assert_array_equal(got, want)


def test_the_observed_pair_counts_are_those_of_the_cooccurrence_stage():
    from spadot_amd.cooccurrence import cooccurrence_counts
    probs = [cases.tile_case(513), cases.edge_call()[3], cases.lattice()]
    got = _counts(probs, modes=("L",))
    co = cooccurrence_counts([_dev(p["xy"]) for p in probs], [p["lab"] for p in probs], radii_sq=[p["r2"] for p in probs],
                             n_clusters=[p["K"] for p in probs])
    for p, g, N in zip(probs, got, co):
        np.testing.assert_array_equal(g[:, 0, 0, :], N[np.arange(p["K"]), np.arange(p["K"]), :])


def test_a_problem_alone_in_a_batch_and_run_twice_gives_the_same_integers():
    call = cases.edge_call()
    prob = cases.tile_case(257, "csr")
    want = cases.want("tile257_csr")
    alone = _counts([prob])[0]
    np.testing.assert_array_equal(alone, want)
    batch = _counts([call[3], cases.tile_case(513), prob, call[1], cases.lattice()])   # other n, K, B, S and M around it
    np.testing.assert_array_equal(batch[2], alone)
    np.testing.assert_array_equal(batch[0], cases.want("edge3"))
    np.testing.assert_array_equal(batch[1], cases.want("tile513_labels"))
    np.testing.assert_array_equal(batch[3], cases.want("edge1"))
    np.testing.assert_array_equal(_counts([prob])[0], alone)                            # called twice
    wide = _counts([prob], n_clusters=[9])[0]                                           # a larger K: the same corner, zeros around
    assert wide.shape == (9, 3, 3, 7) and not wide[3:].any()
    np.testing.assert_array_equal(wide[:3], alone)
    more = dict(prob, r2=np.concatenate([prob["r2"], prob["r2"][-1] + 1.0 + np.arange(33.0)]))   # a larger B
    got = _counts([more])[0]
    assert got.shape == (3, 3, 3, 40)
    np.testing.assert_array_equal(got[..., :7], alone)
    out = torch.full((2, 32, 3, 3, 64), -77, dtype=torch.int64, device=DEV)            # every element of the output is written
    both = _counts([prob, call[3]], out=out)
    np.testing.assert_array_equal(both[0], alone)
    res = out.cpu().numpy()
    np.testing.assert_array_equal(res[0, :3, :, :, :7], alone)
    np.testing.assert_array_equal(res[1, :, :2], cases.want("edge3"))
    assert res.min() == 0 and res[0].sum() == alone.sum() and res[1].sum() == cases.want("edge3").sum()


@pytest.mark.parametrize("null", ["labels", "csr"])
def test_another_seed_changes_the_simulations_alone_and_the_mode_mask_skips(null):
    prob = cases.tile_case(257, null)
    want = cases.want(f"tile257_{null}")
    other = _counts([prob], seed=SEED + 1)[0]
    np.testing.assert_array_equal(other, cases.counts_of(prob, seed=SEED + 1))
    np.testing.assert_array_equal(other[:, 0, :2], want[:, 0, :2])               # pattern 0: L and G do not see the seed
    assert not np.array_equal(other[:, 1:], want[:, 1:])
    assert not np.array_equal(other[:, 0, 2], want[:, 0, 2])                     # F does: the probe set is drawn under it
    moved = _counts([prob], problem_ids=[5])[0]                                  # and another problem number draws others
    np.testing.assert_array_equal(moved, cases.counts_of(dict(prob, g=5)))
    assert not np.array_equal(moved[:, 1:], want[:, 1:])
    for modes in (("L",), ("G",), ("F",), ("L", "F"), "G,F"):
        got = _counts([prob], modes=modes)[0]
        for i, name in enumerate(ref.STATS):
            if name in modes:
                np.testing.assert_array_equal(got[:, :, i], want[:, :, i], err_msg=f"{modes} {name}")
            else:
                assert not got[:, :, i].any(), (modes, name)
    box = _counts([prob], window="box")[0]
    np.testing.assert_array_equal(box, cases.counts_of(prob, window="box"))


SENTINEL = -77


def _desc(n=37, K=3, B=17, S=19, M=1, null=0, modes=7, g=2, sizes=(20, 0, 17), V=None):
    d = np.zeros((1, 48), dtype=np.int64)
    d[0, :9] = (0, n, K, B, S, M, null, modes, g)
    d[0, 13:13 + len(sizes)] = np.cumsum(sizes)
    if V is not None:
        d[0, 9:11] = V
    return d


def test_refusals_come_before_any_launch():
    from spadot_amd import stage_ops as ops
    from spadot_amd.ripley import convex_window, ripley_counts, ripley_points
    p = cases.edge_call()[2]
    xy, lab, r2 = p["xy"], p["lab"], p["r2"]
    x = _dev(xy)
    out = torch.full((1, 3, 20, 3, 17), SENTINEL, dtype=torch.int64, device=DEV)
    kw = dict(n_sim=19, n_probes=1, n_clusters=[3], out=out)
    for n_clusters in ([33], [0]):
        with pytest.raises(ValueError, match="1 to 32"):
            ripley_counts([x], [lab], radii_sq=[r2], n_sim=19, n_probes=1, n_clusters=n_clusters, out=out)
    with pytest.raises(ValueError, match=r"labels must lie in 0 \.\. 1"):
        ripley_counts([x], [lab], radii_sq=[r2], n_sim=19, n_probes=1, n_clusters=[2], out=out)
    with pytest.raises(ValueError, match="1 to 64"):
        ripley_counts([x], [lab], radii_sq=[np.arange(65.0)], **kw)
    for bad in ([-1.0, 2.0], [1.0, np.inf], [1.0, np.nan], [1.0, 1.0], [2.0, 1.0]):
        with pytest.raises(ValueError, match="finite, >= 0 and strictly increasing"):
            ripley_counts([x], [lab], radii_sq=[bad], **kw)
    for name, value, what in (("n_sim", 10000, "1 to 9999"), ("n_sim", 0, "1 to 9999"), ("n_probes", 1048577, "1 to 1048576"),
                              ("n_probes", 0, "1 to 1048576")):
        with pytest.raises(ValueError, match=what):
            ripley_counts([x], [lab], radii_sq=[r2], **dict(kw, **{name: value}))
    with pytest.raises(ValueError, match="at most 65535 per problem"):
        ripley_counts([x], [lab], radii_sq=[r2], n_sim=9999, n_probes=1, n_clusters=[7], out=out)     # 7 x 10000 patterns
    for where, value in ((5, np.nan), (40, np.inf)):
        broken = xy.copy()
        broken.reshape(-1)[where] = value
        with pytest.raises(ValueError, match="not finite"):
            ripley_counts([_dev(broken)], [lab], radii_sq=[r2], **kw)
    square = cases.windows()["square"]
    for poly in (square[::-1], np.array([[0.0, 0], [4, 0], [1, 1], [0, 4]])):
        with pytest.raises(ValueError, match="counter-clockwise"):
            ripley_counts([x], [lab], radii_sq=[r2], window=poly, **kw)
    ang = 2 * np.pi * np.arange(300) / 300
    ring = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    with pytest.raises(ValueError, match='at most 256.*window="box"'):
        ripley_counts([_dev(ring)], [np.zeros(300, np.int64)], radii_sq=[r2], n_sim=19, n_probes=1, out=out)
    with pytest.raises(ValueError, match="at most 65535"):
        ripley_counts([x] * 65536, [lab] * 65536, radii_sq=[r2] * 65536, out=out)
    with pytest.raises(RuntimeError, match="MI355X only.*no CPU path"):
        ripley_counts([torch.as_tensor(xy)], [lab], radii_sq=[r2], **kw)
    with pytest.raises(ValueError, match="a labeling of shape"):
        ripley_counts([x], [lab[:-1]], radii_sq=[r2], **kw)
    v, cum, _ = convex_window(xy)
    win = [(v, cum)]
    for desc, k_max, s_max, b_max, what in (
            (_desc(n=2147483392, sizes=(2147483392, 0, 0)), 3, 19, 17, "spots"), (_desc(K=33), 33, 19, 17, "label values"),
            (_desc(B=65), 3, 19, 65, "thresholds"), (_desc(K=4), 3, 19, 17, "label values"), (_desc(B=18), 3, 19, 17, "thresholds"),
            (_desc(S=20), 3, 19, 17, "simulations"), (_desc(S=10000), 3, 10000, 17, "simulations"),
            (_desc(M=1048577), 3, 19, 17, "probe points"), (_desc(M=0), 3, 19, 17, "probe points"),
            (_desc(sizes=(20, 0, 16)), 3, 19, 17, "inconsistent"), (_desc(null=2), 3, 19, 17, "inconsistent"),
            (_desc(modes=8), 3, 19, 17, "inconsistent"), (_desc(modes=0), 3, 19, 17, "inconsistent"),
            (_desc(g=-1), 3, 19, 17, "inconsistent")):
        with pytest.raises(ValueError, match=what):
            ops.ripley_counts(x, desc, [r2], win, k_max, s_max, b_max, out=out)
    with pytest.raises(ValueError, match="counter-clockwise"):
        ops.ripley_counts(x, _desc(), [r2], [(v[::-1], cum)], 3, 19, 17, out=out)
    with pytest.raises(ValueError, match="ascend"):
        ops.ripley_counts(x, _desc(), [r2], [(v, cum[::-1])], 3, 19, 17, out=out)
    with pytest.raises(ValueError, match="at most 65535"):
        ops.ripley_counts(x, np.zeros((65536, 48), dtype=np.int64), [r2] * 65536, win * 65536, 3, 19, 17, out=out)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.ripley_counts(torch.as_tensor(xy), _desc(), [r2], win, 3, 19, 17)
    pts = torch.full((10, 2), float(SENTINEL), dtype=torch.float64, device=DEV)
    for call in (lambda: ops.ripley_points(v, cum, 0, 0, 1 + 32 * 9999 + 1, 10, out=pts), lambda: ops.ripley_points(v, cum, 0, -1, 0, 10, out=pts),
                 lambda: ops.ripley_points(v[::-1], cum, 0, 0, 0, 10, out=pts), lambda: ops.ripley_points(ring, np.ones(298), 0, 0, 0, 10, out=pts),
                 lambda: ops.ripley_points(v, cum, 0, 0, 0, 0, out=pts), lambda: ops.ripley_points(v, cum, 0, 0, 0, 11, out=pts)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match="MI355X only"):
        ripley_points(square, device="cpu")
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL) and torch.all(pts == SENTINEL)                 # nothing was launched

    lib = ops.model_lib()                                                            # the library's own checks, from the host copies
    pad = np.full((1, 32), -1.0)
    pad[0, :17] = r2
    V = v.shape[0]
    hull, areas = np.ascontiguousarray(v), np.concatenate([cum, [0.0, 0.0]])

    def call(desc, thresholds=pad, P=1, k_max=3, s_max=19, b_max=17, h=hull, c=areas, rows=V):
        desc = desc.copy()
        if desc[0, 10] == 0:
            desc[0, 9:11] = (0, V)
        h, c = np.ascontiguousarray(h, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
        return lib.spadot_ripley_counts(x.data_ptr(), ctypes.c_void_p(desc.ctypes.data), _dev(desc).data_ptr(),
                                        ctypes.c_void_p(thresholds.ctypes.data), _dev(thresholds).data_ptr(),
                                        ctypes.c_void_p(h.ctypes.data), _dev(h).data_ptr(), ctypes.c_void_p(c.ctypes.data),
                                        _dev(c).data_ptr(), rows, P, k_max, s_max, b_max, SEED, out.data_ptr(), None)

    for desc in (_desc(n=2147483392, sizes=(2147483392, 0, 0)), _desc(K=4), _desc(K=0), _desc(B=18), _desc(B=0), _desc(S=20),
                 _desc(S=0), _desc(M=0), _desc(M=1048577), _desc(V=(0, 257))):
        assert call(desc) == -7, desc[0, :12].tolist()
    assert call(_desc(), k_max=33) == -7 and call(_desc(), b_max=65) == -7 and call(_desc(), b_max=0) == -7
    assert call(_desc(), s_max=10000) == -7 and call(_desc(), s_max=0) == -7 and call(_desc(), P=65536) == -7
    assert call(_desc(K=7, S=9999, sizes=(20, 0, 17, 0, 0, 0, 0)), k_max=7, s_max=9999) == -7       # 70000 patterns
    for t, value in ((0, -0.5), (3, np.inf), (4, np.nan), (5, pad[0, 4]), (16, pad[0, 2])):
        broken = pad.copy()
        broken[0, t] = value
        assert call(_desc(), broken) == -7, (t, value)
    for desc in (_desc(sizes=(20, 0, 16)), _desc(null=2), _desc(modes=0), _desc(modes=8), _desc(g=-1), _desc(V=(0, 2)),
                 _desc(V=(1, V)), _desc(V=(-1, V))):
        assert call(desc) == -22, desc[0, :12].tolist()
    assert call(_desc(), h=hull[::-1]) == -22                                        # clockwise
    bent = hull.copy()
    bent[1] = hull[[0, 2]].mean(axis=0) + 0.25 * (hull[V // 2] - hull[1])            # vertex 1 pulled inside: a right turn
    assert call(_desc(), h=bent) == -22
    holed = hull.copy()
    holed[2, 0] = np.nan
    assert call(_desc(), h=holed) == -22
    assert call(_desc(), c=areas[::-1]) == -22 and call(_desc(), c=-areas) == -22
    hv, hc = ctypes.c_void_p(hull.ctypes.data), ctypes.c_void_p(areas.ctypes.data)
    dv, dc = _dev(hull), _dev(areas)

    def points(V=V, g=0, stream=0, count=10, h=hv):
        return lib.spadot_ripley_points(h, dv.data_ptr(), hc, dc.data_ptr(), V, SEED, g, stream, count, pts.data_ptr(), None)

    assert points(V=257) == -7 and points(count=0) == -7 and points(count=2147483392) == -7 and points(stream=1 + 32 * 9999 + 1) == -7
    turned = np.ascontiguousarray(hull[::-1])
    assert points(V=2) == -22 and points(g=-1) == -22 and points(h=ctypes.c_void_p(turned.ctypes.data)) == -22
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL) and torch.all(pts == SENTINEL)
    got = ripley_counts([x], [lab], radii_sq=[r2], seed=SEED, problem_ids=[2], **kw)[0]   # and a valid call writes the same tensor
    np.testing.assert_array_equal(got, cases.want("edge2"))
    np.testing.assert_array_equal(out.cpu().numpy()[0], got)


@pytest.mark.parametrize("null", ["labels", "csr"])
def test_planted_domains_read_clustered_on_the_device(null):
    """The verdicts that test_ripley_cpu asserts on the restatement: the device returns the same integers, so the same verdicts."""
    from spadot_amd.ripley import ripley
    p = cases.planted(null)
    radii = cooccur_cases.ref.default_radii(p["xy"], cases.PLANTED_BINS)
    r = ripley([_dev(p["xy"])], [p["lab"]], radii=[radii], n_sim=p["S"], n_probes=p["M"], null=null, seed=SEED, n_clusters=[p["K"]])[0]
    np.testing.assert_array_equal(r.counts, cases.want("planted_" + null))
    want = cases.stats_of(p, cases.want("planted_" + null))
    for key in ("value", "observed", "sim_mean", "sim_min", "sim_max", "p_lo", "p_hi", "p_global", "padj"):
        np.testing.assert_allclose(getattr(r, key), want[key], rtol=1e-12, atol=0, equal_nan=True, err_msg=key)
    np.testing.assert_array_equal(r.p_global[0], np.full(7, 1.0 / (cases.PLANTED_S + 1)))
    assert r.pattern.tolist() == ["clustered"] * 7 and r.null == null and r.area == ref.fan(ref.hull(p["xy"]))[1]


def test_a_domain_relabelled_at_random_reads_random_on_the_device():
    from spadot_amd.ripley import ripley
    p = cases.planted("labels", True)
    radii = cooccur_cases.ref.default_radii(p["xy"], cases.PLANTED_BINS)
    r = ripley([_dev(p["xy"])], [_dev(p["lab"])], radii=[radii], n_sim=p["S"], n_probes=p["M"], seed=SEED)[0]
    np.testing.assert_array_equal(r.counts, cases.want("scattered"))
    assert r.pattern.tolist() == ["clustered"] * 7 + ["random"] and r.padj[0, 7] > 0.05


STAGE_FILES = ["s_ripley.npz", "s_ripley_summary.csv"] + [f"s_ripley_{tp}.csv" for tp in ("E10", "E12", "E14")]


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from spadot_amd.ripley import ripley_stage
    out = tmp_path_factory.mktemp("ripley")
    df = nhood_cases.stage_table()
    path = os.path.join(out, "domains.csv")
    df.to_csv(path, index=False)
    res = ripley_stage(argparse.Namespace(domains=path, output_dir=str(out), prefix="s_", bins=50, radius=None, n_sim=99,
                                          n_probes=1000, null="labels", mode="L,G,F", window="hull", alpha=0.05, seed=0, device=DEV))
    return df, path, str(out), res


def test_the_stage_writes_its_files(stage):
    import pandas as pd
    from spadot_amd.ripley import SUMMARY_COLUMNS, TABLE_COLUMNS
    from spadot_amd.utils._analyze_utils import have_matplotlib
    df, path, out, res = stage
    tps = ["E10", "E12", "E14"]
    want = cases.stage_want()
    assert res["timepoints"] == tps and set(res["timings"]) == {"read_s", "device_s", "write_s", "total_s"}
    z = np.load(os.path.join(out, "s_ripley.npz"))
    per = ("counts", "value", "radii", "sizes", "window", "area", "p_global", "padj")
    assert set(z.files) == {"timepoints", "bins", "n_sim", "n_probes", "seed", "null", "modes"} | {f"{tp}_{n}" for tp in tps for n in per}
    assert z["timepoints"].tolist() == tps and (int(z["bins"]), int(z["n_sim"]), int(z["n_probes"]), int(z["seed"])) == (50, 99, 1000, 0)
    assert str(z["null"]) == "labels" and str(z["modes"]) == "L,G,F"
    summary = pd.read_csv(os.path.join(out, "s_ripley_summary.csv"), float_precision="round_trip")
    assert tuple(summary.columns) == SUMMARY_COLUMNS == ("timepoint", "domain", "statistic", "n", "p_global", "padj", "pattern")
    assert len(summary) == 3 * (4 + 5 + 6) and summary["n"].dtype == np.int64 and summary["p_global"].dtype == np.float64
    back = pd.read_csv(path)
    row = 0
    for tp in tps:
        N, radii, K, sizes, _, area = want[tp]
        st = ref.stats(N, sizes, area, 1000)
        np.testing.assert_array_equal(z[f"{tp}_counts"], N, err_msg=tp)
        assert z[f"{tp}_counts"].dtype == np.int64 and z[f"{tp}_counts"].shape == (K, 100, 3, 50)
        np.testing.assert_array_equal(z[f"{tp}_radii"], radii)
        np.testing.assert_array_equal(z[f"{tp}_sizes"], sizes)
        m = np.asarray(back["timepoint"]) == tp                                   # the window of the spots as the stage read them
        v = ref.hull(np.stack([back["pixel_x"][m], back["pixel_y"][m]], axis=1))
        np.testing.assert_array_equal(z[f"{tp}_window"], v)
        assert float(z[f"{tp}_area"]) == ref.fan(v)[1] and abs(ref.fan(v)[1] - area) <= 1e-12 * area
        for name in ("value", "p_global", "padj"):
            np.testing.assert_allclose(z[f"{tp}_{name}"], st[name], rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
        tab = pd.read_csv(os.path.join(out, f"s_ripley_{tp}.csv"), float_precision="round_trip")
        assert tuple(tab.columns) == TABLE_COLUMNS == ("domain", "statistic", "radius", "observed", "sim_mean", "sim_min", "sim_max",
                                                       "p_lo", "p_hi") and len(tab) == K * 3 * 50
        code = tab["statistic"].map({"L": 0, "G": 1, "F": 2})
        np.testing.assert_array_equal((tab["domain"] * 3 + code) * 50 + np.tile(np.arange(50), K * 3), np.arange(K * 3 * 50))
        np.testing.assert_array_equal(tab["radius"], np.tile(radii, K * 3))
        assert tab["domain"].dtype == np.int64 and tab["observed"].dtype == np.float64
        for name in ("observed", "sim_mean", "sim_min", "sim_max", "p_lo", "p_hi"):
            np.testing.assert_allclose(np.asarray(tab[name]).reshape(K, 3, 50), st[name].transpose(1, 0, 2), rtol=1e-12, atol=0,
                                       equal_nan=True, err_msg=name)
        part = summary.iloc[row:row + 3 * K]
        assert part["timepoint"].tolist() == [tp] * (3 * K) and part["domain"].tolist() == np.repeat(np.arange(K), 3).tolist()
        assert part["statistic"].tolist() == ["L", "G", "F"] * K and part["n"].tolist() == np.repeat(sizes, 3).tolist()
        np.testing.assert_allclose(np.asarray(part["p_global"]).reshape(K, 3), st["p_global"].T, rtol=1e-12, atol=0)
        np.testing.assert_allclose(np.asarray(part["padj"]).reshape(K, 3), st["padj"].T, rtol=1e-12, atol=0)
        assert part["pattern"].tolist() == np.repeat(st["pattern"], 3).tolist() == ["clustered"] * (3 * K)    # planted Voronoi domains
        row += 3 * K
        png = os.path.join(out, f"s_{tp}_ripley.png")
        assert os.path.exists(png) == have_matplotlib() and (not os.path.exists(png) or os.path.getsize(png) > 0)


def test_a_second_run_and_the_sub_command_write_the_same_bytes(stage, tmp_path):
    from spadot_amd.ripley import ripley_stage
    df, path, out, res = stage
    ripley_stage(argparse.Namespace(domains=path, output_dir=str(tmp_path), prefix="s_", device=DEV))       # the defaults
    for name in STAGE_FILES:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(tmp_path, name), "rb").read(), name
    sub = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "spadot_amd", "ripley", "--domains", path, "-o", str(sub), "--prefix", "s_",
                        "--device", DEV], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in STAGE_FILES:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(sub, name), "rb").read(), name
    other = ripley_stage(argparse.Namespace(domains=path, output_dir=str(tmp_path / "csr"), prefix="", bins=8, radius=6.0, n_sim=5,
                                            n_probes=50, null="csr", mode="L,F", window="box", seed=3, device=DEV))
    r12 = other["results"]["E12"]
    np.testing.assert_array_equal(r12.radii, 6.0 * np.arange(1, 9) / 8)
    m = np.asarray(df["timepoint"]) == "E12"
    xy = np.stack([df["pixel_x"][m], df["pixel_y"][m]], axis=1)
    lab = np.asarray(df["kmeans"])[m]
    N = ref.counts(xy, lab, r12.radii ** 2, int(lab.max()) + 1, 5, 50, "csr", 3, 1, window="box", modes=("L", "F"))
    np.testing.assert_array_equal(r12.counts, N)
    assert r12.modes == ("L", "F") and np.all(np.isnan(r12.value[1])) and not np.any(np.isnan(r12.value[[0, 2]]))
    g_rows = other["summary"][other["summary"]["statistic"] == "G"]                  # G was not counted: not reported as zeros
    assert len(g_rows) == 4 + 5 + 6 and g_rows["p_global"].isna().all() and g_rows["padj"].isna().all()
    assert np.asarray(other["tables"]["E12"].query("statistic == 'G'")["observed"].isna()).all()
    assert not r12.counts[:, :, 1].any() and str(np.load(os.path.join(tmp_path / "csr", "ripley.npz"))["null"]) == "csr"
