"""The sepal kernel on the MI355X against the numpy restatement of its definition (tests/sepal_ref.py, held to its own conditions by
tests/test_sepal_cpu.py).  The IMAGE is exact: a step is sequential fp64 additions in CSR order, two products and two further
additions, each rounded once on both sides, so every comparison of images is np.array_equal.  The ENTROPY is bounded: its inputs
are identical on both sides, so the device and the restatement (math.fsum) differ by the rounding of the logarithms and of the two
summation orders alone, sepal_ref.entropy_bound, derived there and computed from the reference image -- no constant of it is fitted
to what the device returns.  The STOP follows from both: the device must stop where the restatement stops unless the restatement's
|dH| comes within twice that bound of the threshold."""
import argparse
import functools
import math
import os

import numpy as np
import pytest
import torch

import autocorr_cases as ac
import sepal_cases as cases
import sepal_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


class Counts:
    """The CSC of autocorr_cases.csc on the device, with what moran.columns reads of a DeviceCounts."""

    def __init__(self, Vs):
        colptr, ridx, vals, off = ac.csc(Vs)
        self.colptr, self.ridx, self.values = _dev(colptr), _dev(ridx), _dev(vals)
        self.tp_off_host, self.T, self.G, self.n, self.device = off, len(Vs), Vs[0].shape[1], int(off[-1]), torch.device(DEV)


def _edges(problems):
    return [(_dev(s, torch.int32), _dev(d, torch.int32)) for s, d, _ in problems]


def _diffuse(problems, dt, steps=cases.STEPS, genes=None, **kw):
    from spadot_amd.sepal import diffuse
    dc = Counts([V for _, _, V in problems])
    return diffuse(_edges(problems), dc, genes, steps=steps, dt=dt, values=dc.values, **kw)


def _sepal(problems, dt, genes=None, **kw):
    from spadot_amd.sepal import sepal
    dc = Counts([V for _, _, V in problems])
    return sepal(_edges(problems), dc, genes, dt=dt, values=dc.values, **kw)


@functools.lru_cache(maxsize=None)
def _got(name):
    return _diffuse(*cases.CASES[name]())


def test_the_case_file_holds_the_library_defaults():
    from spadot_amd import stage_ops as ops
    assert cases.W == ops.SEPAL_THREADS and 2 * cases.W + 1 <= 2100
    assert max(cases.RAGGED) * 8 + ops.SEPAL_LDS_FIXED <= ops.SEPAL_LDS_BYTES        # every case fits in LDS by default


# ------------------------------------------------------------------------------------------------------- 1: the image is exact
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_image_is_exact(name):
    images, _ = _got(name)
    want = cases.want_diffuse(name)
    assert len(images) == len(want)
    for t, (img, (w, _)) in enumerate(zip(images, want)):
        assert img.dtype == np.float64 and img.shape == w.shape
        assert np.array_equal(img, w), f"{name}, time point {t}: {int((img != w).sum())} of {w.size} values differ"
    if name == "loose":
        V = cases.loose()[0][0][2]
        assert np.all(images[0][7] == V[7].astype(np.float64))                       # the spot without a row keeps its value


# ------------------------------------------------------------------------------------------------ 2: the entropy is bounded
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_entropy_is_within_its_derived_bound(name):
    _, traces = _got(name)
    worst = 0.0
    for t, (H, (w, parts)) in enumerate(zip(traces, cases.want_diffuse(name))):
        n = w.shape[0]
        assert H.shape == (len(cases.GENES), cases.STEPS + 1)
        for g in range(H.shape[0]):
            want = np.array([p[0] for p in parts[g]])
            bound = np.array([ref.entropy_bound(n, p[1], p[2]) for p in parts[g]])
            assert np.array_equal(np.isnan(H[g]), np.isnan(want)), (name, t, cases.GENES[g])
            ok = ~np.isnan(want)
            err = np.abs(H[g][ok] - want[ok])
            worst = max(worst, float((err / bound[ok]).max()) if ok.any() else 0.0)
            assert np.all(err <= bound[ok]), (name, t, cases.GENES[g], float(err.max()), float(bound[ok].min()))
    print(f"{name}: largest |H_dev - H_ref| / bound = {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------- 3: the stop
def _check_stop(results, runs_per_tp, dt, thresh, trace0=None):
    total = second = 0
    for t, (r, runs) in enumerate(zip(results, runs_per_tp)):
        assert r.iterations.dtype == np.int64 and r.converged.dtype == bool and r.score.dtype == np.float64
        for g, w in enumerate(runs):
            if w.degenerate:
                assert r.degenerate[g] and math.isnan(r.score[g]) and r.iterations[g] == 0 and not r.converged[g]
                assert math.isnan(r.H0[g]) and math.isnan(r.H[g])
                continue
            total += 1
            H = np.array([p[0] for p in w.parts])
            b = np.array([ref.entropy_bound(r.n, p[1], p[2]) for p in w.parts])
            # both H of a difference are within the bound of test 2: the device's |dH| is within twice it of the restatement's
            close = np.abs(np.abs(H[1:] - H[:-1]) - thresh) <= 2.0 * np.maximum(b[1:], b[:-1])
            if not close.any():
                assert r.iterations[g] == w.iterations and bool(r.converged[g]) == w.converged, (t, g)
            else:                                            # the steps at which rounding may decide, and the restatement's own
                second += 1
                assert r.iterations[g] in set((1 + np.flatnonzero(close)).tolist()) | {w.iterations}, (t, g)
            assert not r.degenerate[g] and r.score[g] == float(dt) * int(r.iterations[g])
            assert abs(r.H0[g] - H[0]) <= b[0]
            if r.iterations[g] == w.iterations:
                assert abs(r.H[g] - H[-1]) <= b[-1] and np.array_equal(r.image[:, g], w.image)
    print(f"{total} genes, {second} under the second clause")
    assert 10 * second <= total                              # on the CPU prototype none: beyond the cap the kernel is wrong


def test_the_stop_on_the_ragged_call():
    problems, dt = cases.ragged()
    res = _sepal(problems, dt)
    _check_stop(res, cases.want_ragged_runs(), dt, cases.THRESH)
    H0 = _got("ragged")[1]
    for t, r in enumerate(res):                              # H0 is the first entry of diffuse's trace, bit for bit
        assert np.array_equal(r.H0, H0[t][:, 0], equal_nan=True)
        assert r.converged[cases.GENES.index("constant")] and r.iterations[cases.GENES.index("constant")] == 1


@functools.lru_cache(maxsize=None)
def _planted():
    """The planted data set on the device as the stage sees it: (DeviceCounts, values, edges, V fp32 [400, 200] on the host in
    the rows of the DeviceCounts, src, dst on the host)."""
    from spadot_amd.neighbors import spatial_edges
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.trends import lognorm_values
    dc = DeviceCounts(cases.planted_raw(), DEV)
    values = lognorm_values(dc)
    edges = spatial_edges(dc.spatial, 6, DEV)
    colptr, ridx, v = dc.colptr.cpu().numpy(), dc.ridx.cpu().numpy(), values.cpu().numpy()
    V = np.zeros((dc.n, dc.G), dtype=np.float32)
    for g in range(dc.G):
        V[ridx[colptr[g]:colptr[g + 1]], g] = v[colptr[g]:colptr[g + 1]]
    return dc, values, edges, V, edges[0].cpu().numpy(), edges[1].cpu().numpy()


def test_the_stop_on_the_planted_data_set():
    from spadot_amd.sepal import sepal
    dc, values, edges, V, src, dst = _planted()
    sel = np.asarray(cases.PLANTED_GENES)
    assert sel.size == 40
    res = sepal([edges], dc, sel, values=values)
    runs = cases.want_runs([(src, dst, V[:, sel])], cases.DT)
    _check_stop(res, runs, cases.DT, cases.THRESH)
    assert res[0].converged.all() and res[0].iterations.min() > 50


# ------------------------------------------------------------------------------------------------------ 4: a cap that bites
def test_a_cap_that_bites():
    problems, dt = cases.ragged()
    sel = [cases.GENES.index(g) for g in ("single", "dense", "sparse")]
    res = _sepal(problems, dt, genes=sel, n_iter=7)
    images, _ = _diffuse(problems, dt, steps=7, genes=sel)
    for t, r in enumerate(res):
        assert r.iterations.tolist() == [7, 7, 7] and not r.converged.any() and not r.degenerate.any()
        assert np.all(r.score == 0.1 * 7) and abs(r.score[0] - 0.7) < 1e-15
        assert np.array_equal(r.image, images[t])


# ---------------------------------------------------------------------------------------------------------- 5: repeatability
def _same(a, b, what):
    for name in ("score", "iterations", "H", "H0", "image", "converged", "degenerate"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), f"{what}: {name}"


@pytest.fixture(scope="module")
def ragged_runs():
    problems, dt = cases.ragged()
    return problems, dt, _sepal(problems, dt)


def test_a_gene_alone_among_others_and_in_reverse(ragged_runs):
    problems, dt, base = ragged_runs
    rev = _sepal(problems, dt, genes=np.arange(len(cases.GENES))[::-1])
    alone = _sepal(problems, dt, genes=[3])
    for t, r in enumerate(base):
        for name in ("score", "iterations", "H", "H0", "converged", "degenerate"):
            assert np.array_equal(getattr(rev[t], name), getattr(r, name)[::-1], equal_nan=True), name
            assert np.array_equal(getattr(alone[t], name), getattr(r, name)[3:4], equal_nan=True), name
        assert np.array_equal(rev[t].image, r.image[:, ::-1]) and np.array_equal(alone[t].image, r.image[:, 3:4])


def test_a_time_point_alone_and_the_same_call_twice(ragged_runs):
    problems, dt, base = ragged_runs
    again = _sepal(problems, dt)
    for t, r in enumerate(base):
        _same(again[t], r, "the same call twice")
        _same(_sepal(problems[t:t + 1], dt)[0], r, f"time point {t} alone")


@pytest.mark.parametrize("kw", [dict(steps_per_launch=1), dict(steps_per_launch=13), dict(lds_limit=0),
                                dict(lds_limit=512 + 8 * 257)], ids=["1_step", "13_steps", "global", "mixed"])
def test_the_split_over_launches_and_the_path_change_no_bit(ragged_runs, kw):
    problems, dt, base = ragged_runs
    if kw.get("steps_per_launch") == 1:                      # a launch per step: keep the number of launches small
        problems, base = problems[:1], base[:1]
        sel = [cases.GENES.index("constant"), cases.GENES.index("sparse"), cases.GENES.index("empty")]
        got = _sepal(problems, dt, genes=sel, n_iter=60, **kw)
        want = _sepal(problems, dt, genes=sel, n_iter=60)
        assert want[0].iterations.tolist() == [1, 60, 0]
    else:
        got, want = _sepal(problems, dt, **kw), base
    for t, r in enumerate(want):
        _same(got[t], r, str(kw))


def test_diffuse_on_the_global_path_and_in_pieces():
    problems, dt = cases.ragged()
    images, traces = _got("ragged")
    for kw in (dict(lds_limit=0), dict(steps_per_launch=7), dict(lds_limit=0, steps_per_launch=7)):     # 7: odd, the slabs swap
        got_i, got_t = _diffuse(problems, dt, **kw)
        for t in range(len(problems)):
            assert np.array_equal(got_i[t], images[t]) and np.array_equal(got_t[t], traces[t], equal_nan=True), (kw, t)


# ------------------------------------------------------------------------------------- 6: the outputs are written completely
def test_no_sentinel_survives_in_a_non_degenerate_item():
    from spadot_amd import stage_ops as ops
    from spadot_amd.sepal import diffusion_graph
    problems = cases.ragged()[0] + cases.size_case(1)[0]
    sizes = [V.shape[0] for _, _, V in problems]
    for lds_limit in (None, 0):
        graph = diffusion_graph(_edges(problems), sizes, torch.device(DEV))
        ng = len(cases.GENES)
        state = ops.sepal_state(graph.desc, ng, DEV, lds_limit)
        for v in state.values():
            v.fill_(SENTINEL if v.dtype == torch.float64 else -7)
        res = _sepal(problems, cases.DT, state=state, lds_limit=lds_limit)
        image, it, done = state["image"].cpu().numpy(), state["iterations"].cpu().numpy(), state["done"].cpu().numpy()
        Hp, H0 = state["H_prev"].cpu().numpy(), state["H0"].cpu().numpy()
        assert not (it == -7).any() and not (done == -7).any() and not (Hp == SENTINEL).any() and not (H0 == SENTINEL).any()
        for t, n in enumerate(sizes):
            rows = image[t * ng:(t + 1) * ng, :n]
            assert not (rows == SENTINEL).any() and np.all(rows >= 0.0)
            r = res[t]
            bad = np.array([g == 0 or n < 2 for g in range(ng)])                     # the empty gene, and the lone spot
            assert np.array_equal(r.degenerate, bad)
            assert np.isnan(r.score[bad]).all() and not r.iterations[bad].any() and not r.converged[bad].any()
            assert np.array_equal(done[t * ng:(t + 1) * ng] == 2, bad)
            assert not np.isnan(r.score[~bad]).any() and np.all(r.iterations[~bad] >= 1)


# ----------------------------------------------------------------------------------------------------------------- 7: the stage
def _planted_counts(path):
    raw = cases.planted_raw()
    np.savez(path, X=np.asarray(raw.X), timepoint=np.asarray(raw.obs["timepoint"]).astype(str),
             spatial=np.asarray(raw.obsm["spatial"]), genes=np.asarray(raw.var_names).astype(str))
    return path


def test_the_stage_writes_its_files(tmp_path):
    import pandas as pd
    from spadot_amd.sepal import FIELDS, TABLE_COLUMNS, sepal, sepal_stage
    path = _planted_counts(str(tmp_path / "counts.npz"))

    def ns(out):
        return argparse.Namespace(data=path, output_dir=str(tmp_path / out), prefix="p_", genes=None, k=6, dt=0.1, thresh=1e-8,
                                  n_iter=30000, device=DEV)

    out = sepal_stage(ns("a"))
    sepal_stage(ns("b"))
    tp = out["timepoints"][0]
    for name in (f"p_sepal_{tp}.csv", "p_sepal.npz"):
        assert os.path.exists(tmp_path / "a" / name)
    assert set(out["timings"]) == {"read_s", "graph_s", "device_s", "write_s", "total_s"}
    tab = pd.read_csv(tmp_path / "a" / f"p_sepal_{tp}.csv")
    assert tuple(tab.columns) == TABLE_COLUMNS and len(tab) == 200
    score = tab["score"].to_numpy()
    nan = np.isnan(score)
    assert nan.sum() == 1 and nan[-1] and np.all(np.diff(score[~nan]) <= 0)          # descending, NaN last
    assert tab["rank"].tolist() == list(range(1, 200)) + [0]
    dc, values, edges, _, _, _ = _planted()
    res = sepal([edges], dc, values=values)[0]
    z = np.load(tmp_path / "a" / "p_sepal.npz")
    for name in FIELDS:
        assert np.array_equal(z[f"{tp}_{name}"], getattr(res, name), equal_nan=True), name
    assert z["genes"].tolist() == np.asarray(dc.genes).astype(str).tolist() and z["timepoints"].tolist() == [tp]
    assert (int(z["k"]), float(z["dt"]), float(z["thresh"]), int(z["n_iter"])) == (6, 0.1, 1e-8, 30000)
    assert tab["gene"].tolist() == np.asarray(dc.genes).astype(str)[ref.order(res.score)].tolist()
    with open(tmp_path / "a" / "p_sepal.npz", "rb") as f, open(tmp_path / "b" / "p_sepal.npz", "rb") as g:
        assert f.read() == g.read()


# --------------------------------------------------------------------------------------- 8: refusals come before any launch
def test_refusals_come_before_any_launch(tmp_path):
    from spadot_amd import stage_ops as ops
    from spadot_amd.sepal import diffusion_graph, sepal, sepal_stage
    (src, dst, V), = cases.size_case(65)[0]
    graph = diffusion_graph(_edges([(src, dst, V)]), [65], torch.device(DEV))
    state = ops.sepal_state(graph.desc, V.shape[1], DEV)
    for v in state.values():
        v.fill_(SENTINEL if v.dtype == torch.float64 else -7)

    def untouched():
        return all(bool((v == (SENTINEL if v.dtype == torch.float64 else -7)).all()) for v in state.values())

    far = dst.copy()
    far[5] = 65
    neg, inf = V.copy(), V.copy()
    neg[3, 3], inf[3, 3] = -1.0, np.inf
    for what, problem, kw in (("edge ends", (src, far, V), {}), ("negative", (src, dst, neg), {}), ("finite", (src, dst, inf), {}),
                              ("dt", (src, dst, V), dict(dt=0.0)), ("dt", (src, dst, V), dict(dt=-0.1)),
                              ("thresh", (src, dst, V), dict(thresh=-1e-9)), ("n_iter|steps", (src, dst, V), dict(n_iter=0))):
        kw = dict(dict(dt=cases.DT), **kw)
        with pytest.raises(ValueError, match=what):
            _sepal([problem], kw.pop("dt"), state=state, **kw)
        assert untouched(), what
    (hs, hd, hV), = cases.hub()[0]
    hub_graph = diffusion_graph(_edges([(hs, hd, hV)]), [300], torch.device(DEV))
    top = hub_graph.max_dt()
    assert top == ref.max_dt(300, len(hs), 120) and hub_graph.max_degree.tolist() == [120]
    hub_state = ops.sepal_state(hub_graph.desc, hV.shape[1], DEV)
    hub_state["image"].fill_(SENTINEL)
    with pytest.raises(ValueError, match="largest admissible dt is " + repr(top).replace(".", r"\.")):
        _sepal([(hs, hd, hV)], float(np.nextafter(top, np.inf)), state=hub_state)
    assert bool((hub_state["image"] == SENTINEL).all()) and not hub_state["iterations"].any()
    assert _sepal([(hs, hd, hV)], top, n_iter=3)[0].iterations.max() == 3           # and just below the limit it runs
    dc = Counts([V])
    with pytest.raises(RuntimeError, match="MI355X only"):
        sepal([(torch.as_tensor(src), torch.as_tensor(dst))], dc, values=dc.values, state=state)
    with pytest.raises(RuntimeError, match="MI355X only"):
        sepal(_edges([(src, dst, V)]), [torch.as_tensor(V)], state=state)
    assert untouched()
    path = _planted_counts(str(tmp_path / "counts.npz"))
    args = argparse.Namespace(data=path, output_dir=str(tmp_path / "out"), prefix="", genes="g0000,nope", k=6, dt=0.1, thresh=1e-8,
                              n_iter=10, device=DEV)
    with pytest.raises(ValueError, match="does not hold: nope"):
        sepal_stage(args)
    assert not os.path.exists(tmp_path / "out")
