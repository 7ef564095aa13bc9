"""The cases of tests/pre_cases.py have the edges they are built for, the tile constants they restate are those of the two
.hip files, and the fp64 restatements that the GPU edge tests compare with are finite and in range on every case (or yield
the value documented where the kernels deviate)."""
import os
import re

import numpy as np
import pytest

import pre_cases as pc
import preprocess_ref as ref
import sct_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(path, name):
    text = open(os.path.join(ROOT, "spadot_amd", "csrc", path)).read()
    return int(re.search(r"^#define\s+%s\s+(\d+)" % name, text, re.M).group(1))


def test_tile_constants_and_rule_match_the_kernels():
    assert _define("preprocess.hip", "PRE_TILE") == pc.PRE_TILE
    assert _define("sctransform.hip", "SCT_TILE") == pc.SCT_TILE
    assert _define("preprocess.hip", "PRE_WAVE") == pc.WAVE == _define("sctransform.hip", "SCT_WAVE")
    assert [pc.tile_rule(n, pc.SCT_TILE) for n in pc.RT_KEPT] == [(1, 4096), (2, 2049), (3, 2731)]
    assert [pc.tile_rule(s, pc.PRE_TILE) for s in pc.ST_S] == [(1, 15360), (2, 7681), (3, 10241)]
    for text, rule in (("preprocess.hip", "(S + ntile - 1) / ntile"), ("sctransform.hip", "(N + ntile - 1) / ntile")):
        assert rule in open(os.path.join(ROOT, "spadot_amd", "csrc", text)).read()


def _check_layout(c):
    """What every Case promises: B is X in device order, blocks in order of first appearance, input order inside a block."""
    from spadot_amd.utils._preprocess_utils import timepoint_order
    assert c.X.dtype == np.float32 and c.X.format == "csr"
    assert timepoint_order(c.timepoint) == c.labels
    want = np.concatenate([np.flatnonzero(c.timepoint == t) for t in c.labels])
    np.testing.assert_array_equal(c.perm, want)
    assert (c.X[c.perm] != c.B).nnz == 0
    np.testing.assert_array_equal(c.spatial[c.perm], c.spatial_block)
    np.testing.assert_array_equal(np.diff(c.tp_off), c.sizes)
    assert np.all(c.B.data == np.rint(c.B.data)) and c.B.data.min() >= 1
    zero = np.flatnonzero(np.asarray(c.B.sum(1)).ravel() == 0)
    if "zero_rows" in c.facts:
        np.testing.assert_array_equal(zero, c.facts["zero_rows"])
    assert tuple(pc.kept_rows(c, t).size for t in range(len(c.sizes))) == tuple(c.facts["kept"])


def test_segments_case_has_its_edges():
    c = pc.segments()
    _check_layout(c)
    assert c.B.shape == (202, pc.SEG_G) and c.sizes == (70, 1, 131)
    assert not np.array_equal(c.perm, np.arange(202))
    assert c.B.data.min() == 1 and c.B.data.max() == 60000
    D = np.asarray(c.B.todense())
    nnz = np.stack([(D[c.tp_off[t]:c.tp_off[t + 1]] > 0).sum(0) for t in range(3)])
    for g, per in c.facts["nnz"].items():
        assert tuple(nnz[:, g]) == per, g
    for t, N in ((0, 68), (2, 129)):                       # every segment length around the wavefront, and both ends
        assert {0, 1, 5, 63, 64, 65, N - 1, N} <= set(nnz[t].tolist())
    assert set(nnz[1].tolist()) == {0, 1}
    assert nnz[0, 0] == 68 and nnz[2, 0] == 0 and nnz[0, 23] == 0 and nnz[2, 23] == 65     # both ends of colptr
    assert tuple(nnz[:, pc.SEG_MIDDLE_ONLY]) == (0, 1, 0) and nnz[:, pc.SEG_ALL_ZERO].sum() == 0
    g, t, v = pc.SEG_CONSTANT
    assert np.all(D[pc.kept_rows(c, t), g] == v)
    # the zero-total spots: first row, last row, and both rows next to the boundaries 70 | 71
    assert c.facts["zero_rows"] == (0, c.tp_off[1] - 1, c.tp_off[2], 201)
    # single nonzeros sit on the first / last kept row of their time point
    assert D[1, 2] > 0 and D[200, 2] > 0 and D[1, 3] > 0 and D[68, 3] > 0 and D[72, 3] > 0 and D[200, 3] > 0
    assert len(set(pc.SEG_COLS)) == len(pc.SEG_COLS) < pc.SEG_G and list(pc.SEG_COLS) != sorted(pc.SEG_COLS)
    assert {0, 23, pc.SEG_ALL_ZERO, pc.SEG_MIDDLE_ONLY, pc.SEG_CONSTANT[0]} <= set(pc.SEG_COLS)


def test_tiny_and_fit_cases_have_their_edges():
    c = pc.tiny()
    _check_layout(c)
    assert pc.kept_rows(c, 0).tolist() == [0, 2, 3, 4, 5]
    assert (c.B[:, 4].nnz, c.B[:7, 3].nnz) == (c.B[7:, 4].nnz, 1)
    f = pc.fit()
    _check_layout(f)
    assert f.B.shape == (192, pc.FIT_G) and f.facts["kept"] == (150, 40) and f.facts["kept"][1] < pc.WAVE
    for t in range(2):
        Y = np.asarray(f.B[pc.kept_rows(f, t)].todense())
        assert np.all(Y.sum(0) > 0)                        # log(mean y) is finite for every gene
    assert f.facts["theta"].min() == pytest.approx(0.5) and f.facts["theta"].max() == pytest.approx(50.0)


def test_resid_tiles_case_has_its_edges():
    c = pc.resid_tiles()
    _check_layout(c)
    D = np.asarray(c.B.todense())
    total_zero = 0
    for t, N in enumerate(pc.RT_KEPT):
        ntile, w = pc.tile_rule(N, pc.SCT_TILE)
        lo, hi = int(c.tp_off[t]), int(c.tp_off[t + 1])
        rows = pc.kept_rows(c, t)
        assert rows.size == N
        k_of = np.full(hi - lo, -1)
        k_of[rows - lo] = np.arange(N)
        assert np.all(rows - lo != np.arange(N))           # the kept position differs from the row everywhere
        assert k_of[0] == -1 and k_of[-1] == -1
        total_zero += hi - lo - N
        for j in range(1, ntile):                          # a zero-total row on each side of the boundary and on it
            b = rows[j * w] - lo
            assert k_of[b - 1] == -1 and k_of[b - 2] == j * w - 1 and k_of[b - 3] == -1 and k_of[b + 1] == -1
        Y = D[rows]
        tile_of = np.arange(N) // w
        edge = sorted({0, N - 1} | {j * w - 1 for j in range(1, ntile)} | {j * w for j in range(1, ntile)})
        assert np.flatnonzero(Y[:, 0]).tolist() == edge
        per_tile = [np.count_nonzero(Y[tile_of == j], axis=0) for j in range(ntile)]
        assert np.all(Y[:, 3] > 0)
        assert per_tile[-1][2] > 100 and all(p[2] == 0 for p in per_tile[:-1])
        assert per_tile[0][1] > 100
        if ntile == 3:
            assert per_tile[1][1] == 0 and per_tile[2][1] > 100
        if ntile == 2:
            assert per_tile[1][1] == 0
    assert 35 <= total_zero <= 45


@pytest.mark.parametrize("S", pc.ST_S)
def test_scale_tiles_case_has_its_edges(S):
    c = pc.scale_tiles(S)
    _check_layout(c)
    cols = c.facts["cols"]
    G = S + pc.ST_EXTRA
    ntile, w = pc.tile_rule(S, pc.PRE_TILE)
    assert c.B.shape == (6, G) and cols.size == S == np.unique(cols).size and np.any(np.diff(cols) < 0)
    assert w <= pc.PRE_TILE and (ntile - 1) * w < S <= ntile * w
    M = np.asarray(c.B[:, cols].todense())
    edges = pc.st_edges(S)
    assert edges == sorted({0, S - 1} | {j * w - 1 for j in range(1, ntile)} | {j * w for j in range(1, ntile)})
    for r in (0, 2, 4, 5):
        assert np.all(M[r, edges] > 0) and np.count_nonzero(M[r]) >= 300
    assert c.B[pc.ST_EMPTY_ROW].nnz == 0
    assert c.B[pc.ST_ZERO_TOTAL_ROW].nnz == pc.ST_EXTRA and M[pc.ST_ZERO_TOTAL_ROW].sum() == 0


# ---------------------------------------------------------------- the restatements on the cases
def test_log_scale_restatement_is_finite_and_well_conditioned():
    c = pc.segments()
    cols = np.asarray(pc.SEG_COLS)
    worst = 0.0
    for target in (1e4, 1e-4):
        for t in range(3):
            M = c.B[c.tp_off[t]:c.tp_off[t + 1]][:, cols]
            v, mu, sd = ref.log_stats(M, target)
            assert np.all(np.isfinite(v)) and np.all(np.isfinite(mu)) and np.all(sd > 0)
            moving = v.std(0, ddof=1) > 0 if v.shape[0] > 1 else np.zeros(cols.size, dtype=bool)
            assert np.all(sd[~moving] == 1)
            if moving.any():
                worst = max(worst, float((np.abs(v).max(0)[moving] / sd[moving]).max()))
            for clip in (None, 1.5):
                assert np.all(np.isfinite(ref.normalize_log_scale(M, target, clip)))
    # the bound that tests/test_preprocess_edges_gpu.py derives its std tolerance from
    assert worst <= 16.0, worst
    assert np.all(ref.log_stats(c.B[70:71][:, cols], 1e4)[2] == 1)                 # one spot: std 0 -> 1
    k = pc.SEG_COLS.index(pc.SEG_ALL_ZERO)
    v, mu, sd = ref.log_stats(c.B[71:202][:, cols], 1e4)
    assert mu[k] == 0 and sd[k] == 1
    for S in pc.ST_S:
        s = pc.scale_tiles(S)
        for t in range(2):
            assert np.all(np.isfinite(ref.normalize_log_scale(s.B[3 * t:3 * t + 3][:, s.facts["cols"]])))


def test_sparkx_restatement_is_finite_on_the_segments():
    c = pc.segments()
    for t in (0, 2):
        rows = pc.kept_rows(c, t)
        loc = c.spatial_block[rows]
        sets = [loc] + [ref.transloc_func_vec(loc, k, "gaussian") for k in range(5)] + \
            [ref.transloc_func_vec(loc, k, "cosine") for k in range(5)]
        genes = np.flatnonzero(np.asarray(c.B[rows].sum(0)).ravel() > 0)
        for s in sets:
            r = ref.sparkx_sk(c.B[rows][:, genes].tocsc(), s)
            assert all(np.all(np.isfinite(r[k])) for k in ("ehl", "sy", "syy", "klam", "stat", "ylam"))


def test_residual_restatement_is_finite_on_the_cases():
    for c, ts, pars_of in ((pc.resid_tiles(), (0, 1, 2), pc.rt_pars), (pc.segments(), (0, 1, 2), pc.cycled_pars),
                           (pc.tiny(), (0, 1), pc.cycled_pars)):
        for t in ts:
            rows = pc.kept_rows(c, t)
            x = np.log10(np.asarray(c.B[rows].sum(1)).ravel())
            pars, center = pars_of(c, t)
            assert pars.shape == (c.B.shape[1], 3) and center.shape == (c.B.shape[1],)
            assert {1e8, 0.05} <= set(pars[:, 0].tolist())
            r = sct_ref.pearson_residuals(np.asarray(c.B[rows].todense()).T, x, pars)
            assert np.all(np.isfinite(r)) and np.all(np.isfinite(pars))
            lim = np.sqrt(rows.size / 30.0)
            if rows.size > 1:
                assert np.any(np.abs(r) > lim) and np.any(np.abs(r) < lim)         # the clip is active and not everywhere


@pytest.fixture(scope="module")
def fits():
    f = pc.fit()
    out = []
    for t in range(2):
        rows = pc.kept_rows(f, t)
        x = np.log10(np.asarray(f.B[rows].sum(1)).ravel())
        Y = np.asarray(f.B[rows].todense()).T
        b, mu, iters, bl = sct_ref.fit_poisson(Y, x, full=True)
        th, tit = sct_ref.theta_ml(Y, mu, full=True)
        b4, mu4, it4, bl4 = sct_ref.fit_poisson(Y, x, maxiters=4, full=True)
        th3, tit3 = sct_ref.theta_ml(Y, mu4, limit=3, full=True)
        out.append(dict(x=x, b=b, mu=mu, iters=iters, bl=bl, th=th, tit=tit, b4=b4, it4=it4, bl4=bl4, th3=th3, tit3=tit3))
    return out


def test_fit_restatement_is_finite_and_both_early_stops_act(fits):
    for r in fits:
        for k in ("b", "mu", "bl", "th", "b4", "bl4", "th3"):
            assert np.all(np.isfinite(r[k])), k
        assert np.all(r["th"] >= 0) and np.all(r["th3"] >= 0)
        np.testing.assert_allclose(r["mu"], np.exp(r["bl"][:, :1] + r["bl"][:, 1:] * r["x"][None, :]), rtol=1e-13)
        # the defaults reach neither stop; maxit = 4 and limit = 3 cut every gene short
        assert r["iters"].max() < 98 and r["iters"].min() > 2 and r["tit"].min() >= 2
        assert np.all(r["it4"] == 2) and np.all(r["tit3"] == 2)
        assert np.any(r["tit"] < 9), "the theta loop also ends by its eps rule"
        assert np.any(r["th"] < 1e3) and np.any(r["th3"] < 1e3)


def test_pvalue_rows_reach_their_branches():
    mom, pt, names = pc.pvalue_rows()
    n = pc.PV_N
    small = lambda p: (p > 1e-300) & (p < 1e-16)
    for i, name in enumerate(names):
        sy, syy = mom[i, 0], mom[i, 1]
        lam = pc.PV_LAM[pt[i]]
        if name == "all_zero":
            assert not mom[i].any()
            continue
        ylam = 1 - n * (sy / n) ** 2 / syy
        if name == "ylam_zero":
            assert ylam == 0.0
            continue
        assert 0.99 < ylam <= 1
        q = (mom[i, 2::2] ** 2 + mom[i, 3::2] ** 2) * n / syy
        p = np.array([ref.sf_two_term(q[k], ylam * lam[k, 0], ylam * lam[k, 1]) for k in range(11)])
        assert np.all(np.isfinite(p)) and np.all((p >= 0) & (p <= 1))
        comb = ref.acat(p)
        assert 0 <= comb <= 1
        with np.errstate(over="ignore"):
            cct = np.sum(np.where(p < 1e-16, 1 / (11 * np.pi * np.maximum(p, 1e-320)), np.tan((0.5 - p) * np.pi) / 11))
        if name == "q_zero":
            assert np.all(q == 0) and np.all(p == 1) and comb == 1
        elif name == "equal_weights":
            assert np.all(lam[:, 0] == lam[:, 1]) and np.all((p > 1e-3) & (p < 1))
        elif name == "underflow":
            assert np.all(p == 0) and comb == 0
        elif name == "zero_and_one":
            assert p[0] == 0 and p[1] == 1 and comb == 0
        elif name == "one_small_cct":
            assert small(p).sum() == 1 and cct > 1e15
        elif name == "one_small_atan":
            assert small(p).sum() == 1 and cct < 1e15
        elif name == "three_small":
            assert small(p).sum() == 3 and cct > 1e15
        elif name == "all_small":
            assert small(p).sum() == 11 and cct > 1e15
        elif name == "small_among_unequal":
            assert small(p).sum() == 1 and pt[i] == 0 and cct > 1e15
        elif name == "one_only":
            assert (p == 1).sum() == 1 and not np.any(p == 0) and comb == 1
        else:
            assert np.all((p > 1e-16) & (p < 1))
