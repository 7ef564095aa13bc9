"""The kernels of csrc/sctransform.hip at their segment and tile edges, launched through the C ABI with given parameters (so
that no check depends on the host regularisation), on the crafted cases of tests/pre_cases.py, against plain fp64 numpy and
tests/sct_ref.py:

    segments / tiny   k_sct_gene_stats, k_sct_resid_stats and k_sct_resid_write on column segments of 0, 1, 5, 63, 64, 65, N-1
                      and N entries, with N = 68, 1, 129 and 5 kept spots, theta from 0.05 to 1e8
    fit               k_sct_fit on 150 and on 40 kept spots (less than a wavefront), with the stage's stop rules and with
                      maxit = 4, limit = 3, which end both loops early
    tiles             k_sct_resid_write with one, two and three spot tiles (N = 4096, 4097, 8193)

Tolerances are the stage test's (tests/test_sctransform_gpu.py): coefficients atol 1e-9, theta rtol 1e-6 below 1e3 and
log10(1 + gmean / theta) at atol 1e-9, residual statistics rtol 1e-9 / atol 1e-12, the block atol 1e-9; counts are integers,
so sum y is exact, and sum log1p(y) and the centred sum of squares are sums of at most 129 non-negative terms: rtol 1e-12.

No gene of the fit case has a restated theta of 0 (the smallest is 0.07 under limit = 3): the t0 < 0 -> 0 rule stays
unreached here, as in the stage test."""
import numpy as np
import pytest
import torch

import pre_cases as pc
import sct_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _d(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Launch:
    """One case on the device and, per time point, what sctransform() uploads for it: the kept rows, log10 umi by kept
    position and by row, the row of each kept position and the position of each row."""

    def __init__(self, case):
        from spadot_amd._lib import model_lib
        from spadot_amd.preprocess import DeviceCounts
        self.case, self.lib = case, model_lib()
        self.dc = DeviceCounts(pc.raw_counts(case), DEV)
        np.testing.assert_array_equal(self.dc.perm, case.perm)
        self.tp = {}

    def at(self, t):
        if t not in self.tp:
            c, n = self.case, self.case.B.shape[0]
            rows = pc.kept_rows(c, t)
            x = np.log10(np.asarray(c.B[rows].sum(1)).ravel())
            lur = np.zeros(n)
            lur[rows] = x
            rowmap = np.full(n, -1, dtype=np.int32)
            rowmap[rows] = np.arange(rows.size)
            self.tp[t] = dict(rows=rows, x=x, N=int(rows.size), Y=np.asarray(c.B[rows].todense()).T, lur=_d(lur), lu=_d(x),
                              krow=_d(rows, torch.int32), rowmap=_d(rowmap, torch.int32))
        return self.tp[t]

    def _head(self, t, genes):
        return (*self.dc._csc(), self.dc.tp_off.data_ptr(), t, int(genes.numel()), genes.data_ptr())

    def gene_stats(self, t, genes):
        a, g = self.at(t), _d(genes, torch.int32)
        out = torch.empty((len(genes), 3), dtype=torch.float64, device=DEV)
        assert self.lib.spadot_sct_gene_stats(*self._head(t, g), a["N"], out.data_ptr(), _stream()) == 0
        return out.cpu().numpy()

    def fit(self, t, genes, tol, maxit, limit, eps):
        a, g = self.at(t), _d(genes, torch.int32)
        out = torch.empty((len(genes), 8), dtype=torch.float64, device=DEV)
        assert self.lib.spadot_sct_fit(*self._head(t, g), a["lur"].data_ptr(), a["lu"].data_ptr(), a["N"], tol, maxit, limit,
                                       eps, out.data_ptr(), _stream()) == 0
        return out.cpu().numpy()

    def resid_stats(self, t, genes, pars, clip_hi, clip_lo):
        a, g, p = self.at(t), _d(genes, torch.int32), _d(pars)
        out = torch.empty((len(genes), 3), dtype=torch.float64, device=DEV)
        assert self.lib.spadot_sct_resid_stats(*self._head(t, g), a["lur"].data_ptr(), a["lu"].data_ptr(), a["N"], p.data_ptr(),
                                               clip_hi, clip_lo, out.data_ptr(), _stream()) == 0
        return out.cpu().numpy()

    def resid_write(self, t, genes, pars, center, clip_lo):
        a, g, p, c = self.at(t), _d(genes, torch.int32), _d(pars), _d(center)
        out = torch.full((len(genes), a["N"]), float("nan"), dtype=torch.float64, device=DEV)
        assert self.lib.spadot_sct_resid_write(*self._head(t, g), a["lur"].data_ptr(), a["lu"].data_ptr(), a["krow"].data_ptr(),
                                               a["rowmap"].data_ptr(), a["N"], p.data_ptr(), c.data_ptr(), clip_lo,
                                               out.data_ptr(), _stream()) == 0
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def seg():
    return Launch(pc.segments())


@pytest.fixture(scope="module")
def tiny():
    return Launch(pc.tiny())


@pytest.mark.parametrize("t", [0, 2])
def test_gene_stats_on_short_segments(seg, t):
    a = seg.at(t)
    assert a["N"] == pc.SEG_KEPT[t]
    Y = a["Y"]
    got = seg.gene_stats(t, np.arange(pc.SEG_G))
    np.testing.assert_allclose(got[:, 0], np.log1p(Y).sum(1), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got[:, 1], Y.sum(1))
    np.testing.assert_allclose(got[:, 2], ((Y - Y.mean(1, keepdims=True)) ** 2).sum(1), rtol=1e-12, atol=0)
    assert np.all(got[pc.SEG_ALL_ZERO] == 0)
    if t == pc.SEG_CONSTANT[1]:
        assert got[pc.SEG_CONSTANT[0], 2] == 0                     # a constant gene: the centred sum of squares is exactly 0


def _residual_checks(launch, t):
    a = launch.at(t)
    N, Y, x = a["N"], a["Y"], a["x"]
    G = Y.shape[0]
    order = np.random.default_rng(t).permutation(G)                # the gene list is not in column order
    pars, center = pc.cycled_pars(launch.case, t)
    hi, lo = float(np.sqrt(N)), float(np.sqrt(N / 30.0))
    r = ref.pearson_residuals(Y, x, pars)
    rh, rl = np.clip(r, -hi, hi), np.clip(r, -lo, lo)
    assert np.all(np.isfinite(r))
    got = launch.resid_stats(t, order, pars[order], hi, lo)
    np.testing.assert_allclose(got[:, 0], rh.mean(1)[order], rtol=1e-9, atol=1e-12)
    var = rh.var(1, ddof=1) if N > 1 else np.zeros(G)              # the kernel's rule for a single spot
    np.testing.assert_allclose(got[:, 1], var[order], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got[:, 2], rl.mean(1)[order], rtol=1e-9, atol=1e-12)
    blk = launch.resid_write(t, order, pars[order], center[order], lo)
    assert blk.shape == (G, N)
    np.testing.assert_allclose(blk, (rl - center[:, None])[order], rtol=0, atol=1e-9)


@pytest.mark.parametrize("t", [0, 1, 2])
def test_residuals_on_short_segments(seg, t):
    _residual_checks(seg, t)


def test_residuals_with_five_kept_spots(tiny):
    assert tiny.at(0)["N"] == 5 and tiny.at(0)["rows"].tolist() == [0, 2, 3, 4, 5]
    _residual_checks(tiny, 0)
    _residual_checks(tiny, 1)


# ---------------------------------------------------------------- k_sct_fit
@pytest.fixture(scope="module")
def fitcase():
    return Launch(pc.fit())


@pytest.mark.parametrize("maxit,limit", [(100, 10), (4, 3)])
@pytest.mark.parametrize("t", [0, 1])
def test_fit_matches_the_restatement(fitcase, t, maxit, limit):
    from spadot_amd.sctransform import POIS_MAXIT, POIS_TOL, THETA_EPS, THETA_LIMIT
    assert (POIS_MAXIT, THETA_LIMIT) == (100, 10)
    a = fitcase.at(t)
    assert a["N"] == pc.FIT_KEPT[t]
    Y, x = a["Y"], a["x"]
    genes = np.random.default_rng(t).permutation(pc.FIT_G)
    got = fitcase.fit(t, genes, POIS_TOL, maxit, limit, THETA_EPS)
    coef, mu, iters, before = ref.fit_poisson(Y[genes], x, tol=POIS_TOL, maxiters=maxit, full=True)
    theta, titers = ref.theta_ml(Y[genes], mu, limit=limit, eps=THETA_EPS, full=True)
    if (maxit, limit) == (4, 3):                                   # both loops end by their counters
        assert np.all(iters == 2) and np.all(titers == 2)
    np.testing.assert_array_equal(got[:, 5], iters)
    np.testing.assert_array_equal(got[:, 6], titers)
    np.testing.assert_array_equal(got[:, 7], Y[genes].sum(1))
    np.testing.assert_allclose(got[:, 1:3], coef, rtol=0, atol=1e-9)
    np.testing.assert_allclose(got[:, 3:5], before, rtol=0, atol=1e-9)
    small = theta < 1e3
    np.testing.assert_allclose(got[small, 0], theta[small], rtol=1e-6, atol=0)
    gmean = 10 ** ref.log_gmean(Y[genes])
    np.testing.assert_allclose(np.log10(1 + gmean / got[:, 0]), np.log10(1 + gmean / theta), rtol=0, atol=1e-9)


# ---------------------------------------------------------------- tiles of k_sct_resid_write
@pytest.fixture(scope="module")
def tiles():
    return Launch(pc.resid_tiles())


@pytest.mark.parametrize("t", [0, 1, 2])
def test_resid_write_across_spot_tiles(tiles, t):
    a = tiles.at(t)
    N, Y, x = a["N"], a["Y"], a["x"]
    assert N == pc.RT_KEPT[t]
    ntile, w = pc.tile_rule(N, pc.SCT_TILE)
    pars, center = pc.rt_pars(tiles.case, t)
    lo = float(np.sqrt(N / 30.0))
    want = np.clip(ref.pearson_residuals(Y, x, pars), -lo, lo) - center[:, None]
    order = np.asarray([2, 0, 3, 1])
    blk = tiles.resid_write(t, order, pars[order], center[order], lo)
    assert blk.shape == (4, N) and not np.isnan(blk).any()
    for j in range(ntile):                                         # tile by tile, so that a failure names its tile
        s = slice(j * w, min((j + 1) * w, N))
        np.testing.assert_allclose(blk[:, s], want[order][:, s], rtol=0, atol=1e-9, err_msg=f"tile {j} of {ntile}")
    # the zero and the nonzero entries differ by far more than the tolerance around every tile boundary
    zero = np.clip(ref.pearson_residuals(np.zeros_like(Y), x, pars), -lo, lo) - center[:, None]
    edge = np.flatnonzero(Y[0])
    assert np.all(np.abs(want[0, edge] - zero[0, edge]) > 1e-3)
