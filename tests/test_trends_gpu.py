"""The trends stage on the MI355X against tests/trends_ref.py, computed on the device's own fp32 values.

The three sums: a sum of m terms in any order is within (m - 1) 2^-53 A of exact (A: the sum of the absolute values of the
terms), v^2 and the conversions add a few ulps, and the restatement's own sum has the same bound, so
|device - restatement| <= 4 (m + 2) 2^-53 A per element, with m and A from the restatement.  mean, var, r and p are then compared
with the restatement evaluated from the restatement's sums.  Every edge of the issue, every segment length around the wave, the
workgroup and the LDS chunk, every column count at which another kernel instance is launched, time point boundaries, bitwise
reproducibility, the refusals and the stage end to end with its command line."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import trends_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
TILE = 64                      # columns per lane slot of the kernel (TR_WAVE)


def _raw(X, tp):
    from spadot_amd.utils._preprocess_utils import RawCounts
    X = sp.csr_matrix(np.asarray(X, dtype=np.float32))
    rng = np.random.default_rng(11)
    return RawCounts(X, np.asarray(tp), rng.random((X.shape[0], 2)), np.array([f"g{i}" for i in range(X.shape[1])]))


class Problem:
    """Counts on the device with their values, and the host's view of both."""

    def __init__(self, X, tp):
        from spadot_amd.preprocess import DeviceCounts
        from spadot_amd.trends import lognorm_values
        self.dc = DeviceCounts(_raw(X, tp), DEV)
        self.values = lognorm_values(self.dc)
        self.res = dict(values=self.values.cpu().numpy(), colptr=self.dc.colptr.cpu().numpy(), ridx=self.dc.ridx.cpu().numpy(),
                        tp_off=self.dc.tp_off_host.astype(np.int64), genes=self.dc.genes)
        self.V = [ref.dense_values(self.res, t) for t in range(self.dc.T)]
        self.stored = [ref.stored_mask(self.res, t) for t in range(self.dc.T)]

    def run(self, W):
        """W: numpy [n, C] in the permuted row order.  Returns S0, S1, S2 as numpy [T, G, C]."""
        import torch
        from spadot_amd.trends import weighted_moments
        S = weighted_moments(self.dc, self.values, torch.as_tensor(np.ascontiguousarray(W, dtype=np.float64), device=DEV))
        return [s.cpu().numpy() for s in S]

    def ref_sums(self, W):
        """Per time point: (S, A, m) of the restatement."""
        off = self.res["tp_off"]
        return [ref.moments(self.V[t], W[int(off[t]):int(off[t + 1])], self.stored[t]) for t in range(self.dc.T)]

    def check(self, W, S=None):
        S = self.run(W) if S is None else S
        worst = 0.0
        for t, (Sr, A, m) in enumerate(self.ref_sums(W)):
            for p in range(3):
                tol = 4.0 * (m[:, None] + 2) * EPS * A[p]
                err = np.abs(S[p][t] - Sr[p])
                assert np.all(err <= tol), (t, p, float((err - tol).max()))
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(A[p] > 0, err / (EPS * A[p]), 0.0))))
        print(f"largest |device - restatement| = {worst:.2f} x 2^-53 A")
        return S


# ---------------------------------------------------------------------------------------------------------------- edges
def _small():
    """T = 2 with 37 and 300 spots, 40 genes: an all-zero gene, a gene nonzero in every spot, a single nonzero per time point."""
    rng = np.random.default_rng(1993)
    n0, n1, G = 37, 300, 40
    n = n0 + n1
    X = rng.poisson(0.6, size=(n, G)).astype(np.float32) * (rng.random((n, G)) < 0.5)
    tp = np.repeat(np.array(["d0", "d1"]), [n0, n1])
    X[:n0, 3] = 0                      # all zero in time point 0 only
    X[:, 4] = 1 + rng.poisson(1.0, size=n)                 # nonzero in every spot
    X[:, 6] = 0
    X[9, 6] = 3                        # a single nonzero per time point
    X[n0 + 100, 6] = 1
    X[:, 8] = 0                        # all zero everywhere
    X[:, 39] = 0
    X[:, 39] = 200 - X.sum(1)          # equal row totals
    assert X.min() >= 0
    W = rng.random((n, 6))
    W[::9, :] = 0.0                    # rows of zeros ...
    W[:, 1] *= rng.random(n) < 0.3
    W[:, 2] = 0.0                      # a column of zeros: s = 0
    W[:, 3] -= W[:, 3].mean()          # a centred column: negative entries
    W[:n0, 4] = 0.0                    # no mass in time point 0 only
    W[:, 5] = 1.0                      # ... except in the column of ones
    F = rng.random((n, 4))
    F[::7] = 0.0
    return X, tp, W, F


@pytest.fixture(scope="module")
def small():
    X, tp, W, F = _small()
    return Problem(X, tp), X, tp, W, F


def test_small_shape_with_every_edge(small):
    pb, X, tp, W, F = small
    assert pb.dc.T == 2 and pb.dc.G == 40 and np.array_equal(pb.dc.perm, np.arange(337))
    assert not pb.V[0][:, 3].any() and not pb.V[0][:, 8].any() and (pb.V[1][:, 4] > 0).all()
    assert (pb.V[0][:, 6] > 0).sum() == 1 and (pb.V[1][:, 6] > 0).sum() == 1
    assert W[:, 3].min() < 0 and not W[9, :3].any() and W[9, 5] == 1
    S = pb.check(W)
    assert not S[0][0, 3].any() and not S[1][0, 8].any() and not S[2][1, 8].any()          # empty segments: exact zeros
    assert not S[0][:, :, 2].any() and not S[1][:, :, 2].any()                             # the column of zeros
    np.testing.assert_array_equal(S[0][0, 6], W[9])                                        # one entry: S0 is its row of W
    np.testing.assert_array_equal(S[1][0, 6], float(pb.V[0][9, 6]) * W[9])
    np.testing.assert_array_equal(S[0][1, 6], W[37 + 100])
    np.testing.assert_array_equal(S[0][1, 4, 5], 300.0)                                    # the ones column counts the entries


def test_gene_trends_against_the_restatement(small):
    from spadot_amd.trends import gene_trends
    pb, X, tp, W, F = small
    Wn = W[:, [0, 1, 2, 4]]
    res = gene_trends(_raw(X, tp), Wn, device=DEV)
    assert res["values"].tobytes() == pb.res["values"].tobytes()
    C = 4
    Wd = np.concatenate([Wn, np.ones((337, 1))], axis=1)
    pb.check(Wd, [res["S0"], res["S1"], res["S2"]])
    means, s_all, eps_all = [], [], []
    for t, (Sr, A, m) in enumerate(pb.ref_sums(Wd)):
        lo, hi = int(pb.res["tp_off"][t]), int(pb.res["tp_off"][t + 1])
        s = Wn[lo:hi].sum(0)
        mean, var, pct, delta, baseline = ref.trend_stats(Sr[0], Sr[1], Sr[2], s, hi - lo)
        np.testing.assert_allclose(res["colsum"][t], s, rtol=1e-13)
        eps = 4.0 * (hi - lo + 2) * EPS                    # the bound of the sums, relative: W >= 0, so A = S
        live = s > 0
        assert live.tolist() == ([True, True, False, False] if t == 0 else [True, True, False, True])
        for key in ("mean", "var", "pct", "delta"):
            assert np.all(np.isnan(res[key][t][:, ~live]))
        np.testing.assert_allclose(res["mean"][t][:, live], mean[:, live], rtol=3 * eps, atol=0)
        np.testing.assert_allclose(res["pct"][t][:, live], pct[:, live], rtol=3 * eps, atol=0)
        np.testing.assert_allclose(res["baseline"][t], baseline, rtol=3 * eps, atol=0)
        with np.errstate(invalid="ignore"):
            m2 = np.where(live[None, :], Sr[2][:, :C] / np.where(live, s, 1.0), 0.0)   # var = m2 - mean^2: both carry eps m2
        assert np.all(np.abs(res["var"][t] - var)[:, live] <= (6 * eps * m2)[:, live])
        assert np.all(np.abs(res["delta"][t] - delta)[:, live] <= (6 * eps * (mean + baseline[:, None]))[:, live])
        assert np.all(res["var"][t][:, live] >= 0)
        means.append(mean); s_all.append(s); eps_all.append(eps)
    want = ref.change(np.stack(means), np.stack(s_all))
    assert np.all(np.isnan(res["change"][:, 2])) and np.all(np.isnan(want[:, 2]))
    tol = 6 * max(eps_all) * (np.abs(means[0]) + np.abs(means[1]))                         # a difference of two means
    assert np.all(np.abs(res["change"] - want)[:, :2] <= tol[:, :2])
    np.testing.assert_array_equal(res["change"][:, 3], 0.0)                                # one live time point: last = first
    assert res["names"].tolist() == [f"trajectory_{c}" for c in range(4)]
    assert {"upload_s", "device_s", "host_s", "moments_ms", "lognorm_ms"} <= set(res["timings"])


def test_fate_drivers_against_the_restatement(small):
    from spadot_amd.trends import fate_drivers
    pb, X, tp, W, F = small
    Fz = F.copy()
    Fz[:37] = 0.0
    Fz[[3, 20]] = [[0.2, 0.8, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]]                             # time point 0: n' = 2
    for Fm in (F, Fz):
        res = fate_drivers(_raw(X, tp), Fm, device=DEV)
        for t in range(2):
            lo, hi = int(pb.res["tp_off"][t]), int(pb.res["tp_off"][t + 1])
            Wd, nv, ssf = ref.centred_fates(Fm[lo:hi])
            assert res["n_valid"][t] == nv
            np.testing.assert_allclose(res["Wc"][lo:hi], Wd, rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(res["ssf"][t], ssf, rtol=1e-13)
        pb.check(res["Wc"], [res["S0"], res["S1"], res["S2"]])
        dr = dp = 0.0
        for t, (Sr, A, m) in enumerate(pb.ref_sums(res["Wc"])):
            r, p, padj = ref.driver_stats(Sr[1], Sr[2], int(res["n_valid"][t]), res["ssf"][t])
            dr = max(dr, float(np.abs(res["r"][t] - r).max()))
            dp = max(dp, float((np.abs(res["pval"][t] - p) / p).max()))
            np.testing.assert_allclose(res["padj"][t], padj, rtol=1e-8, atol=0)
            assert np.all(res["r"][t][8] == 0) and np.all(res["pval"][t][8] == 1) and np.all(res["padj"][t][8] == 1)
        print(f"max |dr| = {dr:.3g}, max rel dp = {dp:.3g}")
        assert dr <= 1e-10 and dp <= 1e-8
    assert res["n_valid"][0] == 2 and np.all(res["r"][0] == 0) and np.all(res["pval"][0] == 1) and np.all(res["padj"][0] == 1)
    assert np.abs(res["r"][1]).max() > 0.05


# ---------------------------------------------------------------------------------------------------------------- segment lengths
def _chunk():
    from spadot_amd._lib import model_lib
    return int(model_lib().spadot_weighted_moments_chunk())


def test_segment_lengths_across_every_wave_workgroup_and_chunk_edge():
    chunk = _chunk()
    assert chunk + 1 < 1500
    lengths = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, 1500, 1600]
    rng = np.random.default_rng(64)
    n, G = 1600, len(lengths) + 1
    X = np.zeros((n, G), dtype=np.float32)
    for g, m in enumerate(lengths):
        X[rng.choice(n, m, replace=False), g] = rng.integers(1, 30, size=m)
    X[:, G - 1] = 1000 - X.sum(1)                          # dense as well; equal row totals
    assert (X[:, G - 1] >= 1).all()
    pb = Problem(X, np.zeros(n, dtype=np.int64))
    np.testing.assert_array_equal((pb.V[0] > 0).sum(0), lengths + [n])
    W = rng.normal(size=(n, 5))
    W[:, 4] = 1.0
    S = pb.check(W)
    np.testing.assert_array_equal(S[0][0, :, 4], np.asarray(lengths + [n], dtype=np.float64))


# ---------------------------------------------------------------------------------------------------------------- column counts
@pytest.fixture(scope="module")
def columns_problem():
    rng = np.random.default_rng(161)
    n0, n1, G = 70, 150, 6
    X = rng.poisson(1.0, size=(n0 + n1, G)).astype(np.float32)
    X[:, 2] = 0
    return Problem(X, np.repeat([0, 1], [n0, n1])), rng.normal(size=(n0 + n1, 1024))


# 1, the tile and its neighbours, the issue's 33 and 161, and the first column count of every kernel instance (2, 3, 4, 6, 8,
# 12 and 16 slots per lane) with the last of the one before, up to the limit
@pytest.mark.parametrize("C", [1, 33, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 161, 3 * TILE + 1, 4 * TILE, 4 * TILE + 1,
                               6 * TILE, 6 * TILE + 1, 8 * TILE + 1, 12 * TILE, 12 * TILE + 1, 1024])
def test_column_counts(columns_problem, C):
    pb, W = columns_problem
    pb.check(W[:, :C])


# ---------------------------------------------------------------------------------------------------------------- boundaries
def test_time_point_boundaries():
    rng = np.random.default_rng(5)
    sizes = [5, 64, 1]
    n, G = sum(sizes), 4
    X = np.zeros((n, G), dtype=np.float32)
    X[:, 0] = rng.integers(1, 9, size=n)                   # nonzero everywhere: the middle segment is exactly rows 5 .. 68
    X[5:69, 1] = rng.integers(1, 9, size=64)               # only the middle time point
    X[[4, 69], 2] = 7                                      # only the neighbours' rows next to the middle one
    X[[5, 68], 3] = 2                                      # the first and the last row of the middle one
    pb = Problem(X, np.repeat(["a", "b", "c"], sizes))
    W = rng.normal(size=(n, 3))
    W[:, 2] = 1.0
    S = pb.check(W)
    np.testing.assert_array_equal(S[0][:, :, 2], [[5, 0, 1, 0], [64, 64, 0, 2], [1, 0, 1, 0]])
    np.testing.assert_array_equal(S[0][2, 0], W[69])
    np.testing.assert_array_equal(S[0][0, 2], W[4])


# ---------------------------------------------------------------------------------------------------------------- bitwise
def test_bitwise_two_runs_a_column_alone_and_another_batch():
    rng = np.random.default_rng(77)
    n, G, C = 1300, 9, 161
    X = rng.poisson(rng.uniform(0.1, 3.0, size=G)[None, :], size=(n, G)).astype(np.float32)
    X[:, 0] = 1 + X[:, 0]                                  # a segment longer than the LDS chunk
    assert n > _chunk()
    pb = Problem(X, np.zeros(n, dtype=np.int64))
    W = rng.normal(size=(n, C))
    first, again = pb.run(W), pb.run(W)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for c in (0, 63, 64, 100, 160):                        # alone (one slot per lane) against its place in the full call
        alone = pb.run(W[:, c:c + 1])
        for a, b in zip(first, alone):
            assert a[:, :, c].tobytes() == b[:, :, 0].tobytes(), c
    part = pb.run(W[:, 60:70])                             # and inside another set of columns
    for a, b in zip(first, part):
        assert a[:, :, 60:70].tobytes() == b.tobytes()
    # the same problem as time point 1 of T = 3, among other genes
    m0, m2 = 40, 333
    Xb = np.zeros((m0 + n + m2, G + 2), dtype=np.float32)
    Xb[m0:m0 + n, 2:] = X
    Xb[:m0, :] = rng.poisson(1.0, size=(m0, G + 2))
    Xb[m0 + n:, :] = rng.poisson(1.0, size=(m2, G + 2))
    Xb[m0:m0 + n, 0] = 0                                   # the row totals of the middle time point as before
    Xb[m0:m0 + n, 1] = 0
    big = Problem(Xb, np.repeat(["x", "y", "z"], [m0, n, m2]))
    assert np.array_equal(big.V[1][:, 2:], pb.V[0])
    Wb = rng.normal(size=(m0 + n + m2, C))
    Wb[m0:m0 + n] = W
    batch = big.run(Wb)
    for a, b in zip(first, batch):
        assert a[0].tobytes() == b[1, 2:].tobytes()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(small, monkeypatch):
    import torch
    from spadot_amd import _lib, trends as tr
    pb = small[0]
    lib = _lib.model_lib()
    buf = torch.zeros(4096, dtype=torch.int64, device=DEV)
    p = buf.data_ptr()
    for n, C in ((100, 0), (100, 1025), (2 ** 31, 4)):     # the entry itself: -7, and `buf` stays zero
        assert lib.spadot_weighted_moments(p, p, p, p, 1, 4, p, n, C, p, p, p, None) == -7
    assert lib.spadot_weighted_moments(p, p, p, p, 65536, 65536, p, 100, 4, p, p, p, None) == -7
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0

    class Never:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")
    monkeypatch.setattr(_lib, "model_lib", lambda: Never())
    n = pb.dc.n
    W = torch.zeros((n, 1025), dtype=torch.float64, device=DEV)
    for bad in (W[:, :0], W, W[:-1, :4], W[:, :4].float(), W[0], pb.values):
        with pytest.raises(ValueError):
            tr.weighted_moments(pb.dc, pb.values, bad)
    with pytest.raises(ValueError):
        tr.weighted_moments(pb.dc, pb.values[:-1], W[:, :4])
    with pytest.raises(RuntimeError):
        tr.weighted_moments(pb.dc, pb.values, W[:, :4].cpu())
    with pytest.raises(RuntimeError):
        tr.weighted_moments(pb.dc, pb.values.cpu(), W[:, :4])
    with pytest.raises(RuntimeError):
        tr.weighted_moments(pb.dc, pb.values, np.zeros((n, 4)))
    X, tp, Wn, F = small[1:]
    with pytest.raises(ValueError, match="non-negative"):
        tr.gene_trends(_raw(X, tp), Wn, device=DEV)
    with pytest.raises(ValueError, match="one row per spot"):
        tr.fate_drivers(_raw(X, tp), F[:-1], device=DEV)
    with pytest.raises(ValueError, match="cuda device"):
        tr.fate_drivers(_raw(X, tp), F, device="cpu")
    with pytest.raises(ValueError, match="1024 columns"):
        tr.gene_trends(_raw(X, tp), np.ones((n, 1024)), device=DEV)


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def planted_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("trends")
    X, tp, F, W = ref.planted()
    n = tp.size
    tp = tp[::-1].copy()                                   # first appearance t1, sorted t0: the two orders differ
    X, F, W = X[::-1].copy(), F[::-1].copy(), W[::-1].copy()
    Xs = sp.csr_matrix(X)
    counts = str(d / "counts.npz")
    np.savez(counts, X_data=Xs.data, X_indices=Xs.indices, X_indptr=Xs.indptr, X_shape=np.asarray(Xs.shape), timepoint=tp,
             spatial=np.random.default_rng(0).random((n, 2)), genes=np.array([f"g{i}" for i in range(X.shape[1])]))
    rows = np.concatenate([np.flatnonzero(tp == t) for t in sorted(set(tp.tolist()))])     # analyze's order
    paths = {}
    for tag, order in (("", rows), ("shuffled_", np.random.default_rng(9).permutation(n))):
        paths[tag + "traj"] = str(d / (tag + "trajectories.npz"))
        paths[tag + "fates"] = str(d / (tag + "fates.npz"))
        np.savez_compressed(paths[tag + "traj"], X=W[order], rows=order, timepoint=tp[order], names=np.array(["t1_0", "t1_1", "t1_2"]))
        np.savez_compressed(paths[tag + "fates"], X=F[order], rows=order, timepoint=tp[order], names=np.array(["t1_0", "t1_1", "t1_2"]))
    return d, counts, paths


def _check_planted(r, delta, padj):
    for t in range(2):
        for k, module in ((0, list(range(0, 10))), (1, list(range(10, 20)))):
            assert sorted(np.argsort(-r[t, :, k])[:10].tolist()) == module
            assert sorted(np.argsort(-delta[t, :, k])[:10].tolist()) == module
            assert padj[t, module, k].max() < 1e-25


def test_stage_finds_the_planted_modules_and_writes_its_files(planted_files):
    import pandas as pd
    from spadot_amd.trends import trends
    d, counts, paths = planted_files
    out = str(d / "out")
    res = trends(argparse.Namespace(data=counts, trajectories=paths["traj"], fates=paths["fates"], output_dir=out, prefix="e_",
                                    top=10, device=DEV))
    assert res["timepoints"].tolist() == ["t1", "t0"]
    _check_planted(res["r"], res["delta"], res["padj"])
    assert set(os.listdir(out)) == {"e_trends.npz", "e_trends_top.csv", "e_drivers.npz", "e_drivers_t0.csv", "e_drivers_t1.csv"}
    z = np.load(os.path.join(out, "e_trends.npz"), allow_pickle=False)
    assert set(z.files) == {"mean", "var", "pct", "delta", "baseline", "change", "names", "genes", "timepoints"}
    for key in ("mean", "var", "pct", "delta"):
        assert z[key].shape == (2, 60, 3) and z[key].tobytes() == res[key].tobytes()
    assert z["baseline"].shape == (2, 60) and z["change"].shape == (60, 3) and z["genes"].shape == (60,)
    np.testing.assert_array_equal(z["change"], z["mean"][1] - z["mean"][0])
    q = np.load(os.path.join(out, "e_drivers.npz"), allow_pickle=False)
    assert set(q.files) == {"r", "pval", "padj", "n_valid", "names", "genes", "timepoints"}
    assert q["r"].shape == (2, 60, 3) and q["n_valid"].shape == (2,) and q["n_valid"].sum() == 1000 - 50
    top = pd.read_csv(os.path.join(out, "e_trends_top.csv"))
    assert list(top.columns) == ["trajectory", "gene", "change", "mean_t1", "mean_t0"] and len(top) == 3 * 10
    key = np.abs(top[top["trajectory"] == "t1_0"]["change"].to_numpy())
    assert np.all(np.diff(key) <= 0)
    drv = pd.read_csv(os.path.join(out, "e_drivers_t0.csv"))
    assert list(drv.columns) == ["gene", "fate", "r", "pval", "padj"] and len(drv) == 3 * 10
    assert sorted(drv[drv["fate"] == "t1_1"]["gene"].tolist()) == sorted(f"g{i}" for i in range(10, 20))
    assert np.all(np.diff(drv[drv["fate"] == "t1_1"]["r"].to_numpy()) <= 0)
    for key in ("trends", "drivers"):
        assert {"upload_s", "device_s", "host_s", "moments_ms"} <= set(res["timings"][key])

    again = trends(argparse.Namespace(data=counts, trajectories=paths["shuffled_traj"], fates=paths["shuffled_fates"],
                                      output_dir=str(d / "shuffled"), prefix="", top=0, device=DEV))
    for key in ("mean", "var", "pct", "delta", "baseline", "change", "r", "pval", "padj", "n_valid"):
        assert again[key].tobytes() == res[key].tobytes(), key


def test_command_line_trends(planted_files):
    d, counts, paths = planted_files
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = str(d / "cli")
    p = subprocess.run([sys.executable, "-m", "spadot_amd", "trends", "-i", counts, "--trajectories", paths["traj"], "--fates",
                        paths["fates"], "-o", out, "--top", "5"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert set(os.listdir(out)) == {"trends.npz", "trends_top.csv", "drivers.npz", "drivers_t0.csv", "drivers_t1.csv"}
    with open(os.path.join(out, "drivers_t1.csv")) as f:
        assert len(f.read().splitlines()) == 1 + 3 * 5
    z, q = np.load(os.path.join(out, "trends.npz")), np.load(os.path.join(out, "drivers.npz"))
    _check_planted(q["r"], z["delta"], q["padj"])
