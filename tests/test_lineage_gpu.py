"""Lineages on the MI355X: the plan-apply kernels (spadot_ot_plan_apply_dev / OTSolver.apply) against a host product in
longdouble that does not go through the plan kernel, their refusals, determinism, chunking and an exact integer regime;
lineage.TransportChain against tests/lineage_ref.py on the dense plans; analyze(lineage=True) end to end and the command line.

Bound of the kernel tests: every output is a sum of n products (n = J pulling back, n = I pushing forward), each product with
at most five roundings, so |Q - Q_ref| <= (n + 16) * 2^-53 * (|Pi| |P|) element-wise, for every element."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lineage_ref as ref
from lineage_ref import EPS, LD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 5), (7, 13), (257, 64), (300, 400), (1000, 1031), (2300, 1900)]
NRHS = [1, 2, 10, 33, 64]


def _solved(I, J, storage, seed=0):
    from spadot_amd.analyze_ot import ANALYZE_OT_CONFIG
    from spadot_amd.ot import OTSolver
    rng = np.random.default_rng(1000 * seed + 7 * I + J)
    x, y = rng.normal(size=(I, 20)), rng.normal(size=(J, 20))
    s = OTSolver(I, J, storage=storage, device=DEV)
    s.set_cost_from_latents(x, y)
    s.solve(dict(ANALYZE_OT_CONFIG))
    return s


def _host_plan(s):
    """Pi = diag(a) K diag(b) / J in the wide type, from the solver's own K, a, b (not through the plan kernel)."""
    K, a, b = s.matrix("K"), s.vector("a"), s.vector("b")
    wide = LD if ref.WIDE else np.float64
    return a.astype(wide)[:, None] * K.astype(wide) * b.astype(wide)[None, :] / wide(s.J)


def _host_products(Pi, P, transpose):
    """(Pi P or Pi^T P, |Pi| |P|) in the wide type."""
    A = Pi.T if transpose else Pi
    want = ref.matmul(A, P)
    return want, (want if (P >= 0).all() else ref.matmul(A, np.abs(P)))        # (Pi >= 0)


def _check(Q, want, mag, n, what):
    """Q (device result) against the host product within the bound, every element; returns the worst error as a share of
    the bound."""
    bound = (n + 16) * EPS * mag
    err = np.abs(Q.cpu().numpy().astype(want.dtype) - want)
    assert np.isfinite(np.asarray(err, dtype=np.float64)).all(), what
    bad = err > bound
    share = float(np.max(np.where(mag > 0, err / np.where(mag > 0, bound, 1), 0))) if err.size else 0.0
    assert not bad.any(), (what, int(bad.sum()), share)
    return share


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_against_the_host_product(shape, storage):
    I, J = shape
    s = _solved(I, J, storage)
    try:
        Pi = _host_plan(s)
        assert float(np.asarray(Pi, dtype=np.float64).sum()) > 0
        rng = np.random.default_rng(I * 31 + J)
        worst = 0.0
        for transpose in (False, True):
            n_in = I if transpose else J
            for shift in (0.0, 0.5):                                  # [0, 1) and [-0.5, 0.5)
                P64 = rng.uniform(size=(n_in, 64)) - shift
                want, mag = _host_products(Pi, P64, transpose)        # column by column: the leading nrhs columns serve nrhs
                for nrhs in NRHS:
                    P = np.ascontiguousarray(P64[:, :nrhs])
                    Q = s.apply(torch.as_tensor(P, device=DEV), transpose=transpose)
                    assert Q.dtype == torch.float64 and tuple(Q.shape) == ((J if transpose else I), nrhs)
                    share = _check(Q, want[:, :nrhs], mag[:, :nrhs], n_in, (shape, storage, transpose, shift, nrhs))
                    worst = max(worst, share)
                    Q2 = s.apply(torch.as_tensor(P, device=DEV), transpose=transpose)
                    assert torch.equal(Q, Q2), ("two calls, different bits", shape, storage, transpose, nrhs)
        print(f"apply {I}x{J} {storage}: worst error {worst:.3f} of the bound")
        v = rng.uniform(size=J)
        q1 = s.apply(v)                                               # 1-D in, 1-D out
        assert q1.dim() == 1 and torch.equal(q1, s.apply(v[:, None])[:, 0])
    finally:
        s.close()


def test_a_column_does_not_depend_on_its_company_and_chunks_concatenate():
    s = _solved(300, 400, "f32", seed=1)
    try:
        rng = np.random.default_rng(5)
        for transpose, n_in in ((False, 400), (True, 300)):
            for ncol in (65, 100, 128, 130):
                P = torch.as_tensor(rng.uniform(size=(n_in, ncol)) - 0.5, device=DEV)
                Q = s.apply(P, transpose=transpose)
                assert tuple(Q.shape) == (400 if transpose else 300, ncol)
                parts = [s.apply(P[:, c:c + 64].contiguous(), transpose=transpose) for c in range(0, ncol, 64)]
                assert torch.equal(Q, torch.cat(parts, dim=1)), (transpose, ncol)
            P = torch.as_tensor(rng.uniform(size=(n_in, 33)), device=DEV)
            Q = s.apply(P, transpose=transpose)
            for c in (0, 17, 32):                                     # alone (one column, no padding) or in company: same bits
                assert torch.equal(Q[:, c], s.apply(P[:, c].contiguous(), transpose=transpose)), (transpose, c)
    finally:
        s.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_apply_of_one_hot_columns_is_the_group_sums_kernel(storage):
    I, J, G = 300, 400, 7
    s = _solved(I, J, storage, seed=2)
    try:
        rng = np.random.default_rng(9)
        lab = np.concatenate([np.arange(G), rng.integers(0, G, J - G)])
        onehot = np.zeros((J, G))
        onehot[np.arange(J), lab] = 1.0
        cl = torch.as_tensor(lab, dtype=torch.int32, device=DEV)
        Qg = torch.empty((I, G), dtype=torch.float64, device=DEV)
        rc = s.lib.spadot_ot_plan_group_sums_dev(s.h, ctypes.c_void_p(cl.data_ptr()), G, ctypes.c_void_p(Qg.data_ptr()))
        assert rc == 0
        Qa = s.apply(torch.as_tensor(onehot, device=DEV))
        torch.cuda.synchronize()
        want, mag = _host_products(_host_plan(s), onehot, False)
        bound = (J + 16) * EPS * np.asarray(mag, dtype=np.float64)
        assert np.all(np.abs(Qa.cpu().numpy() - Qg.cpu().numpy()) <= bound)
        _check(Qa, want, mag, J, "one-hot")
    finally:
        s.close()


def test_apply_refuses_bad_arguments_and_launches_nothing():
    s = _solved(7, 13, "f64", seed=3)
    try:
        P = torch.ones((13, 64), dtype=torch.float64, device=DEV)
        Q = torch.full((13, 64), float("nan"), dtype=torch.float64, device=DEV)
        pp, qp = ctypes.c_void_p(P.data_ptr()), ctypes.c_void_p(Q.data_ptr())
        call = s.lib.spadot_ot_plan_apply_dev
        for args in ((s.h, 0, pp, 0, qp), (s.h, 0, pp, 65, qp), (s.h, 1, pp, -1, qp), (s.h, 2, pp, 3, qp), (s.h, -1, pp, 3, qp),
                     (None, 0, pp, 3, qp), (s.h, 0, None, 3, qp), (s.h, 0, pp, 3, None)):
            assert call(*args) == -22, args[1:]
        torch.cuda.synchronize()
        assert bool(torch.isnan(Q).all())
        with pytest.raises(ValueError):
            s.apply(torch.ones((12, 3), device=DEV))                  # 12 rows for J = 13
        assert call(s.h, 0, pp, 3, qp) == 0                           # and the same call with good arguments runs
        torch.cuda.synchronize()
        assert bool(torch.isfinite(Q.view(-1)[:7 * 3]).all()) and bool(torch.isnan(Q.view(-1)[7 * 3:]).all())
    finally:
        s.close()


class _DeviceView:
    """A raw device pointer as something torch.as_tensor understands."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(70, 32), (5, 16), (130, 128), (200, 512), (1031, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_is_exact_where_the_arithmetic_is(shape, storage):
    """K small integers, a and b powers of two, J a power of two, P integers: every product and every partial sum is an exact
    fp64 number, so the result must equal the host's bit for bit whatever the order of summation.  The pad columns of K
    (ld > J) hold a large value that must not be read into any result."""
    from spadot_amd.ot import OTSolver
    I, J = shape
    s = OTSolver(I, J, storage=storage, device=DEV)
    try:
        ld = s.ld
        rng = np.random.default_rng(I + 3 * J)
        K = rng.integers(0, 8, size=(I, ld)).astype(np.float64)
        K[:, J:] = 1000.0
        a = 2.0 ** rng.integers(-3, 4, size=I)
        b = 2.0 ** rng.integers(-3, 4, size=J)
        kt = torch.as_tensor(_DeviceView(s.lib.spadot_ot_matrix_dev(s.h, 1), (I, ld), "<f8" if storage == "f64" else "<f4"),
                             device=DEV)
        at = torch.as_tensor(_DeviceView(s.lib.spadot_ot_vector_dev(s.h, 0), (I,), "<f8"), device=DEV)
        bt = torch.as_tensor(_DeviceView(s.lib.spadot_ot_vector_dev(s.h, 1), (J,), "<f8"), device=DEV)
        kt.copy_(torch.as_tensor(K, device=DEV).to(kt.dtype))
        at.copy_(torch.as_tensor(a, device=DEV))
        bt.copy_(torch.as_tensor(b, device=DEV))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(s.matrix("K"), K[:, :J])        # the views wrote what the solver reads
        np.testing.assert_array_equal(s.vector("a"), a)
        Pi = a[:, None] * K[:, :J] * b[None, :] / J                    # exact
        for transpose in (False, True):
            for nrhs in (1, 3, 16, 33, 64):
                P = rng.integers(-8, 9, size=(I if transpose else J, nrhs)).astype(np.float64)
                want = (Pi.T if transpose else Pi) @ P                 # exact in any order
                got = s.apply(torch.as_tensor(P, device=DEV), transpose=transpose).cpu().numpy()
                np.testing.assert_array_equal(got, want, err_msg=str((shape, storage, transpose, nrhs)))
    finally:
        s.close()


# ---- the chain against the host statement of the definitions ----
def _mixture_latents(rng, sizes, k=5):
    cen = rng.normal(size=(k, 20))
    return [cen[rng.integers(0, k, n)] + 0.3 * rng.normal(size=(n, 20)) for n in sizes]


def _labels(rng, sizes, ks):
    return [rng.permutation(np.concatenate([np.arange(k), rng.integers(0, k, n - k)])) for n, k in zip(sizes, ks)]


def _assert_rel(got, want, rtol, what):
    got = np.asarray(got, dtype=np.float64)
    want_w = np.asarray(want)
    assert got.shape == want_w.shape, what
    err = np.abs(got.astype(want_w.dtype) - want_w)
    lim = rtol * np.abs(want_w)
    worst = float(np.max(np.where(want_w != 0, err / np.where(want_w != 0, lim, 1), np.where(err == 0, 0, np.inf)))) if err.size else 0
    assert np.all(err <= lim), (what, worst)
    return worst


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("sizes,ks,seed", [((150, 130, 170), (4, 5, 3), 3), ((500, 650, 400, 700), (6, 4, 7, 5), 8)],
                         ids=["three", "four"])
def test_chain_against_the_reference(sizes, ks, seed, storage):
    from spadot_amd import analyze_ot, lineage
    rng = np.random.default_rng(seed)
    lat = _mixture_latents(rng, sizes)
    lab = _labels(rng, sizes, ks)
    T, n_max = len(sizes), max(sizes)
    rt = lambda L: 4 * max(L, 1) * (n_max + 16) * EPS
    worst = 0.0
    with lineage.TransportChain(lat, storage=storage, device=DEV) as chain:
        if storage == "f64":
            plans = [s.plan("numpy") for s in chain.solvers]
        else:                                                          # its own K, read back: not the f64 plan
            plans = [_host_plan(s) for s in chain.solvers]
        for t in range(T):
            got = chain.trajectories(lab[t], t)
            want = ref.trajectories(plans, lab[t], t)
            for u in range(T):
                worst = max(worst, _assert_rel(got[u], want[u], rt(abs(u - t)), ("trajectories", t, u)))
        for u in range(1, T):
            for t in range(u):
                worst = max(worst, _assert_rel(chain.fates(lab[u], u, t), ref.fates(plans, lab[u], u, t), rt(u - t), ("fates", u, t)))
                worst = max(worst, _assert_rel(chain.transition_table(lab[t], lab[u], t, u),
                                               ref.transition_table(plans, lab[t], lab[u], t, u), rt(u - t), ("table", t, u)))
        consecutive = [chain.transition_table(lab[t], lab[t + 1], t, t + 1) for t in range(T - 1)]
        assert len(chain.infos) == T - 1 and all(len(i) == 3 for i in chain.infos)
    print(f"chain {sizes} {storage}: worst error {worst:.4f} of rtol")
    again = analyze_ot.transition_tables(lat, lab, storage=storage, device=DEV)
    for t, (tab, _) in enumerate(again):
        np.testing.assert_allclose(consecutive[t], tab, rtol=1e-12, atol=0)
    assert not chain.solvers


# ---- end to end ----
def test_analyze_with_lineage_end_to_end(tmp_path):
    import pandas as pd
    from spadot_amd import analyze, analyze_ot
    from spadot_amd.utils._analyze_utils import have_matplotlib
    from test_analyze_gpu import _Args, _write_latent
    f = tmp_path / "latent.npz"
    X, tp, rows = _write_latent(f)
    out = analyze(_Args(data=str(f), n_clusters=[5, 6, 7], lineage=True, write_tmaps=True))
    tps = ["E1", "E2", "E3"]
    files = set(os.listdir(tmp_path))
    want = {"domains.csv", "OT_g.txt", "trajectories.npz", "fates.npz"} | \
           {f"transition_table_{d}_{e}.{x}" for d, e in ((0, 1), (1, 2), (0, 2)) for x in ("csv", "npz")}
    if have_matplotlib():
        want |= {f"{t}_domains.png" for t in tps} | {f"transition_dotplot_{d}_{e}.png" for d, e in ((0, 1), (1, 2), (0, 2))}
    assert want <= files, want - files
    assert {"tmap_0_1.npz", "tmap_1_2.npz"} <= set(os.listdir(tmp_path / "OT"))
    assert out["timings"]["lineage"] > 0 and set(out["timings"]) == {"clustering", "ot", "lineage", "writing"}
    labels = [out["labels"][t] for t in tps]
    np.testing.assert_array_equal(pd.read_csv(tmp_path / "domains.csv")["row"].to_numpy(), rows)
    tabs = analyze_ot.transition_tables([X[tp == t] for t in tps], labels, device=DEV)
    for d, (tab, _) in enumerate(tabs):
        z = np.load(tmp_path / f"transition_table_{d}_{d + 1}.npz")
        np.testing.assert_allclose(z["X"], tab, rtol=1e-12, atol=0)
        np.testing.assert_allclose(out["tables"][d], tab, rtol=1e-12, atol=0)
    z = np.load(tmp_path / "transition_table_0_2.npz")
    assert z["X"].shape == (5, 7) and z["obs_names"].tolist() == [f"E1_{c}" for c in range(5)]
    assert z["var_names"].tolist() == [f"E3_{c}" for c in range(7)] and (z["X"] >= 0).all() and z["X"].sum() > 0
    np.testing.assert_array_equal(z["X"], out["lineage"]["long_tables"][(0, 2)])
    csv = (tmp_path / "transition_table_0_2.csv").read_text().splitlines()
    assert csv[0].split(",")[1] == "E3_0" and len(csv) == 6
    # with no zero row sum the long-range table hands on all the mass of the first plan
    assert z["X"].sum() == pytest.approx(tabs[0][0].sum(), rel=1e-9)

    tr = np.load(tmp_path / "trajectories.npz")
    np.testing.assert_array_equal(tr["rows"], rows)                   # input order
    np.testing.assert_array_equal(tr["timepoint"].astype(str), tp)
    assert tr["names"].tolist() == [f"{t}_{c}" for t, k in zip(tps, (5, 6, 7)) for c in range(k)]
    Xt = tr["X"]
    assert Xt.dtype == np.float64 and Xt.shape == (X.shape[0], 18) and np.isfinite(Xt).all() and (Xt >= 0).all()
    np.testing.assert_array_equal(Xt, out["lineage"]["trajectories"])
    for t in tps:
        m = tp == t
        s = Xt[m].sum(0)
        assert np.all(np.abs(s - 1) <= 2 * (m.sum() + 16) * EPS), (t, s)      # a sum of n roundings of a normalised column
    c0 = 0
    for t, k, lab in zip(tps, (5, 6, 7), labels):                      # at its own time point a domain is 1_c / |c|
        own = Xt[tp == t][:, c0:c0 + k]
        for c in range(k):
            np.testing.assert_array_equal(own[:, c], np.where(lab == c, 1.0 / (lab == c).sum(), 0.0))
        c0 += k

    fa = np.load(tmp_path / "fates.npz")
    np.testing.assert_array_equal(fa["rows"], rows)
    assert fa["names"].tolist() == [f"E3_{c}" for c in range(7)]
    Xf = fa["X"]
    assert Xf.shape == (X.shape[0], 7) and np.isfinite(Xf).all() and (Xf >= 0).all()
    assert np.all(np.abs(Xf.sum(1) - 1) <= 16 * EPS)
    np.testing.assert_array_equal(Xf[tp == "E3"], np.eye(7)[labels[2]])


def test_analyze_without_lineage_writes_none_of_it(tmp_path):
    from spadot_amd import analyze
    from test_analyze_gpu import _Args, _write_latent
    f = tmp_path / "latent.npz"
    _write_latent(f)
    out = analyze(_Args(data=str(f), n_clusters=[5, 6, 7], lineage=False))
    files = set(os.listdir(tmp_path))
    assert not files & {"trajectories.npz", "fates.npz", "transition_table_0_2.csv", "transition_table_0_2.npz",
                        "transition_dotplot_0_2.png"}
    assert "lineage" not in out and set(out["timings"]) == {"clustering", "ot", "writing"}
    assert {"transition_table_0_1.csv", "transition_table_1_2.npz"} <= files


def test_command_line_lineage(tmp_path):
    from test_analyze_gpu import _write_latent
    f = tmp_path / "latent.npz"
    _write_latent(f)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "spadot_amd", "analyze", "-i", str(f), "--n_clusters", "5,6,7", "-o",
                        str(tmp_path / "out"), "--lineage"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    files = set(os.listdir(tmp_path / "out"))
    assert {"domains.csv", "transition_table_0_1.csv", "transition_table_0_2.csv", "trajectories.npz", "fates.npz"} <= files
