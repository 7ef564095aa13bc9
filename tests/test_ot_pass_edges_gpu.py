"""The Sinkhorn scaling pass on the MI355X against tests/ot_pass_ref.py (plain numpy, longdouble sums; held to the C oracle by
tests/test_ot_pass_ref_cpu.py) at every register-tile width of the fused pass (fp32 vpt 1..10, fp64 vpt 1..12), the band shapes
its row loop distinguishes, a band longer than the workgroup, and the two-sweep kernels' loop tails (tests/ot_pass_cases.py).

Every case asserts OTSolver.fused_geometry() against cases.fused_geometry_expected before it looks at a value.  The expected
values come from the K the kernel read, so exp() does not enter, and the bounds are derived, not measured:

  fp64 storage, and a' of fp32 storage (K exact, fp64 sums): a sum of n <= 20 480 positive terms is off by at most n * 2^-53 =
      2.3e-12 relative, the exponent alpha < 1 does not enlarge it, log / exp add a few ulps: RTOL64 = 1e-11 (the figure of
      test_compat_step1_matches_reference_vectors); K after an absorb the same with atol 1e-300.
  a' of fp32 vpt 9, 10 (w staged as fp32): RTOL64 against the reference that rounds w to fp32; against the exact-w reference
      2^-23 (each w_j off by at most 2^-24 relative, all terms positive, doubled).
  b' of fp32 storage, fused pass: the column partials are stored as fp32, one per workgroup, all positive, each off by at most
      2^-24: 2^-23.  The two-sweep kernels keep fp64 partials: RTOL64.

All comparisons run over all I and all J entries (the one exception is stated at test 5: plan entries of fp32 solves, by the
project's own rule)."""
import contextlib
import os

import numpy as np
import pytest
import torch

import ot_pass_cases as cases
import ot_pass_ref as ref

pytestmark = pytest.mark.gpu

RTOL64 = 1e-11
RTOL_F32 = 2.0 ** -23
STD_CFG = dict(lambda1=0.1, lambda2=5.0, epsilon=0.05, epsilon0=1.0, tolerance=1e-8, tau=1000.0, batch_size=5, max_iter=10 ** 7)

F64_SPECS = [s for s in cases.WIDTH_SPECS + cases.BAND_SPECS + [cases.LONG_SPEC] + cases.TWO_SWEEP_SPECS if s[1] == "f64"]
ABSORB_SPECS = [("width", "f64", vpt, "lo") for vpt in range(1, 13)]
FAST_SPECS = ([s for s in cases.WIDTH_SPECS + cases.BAND_SPECS + cases.TWO_SWEEP_SPECS if s[1] == "f32"]
              + [s for s in cases.WIDTH_SPECS if s[1] == "f64" and s[2] in (1, 6, 7, 12)])
SHORT_ROWS = 24          # tests 4 and 5: the single-thread oracle runs whole stages, so the problems are short and wide


@pytest.fixture(scope="module")
def shim():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spadot_amd.utils.OT_loss import ot_func
    return ot_func


@pytest.fixture(scope="module")
def OTSolver():
    from spadot_amd.ot import OTSolver
    return OTSolver


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@contextlib.contextmanager
def _kernels_of(case):
    """SPADOT_OT_NO_FUSED=1 around a forced two-sweep case (read when a solver is created)."""
    if not case["no_fused"]:
        yield
        return
    os.environ["SPADOT_OT_NO_FUSED"] = "1"
    try:
        yield
    finally:
        del os.environ["SPADOT_OT_NO_FUSED"]


def _assert_geometry(OTSolver, case, cus):
    """The geometry the library chooses for the case's shape is the one the case names; returns the expectation."""
    want = cases.fused_geometry_expected(case["I"], case["J"], case["storage"], cus, no_fused=case["no_fused"])
    s = OTSolver(case["I"], case["J"], storage=case["storage"])
    try:
        assert s.fused_geometry() == cases.public_geometry(want), case["name"]
        assert s.ld == want["ld"]
    finally:
        s.close()
    assert want["vpt"] == case["vpt"], case["name"]
    if case["kind"] == "sweep":
        assert cases.public_geometry(want) == cases.ZERO_GEOMETRY
    return want


def _step1(shim, st, tau, iters, l1=cases.L1, l2=cases.L2):
    o = {k: st[k].copy() for k in ("a", "b", "K", "u", "v")}
    o["old_a"], o["old_b"] = np.ones_like(st["a"]), np.ones_like(st["b"])
    eps = cases.EPS
    o["ret"] = shim.step1_process_c(o["a"], o["b"], o["old_a"], o["old_b"], o["K"], st["C"], st["dx"], st["dy"], st["p"], st["q"],
                                    o["u"], o["v"], 0, 10 ** 7, iters, tau, l1, l2, l1 / (l1 + eps), l2 / (l2 + eps), eps)
    return o


def _ref1(st, l1=cases.L1, l2=cases.L2, **kw):
    return ref.ref_iteration(st["a"], st["b"], st["K"], st["dx"], st["dy"], st["p"], st["q"], st["u"], st["v"], l1, l2, cases.EPS, **kw)


# ------------------------------------------------------------------------------------------------ 1. fp64, one pass, any state

@pytest.mark.parametrize("spec", F64_SPECS, ids=cases.spec_id)
def test_f64_one_pass_from_an_arbitrary_state(shim, OTSolver, cus, spec):
    case = cases.resolve(spec, cus)
    with _kernels_of(case):
        _assert_geometry(OTSolver, case, cus)
        st = cases.make_state(case["I"], case["J"], cases.seed_of(case))
        ra, rb = _ref1(st)[:2]
        assert np.isfinite(ra).all() and np.isfinite(rb).all() and max(ra.max(), rb.max()) < 1e-2 * cases.TAU_OFF
        out = _step1(shim, st, cases.TAU_OFF, 1)
    assert out["ret"] == 1
    np.testing.assert_allclose(out["a"], ra, rtol=RTOL64, err_msg="a")
    np.testing.assert_allclose(out["b"], rb, rtol=RTOL64, err_msg="b")
    np.testing.assert_array_equal(out["old_a"], st["a"])
    np.testing.assert_array_equal(out["old_b"], st["b"])
    for k in ("K", "u", "v"):
        np.testing.assert_array_equal(out[k], st[k], err_msg=k)


# ------------------------------------------------------------------------------------------------ 2. fp64, absorb at width

@pytest.mark.parametrize("spec", ABSORB_SPECS, ids=cases.spec_id)
def test_f64_absorb_at_width(shim, OTSolver, oracle_ot, cus, spec):
    """tau between the two largest scalings of the first iteration: the one exceeding element is a' of the last row (p x 50),
    which sits in the short last band.  Two iterations, against the numpy reference and the C oracle; with tau just above
    the largest scaling nothing is absorbed."""
    case = cases.resolve(spec, cus)
    _assert_geometry(OTSolver, case, cus)
    st = cases.make_state(case["I"], case["J"], cases.seed_of(case), boost_last=True)
    l1, l2, eps = cases.ABSORB_L1, cases.ABSORB_L2, cases.EPS
    ra, rb = _ref1(st, l1, l2)[:2]
    top, second = ref.two_largest(ra, rb)
    assert top == ra[-1] and top > second * (1 + 1e-6)                  # conditions on the inputs, from the reference alone
    tau = float(np.sqrt(top * second))
    want = ref.ref_step(st["a"], st["b"], st["K"], st["C"], st["dx"], st["dy"], st["p"], st["q"], st["u"], st["v"], l1, l2, eps, tau, 2)
    assert want["absorbs"] >= 1
    for ma, mb in want["maxima"][1:]:                                    # the second iteration's decision is unambiguous too
        assert abs(max(ma, mb) / tau - 1) > 1e-6
    out = _step1(shim, st, tau, 2, l1, l2)
    assert out["ret"] == 2
    orc = {k: st[k].copy() for k in ("a", "b", "K", "u", "v")}
    orc["old_a"], orc["old_b"] = np.ones_like(st["a"]), np.ones_like(st["b"])
    oracle_ot.step1_process(orc["a"], orc["b"], orc["old_a"], orc["old_b"], orc["K"], st["C"], st["dx"], st["dy"], st["p"], st["q"],
                            orc["u"], orc["v"], 0, 10 ** 7, 2, tau, l1, l2, l1 / (l1 + eps), l2 / (l2 + eps), eps)
    for k in ("u", "v", "K", "a", "b", "old_a", "old_b"):
        np.testing.assert_allclose(out[k], want[k], rtol=RTOL64, atol=1e-300, err_msg=f"{k} vs reference")
        np.testing.assert_allclose(out[k], orc[k], rtol=RTOL64, atol=1e-300, err_msg=f"{k} vs oracle")
    assert not np.array_equal(out["K"], st["K"])
    # tau just above the largest scaling: nothing is absorbed
    calm = _step1(shim, st, top * (1 + 1e-6), 1, l1, l2)
    for k in ("K", "u", "v"):
        np.testing.assert_array_equal(calm[k], st[k], err_msg=k)
    np.testing.assert_allclose(calm["a"], ra, rtol=RTOL64)
    np.testing.assert_allclose(calm["b"], rb, rtol=RTOL64)


# ------------------------------------------------------------------------------------------------ 3. one fast pass on the solver

def _mixture(rng, n, cen, sigma=0.3):
    return cen[rng.integers(0, cen.shape[0], size=n)] + sigma * rng.normal(size=(n, cen.shape[1]))


@pytest.mark.parametrize("spec", FAST_SPECS, ids=cases.spec_id)
def test_fast_pass_on_the_solver_state(OTSolver, cus, spec):
    """After a whole solve the solver holds a consistent state; K and the vectors are read back and ONE fast-mode pass with
    another lambda1, lambda2 and epsilon (far from the state's fixed point: an un-updated row cannot hide) is compared with
    the reference on the read-back K.  The tau flag is raised exactly when a scaling exceeds tau."""
    case = cases.resolve(spec, cus)
    I, J, storage = case["I"], case["J"], case["storage"]
    fused = case["kind"] != "sweep"
    with _kernels_of(case):
        want_geo = _assert_geometry(OTSolver, case, cus)
        rng = np.random.default_rng(cases.seed_of(case))
        cen = rng.normal(size=(10, 20))
        x, y = _mixture(rng, I, cen), _mixture(rng, J, cen + 0.05)
        G = rng.uniform(0.5, 2.0, I)
        G[-1] *= 50.0
        s = OTSolver(I, J, storage=storage)
    try:
        s.set_cost_from_latents(x, y)
        s.solve(STD_CFG, G)
        K = s.matrix("K")
        fix = dict(K=K, p=G, q=np.full(J, G.sum() / I), dx=np.full(I, 1.0 / I), dy=np.full(J, 1.0 / J), u=s.vector("u"), v=s.vector("v"))
        l1, l2, eps2 = 0.3, 2.0, 0.2
        w_fp32 = storage == "f32" and want_geo["vpt"] > 8

        def reference(a, b, **kw):
            return ref.ref_iteration(a, b, K, fix["dx"], fix["dy"], fix["p"], fix["q"], fix["u"], fix["v"], l1, l2, eps2, **kw)

        s.tau_flag(reset=True)
        for round_, place in enumerate(("between", "above")):
            a0, b0 = s.vector("a"), s.vector("b")
            ra, rb = reference(a0, b0, w_fp32=w_fp32)[:2]
            assert np.isfinite(ra).all() and np.isfinite(rb).all() and ra.min() > 0 and rb.min() > 0
            top, second = ref.two_largest(ra, rb)
            assert top > second * (1 + 1e-4), "the inputs leave no unambiguous place for tau"
            tau = float(np.sqrt(top * second)) if place == "between" else top * (1 + 1e-4)
            s.run_iterations(dict(STD_CFG, lambda1=l1, lambda2=l2, tau=tau), eps2, 1, timed=False)
            assert s.tau_flag(reset=True) == (place == "between"), place
            a1, b1 = s.vector("a"), s.vector("b")
            np.testing.assert_allclose(a1, ra, rtol=RTOL64, err_msg=f"a ({place})")
            np.testing.assert_array_equal(s.vector("old_a"), a0)
            np.testing.assert_array_equal(s.vector("old_b"), b0)
            if round_ == 0:
                if w_fp32:
                    ra_exact, rb_dev = reference(a0, b0, a_col=a1)[:2]
                    np.testing.assert_allclose(a1, ra_exact, rtol=RTOL_F32, err_msg="a (exact w)")
                else:
                    rb_dev = reference(a0, b0, a_col=a1, columns_only=True)[1]
                np.testing.assert_allclose(b1, rb_dev, rtol=RTOL_F32 if (storage == "f32" and fused) else RTOL64, err_msg="b")
            else:
                # the second pass starts from the first one's scalings; b' against the reference's own a' (a' is within RTOL64)
                np.testing.assert_allclose(b1, rb, rtol=RTOL_F32 + 2 * RTOL64 if (storage == "f32" and fused) else 2 * RTOL64,
                                           err_msg="b (second pass)")
        np.testing.assert_array_equal(s.matrix("K"), K)                  # fast mode leaves K, u, v alone
        np.testing.assert_array_equal(s.vector("u"), fix["u"])
        np.testing.assert_array_equal(s.vector("v"), fix["v"])
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ 4. exact-mode stage at width

@pytest.mark.parametrize("vpt", [2, 6, 7, 12])
def test_f64_exact_mode_stage_at_width(shim, OTSolver, oracle_ot, cus, vpt):
    """update_process on the last stage (the full gap measure with R each batch) from test 1's state, 24 rows wide."""
    I, J = SHORT_ROWS, cases.width_J("f64", vpt, "lo")
    _assert_geometry(OTSolver, dict(name=f"short-f64-{vpt}", kind="short", storage="f64", I=I, J=J, no_fused=False, vpt=vpt), cus)
    st = cases.make_state(I, J, seed=4000 + vpt)
    l1, l2, eps = cases.ABSORB_L1, cases.ABSORB_L2, cases.EPS
    Kb = np.exp(-st["C"] / eps)
    res = []
    for impl in ("hip", "oracle"):
        o = {k: st[k].copy() for k in ("a", "b", "K", "u", "v")}
        o["old_a"], o["old_b"], o["R"] = np.ones(I), np.ones(J), np.zeros((I, J))
        args = (o["R"], o["a"], o["b"], o["old_a"], o["old_b"], o["K"], Kb, st["C"], st["dx"], st["dy"], st["p"], st["q"], o["u"], o["v"],
                5, 5, 5, eps, 1e-8, cases.TAU_OFF, l1, l2, l1 / (l1 + eps), l2 / (l2 + eps), 0, 10 ** 7)
        if impl == "hip":
            o["gap"] = shim.update_process_c(*args)
        else:
            o["gap"], o["iters"] = oracle_ot.update_process(*args)
        res.append(o)
    assert res[0]["gap"] <= 1e-8 and res[1]["gap"] <= 1e-8 and res[1]["iters"] >= 10
    for k in ("K", "R", "a", "b", "u", "v", "old_a", "old_b"):
        np.testing.assert_allclose(res[0][k], res[1][k], rtol=1e-9, atol=1e-300, err_msg=k)


# ------------------------------------------------------------------------------------------------ 5. row-dot and pipelined loop

SOLVE_SPECS = ([("f64", vpt, SHORT_ROWS) for vpt in range(1, 13)] + [("f32", vpt, SHORT_ROWS) for vpt in (2, 6, 8, 9, 10)]
               + [("f64", 2, "tall")])
ABSORB_ALWAYS = 0.5      # a tau below the scalings of every iteration (they start from 1 after each absorb)


@pytest.mark.parametrize("tau", [1000.0, ABSORB_ALWAYS], ids=["pipelined", "rowdot"])
@pytest.mark.parametrize("storage,vpt,rows", SOLVE_SPECS, ids=lambda x: str(x))
def test_whole_solve_at_width_vs_oracle(OTSolver, oracle_ot, cus, storage, vpt, rows, tau):
    """Whole solves against the C oracle.  tau = 1000: the last stage is the pipelined loop, whose measure takes the row sums the
    next batch's first pass stores (the WRS instantiation of k_fused_pass).  tau = 0.5: every iteration exceeds tau, so every
    batch is flagged, restored and redone exactly (info.absorbs counts one absorb per iteration) and its gap is the plain
    measure, whose row sums are k_fused_rowdot's: that kernel decides when the stage ends.  fp64: equal iteration counts, the
    same gap (rel 1e-3, the figure of test_small_solver_vs_oracle_absorb_batch_and_edges), plan entries rtol 1e-8; fp32: counts
    within one check (5) per stage, entries above 1e-9 * max rtol 1e-3 (the rule of test_solver_f32_within_stated_tolerance:
    smaller entries underflow in fp32 storage), marginals rtol 1e-4.  'tall': cus * 8 + 3 rows, five groups a band."""
    I = cus * 8 + 3 if rows == "tall" else rows
    J = 1100 if rows == "tall" else cases.width_J(storage, vpt, "lo")
    _assert_geometry(OTSolver, dict(name=f"solve-{storage}-{vpt}-{rows}", kind="short", storage=storage, I=I, J=J, no_fused=False,
                                    vpt=vpt), cus)
    rng = np.random.default_rng(500 + 13 * vpt + I)
    cen = rng.normal(size=(10, 20))
    x, y = _mixture(rng, I, cen), _mixture(rng, J, cen + 0.1)
    C = oracle_ot.sqeuclidean_cost(x, y)
    C = C / np.median(C)
    G = rng.uniform(0.5, 2.0, I)
    cfg = dict(STD_CFG, tau=tau)
    want, winfo = oracle_ot.optimal_transport_duality_gap(C, G, return_info=True, **cfg)
    assert winfo["gap"] <= cfg["tolerance"]
    s = OTSolver(I, J, storage=storage)
    try:
        s.set_cost(C)
        info = s.solve(cfg, G)
        P = s.plan("numpy")
        rows_dev = s.plan_rowsums()
    finally:
        s.close()
    assert info.gap <= cfg["tolerance"]
    if tau == ABSORB_ALWAYS:
        assert info.absorbs == sum(info.stage_iters)
    if storage == "f64":
        assert list(info.stage_iters) == winfo["stage_iters"].tolist()
        assert info.gap == pytest.approx(winfo["gap"], rel=1e-3, abs=1e-12)
        np.testing.assert_allclose(P, want, rtol=1e-8, atol=1e-300)
        np.testing.assert_allclose(rows_dev, want.sum(axis=1), rtol=1e-9)
    else:
        for got, ref_it in zip(info.stage_iters, winfo["stage_iters"].tolist()):
            assert abs(got - ref_it) <= 5
        big = want > 1e-9 * want.max()
        np.testing.assert_allclose(P[big], want[big], rtol=1e-3)
        np.testing.assert_allclose(P.sum(axis=1), want.sum(axis=1), rtol=1e-4)
        np.testing.assert_allclose(P.sum(axis=0), want.sum(axis=0), rtol=1e-4)
        np.testing.assert_allclose(rows_dev, want.sum(axis=1), rtol=1e-4)
