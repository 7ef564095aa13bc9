"""CPU checks of tests/svgp_cases.py: the fp64 reference of the SVGP branch against the golden values and against
finite differences, its own conditioning on every case, and every case against the branch it is there for -- derived here
from the recorded geometry constants and the case's shape, so that a case which no longer reaches its branch fails on
the CPU instead of passing quietly on the GPU."""
import numpy as np
import pytest
import torch

import svgp_cases as C
from conftest import load_golden

G = C.GEOM
cdiv = lambda a, b: -(-a // b)


# ----------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("tag", ["s", "l"])
def test_core_ref_reproduces_the_golden_posterior_and_elbo_terms(tag):
    """One latent dimension (y, noise) of tests/golden/model_svgp.npz, at the tolerances
    test_kernel_matrix_and_svgp_match_reference uses for the same quantities.  z carries log(noise) in fp64 (fp64_z): the
    golden noise is not the fp32 exponential of anything."""
    g = load_golden("model_svgp.npz")
    y, noise = torch.as_tensor(g[f"{tag}_y"]), torch.as_tensor(g[f"{tag}_noise"])
    z = torch.stack([y, torch.log(noise)], dim=1)
    ref = C.svgp_core_ref(g[f"{tag}_z"], torch.as_tensor(g[f"{tag}_x"]), z, float(g[f"{tag}_N_train"]), None, None, None, fp64_z=True)
    np.testing.assert_allclose(ref["p_m"][:, 0].numpy(), g[f"{tag}_mean"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(ref["p_v"][:, 0].numpy(), g[f"{tag}_B"], rtol=1e-6, atol=1e-9)
    assert ref["l3"] == pytest.approx(float(g[f"{tag}_l3"]), rel=1e-7)
    assert ref["kl"] == pytest.approx(float(g[f"{tag}_kl"]), rel=1e-7)
    assert ref["dz"] is None


FD_CASES = [c for c in C.CORE_CASES if (c["b"], c["m"], c["L"], c["N"]) in {(37, 17, 3, 5000.0), (70, 65, 2, 37.0)}]


@pytest.mark.parametrize("case", FD_CASES, ids=C.case_id)
def test_core_ref_gradient_equals_central_differences(case):
    """dz of the fp64 copy of the reference (z and the exponential in fp64) against central differences of
    <G_pm, p_m> + <G_pv, p_v> + g_skl SVGP_KL at six random coordinates, for both signs of dd and every gradient subset.
    Step 1e-4: measured over h = 1e-3 .. 1e-6 on these eight cases, the worst difference was 4.5e-8 of max |dz| at 1e-3
    (truncation), 2.6e-8 at 1e-4, 5.7e-7 at 1e-5 and 7.3e-6 at 1e-6 (rounding of the two inverses, cond ~1e6, over 2 h).
    Bound: 2e-7 of max |dz|, eight times the worst at the chosen step."""
    inp = C.core_inputs(case)
    z = inp["z32"].double()
    args = (inp["inducing"], inp["x"])
    ref = C.svgp_core_ref(*args, z, inp["N"], inp["G_pm"], inp["G_pv"], inp["g_skl"], fp64_z=True)
    assert np.sign(ref["dd"]) == case["sign"]

    def objective(zz):
        r = C.svgp_core_ref(*args, zz, inp["N"], None, None, None, fp64_z=True)
        assert np.sign(r["dd"]) == case["sign"]              # (no kink of |dd| inside the stencil)
        tot = 0.0
        if inp["G_pm"] is not None:
            tot += float((inp["G_pm"] * r["p_m"]).sum())
        if inp["G_pv"] is not None:
            tot += float((inp["G_pv"] * r["p_v"]).sum())
        if inp["g_skl"] is not None:
            tot += float(inp["g_skl"]) * r["skl"]
        return tot

    h, scale = 1e-4, float(ref["dz"].abs().max())
    rng = np.random.default_rng(3)
    for _ in range(6):
        i, j = int(rng.integers(case["b"])), int(rng.integers(2 * case["L"]))
        zp, zm = z.clone(), z.clone()
        zp[i, j] += h; zm[i, j] -= h
        fd = (objective(zp) - objective(zm)) / (2 * h)
        assert abs(fd - float(ref["dz"][i, j])) <= 2e-7 * scale, (i, j, fd, float(ref["dz"][i, j]), scale)


def test_core_ref_takes_the_exponential_in_fp32_and_leaves_out_null_gradients():
    case = next(c for c in C.CORE_CASES if c["grads"] == C.ALL and (c["b"], c["m"], c["L"]) == (37, 17, 3))
    inp, ref = C.core_reference(case)
    L = case["L"]
    # the reference's var is the fp32 exponential: its p_v differs from the fp64 copy's by what that rounding is worth
    r64 = C.svgp_core_ref(inp["inducing"], inp["x"], inp["z32"], inp["N"], None, None, None, fp64_z=True)
    assert not torch.equal(ref["p_v"], r64["p_v"])
    np.testing.assert_allclose(ref["p_v"].numpy(), r64["p_v"].numpy(), rtol=1e-5)
    assert ref["dz"].dtype == torch.float32 and ref["dz"].shape == (case["b"], 2 * L)
    # linear in the upstream gradients: the subsets add up to the whole (three fp32 roundings of dz, 2^-24 each, doubled)
    parts = [C.core_reference(c)[1]["dz"].double() for c in C.CORE_CASES
             if (c["b"], c["m"], c["L"], c["N"]) == (37, 17, 3, 5000.0) and c["grads"] in (C.PV_SKL, C.PM)]
    assert len(parts) == 2
    np.testing.assert_allclose((parts[0] + parts[1]).numpy(), ref["dz"].double().numpy(), rtol=0, atol=4e-7 * float(ref["dz"].abs().max()))
    assert ref["skl"] == -abs(ref["dd"]) / L
    # var32: the exponential's values handed in -- this CPU's own give the same bits back, values and gradient
    own = C.svgp_core_ref(inp["inducing"], inp["x"], inp["z32"], inp["N"], inp["G_pm"], inp["G_pv"], inp["g_skl"],
                          var32=torch.exp(inp["z32"][:, L:]))
    assert torch.equal(own["p_m"], ref["p_m"]) and torch.equal(own["dz"], ref["dz"]) and own["dd"] == ref["dd"]
    # ... and one fp32 ulp more on every var moves p_v and dz (the override is live, in the values and in the slope), dz by
    # no more than a relative 2^-23 of var is worth through terms in 1 / var, 1 / var^2 and var: 1e-5 is generous
    up = C.svgp_core_ref(inp["inducing"], inp["x"], inp["z32"], inp["N"], inp["G_pm"], inp["G_pv"], inp["g_skl"],
                         var32=torch.nextafter(torch.exp(inp["z32"][:, L:]), torch.tensor(10.0)))
    assert not torch.equal(up["p_v"], ref["p_v"])
    np.testing.assert_allclose(up["dz"].numpy(), ref["dz"].numpy(), rtol=0, atol=1e-5 * float(ref["dz"].abs().max()))


# ----------------------------------------------------------------------------------------------- conditioning gate
@pytest.mark.parametrize("case", C.CORE_CASES + C.LARGE_M_CASES, ids=C.case_id)
def test_case_is_well_conditioned_for_the_gradient_bound(case):
    """The reference twice, with the inducing points in the given and in a permuted order: mathematically the same
    function, so the difference is the reference's own rounding at this case.  It has to stay below a tenth of the GPU
    test's gradient bound (2e-6 of max |dz|); measured: 0 .. 6e-8 absolute, the fp32 rounding of dz.  A case that fails
    here gets other inputs, not a looser bound."""
    inp, ref = C.core_reference(case)
    perm = np.random.default_rng(1).permutation(case["m"])
    again = C.svgp_core_ref(inp["inducing"][perm], inp["x"], inp["z32"], inp["N"], inp["G_pm"], inp["G_pv"], inp["g_skl"])
    diff = float((again["dz"].double() - ref["dz"].double()).abs().max())
    scale = float(ref["dz"].abs().max())
    print(f"{C.case_id(case)}: max |d dz| {diff:.3e}, gate {0.1 * 2e-6 * scale:.3e}")
    assert scale > 0 and diff <= 0.1 * 2e-6 * scale, (diff, scale)
    assert case["N"] <= 1e6                                   # (beyond, the reference's own gradient noise reaches 5e-5)


# ----------------------------------------------------------------------------------------------- the cases reach their branches
def _grid(b, m, L):
    ext = {"bL": b * L, "Lm": L * m, "mm": m * m}
    top = max(ext.values())
    best = [k for k, v in ext.items() if v == top]
    return "tie" if len(best) == 3 else (best[0] if len(best) == 1 else "+".join(best))


@pytest.mark.parametrize("case", C.CORE_CASES + C.LARGE_M_CASES, ids=C.case_id)
def test_core_case_records_its_grid_and_sign(case):
    assert case["grid"] == _grid(case["b"], case["m"], case["L"])
    assert np.sign(C.core_reference(case)[1]["dd"]) == case["sign"]
    assert abs(C.core_reference(case)[1]["dd"]) > 1e-3        # (not so close to the kink that rounding picks the sign)


def test_core_cases_cover_the_branches():
    cases = C.CORE_CASES
    shapes = {(c["b"], c["m"], c["L"]) for c in cases}
    bL = {b * L for b, m, L in shapes}
    # k_svgp_post_bwd: each extent sizes the grid somewhere, and somewhere L > m > b and b < m
    assert {"bL", "Lm", "mm", "tie"} <= {c["grid"] for c in cases}
    assert any(L > m > b for b, m, L in shapes) and (1, 1, 1) in shapes
    assert any(c["grid"] == "mm" and c["b"] < c["m"] for c in cases)
    # k_svgp_post_fwd: one workgroup of 1024, unroll 5 -- thread 0 makes ceil(bL / 1024) trips; 1024 fills the first trip
    # exactly, 1025 starts a second one (a remainder of the unrolled group, for one thread only)
    T = G["post_fwd_threads"]
    trips = {n: cdiv(n, T) for n in bL}
    assert T in bL and T + 1 in bL and trips[T] == 1 and trips[T + 1] == 2
    assert all(t % G["post_fwd_unroll"] != 0 for t in trips.values())          # (every case ends in the unroll's remainder ...)
    assert max(trips.values()) < G["post_fwd_unroll"]                          # ... none fills it: b*L >= 5120 is the default shape's
    # the 256-thread flat grids: exactly one workgroup, a second with one thread, several
    W = G["flat_wg"]
    assert W + 1 in bL and any(n <= W for n in bL) and any(n > 2 * W for n in bL)
    assert any(L == 1 for b, m, L in shapes)
    # wave-per-row kernels: trips over m of a 64-lane wave, and rows in the last workgroup of four
    S = G["lane_stride"]
    ms = {m for b, m, L in shapes}
    assert {S - 1, S, S + 1} <= ms and {1, 2, 3} <= {cdiv(m, S) for m in ms}
    assert any(m % G["rows_per_wg"] == 1 for m in ms) and any(m % G["rows_per_wg"] == 0 for m in ms)
    assert len({(m + 2 * b) % G["rows_per_wg"] for b, m, L in shapes}) >= 3    # mid2's rows: M's and X2's together
    assert any((b * L) % G["rows_per_wg"] for b, m, L in shapes)               # pre2: a last workgroup with idle waves
    # k_svgp_q1t (the HOOK_CASES run it): partial 16 x 16 tiles, one tile and several
    Q = G["q1t_tile"]
    hb = {c["b"] for c in C.HOOK_CASES}
    assert len(C.HOOK_CASES) == 3 and all(b % Q for b in hb)
    assert {cdiv(b, Q) for b in hb} >= {3, 5}
    # both signs at least twice, and every gradient subset on two shapes, one of each sign
    for s in (+1, -1):
        assert len({(c["b"], c["m"], c["L"], c["N"]) for c in cases if c["sign"] == s}) >= 2
    for sub in (C.ALL, C.PV_SKL, C.SKL, C.PM):
        assert {c["sign"] for c in cases if c["grads"] == sub} == {+1, -1}
    assert all(c["N"] <= 1e6 for c in cases)


def test_large_m_cases_take_the_recursive_route():
    """With SWEEP_DIRECT_M = ops._SPLIT[0] = 16 both cases leave the direct sweep, and the two-block elimination
    (m1 = ceil(m / 2)) recurses at least twice, with uneven blocks for the odd m."""
    def depth(m):
        return 0 if m <= C.LARGE_M_SPLIT else 1 + max(depth((m + 1) // 2), depth(m - (m + 1) // 2))
    assert [depth(c["m"]) for c in C.LARGE_M_CASES] == [2, 3, 2, 3]
    assert [c["parts"] for c in C.LARGE_M_CASES] == [0, 0, 3, 3]
    assert any(c["m"] % 2 for c in C.LARGE_M_CASES) and {c["sign"] for c in C.LARGE_M_CASES} == {+1, -1}
    assert all(c["m"] <= G["sweep_max_m"] for c in C.LARGE_M_CASES)


def test_direct_entry_shapes_reach_their_edges():
    S, R, W, T = G["lane_stride"], G["rows_per_wg"], G["flat_wg"], G["post_fwd_threads"]
    # front kernels: every lane count of the partials' wave from one to all 64; one wave, idle waves, several trips over m
    assert C.FRONT_PARTS[0] == 1 and C.FRONT_PARTS[-1] == G["max_parts"] == S
    assert {cdiv(m, S) for b, L, m in C.FRONT_SHAPES} == {1, 2} and any((b * L) % R for b, L, m in C.FRONT_SHAPES)
    assert any(b * L > W for b, L, m in C.FRONT_SHAPES) and (1, 1, 1) in C.FRONT_SHAPES
    # mid: m around the stride and the row group; rows2 so that m + rows2 is and is not a multiple of four
    assert {S - 1, S, S + 1, 2 * S + 1, 1} <= set(C.MID_M) and {m % R for m in C.MID_M} == {0, 1, 3}
    assert len({(m + r) % R for m in C.MID_M for r in (1, 5, 2 * C.MID_B)}) == R
    # q1t: b and nh around the tile, nh != b
    Q = G["q1t_tile"]
    assert {Q - 1, Q, Q + 1, 2 * Q + 1, 1} <= set(C.Q1T_B) and {Q, Q + 1, 1} <= set(C.Q1T_NH) and max(C.Q1T_NH) > 2 * Q
    # post_forward / post_pm_pv
    assert [b * L for b, L in C.POST_BL] == [1, W - 1, W, W + 1, T, T + 1]
    # post_backward / grad_tail: every ordering of the three extents
    assert [_grid(b, m, L) for b, m, L in C.BWD_SHAPES] == ["bL", "Lm", "mm"]
    assert C.BWD_SHAPES[0][0] * C.BWD_SHAPES[0][2] > 2 * W                      # more than two workgroups of elements
    # sweep: TS = ceil(m / 31) from 1 to 10, each tile width at its largest m and the next at its smallest
    ts = lambda m: cdiv(m, G["sweep_grid"])
    assert {ts(m) for m in C.SWEEP_M} >= {1, 2, 3, 7, 8, 9, 10} and max(C.SWEEP_M) == G["sweep_max_m"]
    assert ts(G["sweep_max_m"] + 1) > 10
    for t in (1, 2, 8, 9):
        assert t * G["sweep_grid"] in C.SWEEP_M and t * G["sweep_grid"] + 1 in C.SWEEP_M
    assert ts(279) == G["sweep_core"] and ts(280) > G["sweep_core"]             # the first tile with a border in LDS
    assert (2, 5) in C.SWEEP_BATCH and 5 % 2 and (0, 3) in C.SWEEP_BATCH and max(L for _, L in C.SWEEP_BATCH) <= 6
    # kernel matrix: the last row of the first slab, the first and second of the second
    K = G["kmat_slab"]
    assert C.KMAT_N == [K, K + 1, K + 2]
