"""Holds tests/ot_pass_ref.py and tests/ot_pass_cases.py to their own conditions, without a GPU: the numpy reference agrees with
the C oracle the project already trusts, the case table reaches every instantiated geometry and every band shape it names, and
the generated inputs satisfy what tests/test_ot_pass_edges_gpu.py relies on (finite scalings, an unambiguous place for tau, a
stored kernel inside the fp32 normal range)."""
import os
import re

import numpy as np
import pytest

import ot_pass_cases as cases
import ot_pass_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = cases.CPU_CUS
ALL_SPECS = cases.WIDTH_SPECS + cases.BAND_SPECS + [cases.LONG_SPEC] + cases.TWO_SWEEP_SPECS


# ------------------------------------------------------------------------------------------------ reference vs C oracle

@pytest.mark.parametrize("I,J", [(1, 1), (3, 129), (130, 67), (24, 1025), (257, 300)])
def test_ref_iteration_matches_oracle(oracle_ot, I, J):
    st = cases.make_state(I, J, seed=7 * I + J)
    l1, l2, eps = cases.L1, cases.L2, cases.EPS
    a, b = st["a"].copy(), st["b"].copy()
    oracle_ot.update_a_b(a, b, st["K"], st["dx"], st["dy"], st["p"], st["q"], st["u"], st["v"], l1, l2, l1 / (l1 + eps),
                         l2 / (l2 + eps), eps)
    ra, rb, roa, rob, ma, mb = ref.ref_iteration(st["a"], st["b"], st["K"], st["dx"], st["dy"], st["p"], st["q"], st["u"], st["v"],
                                                 l1, l2, eps)
    np.testing.assert_allclose(ra, a, rtol=1e-12)
    np.testing.assert_allclose(rb, b, rtol=1e-12)
    np.testing.assert_array_equal(roa, st["a"])
    np.testing.assert_array_equal(rob, st["b"])
    assert ma == ra.max() and mb == rb.max()
    # a_col: the column sums take the a' they are given
    ra2, rb2 = ref.ref_iteration(st["a"], st["b"], st["K"], st["dx"], st["dy"], st["p"], st["q"], st["u"], st["v"], l1, l2, eps,
                                 a_col=2.0 * ra)[:2]
    np.testing.assert_array_equal(ra2, ra)
    np.testing.assert_allclose(rb2, rb * 2.0 ** -(l2 / (l2 + eps)), rtol=1e-14)
    # w_fp32 moves a' by at most the rounding of w (all terms positive) and not at all when w is representable
    ra3 = ref.ref_iteration(st["a"], st["b"], st["K"], st["dx"], st["dy"], st["p"], st["q"], st["u"], st["v"], l1, l2, eps,
                            w_fp32=True)[0]
    np.testing.assert_allclose(ra3, ra, rtol=2.0 ** -24)
    assert J == 1 or not np.array_equal(ra3, ra)


@pytest.mark.parametrize("I,J,iters,mode", [(3, 129, 1, "none"), (130, 67, 2, "first"), (24, 1025, 2, "first"), (257, 300, 3, "first"),
                                            (40, 56, 3, "all")])
def test_ref_step_matches_oracle_step1(oracle_ot, I, J, iters, mode):
    """With no absorb, with an absorb after the first iteration only, and with one after every iteration."""
    st = cases.make_state(I, J, seed=11 * I + J, boost_last=True)
    l1, l2, eps = cases.ABSORB_L1, cases.ABSORB_L2, cases.EPS
    first = ref.ref_iteration(st["a"], st["b"], st["K"], st["dx"], st["dy"], st["p"], st["q"], st["u"], st["v"], l1, l2, eps)
    top, second = ref.two_largest(first[0], first[1])
    assert top > second * (1 + 1e-6)
    tau = {"none": top * (1 + 1e-6), "first": np.sqrt(top * second), "all": 1e-3}[mode]
    got = ref.ref_step(st["a"], st["b"], st["K"], st["C"], st["dx"], st["dy"], st["p"], st["q"], st["u"], st["v"], l1, l2, eps, tau, iters)
    o = {k: st[k].copy() for k in ("a", "b", "K", "u", "v")}
    oa, ob = st["a"].copy(), st["b"].copy()
    oracle_ot.step1_process(o["a"], o["b"], oa, ob, o["K"], st["C"], st["dx"], st["dy"], st["p"], st["q"], o["u"], o["v"], 0, 10 ** 7,
                            iters, tau, l1, l2, l1 / (l1 + eps), l2 / (l2 + eps), eps)
    o.update(old_a=oa, old_b=ob)
    for k in ("a", "b", "old_a", "old_b", "K", "u", "v"):
        # u, v pass zero, hence the absolute term: one ulp of eps * ln(a)
        np.testing.assert_allclose(got[k], o[k], rtol=1e-12, atol=1e-15 if k in "uv" else 0.0, err_msg=k)
    if mode == "none":
        assert got["absorbs"] == 0
        np.testing.assert_array_equal(got["K"], st["K"])
    elif mode == "all":
        assert got["absorbs"] == iters and (got["a"] == 1).all() and (got["b"] == 1).all()
    else:
        assert got["absorbs"] >= 1


# ------------------------------------------------------------------------------------------------ the case table

def _dispatch_table(fn):
    """(storage, vpt, rows per group) of every case of a dispatch switch in csrc/ot_sinkhorn.hip."""
    src = open(os.path.join(ROOT, "spadot_amd", "csrc", "ot_sinkhorn.hip")).read()
    out = set()
    for T, st in (("float", "f32"), ("double", "f64")):
        m = re.search(r"template <> void %s<%s>\(.*?\n}\n" % (fn, T), src, re.S)
        assert m, (fn, T)
        body = m.group(0)
        out |= {(st, int(v), int(r)) for v, r in re.findall(r"FUSED_CASE\(%s, (\d+), (\d+)\)" % T, body)}
        out |= {(st, int(v), int(r)) for v, r in re.findall(r"case (\d+): launch_fused\w*<%s, \d+, (\d+)" % T, body)}
    return out


def test_case_table_covers_every_instantiated_geometry():
    want = {(st, vpt, cases.rows_per_group(st, vpt)) for st in ("f32", "f64") for vpt in range(1, cases.MAX_VPT[st] + 1)}
    assert len(want) == 22
    assert _dispatch_table("fused_pass_T") == want
    assert _dispatch_table("fused_rowdot_T") == want
    for cus in (CUS, 304, 64):
        seen = {}
        for spec in cases.WIDTH_SPECS:
            c = cases.resolve(spec, cus)
            g = cases.fused_geometry_expected(c["I"], c["J"], c["storage"], cus)
            assert g["vpt"] == spec[2] and g["rows_per_group"] == cases.rows_per_group(spec[1], spec[2]), spec
            assert g["lds"] <= cases.LDS_LIMIT
            V, ld = cases.VEC[spec[1]], g["ld"]
            tile = g["vpt"] * V * cases.THREADS
            if spec[3] == "lo":
                assert ld - (tile - V * cases.THREADS) == 64 and ld - c["J"] == 63
            else:
                assert ld == tile and c["J"] == ld - 63
            full, last, last_rows = cases.band_groups(g, c["I"])
            # five groups a band: one round of the double-buffer loop and a tail of three; the last band is short
            assert full == 5 and g["workgroups"] > 1, (spec, g)
            last_band_rows = c["I"] - (g["workgroups"] - 1) * g["rows_per_workgroup"]
            assert last_band_rows < g["rows_per_workgroup"], (spec, g)
            if cus == 256:
                assert last_band_rows in (1, 2) and g["workgroups"] == 206
            seen.setdefault((spec[1], spec[2]), set()).add(spec[3])
        assert len(seen) == 22 and all(v == {"lo", "hi"} for v in seen.values())
    assert cases.resolve(("width", "f64", 1, "lo"), 256)["I"] == 2051 and cases.resolve(("width", "f64", 7, "lo"), 256)["I"] == 1027
    assert max(c["I"] * c["J"] * 8 for c in (cases.resolve(s, 256) for s in ALL_SPECS)) < 171e6


def test_case_table_covers_every_band_shape():
    for cus in (CUS, 304, 64):
        for st in ("f32", "f64"):
            for vpt in cases.BAND_VPT[st]:
                R = cases.rows_per_group(st, vpt)
                shapes = {}
                for sh in cases.BAND_SHAPES:
                    c = cases.resolve(("band", st, vpt, sh), cus)
                    g = cases.fused_geometry_expected(c["I"], c["J"], st, cus)
                    assert g["vpt"] == vpt and g["rows_per_group"] == R and g["lds"] <= cases.LDS_LIMIT
                    assert g["ld"] % (cases.VEC[st] * cases.THREADS) != 0          # the column clamp is in play
                    shapes[sh] = (g["workgroups"],) + cases.band_groups(g, c["I"])
                for n in (2, 3, 4, 6):
                    # every band n groups; the last band one row short: an odd row (two-row groups) or one group less
                    wg, full, last, last_rows = shapes[f"g{n}"]
                    assert wg == cus and full == n and last_rows == 1 and last == (n if R == 2 else n - 1)
                assert shapes["g1"] == (1, 1, 1, R)
                assert shapes["i1"] == (1, 1, 1, 1)
                assert shapes["i2r"] == (1, 2, 2, R)
                assert shapes["i2r1"] == (2, 2, 1, 1)
                # the row loop of k_fused_pass: rounds of the double-buffer loop and groups left for its tail
                loops = {cases.loop_rounds_and_tail(n) for sh in shapes.values() for n in sh[1:3]}
                assert {t for _, t in loops} == {1, 2, 3} and {r for r, _ in loops} >= {0, 1, 2}
        assert [cases.loop_rounds_and_tail(n) for n in (1, 2, 3, 4, 5, 6)] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 2)]
        c = cases.resolve(cases.LONG_SPEC, cus)
        g = cases.fused_geometry_expected(c["I"], c["J"], "f64", cus)
        assert g["vpt"] == 1 and g["rows_per_workgroup"] > cases.THREADS and g["lds"] <= cases.LDS_LIMIT
    assert cases.resolve(cases.LONG_SPEC, 256)["I"] == 131329


def test_two_sweep_cases_reach_every_loop_tail():
    for st in ("f32", "f64"):
        unit = 64 * cases.VEC[st]
        ratios, mods, natural = set(), set(), 0
        for spec in cases.TWO_SWEEP_SPECS:
            if spec[1] != st:
                continue
            c = cases.resolve(spec, CUS)
            g = cases.fused_geometry_expected(c["I"], c["J"], st, CUS, no_fused=c["no_fused"])
            assert cases.public_geometry(g) == cases.ZERO_GEOMETRY, spec
            natural += not c["no_fused"]
            ld = g["ld"]
            ratios.add("frac" if ld % unit else ("odd" if (ld // unit) % 2 else "even"))
            rpc, nchunk = cases.chunks_expected(c["I"], c["J"], st)
            if c["I"] < 16:
                assert nchunk == 1
            else:
                assert nchunk > 1 and c["I"] - (nchunk - 1) * rpc < rpc          # a short last chunk
                mods.add(rpc % 4)
        assert natural == 1 and ratios == {"frac", "odd", "even"} and mods == {0, 1, 2, 3}
    # one column past the widest tile is the natural fall-back, one column less is still fused
    assert cases.fused_geometry_expected(37, 20480, "f32", CUS)["vpt"] == 10 and cases.fused_geometry_expected(37, 12288, "f64", CUS)["vpt"] == 12


def test_expected_geometry_restates_known_shapes():
    """The two shapes tests/test_ot_gpu.py pins, and the LDS fall-back of a band too long for its row constants."""
    assert cases.fused_geometry_expected(10000, 10000, "f32", 256)["vpt"] == 5
    assert cases.fused_geometry_expected(1500, 20000, "f32", 256)["vpt"] == 10
    g = cases.fused_geometry_expected(256 * 4000, 12288, "f64", 256)
    assert cases.public_geometry(g) == cases.ZERO_GEOMETRY


# ------------------------------------------------------------------------------------------------ input conditions

COND_SPECS = [("width", "f64", 1, "lo"), ("width", "f64", 6, "lo"), ("width", "f64", 7, "hi"), ("band", "f64", 1, "g3"),
              ("band", "f64", 1, "i1"), ("band", "f64", 7, "g2"), ("sweep", "f64", 3, "forced"), ("sweep", "f64", 5, "natural")]


@pytest.mark.parametrize("spec", COND_SPECS, ids=cases.spec_id)
def test_generated_inputs_meet_the_gpu_tests_conditions(spec):
    c = cases.resolve(spec, CUS)
    for boost in (False, True):
        st = cases.make_state(c["I"], c["J"], cases.seed_of(c), boost_last=boost)
        assert st["K"].min() > np.finfo(np.float32).tiny          # (C < 4, |u + v| small: exp(-20 - ...) ~ 1e-9)
        l1, l2 = (cases.ABSORB_L1, cases.ABSORB_L2) if boost else (cases.L1, cases.L2)
        a, b = ref.ref_iteration(st["a"], st["b"], st["K"], st["dx"], st["dy"], st["p"], st["q"], st["u"], st["v"], l1, l2, cases.EPS)[:2]
        assert np.isfinite(a).all() and np.isfinite(b).all() and a.min() > 0 and b.min() > 0
        assert boost or max(a.max(), b.max()) < 1e-2 * cases.TAU_OFF          # the one-pass test's tau is out of reach
        top, second = ref.two_largest(a, b)
        if c["I"] + c["J"] > 2:
            assert top > second * (1 + 1e-6)
        if boost and c["kind"] == "width":
            assert top == a[-1]                  # the absorb test's one exceeding element: a' of the last row
