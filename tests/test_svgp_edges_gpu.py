"""The SVGP branch's fp64 kernels against an independent reference, at the shapes where their launch geometry changes.

(a), (b): _SVGPCore as the model drives it (direct sweep and the large-m route) against svgp_cases.svgp_core_ref -- the
reference's per-dimension arithmetic under torch autograd, which shares neither the device's algebra nor its hand-derived
backward.  (c) - (i): the C entries of the branch called directly, each against numpy / torch fp64 of its own formula.

The cases, the branch each one is there for and the reference are in svgp_cases.py; test_svgp_ref_cpu.py checks on the CPU
that the reference is right, that every case is well enough conditioned for the bounds used here, and that it reaches its
branch.  Tolerances: the project's stated ones (test_model_gpu.py) unless written beside the assertion."""
import ctypes
import math

import numpy as np
import pytest
import torch

import svgp_cases as C
from oracle import model_oracle as mo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spadot_amd import ops
    return ops


@pytest.fixture(scope="module")
def lib(ops):
    return ops.model_lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=F64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV).contiguous()


def host(t):
    return t.detach().cpu().numpy()


class Padded:
    """An output buffer of n elements between two NaN-filled margins: the entry has to overwrite all of it and nothing else."""

    def __init__(self, n, dtype=F64, pad=160):
        self.n, self.pad = n, pad
        self.full = torch.full((n + 2 * pad,), NAN, dtype=dtype, device=DEV)
        self.t = self.full[pad:pad + n]

    def check(self, name):
        f = host(self.full)
        assert np.isnan(f[:self.pad]).all() and np.isnan(f[self.pad + self.n:]).all(), f"{name}: written outside the buffer"
        assert not np.isnan(f[self.pad:self.pad + self.n]).any(), f"{name}: not fully written"
        return f[self.pad:self.pad + self.n]


# ------------------------------------------------------------------ (a), (b): the core as the model drives it

def run_core(sv, case, form=None):
    """One forward + backward of _SVGPCore through SVGP.batch_constants / elbo_start / elbo_finish on the case's inputs.
    form = (mid, pre, q1t, late) sets the backward's hooks as the forms-agree test does; None leaves them alone."""
    inp, _ = C.core_reference(case)
    mod = sv.SVGP(dict(device=DEV, kernel_type="Gaussian", kernel_scale=0.1), inp["inducing"], case["N"])
    x = inp["x"].to(DEV)
    old = sv.MID_BWD[0], sv.Q1T[0], sv.ELBO_LATE[0]
    mid, pre, q1t, late = form if form is not None else (old[0], False, old[1], False)
    try:
        sv.MID_BWD[0], sv.Q1T[0] = mid, q1t
        partials = None
        if case.get("parts"):
            z = torch.full(tuple(inp["z32"].shape), NAN, dtype=torch.float32, device=DEV).requires_grad_(True)
            partials = (inp["pz"].to(DEV).contiguous(), case["parts"], inp["bias"].to(DEV))
        else:
            z = inp["z32"].to(DEV).clone().requires_grad_(True)
        bc = mod.batch_constants(x)
        queue = [] if late else None
        sv.ELBO_LATE[0] = queue
        try:
            p_m, p_v, skl = mod.elbo_finish(bc, mod.elbo_start(bc, z, partials))
        finally:
            sv.ELBO_LATE[0] = old[2]
        head = p_m.detach().clone(), p_v.detach().clone()
        if late:
            assert len(queue) == 1
            with torch.no_grad():
                queue[0]()
        if pre:
            h = sv.precompute_backward(sv.holder_of(p_m))
            assert "q2" in h and "KS" in h and (("Ta" in h) == q1t)
        saved = p_m.grad_fn.saved_tensors                     # (mu, var, w, X, r, Mr, p_m, p_v, mv, tr, out4)
        out4, var = saved[-1].clone(), saved[1].clone()
        assert out4.shape == (4,) and out4.dtype == F64 and var.shape == (case["b"], case["L"])
        seeds = [(p_m, inp["G_pm"]), (p_v, inp["G_pv"]), (skl, None if inp["g_skl"] is None else inp["g_skl"].float())]
        seeds = [(o, g.to(DEV)) for o, g in seeds if g is not None]
        (dz,) = torch.autograd.grad([o for o, _ in seeds], [z], [g for _, g in seeds])
        return {"p_m": host(head[0]), "p_v": host(head[1]), "skl": skl.detach().cpu(), "out4": host(out4),
                "dz": host(dz.double()), "z": host(z), "var": host(var)}
    finally:
        sv.MID_BWD[0], sv.Q1T[0], sv.ELBO_LATE[0] = old


_REF_AT_VAR = {}


def check_core(case, got, tag=""):
    """The device's var = exp(logvar) against the fp64 exponential first (it is an fp32 value within VAR_RTOL); then
    everything behind it against the reference evaluated at that var (svgp_core_ref says why)."""
    inp, _ = C.core_reference(case)
    L = case["L"]
    var = got["var"]
    exact = np.exp(inp["z32"][:, L:].numpy().astype(np.float64))
    assert np.array_equal(var, var.astype(np.float32).astype(np.float64))
    assert (np.abs(var - exact) <= C.VAR_RTOL * exact).all(), float((np.abs(var - exact) / exact).max())
    key = (C.case_id(case), var.tobytes())
    if key not in _REF_AT_VAR:
        _REF_AT_VAR[key] = C.svgp_core_ref(inp["inducing"], inp["x"], inp["z32"], inp["N"], inp["G_pm"], inp["G_pv"], inp["g_skl"],
                                           var32=var.astype(np.float32))
    ref = _REF_AT_VAR[key]
    l3, ce, kl, skl64 = (float(v) for v in got["out4"])
    dz_ref = ref["dz"].double().numpy()
    scale = np.abs(dz_ref).max()
    err = np.abs(got["dz"] - dz_ref).max()
    print(f"{C.case_id(case)} {tag}: p_m {np.abs(got['p_m'] - ref['p_m'].numpy()).max():.2e} p_v {np.abs(got['p_v'] - ref['p_v'].numpy()).max():.2e} "
          f"l3 {abs(l3 / ref['l3'] - 1):.1e} ce {abs(ce / ref['ce'] - 1):.1e} kl {abs(kl / ref['kl'] - 1):.1e} dz {err / scale:.2e} of max |dz|")
    np.testing.assert_allclose(got["p_m"], ref["p_m"].numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(got["p_v"], ref["p_v"].numpy(), rtol=1e-6, atol=1e-9)
    assert l3 == pytest.approx(ref["l3"], rel=1e-7)
    assert ce == pytest.approx(ref["ce"], rel=1e-7)
    assert kl == pytest.approx(ref["kl"], rel=1e-7)
    # SVGP_KL = -|dd| / L from the kernel's own l3, ce, kl: the same three fp64 operations (the product may be fused into
    # the subtraction), so at most a few roundings of the largest operand apart; the fp32 copy is that value rounded once
    b_over_N = case["b"] / case["N"]
    dd = ce - (l3 - b_over_N * kl)
    assert np.sign(dd) == case["sign"] == np.sign(ref["dd"])
    assert abs(skl64 - (-abs(dd) / L)) <= 4 * 2.0 ** -52 * (abs(ce) + abs(l3) + abs(b_over_N * kl)) / L
    assert got["skl"].dtype == torch.float32 and float(got["skl"]) == float(np.float32(skl64))
    assert err <= 2e-6 * scale, (tag, err, scale)


@pytest.mark.parametrize("case", C.CORE_CASES, ids=C.case_id)
def test_core_matches_the_reference_at_every_geometry_edge(ops, case):
    """Values and the hand-written backward on the default path, every CORE_CASE."""
    from spadot_amd.model import svgp as sv
    assert case["m"] <= sv.SWEEP_DIRECT_M
    check_core(case, run_core(sv, case))


@pytest.mark.parametrize("case", C.HOOK_CASES, ids=C.case_id)
def test_core_matches_the_reference_in_every_backward_form(ops, case):
    """The plain backward and the restructured ones (MID_BWD, precompute_backward with and without Q1T, ELBO_LATE), each
    against the reference rather than against one another."""
    from spadot_amd.model import svgp as sv
    for form in C.HOOK_FORMS:
        check_core(case, run_core(sv, case, form), "mid %d pre %d q1t %d late %d" % form)


@pytest.mark.parametrize("case", C.LARGE_M_CASES, ids=C.case_id)
def test_core_large_m_route_on_small_matrices(ops, case):
    """m > SWEEP_DIRECT_M: spadot_svgp_pre (spadot_enc_sum_z in front when the encoder left partial products), library
    products for Sigma_l and the recursive two-block inverse -- with both thresholds lowered to 16, at m = 40 and 65."""
    from spadot_amd.model import svgp as sv
    old = sv.SWEEP_DIRECT_M, ops._SPLIT[0]
    try:
        sv.SWEEP_DIRECT_M = ops._SPLIT[0] = C.LARGE_M_SPLIT
        got = run_core(sv, case)
    finally:
        sv.SWEEP_DIRECT_M, ops._SPLIT[0] = old
    if case["parts"]:
        assert np.array_equal(got["z"], C.core_reference(case)[0]["z32"].numpy())       # z itself was stored on the way
    check_core(case, got, "large-m route")


# ------------------------------------------------------------------ (c) the three front kernels

@pytest.mark.parametrize("NP", C.FRONT_PARTS)
@pytest.mark.parametrize("b,L,m", C.FRONT_SHAPES)
def test_front_kernels_agree_bit_for_bit(lib, b, L, m, NP):
    """spadot_svgp_pre2_partials, spadot_enc_sum_z + spadot_svgp_pre2 and spadot_enc_sum_z + spadot_svgp_pre."""
    rng = np.random.default_rng(1000 * b + 10 * m + NP)
    pz = rng.normal(0, 0.5, (NP, b, 2 * L)).astype(np.float32)
    bias = rng.normal(0, 0.3, 2 * L).astype(np.float32)
    bias[L:] -= 1.0
    Kn = rng.uniform(0, 1, (b, m))
    pz_d, bias_d, Kn_d = dev(pz, torch.float32), dev(bias, torch.float32), dev(Kn)

    def buffers(with_A):
        o = {"z": Padded(b * 2 * L, torch.float32)}
        o.update({k: Padded(b * L) for k in ("mu", "var", "w", "muw")})
        if with_A:
            o["A"] = Padded(L * b * m)
        return o

    r1 = buffers(True)
    assert lib.spadot_svgp_pre2_partials(P(pz_d), NP, P(bias_d), P(Kn_d), b, L, m, P(r1["z"].t), P(r1["mu"].t), P(r1["var"].t),
                                         P(r1["w"].t), P(r1["muw"].t), P(r1["A"].t), ST()) == 0
    r2 = buffers(True)
    assert lib.spadot_enc_sum_z(P(pz_d), NP, P(bias_d), b, 2 * L, P(r2["z"].t), ST()) == 0
    assert lib.spadot_svgp_pre2(P(r2["z"].t), P(Kn_d), b, L, m, P(r2["mu"].t), P(r2["var"].t), P(r2["w"].t), P(r2["muw"].t),
                                P(r2["A"].t), ST()) == 0
    r3 = buffers(False)
    assert lib.spadot_enc_sum_z(P(pz_d), NP, P(bias_d), b, 2 * L, P(r3["z"].t), ST()) == 0
    assert lib.spadot_svgp_pre(P(r3["z"].t), b, L, P(r3["mu"].t), P(r3["var"].t), P(r3["w"].t), P(r3["muw"].t), ST()) == 0
    got = [{k: v.check(f"route {i + 1} {k}") for k, v in r.items()} for i, r in enumerate((r1, r2, r3))]

    z = C.sum_partials(pz, bias)
    a = got[0]
    assert np.array_equal(a["z"].reshape(b, 2 * L), z)
    mu, var = a["mu"].reshape(b, L), a["var"].reshape(b, L)
    assert np.array_equal(mu, z[:, :L].astype(np.float64))
    exact = np.exp(z[:, L:].astype(np.float64))
    assert (np.abs(var - exact) <= C.VAR_RTOL * exact).all(), float((np.abs(var - exact) / exact).max())
    assert np.array_equal(var, var.astype(np.float32).astype(np.float64))              # an fp32 value, as torch.exp gives
    assert np.array_equal(a["w"].reshape(b, L), 1.0 / var)
    assert np.array_equal(a["muw"].reshape(b, L), mu / var)
    assert np.array_equal(a["A"].reshape(L, b, m), Kn[None, :, :] * (1.0 / var).T[:, :, None])
    for i, other in enumerate(got[1:]):
        for k, v in other.items():
            assert np.array_equal(v, a[k]), f"route {i + 2} differs from route 1 in {k}"


def test_front_kernels_refuse_bad_arguments(lib):
    b, L, m = 3, 2, 5
    pz = torch.zeros((2, b, 2 * L), dtype=torch.float32, device=DEV)
    bias = torch.zeros(2 * L, dtype=torch.float32, device=DEV)
    Kn = torch.zeros((b, m), dtype=F64, device=DEV)
    z = torch.zeros((b, 2 * L), dtype=torch.float32, device=DEV)
    o = [torch.zeros((b, L), dtype=F64, device=DEV) for _ in range(4)]
    A = torch.zeros((L, b, m), dtype=F64, device=DEV)

    def pre2p(pz_=pz, n=2, bias_=bias, Kn_=Kn, z_=z, A_=A):
        return lib.spadot_svgp_pre2_partials(P(pz_), n, P(bias_), P(Kn_), b, L, m, P(z_), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(A_), ST())

    def sumz(pz_=pz, n=2, bias_=bias, z_=z):
        return lib.spadot_enc_sum_z(P(pz_), n, P(bias_), b, 2 * L, P(z_), ST())

    assert pre2p() == 0 and sumz() == 0
    for n in (0, C.GEOM["max_parts"] + 1):
        assert pre2p(n=n) == -22 and sumz(n=n) == -22
    for kw in ({"pz_": None}, {"bias_": None}, {"z_": None}):
        assert pre2p(**kw) == -22 and sumz(**kw) == -22
    assert pre2p(Kn_=None) == -22 and pre2p(A_=None) == -22
    assert lib.spadot_svgp_pre2(P(z), None, b, L, m, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(A), ST()) == -22
    assert lib.spadot_svgp_pre2(P(z), P(Kn), b, L, m, P(o[0]), P(o[1]), P(o[2]), P(o[3]), None, ST()) == -22


# ------------------------------------------------------------------ (d) spadot_svgp_mid

@pytest.mark.parametrize("m", C.MID_M)
def test_mid_products_row_by_row(lib, m):
    """r = S t, Mr = M r, raw = X2 r^T, sm = <S, M>: every entry within dot_bound of its own dot product (for Mr and raw
    the dot product with the kernel's own r); the rows past m of a four-row workgroup add exactly 0 to sm."""
    L, b = C.MID_L, C.MID_B
    nparts = -(-m // 4) * 4
    for rows2 in (1, 5, 2 * b):
        rng = np.random.default_rng(100 * m + rows2)
        S, t, M, X2 = rng.normal(size=(L, m, m)), rng.normal(size=(L, m)), rng.normal(size=(m, m)), rng.normal(size=(rows2, m))
        # (input margins as well: a row index one too far reads the margin's NaN instead of a neighbour's memory)
        Sd, td, Md, X2d = (Padded(a.size) for a in (S, t, M, X2))
        for buf, a in ((Sd, S), (td, t), (Md, M), (X2d, X2)):
            buf.t.copy_(torch.as_tensor(a.ravel()))
        r, Mr, raw, sm, smpart = Padded(L * m), Padded(L * m), Padded(rows2 * L), Padded(L), Padded(L * nparts)
        args = lambda n: (P(Sd.t), P(td.t), P(Md.t), P(X2d.t), L, m, rows2, P(r.t), P(Mr.t), P(raw.t), P(sm.t), P(smpart.t), n, ST())
        assert lib.spadot_svgp_mid(*args(L * nparts - 1)) == -22
        assert torch.isnan(r.full).all() and torch.isnan(sm.full).all()          # refused: nothing launched
        assert lib.spadot_svgp_mid(*args(L * nparts)) == 0
        r_, Mr_, raw_, sm_, part = (o.check(n) for o, n in ((r, "r"), (Mr, "Mr"), (raw, "raw"), (sm, "sm"), (smpart, "smpart")))
        r_, Mr_, raw_, part = r_.reshape(L, m), Mr_.reshape(L, m), raw_.reshape(rows2, L), part.reshape(L, nparts)
        assert (np.abs(r_ - np.einsum("lij,lj->li", S, t)) <= C.dot_bound(S, t[:, None, :], m)).all()
        assert (np.abs(Mr_ - np.einsum("ij,lj->li", M, r_)) <= C.dot_bound(M[None], r_[:, None, :], m)).all()
        assert (np.abs(raw_ - np.einsum("qj,lj->ql", X2, r_)) <= C.dot_bound(X2[:, None, :], r_[None], m)).all()
        rows = np.einsum("lij,ij->li", S, M)
        assert (np.abs(part[:, :m] - rows) <= C.dot_bound(S, M[None], m)).all()
        assert (part[:, m:] == 0.0).all()
        assert (np.abs(sm_ - rows.sum(1)) <= 2 * m * 2.0 ** -52 * np.abs(S * M[None]).sum((1, 2))).all()


# ------------------------------------------------------------------ (e) spadot_svgp_q1t

@pytest.mark.parametrize("b", C.Q1T_B)
def test_q1t_reduction_with_its_own_row_count(lib, b):
    """q1[l, i] = sum_n G2T[l, n] T[l, n, i]^2 + g_kl / 2 m0[l, i] with nh != b (the model only ever passes nh = b)."""
    L = C.Q1T_L
    for nh in C.Q1T_NH:
        rng = np.random.default_rng(100 * b + nh)
        Ta, Tb = rng.normal(size=(L, nh, b)), rng.normal(size=(L, nh, b))
        G2T, m0, g = rng.normal(size=(L, 2 * nh)), rng.normal(size=(L, b)), rng.normal(size=1)
        ins = [dev(a) for a in (Ta, Tb, G2T, m0, g)]
        outs = [Padded(L * b), Padded(L * b)]
        for o in outs:
            assert lib.spadot_svgp_q1t(*(P(t) for t in ins), L, nh, b, P(o.t), ST()) == 0
        q = [o.check("q1").reshape(L, b) for o in outs]
        assert np.array_equal(q[0], q[1])
        T2 = np.concatenate([Ta, Tb], axis=1) ** 2                                   # [L, 2 nh, b]
        ref = np.einsum("ln,lni->li", G2T, T2) + 0.5 * g[0] * m0
        mag = np.einsum("ln,lni->li", np.abs(G2T), T2) + np.abs(0.5 * g[0] * m0)
        # 2 nh + 1 terms; the square and the weight are two roundings a term, inside the factor 2 of the bound
        assert (np.abs(q[0] - ref) <= 2 * (2 * nh + 1) * 2.0 ** -52 * mag).all(), (nh, float((np.abs(q[0] - ref) / mag).max()))
    null = [None] * 5
    assert lib.spadot_svgp_q1t(*null, L, 3, b, P(outs[0].t), ST()) == -22


# ------------------------------------------------------------------ (f) spadot_svgp_post_forward / post_pm_pv

@pytest.mark.parametrize("b,L", C.POST_BL, ids=lambda v: str(v))
def test_post_forward_and_its_early_half(lib, b, L):
    m = C.POST_M
    rng = np.random.default_rng(b * L)
    raw, rd = rng.normal(size=(2 * b, L)), rng.uniform(0.1, 1.0, size=(L, 2 * b))
    r, Mr = rng.uniform(0.1, 1.0, size=(L, m)), rng.uniform(0.1, 1.0, size=(L, m))
    ld = np.concatenate([rng.uniform(5, 6, L), rng.uniform(0, 1, L)])
    sm = rng.uniform(0.5, 1.5, L)
    mu, var, kt = rng.normal(size=(b, L)), rng.uniform(0.3, 1.3, size=(b, L)), rng.uniform(0.0, 0.5, b)
    c, kl_const, bN = 3.7, 2.5, 0.013
    d = {k: dev(v) for k, v in dict(raw=raw, rd=rd, r=r, Mr=Mr, ld=ld, sm=sm, mu=mu, var=var, kt=kt, rd_a=rd[:, :b].copy()).items()}
    o = {k: Padded(b * L) for k in ("p_m", "mv", "p_v", "tr", "p_m2", "p_v2")}
    out4, skl32 = Padded(4), Padded(1, torch.float32)
    assert lib.spadot_svgp_post_forward(P(d["raw"]), P(d["rd"]), P(d["r"]), P(d["Mr"]), P(d["ld"]), P(d["sm"]), P(d["mu"]), P(d["var"]),
                                        P(d["kt"]), b, L, m, c, kl_const, bN, P(o["p_m"].t), P(o["mv"].t), P(o["p_v"].t), P(o["tr"].t),
                                        P(out4.t), P(skl32.t), ST()) == 0
    assert lib.spadot_svgp_post_pm_pv(P(d["raw"]), P(d["rd_a"]), P(d["kt"]), b, L, c, P(o["p_m2"].t), P(o["p_v2"].t), ST()) == 0
    g = {k: v.check(k).reshape(b, L) for k, v in o.items()}
    assert np.array_equal(g["p_m"], g["p_m2"]) and np.array_equal(g["p_v"], g["p_v2"])
    assert np.array_equal(g["p_m"], c * raw[:b]) and np.array_equal(g["p_v"], kt[:, None] + rd[:, :b].T)
    mv, tr = c * raw[b:], rd[:, b:].T
    np.testing.assert_allclose(g["mv"], mv, rtol=1e-12); np.testing.assert_allclose(g["tr"], tr, rtol=1e-12)
    LOG_2PI = 1.8378770664093453
    pm, pv = g["p_m"], g["p_v"]
    l3 = -0.5 * math.fsum(((kt[:, None] + tr) / var + np.log(var) + LOG_2PI + (mu - mv) ** 2 / var).ravel())
    ce = -0.5 * math.fsum((LOG_2PI + np.log(var) + (pv + pm * pm - 2.0 * pm * mu + mu * mu) / var).ravel())
    kl = 0.5 * (math.fsum((c * c * Mr * r).ravel()) + math.fsum(kl_const + ld[:L] - ld[L:] + sm))
    got = out4.check("out4")
    assert got[0] == pytest.approx(l3, rel=1e-12) and got[1] == pytest.approx(ce, rel=1e-12) and got[2] == pytest.approx(kl, rel=1e-12)
    assert got[3] == pytest.approx(-abs(ce - (l3 - bN * kl)) / L, rel=1e-12)
    assert float(skl32.check("skl32")[0]) == float(np.float32(got[3]))
    assert lib.spadot_svgp_post_pm_pv(None, P(d["rd_a"]), P(d["kt"]), b, L, c, P(o["p_m2"].t), P(o["p_v2"].t), ST()) == -22


# ------------------------------------------------------------------ (g) spadot_svgp_post_backward / grad_tail

def _post_bwd_reference(v, gs, G_pm, G_pv, kl0, c, bN, L):
    """torch autograd (fp64, CPU) of gs * SVGP_KL + <G_pm, p_m> + <G_pv, p_v> with SVGP_KL = -|ce - (l3 - b/N kl)| / L,
    l3 and ce as k_svgp_post_fwd writes them and kl = kl0 + sum_l c^2/2 r_l^T M r_l + 1/2 <S, M> (the two terms whose
    gradients the kernel hands on as gMr and gM)."""
    leaf = {k: torch.tensor(a, dtype=F64, requires_grad=True) for k, a in v.items() if k not in ("kt", "M")}
    kt, M = torch.tensor(v["kt"]), torch.tensor(v["M"])
    mu, var, mvv, tr, pm, pv, r, S = (leaf[k] for k in ("mu", "var", "mv", "tr", "pm", "pv", "r", "S"))
    l3 = -0.5 * ((kt[:, None] + tr) / var + torch.log(var) + 1.8378770664093453 + (mu - mvv) ** 2 / var).sum()
    ce = mo.gauss_cross_entropy(pm, pv, mu, var).sum()
    kl0 = torch.tensor(kl0, dtype=F64, requires_grad=True)
    kl = kl0 + 0.5 * c * c * ((r @ M) * r).sum() + 0.5 * (S * M).sum()
    skl = -torch.abs(ce - (l3 - bN * kl)) / L
    tot = gs * skl
    if G_pm is not None:
        tot = tot + (torch.tensor(G_pm) * pm).sum()
    if G_pv is not None:
        tot = tot + (torch.tensor(G_pv) * pv).sum()
    tot.backward()
    grads = {k: t.grad.numpy() for k, t in leaf.items()}
    grads["g_kl"] = kl0.grad.numpy().reshape(1)
    return grads, tuple(float(t.detach()) for t in (l3, ce, kl, skl))


@pytest.mark.parametrize("b,m,L", C.BWD_SHAPES)
def test_post_backward_against_autograd_with_every_null_gradient_and_sign(lib, b, m, L):
    """Every combination of present / null g_skl, G_pm, G_pv, at dd > 0, dd < 0 and dd == 0 exactly (hand-made out4 =
    (0, 0, 0, .): nothing flows through |.|, as torch.abs gives).  Tolerances: test_reduction_kernels_gradients_vs_torch's
    for the same formulas (rtol 1e-10, atol 1e-12)."""
    rng = np.random.default_rng(b + 10 * m + 100 * L)
    v = {k: rng.normal(size=(b, L)) for k in ("mu", "mv", "tr", "pm")}
    v["var"], v["pv"] = rng.uniform(0.3, 1.3, size=(b, L)), rng.uniform(0.1, 1.1, size=(b, L))
    v["kt"] = rng.uniform(0, 0.5, b)
    v["r"], v["S"] = rng.normal(size=(L, m)), rng.normal(size=(m, m))
    M = rng.normal(size=(m, m)); v["M"] = 0.5 * (M + M.T)
    G_pm, G_pv = rng.normal(size=(b, L)), rng.normal(size=(b, L))
    c, bN, gs = 2.3, 0.04, np.float32(0.7)
    Mr = v["r"] @ v["M"]
    d = {k: dev(a) for k, a in v.items()}
    d["Mr"], d["G_pm"], d["G_pv"], d["gs"] = dev(Mr), dev(G_pm), dev(G_pv), dev([gs], torch.float32)
    _, (l3, ce, _, _) = _post_bwd_reference(v, 0.0, None, None, 0.0, c, bN, L)
    kl_quad = 0.5 * c * c * float((Mr * v["r"]).sum()) + 0.5 * float((v["S"] * v["M"]).sum())
    for sign in (+1, -1, 0):
        kl0 = (sign * 5.0 - (ce - l3)) / bN - kl_quad            # dd = ce - l3 + b/N kl = 5, -5
        for use_gs in (True, False):
            for use_pm in (True, False):
                for use_pv in (True, False):
                    ref, o4 = _post_bwd_reference(v, float(gs) if use_gs else 0.0, G_pm if use_pm else None,
                                                  G_pv if use_pv else None, kl0, c, bN, L)
                    if sign == 0:
                        o4 = (0.0, 0.0, 0.0, 123.0)
                    else:
                        assert np.sign(o4[1] - (o4[0] - bN * o4[2])) == sign
                    o = {"g_mu": Padded(b * L), "g_var": Padded(b * L), "G1": Padded(2 * b * L), "G2T": Padded(2 * b * L),
                         "g_kl": Padded(1), "gMr": Padded(L * m), "gM": Padded(m * m)}
                    assert lib.spadot_svgp_post_backward(
                        P(d["gs"]) if use_gs else None, P(dev(o4)), P(d["G_pm"]) if use_pm else None, P(d["G_pv"]) if use_pv else None,
                        P(d["mu"]), P(d["var"]), P(d["mv"]), P(d["tr"]), P(d["pm"]), P(d["pv"]), P(d["kt"]), P(d["Mr"]), P(d["M"]),
                        b, L, m, c, bN, P(o["g_mu"].t), P(o["g_var"].t), P(o["G1"].t), P(o["G2T"].t), P(o["g_kl"].t), P(o["gMr"].t),
                        P(o["gM"].t), ST()) == 0
                    g = {k: t.check(k) for k, t in o.items()}
                    G1, G2T = g["G1"].reshape(2 * b, L), g["G2T"].reshape(L, 2 * b)
                    zero = np.zeros((b, L))
                    if sign == 0 or not use_gs:
                        # nothing through SVGP_KL: exactly zero, and the upstream gradients passed on untouched
                        want = {"g_mu": zero, "g_var": zero, "G1a": G_pm if use_pm else zero, "G1b": zero,
                                "G2a": G_pv if use_pv else zero, "G2b": zero, "g_kl": np.zeros(1), "gMr": np.zeros((L, m)),
                                "gM": np.zeros((m, m))}
                        tol = dict(rtol=0, atol=0)
                    else:
                        want = {"g_mu": ref["mu"], "g_var": ref["var"], "G1a": ref["pm"], "G1b": ref["mv"], "G2a": ref["pv"],
                                "G2b": ref["tr"], "g_kl": ref["g_kl"], "gMr": ref["r"], "gM": ref["S"]}
                        tol = dict(rtol=1e-10, atol=1e-12)
                    have = {"g_mu": g["g_mu"].reshape(b, L), "g_var": g["g_var"].reshape(b, L), "G1a": G1[:b], "G1b": G1[b:],
                            "G2a": G2T[:, :b].T, "G2b": G2T[:, b:].T, "g_kl": g["g_kl"], "gMr": g["gMr"].reshape(L, m),
                            "gM": g["gM"].reshape(m, m)}
                    for k in want:
                        np.testing.assert_allclose(have[k], want[k], err_msg=f"{k} sign {sign} gs {use_gs} pm {use_pm} pv {use_pv}", **tol)


@pytest.mark.parametrize("b,m,L", C.BWD_SHAPES)
def test_grad_tail_against_autograd_of_the_chain_it_closes(lib, b, m, L):
    """dw = c (g/2 (p_v - k~ - q2) - q1) + (mu - p_m) Kdt is the gradient that reaches w = 1/var (the written formula);
    from there the kernel applies the chain rule of w = 1/var, mu w and var = exp(logvar) and adds the direct g_mu, g_var:
    torch autograd of  sum (dw - mu Kdt) w + Kdt (mu w) + g_mu mu + g_var var  over (mu, logvar).  fp64 outputs at
    rtol 1e-10 (as above); dz is that rounded once to fp32 (2^-24 relative, doubled for the atol-free comparison)."""
    rng = np.random.default_rng(7 * b + m + L)
    q1, q2 = rng.normal(size=(L, b)), rng.normal(size=(L, b))
    Kdt, pv, pm, mu, g_mu, g_var = (rng.normal(size=(b, L)) for _ in range(6))
    kt, logvar, g, c = rng.uniform(0, 0.5, b), rng.normal(-1, 0.3, size=(b, L)), rng.normal(size=1), 2.3
    var = np.exp(logvar); w = 1.0 / var
    a = c * (0.5 * g[0] * (pv - kt[:, None] - q2.T) - q1.T) - pm * Kdt          # everything of dw that is not mu Kdt
    mu_t, lv_t = torch.tensor(mu, requires_grad=True), torch.tensor(logvar, requires_grad=True)
    var_t = torch.exp(lv_t); var_t.retain_grad()
    w_t = 1.0 / var_t
    (torch.tensor(a) * w_t + torch.tensor(Kdt) * (mu_t * w_t) + torch.tensor(g_mu) * mu_t + torch.tensor(g_var) * var_t).sum().backward()
    d = [dev(x) for x in (q1, q2, Kdt, pv, kt, pm, mu, w, g, g_mu, g_var)]
    dmu, dvar, dz = Padded(b * L), Padded(b * L), Padded(2 * b * L, torch.float32)
    call = lambda x, y, z_: lib.spadot_svgp_grad_tail(*(P(t) for t in d), b, L, c, x, y, z_, ST())
    assert call(None, None, None) == -22 and call(P(dmu.t), None, None) == -22 and call(None, P(dvar.t), None) == -22
    assert call(P(dmu.t), None, P(dz.t)) == -22 and call(None, P(dvar.t), P(dz.t)) == -22      # half of the fp64 pair: the kernel writes both
    assert torch.isnan(dz.full).all()
    assert torch.isnan(dmu.full).all() and torch.isnan(dvar.full).all()
    assert call(None, None, P(dz.t)) == 0
    assert torch.isnan(dmu.full).all() and torch.isnan(dvar.full).all()          # dz only: the fp64 pair stays untouched
    got_z = dz.check("dz").reshape(b, 2 * L).astype(np.float64)
    assert call(P(dmu.t), P(dvar.t), None) == 0
    np.testing.assert_allclose(dmu.check("dmu").reshape(b, L), mu_t.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(dvar.check("dvar").reshape(b, L), var_t.grad.numpy(), rtol=1e-10, atol=1e-12)
    want_z = np.concatenate([mu_t.grad.numpy(), lv_t.grad.numpy()], axis=1)
    np.testing.assert_allclose(got_z, want_z, rtol=2.0 ** -23, atol=1e-12)


# ------------------------------------------------------------------ (h) spadot_spd_inverse_logdet2

@pytest.mark.parametrize("m", C.SWEEP_M)
def test_sweep_adds_its_terms_while_it_loads(lib, m):
    """Matrix l = A[l mod Lsrc] + add0 (+ add1 for l >= Lsrc) against torch.linalg on the same matrices built on the
    host side, by test_spd_inverse_logdet_vs_torch's criteria and conditioning: B B^T 50 + 1e-2 I (split between A and
    add0), add1 a PSD term of K^2 / j's size.  m up to 310: the tile widths 1 .. 10, which ops.spd_inverse_logdet (split
    at 279) no longer reaches above 9."""
    rng = np.random.default_rng(m)
    k = max(2, m // 3)
    eye = torch.eye(m, dtype=F64, device=DEV)
    jit = 1e-2 * np.eye(m)
    B0, C1 = rng.normal(size=(m, k)), rng.normal(size=(m, k))
    add0_full = dev(B0 @ B0.T * 25.0 + jit)
    add1_full = dev(C1 @ C1.T * 100.0)
    for Lsrc, L in C.SWEEP_BATCH:
        nsrc = Lsrc if Lsrc else L
        Bs = rng.normal(size=(nsrc, m, k))
        low = Bs @ Bs.transpose(0, 2, 1) * 25.0
        forms = (("both", low, add0_full, add1_full), ("add1 null", low, add0_full, None), ("both null", low * 2.0 + jit, None, None))
        for name, A_np, add0, add1 in (forms if Lsrc else forms[2:]):
            A = dev(A_np)
            idx = torch.arange(L, device=DEV) % nsrc
            full = A[idx].clone()
            if add0 is not None:
                full += add0
            if add1 is not None:
                full[Lsrc:] += add1
            X, ld = Padded(L * m * m, pad=1024), Padded(L)
            assert lib.spadot_spd_inverse_logdet2(P(A), Lsrc, L, m, P(add0), P(add1), P(X.t), P(ld.t), ST()) == 0
            Xg = torch.as_tensor(X.check(f"X {name}")).reshape(L, m, m).to(DEV)
            Xr, ldr = torch.linalg.inv(full), torch.linalg.slogdet(full)[1]
            res = float((full @ Xg - eye).abs().max())
            res_ref = float((full @ Xr - eye).abs().max())
            assert res <= 10 * res_ref + 1e-12, (name, Lsrc, L, res, res_ref)
            np.testing.assert_allclose(ld.check("logdet"), host(ldr), rtol=1e-9, atol=1e-7, err_msg=f"{name} {Lsrc} {L}")
            np.testing.assert_allclose(host(Xg), host(Xr), rtol=1e-6, atol=1e-7 * float(Xr.abs().max()), err_msg=f"{name} {Lsrc} {L}")
            if add1 is not None:
                # the first Lsrc outputs are the inverses of A + add0 alone
                plain = torch.linalg.inv(A + add0)
                np.testing.assert_allclose(host(Xg[:Lsrc]), host(plain), rtol=1e-6, atol=1e-7 * float(plain.abs().max()))
                nhi = min(Lsrc, L - Lsrc)                                          # ... and the next ones are not
                assert float((Xg[Lsrc:Lsrc + nhi] - plain[:nhi]).abs().max()) > 1e-3 * float(plain.abs().max())


def test_sweep_refuses_what_it_cannot_hold(lib):
    A = torch.eye(4, dtype=F64, device=DEV).repeat(3, 1, 1).contiguous()
    X, ld = torch.empty_like(A), torch.empty(3, dtype=F64, device=DEV)
    assert lib.spadot_spd_inverse_logdet2(P(A), 4, 3, 4, None, None, P(X), P(ld), ST()) == -22       # Lsrc > L
    assert lib.spadot_spd_inverse_logdet2(P(A), -1, 3, 4, None, None, P(X), P(ld), ST()) == -22
    assert lib.spadot_spd_inverse_logdet2(P(A), 0, 0, 4, None, None, P(X), P(ld), ST()) == -22
    big = C.GEOM["sweep_max_m"] + 1
    assert lib.spadot_spd_inverse_logdet2(P(A), 0, 1, big, None, None, P(X), P(ld), ST()) == -34    # (refused before any launch)
    assert lib.spadot_spd_inverse_logdet2(P(A), 3, 3, 4, None, None, P(X), P(ld), ST()) == 0
    torch.cuda.synchronize()
    assert torch.equal(X, A) and torch.equal(ld, torch.zeros_like(ld))


# ------------------------------------------------------------------ (i) kernel matrix slabs

@pytest.mark.parametrize("d", C.KMAT_D)
@pytest.mark.parametrize("n", C.KMAT_N)
def test_kernel_matrix_across_row_slabs(ops, n, d):
    """K(x, z) goes out in slabs of 65535 rows (gridDim.y): one slab exactly, one row into the second, two rows into it."""
    rng = np.random.default_rng(n + d)
    x, z = torch.as_tensor(rng.uniform(0, 1, (n, d))), torch.as_tensor(rng.uniform(0, 1, (3, d)))
    slab = C.GEOM["kmat_slab"]
    rows = sorted({0, slab - 1, min(slab, n - 1), n - 1})
    for kt in ("Gaussian", "Cauchy", "Quadratic"):
        K = host(ops.kernel_matrix(x.to(DEV), z.to(DEV), kt, 0.1))
        ref = mo.rbf_kernel(x, z, kt, 0.1).numpy()
        assert K.shape == (n, 3)
        np.testing.assert_allclose(K[rows], ref[rows], rtol=1e-12, atol=1e-15, err_msg=f"{kt} rows {rows}")
        np.testing.assert_allclose(K, ref, rtol=1e-12, atol=1e-15, err_msg=kt)
    K32 = host(ops.kernel_matrix(x.float().to(DEV), z.float().to(DEV), "Gaussian", 0.1))
    ref = mo.rbf_kernel(x, z, "Gaussian", 0.1).numpy()
    assert K32.dtype == np.float32
    np.testing.assert_allclose(K32[rows], ref[rows], rtol=2e-5, atol=1e-7, err_msg=f"fp32 rows {rows}")
    np.testing.assert_allclose(K32, ref, rtol=2e-5, atol=1e-7)
