"""Case tables and the fp64 reference for the edge tests of the SVGP branch (spadot_amd/model/svgp.py:_SVGPCore and, in
csrc/model_kernels.hip / enc_fused.hip, k_svgp_pre / pre2 / pre2p / mid1 / mid2 / post_fwd / post_pmpv / post_bwd / q1t /
grad_tail, k_enc_sum_z and the add-on-load form of k_spd_sweep).

Nothing here touches the GPU.  tests/test_svgp_ref_cpu.py checks the reference (golden values, finite differences, its own
conditioning) and that every case reaches the branch it records, from the geometry constants below and the case's shape
alone; tests/test_svgp_edges_gpu.py runs the cases on the device.

The reference is oracle.model_oracle.SVGPOracle -- the reference implementation's arithmetic, one latent dimension at a
time, with the literal (b, m, m) tensor -- under torch autograd: it shares neither the device's algebra (Sylvester form,
<S, M>, the T = X2 S K_mn route) nor its hand-derived backward."""
import functools

import numpy as np
import torch

from oracle import model_oracle as mo

F64 = torch.float64

# Launch geometry the cases assume (model_kernels.hip, enc_fused.hip).  A change there has to be made here as well: the CPU
# test then says which cases no longer reach their branch.
GEOM = {
    "row_wg": 256,             # threads of a wave-per-row workgroup (pre2, pre2p, mid1, mid2)
    "rows_per_wg": 4,          # ... one wave (64 lanes) per row
    "lane_stride": 64,         # a row's wave strides m in steps of 64
    "q1t_tile": 16,            # k_svgp_q1t: 16 columns x 16 row slices per workgroup
    "post_fwd_threads": 1024,  # k_svgp_post_fwd: ONE workgroup striding b * L ...
    "post_fwd_unroll": 5,      # ... with #pragma unroll 5
    "flat_wg": 256,            # threads of the flat grids (pre, post_pmpv, post_bwd, grad_tail, enc_sum_z)
    "max_parts": 64,           # partials a front kernel takes: one lane of the row's wave each
    "sweep_grid": 31,          # k_spd_sweep: T <= 31 tiles per edge (T (T + 1) / 2 <= 512 threads), TS = ceil(m / 31)
    "sweep_core": 9,           # SWEEP_RS: tile edge kept in registers; a wider tile keeps its border in LDS
    "sweep_max_m": 310,        # TS <= 10: the entry refuses m above
    "kmat_slab": 65535,        # rows of K(x, z) per launch (gridDim.y)
}

G_SKL = 0.7                    # d loss / d SVGP_KL of the backward seed (the existing forms-agree test's)
ALL, PV_SKL, SKL, PM = ("pm", "pv", "skl"), ("pv", "skl"), ("skl",), ("pm",)


def _case(b, m, L, N, grads, sign, grid, why, parts=0):
    """grid: which of b*L / L*m / m*m sizes k_svgp_post_bwd's grid ("tie": all equal); sign: of dd = ce - (l3 - b/N kl);
    parts: z reaches the branch as that many partial products plus a bias (0: as z itself)."""
    return {"b": b, "m": m, "L": L, "N": float(N), "grads": grads, "sign": sign, "grid": grid, "why": why, "parts": parts}


# Inputs are drawn as in test_svgp_backward_precomputed_and_restructured_forms_agree (core_inputs, seed 7).  The signs
# were read off the reference on the CPU and are asserted from it in test_svgp_ref_cpu.py.
CORE_CASES = [
    _case(1, 1, 1, 5000, ALL, +1, "tie", "every loop runs exactly once"),
    _case(2, 3, 5, 5000, ALL, +1, "Lm", "L > m > b: L*m sizes the post_bwd grid"),
    _case(67, 129, 2, 5000, ALL, +1, "mm", "m*m largest, b < m; m crosses two 64-lane strides, m % 4 = 1"),
    _case(205, 9, 5, 5000, ALL, +1, "bL", "b*L = 1025: second trip of post_fwd's stride, remainder of its unroll"),
    _case(256, 11, 4, 5000, ALL, +1, "bL", "b*L = 1024 exactly: one full trip of post_fwd, no second"),
    _case(257, 6, 1, 5000, ALL, +1, "bL", "b*L = 257: second workgroup of the 256-thread kernels, L = 1"),
    _case(19, 63, 1, 5000, ALL, +1, "mm", "m = 63: one short trip over m; partial q1t tile"),
    _case(37, 64, 3, 5000, ALL, +1, "mm", "m = 64: exactly one trip over m"),
    _case(70, 65, 2, 37, ALL, -1, "mm", "m = 65: one lane in the second trip; dd < 0"),
    _case(37, 17, 3, 5000, ALL, +1, "mm", "ordinary point"),
    _case(130, 100, 2, 5000, ALL, +1, "mm", "ordinary point"),
    _case(130, 100, 2, 60, ALL, -1, "mm", "ordinary point, dd < 0"),
    # gradient subsets: G_pm / G_pv / g_skl reach the kernels as null pointers
    _case(37, 17, 3, 5000, PV_SKL, +1, "mm", "G_pm null"),
    _case(37, 17, 3, 5000, SKL, +1, "mm", "G_pm and G_pv null"),
    _case(37, 17, 3, 5000, PM, +1, "mm", "g_skl and G_pv null"),
    _case(70, 65, 2, 37, PV_SKL, -1, "mm", "G_pm null, dd < 0"),
    _case(70, 65, 2, 37, SKL, -1, "mm", "G_pm and G_pv null, dd < 0"),
    _case(70, 65, 2, 37, PM, -1, "mm", "g_skl and G_pv null, dd < 0"),
]
# the shapes that also run every backward form (MID_BWD, precompute_backward, Q1T, ELBO_LATE)
HOOK_CASES = [c for c in CORE_CASES if c["grads"] == ALL and (c["b"], c["m"], c["L"], c["N"]) in
              {(37, 17, 3, 5000.0), (70, 65, 2, 37.0), (67, 129, 2, 5000.0)}]
# the large-m route of _SVGPCore.start at small m (SWEEP_DIRECT_M and ops._SPLIT lowered to LARGE_M_SPLIT)
LARGE_M_SPLIT = 16
LARGE_M_CASES = [_case(37, 40, 3, 5000, ALL, +1, "mm", "two levels of the two-block elimination"),
                 _case(70, 65, 2, 37, ALL, -1, "mm", "odd m: uneven blocks; dd < 0"),
                 _case(37, 40, 3, 5000, ALL, +1, "mm", "spadot_enc_sum_z in front", parts=3),
                 _case(70, 65, 2, 37, ALL, -1, "mm", "spadot_enc_sum_z in front; dd < 0", parts=3)]
# (mid, pre, q1t, late) as in the forms-agree test, the plain form first
HOOK_FORMS = [(False, False, False, False), (True, False, False, False), (True, True, False, False), (True, True, True, False),
              (False, True, True, False), (True, True, True, True), (True, False, False, True)]


def case_id(c):
    return "%dx%dx%d-N%g-%s%s" % (c["b"], c["m"], c["L"], c["N"], "+".join(c["grads"]), "-p%d" % c["parts"] if c.get("parts") else "")


def sum_partials(pz, bias):
    """z = bias + sum_g pz[g] as the front kernels form it: fp32, g ascending from 0, the bias last."""
    acc = np.zeros(pz.shape[1:], dtype=np.float32)
    for g in range(pz.shape[0]):
        acc = acc + pz[g]
    return acc + bias[None, :]


def core_inputs(case):
    """Inducing points and coordinates uniform on [0, 1]^2, mu ~ N(0, 1), logvar ~ N(-1, 0.3) as fp32 z = (mu | logvar),
    upstream gradients ~ N(0, 1); seed 7.  Gradients the case leaves out are None.  With parts, z is cut into that many
    fp32 partial products pz [parts, b, 2L] and a bias, and z32 is their sum in the kernels' order."""
    b, m, L = case["b"], case["m"], case["L"]
    rng = np.random.default_rng(7)
    inducing = rng.uniform(0, 1, (m, 2))
    x = torch.as_tensor(rng.uniform(0, 1, (b, 2)), dtype=F64)
    z32 = torch.as_tensor(np.concatenate([rng.normal(0, 1, (b, L)), rng.normal(-1, 0.3, (b, L))], 1), dtype=torch.float32)
    gpm, gpv = (torch.as_tensor(rng.normal(0, 1, (b, L)), dtype=F64) for _ in range(2))
    g = case["grads"]
    extra = {}
    if case.get("parts"):
        NP = case["parts"]
        bias = rng.normal(0, 0.1, 2 * L).astype(np.float32)
        pz = ((z32.numpy() - bias[None, :])[None] / NP + rng.normal(0, 0.05, (NP, b, 2 * L))).astype(np.float32)
        z32 = torch.from_numpy(sum_partials(pz, bias))
        extra = {"pz": torch.from_numpy(pz), "bias": torch.from_numpy(bias)}
    return {**extra, "inducing": inducing, "x": x, "z32": z32, "N": case["N"], "G_pm": gpm if "pm" in g else None,
            "G_pv": gpv if "pv" in g else None, "g_skl": torch.tensor(G_SKL, dtype=F64) if "skl" in g else None}


def svgp_core_ref(inducing, x, z32, N_train, G_pm, G_pv, g_skl, fp64_z=False, var32=None):
    """What _SVGPCore computes, from the reference's arithmetic (SVGPOracle per latent dimension) in fp64 on the CPU:
    p_m, p_v [b, L], l3, ce, kl, SVGP_KL = -|dd| / L with dd = ce - (l3 - b/N kl), and dz = the gradient of
    <G_pm, p_m> + <G_pv, p_v> + g_skl SVGP_KL w.r.t. z (None where every gradient is None).
    z = (mu | logvar) is fp32 and exp(logvar) is taken in fp32, as on the device; fp64_z: z and the exponential in fp64
    (the smooth function that finite differences and the golden values are compared with).
    var32 [b, L]: the VALUES of the fp32 exponential to use instead of this CPU's (d var / d logvar = var as before).  Two
    correct fp32 exponentials may differ in the last bit -- this CPU's own differs from the correctly rounded one on 11 of
    the 1025 entries of the (205, 9, 5) case -- and one such bit on a tenth of the entries moves p_m there by 1.95e-8: twelve
    entries near zero then miss rtol 1e-6 / atol 1e-9.  The GPU test therefore checks the device's var against the fp64
    exponential on its own (VAR_RTOL) and hands it in here, so that everything behind it is compared on the same var."""
    z = torch.as_tensor(z32).detach().clone().to(F64 if fp64_z else torch.float32).requires_grad_(True)
    x = torch.as_tensor(x, dtype=F64)
    b, L = z.shape[0], z.shape[1] // 2
    e = torch.exp(z[:, L:])
    if var32 is not None:
        assert not fp64_z
        e = torch.as_tensor(var32, dtype=torch.float32) * (e / e.detach())        # (x / x = 1 exactly: the given values, exp's slope)
    mu, var = z[:, :L].double(), e.double()
    orc = mo.SVGPOracle(inducing, N_train)
    pm, pv, l3s, kls = [], [], [], []
    for l in range(L):
        m_l, v_l, mu_hat, A_hat = orc.approximate_posterior_params(x, x, mu[:, l], var[:, l])
        l3_l, kl_l = orc.variational_loss(x, mu[:, l], var[:, l], mu_hat, A_hat)
        pm.append(m_l); pv.append(v_l); l3s.append(l3_l); kls.append(kl_l)
    p_m, p_v = torch.stack(pm, dim=1), torch.stack(pv, dim=1)
    l3, kl = torch.stack(l3s).sum(), torch.stack(kls).sum()
    ce = mo.gauss_cross_entropy(p_m, p_v, mu, var).sum()
    dd = ce - (l3 - (b / float(N_train)) * kl)
    skl = -torch.abs(dd) / L
    outs = [(o, g) for o, g in ((p_m, G_pm), (p_v, G_pv), (skl, g_skl)) if g is not None]
    dz = None
    if outs:
        (dz,) = torch.autograd.grad([o for o, _ in outs], [z], [torch.as_tensor(g, dtype=F64) for _, g in outs])
    return {"p_m": p_m.detach(), "p_v": p_v.detach(), "l3": float(l3.detach()), "ce": float(ce.detach()),
            "kl": float(kl.detach()), "skl": float(skl.detach()), "dd": float(dd.detach()), "dz": dz}


@functools.lru_cache(maxsize=None)
def _core_reference(b, m, L, N, grads, parts):
    case = {"b": b, "m": m, "L": L, "N": N, "grads": grads, "parts": parts}
    inp = core_inputs(case)
    return inp, svgp_core_ref(inp["inducing"], inp["x"], inp["z32"], inp["N"], inp["G_pm"], inp["G_pv"], inp["g_skl"])


def core_reference(case):
    """(inputs, reference) of a case, computed once per process and shared: treat both as read-only."""
    return _core_reference(case["b"], case["m"], case["L"], case["N"], case["grads"], case.get("parts", 0))


# ----------------------------------------------------------------------------------------------- the entries called directly
def dot_bound(A, B, m):
    """Bound on the error of an m-term fp64 dot product sum_k A[.., k] B[.., k] accumulated in any order, fused or not:
    2 m 2^-52 sum |a| |b| (gamma_m = m u / (1 - m u) with u = 2^-53, doubled)."""
    return 2.0 * m * 2.0 ** -52 * np.sum(np.abs(A) * np.abs(B), axis=-1)


FRONT_SHAPES = [(1, 1, 1), (5, 3, 65), (37, 10, 17)]               # (b, L, m)
FRONT_PARTS = [1, 2, 32, 64]
VAR_RTOL = 2.0 ** -22          # expf within one ulp (2^-23) plus the rounding of its result (2^-24), rounded up

MID_M = [1, 3, 63, 64, 65, 129]
MID_B = 7                      # rows2 in {1, 5, 2 * MID_B}
MID_L = 3

Q1T_B = [1, 15, 16, 17, 33]
Q1T_NH = [1, 16, 17, 40]
Q1T_L = 2

POST_BL = [(1, 1), (51, 5), (64, 4), (257, 1), (256, 4), (205, 5)]   # (b, L): b*L = 1, 255, 256, 257, 1024, 1025
POST_M = 9

# (b, m, L) of post_backward / grad_tail called directly: b*L, L*m and m*m largest in turn
BWD_SHAPES = [(300, 5, 2), (3, 7, 9), (5, 40, 2)]

SWEEP_M = [1, 31, 32, 62, 63, 217, 248, 249, 279, 280, 310]
SWEEP_BATCH = [(3, 6), (2, 5), (0, 3)]                               # (Lsrc, L)

KMAT_N = [65535, 65536, 65537]
KMAT_D = [1, 2, 3]
