"""Case tables and fp64 references for the edge tests of the training step's tail kernels (csrc/model_kernels.hip):
gradient norm, clip + AdamW, BatchNorm / LayerNorm + LeakyReLU, the latent head and the K-means / OT cluster losses.

Nothing here touches the GPU.  tests/test_step_tail_ref_cpu.py checks the references against torch in fp64 and checks
that every case reaches the branch it records, from the geometry constants below and the case's shape alone;
tests/test_step_tail_edges_gpu.py runs the cases on the device.

A tolerance that had to be measured stands next to its case with the number it came from; every other tolerance is
the one the default-shape tests in tests/test_model_gpu.py already use."""
import math

import numpy as np
import torch

from oracle import model_oracle as mo

# Launch geometry the cases assume (model_kernels.hip).  A change there has to be made here as well: the CPU test
# then says which cases no longer reach their branch.
GEOM = {
    "wg": 256,                 # threads of a streaming workgroup (norm, update)
    "sumsq_unroll": 4,         # k_sumsq_part_u<4>: float4 loads in flight per thread and trip
    "sumsq_cap": 2048,         # workgroups of the norm's partial pass, at most
    "final_sum_threads": 1024,  # k_final_sum_step: one workgroup, strided over the partials
    "adamw_cap": 4096,         # workgroups of step()'s update (k_adamw: 1 element, k_adamw_img: 4 elements per thread)
    "range_cap": 512,          # workgroups of spadot_adamw_range_dev (step_head / step_rest)
    "bn_rows": 512,            # BN_RG * BN_RPT: rows of the BatchNorm register path
    "bn_cols": 16,             # columns per BatchNorm / LayerNorm-column workgroup
    "bn_rg": 16,               # row lanes of a BatchNorm workgroup
    "ln_rg": 64,               # row lanes of the LayerNorm column pass
    "ln_rows_per_wg": 4,       # one wave (64 lanes) per row
    "head_rows_per_wg": 8,     # latent head: 32 lanes per row
    "head_sum_stride": 256,    # the last workgroup's stride over the partials
    "cl_threads": 512,         # cluster losses: one 512-thread workgroup
    "cl_chunk_floats": 10240,  # latent values staged per chunk
    "cl_min_chunk": 64,        # CL_MAXK rows at least
    "cl_zb": 20,               # latent values per thread the first chunk brings in registers
    "cl_kreg": 16,             # CL_KREG: most clusters on the fast path
    "cl_maxk": 64,
}


# ----------------------------------------------------------------------------------------------- gradient norm
# count -> what of k_sumsq_part_u<4> / k_final_sum_step it reaches:
#   n4 float4 groups over `wgs` workgroups, `tail` scalar elements in workgroup 0, `lanes` = unroll lanes u that see
#   data, `trips` of the k loop, `final_trips` of the one-workgroup sum over the partials.
_FULL = 4 * 256 * 2048
SUMSQ_CASES = [
    {"count": 1, "wgs": 1, "n4": 0, "tail": 1, "lanes": 0, "trips": 0, "final_trips": 1},
    {"count": 3, "wgs": 1, "n4": 0, "tail": 3, "lanes": 0, "trips": 0, "final_trips": 1},
    {"count": 5, "wgs": 1, "n4": 1, "tail": 1, "lanes": 1, "trips": 1, "final_trips": 1},
    {"count": 1023, "wgs": 1, "n4": 255, "tail": 3, "lanes": 1, "trips": 1, "final_trips": 1},
    {"count": 1027, "wgs": 1, "n4": 256, "tail": 3, "lanes": 1, "trips": 1, "final_trips": 1},
    {"count": _FULL + 4 + 3, "wgs": 2048, "n4": 524289, "tail": 3, "lanes": 2, "trips": 1, "final_trips": 2},
    {"count": 4 * _FULL + 1028 + 2, "wgs": 2048, "n4": 2097409, "tail": 2, "lanes": 4, "trips": 2, "final_trips": 2},
]


def sumsq_values(count):
    """fp32 gradient values with a 1e4 dynamic range and mixed sign."""
    rng = np.random.default_rng(count)
    mag = np.power(10.0, rng.uniform(-2.0, 2.0, size=count))
    return (mag * rng.choice([-1.0, 1.0], size=count)).astype(np.float32)


def sumsq_ref(g):
    return float(np.sum(g.astype(np.float64) ** 2))


# The kernels add in fp64 and round once to fp32: half an ulp (2**-24 relative), doubled for the fp64 ordering noise.
SUMSQ_RTOL = 2.0 ** -23


# ----------------------------------------------------------------------------------------------- clip + AdamW
def clip_adamw_ref(p, g, m, v, t, lr, betas, eps, wd, max_norm, grad_scale=1.0):
    """One clip_grad_norm_(max_norm) + AdamW step in numpy fp64: the arithmetic of adamw_clip_coef + adamw_element.
    p, g, m, v: arrays or lists of arrays (one global norm over all of g); g stands for grad_scale * gradient.
    t: the step count of THIS step (1 for the first).  Returns (p, m, v, sumsq) -- new arrays, inputs untouched."""
    single = isinstance(p, np.ndarray)
    ps, gs_, ms, vs = ([np.asarray(a, dtype=np.float64) for a in ([x] if single else x)] for x in (p, g, m, v))
    b1, b2 = betas
    sumsq = math.fsum(float(np.sum(a * a)) for a in gs_)
    total = math.sqrt(sumsq) * grad_scale
    coef = min(1.0, max_norm / (total + 1e-6)) * grad_scale
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    po, mo_, vo = [], [], []
    for pp, gg, mm, vv in zip(ps, gs_, ms, vs):
        gg = gg * coef
        pn = pp * (1.0 - lr * wd)                                  # decoupled decay
        mn = mm + (gg - mm) * (1.0 - b1)                           # lerp_(grad, 1 - beta1)
        vn = vv * b2 + gg * gg * (1.0 - b2)
        denom = np.sqrt(vn) / math.sqrt(bc2) + eps
        pn = pn - (lr / bc1) * (mn / denom)
        po.append(pn); mo_.append(mn); vo.append(vn)
    if single:
        return po[0], mo_[0], vo[0], sumsq
    return po, mo_, vo, sumsq


# 8 397 836 elements with padding.  More than 4 * 256 * 4 * 2048 (second trip of the norm's k loop), more than
# 4096 * 256 * 4 (k_adamw_img grid-strides under step(); k_adamw, one element per thread, all the more), and every
# range of step_head() / step_rest() is more than 512 * 256 * 4.
ADAMW_CASE = {
    "shapes": [(2048, 2052), (1024, 1024), (3,), (1031,), (2048, 1536)],
    "padded": 8397836,
    "images": {4: 1568, 1: 1024},          # parameter index -> Kp of its bf16 image (1568 > K = 1536: pad columns)
    "first": [1], "last": [0],
    "head_count": 1024 * 1024,
    "lr": 3e-4, "betas": (0.9, 0.999), "eps": 1e-8, "wd": 1e-2, "max_norm": 0.3,      # FlatAdamW's defaults
    "step0": 20000,                        # bias corrections near 1: what a long run sees
    # sigma of the gradient entries (the norm is ~2898 sigma) and grad_scale of the three steps
    "steps": [{"sigma": 1e-2, "grad_scale": 1.0, "clipped": True},
              {"sigma": 1e-5, "grad_scale": 1.0, "clipped": False},
              {"sigma": 4e-2, "grad_scale": 0.25, "clipped": True}],
    "sumsq_trips": 2, "img_strides": True, "range_strides": True,
    # parameters against clip_adamw_ref: the default-shape test's bound
    "rtol": 2e-6, "atol": 1e-7,
    # moments (not checked by the default-shape test), from the number formats: a handful of fp32 roundings per step,
    # 3 steps -- 2e-6 relative -- plus what the kernels' fp32 betas cost: beta rounds to fp32 with an error of up to
    # 2**-25, which is 2**-25 / (1 - beta) of the weight (1 - beta) the new gradient gets.  (fp32(0.999) = 0.99900001...:
    # the second moment sits 1.3e-5 below the fp64 reference's.)  The lerp's difference (g - m) can cancel, so the
    # absolute part is the same fraction of the largest entry.
    "m_rtol": 2e-6 + 2.0 ** -25 / 0.1, "v_rtol": 2e-6 + 2.0 ** -25 / 0.001,
}


def adamw_params(case):
    rng = np.random.default_rng(11)
    return [rng.standard_normal(s, dtype=np.float32) for s in case["shapes"]]


def adamw_grads(case, step):
    rng = np.random.default_rng(100 + step)
    sigma = np.float32(case["steps"][step]["sigma"])
    return [rng.standard_normal(s, dtype=np.float32) * sigma for s in case["shapes"]]


# ----------------------------------------------------------------------------------------------- BatchNorm + LeakyReLU
# (b, F, dtype of x, Linear bias or None).  path: "register" (b <= 512) or "looped"; wgs = ceil(F / 16).
# Tolerances: those of test_bn_act_matches_batchnorm_leakyrelu (y rtol 2e-4 / atol 2e-5, running statistics rtol 1e-5 /
# atol 1e-6, gradients 2e-4, bf16: 2e-2, of the largest entry) unless a case carries its own.
BN_CASES = [
    {"b": 513, "F": 70, "dtype": "float32", "bias": True, "path": "looped", "wgs": 5, "idle_cols": 10},
    {"b": 1300, "F": 256, "dtype": "bfloat16", "bias": True, "path": "looped", "wgs": 16, "idle_cols": 0},
    {"b": 2048, "F": 17, "dtype": "float32", "bias": False, "path": "looped", "wgs": 2, "idle_cols": 15},
    # two rows: 14 of the 16 row lanes idle; x_hat = +-1, so dx cancels to ~eps / var of dz
    {"b": 2, "F": 16, "dtype": "float32", "bias": True, "path": "register", "wgs": 1, "idle_cols": 0},
    {"b": 600, "F": 1, "dtype": "float32", "bias": True, "path": "looped", "wgs": 1, "idle_cols": 15},
]


def bn_inputs(case):
    """x (already rounded to the case's dtype), Linear bias, the weights of the backward seed, gamma, beta -- fp64 tensors."""
    b, F = case["b"], case["F"]
    rng = np.random.default_rng(7 * b + F)
    x = torch.as_tensor(rng.normal(size=(b, F)) * 2 + 0.5).to(getattr(torch, case["dtype"])).double()
    lb = torch.as_tensor(rng.normal(size=F))
    w = torch.as_tensor(rng.normal(size=(b, F)))
    gamma = torch.as_tensor(rng.normal(size=F) * 0.5 + 1).float().double()
    beta = torch.as_tensor(rng.normal(size=F) * 0.3).float().double()
    return x, (lb if case["bias"] else None), w, gamma, beta


def bn_reference(case, dtype=torch.float64):
    """leaky_relu(BatchNorm1d(x + bias)) in training mode on the CPU: y, running mean / variance, counter, dx, dgamma, dbeta."""
    x, lb, w, gamma, beta = bn_inputs(case)
    bn = torch.nn.BatchNorm1d(case["F"]).to(dtype)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    xr = x.to(dtype).requires_grad_(True)
    y = torch.nn.functional.leaky_relu(bn(xr if lb is None else xr + lb.to(dtype)), 0.01)
    (y * w.to(dtype)).sum().backward()
    return {"y": y.detach(), "running_mean": bn.running_mean, "running_var": bn.running_var,
            "count": int(bn.num_batches_tracked), "dx": xr.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad}


# ----------------------------------------------------------------------------------------------- LayerNorm + LeakyReLU
# (b, F).  row_wgs = ceil(b / 4) with `last_rows` rows in the last one; idle_lanes of the row's wave; the column pass
# makes col_trips = ceil(b / 64) trips in col_wgs = ceil(F / 16) workgroups, `ragged` = F % 16 live columns in the last.
LN_CASES = [
    {"b": 5, "F": 17, "row_wgs": 2, "last_rows": 1, "idle_lanes": 47, "col_trips": 1, "col_wgs": 2, "ragged": 1},
    {"b": 7, "F": 33, "row_wgs": 2, "last_rows": 3, "idle_lanes": 31, "col_trips": 1, "col_wgs": 3, "ragged": 1},
    {"b": 1030, "F": 257, "row_wgs": 258, "last_rows": 2, "idle_lanes": 0, "col_trips": 17, "col_wgs": 17, "ragged": 1},
    {"b": 130, "F": 1, "row_wgs": 33, "last_rows": 2, "idle_lanes": 63, "col_trips": 3, "col_wgs": 1, "ragged": 1},
]


def ln_inputs(case):
    b, F = case["b"], case["F"]
    rng = np.random.default_rng(3 * b + F)
    x = torch.as_tensor(rng.normal(size=(b, F)) * 1.5 - 0.2).float().double()
    w = torch.as_tensor(rng.normal(size=(b, F)))
    gamma = torch.as_tensor(rng.normal(size=F) * 0.5 + 1).float().double()
    beta = torch.as_tensor(rng.normal(size=F) * 0.3).float().double()
    return x, w, gamma, beta


def ln_reference(case, dtype=torch.float64):
    x, w, gamma, beta = ln_inputs(case)
    ln = torch.nn.LayerNorm(case["F"]).to(dtype)
    with torch.no_grad():
        ln.weight.copy_(gamma); ln.bias.copy_(beta)
    xr = x.to(dtype).requires_grad_(True)
    y = torch.nn.functional.leaky_relu(ln(xr), 0.01)
    (y * w.to(dtype)).sum().backward()
    return {"y": y.detach(), "dx": xr.grad, "dgamma": ln.weight.grad, "dbeta": ln.bias.grad}


# ----------------------------------------------------------------------------------------------- latent head
# (b, Ls, Lg).  wgs = ceil(b / 8); sum_trips = ceil(wgs / 256) of the last workgroup's loop over the partials.
HEAD_CASES = [
    {"b": 8, "Ls": 16, "Lg": 16, "wgs": 1, "sum_trips": 1, "lanes": 32},           # the full half wave
    {"b": 9, "Ls": 22, "Lg": 10, "wgs": 2, "sum_trips": 1, "lanes": 32},           # Ls > Lg, one row in the last workgroup
    {"b": 1, "Ls": 1, "Lg": 1, "wgs": 1, "sum_trips": 1, "lanes": 2},
    {"b": 2049, "Ls": 10, "Lg": 10, "wgs": 257, "sum_trips": 2, "lanes": 20},
]
HEAD_WEIGHTS = (0.37, -1.3)          # d loss / d GAT_KL, d loss / d alignment of the backward seed


def head_inputs(b, Ls, Lg, seed=None):
    rng = np.random.default_rng(b if seed is None else seed)
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    zg = T(rng.normal(size=(b, 2 * Lg)) * 0.7); p_m = T(rng.normal(size=(b, Ls))); p_v = T(rng.uniform(0.05, 2.0, size=(b, Ls)))
    eps = T(rng.normal(size=(b, Ls + Lg))).float().double()            # the op takes fp32 noise
    gl = T(rng.normal(size=(b, Ls + Lg)))
    return zg, p_m, p_v, eps, gl


def latent_head_ref(zg, p_m, p_v, eps, gl, Ls, Lg, wk=HEAD_WEIGHTS[0], wa=HEAD_WEIGHTS[1]):
    """The line-by-line torch formulation of SpaDOT.py:78-93 in the dtype of its inputs (fp64 for the reference), and the
    gradients of sum(latent * gl) + wk * GAT_KL + wa * alignment w.r.t. the GAT_fc output and the SVGP posterior."""
    zr, pmr, pvr = (t.clone().requires_grad_(True) for t in (zg, p_m, p_v))
    mu, var = zr[:, :Lg], torch.exp(zr[:, Lg:])
    s_lat = pmr + eps[:, :Ls] * torch.sqrt(pvr)
    g_lat = mu + eps[:, Ls:] * torch.sqrt(var)
    kl = -0.5 * torch.sum(1 + torch.log(var) - mu.pow(2) - var) / Lg
    al = torch.nn.functional.mse_loss(s_lat.norm(dim=1) / Ls, g_lat.norm(dim=1) / Lg, reduction="sum")
    lat = torch.cat([s_lat, g_lat], 1)
    ((lat * gl).sum() + wk * kl + wa * al).backward()
    return {"latent": lat.detach(), "kl": float(kl.detach()), "al": float(al.detach()), "zg": zr.grad, "p_m": pmr.grad, "p_v": pvr.grad}


# ----------------------------------------------------------------------------------------------- cluster losses
# chunk = rows staged per pass (10240 // D, at most b, at least 64, rounded up to 8); chunks = ceil(b / chunk);
# path "fast" needs K <= 16 and K * D <= 512; slots = ceil(K * D / 512) PAIRS slots in use; overflow: the first chunk
# holds more than 20 * 512 latent values; fb: cluster_losses_fb serves the shape (fast path, one chunk), else None.
# Every case has one cluster missing from the time point (2), one missing from the batch (1) and one all-zero plan row (3).
CLUSTER_CASES = [
    {"b": 513, "D": 20, "K": 10, "Kp": 10, "chunk": 512, "chunks": 2, "path": "fast", "slots": 1, "overflow": False, "fb": False},
    {"b": 1100, "D": 20, "K": 10, "Kp": 7, "chunk": 512, "chunks": 3, "path": "fast", "slots": 1, "overflow": False, "fb": False},
    {"b": 500, "D": 24, "K": 12, "Kp": 12, "chunk": 432, "chunks": 2, "path": "fast", "slots": 1, "overflow": True, "fb": False},
    {"b": 512, "D": 20, "K": 17, "Kp": 17, "chunk": 512, "chunks": 1, "path": "general", "slots": 1, "overflow": False, "fb": False},
    {"b": 1100, "D": 20, "K": 32, "Kp": 20, "chunk": 512, "chunks": 3, "path": "general", "slots": 2, "overflow": False, "fb": False},
    {"b": 96, "D": 32, "K": 64, "Kp": 64, "chunk": 96, "chunks": 1, "path": "general", "slots": 4, "overflow": False, "fb": False},
    {"b": 200, "D": 32, "K": 16, "Kp": 16, "chunk": 200, "chunks": 1, "path": "fast", "slots": 1, "overflow": False, "fb": True},
    # K <= 16 but K * D = 640: pairs 512.. have no fast-path slot (the fold fills slot 0 only), so this is the general path
    {"b": 200, "D": 40, "K": 16, "Kp": 16, "chunk": 200, "chunks": 1, "path": "general", "slots": 2, "overflow": False, "fb": False},
    {"b": 5, "D": 20, "K": 10, "Kp": 10, "chunk": 64, "chunks": 1, "path": "fast", "slots": 1, "overflow": False, "fb": True},
]
CLUSTER_WEIGHTS = (0.7, -1.9)        # d loss / d km, d loss / d ot of the backward seed
CLUSTER_ABSENT_TIMEPOINT, CLUSTER_ABSENT_BATCH, CLUSTER_DEAD_ROW = 2, 1, 3


def cluster_inputs(case):
    """numpy inputs of one case: labels of the time point, seed ids, latent rows, centres, previous centres, the plan
    (raw and row-normalised, NaN -> 0), the time point's cluster list."""
    b, D, K, Kp = case["b"], case["D"], case["K"], case["Kp"]
    rng = np.random.default_rng(1000 * b + 10 * D + K)
    N = 3000
    all_labels = rng.integers(0, K, size=N)
    all_labels[all_labels == CLUSTER_ABSENT_TIMEPOINT] = 3
    seeds = np.array([s for s in rng.permutation(N) if all_labels[s] != CLUSTER_ABSENT_BATCH][:b])
    z = rng.normal(size=(b, D)); centres = rng.normal(size=(K, D)); prev = rng.normal(size=(Kp, D))
    clusters = sorted(set(all_labels.tolist()))
    gamma = rng.uniform(size=(Kp, len(clusters))); gamma[CLUSTER_DEAD_ROW] = 0.0
    with np.errstate(invalid="ignore"):
        g_norm = np.nan_to_num(gamma / gamma.sum(1, keepdims=True), nan=0.0, posinf=0.0, neginf=0.0)
    return {"all_labels": all_labels, "seeds": seeds, "z": z, "centres": centres, "prev": prev, "gamma": gamma,
            "g_norm": g_norm, "clusters": clusters}


def cluster_reference(inp):
    """Oracle values in fp64, the gradient of 0.7 km - 1.9 ot w.r.t. z by autograd, per-cluster counts and batch means
    (the stored centre where a cluster has no row in the batch)."""
    lab = inp["all_labels"][inp["seeds"]]
    zr = torch.as_tensor(inp["z"], dtype=torch.float64).requires_grad_(True)
    km = mo.kmeans_loss(zr, inp["centres"], lab)
    ot = mo.ot_loss(zr, lab, inp["all_labels"], inp["centres"], inp["prev"], inp["gamma"])
    (CLUSTER_WEIGHTS[0] * km + CLUSTER_WEIGHTS[1] * ot).backward()
    K = inp["centres"].shape[0]
    counts = np.bincount(lab, minlength=K)
    means = inp["centres"].copy()
    for k in range(K):
        if counts[k]:
            means[k] = inp["z"][lab == k].mean(0)
    return {"km": float(km.detach()), "ot": float(ot.detach()), "dz": zr.grad.numpy(), "counts": counts, "means": means, "labels": lab}
