"""GPU parity tests for the model side: HIP kernels (through the C-ABI of libspadot_model.so) and the
model mirror vs the fp64 CPU oracle and the reference-generated golden vectors.

Stated tolerances (reference fp64 CPU vs this fp32 device path): single forward from
identical weights/batch/noise -- latent embeddings and loss terms rtol 1e-4 / atol 1e-5; SVGP
posterior (fp64 on the device) rtol 1e-6; bf16 storage relaxes latents to rtol 2e-2; integer
cluster labels exact."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import model_oracle as mo
from step_tail_cases import head_inputs, latent_head_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def T(x, dtype=F64):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spadot_amd import ops
    return ops


def _graph(ei, n):
    from spadot_amd.graph import build_batch_graph
    return build_batch_graph(ei, n, DEV)


# ------------------------------------------------------------------ GAT edge phase

@pytest.mark.parametrize("H,C,concat,act", [(4, 8, True, True), (4, 8, False, False), (4, 512, True, True),
                                           (4, 512, False, False), (2, 96, True, False), (3, 256, True, True)])
def test_gat_edge_forward_backward_vs_oracle(ops, H, C, concat, act):
    rng = np.random.default_rng(H * 1000 + C)
    n, k = 97, 7
    coords = rng.uniform(size=(n, 2))
    ei = mo.knn_graph(coords, k)
    # add a hub (in-degree > 64 exercises the multi-chunk path) and drop its duplicates
    extra = np.stack([np.arange(n), np.full(n, 5)])
    ei = torch.as_tensor(np.unique(np.concatenate([ei.numpy(), extra], axis=1), axis=1))
    fin = 24
    x = T(rng.normal(size=(n, fin)))
    W = T(rng.normal(size=(H * C, fin)) / np.sqrt(fin))
    a_s = T(rng.normal(size=(1, H, C)) * 0.3); a_d = T(rng.normal(size=(1, H, C)) * 0.3)
    bias = T(rng.normal(size=(H * C if concat else C)) * 0.1)
    # oracle (fp64, autograd through the plain formulas)
    xo, Wo, aso, ado, bo = (t.clone().requires_grad_(True) for t in (x, W, a_s, a_d, bias))
    out_o = mo.gat_conv(xo, ei, Wo, aso, ado, bo, H, concat)
    if act:
        out_o = mo.leaky_relu(out_o)
    gsel = T(rng.normal(size=tuple(out_o.shape)))
    (out_o * gsel).sum().backward()
    # device: same decomposition as spadot_amd.model.encoder.GATConv
    g = _graph(ei, n)
    xd, Wd, asd, add_, bd = (t.to(DEV, torch.float32).requires_grad_(True) for t in (x, W, a_s, a_d, bias))
    h = xd @ Wd.T
    out_d = ops.gat_edge(h, asd, add_, bd, g, H, C, concat, act)
    (out_d * gsel.to(DEV, torch.float32)).sum().backward()
    np.testing.assert_allclose(out_d.detach().cpu().numpy(), out_o.detach().numpy(), rtol=1e-4, atol=1e-5)
    for name, d, o in (("x", xd, xo), ("W", Wd, Wo), ("att_src", asd, aso), ("att_dst", add_, ado), ("bias", bd, bo)):
        ref = o.grad.numpy()
        np.testing.assert_allclose(d.grad.cpu().numpy(), ref, rtol=2e-3, atol=2e-4 * np.abs(ref).max(), err_msg=name)


@pytest.mark.parametrize("H,C,concat,act,dt", [(4, 512, False, False, torch.float32), (4, 64, True, True, torch.float32),
                                              (4, 512, False, False, torch.bfloat16)])
def test_gat_edge_seed_targets_only(ops, H, C, concat, act, dt):
    """Last GAT layer: the edge phase with only the first `rows` nodes as targets (BatchGraph.seed_graph) gives
    the same seed rows and the same gradients as the full graph followed by [:rows]."""
    from spadot_amd.graph import build_batch_graph
    rng = np.random.default_rng(11)
    n, k, rows = 300, 9, 41
    ei = mo.knn_graph(rng.uniform(size=(n, 2)), k)
    g = build_batch_graph(ei, n, DEV, seeds=rows)
    gs = g.seed_graph
    assert gs is not None and gs.n == n and gs.n_tgt == rows and gs.E == int(g.rowptr[rows])
    h0 = T(rng.normal(size=(n, H * C)) * 0.5).to(DEV, dt)
    a_s = T(rng.normal(size=(1, H, C)) * 0.2).to(DEV, torch.float32); a_d = T(rng.normal(size=(1, H, C)) * 0.2).to(DEV, torch.float32)
    bias = T(rng.normal(size=(H * C if concat else C)) * 0.1).to(DEV, torch.float32)
    w = T(rng.normal(size=(rows, H * C if concat else C))).to(DEV, dt)
    res = []
    for graph in (g, gs):
        leaves = [t.clone().requires_grad_(True) for t in (h0, a_s, a_d, bias)]
        out = ops.gat_edge(*leaves, graph, H, C, concat, act)
        assert out.shape[0] == graph.n_tgt
        out = out[:rows]
        (out.float() * w.float()).sum().backward()
        res.append([out.detach().float().cpu().numpy()] + [t.grad.float().cpu().numpy() for t in leaves])
    assert np.array_equal(res[0][0], res[1][0])                       # forward: same launches per target row
    tol = 2e-2 if dt == torch.bfloat16 else 1e-5
    for name, a, b in zip(("h", "att_src", "att_dst", "bias"), res[0][1:], res[1][1:]):
        np.testing.assert_allclose(b, a, rtol=tol, atol=tol * np.abs(a).max(), err_msg=name)


def test_gat_encoder_layer_graphs_match_full_graph(ops):
    """Batches carry per-layer graphs (layer 2 for seeds + hop 1 only, layer 3 for the seeds only): the seeds'
    encoder output and every parameter gradient equal those of the three layers run on the whole batch graph."""
    from spadot_amd.graph import knn_graph, precompute_batches, build_batch_graph, induced_batch
    from spadot_amd.model.encoder import GATEncoder
    rng = np.random.default_rng(21)
    n, k, bs, G = 900, 6, 64, 30
    side = 30
    coords = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2) + rng.uniform(-0.3, 0.3, (n, 2))
    ei = knn_graph(coords, k)                       # spatially ordered spots: the 2-hop closure is a small part of the graph
    batch = precompute_batches(ei, n, bs, DEV, coords=coords)[5]
    g = batch.graph
    assert g.layer_graphs is not None
    g2, g3 = g.layer_graphs
    assert bs == g3.n_tgt < g3.n == g2.n_tgt < g2.n == g.n < n
    # same node set and edges as the reference batch construction (oracle), up to the order inside a hop
    n_id_o, _ = mo.induced_batch(torch.as_tensor(ei), n, np.arange(5 * bs, 6 * bs))
    assert sorted(batch.n_id.cpu().tolist()) == sorted(np.asarray(n_id_o).tolist())
    torch.manual_seed(3)
    enc = GATEncoder(G, 5, hidden_dim=16, num_heads=4).to(DEV)
    x = torch.randn((g.n, G), device=DEV)
    w = torch.randn((bs, 10), device=DEV)
    full = build_batch_graph(torch.stack([g.col.long(), torch.repeat_interleave(
        torch.arange(g.n, device=DEV), (g.rowptr[1:] - g.rowptr[:-1]).long())]), g.n, DEV)      # no per-layer graphs
    res = []
    for graph in (full, g):
        enc.zero_grad()
        z = enc.pre_head(x, graph, rows=bs)
        (z * w).sum().backward()
        res.append((z.detach().cpu().numpy(), {k_: p.grad.cpu().numpy().copy() for k_, p in enc.named_parameters()}))
    np.testing.assert_allclose(res[1][0], res[0][0], rtol=1e-5, atol=1e-6)
    for name in res[0][1]:
        a, b_ = res[0][1][name], res[1][1][name]
        np.testing.assert_allclose(b_, a, rtol=1e-4, atol=1e-6 * max(1.0, np.abs(a).max()), err_msg=name)


def test_gat_edge_bf16_storage(ops):
    rng = np.random.default_rng(3)
    n, H, C = 64, 4, 512
    ei = mo.knn_graph(rng.uniform(size=(n, 2)), 6)
    g = _graph(ei, n)
    h = T(rng.normal(size=(n, H * C)), torch.float32).to(DEV)
    s1 = T(rng.normal(size=(1, H, C)) * 0.05, torch.float32).to(DEV); s2 = T(rng.normal(size=(1, H, C)) * 0.05, torch.float32).to(DEV)
    bias = torch.zeros(H * C, device=DEV)
    o32 = ops.gat_edge(h, s1, s2, bias, g, H, C, True, True)
    o16 = ops.gat_edge(h.bfloat16(), s1, s2, bias, g, H, C, True, True)
    assert o16.dtype == torch.bfloat16
    np.testing.assert_allclose(o16.float().cpu().numpy(), o32.cpu().numpy(), rtol=2e-2, atol=2e-2)


# ------------------------------------------------------------------ SVGP pieces

@pytest.mark.parametrize("tag", ["s", "l"])
def test_kernel_matrix_and_svgp_match_reference(ops, tag):
    from spadot_amd.model.svgp import SVGP
    g = load_golden("model_svgp.npz")
    x, z = T(g[f"{tag}_x"]).to(DEV), T(g[f"{tag}_z"]).to(DEV)
    for kt in ("Gaussian", "Cauchy", "Quadratic"):
        K = ops.kernel_matrix(x, z, kt, 0.1)
        np.testing.assert_allclose(K.cpu().numpy(), g[f"{tag}_K_{kt}"], rtol=1e-12, atol=1e-15)
        K32 = ops.kernel_matrix(x.float(), z.float(), kt, 0.1)
        np.testing.assert_allclose(K32.cpu().numpy(), g[f"{tag}_K_{kt}"], rtol=2e-5, atol=1e-7)
    cfg = dict(device=DEV, kernel_type="Gaussian", kernel_scale=0.1)
    sv = SVGP(cfg, g[f"{tag}_z"], float(g[f"{tag}_N_train"]))
    y, noise = T(g[f"{tag}_y"]).to(DEV), T(g[f"{tag}_noise"]).to(DEV)
    mean, B, mu_hat, A_hat = sv.approximate_posterior_params(x, x, y, noise)
    # fp64 on the device; two jittered inverses (cond ~1e6) -> 1e-6
    np.testing.assert_allclose(mean.cpu().numpy(), g[f"{tag}_mean"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(B.cpu().numpy(), g[f"{tag}_B"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(mu_hat.cpu().numpy(), g[f"{tag}_mu_hat"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(A_hat.cpu().numpy(), g[f"{tag}_A_hat"], rtol=1e-6, atol=1e-9)
    l3, kl = sv.variational_loss(x, y, noise, mu_hat, A_hat)
    assert float(l3) == pytest.approx(float(g[f"{tag}_l3"]), rel=1e-7)
    assert float(kl) == pytest.approx(float(g[f"{tag}_kl"]), rel=1e-7)
    xt = T(g[f"{tag}_xt"]).to(DEV)
    mean_t, B_t, _, _ = sv.approximate_posterior_params(xt, x, y, noise)
    np.testing.assert_allclose(mean_t.cpu().numpy(), g[f"{tag}_mean_t"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(B_t.cpu().numpy(), g[f"{tag}_B_t"], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("b,m,L", [(64, 17, 3), (512, 236, 10), (200, 261, 4)])
def test_svgp_backward_precomputed_and_restructured_forms_agree(ops, b, m, L):
    """_SVGPCore.backward three ways: plain (library products for dt, K dt, D, K S D), with dt / K dt on the wave-per-row
    kernels (MID_BWD), and with its gradient-independent products formed ahead of the backward pass (precompute_backward:
    q2, K S, and -- Q1T -- T = X2 S K_mn, m0, after which q1 is one reduction launch).  Same algebra, fp64: the encoder
    gradients agree to rounding."""
    from spadot_amd.model import svgp as sv
    rng = np.random.default_rng(7)
    cfg = dict(device=DEV, kernel_type="Gaussian", kernel_scale=0.1)
    mod = sv.SVGP(cfg, rng.uniform(0, 1, (m, 2)), 5000.0)
    x = T(rng.uniform(0, 1, (b, 2))).to(DEV)
    z0 = torch.as_tensor(np.concatenate([rng.normal(0, 1, (b, L)), rng.normal(-1, 0.3, (b, L))], 1), dtype=torch.float32).to(DEV)
    gpm, gpv = T(rng.normal(0, 1, (b, L))).to(DEV), T(rng.normal(0, 1, (b, L))).to(DEV)

    def run(mid, pre, q1t, late=False):
        old = sv.MID_BWD[0], sv.Q1T[0]
        sv.MID_BWD[0], sv.Q1T[0] = mid, q1t
        try:
            z = z0.clone().requires_grad_(True)
            bc = mod.batch_constants(x)
            queue = [] if late else None
            sv.ELBO_LATE[0] = queue          # (late: forward hands p_m / p_v over first and queues the rest of its ELBO)
            try:
                p_m, p_v, skl = mod.elbo_finish(bc, mod.elbo_start(bc, z))
            finally:
                sv.ELBO_LATE[0] = None
            head = (p_m.detach().clone(), p_v.detach().clone())
            if late:
                assert len(queue) == 1
                with torch.no_grad():
                    queue[0]()
            if pre:
                h = sv.precompute_backward(sv.holder_of(p_m))
                assert "q2" in h and "KS" in h and (("Ta" in h) == q1t)
            (dz,) = torch.autograd.grad([p_m, p_v, skl], [z], [gpm, gpv, torch.tensor(0.7, device=DEV)])
            return dz.double().cpu().numpy(), head[0].cpu().numpy(), head[1].cpu().numpy(), float(skl)
        finally:
            sv.MID_BWD[0], sv.Q1T[0] = old

    ref, pm0, pv0, skl0 = run(False, False, False)
    scale = np.abs(ref).max()
    for mid, pre, q1t, late in ((True, False, False, False), (True, True, False, False), (True, True, True, False),
                                (False, True, True, False), (True, True, True, True), (True, False, False, True)):
        got, pm, pv, skl = run(mid, pre, q1t, late)
        assert np.abs(got - ref).max() <= 2e-6 * scale, (mid, pre, q1t, late, np.abs(got - ref).max(), scale)
        np.testing.assert_allclose(pm, pm0, rtol=1e-9, atol=1e-12)           # (K_nm S_l as a product of its own: other tiles)
        np.testing.assert_allclose(pv, pv0, rtol=1e-9, atol=1e-12)
        assert skl == pytest.approx(skl0, rel=1e-6)


def test_reduction_kernels_gradients_vs_torch(ops):
    """rowdot / elbo_reduce / sqerr_sum: values and gradients against the same formulas in plain torch fp64."""
    rng = np.random.default_rng(4)
    L, n, m, b = 3, 37, 21, 37
    A = T(rng.normal(size=(L, n, m))).to(DEV).requires_grad_(True)
    B = T(rng.normal(size=(n, m))).to(DEV)
    out = ops.rowdot(A, B)
    ref = (A.detach() * B[None]).sum(-1)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-12)
    w = T(rng.normal(size=(L, n))).to(DEV)
    (out * w).sum().backward()
    np.testing.assert_allclose(A.grad.cpu().numpy(), (w[:, :, None] * B[None]).cpu().numpy(), rtol=1e-12)

    names = ("mu", "var", "mv", "tr", "pm", "pv")
    vals = {k: T(rng.normal(size=(b, L))).to(DEV) for k in names}
    vals["var"] = vals["var"].abs() + 0.3; vals["pv"] = vals["pv"].abs() + 0.1
    kt = T(rng.uniform(size=b)).to(DEV)
    leaf = {k: v.clone().requires_grad_(True) for k, v in vals.items()}
    l3, ce = ops.elbo_reduce(*(leaf[k] for k in names), kt)
    (2.0 * l3 - 0.7 * ce).backward()
    ref = {k: v.clone().requires_grad_(True) for k, v in vals.items()}
    l3r = -0.5 * ((kt[:, None] + ref["tr"]) / ref["var"] + torch.log(ref["var"]) + np.log(2 * np.pi)
                  + (ref["mu"] - ref["mv"]) ** 2 / ref["var"]).sum()
    cer = mo.gauss_cross_entropy(ref["pm"], ref["pv"], ref["mu"], ref["var"]).sum()
    (2.0 * l3r - 0.7 * cer).backward()
    assert float(l3) == pytest.approx(float(l3r), rel=1e-12) and float(ce) == pytest.approx(float(cer), rel=1e-12)
    for k in names:
        np.testing.assert_allclose(leaf[k].grad.cpu().numpy(), ref[k].grad.cpu().numpy(), rtol=1e-10, atol=1e-12, err_msg=k)

    y = T(rng.normal(size=(50, 33)), torch.float32).to(DEV)
    yh = T(rng.normal(size=(50, 33)), torch.float32).to(DEV).requires_grad_(True)
    r = ops.sqerr_sum(y, yh, 1.0 / 33)
    (3.0 * r).backward()
    assert float(r) == pytest.approx(float(((y - yh.detach()) ** 2).sum() / 33), rel=1e-6)
    np.testing.assert_allclose(yh.grad.cpu().numpy(), (3.0 * -2.0 / 33 * (y - yh.detach())).cpu().numpy(), rtol=1e-6)


@pytest.mark.parametrize("L,m", [(1, 1), (3, 17), (3, 95), (3, 96), (4, 100), (3, 128), (10, 204), (10, 217), (10, 236), (4, 248), (40, 256), (3, 257), (40, 261),
                                 (5, 272), (3, 273), (3, 279), (3, 288), (2, 289), (3, 310), (2, 311), (2, 389), (10, 600), (2, 621), (2, 870), (1, 1300)])
def test_spd_inverse_logdet_vs_torch(ops, L, m):
    """Batched SPD inverse + logdet (sweep kernel: register tiles up to 279; recursive two-block elimination beyond -- ops splits
    at 279, so the kernel's widest tiles, m = 280 .. 310 with their border in LDS, are reached by test_svgp_edges_gpu.py's direct
    calls only) against torch.linalg on matrices conditioned like the SVGP's Sigma_l (jitter 1e-2, cond ~1e6)."""
    rng = np.random.default_rng(m)
    B = rng.normal(size=(L, m, max(2, m // 3)))
    A = T(B @ B.transpose(0, 2, 1) * 50.0 + 1e-2 * np.eye(m)).to(DEV).requires_grad_(True)
    X, ld = ops.spd_inverse_logdet(A)
    Ar = A.detach().clone().requires_grad_(True)
    Xr = torch.linalg.inv(Ar)
    ldr = torch.linalg.slogdet(Ar)[1]
    eye = torch.eye(m, dtype=F64, device=DEV)
    # residual-based check (the inverse itself is only defined to cond * eps): no worse than 10x the library's
    res = float((A.detach() @ X.detach() - eye).abs().max())
    res_ref = float((Ar.detach() @ Xr.detach() - eye).abs().max())
    assert res <= 10 * res_ref + 1e-12, (res, res_ref)
    # 2/3 of the pivots are jitter-sized Schur complements (cancellation ~ cond * eps): 1e-7 absolute
    np.testing.assert_allclose(ld.detach().cpu().numpy(), ldr.detach().cpu().numpy(), rtol=1e-9, atol=1e-7)
    np.testing.assert_allclose(X.detach().cpu().numpy(), Xr.detach().cpu().numpy(), rtol=1e-6, atol=1e-7 * float(Xr.abs().max()))
    W = T(rng.normal(size=(L, m, m))).to(DEV)
    wl = T(rng.normal(size=L)).to(DEV)
    ((X * W).sum() + (ld * wl).sum()).backward()
    ((Xr * W).sum() + (ldr * wl).sum()).backward()
    ga, gr = A.grad.cpu().numpy(), Ar.grad.cpu().numpy()
    np.testing.assert_allclose(ga, gr, rtol=1e-5, atol=1e-6 * np.abs(gr).max())


# ------------------------------------------------------------------ composite model

def _model(g, compute_dtype=torch.float32):
    from spadot_amd.model import SpaDOT
    cfg = dict(input_dim=g["Y"].shape[1], z_dim=20, device=DEV, svgp_encoder_layers=[24, 12],
               gat_encoder_hidden=8, gat_attention_heads=int(g["heads"]), decoder_layers=[12, 24],
               kernel_type="Gaussian", kernel_scale=0.1, timepoints=[0, 1], compute_dtype=compute_dtype)
    m = SpaDOT.SpaDOT(cfg, {"inducing_points": {0: g["ind0"], 1: g["ind1"]},
                            "N_train": {0: float(g["N_train0"]), 1: float(g["N_train1"])}}).to(DEV)
    m.load_state_dict({k[3:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("sd/")})
    return m


def test_composite_forward_and_gradients_match_reference(ops):
    g = load_golden("model_composite.npz")
    m = _model(g)
    m.train()
    b = int(g["batch_size"])
    n_id = torch.as_tensor(g["n_id"])
    xb = T(g["X"])[n_id].to(DEV)
    yb = T(g["Y"], torch.float32)[n_id].to(DEV)
    graph = _graph(g["sub_edge_index"], n_id.numel())
    noise = (T(g["noise_svgp"]).to(DEV), T(g["noise_gat"], torch.float32).to(DEV))
    recon, skl, gkl, align, z = m.forward(xb, yb, graph, 0, b, noise=noise)
    # reference fp64 CPU vs fp32 device path: loss terms and latents rtol 1e-4 / atol 1e-5
    assert float(recon) == pytest.approx(float(g["recon"]), rel=1e-4)
    assert float(skl) == pytest.approx(float(g["SVGP_KL"]), rel=1e-4)
    assert float(gkl) == pytest.approx(float(g["GAT_KL"]), rel=1e-4)
    assert float(align) == pytest.approx(float(g["alignment"]), rel=1e-4)
    np.testing.assert_allclose(z.detach().cpu().numpy(), g["final_latent"], rtol=1e-4, atol=1e-5)
    # gradients of the step loss w.r.t. every parameter
    loss = 0.1 * recon - 0.5 * skl + 1e-4 * gkl + 0.1 * align
    m.zero_grad()
    loss.backward()
    for name, p in m.named_parameters():
        ref = g["grad/" + name]
        assert p.grad is not None, name
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=5e-3, atol=5e-5 * max(1e-3, np.abs(ref).max()),
                                   err_msg=name)
    # BatchNorm running statistics after one train-mode forward
    sd = m.state_dict()
    for k in g.files:
        if k.startswith("sd_after/") and "running" in k:
            np.testing.assert_allclose(sd[k[9:]].cpu().numpy(), g[k], rtol=1e-4, atol=1e-6, err_msg=k)


def test_whole_time_point_row_contraction_in_slabs(ops):
    """svgp._contract_rows: K_mn (y / noise) over a whole time point's rows (10^4) as slabs + a fixed-order sum equals the
    plain contraction (fp64: 1e-12 of the summed magnitudes), remainder rows included; small batches keep the plain form."""
    from spadot_amd.model.svgp import _contract_rows
    g = torch.Generator(device=DEV).manual_seed(11)
    for b in (10000, 2048, 2300, 512):
        K = torch.rand((b, 236), dtype=torch.float64, device=DEV, generator=g)
        Y = torch.randn((b, 20), dtype=torch.float64, device=DEV, generator=g) * 50.0
        t = _contract_rows(K, Y)
        ref = torch.einsum("bm,bl->lm", K.cpu(), Y.cpu())
        mag = torch.einsum("bm,bl->lm", K.cpu().abs(), Y.cpu().abs())
        assert t.shape == (20, 236)
        assert bool(((t.cpu() - ref).abs() <= 1e-12 * mag).all())
        assert torch.equal(t, _contract_rows(K, Y))


def test_all_latent_samples_matches_reference(ops):
    g = load_golden("model_composite.npz")
    m = _model(g)
    m.eval()
    with torch.no_grad():
        lat = m.all_latent_samples(g["X"], g["Y"].astype(np.float32), g["edge_index"], 1)
    assert isinstance(lat, np.ndarray) and lat.shape == (g["X"].shape[0], 20)
    np.testing.assert_allclose(lat, g["all_latent_tp1"], rtol=1e-4, atol=1e-5)


def test_composite_forward_bf16_compute(ops):
    g = load_golden("model_composite.npz")
    m = _model(g, torch.bfloat16)
    m.train()
    b = int(g["batch_size"])
    n_id = torch.as_tensor(g["n_id"])
    xb = T(g["X"])[n_id].to(DEV)
    yb = T(g["Y"], torch.float32)[n_id].to(DEV)
    graph = _graph(g["sub_edge_index"], n_id.numel())
    noise = (T(g["noise_svgp"]).to(DEV), T(g["noise_gat"], torch.float32).to(DEV))
    recon, skl, gkl, align, z = m.forward(xb, yb, graph, 0, b, noise=noise)
    # bf16 compute in the GAT branch and in the two G-sized dense maps: latents rtol 2e-2
    np.testing.assert_allclose(z.detach().cpu().numpy(), g["final_latent"], rtol=2e-2, atol=2e-2)
    # all four loss terms of the reference-generated fixture (fp64) ...
    for name, got in (("recon", recon), ("SVGP_KL", skl), ("GAT_KL", gkl), ("alignment", align)):
        assert float(got) == pytest.approx(float(g[name]), rel=2e-2), name
    # ... and the gradient of the step loss w.r.t. every parameter.  8 significant bits in the GAT branch's activations,
    # three layers deep, on a model this small (hidden width 8: no averaging over channels) -> per parameter relative L2
    # error <= 0.3 and cosine >= 0.98; at the benchmarked width the same comparison is held to 0.1 / 0.99
    # (tests/test_step_parity_gpu.py)
    loss = 0.1 * recon - 0.5 * skl + 1e-4 * gkl + 0.1 * align
    m.zero_grad()
    loss.backward()
    worst = {}
    for name, p in m.named_parameters():
        ref = g["grad/" + name].astype(np.float64)
        assert p.grad is not None, name
        got = p.grad.double().cpu().numpy()
        nr = np.linalg.norm(ref)
        if nr <= 1e-12:
            assert np.linalg.norm(got) <= 1e-6, name
            continue
        worst[name] = (np.linalg.norm(got - ref) / nr, float((got * ref).sum() / (nr * np.linalg.norm(got))))
    print({k: (round(v[0], 4), round(v[1], 6)) for k, v in worst.items()})
    for name, (rel, cos) in worst.items():
        assert rel <= 0.3 and cos >= 0.98, (name, rel, cos)


# ------------------------------------------------------------------ spatial graph on the device

@pytest.mark.parametrize("n,kk,d", [(1500, 31, 2), (300, 7, 2), (50, 50, 3), (10000, 31, 2)])
def test_device_knn_matches_host_neighbours(ops, n, kk, d):
    """ops.knn (brute force, fp64) returns sklearn's neighbours in sklearn's order on points without exact ties;
    graph.knn_graph gives the same edge list with either backend."""
    from sklearn.neighbors import NearestNeighbors
    from spadot_amd.graph import knn_graph
    rng = np.random.default_rng(n + kk)
    pts = rng.uniform(size=(n, d)) * 30.0
    _, ref = NearestNeighbors(n_neighbors=kk).fit(pts).kneighbors(pts)
    got = ops.knn(torch.as_tensor(pts, device=DEV), kk).cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    if d == 2 and kk > 8:
        a = knn_graph(pts, 6, max_neigh=kk - 1)
        b_ = knn_graph(pts, 6, max_neigh=kk - 1, backend="device", device=DEV)
        np.testing.assert_array_equal(a, b_)
    # exact duplicates: ordered by index among equal distances, every point finds itself at distance 0
    dup = np.repeat(pts[:20], 2, axis=0)
    g2 = ops.knn(torch.as_tensor(dup, device=DEV), 4).cpu().numpy()
    assert (g2[:, :2] // 2 == np.arange(40)[:, None] // 2).all() and (g2[:, 0] < g2[:, 1]).all()


# ------------------------------------------------------------------ glue: k-means labels, optimiser

def test_kmeans_assignment_is_bit_exact(ops):
    g = load_golden("model_glue.npz")
    for dt in (torch.float64, torch.float32):
        lab = ops.kmeans_assign(T(g["km_points"], dt).to(DEV), T(g["km_centers"], dt).to(DEV))
        assert lab.dtype == torch.int32
        np.testing.assert_array_equal(lab.cpu().numpy(), g["km_predict"])
    # ties go to the first centre, empty / single inputs work
    x = torch.zeros((3, 4), dtype=torch.float64, device=DEV)
    c = torch.zeros((5, 4), dtype=torch.float64, device=DEV)
    assert ops.kmeans_assign(x, c).cpu().tolist() == [0, 0, 0]


def test_flat_adamw_matches_torch_clip_and_adamw(ops):
    torch.manual_seed(0)
    shapes = [(7, 13), (13,), (5, 3, 2), (1,)]
    ref_p = [torch.randn(s, device=DEV).requires_grad_(True) for s in shapes]
    my_p = [p.detach().clone().requires_grad_(True) for p in ref_p]
    opt_ref = torch.optim.AdamW(ref_p, lr=3e-4)
    opt_my = ops.FlatAdamW(my_p, lr=3e-4, max_norm=0.3)
    for step in range(4):
        grads = [torch.randn(s, device=DEV) * (3.0 if step % 2 else 0.01) for s in shapes]   # clipped / not clipped
        opt_ref.zero_grad(); opt_my.zero_grad()
        for p, q, gr in zip(ref_p, my_p, grads):
            p.grad = gr.clone()
            q.grad.copy_(gr)
        total = torch.nn.utils.clip_grad_norm_(ref_p, 0.3)
        assert float(opt_my.grad_norm_sq().sqrt()) == pytest.approx(float(total), rel=1e-5)
        opt_ref.step(); opt_my.step()
        for p, q in zip(ref_p, my_p):
            np.testing.assert_allclose(q.detach().cpu().numpy(), p.detach().cpu().numpy(), rtol=2e-6, atol=1e-7)


def test_flat_adamw_keeps_bf16_weight_images_current(ops):
    """FlatAdamW.maintain_image: the update kernel that also stores bf16(new weight) into a padded [rows, Kp] image gives
    the SAME parameters, bit for bit, as the plain update, the image equals a cast of the parameter after every step,
    pad columns stay untouched, parameters without an image are updated as before; unsuitable pairs are refused."""
    torch.manual_seed(3)
    shapes = [(64, 20), (20,), (48, 24), (7, 12), (5,)]
    base = [torch.randn(s, device=DEV) for s in shapes]
    pa = [p.clone().requires_grad_(True) for p in base]
    pb = [p.clone().requires_grad_(True) for p in base]
    oa, ob = ops.FlatAdamW(pa, lr=1e-2, max_norm=0.3), ops.FlatAdamW(pb, lr=1e-2, max_norm=0.3)
    img0 = torch.full((64, 32), 5.0, dtype=torch.bfloat16, device=DEV)      # Kp = 32 > K = 20: columns 20.. are padding
    img2 = torch.zeros((48, 24), dtype=torch.bfloat16, device=DEV)
    assert ob.maintain_image(pb[0], img0) and ob.maintain_image(pb[2], img2) and ob.maintain_image(pb[0], img0)
    assert ob.maintains(img0) and ob.images_version == 2
    assert not ob.maintain_image(pb[1], torch.zeros((20, 4), dtype=torch.bfloat16, device=DEV))     # not a matrix
    assert not ob.maintain_image(pb[3], torch.zeros((7, 12), dtype=torch.float32, device=DEV))      # not a bf16 image
    assert not ob.maintain_image(base[0], torch.zeros((64, 20), dtype=torch.bfloat16, device=DEV))  # not its parameter
    np.testing.assert_array_equal(img0[:, :20].float().cpu().numpy(), pb[0].detach().bfloat16().float().cpu().numpy())
    for step in range(4):
        grads = [torch.randn(s, device=DEV) * (3.0 if step % 2 else 0.01) for s in shapes]
        for q, r, gr in zip(pa, pb, grads):
            q.grad.copy_(gr); r.grad.copy_(gr)
        oa.step(); ob.step()
        torch.cuda.synchronize()
        assert torch.equal(oa.flat_param, ob.flat_param) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
        assert torch.equal(img0[:, :20], pb[0].detach().bfloat16()) and torch.equal(img2, pb[2].detach().bfloat16())
        assert bool((img0[:, 20:] == 5.0).all())
    with torch.no_grad():
        pb[2].mul_(2.0)
    ob.refresh_images()
    assert torch.equal(img2, pb[2].detach().bfloat16())


def test_flat_adamw_update_in_two_parts_is_bit_identical(ops):
    """FlatAdamW(first=...): the `first` group sits at the start of the flat buffers whatever the order of the parameters, and
    step_head() + step_rest() (gradient norm + the first group, then everything else: spadot_grad_norm_step_dev,
    spadot_adamw_range_dev) leave the bits step() leaves -- parameters, both moments, the step count, maintained images."""
    torch.manual_seed(5)
    shapes = [(64, 20), (20,), (48, 24), (7, 12), (5,), (16, 8)]
    base = [torch.randn(s, device=DEV) for s in shapes]
    pa = [p.clone().requires_grad_(True) for p in base]
    pb = [p.clone().requires_grad_(True) for p in base]
    oa = ops.FlatAdamW(pa, lr=1e-2, max_norm=0.3)
    ob = ops.FlatAdamW(pb, lr=1e-2, max_norm=0.3, first=[pb[3], pb[2]], last=[pb[0]])
    assert oa.head_count == 0 and ob.head_count == 48 * 24 + 7 * 12
    assert [id(p) for p in ob.params] == [id(pb[i]) for i in (2, 3, 1, 4, 5, 0)]
    assert pb[2].data_ptr() == ob.flat_param.data_ptr() and ob.tail_offset == ob.count - 64 * 20
    ia, ib = (torch.zeros((48, 32), dtype=torch.bfloat16, device=DEV) for _ in range(2))      # an image INSIDE the first group
    ja, jb = (torch.zeros((64, 20), dtype=torch.bfloat16, device=DEV) for _ in range(2))      # and one in the rest
    assert oa.maintain_image(pa[2], ia) and ob.maintain_image(pb[2], ib) and oa.maintain_image(pa[0], ja) and ob.maintain_image(pb[0], jb)
    for step in range(4):
        grads = [torch.randn(s, device=DEV) * (3.0 if step % 2 else 0.01) for s in shapes]
        for q, r, gr in zip(pa, pb, grads):
            q.grad.copy_(gr); r.grad.copy_(gr)
        oa.step()
        ob.step_head(); ob.step_rest()
        torch.cuda.synchronize()
        for q, r in zip(pa, pb):
            assert torch.equal(q.detach(), r.detach())
        assert int(oa.step_dev.item()) == int(ob.step_dev.item()) == step + 1 and torch.equal(oa.sumsq, ob.sumsq)
        assert torch.equal(ia, ib) and torch.equal(ja, jb) and torch.equal(ib[:, :24], pb[2].detach().bfloat16())
    # the moments too (compared through the parameters' views: the two buffers are ordered differently)
    for q, r in zip(pa, pb):
        oq = (q.data_ptr() - oa.flat_param.data_ptr()) // 4
        orr = (r.data_ptr() - ob.flat_param.data_ptr()) // 4
        n = q.numel()
        assert torch.equal(oa.exp_avg[oq:oq + n], ob.exp_avg[orr:orr + n]) and torch.equal(oa.exp_avg_sq[oq:oq + n], ob.exp_avg_sq[orr:orr + n])
    lib = ops.model_lib()
    z = torch.zeros(8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.spadot_adamw_range_dev(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 2, 4, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.3,
                                      ob.sumsq.data_ptr(), ob.step_dev.data_ptr(), None, None, st) == -22          # offset % 4


# ------------------------------------------------------------------ fused small-MLP stages

@pytest.mark.parametrize("b,F_,dt", [(512, 256, torch.float32), (37, 70, torch.float32), (512, 256, torch.bfloat16), (300, 64, torch.float32)])
def test_bn_act_matches_batchnorm_leakyrelu(ops, b, F_, dt):
    """ops.bn_act = leaky_relu(BatchNorm1d(x + bias)) in training mode: output, running statistics, counter and
    all gradients against torch's modules (fp64 reference)."""
    rng = np.random.default_rng(b + F_)
    x = T(rng.normal(size=(b, F_)) * 2 + 0.5).to(dt).double(); lb = T(rng.normal(size=F_))
    w = T(rng.normal(size=(b, F_)))
    ref_bn = torch.nn.BatchNorm1d(F_).double(); my_bn = torch.nn.BatchNorm1d(F_).to(DEV)
    with torch.no_grad():
        for bn in (ref_bn, my_bn):
            bn.weight.copy_(T(rng.normal(size=F_) * 0.5 + 1).to(bn.weight)) if bn is ref_bn else bn.weight.copy_(ref_bn.weight.float())
            bn.bias.copy_(T(rng.normal(size=F_) * 0.3).to(bn.bias)) if bn is ref_bn else bn.bias.copy_(ref_bn.bias.float())
    xr = x.clone().requires_grad_(True); lbr = lb.clone().requires_grad_(True)
    yr = torch.nn.functional.leaky_relu(ref_bn(xr + lbr), 0.01)
    (yr * w).sum().backward()
    xd = x.to(DEV, dt).requires_grad_(True); lbd = lb.to(DEV, torch.float32).requires_grad_(True)
    yd = ops.bn_act(xd, lbd, my_bn, 0.01)
    (yd * w.to(DEV, torch.float32)).sum().backward()
    tol = 2e-2 if dt == torch.bfloat16 else 2e-4
    np.testing.assert_allclose(yd.detach().cpu().numpy(), yr.detach().numpy(), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(my_bn.running_mean.cpu().numpy(), ref_bn.running_mean.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(my_bn.running_var.cpu().numpy(), ref_bn.running_var.numpy(), rtol=1e-5, atol=1e-6)
    assert int(my_bn.num_batches_tracked) == 1
    for name, a, r in (("x", xd.grad, xr.grad), ("gamma", my_bn.weight.grad, ref_bn.weight.grad), ("beta", my_bn.bias.grad, ref_bn.bias.grad)):
        r = r.numpy()
        np.testing.assert_allclose(a.float().cpu().numpy(), r, rtol=tol, atol=tol * np.abs(r).max(), err_msg=name)
    assert float(lbd.grad.abs().max()) == 0.0 and float(lbr.grad.abs().max()) < 1e-9      # the batch mean removes the shift


@pytest.mark.parametrize("b,G,hid", [(512, 300, (256, 64)), (235, 96, (256, 64)), (64, 40, (32, 16))])
def test_svgp_encoder_fused_stages_match_the_reference_modules(ops, b, G, hid):
    """SVGPEncoder.pre_head in training mode (encoder.py:7-34) with the stages behind the first map as two launches
    (csrc/enc_fused.hip: partial products across workgroups, round 5) against torch's own modules in fp64: the output z, both
    BatchNorms' running statistics and counters, every parameter's gradient and the input's -- and the same again through the
    deferred form, where SVGP_fc's partial products are summed by the SVGP stage's first kernel (svgp.elbo_start(partials=...))."""
    from spadot_amd.model.encoder import SVGPEncoder
    from spadot_amd.model import svgp as sv
    torch.manual_seed(b + G)
    enc = SVGPEncoder(G, 10, list(hid)).to(DEV)
    ref = torch.nn.Sequential()
    dims = [G] + list(hid)
    mods = []
    for i in range(len(hid)):
        mods += [torch.nn.Linear(dims[i], dims[i + 1]), torch.nn.BatchNorm1d(dims[i + 1]), torch.nn.LeakyReLU()]
    ref = torch.nn.Sequential(*mods).double()
    fc = torch.nn.Linear(hid[-1], 20).double()
    with torch.no_grad():
        for k in (0, 1, 3, 4):
            for pn in ("weight", "bias"):
                getattr(enc.SVGP_encoder_net[k], pn).copy_(torch.randn_like(getattr(enc.SVGP_encoder_net[k], pn)) * (0.05 if k in (0, 3) else 0.5)
                                                           + (1.0 if (k in (1, 4) and pn == "weight") else 0.0))
                getattr(ref[k], pn).copy_(getattr(enc.SVGP_encoder_net[k], pn).double().cpu())
        fc.weight.copy_(enc.SVGP_fc.weight.double().cpu()); fc.bias.copy_(enc.SVGP_fc.bias.double().cpu())
    x = torch.randn((b, G), device=DEV)
    w = torch.randn((b, 20), device=DEV)
    xr = x.double().cpu().requires_grad_(True)
    ref.train()
    zr = fc(ref(xr))
    (zr * w.double().cpu()).sum().backward()
    enc.train()
    assert ops.encoder_mid_ok(torch.empty((b, hid[0]), device=DEV), enc.SVGP_encoder_net[3].weight, enc.SVGP_fc.weight)
    xd = x.clone().requires_grad_(True)
    z = enc.pre_head(xd)
    assert not hasattr(z, "_enc_partials")
    (z * w).sum().backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(z.detach().cpu().numpy(), zr.detach().numpy(), rtol=2e-4, atol=2e-5)
    for k in (1, 4):
        np.testing.assert_allclose(enc.SVGP_encoder_net[k].running_mean.cpu().numpy(), ref[k].running_mean.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(enc.SVGP_encoder_net[k].running_var.cpu().numpy(), ref[k].running_var.numpy(), rtol=1e-5, atol=1e-6)
        assert int(enc.SVGP_encoder_net[k].num_batches_tracked) == 1
    pairs = [("x", xd.grad, xr.grad), ("fc.W", enc.SVGP_fc.weight.grad, fc.weight.grad), ("fc.b", enc.SVGP_fc.bias.grad, fc.bias.grad)]
    for k in (0, 1, 3, 4):
        pairs.append((f"{k}.weight", enc.SVGP_encoder_net[k].weight.grad, ref[k].weight.grad))
        if k in (1, 4):
            pairs.append((f"{k}.bias", enc.SVGP_encoder_net[k].bias.grad, ref[k].bias.grad))
    for name, a, r in pairs:
        r = r.numpy()
        np.testing.assert_allclose(a.float().cpu().numpy(), r, rtol=5e-4, atol=5e-4 * np.abs(r).max(), err_msg=name)
    for k in (0, 3):                                    # a Linear bias in front of BatchNorm: zero gradient
        assert float(enc.SVGP_encoder_net[k].bias.grad.abs().max()) == 0.0
    # the deferred form: z is filled by the SVGP stage's first kernel from the partials -- same z, same downstream values
    m = 23
    mod = sv.SVGP(dict(device=DEV, kernel_type="Gaussian", kernel_scale=0.1), np.random.default_rng(0).uniform(0, 1, (m, 2)), 4000.0)
    xy = torch.as_tensor(np.random.default_rng(1).uniform(0, 1, (b, 2))).to(DEV)
    bc = mod.batch_constants(xy)
    with torch.no_grad():
        z_plain = enc.pre_head(x)
        st_plain = mod.elbo_start(bc, z_plain)
        z_def = enc.pre_head(x, defer_fc=True)
        assert hasattr(z_def, "_enc_partials")
        st_def = mod.elbo_start(bc, z_def, partials=z_def._enc_partials)
    torch.cuda.synchronize()
    np.testing.assert_allclose(z_def.cpu().numpy(), z_plain.cpu().numpy(), rtol=1e-6, atol=1e-7)
    for u, v in zip(st_plain[1][:3], st_def[1][:3]):            # mu, var, w
        np.testing.assert_allclose(v.cpu().numpy(), u.cpu().numpy(), rtol=1e-6, atol=1e-9)
    # bit-repeatable
    with torch.no_grad():
        z2 = enc.pre_head(x)
    assert torch.equal(z2, z_plain)


@pytest.mark.parametrize("b,F_", [(512, 64), (512, 256), (19, 100)])
def test_ln_act_matches_layernorm_leakyrelu(ops, b, F_):
    rng = np.random.default_rng(b * 3 + F_)
    x = T(rng.normal(size=(b, F_)) * 1.5 - 0.2); w = T(rng.normal(size=(b, F_)))
    ref = torch.nn.LayerNorm(F_).double(); mine = torch.nn.LayerNorm(F_).to(DEV)
    with torch.no_grad():
        ref.weight.copy_(T(rng.normal(size=F_) * 0.5 + 1)); ref.bias.copy_(T(rng.normal(size=F_) * 0.3))
        mine.weight.copy_(ref.weight.float()); mine.bias.copy_(ref.bias.float())
    xr = x.clone().requires_grad_(True)
    (torch.nn.functional.leaky_relu(ref(xr), 0.01) * w).sum().backward()
    xd = x.to(DEV, torch.float32).requires_grad_(True)
    yd = ops.ln_act(xd, mine, 0.01)
    (yd * w.to(DEV, torch.float32)).sum().backward()
    np.testing.assert_allclose(yd.detach().cpu().numpy(), torch.nn.functional.leaky_relu(ref(x), 0.01).detach().numpy(), rtol=2e-4, atol=2e-5)
    for name, a, r in (("x", xd.grad, xr.grad), ("gamma", mine.weight.grad, ref.weight.grad), ("beta", mine.bias.grad, ref.bias.grad)):
        r = r.numpy()
        np.testing.assert_allclose(a.cpu().numpy(), r, rtol=2e-4, atol=2e-4 * np.abs(r).max(), err_msg=name)


# ------------------------------------------------------------------ loss tail kernels

@pytest.mark.parametrize("b,Ls,Lg", [(512, 10, 10), (37, 3, 5), (1300, 10, 10)])
def test_latent_head_vs_torch_formulas(ops, b, Ls, Lg):
    """ops.latent_head against the line-by-line torch formulation of SpaDOT.py:78-93 in fp64 (values and
    gradients w.r.t. the GAT_fc output and the SVGP posterior)."""
    zg, p_m, p_v, eps, gl = head_inputs(b, Ls, Lg)
    wk, wa = 0.37, -1.3
    # reference (the fp64 formulas, shared with the edge cases of test_step_tail_edges_gpu.py)
    want = latent_head_ref(zg, p_m, p_v, eps, gl, Ls, Lg, wk, wa)
    # device
    zd = zg.to(DEV, torch.float32).requires_grad_(True)
    pmd, pvd = (t.to(DEV).requires_grad_(True) for t in (p_m, p_v))
    lat, kl_d, al_d = ops.latent_head(zd, pmd, pvd, eps.to(DEV, torch.float32), Ls, Lg)
    ((lat * gl.to(DEV, torch.float32)).sum() + wk * kl_d + wa * al_d).backward()
    np.testing.assert_allclose(lat.detach().cpu().numpy(), want["latent"].numpy(), rtol=2e-6, atol=2e-6)
    assert float(kl_d) == pytest.approx(want["kl"], rel=1e-5) and float(al_d) == pytest.approx(want["al"], rel=1e-5)
    for name, d in (("zg", zd), ("p_m", pmd), ("p_v", pvd)):
        ref = want[name].numpy()
        np.testing.assert_allclose(d.grad.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max(), err_msg=name)


def test_latent_head_draws_its_own_standard_normals(ops):
    """eps=None: the kernel fills eps from (seed, launch count) on the device -- standard normal moments, a new draw per
    launch, the same draws for the same state, and the sample it returns is mu + eps * sigma of those eps."""
    b, Ls, Lg = 4096, 10, 10
    zg = torch.zeros((b, 2 * Lg), device=DEV); pm = torch.zeros((b, Ls), device=DEV, dtype=torch.float64); pv = torch.ones_like(pm)
    st = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    lat1, _, _ = ops.latent_head(zg, pm, pv, None, Ls, Lg, st)
    lat2, _, _ = ops.latent_head(zg, pm, pv, None, Ls, Lg, st)
    assert st.cpu().tolist() == [1234, 2]
    x1, x2 = lat1.cpu().numpy().ravel(), lat2.cpu().numpy().ravel()      # mu = 0, sigma = 1: the latent IS eps
    assert abs(x1.mean()) < 0.02 and abs(x1.std() - 1.0) < 0.02 and abs((x1 ** 3).mean()) < 0.05 and abs((x1 ** 4).mean() - 3.0) < 0.15
    assert abs(np.corrcoef(x1, x2)[0, 1]) < 0.02 and not np.array_equal(x1, x2)
    assert abs(np.corrcoef(x1[:-1], x1[1:])[0, 1]) < 0.02
    st2 = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    lat3, _, _ = ops.latent_head(zg, pm, pv, None, Ls, Lg, st2)
    assert torch.equal(lat3, lat1)


@pytest.mark.parametrize("b,K,absent", [(512, 10, False), (64, 10, True), (700, 7, True), (700, 7, False)])
def test_cluster_losses_vs_oracle_and_torch_gradient(ops, b, K, absent):
    """ops.cluster_losses: values against the oracle's restatement of _train_utils.py:240-253/272-307, the
    gradient against torch autograd of the same formulas in fp64."""
    rng = np.random.default_rng(b + K)
    D, N = 20, 3000
    all_labels = rng.integers(0, K, size=N)
    if absent:
        all_labels[all_labels == 2] = 3                                   # cluster 2 does not exist in this time point
    seeds = rng.choice(N, size=b, replace=False)
    if absent:
        seeds = np.array([s for s in seeds if all_labels[s] != 1][: max(8, b // 2)])   # cluster 1 absent from the batch
    b = seeds.size
    z = rng.normal(size=(b, D)); centres = rng.normal(size=(K, D)); prev = rng.normal(size=(K, D))
    clusters = sorted(set(all_labels.tolist()))
    gamma = rng.uniform(size=(K, len(clusters))); gamma[3] = 0.0          # a dead row: nan_to_num path of the reference
    with np.errstate(invalid="ignore"):
        g_norm = np.nan_to_num(gamma / gamma.sum(1, keepdims=True), nan=0.0, posinf=0.0, neginf=0.0)
    lab = all_labels[seeds]
    zr = T(z).requires_grad_(True)
    km_r = mo.kmeans_loss(zr, centres, lab)
    ot_r = mo.ot_loss(zr, lab, all_labels, centres, prev, gamma)
    (0.7 * km_r - 1.9 * ot_r).backward()
    f32 = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV).contiguous()
    zd = f32(z).requires_grad_(True)
    km, ot = ops.cluster_losses(zd, torch.as_tensor(all_labels, dtype=torch.int64, device=DEV),
                                torch.as_tensor(seeds, dtype=torch.int64, device=DEV), f32(centres), f32(prev), f32(g_norm),
                                torch.as_tensor(clusters, dtype=torch.int64, device=DEV), True, True)
    (0.7 * km - 1.9 * ot).backward()
    assert float(km) == pytest.approx(float(km_r), rel=2e-5) and float(ot) == pytest.approx(float(ot_r), rel=2e-5)
    ref = zr.grad.numpy()
    np.testing.assert_allclose(zd.grad.cpu().numpy(), ref, rtol=2e-4, atol=2e-6 * np.abs(ref).max())
    # each term alone (the switches of the first epochs)
    km1, ot1 = ops.cluster_losses(zd.detach(), torch.as_tensor(all_labels, dtype=torch.int64, device=DEV),
                                  torch.as_tensor(seeds, dtype=torch.int64, device=DEV), f32(centres), do_km=True, do_ot=False)
    assert float(km1) == float(km) and float(ot1) == 0.0
    # forward + gradient in ONE launch for seeds known in advance (cluster_losses_fb): the same bits as the two launches, no
    # gradient path of its own to z, and a backward seeded with anything but the promised weights refuses
    wv = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.7, -1.9], dtype=torch.float32, device=DEV)
    args = (torch.as_tensor(all_labels, dtype=torch.int64, device=DEV), torch.as_tensor(seeds, dtype=torch.int64, device=DEV),
            f32(centres), f32(prev), f32(g_norm), torch.as_tensor(clusters, dtype=torch.int64, device=DEV))
    for do_km, do_ot in ((True, True), (True, False)):
        zp = f32(z).requires_grad_(True)
        kmp, otp = ops.cluster_losses(zp, *args, do_km, do_ot)
        torch.autograd.backward([kmp, otp], [wv[4], wv[5]])
        zq = f32(z).requires_grad_(True)
        res = ops.cluster_losses_fb(zq, *args, do_km, do_ot, wv[4], wv[5])
        if b * D > 10240:                    # more than one chunk: outside the fused kernel's range, the caller falls back
            assert res is None
            return
        kmq, otq, dzq = res
        assert float(kmq) == float(kmp) and float(otq) == float(otp)
        assert torch.equal(dzq, zp.grad)
        torch.autograd.backward([kmq, otq], [wv[4], wv[5]])
        assert zq.grad is None
    zq = f32(z).requires_grad_(True)
    kmq, otq, _ = ops.cluster_losses_fb(zq, *args, True, True, wv[4], wv[5])
    with pytest.raises(RuntimeError, match="cluster_losses_fb"):
        torch.autograd.backward([kmq, otq], [wv[4].clone(), wv[5]])


def test_mix_losses(ops):
    w = torch.tensor([0.1, -0.4, 1e-4, 0.1, 0.1, 1.0], device=DEV)
    terms = [torch.tensor(v, device=DEV, requires_grad=(i != 4)) for i, v in enumerate([3.0, -2.0, 50.0, 0.25, 7.0, 0.5])]
    elbo, log7 = ops.mix_losses(w, terms)
    want = sum(float(a) * float(t) for a, t in zip(w, terms))
    assert float(elbo) == pytest.approx(want, rel=1e-6) and float(log7[0]) == float(elbo)
    assert [float(v) for v in log7[1:]] == [float(t) for t in terms] and not log7.requires_grad
    (2.0 * elbo).backward()
    for i, t in enumerate(terms):
        if i == 4:
            assert t.grad is None
        else:
            assert float(t.grad) == pytest.approx(2.0 * float(w[i]), rel=1e-6)


# ------------------------------------------------------------------ BASELINE.json full size (cfg3 batch graph)

def test_gat_edge_full_size_vs_torch_scatter(ops):
    """n = 10k nodes, k = 30 (+ self loops), H = 4, C = 512 (cfg3 layer shape): the HIP edge kernels (fp32)
    against an independent scatter-based formulation in plain torch, in fp64, forward and backward.
    A LeakyReLU pre-activation within fp32 rounding of 0 may take the other slope than the fp64 one; the
    rows such a tie feeds (found from the fp64 pre-activations) are left out of the gradient comparison,
    everything else has to agree to fp32 accuracy."""
    rng = np.random.default_rng(0)
    torch.manual_seed(1)
    n, H, C, k = 10000, 4, 512, 30
    from spadot_amd.graph import knn_graph
    ei = knn_graph(rng.uniform(size=(n, 2)), k)
    g = _graph(ei, n)
    assert g.E == n * (k + 1)
    h = (torch.randn((n, H * C), device=DEV) * 0.5).requires_grad_(True)
    s1 = (torch.randn((1, H, C), device=DEV) * 0.1).requires_grad_(True)      # att_src
    s2 = (torch.randn((1, H, C), device=DEV) * 0.1).requires_grad_(True)      # att_dst
    bias = (0.1 * torch.randn(H * C, device=DEV)).requires_grad_(True)
    out = ops.gat_edge(h, s1, s2, bias, g, H, C, True, True)
    w = torch.randn_like(out)
    (out * w).sum().backward()
    got = [t.grad.clone() for t in (h, s1, s2, bias)]
    # reference: explicit per-edge tensors + index_add (what a scatter-based GATConv does), fp64
    f64 = torch.float64
    hd, s1d, s2d, bd = (t.detach().to(f64).requires_grad_(True) for t in (h, s1, s2, bias))
    tgt = torch.repeat_interleave(torch.arange(n, device=DEV), (g.rowptr[1:] - g.rowptr[:-1]).long())
    src = g.col.long()
    hv = hd.view(n, H, C)
    pre = (hv * s1d).sum(-1)[src] + (hv * s2d).sum(-1)[tgt]
    e = torch.nn.functional.leaky_relu(pre, 0.2)
    emax = torch.full((n, H), -float("inf"), device=DEV, dtype=f64).scatter_reduce(
        0, tgt[:, None].expand(-1, H), e, "amax")
    ex = torch.exp(e - emax[tgt])
    den = torch.zeros((n, H), device=DEV, dtype=f64).index_add_(0, tgt, ex) + 1e-16
    alpha = ex / den[tgt]
    opre = torch.zeros((n, H, C), device=DEV, dtype=f64).index_add_(0, tgt, alpha[:, :, None] * hv[src])
    opre = opre.reshape(n, H * C) + bd
    ref = torch.nn.functional.leaky_relu(opre, 0.01)
    (ref * w.to(f64)).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().cpu().numpy(), rtol=2e-5, atol=2e-6)
    # rows a possible slope tie feeds: both ends of a tied edge; a tied output element's node and in-neighbours
    tie_e = (pre.detach().abs() < 2e-5).any(1)
    tie_o = (opre.detach().abs() < 5e-7).any(1)
    skip = torch.zeros(n, dtype=torch.bool, device=DEV)
    skip[src[tie_e]] = True
    skip[tgt[tie_e]] = True
    skip |= tie_o
    skip[src[tie_o[tgt]]] = True
    assert int(skip.sum()) < 0.25 * n
    keep = (~skip).cpu().numpy()
    for name, a, t in zip(("h", "att_src", "att_dst", "bias"), got, (hd, s1d, s2d, bd)):
        r, a = t.grad.cpu().numpy(), a.cpu().numpy().astype(np.float64)
        if name == "h":
            np.testing.assert_allclose(a[keep], r[keep], rtol=2e-4, atol=1e-5 * np.abs(r).max(), err_msg=name)
        else:       # sums over every edge / node: the ties stay in, each worth at most one term of the sum
            np.testing.assert_allclose(a, r, rtol=2e-3, atol=2e-3 * np.abs(r).max(), err_msg=name)
    # bitwise reproducible (no atomics in the HIP path)
    out2 = ops.gat_edge(h, s1, s2, bias, g, H, C, True, True)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("M,N,K", [(512, 64, 256), (512, 20, 64), (235, 33, 70), (1, 1, 1), (64, 256, 512)])
def test_sgemm_small_three_modes_match_fp64(ops, M, N, K):
    """csrc k_sgemm_small (the MLP stages' small fp32 products with a small footprint): y = x W^T + b, dx = g W, dW = g^T x
    against fp64, ragged sizes included; bitwise repeatable; and through the autograd functions that use it."""
    rng = np.random.default_rng(M + N + K)
    x = T(rng.normal(size=(M, K))).float().to(DEV); W = T(rng.normal(size=(N, K))).float().to(DEV)
    b = T(rng.normal(size=N)).float().to(DEV); g = T(rng.normal(size=(M, N))).float().to(DEV)
    with pytest.raises(RuntimeError):
        ops.sgemm_small(1, x.cpu(), W, b)                       # a host tensor is refused before anything is launched
    y = ops.sgemm_small(1, x, W, b)
    np.testing.assert_allclose(y.cpu().numpy(), (x.double() @ W.double().T + b.double()).cpu().numpy(), rtol=2e-5, atol=2e-5 * K ** 0.5)
    dx = ops.sgemm_small(0, g, W)
    np.testing.assert_allclose(dx.cpu().numpy(), (g.double() @ W.double()).cpu().numpy(), rtol=2e-5, atol=2e-5 * N ** 0.5)
    dW = ops.sgemm_small(2, g, x)
    np.testing.assert_allclose(dW.cpu().numpy(), (g.double().T @ x.double()).cpu().numpy(), rtol=2e-5, atol=2e-5 * M ** 0.5)
    assert torch.equal(dW, ops.sgemm_small(2, g, x))
    dWs = ops.wgrad_small(g, x)                                     # row slices in one launch + a fixed-order sum
    np.testing.assert_allclose(dWs.cpu().numpy(), (g.double().T @ x.double()).cpu().numpy(), rtol=2e-5, atol=2e-5 * M ** 0.5)
    assert torch.equal(dWs, ops.wgrad_small(g, x))
    # autograd: hidden_map gives the library's values and gradients
    xr = x.clone().requires_grad_(True); Wr = W.clone().requires_grad_(True)
    (ops.hidden_map(xr, Wr) * g).sum().backward()
    np.testing.assert_allclose(xr.grad.cpu().numpy(), dx.cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(Wr.grad.cpu().numpy(), (g.double().T @ x.double()).cpu().numpy(), rtol=2e-5, atol=2e-5 * M ** 0.5)
