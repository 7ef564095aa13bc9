"""GPU: the premasked-gradient handoff of the GAT encoder's backward pass, through autograd.

A gat_edge(act=True, act_cell=c) shares the dict c with the op that consumes its output (dense_cd / gat_tail, in_cell=c).  That
consumer holds the activated output as its input, so its backward multiplies the gradient it hands back by LeakyReLU'(out) as it
produces it -- the mask epilogue of k_gemm_bf16<true> (spadot_gemm_nn_bf16_masked) resp. the `msk` argument of k_tail_src_bwd --
and sets c["premasked"]; the producer's backward then skips its own masking (act_here = 0, g_pre = g_out).

Each chain runs twice on identical inputs, with the shared cell (fused) and with act_cell = in_cell = None (unfused: the
consumer hands back the plain gradient, the producer's k_gat_edot masks it).  The mask comes from the same bits of `out` in
both runs, so no element near the activation's kink is excluded anywhere.  Both runs are also held to tests/gat_ref.py's fp64
chains on the same bf16-rounded inputs: the fused path may be no further from fp64 than twice the unfused path plus the floors of
tests/test_gat_tail_gpu.py (1e-3 outputs, 5e-3 gradients).  The graphs are tests/gat_cases.py's, their properties asserted
on the host in tests/test_gat_ref_cpu.py."""
import numpy as np
import pytest
import torch

import gat_cases
import gat_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, C = 4, 512                    # the producer: bf16 rows, the matrix-core edge kernels
SLOPE = 0.01


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from spadot_amd import ops
    return ops


class _Holder:
    """Keeps a dense map's bf16 weight image between calls (ops.weight_image)."""


def _layer(gen, heads, channels, concat, scale):
    a_s = torch.randn((1, heads, channels), device=DEV, generator=gen) * scale
    a_d = torch.randn((1, heads, channels), device=DEV, generator=gen) * scale
    bias = 0.1 * torch.randn(heads * channels if concat else channels, device=DEV, generator=gen)
    return [a_s, a_d, bias]


def _leaf(t):
    return t.clone().requires_grad_(True)


def _masked(dx, out):
    """What the producer's own masking makes of the plain gradient: bf16(float(dx) * slope) where out <= 0."""
    slope = torch.tensor(SLOPE, dtype=torch.float32, device=dx.device)
    return torch.where(out > 0, dx, (dx.float() * slope).bfloat16())


def _ordinal(t):
    """bf16 -> int32 that counts representable values in order (+0.0 and -0.0 both 0): |difference| = distance in ulps."""
    i = t.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _watch(out1, cell, seen, mid):
    """Tensor hook on the intermediate: runs between the consumer's and the producer's backward node."""
    def hook(grad):
        seen.append(cell is not None and cell.get("premasked") is True)
        mid["dx"] = grad.detach().clone()
    out1.register_hook(hook)


def _report(tag, names, fused, unfused, ref, floor):
    for name, f_, u_, r_ in zip(names, fused, unfused, ref):
        ef, eu = gat_ref.rel_l2(f_, r_.reshape(f_.shape)), gat_ref.rel_l2(u_, r_.reshape(u_.shape))
        print("%s %-9s rel-L2 vs fp64: fused %.3e, unfused %.3e" % (tag, name, ef, eu))
        assert ef <= 2.0 * eu + floor, (tag, name, ef, eu)


NAMES = ("h", "att_src1", "att_dst1", "bias1", "W", "att_src2", "att_dst2", "bias2")


def test_handoff_into_a_dense_map_is_bit_identical_to_the_producers_own_masking(ops):
    """gat_edge(act, act_cell=c) -> dense_cd(in_cell=c) -> gat_edge -> weighted sum, 2600 nodes (all targets; no multiple of the
    GEMM's 320-row panel) + 5 pad rows of h, 2048 -> 2048 channels: the (2605, 2048, 2048) masked input-gradient GEMM.
    ops.GEMM_DGRAD_MIN_WGS only gates on speed (72 tiles here): lowered for the test, so that both runs take the own GEMM.
    Both runs round g W to bf16 and THEN scale and round again (the GEMM's mask epilogue works on the rounded patch, like
    k_gat_edot on the rounded gradient it loads): every output and every gradient is asserted BIT-IDENTICAL.
    Measured (MI355X): bit-identical.  rel-L2 against fp64, the same number for fused and unfused: out1 1.66e-3, out2 2.12e-3,
    dh 8.9e-3, att_src1 8.4e-3, att_dst1 9.7e-3, bias1 5.5e-3, dW 6.1e-3, att_src2 2.8e-2, att_dst2 8.6e-2, bias2 3.7e-8."""
    case = gat_cases.handoff_dense()
    g = case.graph(DEV)
    n, pad = case.n, 5
    assert ops._mfma_plans(torch.empty((1, H * C), dtype=torch.bfloat16, device=DEV), g, H, C, True) is not None
    gen = torch.Generator(device=DEV).manual_seed(21)
    h = (torch.randn((n + pad, H * C), device=DEV, generator=gen) * 0.5).bfloat16()
    h[n:] = 1.0e4                                    # pad rows: never read (a read would show)
    p1, p2 = _layer(gen, H, C, True, 0.1), _layer(gen, H, C, True, 0.1)
    W = (torch.randn((H * C, H * C), device=DEV, generator=gen) * 0.03).bfloat16().float()        # bf16-representable
    w = torch.randn((n + pad, H * C), device=DEV, generator=gen).bfloat16()

    def run(fused):
        cell = {} if fused else None
        seen, mid = [], {}
        lv = [_leaf(h)] + [_leaf(t) for t in p1] + [_leaf(W)] + [_leaf(t) for t in p2]
        out1 = ops.gat_edge(lv[0], lv[1], lv[2], lv[3], g, H, C, True, True, act_cell=cell)
        _watch(out1, cell, seen, mid)
        d = ops.dense_cd(out1, lv[4], _Holder(), in_cell=cell)
        out2 = ops.gat_edge(d, lv[5], lv[6], lv[7], g, H, C, True, False)
        (out2.float() * w.float()).sum().backward()
        torch.cuda.synchronize()
        return out1.detach(), out2.detach(), mid["dx"], [t.grad.detach() for t in lv], seen

    keep = ops.GEMM_DGRAD_MIN_WGS
    ops.GEMM_DGRAD_MIN_WGS = 1
    try:
        o1f, o2f, dxf, gf, seen_f = run(True)
        o1u, o2u, dxu, gu, seen_u = run(False)
    finally:
        ops.GEMM_DGRAD_MIN_WGS = keep
    assert seen_f == [True], "the masked GEMM did not run: the handoff was not taken"
    assert seen_u == [False]
    # pad rows: zero output, zero gradient coming back, zero gradient going on
    assert o1f.shape == (n + pad, H * C) and float(o1f[n:].float().abs().max()) == 0.0
    for dx in (dxf, dxu):
        assert dx.shape == o1f.shape and float(dx[n:].float().abs().max()) == 0.0
    assert float(gf[0][n:].float().abs().max()) == 0.0 and float(gu[0][n:].float().abs().max()) == 0.0
    # fused == unfused, bit for bit
    assert torch.equal(o1f, o1u) and torch.equal(o2f, o2u)
    want = _masked(dxu, o1u)
    diff = dxf.view(torch.int16) != want.view(torch.int16)
    assert not bool(diff.any()), ("dx", int(diff.sum()), torch.nonzero(diff)[:8].tolist())
    for name, a, b in zip(NAMES, gf, gu):
        assert a.dtype == b.dtype and torch.equal(a, b), (name, int((a != b).sum()), float((a.float() - b.float()).abs().max()))
    # both against fp64
    rl = gat_ref.leaves(h[:n], *p1, W, *p2)
    r1, r2, loss = gat_ref.chain_dense(rl[0], rl[1:4], rl[4], rl[5:8], (g.rowptr, g.col), H, C, w[:n].to(torch.float64))
    loss.backward()
    _report("dense", ("out1", "out2"), (o1f[:n], o2f[:n]), (o1u[:n], o2u[:n]), (r1, r2), 1e-3)
    _report("dense", NAMES, [gf[0][:n]] + gf[1:], [gu[0][:n]] + gu[1:], [t.grad for t in rl], 5e-3)


def test_handoff_into_the_tail_masks_in_both_branches_of_the_source_backward(ops):
    """gat_edge(act, act_cell=c) on 900 nodes with the first 658 as targets -> gat_tail(in_cell=c) on gat_cases.tail_hub()
    (658 source rows, 163 targets, K = 2048, H = 4, C = 16): two 8-row source blocks with more than 128 out-edges take
    k_tail_src_bwd's unstaged branch, the others the staged one, and both must apply the mask.
    The fused kernel scales its fp32 sum and rounds once; the unfused path rounds the sum, scales and rounds again: dx is
    bit-identical where out > 0 and within ONE bf16 ulp where it is scaled.  Behind that, every element of the producer's
    g_pre differs by at most 2^-8 relative in half of the elements -- dh is held to the element-wise bound of
    tests/test_gat_mfma_gpu.py between two summation orders (2^-6 |b| + 4e-3 max |b|, no exceptions: the mask bits are the same),
    the parameter gradients (sums over all nodes) to 1e-2 of their norm.
    Measured (MI355X), rel-L2 against fp64, fused / unfused: out1 1.661e-3 / same, out2 2.161e-3 / same, dh 3.675e-3 / 3.676e-3,
    att_src1 3.284e-3 / 3.282e-3, att_dst1 3.065e-3 / 3.070e-3, bias1 1.758e-3 / same, dW 1.794e-3 / same,
    att_src2 8.95e-3 / same, att_dst2 1.98e-2 / same, bias2 9.8e-4 / same."""
    cp, ct = gat_cases.handoff_producer(), gat_cases.tail_hub()
    gp, gt = cp.graph(DEV), ct.graph(DEV, plans=False)
    H2, C2, K = 4, 16, H * C
    assert ops._mfma_plans(torch.empty((1, K), dtype=torch.bfloat16, device=DEV), gp, H, C, True) is not None
    gen = torch.Generator(device=DEV).manual_seed(22)
    h = (torch.randn((cp.n, K), device=DEV, generator=gen) * 0.5).bfloat16()
    p1, p2 = _layer(gen, H, C, True, 0.1), _layer(gen, H2, C2, False, 0.3)
    W = (torch.randn((H2 * C2, K), device=DEV, generator=gen) / np.sqrt(K)).bfloat16().float()
    w = torch.randn((ct.n_tgt, C2), device=DEV, generator=gen)

    def run(fused):
        cell = {} if fused else None
        seen, mid = [], {}
        lv = [_leaf(h)] + [_leaf(t) for t in p1] + [_leaf(W)] + [_leaf(t) for t in p2]
        out1 = ops.gat_edge(lv[0], lv[1], lv[2], lv[3], gp, H, C, True, True, act_cell=cell)
        _watch(out1, cell, seen, mid)
        assert out1.shape == (ct.n, K) and ops.gat_tail_ok(out1, lv[4], gt, H2, C2, False)
        out2 = ops.gat_tail(out1, lv[4], lv[4].detach().to(torch.bfloat16).contiguous(), lv[5], lv[6], lv[7], gt, H2, C2, in_cell=cell)
        (out2.float() * w).sum().backward()
        torch.cuda.synchronize()
        return out1.detach(), out2.detach(), mid["dx"], [t.grad.detach() for t in lv], seen

    o1f, o2f, dxf, gf, seen_f = run(True)
    o1u, o2u, dxu, gu, seen_u = run(False)
    assert seen_f == [True] and seen_u == [False]
    assert torch.equal(o1f, o1u)
    np.testing.assert_allclose(o2f.float().cpu().numpy(), o2u.float().cpu().numpy(), rtol=2 ** -7, atol=1e-6)
    # dx: the same bits where nothing is scaled, one bf16 ulp where the two paths round once / twice
    want = _masked(dxu, o1u)
    kept = o1u > 0
    assert bool(kept.any()) and bool((~kept).any())
    assert torch.equal(dxf[kept], want[kept])
    ulps = (_ordinal(dxf) - _ordinal(want)).abs()
    rows_bad = torch.nonzero((ulps > 1).any(dim=1)).flatten().tolist()
    assert not rows_bad, ("dx rows off by more than one ulp (hub blocks: rows %s)" % [8 * (x // 8) for x in ct.marks["hubs"]], rows_bad[:16])
    for name, a, b in zip(NAMES, gf, gu):
        a, b = a.float().cpu().numpy().astype(np.float64), b.float().cpu().numpy().astype(np.float64)
        if name == "h":
            bad = np.abs(a - b) > 2 ** -6 * np.abs(b) + 4e-3 * (np.abs(b).max() + 1e-30)
            assert not bad.any(), (name, int(bad.sum()), np.abs(a - b).max())
        else:
            assert np.linalg.norm(a - b) <= 1e-2 * np.linalg.norm(b) + 1e-6, (name, np.linalg.norm(a - b), np.linalg.norm(b))
    # both against fp64
    rl = gat_ref.leaves(h, *p1, W, *p2)
    r1, r2, loss = gat_ref.chain_tail(rl[0], rl[1:4], (gp.rowptr, gp.col), H, C, rl[4], rl[5:8], (gt.rowptr, gt.col), H2, C2,
                                      w.to(torch.float64))
    loss.backward()
    _report("tail", ("out1", "out2"), (o1f, o2f), (o1u, o2u), (r1, r2), 1e-3)
    _report("tail", NAMES, gf, gu, [t.grad for t in rl], 5e-3)
