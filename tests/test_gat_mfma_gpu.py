"""GPU: the matrix-core GAT edge kernels (csrc/gat_mfma.hip, bf16 rows, block plans) against
  (a) the per-edge kernels of model_kernels.hip on the same inputs (what they replace: same arithmetic, other order), and
  (b) an independent fp64 scatter formulation of GATConv's message passing.
Tolerances: outputs are bf16 (8 significant bits, rtol 2^-7 on a value, the same rounding in both HIP paths); the weights
keep 16 bits (bf16 hi + lo), accumulation is fp32 -- so the two HIP paths agree to bf16 output rounding, and gradients of
parameters (sums over all nodes) to ~1e-2."""
import numpy as np
import pytest
import torch

import gat_cases
import gat_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from spadot_amd import ops
    return ops


def _problem(n, k, hub, seed, n_tgt=None, spatial=True):
    from spadot_amd.graph import attach_plans, build_batch_graph, knn_graph, morton_key
    rng = np.random.default_rng(seed)
    coords = rng.uniform(size=(n, 2)) * np.sqrt(n)
    ei = knn_graph(coords, k)
    if hub:        # node 5 hears from everybody: in-degree n (a column list far longer than one chunk)
        extra = np.stack([np.arange(n), np.full(n, 5)])
        ei = np.unique(np.concatenate([ei, extra], axis=1), axis=1)
    if n_tgt is not None:                    # only the first n_tgt nodes are targets (layer-2 shape)
        ei = ei[:, ei[1] < n_tgt]
        from spadot_amd.graph import _csr_both
        from spadot_amd.ops import BatchGraph
        src, dst = ei[0], ei[1]
        keep = src != dst
        src = np.concatenate([src[keep], np.arange(n_tgt)]); dst = np.concatenate([dst[keep], np.arange(n_tgt)])
        g = BatchGraph(n, *(torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in _csr_both(src, dst, n, n_tgt)), n_tgt=n_tgt)
    else:
        g = build_batch_graph(ei, n, DEV)
    attach_plans(g, morton_key(coords) if spatial else None)
    assert g.plan_t is not None and g.plan_s is not None
    return g


def _inputs(g, H, C, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    h = (torch.randn((g.n, H * C), device=DEV, generator=gen) * 0.5).bfloat16()
    a_s = torch.randn((1, H, C), device=DEV, generator=gen) * 0.1
    a_d = torch.randn((1, H, C), device=DEV, generator=gen) * 0.1
    bias = 0.1 * torch.randn(H * C, device=DEV, generator=gen)
    w = torch.randn((g.n_tgt, H * C), device=DEV, generator=gen).bfloat16()
    return h, a_s, a_d, bias, w


def _run(ops, g, h, a_s, a_d, bias, w, H, C, act, mfma):
    ops.GAT_MFMA[0] = mfma
    try:
        t = [x.clone().requires_grad_(True) for x in (h, a_s, a_d, bias)]
        out = ops.gat_edge(t[0], t[1], t[2], t[3], g, H, C, True, act)
        (out.float() * w.float()).sum().backward()
        return out.detach(), [x.grad.detach().float() for x in t]
    finally:
        ops.GAT_MFMA[0] = True


@pytest.mark.parametrize("n,k,H,C,act,hub,n_tgt,spatial", [
    (97, 7, 4, 512, True, False, None, True),          # fewer rows than one block of 32 x 4
    (300, 9, 2, 512, False, True, None, True),         # a hub: 300 columns in one block (in-degree 300: 5 softmax passes)
    (1000, 30, 4, 512, True, False, None, True),       # the layer shape
    (1000, 30, 4, 512, True, False, 400, True),        # layer-2 shape: targets are a prefix of the nodes
    (500, 12, 8, 512, False, False, None, False),      # no spatial order: long column lists, many chunks; 8 heads
    (33, 4, 1, 512, True, False, None, True),          # one full block + one row; a single head
])
def test_mfma_path_matches_per_edge_kernels(ops, n, k, H, C, act, hub, n_tgt, spatial):
    g = _problem(n, k, hub, seed=n + C, n_tgt=n_tgt, spatial=spatial)
    h, a_s, a_d, bias, w = _inputs(g, H, C, seed=3)
    assert ops._mfma_plans(h, g, H, C, True) is not None
    out_m, gr_m = _run(ops, g, h, a_s, a_d, bias, w, H, C, act, True)
    out_e, gr_e = _run(ops, g, h, a_s, a_d, bias, w, H, C, act, False)
    assert torch.isfinite(out_m.float()).all()
    # forward: same bf16 rounding of the same fp32 sums (other summation order): at most one bf16 ulp apart
    np.testing.assert_allclose(out_m.float().cpu().numpy(), out_e.float().cpu().numpy(), rtol=2 ** -7, atol=1e-3)
    # dh is bf16 too; att / bias gradients are fp32 sums over all nodes of bf16-rounded terms
    for name, a, b in zip(("h", "att_src", "att_dst", "bias"), gr_m, gr_e):
        a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
        scale = np.abs(b).max() + 1e-30
        if name == "h":
            # element-wise, except where an output within rounding of 0 took the other LeakyReLU slope in one of the two
            # summation orders (act = True: a handful of elements out of millions, each worth one term of one row)
            bad = np.abs(a - b) > 2 ** -6 * np.abs(b) + 4e-3 * scale
            assert bad.sum() <= max(2, 1e-5 * bad.size) if act else not bad.any(), (name, int(bad.sum()), np.abs(a - b).max())
            assert np.linalg.norm(a - b) <= 5e-3 * np.linalg.norm(b), (name, np.linalg.norm(a - b) / np.linalg.norm(b))
        else:
            assert np.linalg.norm(a - b) <= 1e-2 * np.linalg.norm(b) + 1e-6, (name, np.linalg.norm(a - b), np.linalg.norm(b))
    # deterministic: no atomics, fixed order
    out_m2, gr_m2 = _run(ops, g, h, a_s, a_d, bias, w, H, C, act, True)
    assert torch.equal(out_m, out_m2) and all(torch.equal(a, b) for a, b in zip(gr_m, gr_m2))


def test_mfma_path_full_size_vs_fp64_scatter(ops):
    """cfg3 layer shape (10k nodes, k = 30 + self loops, H = 4, C = 512, bf16 rows) against the fp64 scatter formulation
    evaluated on the SAME bf16-rounded inputs: what is checked is the kernels' own error (bf16 output rounding), not
    the input quantisation."""
    from spadot_amd.graph import attach_plans, build_batch_graph, knn_graph, morton_key
    rng = np.random.default_rng(0)
    n, H, C, k = 10000, 4, 512, 30
    side = int(np.sqrt(n))
    coords = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2) + rng.uniform(-0.3, 0.3, (n, 2))
    coords = coords[rng.permutation(n)]
    g = attach_plans(build_batch_graph(knn_graph(coords, k), n, DEV), morton_key(coords))
    assert g.E == n * (k + 1) and g.plan_t.avg_cols < 200
    h, a_s, a_d, bias, w = _inputs(g, H, C, seed=1)
    out, grads = _run(ops, g, h, a_s, a_d, bias, w, H, C, True, True)
    hd, s1d, s2d, bd = gat_ref.leaves(h, a_s, a_d, bias)
    ref = gat_ref.gat_edge(hd, s1d, s2d, bd, g.rowptr, g.col, H, C, True, True)           # the fp64 scatter formulation, on the device
    (ref * w.to(torch.float64)).sum().backward()
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.detach().cpu().numpy(), rtol=2 ** -8, atol=1e-4)
    for name, a, t in zip(("h", "att_src", "att_dst", "bias"), grads, (hd, s1d, s2d, bd)):
        r, a = t.grad.cpu().numpy(), a.cpu().numpy().astype(np.float64)
        rel = np.linalg.norm(a - r) / np.linalg.norm(r)
        assert rel <= (6e-3 if name == "h" else 2e-2), (name, rel)


# ------------------------------------------------------------------------------------------------------------------
# The plan and degree edges of the kernels, on graphs built for them (tests/gat_cases.py; each case's property is asserted on
# the host in tests/test_gat_ref_cpu.py).  Blocks follow the node numbering.

def _fp64(g, h, a_s, a_d, bias, w, H, C, act):
    """(out, [dh, datt_src, datt_dst, dbias]) of tests/gat_ref.py on the same bf16-rounded inputs, in fp64 on the device.
    h may carry pad rows (their gradient is 0); w covers at least the targets' rows."""
    lv = gat_ref.leaves(h, a_s, a_d, bias)
    ref = gat_ref.gat_edge(*lv, g.rowptr, g.col, H, C, True, act)
    (ref * w[:g.n_tgt].to(torch.float64)).sum().backward()
    return ref.detach(), [t.grad for t in lv]


def _check_case(ops, g, H, act, pad=0, expect_mfma=True, seed=3):
    C = 512
    n, nt = g.n, g.n_tgt
    h, a_s, a_d, bias, _ = _inputs(g, H, C, seed=seed)
    gen = torch.Generator(device=DEV).manual_seed(seed + 100)
    if pad:                       # rows past the last node: never read (finite but huge, so that a read would show)
        h = torch.cat([h, torch.full((pad, H * C), 1.0e4, device=DEV, dtype=h.dtype)])
    out_rows = n + pad if (nt == n and pad <= 4096 and expect_mfma) else nt
    w = torch.randn((max(out_rows, nt), H * C), device=DEV, generator=gen).bfloat16()
    assert (ops._mfma_plans(h, g, H, C, True) is not None) == expect_mfma
    out_m, gr_m = _run(ops, g, h, a_s, a_d, bias, w[:out_rows], H, C, act, True)
    out_e, gr_e = _run(ops, g, h, a_s, a_d, bias, w[:nt], H, C, act, False)
    assert out_m.shape[0] == out_rows and out_e.shape[0] == nt
    ref, gr_r = _fp64(g, h, a_s, a_d, bias, w, H, C, act)
    # forward, element-wise against fp64 (the bound test_mfma_path_full_size_vs_fp64_scatter holds at the layer shape)
    for o in (out_m, out_e):
        assert torch.isfinite(o.float()).all()
        np.testing.assert_allclose(o[:nt].float().cpu().numpy(), ref.cpu().numpy(), rtol=2 ** -8, atol=1e-4)
    if out_rows > nt:
        assert float(out_m[nt:].float().abs().max()) == 0.0, "pad rows of the output must be zero"
    if pad:
        assert float(gr_m[0][n:].abs().max()) == 0.0 and float(gr_e[0][n:].abs().max()) == 0.0, "pad rows of h: zero gradient"
    # dh element-wise against the per-edge kernels (bound and kink allowance of test_mfma_path_matches_per_edge_kernels)
    a, b = gr_m[0][:n].cpu().numpy().astype(np.float64), gr_e[0][:n].cpu().numpy().astype(np.float64)
    bad = np.abs(a - b) > 2 ** -6 * np.abs(b) + 4e-3 * (np.abs(b).max() + 1e-30)
    assert bad.sum() <= max(2, 1e-5 * bad.size) if act else not bad.any(), (int(bad.sum()), np.abs(a - b).max())
    # every gradient: no further from fp64 than twice the per-edge kernels (+ the floor of tests/test_gat_tail_gpu.py);
    # attention-vector gradients stay on this norm convention
    for name, m_, e_, r_ in zip(("h", "att_src", "att_dst", "bias"), gr_m, gr_e, gr_r):
        rows = n if name == "h" else m_.shape[0]
        rm, re = gat_ref.rel_l2(m_[:rows], r_[:rows].reshape(m_[:rows].shape)), gat_ref.rel_l2(e_[:rows], r_[:rows].reshape(e_[:rows].shape))
        print("%-8s rel-L2 vs fp64: matrix-core %.3e, per-edge %.3e" % (name, rm, re))
        assert rm <= 2.0 * re + 5e-3, (name, rm, re)
    print("out      rel-L2 vs fp64: matrix-core %.3e, per-edge %.3e" % (gat_ref.rel_l2(out_m[:nt], ref), gat_ref.rel_l2(out_e[:nt], ref)))
    assert gat_ref.rel_l2(out_m[:nt], ref) <= 2.0 * gat_ref.rel_l2(out_e[:nt], ref) + 1e-3
    # deterministic
    out_m2, gr_m2 = _run(ops, g, h, a_s, a_d, bias, w[:out_rows], H, C, act, True)
    assert torch.equal(out_m, out_m2) and all(torch.equal(x, y) for x, y in zip(gr_m, gr_m2))


def test_mfma_longest_accepted_column_list(ops):
    """32 targets x 31 distinct sources (self loop included): 992 columns = agg::MAXC, 62 chunks through the LDS ring."""
    g = gat_cases.column_limit(30).graph(DEV)
    assert g.plan_t.max_cols == 992
    _check_case(ops, g, 4, True)


def test_mfma_refuses_1024_columns_and_the_per_edge_path_takes_over(ops):
    """One column more per target: spadot_gat_mfma_supported says no, _mfma_plans returns None, gat_edge runs the per-edge kernels
    -- and the result is still the fp64 reference's."""
    g = gat_cases.column_limit(31).graph(DEV)
    assert g.plan_t is not None and g.plan_t.max_cols == 1024
    from spadot_amd import _lib
    assert _lib.model_lib().spadot_gat_mfma_supported(ops.DT_BF16, 4, 512, 1024) == 0
    assert _lib.model_lib().spadot_gat_mfma_supported(ops.DT_BF16, 4, 512, 992) == 1
    _check_case(ops, g, 4, True, expect_mfma=False)


@pytest.mark.parametrize("H,act", [(4, True), (1, False)])
def test_mfma_blocks_of_2_and_4_chunks(ops, H, act):
    """Blocks with exactly 32, 48 and 64 distinct columns: lists of 2, 4 and 4 chunks (48 is padded to 64) -- fewer chunks
    than, as many as and more than the ring holds, for a ring of 2 or 3."""
    g = gat_cases.chunk_blocks().graph(DEV)
    sp = g.plan_t.sptr.tolist()
    assert [sp[b + 1] - sp[b] for b in range(3)] == [32, 64, 64]
    _check_case(ops, g, H, act)


@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_mfma_in_degrees_around_the_four_register_passes(ops, H):
    """In-degree 256 // H (the last of the four passes k_gat_alpha / k_gat_softmax_bwd keep in registers), 256 // H + 1 (one
    edge in the loop behind them) and 1 (the self loop only)."""
    c = gat_cases.degree_limit(H)
    g = c.graph(DEV)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).tolist()
    assert deg[:3] == [256 // H, 256 // H + 1, 1]
    _check_case(ops, g, H, H != 2)


@pytest.mark.parametrize("H", [1, 4])
def test_mfma_grid_rounded_up_and_plans_of_different_length(ops, H):
    """nb * H no multiple of 8 (the grid is rounded up to 8: idle workgroups), targets a prefix of the nodes: the by-source plan
    has more blocks than the by-target plan, which leaves rows of the shared partial matrix untouched."""
    g = gat_cases.ragged_blocks().graph(DEV)
    assert g.plan_s.nb > g.plan_t.nb and (g.plan_t.nb * H) % 8 and (g.plan_s.nb * H) % 8
    _check_case(ops, g, H, True)


@pytest.mark.parametrize("pad", [5, 4097])
def test_mfma_row_padding_of_h(ops, pad):
    """h with 5 pad rows: the output carries them, written as zeros by the kernel, and so does dh.  With 4097 (more than the
    kernels clear themselves) the output has n_tgt rows and dh[n:] is cleared by the host.  Either way dh[n:] == 0."""
    g = gat_cases.small_all_targets().graph(DEV)
    _check_case(ops, g, 4, True, pad=pad)
