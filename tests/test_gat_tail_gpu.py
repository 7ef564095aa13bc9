"""GPU: the last GAT layer for the seeds only in its aggregate-first form (csrc/gat_tail.hip, ops.gat_tail) against
(a) the fp64 oracle's gat_conv (oracle/model_oracle.py: PyG GATConv semantics) restricted to the seed rows,
(b) the map-first path it replaces (dense map over all source rows + ops.gat_edge), at the benchmarked layer shape in bf16.
encoder.py:45,58 of the reference: gat3 = GATConv(4 * 512 -> 512, heads = 4, concat = False), seeds' rows only (SpaDOT.py:82)."""
import numpy as np
import pytest
import torch

from oracle import model_oracle as mo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def T(x, dtype=F64):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def _problem(n, rows, k, H, C, K, seed, hub=True, pad=0):
    rng = np.random.default_rng(seed)
    ei = mo.knn_graph(rng.uniform(size=(n, 2)), k).numpy()
    if hub:      # target 3 receives an edge from every node (in-degree > 64: several edge chunks); target 1 keeps only its self loop
        extra = np.stack([np.arange(n), np.full(n, 3)])
        ei = np.unique(np.concatenate([ei, extra], axis=1), axis=1)
        ei = ei[:, ~((ei[1] == 1) & (ei[0] != 1))]
    x = rng.normal(size=(n, K)) * 0.7
    W = rng.normal(size=(H * C, K)) / np.sqrt(K)
    a_s = rng.normal(size=(1, H, C)) * 0.3
    a_d = rng.normal(size=(1, H, C)) * 0.3
    bias = rng.normal(size=C) * 0.1
    gsel = rng.normal(size=(rows, C))
    return torch.as_tensor(ei), x, W, a_s, a_d, bias, gsel


def _oracle(ei, x, W, a_s, a_d, bias, gsel, H, rows):
    leaves = [T(t).clone().requires_grad_(True) for t in (x, W, a_s, a_d, bias)]
    out = mo.gat_conv(leaves[0], ei, leaves[1], leaves[2], leaves[3], leaves[4], H, False)[:rows]
    (out * T(gsel)).sum().backward()
    return out.detach().numpy(), [t.grad.numpy() for t in leaves]


def _tail(ops, ei, x, W, a_s, a_d, bias, gsel, H, C, rows, dt, pad=0):
    from spadot_amd.graph import build_batch_graph
    n, K = x.shape
    g = build_batch_graph(ei, n, DEV, seeds=rows).seed_graph
    assert g.n == n and g.n_tgt == rows
    xd = torch.zeros((n + pad, K), dtype=dt, device=DEV)
    xd[:n] = T(x).to(DEV, dt)
    xd.requires_grad_(True)
    Wd, asd, add_, bd = (T(t).to(DEV, torch.float32).requires_grad_(True) for t in (W, a_s, a_d, bias))
    wimg = None
    if dt != torch.float32:
        wimg = Wd.detach().to(dt).contiguous()
    assert ops.gat_tail_ok(xd, Wd, g, H, C, False)
    out = ops.gat_tail(xd, Wd, wimg, asd, add_, bd, g, H, C)
    (out.float() * T(gsel).to(DEV, torch.float32)).sum().backward()
    torch.cuda.synchronize()
    return out.detach().float().cpu().numpy(), [t.grad.detach().float().cpu().numpy() for t in (xd, Wd, asd, add_, bd)]


@pytest.mark.parametrize("n,rows,k,H,C,K", [(300, 40, 7, 4, 16, 64), (900, 64, 9, 4, 64, 256), (500, 33, 6, 1, 24, 40),
                                            (700, 50, 8, 2, 32, 128), (400, 30, 5, 8, 8, 64), (1500, 128, 12, 4, 512, 2048)])
def test_tail_fp32_matches_the_fp64_oracle(n, rows, k, H, C, K):
    from spadot_amd import ops
    ei, x, W, a_s, a_d, bias, gsel = _problem(n, rows, k, H, C, K, seed=n + H)
    out_o, grads_o = _oracle(ei, x, W, a_s, a_d, bias, gsel, H, rows)
    out_d, grads_d = _tail(ops, ei, x, W, a_s, a_d, bias, gsel, H, C, rows, torch.float32, pad=5)
    np.testing.assert_allclose(out_d, out_o, rtol=1e-4, atol=2e-5)
    for name, d, o in zip(("x", "W", "att_src", "att_dst", "bias"), grads_d, grads_o):
        if name == "x":
            assert np.all(d[n:] == 0.0), "pad rows of the input must get a zero gradient"
            d = d[:n]
        np.testing.assert_allclose(d, o, rtol=2e-3, atol=2e-4 * np.abs(o).max(), err_msg=name)


def test_tail_is_bitwise_repeatable_and_handles_padded_columns():
    from spadot_amd import ops
    n, rows, k, H, C, K = 600, 48, 8, 4, 32, 120
    ei, x, W, a_s, a_d, bias, gsel = _problem(n, rows, k, H, C, K, seed=5)
    a = _tail(ops, ei, x, W, a_s, a_d, bias, gsel, H, C, rows, torch.float32)
    b = _tail(ops, ei, x, W, a_s, a_d, bias, gsel, H, C, rows, torch.float32)
    assert np.array_equal(a[0], b[0])
    for u, v in zip(a[1], b[1]):
        assert np.array_equal(u, v)
    # input rows with zero pad columns (K = 120 stored in rows of 128): same output, zero gradient in the pad columns
    from spadot_amd.graph import build_batch_graph
    g = build_batch_graph(ei, n, DEV, seeds=rows).seed_graph
    xp = torch.zeros((n, 128), dtype=torch.float32, device=DEV)
    xp[:, :K] = T(x).to(DEV, torch.float32)
    xp.requires_grad_(True)
    Wd, asd, add_, bd = (T(t).to(DEV, torch.float32).requires_grad_(True) for t in (W, a_s, a_d, bias))
    out = ops.gat_tail(xp, Wd, None, asd, add_, bd, g, H, C)
    (out * T(gsel).to(DEV, torch.float32)).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), a[0], rtol=1e-6, atol=1e-6)
    assert float(xp.grad[:, K:].abs().max()) == 0.0
    np.testing.assert_allclose(xp.grad[:, :K].cpu().numpy(), a[1][0], rtol=1e-5, atol=1e-6)


def test_tail_bf16_at_the_benchmarked_layer_shape_vs_oracle_and_vs_the_map_first_path():
    """8 000 source rows x 2048 channels, 512 seeds, ~31 incoming edges each, H = 4, C = 512 in bf16: the aggregate-first
    result against the fp64 oracle (bf16-level tolerances, written here) and against the map-first path on the same inputs
    (dense map over all rows + per-edge kernels); both paths must sit equally close to the oracle."""
    n, rows, k, H, C, K = 8000, 512, 30, 4, 512, 2048
    _bf16_vs_oracle_and_map_first(rows, H, C, *_problem(n, rows, k, H, C, K, seed=77, hub=False))


def _bf16_vs_oracle_and_map_first(rows, H, C, ei, x, W, a_s, a_d, bias, gsel, pad=0):
    from spadot_amd import ops
    from spadot_amd.graph import build_batch_graph
    n = x.shape[0]
    # bf16-representable inputs, so that the comparison sees the kernels' arithmetic and not the input rounding
    x = T(x).to(torch.bfloat16).double().numpy()
    W = T(W).to(torch.bfloat16).double().numpy()
    out_o, grads_o = _oracle(ei, x, W, a_s, a_d, bias, gsel, H, rows)
    out_t, grads_t = _tail(ops, ei, x, W, a_s, a_d, bias, gsel, H, C, rows, torch.bfloat16, pad=pad)
    if pad:
        assert np.all(grads_t[0][n:] == 0.0), "pad rows of the input must get a zero gradient"
        grads_t[0] = grads_t[0][:n]
    # the path it replaces
    g = build_batch_graph(ei, n, DEV, seeds=rows).seed_graph
    xd = T(x).to(DEV, torch.bfloat16).requires_grad_(True)
    Wd, asd, add_, bd = (T(t).to(DEV, torch.float32).requires_grad_(True) for t in (W, a_s, a_d, bias))
    h = torch.nn.functional.linear(xd, Wd.to(torch.bfloat16))
    out_m = ops.gat_edge(h, asd, add_, bd, g, H, C, False, False)
    (out_m.float() * T(gsel).to(DEV, torch.float32)).sum().backward()
    grads_m = [t.grad.detach().float().cpu().numpy() for t in (xd, Wd, asd, add_, bd)]
    out_m = out_m.detach().float().cpu().numpy()

    def rel(a, b):
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))

    def cos(a, b):
        return float((a * b).sum() / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))

    e_t, e_m = rel(out_t, out_o), rel(out_m, out_o)
    print("out rel-L2: tail %.3e, map-first %.3e" % (e_t, e_m))
    assert e_t <= 6e-3 and e_t <= 2.0 * e_m + 1e-3
    for name, t_, m_, o_ in zip(("x", "W", "att_src", "att_dst", "bias"), grads_t, grads_m, grads_o):
        rt, rm, ct = rel(t_, o_), rel(m_, o_), cos(t_, o_)
        print("%-8s rel-L2: tail %.3e, map-first %.3e, cos(tail, oracle) %.6f" % (name, rt, rm, ct))
        assert ct >= 0.999 and rt <= 0.05 and rt <= 2.0 * rm + 5e-3, name


# ------------------------------------------------------------------------------------------------------------------
# The source backward's UNSTAGED branch (k_tail_src_bwd: a block of 8 source rows with more than 128 out-edges), which the random
# graphs above never reach -- a source there has about one edge into the few targets.  gat_cases.tail_hub() has two sources that
# send to every one of its 163 targets (asserted on the host in tests/test_gat_ref_cpu.py), a block that straddles n_tgt, and
# with 5 pad rows a last block that straddles both n and rows_out.

def _hub_problem(H, C, K, seed):
    import gat_cases
    c = gat_cases.tail_hub()
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(c.n, K)) * 0.7
    W = rng.normal(size=(H * C, K)) / np.sqrt(K)
    a_s = rng.normal(size=(1, H, C)) * 0.3
    a_d = rng.normal(size=(1, H, C)) * 0.3
    bias = rng.normal(size=C) * 0.1
    gsel = rng.normal(size=(c.n_tgt, C))
    return c, (torch.as_tensor(c.edge_index()), x, W, a_s, a_d, bias, gsel)


# K = 64: 8 of the 256 threads hold columns, K % 32 == 0 (bf16: the matrix-core logit / edge kernels); K = 40: K % 32 != 0
@pytest.mark.parametrize("K", [64, 40])
def test_tail_unstaged_source_blocks_fp32_match_the_fp64_oracle(K):
    from spadot_amd import ops
    H, C = 4, 16
    c, prob = _hub_problem(H, C, K, seed=K)
    out_o, grads_o = _oracle(*prob, H, c.n_tgt)
    out_d, grads_d = _tail(ops, *prob, H, C, c.n_tgt, torch.float32, pad=c.marks["pad"])
    np.testing.assert_allclose(out_d, out_o, rtol=1e-4, atol=2e-5)
    for name, d, o in zip(("x", "W", "att_src", "att_dst", "bias"), grads_d, grads_o):
        if name == "x":
            assert np.all(d[c.n:] == 0.0), "pad rows of the input must get a zero gradient"
            d = d[:c.n]
        np.testing.assert_allclose(d, o, rtol=2e-3, atol=2e-4 * np.abs(o).max(), err_msg=name)


@pytest.mark.parametrize("K", [64, 40])
def test_tail_unstaged_source_blocks_bf16_vs_oracle_and_vs_the_map_first_path(K):
    H, C = 4, 16
    c, prob = _hub_problem(H, C, K, seed=K + 1)
    _bf16_vs_oracle_and_map_first(c.n_tgt, H, C, *prob, pad=c.marks["pad"])
