"""fp64 reference of one GATConv edge phase (everything after the dense map h = x W^T) in its scatter formulation, and of the
two-layer chains the handoff tests run -- plain torch, differentiated by autograd, on whatever device its inputs live on
(the CPU in test_gat_ref_cpu.py, which holds it to oracle/model_oracle.py's gat_conv).

    pre[e, hd]  = <h[src_e, hd], att_src[hd]> + <h[tgt_e, hd], att_dst[hd]>          per edge e = (src_e -> tgt_e)
    alpha       = softmax over the incoming edges of each target of leaky_relu(pre, 0.2)     (exp(e - max) / (sum + 1e-16))
    out[i]      = concat or mean over the heads of  sum_e alpha[e] h[src_e]  + bias,  then leaky_relu(., 0.01) if act

The activation is F.leaky_relu, whose derivative at 0 is the negative slope -- the kernels' `!(x > 0)`.
The graph is the by-target CSR of ops.BatchGraph: rowptr [n_tgt + 1], col [E] (source of every edge); the targets are the
first n_tgt of the n rows of h (rows of h past the graph's nodes are padding and are not read)."""
import torch
import torch.nn.functional as F

F64 = torch.float64
ATT_SLOPE = 0.2          # GATConv's negative_slope on the logits
ACT_SLOPE = 0.01         # the activation between the encoder's layers


def edge_lists(rowptr, col):
    """(src, tgt) int64 [E] of a by-target CSR."""
    rowptr = torch.as_tensor(rowptr).long()
    col = torch.as_tensor(col).long()
    n_tgt = rowptr.numel() - 1
    tgt = torch.repeat_interleave(torch.arange(n_tgt, device=col.device), rowptr[1:] - rowptr[:-1])
    return col, tgt


def gat_edge(h, att_src, att_dst, bias, rowptr, col, H, C, concat=True, act=False):
    """h [>= n, H * C], att_src / att_dst [1, H, C] (or [H, C]), bias [H * C] (concat) or [C] -> out [n_tgt, H * C or C]."""
    src, tgt = edge_lists(rowptr, col)
    n_tgt = torch.as_tensor(rowptr).numel() - 1
    hv = h.reshape(h.shape[0], H, C)
    s_src = (hv * att_src.reshape(1, H, C)).sum(-1)
    s_dst = (hv * att_dst.reshape(1, H, C)).sum(-1)
    e = F.leaky_relu(s_src[src] + s_dst[tgt], ATT_SLOPE)
    emax = torch.full((n_tgt, H), -float("inf"), device=h.device, dtype=h.dtype)
    emax = emax.scatter_reduce(0, tgt[:, None].expand(-1, H), e, "amax")
    ex = torch.exp(e - emax[tgt])
    den = torch.zeros((n_tgt, H), device=h.device, dtype=h.dtype).index_add(0, tgt, ex) + 1e-16
    alpha = ex / den[tgt]
    out = torch.zeros((n_tgt, H, C), device=h.device, dtype=h.dtype).index_add(0, tgt, alpha[:, :, None] * hv[src])
    out = out.reshape(n_tgt, H * C) if concat else out.mean(dim=1)
    out = out + bias
    return F.leaky_relu(out, ACT_SLOPE) if act else out


def leaves(*tensors):
    """fp64 leaf copies (requires_grad) of tensors of any dtype."""
    return [t.detach().to(F64).clone().requires_grad_(True) for t in tensors]


def chain_dense(h, p1, W, p2, csr, H, C, w):
    """The first handoff chain: gat_edge(act) -> x W^T -> gat_edge(no act) -> sum(out * w), both layers on the same graph
    with H heads of C channels.  p1 / p2 = (att_src, att_dst, bias) of the two layers; csr = (rowptr, col).
    Returns (out1, out2, loss)."""
    out1 = gat_edge(h, *p1, *csr, H, C, True, True)
    out2 = gat_edge(out1 @ W.t(), *p2, *csr, H, C, True, False)
    return out1, out2, (out2 * w).sum()


def chain_tail(h, p1, csr1, H1, C1, W, p2, csr2, H2, C2, w):
    """The second handoff chain: gat_edge(act) on a graph whose targets are a prefix of its nodes -> the last layer
    (dense map + edge phase, head mean) on a graph whose sources are those targets -> sum(out * w).
    Returns (out1, out2, loss)."""
    out1 = gat_edge(h, *p1, *csr1, H1, C1, True, True)
    out2 = gat_edge(out1 @ W.t(), *p2, *csr2, H2, C2, False, False)
    return out1, out2, (out2 * w).sum()


def rel_l2(a, b):
    """|a - b| / |b| in fp64 (b the reference)."""
    a, b = a.detach().to(F64), b.detach().to(F64).to(a.device)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
