"""CPU: (a) tests/gat_ref.py -- the fp64 reference the GAT edge-kernel tests compare against -- agrees with the oracle's
gat_conv (oracle/model_oracle.py: PyG GATConv semantics) to 1e-12; (b) every graph of tests/gat_cases.py has the property it
is named for, computed from its CSR and from graph.build_block_plan on CPU tensors.  The properties are conditions of the GPU
tests (which block or degree limit a case reaches), not measurements."""
import numpy as np
import pytest
import torch

import gat_cases as gc
import gat_ref
from oracle import model_oracle as mo

F64 = torch.float64


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("case", [gc.ragged_blocks, gc.small_all_targets, lambda: gc.degree_limit(8)])
def test_gat_ref_matches_the_oracle(case, concat):
    """The oracle maps x with a real weight and treats every node as a target; gat_ref is fed h = x W^T and the case's
    by-target CSR, and is compared on the case's targets (a target's row depends on its incoming edges only)."""
    c = case()
    rng = np.random.default_rng(3)
    H, C, K = 4, 6, 10
    x = torch.as_tensor(rng.normal(size=(c.n, K)))
    W = torch.as_tensor(rng.normal(size=(H * C, K)) / np.sqrt(K))
    a_s, a_d = (torch.as_tensor(rng.normal(size=(1, H, C)) * 0.5) for _ in range(2))
    bias = torch.as_tensor(rng.normal(size=(H * C if concat else C)) * 0.1)
    want = mo.gat_conv(x, torch.as_tensor(c.edge_index()), W, a_s, a_d, bias, H, concat)[:c.n_tgt]
    rowptr, col = c.csr()[:2]
    for act in (False, True):
        got = gat_ref.gat_edge(x @ W.t(), a_s, a_d, bias, rowptr, col, H, C, concat, act)
        ref = torch.nn.functional.leaky_relu(want, 0.01) if act else want
        assert got.dtype == F64 and got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_gat_ref_activation_takes_the_slope_at_zero():
    """d leaky_relu / dx at exactly 0 is the slope (the kernels' `!(x > 0)`), for +0.0 and -0.0."""
    x = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=F64, requires_grad=True)
    torch.nn.functional.leaky_relu(x, gat_ref.ACT_SLOPE).sum().backward()
    assert x.grad.tolist() == [0.01, 0.01, 1.0, 0.01]


def test_every_case_has_one_self_loop_per_target_and_no_duplicate_edge():
    for c in (gc.column_limit(30), gc.column_limit(31), gc.chunk_blocks(), gc.degree_limit(1), gc.degree_limit(2), gc.degree_limit(4),
              gc.degree_limit(8), gc.ragged_blocks(), gc.small_all_targets(), gc.tail_hub(), gc.handoff_dense(), gc.handoff_producer()):
        ei = c.edge_index()
        assert np.unique(ei[0] * c.n + ei[1]).size == ei.shape[1], c.name
        assert int((ei[0] == ei[1]).sum()) == c.n_tgt and ei[1].max() < c.n_tgt, c.name
        rowptr, col, rowptr_t, col_t, eid_t = c.csr()
        assert rowptr.size == c.n_tgt + 1 and rowptr_t.size == c.n + 1 and rowptr[-1] == rowptr_t[-1] == ei.shape[1]
        assert (c.in_degree() >= 1).all(), c.name
        pt, ps = c.plans()
        assert pt is not None and ps is not None, c.name


def test_column_limit_cases_sit_on_either_side_of_the_lds_limit():
    at, over = gc.column_limit(30), gc.column_limit(31)
    assert at.n >= 1024 and at.n_tgt == at.n and at.n % 32 != 0
    assert at.block_columns(0) == 992 == gc.MAXC and over.block_columns(0) == 1024
    pt, ps = at.plans()
    assert pt.max_cols == 992 and int(pt.sptr[1] - pt.sptr[0]) == 992 and ps.max_cols <= gc.MAXC
    pt, ps = over.plans()
    assert pt.max_cols == 1024 and ps.max_cols <= gc.MAXC


def test_chunk_blocks_have_32_48_and_64_columns():
    c = gc.chunk_blocks()
    assert tuple(c.block_columns(b) for b in range(3)) == (32, 48, 64)
    pt, _ = c.plans()
    sp = pt.sptr.tolist()
    assert tuple(sp[b + 1] - sp[b] for b in range(3)) == (32, 64, 64)         # 2, 4 and 4 chunks of 16
    assert pt.max_cols == 64


@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_degree_limit_cases_sit_on_either_side_of_the_register_passes(H):
    c = gc.degree_limit(H)
    deg = c.in_degree()
    assert c.marks["limit"] == 256 // H == 4 * (64 // H)
    assert deg[c.marks["at"]] == 256 // H and deg[c.marks["above"]] == 256 // H + 1 and deg[c.marks["alone"]] == 1
    pt, ps = c.plans()
    assert pt.max_cols <= gc.MAXC and ps.max_cols <= gc.MAXC


def test_ragged_blocks_leave_idle_workgroups_and_rows_only_one_plan_has():
    c = gc.ragged_blocks()
    pt, ps = c.plans()
    assert c.n_tgt < c.n and (pt.nb, ps.nb) == (3, 5)
    for H in (1, 2, 4):
        assert (pt.nb * H) % 8 != 0 and (ps.nb * H) % 8 != 0
    assert pt.max_cols <= gc.MAXC and ps.max_cols <= gc.MAXC


def test_small_and_handoff_graphs_fit_the_matrix_core_kernels():
    for c in (gc.small_all_targets(), gc.handoff_dense(), gc.handoff_producer()):
        pt, ps = c.plans()
        assert pt.max_cols <= gc.MAXC and ps.max_cols <= gc.MAXC and pt.max_cols % 32 == 0, c.name
    d = gc.handoff_dense()
    assert d.n_tgt == d.n == 2600 and d.n >= 2560 and d.n % 320 == 40
    p, t = gc.handoff_producer(), gc.tail_hub()
    assert p.n_tgt == t.n < p.n                               # the producer's targets are the tail's source rows
    pt, ps = p.plans()
    assert ps.nb > pt.nb


def test_tail_hub_reaches_both_branches_of_the_source_backward():
    c = gc.tail_hub()
    assert c.n_tgt >= 160 and c.n_tgt * 4 <= c.n
    ne = c.tail_block_edges()
    hub_blocks = sorted(h // gc.TAIL_ROWS for h in c.marks["hubs"])
    assert sorted(np.flatnonzero(ne > gc.TAIL_MAXE).tolist()) == hub_blocks           # unstaged: the hubs' blocks, only them
    assert int((ne <= gc.TAIL_MAXE).sum()) == ne.size - 2 and (ne[ne <= gc.TAIL_MAXE] > 0).any()
    out = c.out_degree()
    tgt_hub, src_hub = c.marks["hubs"]
    assert tgt_hub < c.n_tgt <= src_hub
    assert out[tgt_hub] == c.n_tgt and out[src_hub] == c.n_tgt                       # every target (self loop included / not a target)
    assert c.n_tgt % gc.TAIL_ROWS != 0                                               # a block straddles n_tgt
    pad = c.marks["pad"]
    last = c.n // gc.TAIL_ROWS
    assert c.n % gc.TAIL_ROWS != 0 and (c.n + pad) // gc.TAIL_ROWS == last and (c.n + pad) % gc.TAIL_ROWS != 0
    assert (out[c.n_tgt:] == 0).any()                                                # rows without any out-edge are flushed too
