"""Graphs of the GAT edge-kernel tests (CPU and GPU), each built for ONE property of the kernels' block plans or degree limits;
tests/test_gat_ref_cpu.py asserts every property on the host, so a case that loses its property fails there instead of
silently testing something else on the device.

A case holds the edges WITHOUT self loops (src -> dst, dst < n_tgt); edge_index() / csr() / graph() add exactly one self loop per
target (GATConv's convention, spadot_amd.graph).  Blocks follow the node numbering (no spatial order): block b of a plan is rows
32 b .. 32 b + 31."""
import functools

import numpy as np
import torch

MAXC = 992          # csrc/gat_mfma.hip agg::MAXC: the longest column list of a block the matrix-core kernels accept
PLAN_ROWS = 32
TAIL_ROWS = 8       # source rows per workgroup of k_tail_src_bwd (csrc/gat_tail.hip)
TAIL_MAXE = 128     # ... and the most out-edges of such a block it stages in LDS


class Case:
    def __init__(self, name, n, n_tgt, src, dst, **marks):
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        assert src.shape == dst.shape and (src != dst).all() and (dst < n_tgt).all() and (src < n).all() and src.min(initial=0) >= 0
        key = np.unique(src * n + dst)                        # (no duplicate edge: a plan tile has one cell per pair)
        self.name, self.n, self.n_tgt = name, int(n), int(n_tgt)
        self.src, self.dst = key // n, key % n
        self.src.setflags(write=False)
        self.dst.setflags(write=False)
        self.marks = marks                                    # the nodes / blocks the case is about
        self._csr = None

    def edge_index(self):
        """int64 [2, E]: the edges plus one self loop per target."""
        loops = np.arange(self.n_tgt, dtype=np.int64)
        return np.stack([np.concatenate([self.src, loops]), np.concatenate([self.dst, loops])])

    def csr(self):
        """(rowptr, col, rowptr_t, col_t, eid_t) as numpy arrays (spadot_amd.graph._csr_both)."""
        if self._csr is None:
            from spadot_amd.graph import _csr_both
            ei = self.edge_index()
            self._csr = tuple(np.ascontiguousarray(p) for p in _csr_both(ei[0], ei[1], self.n, self.n_tgt))
        return self._csr

    def graph(self, device, plans=True):
        from spadot_amd.graph import attach_plans
        from spadot_amd.ops import BatchGraph
        g = BatchGraph(self.n, *(torch.from_numpy(p).to(device) for p in self.csr()), n_tgt=self.n_tgt)
        return attach_plans(g, None) if plans else g

    def plans(self):
        """(plan_t, plan_s) built on CPU tensors, as graph.attach_plans builds them on the device."""
        from spadot_amd.graph import build_block_plan
        rowptr, col, rowptr_t, col_t, eid_t = (torch.from_numpy(p) for p in self.csr())
        return (build_block_plan(rowptr, col, self.n), build_block_plan(rowptr_t, col_t, self.n_tgt, eid=eid_t))

    def in_degree(self):
        rowptr = self.csr()[0]
        return rowptr[1:] - rowptr[:-1]

    def out_degree(self):
        rowptr_t = self.csr()[2]
        return rowptr_t[1:] - rowptr_t[:-1]

    def block_columns(self, b):
        """Number of distinct sources of the targets 32 b .. 32 b + 31."""
        rowptr, col = self.csr()[:2]
        lo, hi = PLAN_ROWS * b, min(PLAN_ROWS * (b + 1), self.n_tgt)
        return int(np.unique(col[rowptr[lo]:rowptr[hi]]).size)

    def tail_block_edges(self):
        """Out-edges of every block of 8 consecutive source rows (what k_tail_src_bwd stages per workgroup)."""
        rowptr_t = self.csr()[2]
        nblk = (self.n + TAIL_ROWS - 1) // TAIL_ROWS
        ends = np.minimum((np.arange(nblk) + 1) * TAIL_ROWS, self.n)
        return rowptr_t[ends] - rowptr_t[np.arange(nblk) * TAIL_ROWS]


def _random_in_edges(rng, n, targets, k):
    """k distinct sources (other than itself) for every target, drawn from all n nodes."""
    src, dst = [], []
    for i in targets:
        c = rng.choice(n - 1, size=k, replace=False)
        src.append(c + (c >= i))
        dst.append(np.full(k, i))
    return np.concatenate(src), np.concatenate(dst)


@functools.lru_cache(maxsize=None)
def column_limit(others):
    """Block 0 = targets 0 .. 31, each with `others` sources of its own outside the block: 32 (1 + others) distinct columns.
    others = 30: 992 = agg::MAXC, the longest list the matrix-core kernels accept; others = 31: 1024, refused.
    Every node is a target; 13 nodes past the last source make the last block partial."""
    n = 32 + 32 * 31 + 13
    dst = np.repeat(np.arange(32), others)
    src = 32 + np.arange(32 * others)
    return Case("column_limit_%d" % (32 * (1 + others)), n, n, src, dst, block=0, columns=32 * (1 + others))


@functools.lru_cache(maxsize=None)
def chunk_blocks():
    """Blocks 0, 1, 2 with exactly 32, 48 and 64 distinct columns: a ring inside each block (no column from outside), plus 16
    resp. 32 sources of their own from outside the block.  graph.PLAN_KPAD pads a column list to a multiple of 32 = two 16-wide
    chunks, so the kernels walk 2, 4 and 4 chunks (a list of 3 chunks does not exist)."""
    src, dst = [], []
    for b in range(3):
        r = np.arange(32)
        src.append(32 * b + r)
        dst.append(32 * b + (r + 1) % 32)
    src.append(100 + np.arange(16)); dst.append(32 + 2 * np.arange(16))            # block 1: 16 outside sources
    src.append(120 + np.arange(32)); dst.append(64 + np.arange(32))                # block 2: 32 outside sources
    return Case("chunk_blocks", 200, 200, np.concatenate(src), np.concatenate(dst), columns=(32, 48, 64), padded=(32, 64, 64))


@functools.lru_cache(maxsize=None)
def degree_limit(H):
    """The per-node kernels (k_gat_alpha, k_gat_softmax_bwd) keep four passes of 64 / H edges in registers: target 0 has
    in-degree 256 // H (the last register slot), target 1 has 256 // H + 1 (one edge in the loop behind them), target 2 only its
    self loop; the other nodes hear from their predecessor."""
    lim = 256 // H
    n = 300
    src = [3 + np.arange(lim - 1), 3 + np.arange(lim), np.arange(3, n - 1)]
    dst = [np.zeros(lim - 1, dtype=np.int64), np.ones(lim, dtype=np.int64), np.arange(4, n)]
    return Case("degree_limit_H%d" % H, n, n, np.concatenate(src), np.concatenate(dst), limit=lim, at=0, above=1, alone=2)


@functools.lru_cache(maxsize=None)
def ragged_blocks():
    """70 targets (3 blocks) out of 150 nodes (5 blocks by source): for H = 1, 2, 4 neither plan's nb * H is a multiple of 8 (the
    grid is rounded up to 8: idle workgroups), and the by-source plan has rows of the shared partial matrix that the by-target
    plan lacks."""
    n, n_tgt = 150, 70
    src, dst = _random_in_edges(np.random.default_rng(11), n, range(n_tgt), 5)
    return Case("ragged_blocks", n, n_tgt, src, dst)


@functools.lru_cache(maxsize=None)
def small_all_targets():
    """97 nodes, all targets, 6 random sources each: the graph under the row-padding cases (h with 5 / 4097 pad rows)."""
    n = 97
    src, dst = _random_in_edges(np.random.default_rng(12), n, range(n), 6)
    return Case("small_all_targets", n, n, src, dst)


@functools.lru_cache(maxsize=None)
def tail_hub(n=658, rows=163, k=6):
    """The last layer's graph (rows targets, a prefix of n sources, rows * 4 <= n) with two hub SOURCES that send to every target:
    node 77 (a target itself) and node 301 (a source only) -- their blocks of 8 source rows hold more than 128 out-edges, every
    other block at most 128, so k_tail_src_bwd takes its unstaged branch for exactly those two and the staged one elsewhere.
    rows % 8 != 0: one block straddles n_tgt.  n % 8 = 2: with 5 pad rows the last block holds the last 2 nodes, the 5 pad rows
    and one row past rows_out."""
    src, dst = _random_in_edges(np.random.default_rng(13), n, range(rows), k)
    hubs = (77, 301)
    for hub in hubs:
        t = np.arange(rows)
        t = t[t != hub]
        src, dst = np.concatenate([src, np.full(t.size, hub)]), np.concatenate([dst, t])
    return Case("tail_hub", n, rows, src, dst, hubs=hubs, pad=5)


@functools.lru_cache(maxsize=None)
def handoff_dense():
    """2600 nodes, all targets, 5 random sources each: 2600 rows are at least the 2560 the input-gradient GEMM asks for and no
    multiple of its 320-row panel (the last panel has 40 rows: it ends inside sub-tile 1 of wave-row 0)."""
    n = 2600
    src, dst = _random_in_edges(np.random.default_rng(14), n, range(n), 5)
    return Case("handoff_dense", n, n, src, dst)


@functools.lru_cache(maxsize=None)
def handoff_producer():
    """The layer below tail_hub(): 900 nodes of which the first 658 -- tail_hub's sources -- are targets."""
    n, n_tgt = 900, tail_hub().n
    src, dst = _random_in_edges(np.random.default_rng(15), n, range(n_tgt), 6)
    return Case("handoff_producer", n, n_tgt, src, dst)
