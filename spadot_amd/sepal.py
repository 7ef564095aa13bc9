"""The sepal stage: HOW LARGE the spatial pattern of a gene is.  The expression of a gene diffuses over the spatial graph and the time
until it has become homogeneous is its score (sepal, Andersson & Lundeberg 2021; squidpy's gr.sepal; csrc/sepal.hip).
A gene with large-scale structure takes long, a gene that looks like noise is flat almost at once.  The reference has no such
stage; the definition is restated in numpy in tests/sepal_ref.py.

    diffusion_graph(edges, sizes, device)                    the symmetric CSR of every time point, its degrees and rates
    diffuse(edges, dc | dense, genes=None, steps=.., dt=0.1)  the image after exactly `steps` steps and the entropy after every step
    sepal(edges, dc | dense, genes=None, dt=0.1, thresh=1e-8, n_iter=30000)    one SepalResult per time point
    sepal_table(r, genes)                                    the genes by descending score
    sepal_stage(args)   the stage.  args: data, output_dir, prefix (''), genes, k (6), dt (0.1), thresh (1e-8), n_iter (30000), device

squidpy's sepal needs a perfect square or hexagonal lattice and treats border nodes specially; the spots here are a jittered grid
or arbitrary coordinates and every stage works on the spatial k-nearest-neighbour graph, so the stage diffuses on that graph.  One
time point: n spots and E directed edges (src, dst).
Graph: W = A + A^T with multiplicity (a pair that is an edge in both directions has weight 2), as a CSR whose row i lists first the
    targets of i's own edges in the order given, then the sources of the edges that end in i in the order given (moran.edge_csr on
    (cat(src, dst), cat(dst, src)), a stable sort).  deg_i is the length of row i; the mean degree is 2 E / n.
Rate: a = dt n / (2 E), formed once in fp64 (the product, then the quotient).  A dt with a max_i deg_i >= 1 is refused before any
    launch: below that the explicit step cannot produce a negative value except by rounding.  On a 4-neighbour square lattice
    every interior spot has degree 8 (every edge in both directions) and the step is c + (dt / 4) (N + S + E + W - 4 c): squidpy's
    5-point stencil at a quarter of its rate.
Image: c^0 is the fp32 value of the gene at every spot widened to fp64, 0 where nothing is stored (trends.lognorm_values of a
    DeviceCounts by default; dense columns through moran.columns).  Negative and non-finite values are refused.
Step t = 1, 2, .., Jacobi, every operation rounded once (no fused multiply-add: the image has the bits of numpy):
    s_i = ((0 + c_j1) + c_j2) + ..  over row i     l_i = s_i - deg_i c_i     c'_i = c_i + a l_i, 0 where that is < 0
Entropy over the spots with c_i > 0: S = sum c_i, Q = sum c_i log c_i, H = (log S - Q / S) / n; H^0 that of c^0.
Stop: after step t if |H^t - H^(t-1)| <= thresh: iterations = t, converged, score = dt t.  No stop up to n_iter: iterations =
    n_iter, not converged, score = dt n_iter (such a gene ranks among the slowest, which is what it is).
Degenerate: a gene without a positive value in the time point, and every gene of a time point with n < 2 or E = 0: score NaN,
    iterations 0, not converged, no step is run.  A constant gene is not degenerate: it stops at t = 1.

Limits: at most 2147483647 spots and 1073741823 edges per time point, n_iter <= 2147483647."""
import sys
import time

import numpy as np

from .moran import columns, edge_csr, gene_selection, moran_order, read_genes
from .utils._stage_utils import edge_pair, open_stage, savez_pinned, timings, write_timepoints

FIELDS = ("score", "iterations", "converged", "H0", "H", "degenerate")
TABLE_COLUMNS = ("gene", "score", "iterations", "converged", "entropy_start", "entropy_end", "rank")
MAX_EDGES = 1073741823             # directed edges of a time point: the symmetric CSR holds twice as many int32 entries


class DiffusionGraph:
    """The symmetric CSRs of a call on the device: rowptr int32 [sum (n + 1)], col int32 [sum 2 E], desc (the descriptor of
    moran.edge_csr, int64 [T, 8] on the host; column 2 holds 2 E), `degrees` ([t] -> int32 device tensor [n_t]), and on the host
    sizes, E (directed edges) and max_degree, int64 [T]."""

    def __init__(self, rowptr, col, desc, degrees, sizes, E, max_degree):
        self.rowptr, self.col, self.desc, self.degrees = rowptr, col, desc, degrees
        self.sizes, self.E, self.max_degree = sizes, E, max_degree

    def rates(self, dt):
        """a = dt n / (2 E) of every time point, fp64 [T] (0.0 without edges)."""
        from .stage_ops import sepal_rate
        return np.asarray([sepal_rate(dt, n, 2 * e) for n, e in zip(self.sizes, self.E)], dtype=np.float64)

    def max_dt(self):
        """The largest dt that every time point admits (inf where no time point has an edge)."""
        from .stage_ops import sepal_max_dt
        return min(sepal_max_dt(n, 2 * e, d) for n, e, d in zip(self.sizes, self.E, self.max_degree))


def diffusion_graph(edges, sizes, device):
    """The graph W = A + A^T of every time point (module docstring) as a DiffusionGraph.  edges[t]: (src, dst) integer device
    tensors of time point t, any order; sizes[t]: its spots.  Edge ends outside 0 .. n-1: ValueError, before anything is sorted;
    CPU tensors: RuntimeError."""
    import torch
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if not edges or len(edges) != sizes.shape[0]:
        raise ValueError(f"sepal takes one edge list per time point ({len(edges) if edges else 0} lists, {sizes.shape[0]} time points)")
    pairs = [edge_pair(e, device, t) for t, e in enumerate(edges)]
    for t, (s, _) in enumerate(pairs):
        if s.numel() > MAX_EDGES:
            raise ValueError(f"time point {t} has {s.numel()} edges: sepal takes at most {MAX_EDGES} (both directions are stored)")
    with torch.cuda.device(device):
        both = [(torch.cat([s.reshape(-1), d.reshape(-1)]), torch.cat([d.reshape(-1), s.reshape(-1)])) for s, d in pairs]
        rowptr, col, desc = edge_csr(both, sizes, device)
        degrees = [torch.diff(rowptr[int(r):int(r) + int(n) + 1]) for r, n in zip(desc[:, 5], sizes)]
        most = torch.stack([d.max() for d in degrees]).cpu().numpy().astype(np.int64)
    return DiffusionGraph(rowptr, col, desc, degrees, sizes, desc[:, 2] // 2, most)


def _prepare(edges, data, genes, values):
    """What both calls share: the Columns, the selection, the graph (its descriptor on the rows of the data) and the genes on the
    device."""
    import torch
    cols = columns(data, values)
    off = np.asarray(cols.tp_off_host, dtype=np.int64)
    sel = gene_selection(np.arange(cols.G) if genes is None else genes, cols.G)
    graph = diffusion_graph(edges, np.diff(off), cols.device)
    graph.desc[:, 3] = off[:-1]
    return cols, off, sel, graph, torch.as_tensor(sel, device=cols.device)


def _images(state, off, ng):
    """[t] -> the image fp64 numpy [n_t, genes] of the items of time point t."""
    img = state["image"].cpu().numpy()
    return [np.ascontiguousarray(img[t * ng:(t + 1) * ng, :int(off[t + 1] - off[t])].T) for t in range(len(off) - 1)]


def diffuse(edges, data, genes=None, steps=100, dt=0.1, values=None, lds_limit=None, steps_per_launch=None):
    """The graph-smoothed expression: the image of every selected gene after exactly `steps` >= 1 steps, with no stop rule, and
    its entropy after every step (module docstring).  edges[t]: (src, dst) device tensors of time point t (spatial_edges or a
    caller's graph); data: a DeviceCounts (values: its fp32 values in CSC order, default trends.lognorm_values) or, per time
    point, a dense float32 / float64 device tensor [n_t, C]; genes: gene (column) indices (default: all).  lds_limit: the LDS
    bytes a workgroup may use; steps_per_launch: the steps of one launch (neither changes a bit).  Returns ([t] -> fp64 numpy
    [n_t, genes], [t] -> fp64 numpy [genes, steps + 1], NaN for a degenerate gene).  ValueError / RuntimeError before any
    launch."""
    import torch
    from . import stage_ops as ops
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"diffuse takes at least one step (got steps = {steps})")
    cols, off, sel, graph, gsel = _prepare(edges, data, genes, values)
    with torch.cuda.device(cols.device):
        state = ops.sepal_steps(graph.rowptr, graph.col, cols.colptr, cols.ridx, cols.values, gsel, graph.desc, dt, 0.0, steps,
                                steps if steps_per_launch is None else steps_per_launch, False, lds_limit, None, steps + 1)
        trace = state["trace"].cpu().numpy()
        return _images(state, off, sel.size), [trace[t * sel.size:(t + 1) * sel.size] for t in range(cols.T)]


class SepalResult:
    """One time point, per selected gene ([genes]): score fp64 (dt * iterations; NaN for a degenerate gene), iterations int64,
    converged bool, H0 and H fp64 (the entropy of the first and of the last image), degenerate bool; `image` fp64 [n, genes]
    (the last image), `genes` (the selection), n, E, dt, thresh, n_iter."""

    def __init__(self, iterations, done, H0, H, image, genes, n, E, dt, thresh, n_iter):
        self.iterations, self.degenerate, self.converged = iterations.astype(np.int64), done == 2, done == 1
        self.score = np.where(self.degenerate, np.nan, float(dt) * self.iterations.astype(np.float64))
        self.H0, self.H, self.image, self.genes = H0, H, image, np.asarray(genes)
        self.n, self.E, self.dt, self.thresh, self.n_iter = int(n), int(E), float(dt), float(thresh), int(n_iter)


def sepal(edges, data, genes=None, dt=0.1, thresh=1e-8, n_iter=30000, values=None, steps_per_launch=None, lds_limit=None,
          state=None):
    """The diffusion time of every selected gene of every time point (module docstring).  edges[t]: (src, dst) device tensors of
    time point t (spatial_edges or a caller's graph); data: a DeviceCounts (values: its fp32 values in CSC order, default
    trends.lognorm_values) or, per time point, a dense float32 / float64 device tensor [n_t, C]; genes: gene (column) indices
    (default: all).  steps_per_launch: the steps of one launch (default 2048), after which the host looks at the flags;
    lds_limit: the LDS bytes a workgroup may use (neither changes a bit); state: a stage_ops.sepal_state to run in.  Returns
    [t] -> SepalResult.  ValueError / RuntimeError before any launch."""
    import torch
    from . import stage_ops as ops
    cols, off, sel, graph, gsel = _prepare(edges, data, genes, values)
    ng = int(sel.size)
    with torch.cuda.device(cols.device):
        state = ops.sepal_steps(graph.rowptr, graph.col, cols.colptr, cols.ridx, cols.values, gsel, graph.desc, dt, thresh, n_iter,
                                steps_per_launch, True, lds_limit, state)
        it, done = state["iterations"].cpu().numpy(), state["done"].cpu().numpy()
        H0, H, images = state["H0"].cpu().numpy(), state["H_prev"].cpu().numpy(), _images(state, off, ng)
    return [SepalResult(it[t * ng:(t + 1) * ng], done[t * ng:(t + 1) * ng], H0[t * ng:(t + 1) * ng], H[t * ng:(t + 1) * ng],
                        images[t], sel, off[t + 1] - off[t], graph.E[t], dt, thresh, n_iter) for t in range(cols.T)]


def sepal_table(r, genes):
    """The rows of {prefix}sepal_{tp}.csv (TABLE_COLUMNS): the selected genes by descending score, NaN last, ties by gene index;
    rank counts from 1 in that order and is 0 for a degenerate gene.  genes: the names of all genes."""
    import pandas as pd
    order = moran_order(r.score)
    rank = np.where(r.degenerate[order], 0, np.arange(1, order.size + 1))
    return pd.DataFrame({"gene": np.asarray(genes)[r.genes][order], "score": r.score[order], "iterations": r.iterations[order],
                         "converged": r.converged[order].astype(np.int64), "entropy_start": r.H0[order], "entropy_end": r.H[order],
                         "rank": rank}, columns=list(TABLE_COLUMNS))


def sepal_stage(args):
    """Reads args.data (counts, as the autocorr stage: coordinates from obsm['spatial']), builds spatial_edges(.., k) of every time
    point and runs one sepal call on the genes of args.genes (a comma list of names or a file with one name per line) or, without
    it, on all genes.  Writes {prefix}sepal_{tp}.csv (TABLE_COLUMNS) and {prefix}sepal.npz ('{tp}_{field}' for FIELDS [genes],
    plus timepoints, genes, k, dt, thresh, n_iter; pinned time stamps: two runs write the same bytes).  Returns {'tables',
    'results' (per time point), 'genes', 'timepoints', 'timings'}."""
    import torch
    from .trends import lognorm_values
    t_start = time.perf_counter()

    def arg(name, default, kind):
        v = getattr(args, name, default)
        return kind(default if v is None else v)

    k, dt, thresh, n_iter = arg("k", 6, int), arg("dt", 0.1, float), arg("thresh", 1e-8, float), arg("n_iter", 30000, int)
    if k < 1 or not (dt > 0.0 and np.isfinite(dt)) or not (thresh >= 0.0 and np.isfinite(thresh)) or n_iter < 1:
        raise ValueError(f"the sepal stage takes k >= 1, a finite dt > 0, a finite thresh >= 0 and n_iter >= 1 (got k = {k}, dt = "
                         f"{dt}, thresh = {thresh}, n_iter = {n_iter})")
    st = open_stage(args, k, "the diffusion times", t_start,
                    lambda raw: read_genes(args.genes, raw.var_names) if getattr(args, "genes", None) else None)
    dc, tps = st.dc, st.tps
    sel = np.arange(dc.G, dtype=np.int32) if st.extras is None else st.extras
    with torch.cuda.device(st.dev):
        res = sepal(st.edges, dc, sel, dt=dt, thresh=thresh, n_iter=n_iter, values=lognorm_values(dc))
    torch.cuda.synchronize(st.dev)
    t_dev = time.perf_counter()
    arrays = dict(timepoints=np.asarray(tps), genes=np.asarray(dc.genes).astype(str)[sel], k=np.int64(k), dt=np.float64(dt),
                  thresh=np.float64(thresh), n_iter=np.int64(n_iter))
    tables, arrays = write_timepoints(st.path, "sepal", tps, res, lambda t, r: sepal_table(r, dc.genes), FIELDS, arrays)
    savez_pinned(st.path("sepal.npz"), arrays)
    t_end = time.perf_counter()
    slow = sum(int((~r.converged & ~r.degenerate).sum()) for r in res)
    print(f"sepal: {sel.size} genes x {dc.n} spots of {dc.T} time points, k = {k}, dt = {dt}, {slow} (time point, gene) pairs "
          f"reached n_iter = {n_iter}, written to {args.output_dir}", file=sys.stderr)
    return {"tables": tables, "results": dict(zip(tps, res)), "genes": sel, "timepoints": tps,
            "timings": timings(st.t_start, st.t_read, t_dev, t_end, st.t_graph)}
