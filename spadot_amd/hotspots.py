"""The hotspots stage: WHERE inside a time point a gene is spatially structured.  Local Moran's I (Anselin's LISA,
esda.Moran_Local) of every spot for selected genes on the spatial k-nearest-neighbour graph, with the quadrant of every spot and a
p-value under conditional permutation (csrc/localmoran.hip).  The reference has no such stage; the definition is
restated in numpy in tests/hotspots_ref.py.

    local_lag(edges, dc, values, centre, genes, n_perms)     the device primitive: lag, ge, le of every (gene, spot)
    local_stats(lag, ge, le, z, m2, n, P, has_neighbours, degenerate)    the host part: I, quadrant, p_sim, padj (numpy only)
    local_moran(edges, dc | dense, genes, n_perms=999)       the test of the selected genes in every spot of every time point
    hotspots(args)    the stage.  args: data, output_dir, prefix (''), k (6), n_perms (999), seed (0), genes, top (50), alpha
                      (0.05), fdr, domains, device

One time point: n spots and directed edges i -> j (no self loops; duplicates count), sorted stably by source: the neighbours of
spot i are its row of a CSR, in edge-list order.  Per gene, v is the fp32 values of trends.lognorm_values (0 where nothing is
stored) promoted to fp64, c and m2 the centre and the spread of autocorr (the mean of v and sum (v_i - c)^2), z_i = v_i - c.  The
neighbour sum of spot i under the shown values x is, in fp64 and in row order,
    lag_i = ((0 + (x_j1 - c)) + (x_j2 - c)) + ...
(subtractions and additions only: the bits are those of numpy).  Observed: x = v.  Permutation p shows x_j = v[pi_p(j)], pi_p the
permutation of neighbors.py's docstring under (seed, index of the time point, p, n), except that while spot i is evaluated the
neighbour j* = pi_p^-1(i), which would show spot i's own value, shows v[pi_p(i)] instead: pi_p composed with the transposition
(i, j*), a uniform draw from the permutations that fix i -- PySAL's conditional permutation without a stored permutation per spot.
The device returns lag (observed), ge = #{p : lag^p >= lag^0} and le = #{p : lag^p <= lag^0} per (gene, spot): exact comparisons
of bit-reproducible sums.  The host:
    I_i = n z_i lag_i / m2                      (sum_i I_i = n N / m2 = S0 times the I of autocorr)
    quadrant: 1 HH (z > 0, lag > 0), 2 LH (z < 0, lag > 0), 3 LL (z < 0, lag < 0), 4 HL (z > 0, lag < 0); 0 where z = 0 or lag = 0
    larger = ge where z > 0, le where z < 0, P where z = 0 (I^p >= I^0 <=> z lag^p >= z lag^0); smaller: the mirror image
    p_sim = (1 + min(larger, smaller)) / (P + 1)
the FOLDED p of esda.Moran_Local.p_sim, one-sided towards the side the observed value lies on: under noise about 10 % of the spots
have p_sim <= 0.05, not 5 %.  padj: Benjamini-Hochberg over the spots of one (time point, gene) that have a neighbour.  A spot
without out-edges has lag 0, I 0, quadrant 0 and NaN in p_sim and padj; a gene that autocorr calls degenerate in a time point (n <
3, E = 0 or m2 <= n 2^-50 sum v^2) is NaN throughout with quadrant 0.  Out of scope: Getis-Ord G_i*, row-standardised weights.

Limits: at most 2147483647 spots and edges per time point; permutation indices below 2^32."""
import sys
import time

import numpy as np

from .moran import centre_spread, columns, degenerate, edge_csr, gene_selection, top_genes
from .moran import read_genes  # noqa: F401  (the --genes of this stage: callers import it from here)
from .utils._stage_utils import edge_pair, open_stage, read_domains, savez_pinned, timings, top_setting, write_timepoints

FIELDS = ("I", "quadrant", "p_sim", "padj", "lag", "ge", "le")
TABLE_COLUMNS = ("gene", "I", "n_HH", "n_LL", "n_LH", "n_HL")
DOMAIN_COLUMNS = ("gene", "domain", "n_HH", "n_LL", "size")
SCRATCH_BYTES = 2 ** 30            # the per-spot state and the images of one launch: the permutations are split beyond that


class HotspotResult:
    """One time point: per (selected gene, spot) the fp64 I, p_sim, padj and lag, the int8 quadrant and the int32 ge and le of the
    module docstring ([genes, n]); `genes` (the selection, gene indices), n, E (= S0), P, z [genes, n], `mean` (the centre) and m2
    [genes], `degenerate` [genes] bool and `has_neighbours` [n] bool."""

    def __init__(self, lag, ge, le, z, mean, m2, n, E, P, has_neighbours, degenerate, genes):
        self.lag, self.ge, self.le, self.z, self.mean, self.m2 = lag, ge, le, z, mean, m2
        self.n, self.E, self.P, self.genes = int(n), int(E), int(P), np.asarray(genes)
        self.has_neighbours, self.degenerate = has_neighbours, degenerate
        for name, v in local_stats(lag, ge, le, z, m2, n, P, has_neighbours, degenerate).items():
            setattr(self, name, v)


def local_stats(lag, ge, le, z, m2, n, P, has_neighbours, degenerate):
    """The host part of one time point (module docstring), numpy only.  lag fp64, ge, le integers and z fp64: [genes, n]; m2
    [genes]; has_neighbours [n] bool; degenerate [genes] bool.  Returns a dict: I, p_sim, padj fp64, quadrant int8, larger and
    smaller int64, all [genes, n]."""
    from .markers import bh_adjust
    lag, z = np.atleast_2d(np.asarray(lag, dtype=np.float64)), np.atleast_2d(np.asarray(z, dtype=np.float64))
    ge, le = np.atleast_2d(np.asarray(ge)).astype(np.int64), np.atleast_2d(np.asarray(le)).astype(np.int64)
    m2, bad = np.asarray(m2, dtype=np.float64).reshape(-1), np.asarray(degenerate, dtype=bool).reshape(-1)
    has = np.asarray(has_neighbours, dtype=bool).reshape(-1)
    n, P = int(n), int(P)
    G = lag.shape[0]
    if lag.shape != (G, n) or z.shape != (G, n) or ge.shape != (G, n) or le.shape != (G, n) or m2.shape != (G,) \
            or bad.shape != (G,) or has.shape != (n,) or P < 1:
        raise ValueError(f"local_stats takes lag, ge, le and z [genes, n], m2 and degenerate [genes], has_neighbours [n] and P >= 1 "
                         f"(got lag {lag.shape}, n = {n}, P = {P})")
    I = n * z * lag / np.where(bad, 1.0, m2)[:, None]
    quadrant = np.zeros((G, n), dtype=np.int8)
    quadrant[(z > 0) & (lag > 0)] = 1
    quadrant[(z < 0) & (lag > 0)] = 2
    quadrant[(z < 0) & (lag < 0)] = 3
    quadrant[(z > 0) & (lag < 0)] = 4
    larger = np.where(z > 0, ge, np.where(z < 0, le, P))
    smaller = np.where(z > 0, le, np.where(z < 0, ge, P))
    p_sim = (1.0 + np.minimum(larger, smaller)) / (P + 1.0)
    lone = ~has[None, :]
    I, p_sim = np.where(lone, 0.0, I), np.where(lone, np.nan, p_sim)
    quadrant[:, ~has] = 0
    padj = np.full((G, n), np.nan)
    for g in np.flatnonzero(~bad):
        if has.any():
            padj[g, has] = bh_adjust(p_sim[g, has])
    I[bad], p_sim[bad], quadrant[bad] = np.nan, np.nan, 0
    return {"I": I, "quadrant": quadrant, "p_sim": p_sim, "padj": padj, "larger": larger, "smaller": smaller}


def local_lag(edges, dc, values, centre, genes, n_perms, seed=0, first=0, lds_limit=None, threads=None, gs=None, perm_chunk=None):
    """lag, ge and le of every (selected gene, spot) of every time point (module docstring).  edges[t]: (src, dst) integer device
    tensors of time point t, in the order of dc's time points (any edge order: the rows are built here by a stable sort by
    source); dc: a DeviceCounts (its colptr, ridx, tp_off); values: fp32 device tensor, one per stored entry in CSC order; centre:
    fp64 [T, G] (device tensor or array); genes: integer gene indices, any order, repeats allowed.  Permutations first .. first
    + n_perms - 1 under seed, time point t as graph index t: a long run may be split over `first`, the counts add and lag is the
    same.  lds_limit: the LDS bytes a workgroup may use (default 163840): a time point whose image does not fit keeps it in
    global memory, with the same results.  threads, gs, perm_chunk: the workgroup, the genes per group and the permutations per
    workgroup (defaults 1024, 4, 128; the results do not depend on them).  One launch (several only where the per-spot state of
    all chunks would pass 1 GiB).  Returns [t] -> (lag fp64, ge int32, le int32) numpy [genes, n_t].  ValueError / RuntimeError
    before any launch."""
    import torch
    from . import stage_ops as ops
    T, G = int(dc.T), int(dc.G)
    if not edges or len(edges) != T:
        raise ValueError(f"local_lag takes one edge list per time point ({len(edges) if edges else 0} lists, {T} time points)")
    pairs = [edge_pair(e, dc.device, t) for t, e in enumerate(edges)]
    if not isinstance(values, torch.Tensor):
        raise RuntimeError("local_lag takes the values as a device tensor (torch), not a host array")
    centre = centre if isinstance(centre, torch.Tensor) else torch.as_tensor(np.asarray(centre, dtype=np.float64), device=dc.device)
    sel = gene_selection(genes, G)
    n_perms, first = int(n_perms), int(first)
    if n_perms < 1:
        raise ValueError(f"local_lag takes at least one permutation (got n_perms = {n_perms})")
    off = np.asarray(dc.tp_off_host, dtype=np.int64)
    with torch.cuda.device(dc.device):
        rowptr, col, desc = edge_csr(pairs, np.diff(off), dc.device)
        desc[:, 3] = off[:-1]
        gsel = torch.as_tensor(sel, device=dc.device)
        args = (rowptr, col, dc.colptr, dc.ridx, values, centre.contiguous(), gsel)
        checked = ops.local_check(*args, desc, first, n_perms, threads, gs, perm_chunk)
        chunk = int(perm_chunk or ops.LOCAL_CHUNK)
        per = ops.local_scratch_bytes(desc, sel.size, chunk, lds_limit, gs, chunk)
        run = max(1, SCRATCH_BYTES // per) * chunk           # the permutations of one launch
        scratch = torch.empty(ops.local_scratch_bytes(desc, sel.size, min(run, n_perms), lds_limit, gs, chunk), dtype=torch.uint8,
                              device=dc.device)
        out = None
        for p0 in range(0, n_perms, run):
            out = ops.local_launch(*args, checked, first + p0, min(run, n_perms - p0), seed, lds_limit, out, scratch, threads, gs,
                                   perm_chunk)
        lag, ge, le = (o.cpu().numpy() for o in out)
    return [(lag[:, off[t]:off[t + 1]], ge[:, off[t]:off[t + 1]], le[:, off[t]:off[t + 1]]) for t in range(T)]


def _dense_rows(dc, values, sel):
    """The fp32 values of the selected genes as a dense device tensor [genes, spots] (0 where nothing is stored)."""
    import torch
    g = torch.as_tensor(sel.astype(np.int64), device=dc.device)
    start, ln = dc.colptr[g], dc.colptr[g + 1] - dc.colptr[g]
    j = torch.repeat_interleave(torch.arange(g.numel(), device=dc.device), ln)
    pos = torch.arange(int(ln.sum()), device=dc.device) - torch.repeat_interleave(torch.cumsum(ln, 0) - ln, ln) \
        + torch.repeat_interleave(start, ln)
    dense = torch.zeros((g.numel(), int(dc.n)), dtype=torch.float32, device=dc.device)
    dense[j, dc.ridx[pos].long()] = values[pos]
    return dense


def local_moran(edges, data, genes, values=None, n_perms=999, seed=0, lds_limit=None):
    """Local Moran's I of the selected genes in every spot of every time point (module docstring).  edges[t]: (src, dst) device
    tensors of time point t (spatial_edges); data: a DeviceCounts (values: its fp32 values in CSC order, default
    trends.lognorm_values) or, per time point, a dense float32 / float64 device tensor [n, C] of columns such as fates or
    memberships, taken as fp32; genes: gene (column) indices.  Time point t permutes under (seed, t).  Returns [t] ->
    HotspotResult."""
    import torch
    n_perms = int(n_perms)
    if n_perms < 1:
        raise ValueError(f"local Moran's I takes at least one permutation (got n_perms = {n_perms})")
    dc = columns(data, values)
    sel = gene_selection(genes, dc.G)
    off = np.asarray(dc.tp_off_host, dtype=np.int64)
    with torch.cuda.device(dc.device):
        _, centre, m2, S2 = centre_spread(dc)
        parts = local_lag(edges, dc, dc.values, centre, sel, n_perms, seed=seed, lds_limit=lds_limit)
        dense = _dense_rows(dc, dc.values, sel).to(torch.float64).cpu().numpy()
        outdeg = [torch.bincount(edge_pair(e, dc.device, t)[0].reshape(-1).long(), minlength=int(off[t + 1] - off[t])).cpu().numpy()
                  for t, e in enumerate(edges)]
        centre, m2, S2 = centre.cpu().numpy()[:, sel], m2.cpu().numpy()[:, sel], S2.cpu().numpy()[:, sel]
    res = []
    for t in range(dc.T):
        n, E = int(off[t + 1] - off[t]), int(outdeg[t].sum())
        z = dense[:, off[t]:off[t + 1]] - centre[t][:, None]
        res.append(HotspotResult(*parts[t], z, centre[t], m2[t], n, E, n_perms, outdeg[t] > 0,
                                 degenerate(n, E, m2[t], S2[t]), sel))
    return res


def significant(r, alpha=0.05, fdr=False):
    """[genes, n] bool: p_sim (padj with fdr) <= alpha."""
    with np.errstate(invalid="ignore"):
        return (r.padj if fdr else r.p_sim) <= alpha


def hotspot_table(r, names, alpha=0.05, fdr=False):
    """The rows of {prefix}hotspots_{tp}.csv, one per selected gene: the global I = sum_i I_i / S0 and the numbers of
    significant spots per quadrant."""
    import pandas as pd
    sig = significant(r, alpha, fdr)
    with np.errstate(invalid="ignore", divide="ignore"):
        I = np.where(r.degenerate, np.nan, r.I.sum(axis=1) / max(r.E, 1))
    cols = {"gene": np.asarray(names)[r.genes], "I": I}
    for name, q in (("n_HH", 1), ("n_LL", 3), ("n_LH", 2), ("n_HL", 4)):
        cols[name] = (sig & (r.quadrant == q)).sum(axis=1)
    return pd.DataFrame(cols, columns=list(TABLE_COLUMNS))


def domain_table(r, names, labels, alpha=0.05, fdr=False):
    """The rows of {prefix}hotspots_domains_{tp}.csv, one per (selected gene, domain): the numbers of significant HH and LL spots
    in the domain and the domain's size."""
    import pandas as pd
    sig = significant(r, alpha, fdr)
    labels = np.asarray(labels, dtype=np.int64)
    K = int(labels.max()) + 1 if labels.size else 0
    sizes = np.bincount(labels, minlength=K)
    rows = []
    for j, g in enumerate(r.genes):
        hh = np.bincount(labels[sig[j] & (r.quadrant[j] == 1)], minlength=K)
        ll = np.bincount(labels[sig[j] & (r.quadrant[j] == 3)], minlength=K)
        rows += [(np.asarray(names)[g], k, int(hh[k]), int(ll[k]), int(sizes[k])) for k in range(K)]
    return pd.DataFrame(rows, columns=list(DOMAIN_COLUMNS))


def hotspots(args):
    """Reads args.data (counts, as the autocorr stage: coordinates from obsm['spatial']), builds spatial_edges(.., k) of every time
    point and runs one local_moran call on the genes of args.genes (a comma list of names or a file with one name per line) or,
    without it, on the union over the time points of the args.top genes by Moran's I (one spatial_autocorr call without
    permutations).  Writes {prefix}hotspots_{tp}.csv (TABLE_COLUMNS; significant: p_sim <= args.alpha, with args.fdr padj <=
    alpha), {prefix}hotspots.npz ('{tp}_{field}' for FIELDS [genes, n_t] and '{tp}_spots', the rows of the data behind the
    columns, plus timepoints, genes, k, n_perms, seed, alpha; pinned time stamps: two runs with one seed write the same bytes) and,
    with args.domains (the domains.csv of analyze), {prefix}hotspots_domains_{tp}.csv (DOMAIN_COLUMNS).  Returns {'tables',
    'domain_tables', 'results' (per time point), 'genes', 'timepoints', 'timings'}."""
    import torch
    from .autocorr import spatial_autocorr
    from .trends import lognorm_values
    t_start = time.perf_counter()
    top = top_setting(args, 50)
    k, n_perms, seed = int(getattr(args, "k", 6)), int(getattr(args, "n_perms", 999)), int(getattr(args, "seed", 0))
    alpha = getattr(args, "alpha", 0.05)
    alpha, fdr = 0.05 if alpha is None else float(alpha), bool(getattr(args, "fdr", False))
    if top < 1 or k < 1 or n_perms < 1 or not 0.0 < alpha <= 1.0:
        raise ValueError(f"the hotspots stage takes top >= 1, k >= 1, n_perms >= 1 and 0 < alpha <= 1 (got top = {top}, k = {k}, "
                         f"n_perms = {n_perms}, alpha = {alpha})")
    st = open_stage(args, k, "the local autocorrelation", t_start, lambda raw: (
        read_genes(args.genes, raw.var_names) if getattr(args, "genes", None) else None,
        read_domains(args.domains, raw.obs["timepoint"]) if getattr(args, "domains", None) else None))
    (sel, labels), dc, tps = st.extras, st.dc, st.tps
    with torch.cuda.device(st.dev):
        values = lognorm_values(dc)
        if sel is None:                                      # the top genes by Moran's I of every time point, unioned
            sel = top_genes(spatial_autocorr(st.edges, dc, values, n_perms=0), top)
            if not sel.size:
                raise ValueError("no gene has a Moran's I in any time point: nothing to test")
        res = local_moran(st.edges, dc, sel, values, n_perms=n_perms, seed=seed)
    torch.cuda.synchronize(st.dev)
    t_dev = time.perf_counter()
    arrays = dict(timepoints=np.asarray(tps), genes=np.asarray(dc.genes).astype(str)[sel], k=np.int64(k), n_perms=np.int64(n_perms),
                  seed=np.int64(seed), alpha=np.float64(alpha))
    tables, arrays = write_timepoints(st.path, "hotspots", tps, res, lambda t, r: hotspot_table(r, dc.genes, alpha, fdr), FIELDS,
                                      arrays, lambda t, r: {"spots": np.asarray(dc.perm[st.rows(t)], dtype=np.int64)})
    domain_tables = {}
    if labels is not None:
        domain_tables, _ = write_timepoints(st.path, "hotspots_domains", tps, res, lambda t, r: domain_table(
            r, dc.genes, labels[dc.perm[st.rows(t)]], alpha, fdr), ())
    savez_pinned(st.path("hotspots.npz"), arrays)
    t_end = time.perf_counter()
    print(f"hotspots: {sel.size} genes x {dc.n} spots of {dc.T} time points, k = {k}, {n_perms} permutations, written to "
          f"{args.output_dir}", file=sys.stderr)
    return {"tables": tables, "domain_tables": domain_tables, "results": dict(zip(tps, res)), "genes": sel, "timepoints": tps,
            "timings": timings(st.t_start, st.t_read, t_dev, t_end, st.t_graph)}
