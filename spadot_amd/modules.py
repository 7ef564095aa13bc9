"""The modules stage: WHICH spatially structured genes go together.  The bivariate Moran's I (esda.Moran_BV, symmetrised) of every
pair of selected genes on the spatial k-nearest-neighbour graph of every time point, with a permutation null, and the spatial
gene modules that average-linkage clustering cuts out of it (csrc/crossmoran.hip).  The reference has no such stage;
the definition is restated in numpy in tests/modules_ref.py.

    cross_sums(edges, dc | dense, values, centre, genes, n_perms)   the device primitive: M of every (time point, labeling)
    cross_moran(edges, dc | dense, genes, n_perms=100)              R, z_sim, p_sim, padj of every pair of every time point
    gene_modules(R, ok, min_sim=0.15, min_genes=2)                  the modules of one time point (host, scipy)
    module_scores(z, m2, n, labels)                                 the score of every module in every spot (device, fp64)
    module_overlap(a, b)                                            the Jaccard index of every pair of modules of two time points
    modules(args)     the stage.  args: data, output_dir, prefix (''), k (6), n_perms (100), seed (0), genes, top (100), min_sim
                      (0.15), min_genes (2), alpha (0.05), top_pairs (0 = all), device

One time point: n spots and directed edges i -> j (duplicates count; E of them), sorted stably by source into a CSR as in
hotspots.  Per selected gene, v is the fp32 values of trends.lognorm_values (0 where nothing is stored) promoted to fp64, c and m2
the centre and the spread of autocorr, z = v - c, and the lag
    Y[i, h] = ((0 + z_h[j1]) + z_h[j2]) + ...          over the row of i in row order (the bits of hotspots.local_lag's lag).
Labeling 0 is the identity; labeling 1 + p uses pi_p, the permutation of neighbors.py's docstring under (seed, index of the time
point, p, n).  The device computes, on the fp64 matrix cores,
    M[l, g, h] = sum_i z_g[pi_l(i)] Y[i, h]
-- the permuted gene moves against the FIXED lag of the other one (moving both together would keep their cross-correlation and
is no null) -- and, with torch ops on the device, B[l] = (M[l] + M[l]^T) / 2 and ge[g, h] = #{p : |B[1 + p, g, h]| >= |B[0, g, h]|}.
The host:
    R[g, h] = n B[0, g, h] / (E sqrt(m2_g m2_h))      (the diagonal is the Moran's I of autocorr: the same E terms in another order)
    p_sim = (1 + ge) / (P + 1)                        (two-sided), z_sim from the mean and sd (ddof 0) of R_p
    padj: Benjamini-Hochberg over the pairs g < h of non-degenerate genes of one time point
A gene that autocorr calls degenerate in a time point (n < 3, E = 0 or m2 <= n 2^-50 sum v^2) gives NaN in its row and column and
stays out of the family.  A permutation null, not an analytic one: the lag of an autocorrelated gene has more energy than that of
a white one, so no variance that knows the graph alone is right for the genes this stage is about.

Modules of a time point: among the selected genes that are not degenerate and have R[g, g] > 0, scipy's average linkage on the
distance 1 - R (condensed upper triangle, genes ascending), cut with fcluster(.., 1 - min_sim, 'distance'); clusters of fewer
than min_genes genes get the label -1; the others are numbered by their smallest gene.  The score of a module in a spot is the mean
over its genes of z_g / sqrt(m2_g / n).  Out of scope: weighted, radius or symmetrised graphs, Lee's L, a bivariate LOCAL Moran,
cross terms between time points, other clusterings.

Limits: 1 to 4096 selected genes; at most 2147483647 spots and edges per time point; permutation indices below 2^32."""
import sys
import time

import numpy as np

from .moran import centre_spread, columns, degenerate, edge_csr, gene_selection, read_genes, top_genes
from .utils._stage_utils import edge_pair, labeling_runs, open_stage, savez_pinned, timings, top_setting, write_timepoints

FIELDS = ("R", "z_sim", "p_sim", "padj")
TABLE_COLUMNS = ("gene", "module", "I", "R_own", "best_other", "R_other")
PAIR_COLUMNS = ("gene_a", "gene_b", "R", "z_sim", "p_sim", "padj", "same_module")
OVERLAP_COLUMNS = ("timepoint_a", "module_a", "timepoint_b", "module_b", "n_a", "n_b", "n_both", "jaccard")
SCRATCH_BYTES = 2 ** 29            # the cross sums of one launch: the labelings are split beyond that
MIN_SIM, MIN_GENES = 0.15, 2


class CrossResult:
    """One time point: R, z_sim, p_sim, padj fp64 [genes, genes] (symmetric; NaN in the row and column of a degenerate gene, padj
    NaN on the diagonal too), ge int64 [genes, genes], I = diag R, m2 and `mean` (the centre) [genes], `degenerate` [genes] bool,
    n, E, P, `genes` (the selection, gene indices) and z, the centred values as an fp64 DEVICE tensor [n, genes]."""

    def __init__(self, B0, ge, s1, s2, mean, m2, n, E, P, degenerate, genes, z):
        from .markers import bh_adjust
        self.n, self.E, self.P, self.genes, self.z = int(n), int(E), int(P), np.asarray(genes), z
        self.mean, self.m2, self.degenerate, self.ge = mean, m2, np.asarray(degenerate, dtype=bool), ge
        G = B0.shape[0]
        bad = self.degenerate[:, None] | self.degenerate[None, :]
        safe = np.where(self.degenerate, 1.0, m2)
        with np.errstate(invalid="ignore", divide="ignore"):
            R = self.n * B0 / (max(self.E, 1) * np.sqrt(safe[:, None] * safe[None, :]))
            if P >= 1:
                mu = s1 / P
                sd = np.sqrt(np.maximum(s2 / P - mu * mu, 0.0))
                z_sim = np.where(sd > 0, (B0 - mu) / np.where(sd > 0, sd, 1.0), np.nan)
                p_sim = (1.0 + ge) / (P + 1.0)
            else:
                z_sim, p_sim = np.full((G, G), np.nan), np.full((G, G), np.nan)
        padj = np.full((G, G), np.nan)
        a, b = np.triu_indices(G, 1)
        fam = ~bad[a, b]
        if P >= 1 and fam.any():
            padj[a[fam], b[fam]] = bh_adjust(p_sim[a[fam], b[fam]])
            padj[b[fam], a[fam]] = padj[a[fam], b[fam]]
        self.R, self.z_sim, self.p_sim, self.padj = (np.where(bad, np.nan, v) for v in (R, z_sim, p_sim, padj))
        self.I = np.diagonal(self.R).copy()


class _Images:
    """Z and Y of a call on the device with what the launches take."""


def _images(edges, cols, centre, genes):
    """The images of a call (module docstring) over the Columns `cols`: a DeviceCounts goes through spadot_cross_dense's CSC
    part, dense columns enter as Z directly.  Every refusal comes before any launch."""
    import torch
    from . import stage_ops as ops
    im = _Images()
    T, G, dev = cols.T, cols.G, cols.device
    off = np.asarray(cols.tp_off_host, dtype=np.int64)
    if not edges or len(edges) != T:
        raise ValueError(f"cross_sums takes one edge list per time point ({len(edges) if edges else 0} lists, {T} time points)")
    pairs = [edge_pair(e, dev, t) for t, e in enumerate(edges)]
    centre = centre if isinstance(centre, torch.Tensor) else torch.as_tensor(np.asarray(centre, dtype=np.float64), device=dev)
    if tuple(centre.shape) != (T, G) or centre.dtype != torch.float64:
        raise ValueError(f"centre must be fp64 [T, G] = [{T}, {G}] (got {tuple(centre.shape)} {centre.dtype})")
    sel = gene_selection(genes, G)
    if sel.size > ops.CROSS_MAX_G:
        raise ValueError(f"cross_sums takes at most {ops.CROSS_MAX_G} selected genes (got {sel.size})")
    sizes = np.diff(off)
    with torch.cuda.device(dev):
        rowptr, col, d8 = edge_csr(pairs, sizes, dev)
        desc = np.zeros((T, ops.CROSS_DESC), dtype=np.int64)
        desc[:, :8] = d8
        desc[:, 3] = off[:-1]
        zoff, zrows = ops.cross_layout(sizes)
        desc[:, 8] = zoff
        centre = centre.contiguous()
        if cols.dense is None:
            gsel = torch.as_tensor(sel, device=dev)
            args = (rowptr, col, cols.colptr, cols.ridx, cols.values, centre, gsel)
            Z, Y = ops.cross_dense_launch(*args, ops.cross_dense_check(*args, desc))
        else:
            gl = torch.as_tensor(sel.astype(np.int64), device=dev)
            Z = torch.zeros((zrows, ops.cross_padded(sel.size)), dtype=torch.float64, device=dev)
            for t, x in enumerate(cols.dense):               # fp32 values promoted, minus the centre: the bits of the CSC part
                Z[int(zoff[t]):int(zoff[t]) + int(sizes[t]), :sel.size] = \
                    x[:, gl].to(torch.float32).to(torch.float64) - centre[t, gl][None, :]
            args = (rowptr, col, None, None, None, None, int(sel.size))
            Z, Y = ops.cross_dense_launch(*args, ops.cross_dense_check(*args, desc, Z), Z)
    im.Z, im.Y, im.desc, im.sel, im.T, im.sizes, im.zoff, im.device = Z, Y, desc, sel, T, sizes, zoff, dev
    im.E = [int(s.numel()) for s, _ in pairs]
    return im


def _runs(im, n_perms, seed, first, observed):
    """Yields (observed in the run, its first permutation, its permutations, M fp64 device [T, labelings, genes, genes]) of the
    runs of a call: every run is one launch, and every check comes before the first one."""
    import torch
    from . import stage_ops as ops
    ng = int(im.sel.size)
    ops.cross_check(im.Z, im.Y, im.desc, ng, observed, first, n_perms)
    runs = labeling_runs(n_perms, observed, first, im.T * ng * ng * 8, SCRATCH_BYTES)
    with torch.cuda.device(im.device):
        desc_dev = torch.as_tensor(im.desc, device=im.device)
        for obs, p0, npm in runs:
            yield obs, p0, npm, ops.cross_launch(im.Z, im.Y, im.desc, ng, obs, p0, npm, seed, None, desc_dev)


def cross_sums(edges, data, values, centre, genes, n_perms, seed=0, first=0, observed=True, images=False):
    """M of every (time point, labeling) (module docstring).  edges[t]: (src, dst) integer device tensors of time point t; data:
    a DeviceCounts (values: fp32 device tensor, one per stored entry in CSC order) or, per time point, a dense float32 / float64
    device tensor [n, C] (values None); centre: fp64 [T, G] (device tensor or array); genes: integer gene (column) indices, any
    order, repeats allowed.  Labelings: the identity first (observed), then the permutations first .. first + n_perms - 1 under
    seed, time point t as graph index t; a long run is split into launches of at most SCRATCH_BYTES of sums, with the same
    bits.  Returns [t] -> fp64 numpy [labelings, genes, genes]; with images=True also [t] -> (Z, Y) fp64 numpy [n_t, genes].
    ValueError / RuntimeError before any launch."""
    import torch
    n_perms, first, observed = int(n_perms), int(first), bool(observed)
    if n_perms < 0:
        raise ValueError(f"the number of permutations must not be negative (got n_perms = {n_perms})")
    from .stage_ops import labelings
    labelings("cross_sums", observed, first, n_perms)        # ahead of the launches that build the images
    if hasattr(data, "colptr") and not isinstance(values, torch.Tensor):
        raise RuntimeError("cross_sums takes the values as a device tensor (torch), not a host array")
    im = _images(edges, columns(data, values), centre, genes)
    M = torch.cat([m for _, _, _, m in _runs(im, n_perms, seed, first, observed)], dim=1).cpu().numpy()
    out = [M[t] for t in range(im.T)]
    if not images:
        return out
    Z, Y, ng = im.Z.cpu().numpy(), im.Y.cpu().numpy(), im.sel.size
    return out, [(Z[int(z):int(z) + int(n), :ng], Y[int(z):int(z) + int(n), :ng]) for z, n in zip(im.zoff, im.sizes)]


def cross_moran(edges, data, genes, values=None, n_perms=100, seed=0):
    """The bivariate Moran's I of every pair of the selected genes in every time point, with its permutation null (module
    docstring).  edges[t]: (src, dst) device tensors of time point t (spatial_edges); data: a DeviceCounts (values: its fp32
    values in CSC order, default trends.lognorm_values) or, per time point, a dense float32 / float64 device tensor [n, C] of
    columns such as fates or memberships, taken as fp32; genes: gene (column) indices.  Time point t permutes under (seed, t).
    The fold of the sums into B, the comparison and the counts are torch ops on the device, run by run: no [P, genes, genes] block
    goes to the host.  Returns [t] -> CrossResult."""
    import torch
    n_perms = int(n_perms)
    if n_perms < 0:
        raise ValueError(f"the number of permutations must not be negative (got n_perms = {n_perms})")
    cols = columns(data, values)
    sel = gene_selection(genes, cols.G)
    with torch.cuda.device(cols.device):
        _, centre, m2, S2 = centre_spread(cols)
        im = _images(edges, cols, centre, sel)
        G = int(sel.size)
        B0 = None
        ge = torch.zeros((im.T, G, G), dtype=torch.int64, device=cols.device)
        s1 = torch.zeros((im.T, G, G), dtype=torch.float64, device=cols.device)
        s2 = torch.zeros_like(s1)
        for obs, _p0, npm, M in _runs(im, n_perms, seed, 0, True):
            B = 0.5 * (M + M.transpose(2, 3))
            if obs:
                B0 = B[:, 0].clone()
                B = B[:, 1:]
            if npm:
                ge += (B.abs() >= B0.abs()[:, None]).sum(1)
                s1 += B.sum(1)
                s2 += (B * B).sum(1)
            del B, M
        B0, ge, s1, s2 = (v.cpu().numpy() for v in (B0, ge, s1, s2))
        centre, m2, S2 = centre.cpu().numpy()[:, sel], m2.cpu().numpy()[:, sel], S2.cpu().numpy()[:, sel]
    res = []
    for t in range(im.T):
        n, E = int(im.sizes[t]), im.E[t]
        z = im.Z[int(im.zoff[t]):int(im.zoff[t]) + n, :G]
        res.append(CrossResult(B0[t], ge[t], s1[t], s2[t], centre[t], m2[t], n, E, n_perms,
                               degenerate(n, E, m2[t], S2[t]), sel, z))
    return res


def gene_modules(R, ok, min_sim=MIN_SIM, min_genes=MIN_GENES):
    """The module of every gene of one time point (module docstring): int64 [genes], -1 for a gene outside every module.  R:
    [genes, genes]; ok [genes] bool: the genes that may join (not degenerate); of those, the ones with R[g, g] > 0 are
    clustered."""
    from scipy.cluster.hierarchy import fcluster, linkage
    R, ok = np.asarray(R, dtype=np.float64), np.asarray(ok, dtype=bool).reshape(-1)
    G = ok.size
    if R.shape != (G, G) or not min_sim <= 1.0 or int(min_genes) < 1:
        raise ValueError(f"gene_modules takes R [genes, genes], ok [genes], min_sim <= 1 and min_genes >= 1 (got R {R.shape}, "
                         f"{G} genes, min_sim = {min_sim}, min_genes = {min_genes})")
    with np.errstate(invalid="ignore"):
        use = np.flatnonzero(ok & (np.diagonal(R) > 0))
    labels = np.full(G, -1, dtype=np.int64)
    if use.size == 0:
        return labels
    if use.size == 1:
        cut = np.ones(1, dtype=np.int64)
    else:
        sub = R[np.ix_(use, use)]
        if not np.all(np.isfinite(sub)):
            raise ValueError("R holds entries that are not finite between genes that may join a module")
        a, b = np.triu_indices(use.size, 1)
        cut = fcluster(linkage(1.0 - sub[a, b], method="average"), 1.0 - float(min_sim), criterion="distance")
    number = 0
    for c in sorted(set(cut.tolist()), key=lambda c: int(use[cut == c].min())):      # numbered by the smallest gene
        members = use[cut == c]
        if members.size >= int(min_genes):
            labels[members] = number
            number += 1
    return labels


def module_scores(z, m2, n, labels):
    """The score of every module in every spot: the mean over the module's genes, in ascending order, of z_g / sqrt(m2_g / n).
    z: fp64 device tensor [n, genes]; m2 [genes]; labels: gene_modules' result.  fp64 torch ops on the device; returns numpy
    [modules, n]."""
    import torch
    if not isinstance(z, torch.Tensor) or not z.is_cuda:
        raise RuntimeError("module_scores takes the centred values as a device tensor; there is no CPU path")
    labels, m2 = np.asarray(labels, dtype=np.int64).reshape(-1), np.asarray(m2, dtype=np.float64).reshape(-1)
    K = int(labels.max()) + 1 if labels.size else 0
    out = torch.zeros((max(K, 0), int(z.shape[0])), dtype=torch.float64, device=z.device)
    for k in range(K):
        members = np.flatnonzero(labels == k)
        for g in members:                                    # one gene after the other: a fixed order of the additions
            out[k] += z[:, int(g)].to(torch.float64) / float(np.sqrt(m2[g] / float(n)))
        out[k] /= float(members.size)
    return out.cpu().numpy()


def module_overlap(a, b):
    """The Jaccard index of every (module of a, module of b): fp64 [modules of a, modules of b], with the sizes of the
    intersections (int64, same shape).  a, b: the labels of the same genes in two time points (-1: no module)."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    if a.shape != b.shape:
        raise ValueError(f"module_overlap takes the labels of the same genes (got {a.size} and {b.size})")
    Ka, Kb = (int(v.max()) + 1 if v.size else 0 for v in (a, b))
    both = np.zeros((max(Ka, 0), max(Kb, 0)), dtype=np.int64)
    inside = (a >= 0) & (b >= 0)
    np.add.at(both, (a[inside], b[inside]), 1)
    na, nb = np.bincount(a[a >= 0], minlength=Ka)[:, None], np.bincount(b[b >= 0], minlength=Kb)[None, :]
    return both / np.maximum(na + nb - both, 1), both


def module_table(r, names, labels):
    """The rows of {prefix}modules_{tp}.csv, one per selected gene: its module, its Moran's I, the mean R to the other genes of
    its module (NaN outside every module and alone in one) and the module, other than its own, with the largest mean R to its
    genes (-1 and NaN if there is none)."""
    import pandas as pd
    G, K = r.R.shape[0], int(labels.max()) + 1 if labels.size else 0
    own, best, other = np.full(G, np.nan), np.full(G, -1, dtype=np.int64), np.full(G, np.nan)
    for g in range(G):
        if r.degenerate[g]:
            continue
        for k in range(K):
            members = np.flatnonzero((labels == k) & (np.arange(G) != g))
            if members.size == 0:
                continue
            mean = float(r.R[g, members].mean())
            if k == labels[g]:
                own[g] = mean
            elif np.isnan(other[g]) or mean > other[g]:
                best[g], other[g] = k, mean
    return pd.DataFrame({"gene": np.asarray(names)[r.genes], "module": labels, "I": r.I, "R_own": own, "best_other": best,
                         "R_other": other}, columns=list(TABLE_COLUMNS))


def pair_table(r, names, labels, top_pairs=0):
    """The rows of {prefix}modules_pairs_{tp}.csv: the pairs g < h of non-degenerate selected genes by descending |R| (then by
    position), the first top_pairs of them (0 = all)."""
    import pandas as pd
    a, b = np.triu_indices(r.R.shape[0], 1)
    keep = ~(r.degenerate[a] | r.degenerate[b])
    a, b = a[keep], b[keep]
    order = np.argsort(-np.abs(r.R[a, b]), kind="stable")
    if top_pairs:
        order = order[:int(top_pairs)]
    a, b = a[order], b[order]
    names = np.asarray(names)[r.genes]
    return pd.DataFrame({"gene_a": names[a], "gene_b": names[b], "R": r.R[a, b], "z_sim": r.z_sim[a, b], "p_sim": r.p_sim[a, b],
                         "padj": r.padj[a, b], "same_module": ((labels[a] >= 0) & (labels[a] == labels[b])).astype(np.int64)},
                        columns=list(PAIR_COLUMNS))


def overlap_table(tps, labels):
    """The rows of {prefix}modules_overlap.csv: every (module, module) of every two consecutive time points."""
    import pandas as pd
    rows = []
    for (ta, la), (tb, lb) in zip(zip(tps, labels), zip(tps[1:], labels[1:])):
        jac, both = module_overlap(la, lb)
        for i in range(jac.shape[0]):
            for j in range(jac.shape[1]):
                rows.append((ta, i, tb, j, int((la == i).sum()), int((lb == j).sum()), int(both[i, j]), float(jac[i, j])))
    return pd.DataFrame(rows, columns=list(OVERLAP_COLUMNS))


def modules(args):
    """Reads args.data (counts, as the autocorr stage: coordinates from obsm['spatial']), builds spatial_edges(.., k) of every time
    point and runs one cross_moran call on the genes of args.genes (a comma list of names or a file with one name per line) or,
    without it, on the union over the time points of the args.top genes by Moran's I (one spatial_autocorr call without
    permutations, as hotspots).  Writes {prefix}modules_{tp}.csv (TABLE_COLUMNS), {prefix}modules_pairs_{tp}.csv (PAIR_COLUMNS;
    args.top_pairs rows, 0 = all), {prefix}modules_overlap.csv (OVERLAP_COLUMNS) and {prefix}modules.npz ('{tp}_{field}' for
    FIELDS [genes, genes], '{tp}_module' [genes], '{tp}_scores' [modules, n_t] and '{tp}_spots', the rows of the data behind the
    columns, plus timepoints, genes, k, n_perms, seed, min_sim, min_genes, alpha; pinned time stamps: two runs with one seed write
    the same bytes).  Returns {'tables', 'pair_tables', 'overlap', 'results', 'modules', 'scores' (per time point), 'genes',
    'timepoints', 'timings'}."""
    import torch
    from .autocorr import spatial_autocorr
    from .trends import lognorm_values
    t_start = time.perf_counter()

    def arg(name, default, kind):
        v = getattr(args, name, default)
        return kind(default if v is None else v)

    top, k, n_perms, seed = top_setting(args, 100), arg("k", 6, int), arg("n_perms", 100, int), arg("seed", 0, int)
    min_sim, min_genes, alpha = arg("min_sim", MIN_SIM, float), arg("min_genes", MIN_GENES, int), arg("alpha", 0.05, float)
    top_pairs = arg("top_pairs", 0, int)
    if top < 1 or k < 1 or n_perms < 1 or not min_sim <= 1.0 or min_genes < 1 or not 0.0 < alpha <= 1.0 or top_pairs < 0:
        raise ValueError(f"the modules stage takes top >= 1, k >= 1, n_perms >= 1, min_sim <= 1, min_genes >= 1, 0 < alpha <= 1 and "
                         f"top_pairs >= 0 (got top = {top}, k = {k}, n_perms = {n_perms}, min_sim = {min_sim}, min_genes = "
                         f"{min_genes}, alpha = {alpha}, top_pairs = {top_pairs})")
    st = open_stage(args, k, "the gene modules", t_start,
                    lambda raw: read_genes(args.genes, raw.var_names) if getattr(args, "genes", None) else None)
    sel, dc, tps = st.extras, st.dc, st.tps
    with torch.cuda.device(st.dev):
        values = lognorm_values(dc)
        if sel is None:                                      # the top genes by Moran's I of every time point, unioned
            sel = top_genes(spatial_autocorr(st.edges, dc, values, n_perms=0), top)
            if not sel.size:
                raise ValueError("no gene has a Moran's I in any time point: nothing to group")
        res = cross_moran(st.edges, dc, sel, values, n_perms=n_perms, seed=seed)
        labels = [gene_modules(r.R, ~r.degenerate, min_sim, min_genes) for r in res]
        scores = [module_scores(r.z, r.m2, r.n, lab) for r, lab in zip(res, labels)]
    torch.cuda.synchronize(st.dev)
    t_dev = time.perf_counter()
    arrays = dict(timepoints=np.asarray(tps), genes=np.asarray(dc.genes).astype(str)[sel], k=np.int64(k), n_perms=np.int64(n_perms),
                  seed=np.int64(seed), min_sim=np.float64(min_sim), min_genes=np.int64(min_genes), alpha=np.float64(alpha))
    tables, arrays = write_timepoints(st.path, "modules", tps, res, lambda t, r: module_table(r, dc.genes, labels[t]), FIELDS, arrays,
                                      lambda t, r: {"module": labels[t], "scores": scores[t],
                                                    "spots": np.asarray(dc.perm[st.rows(t)], dtype=np.int64)})
    pair_tables, _ = write_timepoints(st.path, "modules_pairs", tps, res, lambda t, r: pair_table(r, dc.genes, labels[t], top_pairs), ())
    with np.errstate(invalid="ignore"):
        significant = sum(int((r.padj[np.triu_indices(sel.size, 1)] <= alpha).sum()) for r in res)
    overlap = overlap_table(tps, labels)
    overlap.to_csv(st.path("modules_overlap.csv"), index=False)
    savez_pinned(st.path("modules.npz"), arrays)
    t_end = time.perf_counter()
    print(f"modules: {sel.size} genes x {dc.n} spots of {dc.T} time points, k = {k}, {n_perms} permutations, "
          f"{sum(int(lab.max()) + 1 for lab in labels)} modules, {significant} pairs with padj <= {alpha}, written to "
          f"{args.output_dir}", file=sys.stderr)
    return {"tables": tables, "pair_tables": pair_tables, "overlap": overlap, "results": dict(zip(tps, res)),
            "modules": dict(zip(tps, labels)), "scores": dict(zip(tps, scores)), "genes": sel, "timepoints": tps,
            "timings": timings(st.t_start, st.t_read, t_dev, t_end, st.t_graph)}
