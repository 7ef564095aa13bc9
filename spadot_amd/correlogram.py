"""The correlogram stage: HOW FAR the spatial structure of a gene reaches.  Moran's I of every selected gene over the pairs of spots
in successive distance bands, its twin the empirical semivariogram, and the range, the distance at which the autocorrelation stops
(spdep's sp.correlogram, gstat's variogram; csrc/correlogram.hip).  The reference has no such stage; the definition is
restated in numpy in tests/correlogram_ref.py.

    corr_sums(coords, data | Z=, genes, radii | radii_sq, n_perms)   the device primitive: W, S2c, N, Q
    corr_stats(W, S2c, N, Q, n, m2, radii, sumsq, alpha)             the host part of one time point
    correlogram(coords, dc | dense, genes=None, radii=None, bins=12, n_perms=0, alpha=0.05, seed=0)   one CorrResult per time point
    default_bands(coords, bins=12)                                   pairs.ladder up to the r_max of pairs.default_radii
    correlogram_stage(args)   the stage.  args: data, output_dir, prefix (''), genes, top (50), bins (12), radii, n_perms (0), alpha
                              (0.05), seed (0), k (6; the graph behind --top), device

One time point: n spots with fp64 coordinates and squared thresholds r2_0 < .. < r2_{B-1}, 1 <= B <= 16, validated by
pairs.thresholds / pairs._squares (finite, >= 0, strictly increasing).  d2(i, j) is the unfused squared distance of the stages that
count pairs by distance (pc_d2 of csrc/pair_count.h: the only place where a distance is formed).  Band b holds the ordered pairs
(i, j), i != j, with r2_{b-1} < d2 <= r2_b, r2_{-1} below 0: coincident spots fall into band 0; pairs beyond r2_{B-1} are in no
band.  cnt_b(i) is the number of partners of spot i in band b.
Values are those of autocorr: the fp32 values of trends.lognorm_values promoted to fp64 (or dense columns through moran.columns),
with the centre c.  Labeling 0 is the identity; labeling 1 + p gives spot i the value x_i = v[pi_p(i)], pi_p the permutation of
neighbors.py's docstring under (seed, index of the time point, p, n): the convention of autocorr.  xc = x - c.  The device computes
    W[b] = sum_i cnt_b(i),   S2c[b] = sum_i cnt_b(i)^2                     (int64, exact while sum_i cnt_b(i)^2 < 2^63)
    N[g, l, b] = sum over the pairs of band b of xc_i xc_j,   Q[g, l, b] = sum_i cnt_b(i) xc_i^2       (fp64, a fixed order)
and the host, per band, with the band as a symmetric binary graph:
    D = 2 Q - 2 N          (sum (x_i - x_j)^2 over the ordered pairs of a symmetric band)
    S0 = W_b, S1 = 2 W_b, S2 = 4 S2c_b
    autocorr.autocorr_stats(N[:, :, b], D[:, :, b], n, E = W_b, m2, (S0, S1, S2), sumsq), unchanged: I_b, C_b, z_norm, p_norm, z_sim
    and p_sim where P >= 1, padj (Benjamini-Hochberg over the non-degenerate genes of one time point and band)
    gamma_b = (Q - N) / W_b                                                              (the semivariance)
A band with W_b = 0 and every degenerate gene (moran.degenerate) is NaN and left out of BH.  Per gene and time point:
    range    r_{b* - 1}, b* the number of LEADING bands with I_b > E[I] and padj_b < alpha (0.0 where b* = 0; NaN for a degenerate gene)
    open     b* = B: the structure reaches past the ladder
    I_first, gamma_first (band 0) and sill = m2 / n.

The spots of a time point go to the device in Morton order (graph.morton_key, ties by index) with `order`, position -> original
index: positions give the tiles of the kernel, which skips a tile out of reach of its query block; original indices go into the
permutation.  Limits: 1 to 16 bands, 1 to 4096 selected genes, at most 2147483391 spots per time point, permutation indices below
2^32."""
import sys
import time

import numpy as np

from .moran import Columns, centre_spread, columns, gene_selection, read_genes, top_genes
from .pairs import default_radii, thresholds
from .utils._stage_utils import labeling_runs, open_stage, plot_timepoints, savez_pinned, timings, top_setting, write_timepoints

MAX_BANDS = 16
FIELDS = ("I", "z_norm", "p_norm", "z_sim", "p_sim", "padj", "gamma")
TABLE_COLUMNS = ("gene", "band", "r_lo", "r_hi", "pairs") + FIELDS
SUMMARY_COLUMNS = ("timepoint", "gene", "range", "open", "I_first", "gamma_first", "sill")
ARRAYS = FIELDS + ("C", "N", "Q", "W", "S2c", "radii", "range", "open", "I_first", "gamma_first", "sill", "m2")
SCRATCH_DOUBLES = 2 ** 27          # the scratch of one launch (boxes and partial sums): at most 1 GiB, the labelings are split beyond
PLOT_GENES = 8
NO_CPU = "spadot_amd takes the correlogram on the MI355X only ({}); there is no CPU path"


def default_bands(coords, bins=12):
    """The stage's radii of one time point: pairs.ladder(r_max, bins) with the r_max of pairs.default_radii, a quarter of the
    diagonal of the bounding box.  ValueError outside 1 <= bins <= 16 and where the spots all coincide."""
    bins = int(bins)
    if not 1 <= bins <= MAX_BANDS:
        raise ValueError(f"the correlogram takes 1 to {MAX_BANDS} distance bands (got bins = {bins})")
    return default_radii(coords, bins)


def morton_order(xy):
    """position -> original index of the spots of one time point: ascending graph.morton_key, ties by index."""
    from .graph import morton_key
    xy = np.asarray(xy, dtype=np.float64)
    return np.lexsort((np.arange(xy.shape[0]), morton_key(xy))).astype(np.int32)


def _band_count(r, t):
    if not 1 <= r.shape[0] <= MAX_BANDS:
        raise ValueError(f"time point {t} has {r.shape[0]} distance bands: the correlogram takes 1 to {MAX_BANDS}")


def _image(cols, centre, sel):
    """The centred fp64 image Z [zrows, GP] of the selected genes (stage_ops.cross_layout; the image of cross_dense)."""
    import torch
    from . import stage_ops as ops
    T, dev = cols.T, cols.device
    sizes = np.diff(np.asarray(cols.tp_off_host, dtype=np.int64))
    zoff, zrows = ops.cross_layout(sizes)
    if cols.dense is not None:
        gl = torch.as_tensor(sel.astype(np.int64), device=dev)
        Z = torch.zeros((zrows, ops.cross_padded(sel.size)), dtype=torch.float64, device=dev)
        for t, x in enumerate(cols.dense):               # fp32 values promoted, minus the centre: the bits of the CSC part
            Z[int(zoff[t]):int(zoff[t]) + int(sizes[t]), :sel.size] = \
                x[:, gl].to(torch.float32).to(torch.float64) - centre[t, gl][None, :]
        return Z
    off = np.asarray(cols.tp_off_host, dtype=np.int64)
    desc = np.zeros((T, ops.CROSS_DESC), dtype=np.int64)                      # an empty graph: only the image is wanted
    roff = np.concatenate([[0], np.cumsum(sizes + 1)])[:-1]
    desc[:, 1], desc[:, 3], desc[:, 4], desc[:, 5], desc[:, 8] = sizes, off[:-1], np.arange(T), roff, zoff
    rowptr = torch.zeros(int((sizes + 1).sum()), dtype=torch.int32, device=dev)
    col = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (rowptr, col, cols.colptr, cols.ridx, cols.values, centre.contiguous(), torch.as_tensor(sel, device=dev))
    Z, _ = ops.cross_dense_launch(*args, ops.cross_dense_check(*args, desc))
    return Z


def corr_sums(coords, data=None, genes=None, values=None, centre=None, radii=None, radii_sq=None, n_perms=0, seed=0, first=0,
              observed=True, cull=True, cs=None, Z=None, graph_ids=None, images=False, skipped=False, out=None):
    """W, S2c, N and Q of every (time point, selected gene, labeling, band) (module docstring).  coords[t]: the fp64 device
    tensor [n_t, 2] of time point t; data: a DeviceCounts (values: its fp32 device values in CSC order, default
    trends.lognorm_values) or, per time point, a dense float32 / float64 device tensor [n_t, C], with centre fp64 [T, G] (default:
    moran.centre_spread) and genes, integer gene (column) indices (default: all) -- or Z[t]: the centred values themselves as an
    fp64 device tensor [n_t, genes].  Exactly one of radii[t] and radii_sq[t], the ends of the bands of time point t.
    Labelings: the identity first (observed), then the permutations first .. first + n_perms - 1 under seed, time point t under
    graph_ids[t] (default t).  cull: skip the tiles out of reach (the same bits either way); cs: genes per workgroup, 2 or 4
    (the same bits either way).  A long run is split into launches of at most SCRATCH_DOUBLES doubles of scratch, with the same bits (ValueError where
    one labeling alone needs more).
    Returns (W, S2c, N, Q): [t] -> int64 numpy [B_t] twice, fp64 numpy [genes, labelings, B_t] twice; with images=True also [t] ->
    the image fp64 numpy [n_t, genes]; with skipped=True also the number of skipped tiles of the (first) launch.  out: four
    device tensors to write into, taken by a call that is one launch.  ValueError / RuntimeError before any launch."""
    import torch
    from . import stage_ops as ops
    if not coords or any(not isinstance(xy, torch.Tensor) or not xy.is_cuda for xy in coords):
        raise RuntimeError(NO_CPU.format("the coordinates are not device tensors"))
    T, dev = len(coords), coords[0].device
    n_perms, first, observed = int(n_perms), int(first), bool(observed)
    if n_perms < 0:
        raise ValueError(f"the number of permutations must not be negative (got n_perms = {n_perms})")
    ops.labelings("corr_sums", observed, first, n_perms)
    for t, xy in enumerate(coords):
        if xy.dim() != 2 or xy.shape[1] != 2 or xy.shape[0] < 1 or not xy.dtype.is_floating_point or xy.device != dev:
            raise ValueError(f"the coordinates of time point {t} must form a floating-point [n, 2] block of at least one spot on "
                             f"one device (got {tuple(xy.shape)} {xy.dtype})")
    sizes = np.asarray([int(xy.shape[0]) for xy in coords], dtype=np.int64)
    r2 = thresholds("corr_sums", T, radii, radii_sq)
    for t, r in enumerate(r2):
        _band_count(r, t)
    gids = np.arange(T, dtype=np.int64) if graph_ids is None else np.asarray(graph_ids, dtype=np.int64).reshape(-1)
    if gids.shape[0] != T:
        raise ValueError(f"graph_ids holds {gids.shape[0]} numbers for {T} time points")
    zoff, zrows = ops.cross_layout(sizes)
    with torch.cuda.device(dev):
        if Z is not None:
            if data is not None or len(Z) != T:
                raise ValueError(f"corr_sums takes the data or one centred block Z per time point ({T} time points)")
            ng = int(Z[0].shape[1]) if isinstance(Z[0], torch.Tensor) and Z[0].dim() == 2 else 0
            img = torch.zeros((zrows, ops.cross_padded(max(ng, 1))), dtype=torch.float64, device=dev)
            for t, z in enumerate(Z):
                if not isinstance(z, torch.Tensor) or not z.is_cuda:
                    raise RuntimeError(NO_CPU.format("the values of time point %d are not a device tensor" % t))
                if z.dtype != torch.float64 or tuple(z.shape) != (int(sizes[t]), ng) or ng < 1:
                    raise ValueError(f"Z[{t}] must be an fp64 tensor [{int(sizes[t])}, genes] (got {tuple(z.shape)} {z.dtype})")
                img[int(zoff[t]):int(zoff[t]) + int(sizes[t]), :ng] = z
        else:
            cols = data if isinstance(data, Columns) else columns(data, values)
            if cols.device != dev:
                raise ValueError("the coordinates and the data lie on one device")
            if cols.T != T or np.any(np.diff(np.asarray(cols.tp_off_host, dtype=np.int64)) != sizes):
                raise ValueError(f"the coordinates hold {sizes.tolist()} spots in {T} time points; the data holds "
                                 f"{np.diff(np.asarray(cols.tp_off_host)).tolist()}")
            sel = gene_selection(np.arange(cols.G) if genes is None else genes, cols.G)
            if sel.size > ops.CORR_MAX_G:
                raise ValueError(f"corr_sums takes at most {ops.CORR_MAX_G} selected genes (got {sel.size})")
            if centre is None:
                centre = centre_spread(cols)[1]
            centre = centre if isinstance(centre, torch.Tensor) else torch.as_tensor(np.asarray(centre, dtype=np.float64), device=dev)
            if tuple(centre.shape) != (T, cols.G) or centre.dtype != torch.float64:
                raise ValueError(f"centre must be fp64 [T, G] = [{T}, {cols.G}] (got {tuple(centre.shape)} {centre.dtype})")
            ng, img = int(sel.size), _image(cols, centre, sel)
        host = [xy.detach().to(torch.float64).cpu().numpy() for xy in coords]
        orders = [morton_order(h) for h in host]
        order = torch.as_tensor(np.concatenate(orders), device=dev)
        xy = torch.cat([c.to(torch.float64)[torch.as_tensor(o.astype(np.int64), device=dev)] for c, o in zip(coords, orders)])
        xy = xy.contiguous()
        boff, blocks = ops.corr_layout(sizes)
        desc = np.zeros((T, ops.CORR_DESC), dtype=np.int64)
        desc[:, 0], desc[:, 1] = np.concatenate([[0], np.cumsum(sizes)])[:-1], sizes
        desc[:, 2], desc[:, 3], desc[:, 4], desc[:, 5] = [len(r) for r in r2], gids, zoff, boff
        B_max = int(desc[:, 2].max())
        chunks = -(-ng // int(cs or ops.CORR_CS))
        per = 2 * blocks * ng * B_max                        # the partials of one labeling; the boxes come once per launch
        if 4 * blocks + per > SCRATCH_DOUBLES:
            raise ValueError(f"one labeling alone needs {4 * blocks + per} doubles of scratch, more than the {SCRATCH_DOUBLES} of a "
                             f"launch: split the genes or the time points over several calls")
        budget = min(SCRATCH_DOUBLES - 4 * blocks, per * max(1, ops.CORR_MAX_Y // chunks))
        runs = labeling_runs(n_perms, observed, first, per, budget)
        obs0, p0, np0 = runs[0]
        checked = ops.corr_check(xy, order, img, desc, r2, ng, obs0, p0, np0, cs)
        skip = torch.zeros(1, dtype=torch.int64, device=dev) if skipped else None
        if len(runs) == 1:
            W, S2c, N, Q = ops.corr_launch(xy, order, img, checked, ng, seed, cull, cs, out, None, skip)
        else:                                                # the labelings in runs that share one scratch buffer
            if out is not None:
                raise ValueError("out is taken only by a call that is one launch")
            scratch = torch.empty(ops.corr_scratch_doubles(blocks, ng, int(obs0) + np0, B_max), dtype=torch.float64, device=dev)
            desc_dev, r2_dev = torch.as_tensor(checked[0], device=dev), torch.as_tensor(checked[1], device=dev)
            parts = [ops.corr_launch(xy, order, img, checked[:3] + (int(o), p, m), ng, seed, cull, cs, None, scratch,
                                     skip if i == 0 else None, desc_dev, r2_dev) for i, (o, p, m) in enumerate(runs)]
            W, S2c = parts[0][0], parts[0][1]
            N, Q = (torch.cat([p[i] for p in parts], dim=2) for i in (2, 3))
        L = int(observed) + n_perms
        W, S2c = W.reshape(T, B_max).cpu().numpy(), S2c.reshape(T, B_max).cpu().numpy()
        N, Q = N.reshape(T, ng, L, B_max).cpu().numpy(), Q.reshape(T, ng, L, B_max).cpu().numpy()
        res = tuple([a[t][..., :len(r2[t])] for t in range(T)] for a in (W, S2c, N, Q))
        if images:
            Zh = img.cpu().numpy()
            res += ([Zh[int(z):int(z) + int(n), :ng] for z, n in zip(zoff, sizes)],)
        if skipped:
            res += (int(skip.item()),)
    return res


class CorrResult:
    """One time point: per selected gene and band the fp64 statistics of the module docstring (FIELDS and C, [genes, B]), the
    device's sums N, Q [genes, 1 + P, B] and W, S2c [B], radii [B], per gene `range`, `open`, I_first, gamma_first, sill and m2,
    `degenerate` [genes] bool, `genes` (the selection), n, P and alpha."""

    def __init__(self, W, S2c, N, Q, n, m2, sumsq, radii, genes, alpha):
        self.W, self.S2c, self.N, self.Q, self.n, self.m2 = W, S2c, N, Q, int(n), np.asarray(m2, dtype=np.float64)
        self.radii, self.genes, self.P, self.alpha = np.asarray(radii, dtype=np.float64), np.asarray(genes), N.shape[1] - 1, alpha
        for name, v in corr_stats(W, S2c, N, Q, n, m2, radii, sumsq, alpha).items():
            setattr(self, name, v)


def corr_stats(W, S2c, N, Q, n, m2, radii, sumsq=None, alpha=0.05):
    """The host part of one time point (module docstring).  W, S2c: int64 [B]; N, Q: fp64 [genes, 1 + P, B], labeling 0 the
    observed one; m2 [genes]; radii [B]; sumsq [genes]: sum v^2 of the degeneracy rule (None: degenerate where m2 <= 0).  Returns
    a dict: I, C, z_norm, p_norm, z_sim, p_sim, padj, gamma fp64 [genes, B]; range, I_first, gamma_first, sill fp64 [genes]; open
    and degenerate bool [genes]."""
    from .autocorr import autocorr_stats
    from .moran import degenerate
    N, Q = np.asarray(N, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    W, S2c, radii = np.asarray(W, dtype=np.int64), np.asarray(S2c, dtype=np.int64), np.asarray(radii, dtype=np.float64)
    m2 = np.asarray(m2, dtype=np.float64)
    G, B, n = N.shape[0], N.shape[2], int(n)
    if W.shape != (B,) or S2c.shape != (B,) or radii.shape != (B,) or Q.shape != N.shape or m2.shape != (G,):
        raise ValueError(f"corr_stats takes W, S2c and radii [B], N and Q [genes, labelings, B] and m2 [genes] (got {W.shape}, "
                         f"{S2c.shape}, {radii.shape}, {N.shape}, {Q.shape}, {m2.shape})")
    out = {k: np.full((G, B), np.nan) for k in ("I", "C") + FIELDS[1:]}
    bad = degenerate(n, 1, m2, sumsq)                        # what the data decide; an empty band is NaN for every gene
    D = 2.0 * Q - 2.0 * N
    for b in range(B):
        if W[b] == 0:
            continue
        s = autocorr_stats(N[:, :, b], D[:, :, b], n, int(W[b]), m2, (int(W[b]), 2 * int(W[b]), 4 * int(S2c[b])), sumsq=sumsq)
        out["C"][:, b] = s["C"]
        for name in FIELDS[:-1]:
            out[name][:, b] = s[name if name == "I" else name + "_I"]
        out["gamma"][:, b] = np.where(s["degenerate"], np.nan, (Q[:, 0, b] - N[:, 0, b]) / float(W[b]))
    expected = -1.0 / (n - 1.0) if n > 1 else np.nan
    with np.errstate(invalid="ignore"):
        ok = (out["I"] > expected) & (out["padj"] < alpha)                    # NaN compares false: the run of bands ends there
    lead = np.where(ok.all(axis=1), B, np.argmin(ok, axis=1))                 # the number of leading bands that hold
    ends = np.concatenate([[0.0], radii])
    out["range"] = np.where(bad, np.nan, ends[lead])
    out["open"] = ~bad & (lead == B)
    out["I_first"], out["gamma_first"] = out["I"][:, 0].copy(), out["gamma"][:, 0].copy()
    out["sill"] = np.where(bad, np.nan, m2 / max(n, 1))
    out["degenerate"] = bad
    return out


def _radii_per_timepoint(radii, coords, bins):
    if radii is None:
        return [default_bands(xy, bins) for xy in coords]
    flat = np.asarray(radii[0] if len(radii) else [], dtype=np.float64)
    if flat.ndim == 0:                                       # one ladder for every time point
        return [np.asarray(radii, dtype=np.float64).reshape(-1)] * len(coords)
    return [np.asarray(r, dtype=np.float64).reshape(-1) for r in radii]


def correlogram(coords, data, genes=None, values=None, radii=None, bins=12, n_perms=0, alpha=0.05, seed=0, cull=True):
    """The correlogram of every selected gene of every time point (module docstring).  coords[t]: the device tensor [n_t, 2] of
    time point t; data: a DeviceCounts (values: its fp32 values in CSC order, default trends.lognorm_values) or, per time point,
    a dense float32 / float64 device tensor [n_t, C]; genes: gene (column) indices (default: all, at most 4096); radii: one
    increasing list of band ends for all time points or one per time point (default: default_bands(coords[t], bins)).  Time point
    t permutes under (seed, t).  Returns [t] -> CorrResult."""
    import torch
    n_perms, alpha = int(n_perms), float(alpha)
    if n_perms < 0 or not 0.0 < alpha <= 1.0:
        raise ValueError(f"the correlogram takes n_perms >= 0 and 0 < alpha <= 1 (got n_perms = {n_perms}, alpha = {alpha})")
    if not coords or any(not isinstance(xy, torch.Tensor) or not xy.is_cuda for xy in coords):
        raise RuntimeError(NO_CPU.format("the coordinates are not device tensors"))
    radii = _radii_per_timepoint(radii, coords, bins)
    cols = columns(data, values)
    sel = gene_selection(np.arange(cols.G) if genes is None else genes, cols.G)
    with torch.cuda.device(cols.device):
        _, centre, m2, S2 = centre_spread(cols)
        W, S2c, N, Q = corr_sums(coords, cols, sel, centre=centre, radii=radii, n_perms=n_perms, seed=seed, cull=cull)
        m2, S2 = m2.cpu().numpy()[:, sel], S2.cpu().numpy()[:, sel]
    return [CorrResult(W[t], S2c[t], N[t], Q[t], int(coords[t].shape[0]), m2[t], S2[t], radii[t], sel, alpha)
            for t in range(len(coords))]


def correlogram_table(r, names):
    """The rows of {prefix}correlogram_{tp}.csv, long format: one per (selected gene, band), genes in the order of the selection."""
    import pandas as pd
    G, B = r.I.shape
    lo = np.concatenate([[0.0], r.radii[:-1]])
    cols = {"gene": np.repeat(np.asarray(names)[r.genes], B), "band": np.tile(np.arange(B), G), "r_lo": np.tile(lo, G),
            "r_hi": np.tile(r.radii, G), "pairs": np.tile(np.asarray(r.W, dtype=np.int64), G)}
    cols.update({name: getattr(r, name).reshape(-1) for name in FIELDS})
    return pd.DataFrame(cols, columns=list(TABLE_COLUMNS))


def correlogram_summary(tps, results, names):
    """The rows of {prefix}correlogram_summary.csv: one per (time point, selected gene)."""
    import pandas as pd
    frames = [pd.DataFrame({"timepoint": tp, "gene": np.asarray(names)[r.genes], "range": r.range, "open": r.open.astype(np.int64),
                            "I_first": r.I_first, "gamma_first": r.gamma_first, "sill": r.sill}, columns=list(SUMMARY_COLUMNS))
              for tp, r in zip(tps, results)]
    return pd.concat(frames, ignore_index=True)


def parse_radii(spec):
    """The band ends of --radii: a comma-separated list of 1 to 16 finite radii >= 0 in strictly increasing order."""
    try:
        r = np.asarray([float(w) for w in str(spec).split(",") if w.strip()], dtype=np.float64)
    except ValueError:
        raise ValueError(f"--radii takes a comma-separated list of numbers (got {spec!r})") from None
    if not 1 <= r.size <= MAX_BANDS or not np.all(np.isfinite(r)) or np.any(r < 0) or np.any(np.diff(r) <= 0):
        raise ValueError(f"--radii takes 1 to {MAX_BANDS} finite radii >= 0 in strictly increasing order (got {spec!r})")
    return r


def _plot(path, tp, r, names):
    from .utils import _analyze_utils
    from .moran import moran_order
    lead = moran_order(r.I_first)[:PLOT_GENES]
    lead = [g for g in lead if not np.isnan(r.I_first[g])]
    mids = 0.5 * (np.concatenate([[0.0], r.radii[:-1]]) + r.radii)
    _analyze_utils.plot_correlogram(path, mids, r.I[lead], -1.0 / max(r.n - 1, 1), np.asarray(names)[r.genes][lead], tp)


def correlogram_stage(args):
    """Reads args.data (counts, as the autocorr stage: coordinates from obsm['spatial']) and runs one correlogram call on the genes
    of args.genes (a comma list of names or a file with one name per line) or, without it, on the union over the time points of
    the args.top genes by Moran's I (one spatial_autocorr call without permutations on the args.k nearest neighbours, as
    hotspots).  Bands: args.radii (a comma list, for every time point) or args.bins equal bands per time point (default_bands).
    Writes {prefix}correlogram_{tp}.csv (TABLE_COLUMNS, long format), {prefix}correlogram_summary.csv (SUMMARY_COLUMNS),
    {prefix}correlogram.npz ('{tp}_{field}' for ARRAYS, plus timepoints, genes, n_perms, seed, alpha; pinned time stamps: two runs
    with one seed write the same bytes) and, where matplotlib is installed, {prefix}{tp}_correlogram.png.  Returns {'tables',
    'summary', 'results' (per time point), 'genes', 'timepoints', 'timings'}."""
    import torch
    from .autocorr import spatial_autocorr
    from .trends import lognorm_values
    t_start = time.perf_counter()

    def arg(name, default, kind):
        v = getattr(args, name, default)
        return kind(default if v is None else v)

    top, k, bins, n_perms = top_setting(args, 50), arg("k", 6, int), arg("bins", 12, int), arg("n_perms", 0, int)
    seed, alpha = arg("seed", 0, int), arg("alpha", 0.05, float)
    if top < 1 or k < 1 or not 1 <= bins <= MAX_BANDS or n_perms < 0 or not 0.0 < alpha <= 1.0:
        raise ValueError(f"the correlogram stage takes top >= 1, k >= 1, 1 <= bins <= {MAX_BANDS}, n_perms >= 0 and 0 < alpha <= 1 "
                         f"(got top = {top}, k = {k}, bins = {bins}, n_perms = {n_perms}, alpha = {alpha})")
    radii = parse_radii(args.radii) if getattr(args, "radii", None) is not None else None
    st = open_stage(args, k, "the correlogram", t_start,
                    lambda raw: read_genes(args.genes, raw.var_names) if getattr(args, "genes", None) else None)
    sel, dc, tps = st.extras, st.dc, st.tps
    with torch.cuda.device(st.dev):
        values = lognorm_values(dc)
        if sel is None:                                      # the top genes by Moran's I of every time point, unioned
            sel = top_genes(spatial_autocorr(st.edges, dc, values, n_perms=0), top)
            if not sel.size:
                raise ValueError("no gene has a Moran's I in any time point: nothing to test")
        coords = [torch.as_tensor(np.ascontiguousarray(dc.spatial[st.rows(t)]), device=st.dev) for t in range(dc.T)]
        res = correlogram(coords, dc, sel, values, radii=None if radii is None else [radii] * dc.T, bins=bins, n_perms=n_perms,
                          alpha=alpha, seed=seed)
    torch.cuda.synchronize(st.dev)
    t_dev = time.perf_counter()
    arrays = dict(timepoints=np.asarray(tps), genes=np.asarray(dc.genes).astype(str)[sel], n_perms=np.int64(n_perms),
                  seed=np.int64(seed), alpha=np.float64(alpha))
    tables, arrays = write_timepoints(st.path, "correlogram", tps, res, lambda t, r: correlogram_table(r, dc.genes), ARRAYS, arrays)
    summary = correlogram_summary(tps, res, dc.genes)
    summary.to_csv(st.path("correlogram_summary.csv"), index=False)
    savez_pinned(st.path("correlogram.npz"), arrays)
    plot_timepoints(tps, res, lambda tp, r: _plot(st.path(f"{tp}_correlogram.png"), tp, r, dc.genes))
    t_end = time.perf_counter()
    print(f"correlogram: {sel.size} genes x {dc.n} spots of {dc.T} time points, {max(len(r.radii) for r in res)} bands, {n_perms} "
          f"permutations, written to {args.output_dir}", file=sys.stderr)
    return {"tables": tables, "summary": summary, "results": dict(zip(tps, res)), "genes": sel, "timepoints": tps,
            "timings": timings(st.t_start, st.t_read, t_dev, t_end, st.t_graph)}
