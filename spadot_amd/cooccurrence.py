"""The cooccurrence stage: how far the association of two domains reaches.  For every time point, every ordered pair of domains
and a ladder of radii, the number of pairs of spots within that distance, and from the integers the co-occurrence ratio of
squidpy's gr.co_occurrence (csrc/cooccur.hip).  `neighbors` sees one scale, the k nearest spots; this stage tells a
rim from a gradient and a compact domain from a scattered one.  The reference has no such stage; the definition is restated in
numpy in tests/cooccur_ref.py.

    cooccurrence_counts(coords, labels, radii)     the count arrays of many problems in ONE call to the library
    cooccurrence(coords, labels, radii, bins)      counts and statistics per problem
    cooccurrence_stats(counts, ring)               the host statistics from the integers
    default_radii(coords, bins)                    the stage's radii of one time point
    cooccur(args)      the stage.  args: domains ({prefix}domains.csv of analyze), output_dir, prefix (''), bins (50), radius
                       (None: a quarter of the bounding box's diagonal), ring (False), device

A problem is n >= 1 spots with fp64 coordinates (x, y), a labeling in 0 .. K-1 (1 <= K <= 32) and B radii r[0] < .. < r[B-1]
(1 <= B <= 64, >= 0, finite), compared as squares r2 = r * r formed in fp64 on the host:
    N[a, b, t] = #{ordered pairs (i, j), i != j : lab[i] = a, lab[j] = b, d2(i, j) <= r2[t]}            int64 [K, K, B]
    d2 = fl(fl(dx dx) + fl(dy dy)),  dx = x_i - x_j,  dy = y_i - y_j        five rounded fp64 operations, no fused multiply-add
A spot is never its own neighbour; two different spots at the same coordinates are a pair at distance 0.  In fp64 on the host
from the integers, with row[a, t] = sum_b N, col[b, t] = sum_a N, tot[t] = sum_ab N:
    cond[a, b, t] = N[a, b, t] / row[a, t]      the share of the spots within r_t of a spot of a that belong to b
    marg[b, t] = col[b, t] / tot[t]
    ratio[a, b, t] = cond / marg                NaN where row[a, t] = 0 or col[b, t] = 0; > 1: b is over-represented around a
With ring=True the same formulas on N[.., t] - N[.., t - 1] (N[.., -1] = 0): the pairs in the annulus (r_{t-1}, r_t].

The null (restated in tests/cooccur_null_ref.py): S >= 1 random relabelings under a seed and a problem number g.
    cooccurrence_null_counts(coords, labels, radii, n_perms, seed)     int64 [1 + S, K, K, B] per problem
    cooccurrence_null_stats(N, sizes, ring, alpha)                     the host statistics of one problem
    cooccurrence_null(coords, labels, radii, bins, ring, n_perms, ..)  a CooccurNullResult per problem
    cooccur(args) with args.n_perms = S (at most 9999), args.seed, args.alpha
Pattern 0 is the observed labeling; pattern s >= 1 leaves the labels on the spots stored by (label, index) and hands position j
the coordinates of position pi^-1(j), pi the Feistel permutation (seed, g, s - 1, n) of the neighbors and ripley stages.  The
domain sizes stay, so the integer N[s, a, b, t] itself is the test statistic (the cross-type K function A N / (n_a n_b) under
random labelling).  Per pair and radius, in fp64 from the integers (with ring on the differences along t; NaN where n_a = 0 or
n_b = 0, or a = b with n_a < 2): sim_mean, sim_min, sim_max, z = (N_0 - mean) / sd (population sd, NaN where sd = 0),
p_hi = (1 + #{s >= 1 : N_s >= N_0}) / (S + 1), p_lo with <=; the envelope of the ratio over the relabelings, for plotting only.
Per pair the global envelope test of the ripley stage on the integers over the radii (exact), Benjamini-Hochberg over the
unordered pairs a <= b of a problem (N is symmetric; cell (b, a) reports the padj of (a, b)), and `relation`: 'attract' or
'avoid' where padj <= alpha, by the sign of sum_t (N_0 - sim_mean), 'independent' otherwise.
CAVEAT: random labelling is a joint null.  A pair (R, A) reads significant when A alone is compact, even where R was placed
independently of A (the variance of sum_{i in R} #{A within r of i} over the choice of R is larger than under the null).  On the
45 x 45 planted set of the tests with an eighth label dealt to 300 spots at random (S = 39, seed 7, 20 default radii) the cell
(7, 7) has p_global 0.775 and reads 'independent', and all seven cells (7, c) have p_global 1 / 40.  Read an off-diagonal verdict
as "this pair is not a random labelling", not as "these two interact".

The device counts; the host validates, takes the statistics and writes the files.  Limits: 1 <= K <= 32, 1 <= B <= 64, at most
2147483391 spots per problem and 65535 problems per call."""
import sys
import time

import numpy as np

from .pairs import MAX_BINS, counted, default_radii, ladder, mad_p, sorted_problems, thresholds
from .pairs import MAX_CLUSTERS, MAX_PROBLEMS, MAX_SPOTS  # noqa: F401  (handed on with the names above: tests and tools import them from here)
from .utils._stage_utils import (cuda_device, open_output, plot_timepoints, read_domains_table, savez_pinned, timings,
                                 write_timepoints)

TABLE_COLUMNS = ("domain", "neighbor", "radius", "count", "ratio")
ARRAYS = ("counts", "ratio", "radii", "sizes")


class CooccurResult:
    """One problem: counts int64 [K, K, B], radii fp64 [B], sizes int64 [K], ring, and the fp64 statistics of the module
    docstring (cond, ratio [K, K, B]; marg [K, B])."""

    def __init__(self, counts, radii, sizes, ring=False):
        self.counts, self.radii, self.sizes, self.ring = counts, radii, sizes, bool(ring)
        for name, v in cooccurrence_stats(counts, ring).items():
            setattr(self, name, v)


def cooccurrence_stats(counts, ring=False):
    """The host statistics of one problem from its integers (module docstring): a dict of fp64 arrays cond, marg, ratio."""
    N = np.asarray(counts)
    if N.ndim != 3 or N.shape[0] != N.shape[1]:
        raise ValueError(f"counts must be a [K, K, B] array (got {N.shape})")
    N = N.astype(np.int64)
    if ring:
        N = np.diff(N, axis=2, prepend=0)
    row, col, tot = N.sum(axis=1), N.sum(axis=0), N.sum(axis=(0, 1))
    Nf = N.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(row[:, None, :] > 0, Nf / row[:, None, :], np.nan)
        marg = np.where(tot[None, :] > 0, col / tot[None, :].astype(np.float64), np.nan)
        ratio = np.where((row[:, None, :] > 0) & (col[None, :, :] > 0), cond / marg[None, :, :], np.nan)
    return dict(cond=cond, marg=marg, ratio=ratio)


def _layout(name, coords, labels, radii, radii_sq, n_clusters):
    """What cooccurrence_counts and cooccurrence_null_counts refuse about a call before any launch, and what they hand to the
    library: (the device, xy sorted by (label, index), [g] -> K, [g] -> squared thresholds, the descriptor int64 [P, 40])."""
    from . import stage_ops as ops
    P = len(coords)
    r2 = thresholds(name, P, radii, radii_sq, labelings=len(labels))
    dev, xy, Ks, sizes = sorted_problems(coords, labels, n_clusters)
    desc = np.zeros((P, ops.COOCCUR_DESC), dtype=np.int64)
    first = 0
    for g in range(P):
        n = int(sizes[g].sum())
        desc[g, :4] = (first, n, Ks[g], r2[g].shape[0])
        desc[g, 5:5 + Ks[g]] = np.cumsum(sizes[g, :Ks[g]])
        first += n
    return dev, xy, Ks, r2, desc


def cooccurrence_counts(coords, labels, radii=None, radii_sq=None, n_clusters=None, out=None):
    """coords[g]: the fp64 [n, 2] device tensor of problem g; labels[g]: its integer labeling (numpy or torch); radii[g] its
    radii in the units of the coordinates, or radii_sq[g] their squares (exactly one of the two); n_clusters[g]: its K (default:
    its largest label + 1).  One call to the library for all problems; returns [g] -> int64 numpy [K, K, B].  ValueError /
    RuntimeError before any launch; out: an int64 device tensor [P, K_max, K_max, B_max] to write into."""
    import torch
    from . import stage_ops as ops
    dev, xy, Ks, r2, desc = _layout("cooccurrence_counts", coords, labels, radii, radii_sq, n_clusters)
    with torch.cuda.device(dev):
        K_max, B_max = max(Ks), max(t.shape[0] for t in r2)
        res = ops.cooccur_counts(xy, desc, r2, K_max, B_max, out=out).cpu().numpy()
    return [np.ascontiguousarray(res[g, :Ks[g], :Ks[g], :r2[g].shape[0]]) for g in range(len(Ks))]


def cooccurrence(coords, labels, radii=None, bins=50, ring=False, n_clusters=None):
    """The co-occurrence of every problem (module docstring): coords[g] fp64 [n, 2] device tensors, labels[g] integers, radii[g]
    the radii of problem g (default: default_radii(coords[g], bins)).  One call to the library.  Returns [g] -> CooccurResult."""
    return [CooccurResult(N, r, sizes, ring) for N, r, sizes in
            counted(coords, labels, radii, bins, lambda r: cooccurrence_counts(coords, labels, radii=r, n_clusters=n_clusters))]


def cooccurrence_null_counts(coords, labels, radii=None, radii_sq=None, n_perms=99, seed=0, n_clusters=None, problem_ids=None,
                             max_bytes=256 << 20):
    """The counts of the observed labeling and of n_perms = S >= 1 relabelings of every problem (module docstring, the null):
    coords, labels, radii / radii_sq and n_clusters as for cooccurrence_counts; problem_ids[g]: the number g under which
    problem g draws its relabelings (default: its place in the call).  The relabelings are split into as many calls to the
    library as keep the device output of one call within max_bytes (at least one pattern per call); the observed labeling is
    counted in the first call only, and the result does not depend on max_bytes.  Returns [g] -> int64 numpy [1 + S, K, K, B]."""
    import torch
    from . import stage_ops as ops
    S = int(n_perms)
    if not 1 <= S <= 2 ** 31 - 1:
        raise ValueError(f"cooccurrence_null_counts takes 1 to {2 ** 31 - 1} relabelings (got n_perms = {S})")
    dev, xy, Ks, r2, desc = _layout("cooccurrence_null_counts", coords, labels, radii, radii_sq, n_clusters)
    P = len(Ks)
    gids = list(range(P)) if problem_ids is None else [int(v) for v in problem_ids]
    if len(gids) != P or any(not 0 <= v <= ops.COOCCUR_MAX_G for v in gids):
        raise ValueError(f"problem_ids holds one number in 0 .. {ops.COOCCUR_MAX_G} per problem")
    desc[:, ops.COOCCUR_DESC_G] = gids
    K_max, B_max = max(Ks), max(t.shape[0] for t in r2)
    per_call = int(min(max(int(max_bytes) // (8 * P * K_max * K_max * B_max), 1), ops.COOCCUR_MAX_Y))
    parts, first = [], 0
    with torch.cuda.device(dev):
        desc_dev = r2_dev = None
        while first < S:
            observed = 0 if parts else 1
            count = min(per_call - observed, S - first)
            checked = ops.cooccur_null_check(xy, desc, r2, K_max, B_max, observed, first, count)
            if desc_dev is None:
                desc_dev, r2_dev = torch.as_tensor(checked[0], device=dev), torch.as_tensor(checked[1], device=dev)
            parts.append(ops.cooccur_null_launch(xy, checked, K_max, B_max, seed, desc_dev=desc_dev, r2_dev=r2_dev).cpu().numpy())
            first += count
    res = np.concatenate(parts, axis=1)
    return [np.ascontiguousarray(res[g, :, :Ks[g], :Ks[g], :r2[g].shape[0]]) for g in range(P)]


def cooccurrence_null_stats(N, sizes, ring=False, alpha=0.05):
    """The host statistics of one problem's null from its integers (module docstring).  N int64 [1 + S, K, K, B], S >= 1; sizes
    [K].  Returns a dict: count int64 [K, K, B] (the tested integers: N[0], with ring its differences along t); sim_mean,
    sim_min, sim_max, z, p_lo, p_hi fp64 [K, K, B]; ratio (of pattern 0) and ratio_sim_mean, ratio_sim_min, ratio_sim_max (over
    the relabelings that define one) fp64 [K, K, B]; p_global, padj fp64 [K, K]; relation [K, K] of str."""
    from .markers import bh_adjust
    N = np.asarray(N)
    if N.ndim != 4 or N.shape[1] != N.shape[2] or N.shape[0] < 2:
        raise ValueError(f"the counts of a null must be a [1 + S, K, K, B] array with S >= 1 (got {N.shape})")
    N = N.astype(np.int64)
    S, K = N.shape[0] - 1, N.shape[1]
    nc = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if nc.shape[0] != K:
        raise ValueError(f"sizes holds {nc.shape[0]} domains and the counts {K}")
    T = np.diff(N, axis=3, prepend=0) if ring else N
    defined = (nc[:, None] > 0) & (nc[None, :] > 0) & ~(np.eye(K, dtype=bool) & (nc[:, None] < 2))
    obs, sim = T[0], T[1:]
    nan = np.where(defined, 0.0, np.nan)[:, :, None]                      # + nan: NaN in the cells without a value
    mean = sim.sum(axis=0, dtype=np.float64) / S                          # exact below 2^53, and no int64 sum that could wrap
    d = sim - mean
    sd = np.sqrt((d * d).sum(axis=0) / float(S))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd > 0, (obs - mean) / sd, np.nan)
    out = dict(count=obs.copy(), sim_mean=mean + nan, sim_min=sim.min(axis=0) + nan, sim_max=sim.max(axis=0) + nan, z=z + nan,
               p_lo=(1 + (sim <= obs).sum(axis=0)) / (S + 1.0) + nan, p_hi=(1 + (sim >= obs).sum(axis=0)) / (S + 1.0) + nan)
    # the envelope of the ratio, for plotting only: NaN-aware over the relabelings, one pattern at a time
    tot, cnt = np.zeros(obs.shape), np.zeros(obs.shape)
    lo, hi = np.full(obs.shape, np.inf), np.full(obs.shape, -np.inf)
    for s in range(1, S + 1):
        r = cooccurrence_stats(N[s], ring)["ratio"]
        ok = ~np.isnan(r)
        tot, cnt = tot + np.where(ok, r, 0.0), cnt + ok
        lo, hi = np.where(ok, np.minimum(lo, r), lo), np.where(ok, np.maximum(hi, r), hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        out.update(ratio=cooccurrence_stats(N[0], ring)["ratio"], ratio_sim_mean=np.where(cnt > 0, tot / cnt, np.nan),
                   ratio_sim_min=np.where(cnt > 0, lo, np.nan), ratio_sim_max=np.where(cnt > 0, hi, np.nan))
    p_global = np.where(defined, mad_p(T), np.nan)
    padj = np.full((K, K), np.nan)
    a, b = np.nonzero(np.triu(defined))                                   # N is symmetric: one test per unordered pair
    padj[a, b] = bh_adjust(p_global[a, b])
    padj[b, a] = padj[a, b]
    with np.errstate(invalid="ignore"):
        excess = (obs - mean).sum(axis=-1)
        relation = np.where(padj <= alpha, np.where(excess > 0, "attract", "avoid"), "independent")
    out.update(p_global=p_global, padj=padj, relation=relation)
    return out


NULL_STATS = ("count", "sim_mean", "sim_min", "sim_max", "z", "p_lo", "p_hi", "ratio", "ratio_sim_mean", "ratio_sim_min",
              "ratio_sim_max", "p_global", "padj", "relation")
NULL_TABLE_COLUMNS = ("domain", "neighbor", "radius") + NULL_STATS[:11]
NULL_SUMMARY_COLUMNS = ("timepoint", "domain", "neighbor", "n_domain", "n_neighbor", "p_global", "padj", "relation")
NULL_ARRAYS = ("null_counts", "radii", "sizes") + NULL_STATS[1:7] + NULL_STATS[8:]
MAX_RELABELINGS = 9999             # of the stage
MAX_TABLE_BYTES = 2 << 30          # of one time point's host table [1 + S, K, K, B] int64, in the stage


class CooccurNullResult(CooccurResult):
    """One problem under its null: the fields of the CooccurResult of pattern 0, null_counts int64 [1 + S, K, K, B], n_perms,
    seed, alpha and the statistics of cooccurrence_null_stats as attributes (count, sim_mean, sim_min, sim_max, z, p_lo, p_hi,
    ratio_sim_mean, ratio_sim_min, ratio_sim_max, p_global, padj, relation)."""

    def __init__(self, null_counts, radii, sizes, ring=False, seed=0, alpha=0.05):
        super().__init__(np.ascontiguousarray(null_counts[0]), radii, sizes, ring)
        self.null_counts, self.n_perms, self.seed, self.alpha = null_counts, null_counts.shape[0] - 1, int(seed), float(alpha)
        for name, v in cooccurrence_null_stats(null_counts, sizes, ring, alpha).items():
            setattr(self, name, v)


def cooccurrence_null(coords, labels, radii=None, bins=50, ring=False, n_perms=99, seed=0, alpha=0.05, n_clusters=None,
                      problem_ids=None, max_bytes=256 << 20):
    """The co-occurrence of every problem with its random-labelling null (module docstring): the arguments of cooccurrence and
    of cooccurrence_null_counts.  Returns [g] -> CooccurNullResult."""
    def count(r):
        return cooccurrence_null_counts(coords, labels, radii=r, n_perms=n_perms, seed=seed, n_clusters=n_clusters,
                                        problem_ids=problem_ids, max_bytes=max_bytes)
    return [CooccurNullResult(N, r, sizes, ring, seed, alpha) for N, r, sizes in counted(coords, labels, radii, bins, count, k_axis=1)]


def cooccurrence_null_table(r):
    """The rows of {prefix}cooccurrence_null_{tp}.csv: one per (domain, neighbor, radius), in the order of cooccurrence_table."""
    import pandas as pd
    K, _, B = r.counts.shape
    a, b, t = np.unravel_index(np.arange(K * K * B), (K, K, B))
    cols = {"domain": a, "neighbor": b, "radius": r.radii[t]}
    for name in NULL_TABLE_COLUMNS[3:]:
        cols[name] = getattr(r, name).reshape(-1)
    return pd.DataFrame(cols, columns=list(NULL_TABLE_COLUMNS))


def cooccurrence_null_summary(tps, results):
    """The rows of {prefix}cooccurrence_summary.csv: one per (time point, domain, neighbor)."""
    import pandas as pd
    rows = []
    for tp, r in zip(tps, results):
        K = r.counts.shape[0]
        for a in range(K):
            for b in range(K):
                rows.append((tp, a, b, int(r.sizes[a]), int(r.sizes[b]), r.p_global[a, b], r.padj[a, b], str(r.relation[a, b])))
    return pd.DataFrame(rows, columns=list(NULL_SUMMARY_COLUMNS))


def null_settings(args, K=None, bins=None):
    """(n_perms, seed, alpha) of the stage's arguments; ValueError for an n_perms below 0 or above 9999, and, where K and bins
    are given, for one whose host table of a time point, (1 + S) K^2 B 8 bytes, exceeds 2 GiB."""
    S, seed, alpha = int(getattr(args, "n_perms", 0) or 0), int(getattr(args, "seed", 0) or 0), float(getattr(args, "alpha", 0.05))
    if not 0 <= S <= MAX_RELABELINGS:
        raise ValueError(f"the cooccurrence stage takes 0 to {MAX_RELABELINGS} relabelings (got n_perms = {S})")
    if S and K is not None and (1 + S) * K * K * bins * 8 > MAX_TABLE_BYTES:
        raise ValueError(f"n_perms = {S} relabelings of K = {K} domains over B = {bins} radii need a table of "
                         f"{(1 + S) * K * K * bins * 8} bytes per time point: the limit is {MAX_TABLE_BYTES} (2 GiB)")
    return S, seed, alpha


def cooccurrence_table(r):
    """The rows of {prefix}cooccurrence_{tp}.csv: one per (domain, neighbor, radius), domain-major, then neighbor, then radius."""
    import pandas as pd
    K, _, B = r.counts.shape
    a, b, t = np.unravel_index(np.arange(K * K * B), (K, K, B))
    return pd.DataFrame({"domain": a, "neighbor": b, "radius": r.radii[t], "count": r.counts.reshape(-1),
                         "ratio": r.ratio.reshape(-1)}, columns=list(TABLE_COLUMNS))


def cooccur(args):
    """Reads args.domains (the domains.csv of analyze: row, timepoint, kmeans, pixel_x, pixel_y) and counts every time point in
    one call.  Radii per time point: default_radii(.., bins), or args.radius * (1 .. bins) / bins.  Writes
    {prefix}cooccurrence_{tp}.csv (TABLE_COLUMNS, one row per (domain, neighbor, radius)), {prefix}cooccurrence.npz
    ('{tp}_counts', '{tp}_ratio', '{tp}_radii', '{tp}_sizes', plus timepoints, bins, ring) and, with matplotlib,
    {prefix}{tp}_cooccurrence.png.  Returns {'tables', 'results' (per time point), 'timepoints', 'timings'}.
    With args.n_perms = S >= 1 (at most 9999; default 0: the files above and nothing else) every time point is also counted under
    S relabelings (args.seed, default 0; time point number g in sorted order draws under problem number g), the files above keep
    their bytes, and the files of _write_null are written beside them with verdicts at args.alpha (default 0.05); the result
    then also holds 'null_tables' and 'summary'."""
    from .utils import _analyze_utils
    t_start = time.perf_counter()
    null_settings(args)
    tab = read_domains_table(args, "cooccurrence")
    bins, ring, radius = int(getattr(args, "bins", 50)), bool(getattr(args, "ring", False)), getattr(args, "radius", None)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"the cooccurrence stage takes 1 to {MAX_BINS} radii (got bins = {bins})")
    out_file = open_output(args, tab.beside)

    import torch
    dev = cuda_device(args, "counts co-occurrences")
    tps, masks = tab.tps, tab.masks
    radii = [ladder(radius, bins) if radius is not None else default_radii(tab.coords[m], bins) for m in masks]
    n_perms, seed, alpha = null_settings(args, max(tab.Ks), bins)
    t_read = time.perf_counter()
    coords, labels = [torch.as_tensor(tab.coords[m], device=dev) for m in masks], [tab.labels[m] for m in masks]
    if n_perms == 0:
        res = cooccurrence(coords, labels, radii=radii, ring=ring, n_clusters=tab.Ks)
    else:                                                # time point number g in sorted order draws under problem number g
        res = cooccurrence_null(coords, labels, radii=radii, ring=ring, n_perms=n_perms, seed=seed, alpha=alpha, n_clusters=tab.Ks)
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter()

    head = {"timepoints": np.asarray(tps), "bins": np.int64(bins), "ring": np.bool_(ring)}
    tables, arrays = write_timepoints(out_file, "cooccurrence", tps, res, lambda t, r: cooccurrence_table(r), ARRAYS, dict(head))
    savez_pinned(out_file("cooccurrence.npz"), arrays)
    plot_timepoints(tps, res, lambda tp, r: _analyze_utils.plot_cooccurrence(out_file(f"{tp}_cooccurrence.png"), r.radii,
                                                                            r.ratio, tp, ring))
    out = {"tables": tables, "results": dict(zip(tps, res)), "timepoints": tps}
    if n_perms:
        out.update(_write_null(out_file, tps, res, head, ring))
    t_end = time.perf_counter()
    print(f"cooccurrence: {tab.n} spots of {len(tps)} time points, {bins} radii{' (rings)' if ring else ''}"
          f"{f', {n_perms} relabelings' if n_perms else ''}, written to {args.output_dir}", file=sys.stderr)
    out["timings"] = timings(t_start, t_read, t_dev, t_end)
    return out


def _write_null(out_file, tps, res, head, ring):
    """The files of the null beside the stage's own: {prefix}cooccurrence_null_{tp}.csv (NULL_TABLE_COLUMNS),
    {prefix}cooccurrence_summary.csv (NULL_SUMMARY_COLUMNS), {prefix}cooccurrence_null.npz ('{tp}_' + each of NULL_ARRAYS, plus
    timepoints, bins, ring -- `head` -- and n_perms, seed, alpha) and, with matplotlib, {prefix}{tp}_cooccurrence_null.png.
    Returns {'null_tables', 'summary'}."""
    from .utils import _analyze_utils
    r0 = res[0]
    head = dict(head, n_perms=np.int64(r0.n_perms), seed=np.int64(r0.seed), alpha=np.float64(r0.alpha))
    tables, arrays = write_timepoints(out_file, "cooccurrence_null", tps, res, lambda t, r: cooccurrence_null_table(r), NULL_ARRAYS,
                                      head)
    summary = cooccurrence_null_summary(tps, res)
    summary.to_csv(out_file("cooccurrence_summary.csv"), index=False)
    savez_pinned(out_file("cooccurrence_null.npz"), arrays)
    if _analyze_utils.have_matplotlib():
        for tp, r in zip(tps, res):
            _analyze_utils.plot_cooccurrence_null(out_file(f"{tp}_cooccurrence_null.png"), r.radii, r.ratio, r.ratio_sim_min,
                                                  r.ratio_sim_max, tp, ring, r.relation)
    return {"null_tables": tables, "summary": summary}
