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

The device counts; the host validates, takes the statistics and writes the files.  Limits: 1 <= K <= 32, 1 <= B <= 64, at most
2147483391 spots per problem and 65535 problems per call."""
import os
import sys
import time

import numpy as np

from .utils._stage_utils import savez_pinned

MAX_CLUSTERS = 32
MAX_BINS = 64
MAX_SPOTS = 2147483391
MAX_PROBLEMS = 65535
TABLE_COLUMNS = ("domain", "neighbor", "radius", "count", "ratio")
ARRAYS = ("counts", "ratio", "radii", "sizes")
NO_CPU = "spadot_amd counts co-occurrences on the MI355X only ({}); there is no CPU path"


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


def _bounding_box(xy):
    """(min x, max x, min y, max y) of an [n, 2] array or tensor as Python floats."""
    if hasattr(xy, "is_cuda"):
        import torch
        if xy.dim() != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
            raise ValueError(f"coords must be an [n, 2] array of at least one spot (got {tuple(xy.shape)})")
        lo, hi = torch.aminmax(xy.to(torch.float64), dim=0)
        lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    else:
        xy = np.asarray(xy, dtype=np.float64)
        if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
            raise ValueError(f"coords must be an [n, 2] array of at least one spot (got {xy.shape})")
        lo, hi = xy.min(axis=0), xy.max(axis=0)
    return float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1])


def ladder(r_max, bins):
    """The radii r_max * (1 .. bins) / bins."""
    bins, r_max = int(bins), float(r_max)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"the co-occurrence takes 1 to {MAX_BINS} radii (got bins = {bins})")
    if not np.isfinite(r_max) or r_max <= 0:
        raise ValueError(f"the largest radius must be finite and above 0 (got {r_max})")
    return r_max * np.arange(1, bins + 1) / bins


def default_radii(coords, bins=50):
    """The stage's radii of one time point: r_max = 0.25 * hypot(max x - min x, max y - min y), radii = r_max * (1 .. bins) /
    bins.  ValueError where the spots all coincide (or are not finite)."""
    x0, x1, y0, y1 = _bounding_box(coords)
    r_max = 0.25 * np.hypot(x1 - x0, y1 - y0)
    if not np.isfinite(r_max):
        raise ValueError("the coordinates must be finite")
    if r_max <= 0:
        raise ValueError("the spots all coincide: there is no distance to bin (give radii)")
    return ladder(r_max, bins)


def _squares(radii, g):
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if not 1 <= r.shape[0] <= MAX_BINS:
        raise ValueError(f"problem {g} has {r.shape[0]} radii: the device takes 1 to {MAX_BINS}")
    if not np.all(np.isfinite(r)) or np.any(r < 0) or np.any(np.diff(r) <= 0):
        raise ValueError(f"the radii of problem {g} must be finite, >= 0 and strictly increasing")
    return r * r


def sorted_problems(coords, labels, n_clusters=None, no_cpu=NO_CPU):
    """What the stages that count by distance refuse about the spots and the labelings of a call, before any launch, and the
    layout they hand to the device.  Returns (the device, xy fp64 [sum n, 2] with every problem's spots ordered by (label,
    index), [g] -> K, int64 [P, 32] domain sizes); one host round trip."""
    import torch
    P = len(coords)
    dev, xs, labs = None, [], []
    for g, (xy, lab) in enumerate(zip(coords, labels)):
        if not isinstance(xy, torch.Tensor) or not xy.is_cuda:
            raise RuntimeError(no_cpu.format("the coordinates of problem %d are not a device tensor" % g))
        if xy.dim() != 2 or xy.shape[1] != 2 or xy.shape[0] < 1 or not xy.dtype.is_floating_point:
            raise ValueError(f"the coordinates of problem {g} must form a floating-point [n, 2] block of at least one spot "
                             f"(got {tuple(xy.shape)} {xy.dtype})")
        if dev is not None and xy.device != dev:
            raise ValueError("all problems of a call lie on one device")
        dev = xy.device
        if xy.shape[0] > MAX_SPOTS:
            raise ValueError(f"problem {g} has {xy.shape[0]} spots: the device takes at most {MAX_SPOTS} per problem")
        lab = lab if isinstance(lab, torch.Tensor) else torch.as_tensor(np.asarray(lab))
        if lab.dtype.is_floating_point or lab.dtype == torch.bool or lab.dtype.is_complex:
            raise ValueError(f"labels must be integers (problem {g}: {lab.dtype})")
        if lab.dim() != 1 or lab.shape[0] != xy.shape[0]:
            raise ValueError(f"problem {g} has {xy.shape[0]} spots and a labeling of shape {tuple(lab.shape)}")
        xs.append(xy.to(torch.float64))
        labs.append(lab.to(dev).long())
    with torch.cuda.device(dev):
        stats = []
        for xy, lab in zip(xs, labs):
            lo, hi = torch.aminmax(lab)
            hist = torch.bincount(lab.clamp(0, MAX_CLUSTERS), minlength=MAX_CLUSTERS + 1)[:MAX_CLUSTERS]
            stats.append(torch.cat([torch.stack([lo, hi, torch.isfinite(xy).all().long()]), hist]))
        stats = torch.stack(stats).cpu().numpy()                       # the one host round trip ahead of the launch
        Ks = []
        for g in range(P):
            lo, hi, finite = (int(v) for v in stats[g, :3])
            K = hi + 1 if n_clusters is None else int(n_clusters[g])
            if not 1 <= K <= MAX_CLUSTERS:
                raise ValueError(f"problem {g} has {K} label values: the device counts 1 to {MAX_CLUSTERS} domains")
            if lo < 0 or hi >= K:
                raise ValueError(f"problem {g} holds labels {lo} .. {hi}: labels must lie in 0 .. {K - 1}")
            if not finite:
                raise ValueError(f"problem {g} holds coordinates that are not finite")
            Ks.append(K)
        # the spots of every problem by (label, index): a stable sort of the labels
        xy = torch.cat([x[torch.sort(lab, stable=True)[1]] for x, lab in zip(xs, labs)]).contiguous()
    return dev, xy, Ks, stats[:, 3:]


def cooccurrence_counts(coords, labels, radii=None, radii_sq=None, n_clusters=None, out=None):
    """coords[g]: the fp64 [n, 2] device tensor of problem g; labels[g]: its integer labeling (numpy or torch); radii[g] its
    radii in the units of the coordinates, or radii_sq[g] their squares (exactly one of the two); n_clusters[g]: its K (default:
    its largest label + 1).  One call to the library for all problems; returns [g] -> int64 numpy [K, K, B].  ValueError /
    RuntimeError before any launch; out: an int64 device tensor [P, K_max, K_max, B_max] to write into."""
    import torch
    from . import stage_ops as ops
    if (radii is None) == (radii_sq is None):
        raise ValueError("cooccurrence_counts takes exactly one of radii and radii_sq")
    given = radii if radii is not None else radii_sq
    P = len(coords)
    if P < 1 or len(labels) != P or len(given) != P:
        raise ValueError(f"cooccurrence_counts takes one labeling and one set of radii per problem ({P} problems, {len(labels)} "
                         f"labelings, {len(given)} sets of radii)")
    if n_clusters is not None and len(n_clusters) != P:
        raise ValueError(f"n_clusters holds {len(n_clusters)} cluster counts for {P} problems")
    if P > MAX_PROBLEMS:
        raise ValueError(f"the call holds {P} problems: the device takes at most {MAX_PROBLEMS} per call")
    r2 = []
    for g, r in enumerate(given):
        t = _squares(r, g) if radii is not None else np.asarray(r, dtype=np.float64).reshape(-1)
        r2.append(t)                                     # two radii that differ may still have one square: checked as squares too
        if not 1 <= t.shape[0] <= MAX_BINS:
            raise ValueError(f"problem {g} has {t.shape[0]} thresholds: the device takes 1 to {MAX_BINS}")
        if not np.all(np.isfinite(t)) or np.any(t < 0) or np.any(np.diff(t) <= 0):
            raise ValueError(f"the squared thresholds of problem {g} must be finite, >= 0 and strictly increasing")
    dev, xy, Ks, sizes = sorted_problems(coords, labels, n_clusters)
    with torch.cuda.device(dev):
        desc = np.zeros((P, ops.COOCCUR_DESC), dtype=np.int64)
        first = 0
        for g in range(P):
            n = int(sizes[g].sum())
            desc[g, :4] = (first, n, Ks[g], r2[g].shape[0])
            desc[g, 5:5 + Ks[g]] = np.cumsum(sizes[g, :Ks[g]])
            first += n
        K_max, B_max = max(Ks), max(t.shape[0] for t in r2)
        res = ops.cooccur_counts(xy, desc, r2, K_max, B_max, out=out).cpu().numpy()
    return [np.ascontiguousarray(res[g, :Ks[g], :Ks[g], :r2[g].shape[0]]) for g in range(P)]


def cooccurrence(coords, labels, radii=None, bins=50, ring=False, n_clusters=None):
    """The co-occurrence of every problem (module docstring): coords[g] fp64 [n, 2] device tensors, labels[g] integers, radii[g]
    the radii of problem g (default: default_radii(coords[g], bins)).  One call to the library.  Returns [g] -> CooccurResult."""
    import torch
    for g, xy in enumerate(coords):
        if not isinstance(xy, torch.Tensor) or not xy.is_cuda:
            raise RuntimeError(NO_CPU.format("the coordinates of problem %d are not a device tensor" % g))
    if radii is None:
        radii = [default_radii(xy, bins) for xy in coords]
    radii = [np.asarray(r, dtype=np.float64).reshape(-1) for r in radii]
    counts = cooccurrence_counts(coords, labels, radii=radii, n_clusters=n_clusters)
    out = []
    for g, N in enumerate(counts):
        lab = labels[g].cpu().numpy() if isinstance(labels[g], torch.Tensor) else np.asarray(labels[g])
        out.append(CooccurResult(N, radii[g], np.bincount(lab, minlength=N.shape[0]).astype(np.int64), ring))
    return out


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
    {prefix}{tp}_cooccurrence.png.  Returns {'tables', 'results' (per time point), 'timepoints', 'timings'}."""
    import pandas as pd
    from .markers import read_domains
    from .utils import _analyze_utils
    t_start = time.perf_counter()
    domains = getattr(args, "domains", None)
    if domains is None or (isinstance(domains, str) and not domains):
        raise ValueError("the cooccurrence stage needs the domains table of analyze (--domains)")
    df = pd.read_csv(domains) if isinstance(domains, (str, os.PathLike)) else domains
    for col in ("pixel_x", "pixel_y", "timepoint", "kmeans"):
        if col not in df.columns:
            raise ValueError(f"the domains table has no `{col}` column (expected the domains.csv that analyze writes)")
    n = len(df)
    if n == 0:
        raise ValueError("the domains table is empty")
    tp_all = np.asarray(df["timepoint"])
    labels = read_domains(df.assign(row=np.arange(n)), tp_all).astype(np.int64)     # the table's own order; K <= 32 per time point
    coords = np.stack([np.asarray(df["pixel_x"], dtype=np.float64), np.asarray(df["pixel_y"], dtype=np.float64)], axis=1)
    if not np.all(np.isfinite(coords)):
        raise ValueError("the domains table holds spots without finite pixel_x / pixel_y")
    bins, ring, radius = int(getattr(args, "bins", 50)), bool(getattr(args, "ring", False)), getattr(args, "radius", None)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"the cooccurrence stage takes 1 to {MAX_BINS} radii (got bins = {bins})")
    if not getattr(args, "output_dir", None):
        args.output_dir = (os.path.dirname(os.path.abspath(domains)) if isinstance(domains, (str, os.PathLike))
                           else os.getcwd())
    os.makedirs(args.output_dir, exist_ok=True)
    prefix = getattr(args, "prefix", "") or ""
    device = getattr(args, "device", None) or "cuda:0"

    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(NO_CPU.format("device 'cuda:N'"))
    tps = sorted(set(tp_all.tolist()))
    masks = [tp_all == tp for tp in tps]
    radii = [ladder(radius, bins) if radius is not None else default_radii(coords[m], bins) for m in masks]
    t_read = time.perf_counter()
    res = cooccurrence([torch.as_tensor(coords[m], device=dev) for m in masks], [labels[m] for m in masks], radii=radii,
                       ring=ring, n_clusters=[int(labels[m].max()) + 1 for m in masks])
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter()

    tables, arrays = {}, {"timepoints": np.asarray(tps), "bins": np.int64(bins), "ring": np.bool_(ring)}
    for tp, r in zip(tps, res):
        tables[tp] = cooccurrence_table(r)
        tables[tp].to_csv(os.path.join(args.output_dir, f"{prefix}cooccurrence_{tp}.csv"), index=False)
        for name in ARRAYS:
            arrays[f"{tp}_{name}"] = getattr(r, name)
    savez_pinned(os.path.join(args.output_dir, prefix + "cooccurrence.npz"), arrays)
    if _analyze_utils.have_matplotlib():
        for tp, r in zip(tps, res):
            _analyze_utils.plot_cooccurrence(os.path.join(args.output_dir, f"{prefix}{tp}_cooccurrence.png"), r.radii, r.ratio,
                                             tp, ring)
    else:
        print("matplotlib not installed: no plots")
    t_end = time.perf_counter()
    print(f"cooccurrence: {n} spots of {len(tps)} time points, {bins} radii{' (rings)' if ring else ''}, written to "
          f"{args.output_dir}", file=sys.stderr)
    return {"tables": tables, "results": dict(zip(tps, res)), "timepoints": tps,
            "timings": dict(read_s=t_read - t_start, device_s=t_dev - t_read, write_s=t_end - t_dev, total_s=t_end - t_start)}
