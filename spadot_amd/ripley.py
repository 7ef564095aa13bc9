"""The ripley stage: the shape of one domain on its own.  For every time point and every domain, Ripley's point-pattern functions
L (pair density by radius), G (nearest-neighbour distance inside the domain) and F (empty-space distance from probe points to
the domain) against a Monte-Carlo envelope of simulated patterns, after squidpy's gr.ripley (csrc/ripley.hip): is the
domain one compact territory, a scatter of islands, or spots sprinkled through the tissue no differently from chance, and at
which scale.  The reference has no such stage; the definition is restated in numpy in tests/ripley_ref.py.

    convex_window(coords, window)                  the window of a problem: vertices, cumulative fan areas, area
    ripley_counts(coords, labels, radii, ...)      the integer arrays of many problems in ONE call to the library
    ripley_points(window, seed, g, stream, count)  the generated points of a stream (a simulated pattern to plot)
    ripley_stats(counts, sizes, area, n_probes)    the host statistics from the integers
    ripley(coords, labels, radii, bins, ...)       counts and statistics per problem
    ripley_stage(args)   the stage.  args: domains ({prefix}domains.csv of analyze), output_dir, prefix (''), bins (50), radius
                         (None: a quarter of the bounding box's diagonal), n_sim (99), n_probes (1000), null ('labels'), mode
                         ('L,G,F'), window ('hull'), alpha (0.05), seed (0), device

A problem is one time point: n >= 1 spots with fp64 (x, y), labels in 0 .. K-1 (1 <= K <= 32), B radii (1 <= B <= 64) compared as
squares r2 = r * r formed on the host, S >= 1 simulations, M >= 1 probe points, a seed and a problem number g.  The window W is
the convex hull of the spots (monotone chain in fp64 on the host, counter-clockwise, collinear points dropped), a convex polygon
of the caller's, or "box", the bounding box; at most 256 vertices.  Its area A is the shoelace formula; the device receives the
vertices and the cumulative areas cum[k] of the fan triangles (V0, V_{k+1}, V_{k+2}), a triangle whose area rounding makes
negative counting 0.  The hull is finished under the predicate of the device's window check (see _hull).

A generated point is a pure function of (seed, g, stream, index i): three 64-bit splitmix words at counter 3 i + j,
u_j = (w_j >> 11) 2^-53, the triangle the first k with fl(u_0 cum[last]) < cum[k], (u_1, u_2) reflected where u_1 + u_2 > 1, the
point (A + u_1 (B - A)) + u_2 (C - A), every operation rounded once.  Stream 0 is the problem's probe set (M points shared by all
domains and simulations), stream 1 + c S + s simulation s of domain c.

Domain c of n_c spots has 1 + S patterns of exactly n_c points: pattern 0 its spots; patterns 1 .. S under
    null="labels"   (default; the right null for spots on a lattice such as Visium or Stereo-seq bins) the spots that receive
                    label c when the Feistel permutation (seed, g, s) of the neighbors and autocorr stages relabels the spots
                    stored by (label, index): a gather, no stored permutation;
    null="csr"      (squidpy's) n_c generated points in W.
The device returns, per (domain c, pattern p, threshold t), with d2 the unfused squared distance of the cooccurrence stage:
    Lc = #{ordered pairs i != j of the pattern with d2 <= r2[t]}
    Gc = #{points of the pattern whose nearest other point has d2 <= r2[t]}     (two points at one place are neighbours at 0; a
                                                                                 lone point is never counted)
    Fc = #{probe points whose nearest point of the pattern has d2 <= r2[t]}
and the host, in fp64 from the integers:
    L = sqrt(A Lc / (pi n_c (n_c - 1)))     G = Gc / n_c     F = Fc / M         NaN: L and G where n_c < 2, F where n_c < 1
There is NO edge correction: the observed and the simulated patterns share W, so the bias is the same on both sides of every
comparison (read L against its envelope, not against the line L(r) = r).  Per statistic, domain and radius: the simulations' mean,
minimum and maximum and the pointwise p_hi = (1 + #{s : sim >= obs}) / (S + 1), p_lo with <=, compared on the integers.  Per
statistic and domain the global envelope (maximum absolute deviation) test over the 1 + S curves x_i:
    u_i = max_t |x_i(t) - mean_{k != i} x_k(t)| = max_t |(S + 1) x_i(t) - sum_k x_k(t)| / S       p_global = #{i : u_i >= u_0} / (S + 1)
(on the integers for G and F, in fp64 for L), Benjamini-Hochberg over the domains of a time point, and from L the `pattern`:
'clustered' or 'dispersed' where padj <= alpha, by the sign of sum_t (x_0 - mean of the simulations), 'random' otherwise.  A
statistic outside the modes of a call is not counted: NaN throughout, and without L the pattern is ''.

Limits: K <= 32, B <= 64, S <= 9999, M <= 1048576, 256 vertices, 2147483391 spots per problem, 65535 problems per call and
K (1 + S) <= 65535 patterns per problem."""
import collections
import sys
import time

import numpy as np

from .pairs import MAX_BINS, counted, default_radii, ladder, mad_p, sorted_problems, thresholds
from .utils._stage_utils import (cuda_device, open_output, plot_timepoints, read_domains_table, savez_pinned, timings,
                                 write_timepoints)

MAX_SIMULATIONS = 9999
MAX_PROBES = 1048576
MAX_VERTICES = 256
STATS = ("L", "G", "F")
NULLS = ("labels", "csr")
TABLE_COLUMNS = ("domain", "statistic", "radius", "observed", "sim_mean", "sim_min", "sim_max", "p_lo", "p_hi")
SUMMARY_COLUMNS = ("timepoint", "domain", "statistic", "n", "p_global", "padj", "pattern")
ARRAYS = ("counts", "value", "radii", "sizes", "window", "area", "p_global", "padj")
Window = collections.namedtuple("Window", "vertices cum area")      # what convex_window returns
NO_CPU = "spadot_amd counts Ripley's functions on the MI355X only ({}); there is no CPU path"


def _host_xy(coords):
    xy = coords.detach().cpu().numpy() if hasattr(coords, "is_cuda") else np.asarray(coords)
    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
        raise ValueError(f"coords must be an [n, 2] array of at least one spot (got {xy.shape})")
    if not np.all(np.isfinite(xy)):
        raise ValueError("the coordinates must be finite")
    return xy


def _turn(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _hull(xy):
    """Andrew's monotone chain: counter-clockwise from the lexicographically smallest point, collinear points dropped.  The chain
    tests (a - o) x (b - o); the device's check of a window tests (b - a) x (c - b) on every consecutive triple, and on vertices
    that are collinear up to rounding (a rotated lattice of spots) the two can disagree.  So the chain's result is finished under
    the check's own predicate: while a triple turns right there, its middle vertex goes (it lies within rounding of the line
    through its neighbours)."""
    pts = np.unique(xy, axis=0).tolist()                               # sorted by (x, y), duplicates dropped
    if len(pts) < 3:
        return pts
    chains = []
    for seq in (pts, pts[::-1]):
        chain = []
        for p in seq:
            while len(chain) >= 2 and _turn(chain[-2], chain[-1], p) <= 0:
                chain.pop()
            chain.append(p)
        chains.append(chain[:-1])
    v = chains[0] + chains[1]
    while len(v) > 2:
        a = np.array(v)
        e = np.roll(a, -1, axis=0) - a
        f = np.roll(e, -1, axis=0)
        right = np.flatnonzero(e[:, 0] * f[:, 1] < e[:, 1] * f[:, 0])
        if right.size == 0:
            break
        del v[(int(right[0]) + 1) % len(v)]                            # the middle of the first triple that turns right
    return v


def convex_window(coords, window="hull"):
    """The window of a problem: a Window (vertices fp64 [V, 2] counter-clockwise, cum fp64 [V - 2], area).  window: "hull" (the convex hull
    of coords), "box" (their bounding box) or a convex polygon [V, 2] with its vertices counter-clockwise (coords may then be
    None).  Spots that all lie on one line, or fewer than three of them, give a window without area: its ends, padded to three
    vertices by repeating the last.  ValueError for more than 256 vertices (window="box" has four)."""
    from .stage_ops import ripley_window
    if isinstance(window, str):
        if window not in ("hull", "box"):
            raise ValueError(f"window is 'hull', 'box' or a convex polygon (got {window!r})")
        xy = _host_xy(coords)
        if window == "box":
            (x0, y0), (x1, y1) = xy.min(axis=0), xy.max(axis=0)
            v = [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]
        else:
            v = _hull(xy)
            while len(v) < 3:
                v.append(v[-1])
        v = np.array(v, dtype=np.float64)
    else:
        v = np.array(window, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != 2 or v.shape[0] < 3:
            raise ValueError(f"a window polygon holds at least three vertices [V, 2] (got {v.shape})")
        e = np.roll(v, -1, axis=0) - v
        f = np.roll(e, -1, axis=0)
        if np.all(np.isfinite(v)) and not np.all(e[:, 0] * f[:, 1] > e[:, 1] * f[:, 0]):
            raise ValueError("the window must be convex with its vertices counter-clockwise and no three of them on a line")
    if v.shape[0] > MAX_VERTICES:
        raise ValueError(f"the window has {v.shape[0]} vertices: the device takes at most {MAX_VERTICES}; window=\"box\" has four")
    d = v[1:] - v[0]
    cum = np.cumsum(0.5 * np.maximum(d[:-1, 0] * d[1:, 1] - d[:-1, 1] * d[1:, 0], 0.0))     # a sliver that rounding turns over: 0
    x, y = v[:, 0], v[:, 1]
    area = 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
    v, cum = ripley_window(v, cum)
    return Window(v, cum, area)


def _per(value, P, name):
    """A setting given once for the call, or as a list with one value per problem."""
    if isinstance(value, list):
        if len(value) != P:
            raise ValueError(f"{name} holds {len(value)} values for {P} problems")
        return value
    return [value] * P


def _per_window(window, P):
    """The window setting per problem.  One value for the call: "hull", "box", a Window, or a polygon as an array or a sequence
    of (x, y) pairs.  A list (or tuple) of P such values, none of them a bare (x, y) pair: one per problem."""
    if isinstance(window, (str, Window, np.ndarray)) or not isinstance(window, (list, tuple)):
        return [window] * P
    if all(not isinstance(w, (str, Window)) and np.ndim(w) == 1 for w in window):
        return [window] * P                                              # a polygon as a sequence of (x, y) pairs
    return _per(list(window), P, "window")


def _mode_mask(modes):
    from .stage_ops import RIPLEY_MODES
    names = [m.strip() for m in modes.split(",")] if isinstance(modes, str) else list(modes)
    if not names or any(m not in RIPLEY_MODES for m in names):
        raise ValueError(f"modes are taken from L, G and F (got {modes!r})")
    return sum(RIPLEY_MODES[m] for m in set(names))


def ripley_counts(coords, labels, radii=None, radii_sq=None, n_sim=99, n_probes=1000, null="labels", modes=STATS, seed=0,
                  window="hull", n_clusters=None, out=None, problem_ids=None, windows_out=None):
    """coords[g]: the fp64 [n, 2] device tensor of problem g; labels[g]: its integer labeling (numpy or torch); radii[g] its radii,
    or radii_sq[g] their squares (exactly one of the two); n_sim, n_probes, null, modes and window: one value for the call or a
    list with one per problem (modes: a tuple or "L,G,F"; window: "hull", "box", a polygon [V, 2] as an array or a sequence of
    (x, y) pairs, or the Window that convex_window returned); n_clusters[g]: its K (default: its largest label + 1); problem_ids[g]: the number g under which problem g draws
    its simulations (default: its place in the call).  One call to the library; returns [g] -> int64 numpy [K, 1 + S, 3, B] (Lc,
    Gc, Fc along axis 2; a statistic outside `modes` is not counted and stays zero).  ValueError / RuntimeError before any launch; out: an int64 device tensor
    [P, K_max, 1 + S_max, 3, B_max] to write into; windows_out: a list that receives every problem's Window."""
    import torch
    from . import stage_ops as ops
    P = len(coords)
    r2 = thresholds("ripley_counts", P, radii, radii_sq, labelings=len(labels))
    S = [int(v) for v in _per(n_sim, P, "n_sim")]
    M = [int(v) for v in _per(n_probes, P, "n_probes")]
    nulls = _per(null, P, "null")
    masks = [_mode_mask(m) for m in _per(modes, P, "modes")]
    gids = list(range(P)) if problem_ids is None else [int(v) for v in problem_ids]
    if len(gids) != P or any(not 0 <= v <= ops.RIPLEY_MAX_G for v in gids):
        raise ValueError(f"problem_ids holds one number in 0 .. {ops.RIPLEY_MAX_G} per problem")
    for g in range(P):
        if not 1 <= S[g] <= MAX_SIMULATIONS:
            raise ValueError(f"problem {g} asks for {S[g]} simulations: the device takes 1 to {MAX_SIMULATIONS}")
        if not 1 <= M[g] <= MAX_PROBES:
            raise ValueError(f"problem {g} asks for {M[g]} probe points: the device takes 1 to {MAX_PROBES}")
        if nulls[g] not in NULLS:
            raise ValueError(f"null is 'labels' or 'csr' (problem {g}: {nulls[g]!r})")
    dev, xy, Ks, sizes = sorted_problems(coords, labels, n_clusters, NO_CPU)
    wins = []
    for g, w in enumerate(_per_window(window, P)):
        wins.append(w if isinstance(w, Window) else convex_window(coords[g], w))
    if windows_out is not None:
        windows_out.extend(wins)
    with torch.cuda.device(dev):
        desc = np.zeros((P, ops.RIPLEY_DESC), dtype=np.int64)
        first = 0
        for g in range(P):
            n = int(sizes[g].sum())
            desc[g, :9] = (first, n, Ks[g], r2[g].shape[0], S[g], M[g], NULLS.index(nulls[g]), masks[g], gids[g])
            desc[g, 13:13 + Ks[g]] = np.cumsum(sizes[g, :Ks[g]])
            first += n
        K_max, S_max, B_max = max(Ks), max(S), max(t.shape[0] for t in r2)
        res = ops.ripley_counts(xy, desc, r2, [w[:2] for w in wins], K_max, S_max, B_max, seed=seed, out=out).cpu().numpy()
    return [np.ascontiguousarray(res[g, :Ks[g], :1 + S[g], :, :r2[g].shape[0]]) for g in range(P)]


def ripley_points(window, seed=0, g=0, stream=0, count=1000, device="cuda:0"):
    """The generated points 0 .. count - 1 of (seed, problem g, stream) in a window (the Window that convex_window returned, or a polygon): an
    fp64 device tensor [count, 2] from the device function that the counting kernel uses.  Stream 0 is the probe set of problem
    g, stream 1 + c S + s simulation s of domain c under null="csr"."""
    from . import stage_ops as ops
    w = window if isinstance(window, Window) else convex_window(None, window)
    return ops.ripley_points(w.vertices, w.cum, seed, g, stream, count, device=device)


def ripley_stats(counts, sizes, area, n_probes, alpha=0.05, modes=STATS):
    """The host statistics of one problem from its integers (module docstring).  counts int64 [K, 1 + S, 3, B]; sizes [K]; area,
    n_probes: the window's area and M; modes: the statistics that were counted.  Returns a dict: value fp64 [3, K, 1 + S, B] (L,
    G, F of every pattern), observed, sim_mean, sim_min, sim_max, p_lo, p_hi fp64 [3, K, B], p_global, padj fp64 [3, K], pattern
    [K] of str.  A statistic outside `modes` was not counted (its integers are zero): it is NaN throughout, and without L the
    pattern is '' for every domain."""
    from .markers import bh_adjust
    N = np.asarray(counts)
    if N.ndim != 4 or N.shape[2] != 3 or N.shape[1] < 2:
        raise ValueError(f"counts must be a [K, 1 + S, 3, B] array with S >= 1 (got {N.shape})")
    N = N.astype(np.int64)
    K, P, _, B = N.shape
    nc = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if nc.shape[0] != K:
        raise ValueError(f"sizes holds {nc.shape[0]} domains and counts {K}")
    S, M, area = P - 1, int(n_probes), float(area)
    if M < 1:
        raise ValueError(f"n_probes is at least 1 (got {M})")
    mask = _mode_mask(modes)
    value = np.full((3, K, P, B), np.nan)
    defined = np.stack([nc >= 2, nc >= 2, nc >= 1]) & np.array([mask >> i & 1 for i in range(3)], dtype=bool)[:, None]
    pairs = (nc[defined[0]] * (nc[defined[0]] - 1)).astype(np.float64)
    value[0, defined[0]] = np.sqrt(area * N[defined[0], :, 0, :].astype(np.float64) / (np.pi * pairs)[:, None, None])
    value[1, defined[1]] = N[defined[1], :, 1, :] / nc[defined[1]].astype(np.float64)[:, None, None]
    value[2, defined[2]] = N[defined[2], :, 2, :] / float(M)
    obs, sim = value[:, :, 0], value[:, :, 1:]
    Ni = N.transpose(2, 0, 1, 3)                                         # [3, K, 1 + S, B]
    with np.errstate(invalid="ignore"):
        p_hi = np.where(defined[:, :, None], (1 + (Ni[:, :, 1:] >= Ni[:, :, :1]).sum(axis=2)) / (S + 1.0), np.nan)
        p_lo = np.where(defined[:, :, None], (1 + (Ni[:, :, 1:] <= Ni[:, :, :1]).sum(axis=2)) / (S + 1.0), np.nan)
    p_global = np.full((3, K), np.nan)
    p_global[0, defined[0]] = mad_p(value[0, defined[0]], axis=-2)        # L in fp64, G and F on the integers
    p_global[1, defined[1]] = mad_p(Ni[1, defined[1]], axis=-2)
    p_global[2, defined[2]] = mad_p(Ni[2, defined[2]], axis=-2)
    padj = np.full((3, K), np.nan)
    for i in range(3):
        padj[i, defined[i]] = bh_adjust(p_global[i, defined[i]])
    with np.errstate(invalid="ignore"):
        excess = np.sum(obs[0] - sim[0].mean(axis=1), axis=-1)
        pattern = np.where(padj[0] <= alpha, np.where(excess > 0, "clustered", "dispersed"), "random" if mask & 1 else "")
    out = dict(value=value, observed=obs, sim_mean=sim.mean(axis=2), sim_min=sim.min(axis=2), sim_max=sim.max(axis=2))
    out.update(p_lo=p_lo, p_hi=p_hi, p_global=p_global, padj=padj, pattern=pattern)
    return out


class RipleyResult:
    """One problem: counts int64 [K, 1 + S, 3, B], radii fp64 [B], sizes int64 [K], window fp64 [V, 2], area, n_probes, null, seed,
    modes, and the statistics of ripley_stats as attributes (value, observed, sim_mean, sim_min, sim_max, p_lo, p_hi, p_global, padj,
    pattern)."""

    def __init__(self, counts, radii, sizes, window, area, n_probes, null="labels", seed=0, alpha=0.05, modes=STATS):
        self.counts, self.radii, self.sizes, self.window, self.area = counts, radii, sizes, window, float(area)
        self.n_probes, self.null, self.seed, self.alpha = int(n_probes), null, int(seed), float(alpha)
        self.modes = tuple(m for i, m in enumerate(STATS) if _mode_mask(modes) >> i & 1)
        for name, v in ripley_stats(counts, sizes, area, n_probes, alpha, modes).items():
            setattr(self, name, v)


def ripley(coords, labels, radii=None, bins=50, n_sim=99, n_probes=1000, null="labels", modes=STATS, seed=0, window="hull",
           alpha=0.05, n_clusters=None, problem_ids=None):
    """Ripley's L, G and F of every domain of every problem (module docstring): coords[g] fp64 [n, 2] device tensors, labels[g]
    integers, radii[g] the radii of problem g (default: default_radii(coords[g], bins)).  One call to the library.  Returns
    [g] -> RipleyResult."""
    wins = []

    def count(r):
        return ripley_counts(coords, labels, radii=r, n_sim=n_sim, n_probes=n_probes, null=null, modes=modes, seed=seed,
                             window=window, n_clusters=n_clusters, problem_ids=problem_ids, windows_out=wins)
    res = counted(coords, labels, radii, bins, count, no_cpu=NO_CPU)
    P = len(coords)
    M, nulls, masks = _per(n_probes, P, "n_probes"), _per(null, P, "null"), _per(modes, P, "modes")
    return [RipleyResult(N, r, sizes, wins[g].vertices, wins[g].area, M[g], nulls[g], seed, alpha, masks[g])
            for g, (N, r, sizes) in enumerate(res)]


def ripley_table(r):
    """The rows of {prefix}ripley_{tp}.csv: one per (domain, statistic, radius), domain-major, then L, G, F, then radius."""
    import pandas as pd
    K, B = r.counts.shape[0], r.counts.shape[3]
    c, i, t = np.unravel_index(np.arange(K * 3 * B), (K, 3, B))
    cols = {"domain": c, "statistic": np.array(STATS)[i], "radius": r.radii[t]}
    for name in TABLE_COLUMNS[3:]:
        cols[name] = getattr(r, name)[i, c, t]
    return pd.DataFrame(cols, columns=list(TABLE_COLUMNS))


def ripley_summary(tps, results):
    """The rows of {prefix}ripley_summary.csv: one per (time point, domain, statistic)."""
    import pandas as pd
    rows = []
    for tp, r in zip(tps, results):
        for c in range(r.counts.shape[0]):
            for i, name in enumerate(STATS):
                rows.append((tp, c, name, int(r.sizes[c]), r.p_global[i, c], r.padj[i, c], str(r.pattern[c])))
    return pd.DataFrame(rows, columns=list(SUMMARY_COLUMNS))


def ripley_stage(args):
    """Reads args.domains (the domains.csv of analyze: row, timepoint, kmeans, pixel_x, pixel_y) and counts every time point in one
    call (time point number g in sorted order draws under problem number g).  Radii per time point: default_radii(.., bins), or
    args.radius * (1 .. bins) / bins.  Writes {prefix}ripley_{tp}.csv (TABLE_COLUMNS), {prefix}ripley_summary.csv
    (SUMMARY_COLUMNS), {prefix}ripley.npz ('{tp}_counts', '{tp}_value', '{tp}_radii', '{tp}_sizes', '{tp}_window', '{tp}_area',
    '{tp}_p_global', '{tp}_padj', plus timepoints, bins, n_sim, n_probes, seed, null, modes) and, with matplotlib,
    {prefix}{tp}_ripley.png.  Returns {'tables', 'summary', 'results' (per time point), 'timepoints', 'timings'}."""
    from .utils import _analyze_utils
    t_start = time.perf_counter()
    tab = read_domains_table(args, "ripley")
    bins, radius = int(getattr(args, "bins", 50)), getattr(args, "radius", None)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"the ripley stage takes 1 to {MAX_BINS} radii (got bins = {bins})")
    n_sim, n_probes = int(getattr(args, "n_sim", 99)), int(getattr(args, "n_probes", 1000))
    null, window = getattr(args, "null", "labels") or "labels", getattr(args, "window", "hull") or "hull"
    mask = _mode_mask(getattr(args, "mode", None) or STATS)
    modes = tuple(m for i, m in enumerate(STATS) if mask >> i & 1)
    alpha, seed = float(getattr(args, "alpha", 0.05)), int(getattr(args, "seed", 0))
    if window not in ("hull", "box"):
        raise ValueError(f"the ripley stage takes the window 'hull' or 'box' (got {window!r})")
    out_file = open_output(args, tab.beside)

    import torch
    dev = cuda_device(args, "counts Ripley's functions")
    tps, masks = tab.tps, tab.masks
    radii = [ladder(radius, bins) if radius is not None else default_radii(tab.coords[m], bins) for m in masks]
    t_read = time.perf_counter()
    res = ripley([torch.as_tensor(tab.coords[m], device=dev) for m in masks], [tab.labels[m] for m in masks], radii=radii,
                 n_sim=n_sim, n_probes=n_probes, null=null, modes=modes, seed=seed, window=window, alpha=alpha, n_clusters=tab.Ks)
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter()

    arrays = {"timepoints": np.asarray(tps), "bins": np.int64(bins), "n_sim": np.int64(n_sim), "n_probes": np.int64(n_probes),
              "seed": np.int64(seed), "null": np.asarray(null), "modes": np.asarray(",".join(modes))}
    tables, arrays = write_timepoints(out_file, "ripley", tps, res, lambda t, r: ripley_table(r), ARRAYS, arrays)
    summary = ripley_summary(tps, res)
    summary.to_csv(out_file("ripley_summary.csv"), index=False)
    savez_pinned(out_file("ripley.npz"), arrays)
    plot_timepoints(tps, res, lambda tp, r: _analyze_utils.plot_ripley(out_file(f"{tp}_ripley.png"), r.radii, r.observed,
                                                                      r.sim_mean, r.sim_min, r.sim_max, tp, r.pattern))
    t_end = time.perf_counter()
    print(f"ripley: {tab.n} spots of {len(tps)} time points, {bins} radii, {n_sim} simulations under null '{null}', written to "
          f"{args.output_dir}", file=sys.stderr)
    return {"tables": tables, "summary": summary, "results": dict(zip(tps, res)), "timepoints": tps,
            "timings": timings(t_start, t_read, t_dev, t_end)}
