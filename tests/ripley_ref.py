"""The definition of the ripley stage, restated in numpy after squidpy's gr.ripley: what csrc/ripley.hip and
spadot_amd.ripley are held to.  It forms every simulated pattern and every distance matrix, which the device never does.

A problem: n spots, labels in 0 .. K-1, B squared thresholds r2, S simulations, M probe points, a seed, a problem number g and a
convex window W (the hull of the spots by a monotone chain, counter-clockwise, collinear points dropped).  Domain c of n_c spots
has 1 + S patterns of n_c points: pattern 0 its spots; pattern s under null "labels" the spots that receive label c when the
Feistel permutation (seed, g, s - 1) of nhood_ref relabels the spots stored by (label, index), under null "csr" n_c generated
points of stream 1 + c S + s - 1.  Stream 0 is the probe set.  Per pattern and threshold:
    Lc = #{ordered pairs i != j : d2 <= r2}     Gc = #{points whose nearest other point has d2 <= r2}
    Fc = #{probes whose nearest point of the pattern has d2 <= r2}        d2 = dx * dx + dy * dy, unfused, as cooccur_ref
    L = sqrt(A Lc / (pi n_c (n_c - 1)))    G = Gc / n_c    F = Fc / M        (NaN: L, G where n_c < 2; F where n_c < 1)

Where this departs from squidpy's gr.ripley:
  * no edge correction and no distance-transform shortcuts: the observed and the simulated patterns share W, so the bias is the
    same on both sides of every comparison; L is sqrt(K / pi) with the plain estimator K = A Lc / (n_c (n_c - 1));
  * the window is the convex hull (or a given convex polygon, or the bounding box), not always the bounding box;
  * the default null permutes the labels over the spots (the right null on a lattice of spots); squidpy's null, points uniform in
    W, is null "csr"; every simulated pattern has exactly n_c points (squidpy draws n_simulations x n_observations fixed sizes);
  * the random numbers are counter-based (splitmix64), a pure function of (seed, g, stream, index), not numpy's generator;
  * besides the pointwise envelope and p-values there is a global envelope (maximum absolute deviation) test per domain, with
    Benjamini-Hochberg over the domains of a time point; squidpy reports one pointwise p-value per radius."""
import functools
import math

import numpy as np

import nhood_ref

GOLD = 0x9E3779B97F4A7C15
SALT = 0x52504C5953494D31
MASK = (1 << 64) - 1
STATS = ("L", "G", "F")


def stream_key(seed, g, stream):
    """The key of (seed, g, stream): one splitmix draw of seed ^ (g << 32) ^ stream, salted.  A Python int below 2^64."""
    s = (int(seed) & MASK) ^ ((int(g) << 32) & MASK) ^ (int(stream) & MASK)
    return int(nhood_ref.splitmix64(np.uint64(s))[1]) ^ SALT


def words(key, counters):
    """The splitmix64 outputs at the given counters (uint64 array): output of state key + counter * GOLD."""
    with np.errstate(over="ignore"):
        state = np.uint64(key) + np.asarray(counters, dtype=np.uint64) * np.uint64(GOLD)
    return nhood_ref.splitmix64(state)[1]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _right_turn(a, b, c):
    """The predicate of the device's window check on the triple (a, b, c): (b - a) x (c - b) < 0, as two products compared."""
    ux, uy, vx, vy = b[0] - a[0], b[1] - a[1], c[0] - b[0], c[1] - b[1]
    return ux * vy < uy * vx


def hull(xy):
    """The convex hull by Andrew's monotone chain in fp64: vertices counter-clockwise from the lexicographically smallest point,
    collinear points dropped; then, while a consecutive triple (cyclically, the first such in vertex order) turns right under the
    window check's own predicate -- the chain tests another form of the cross product, and the two can disagree on vertices that
    are collinear up to rounding -- the middle vertex of that triple is dropped.  Fewer than three distinct or only collinear
    points give their two ends (or the one point), padded to three vertices by repeating the last (a window without area)."""
    pts = sorted(set(map(tuple, np.asarray(xy, dtype=np.float64).tolist())))
    if len(pts) > 2:
        lower, upper = [], []
        for p in pts:
            while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
                lower.pop()
            lower.append(p)
        for p in reversed(pts):
            while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
                upper.pop()
            upper.append(p)
        pts = lower[:-1] + upper[:-1]
        again = True
        while again and len(pts) > 2:
            again = False
            for i in range(len(pts)):
                if _right_turn(pts[i], pts[(i + 1) % len(pts)], pts[(i + 2) % len(pts)]):
                    del pts[(i + 1) % len(pts)]
                    again = True
                    break
    while len(pts) < 3:
        pts.append(pts[-1])
    return np.array(pts, dtype=np.float64)


def box(xy):
    xy = np.asarray(xy, dtype=np.float64)
    (x0, y0), (x1, y1) = xy.min(axis=0), xy.max(axis=0)
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])


def fan(vertices):
    """(cum fp64 [V - 2], area): the cumulative areas of the triangles (V0, V_{k+1}, V_{k+2}), and the shoelace area."""
    v = np.asarray(vertices, dtype=np.float64)
    cum, run = [], 0.0
    for k in range(v.shape[0] - 2):
        run = run + 0.5 * max(_cross(v[0], v[k + 1], v[k + 2]), 0.0)       # a sliver that rounding turns over counts 0
        cum.append(run)
    x, y = v[:, 0], v[:, 1]
    area = 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
    return np.array(cum), area


def points(vertices, cum, seed, g, stream, count):
    """The generated points 0 .. count - 1 of a stream, fp64 [count, 2]: every operation rounded once."""
    v, cum = np.asarray(vertices, dtype=np.float64), np.asarray(cum, dtype=np.float64)
    key = stream_key(seed, g, stream)
    i = np.arange(count, dtype=np.uint64) * np.uint64(3)
    u = [(words(key, i + np.uint64(j)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 for j in range(3)]
    w = u[0] * cum[-1]
    k = np.minimum(np.searchsorted(cum, w, side="right"), cum.shape[0] - 1)        # the first k with w < cum[k]
    flip = u[1] + u[2] > 1.0
    u1, u2 = np.where(flip, 1.0 - u[1], u[1]), np.where(flip, 1.0 - u[2], u[2])
    A, Bv, C = v[0], v[k + 1], v[k + 2]
    return np.stack([(A[0] + u1 * (Bv[:, 0] - A[0])) + u2 * (C[:, 0] - A[0]),
                     (A[1] + u1 * (Bv[:, 1] - A[1])) + u2 * (C[:, 1] - A[1])], axis=1)


def by_label(xy, lab, K):
    """The spots stored by (label, index) and the cluster offsets [K + 1]."""
    lab = np.asarray(lab, dtype=np.int64)
    order = np.argsort(lab, kind="stable")
    return np.asarray(xy, dtype=np.float64)[order], np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=K))])


def window_of(xy, window="hull"):
    if isinstance(window, str):
        return hull(xy) if window == "hull" else box(xy)
    return np.asarray(window, dtype=np.float64)


@functools.lru_cache(maxsize=4)
def _inverse(n, seed, g, p):
    """pi^-1 of nhood_ref.perm: position j receives the label of position pi(j), so label c goes to pi^-1 of its positions."""
    pi = nhood_ref.perm(n, seed, g, p)
    inv = np.empty_like(pi)
    inv[pi] = np.arange(n)
    return inv


def pattern(xs, off, c, p, S, null, seed, g, vertices, cum):
    """Pattern p of domain c: fp64 [n_c, 2]."""
    lo, hi = int(off[c]), int(off[c + 1])
    if p == 0:
        return xs[lo:hi]
    if null == "labels":
        return xs[_inverse(xs.shape[0], seed, g, p - 1)[lo:hi]]
    return points(vertices, cum, seed, g, 1 + c * S + p - 1, hi - lo)


def d2_cross(a, b):
    dx = a[:, 0][:, None] - b[:, 0][None, :]
    dy = a[:, 1][:, None] - b[:, 1][None, :]
    return dx * dx + dy * dy


def pattern_counts(pts, probes, r2):
    """int64 [3, B]: Lc, Gc, Fc of one pattern."""
    r2 = np.asarray(r2, dtype=np.float64)
    out = np.zeros((3, r2.shape[0]), dtype=np.int64)
    m = pts.shape[0]
    if m == 0:
        return out
    d2 = d2_cross(pts, pts)
    d2[np.arange(m), np.arange(m)] = np.inf                          # a point is never its own neighbour
    near = d2.min(axis=1)                                            # inf for a lone point
    far = d2_cross(probes, pts).min(axis=1)
    for i, v in enumerate((d2.reshape(-1), near, far)):              # #{v <= r} for every r at once
        out[i] = np.searchsorted(np.sort(v), r2, side="right")
    return out


def counts(xy, lab, r2, K, S, M, null="labels", seed=0, g=0, window="hull", modes=("L", "G", "F")):
    """int64 [K, 1 + S, 3, B] of one problem; a statistic outside `modes` stays zero."""
    xs, off = by_label(xy, lab, K)
    v = window_of(xy, window)
    cum, _ = fan(v)
    probes = points(v, cum, seed, g, 0, M)
    out = np.zeros((K, 1 + S, 3, np.asarray(r2).shape[0]), dtype=np.int64)
    for p in range(1 + S):
        for c in range(K):
            out[c, p] = pattern_counts(pattern(xs, off, c, p, S, null, seed, g, v, cum), probes, r2)
    for i, name in enumerate(STATS):
        if name not in modes:
            out[:, :, i] = 0
    return out


def curves(N, sizes, area, M):
    """fp64 [3, K, 1 + S, B]: L, G, F from the integers."""
    N = np.asarray(N, dtype=np.int64)
    K, P, _, B = N.shape
    out = np.full((3, K, P, B), np.nan)
    for c in range(K):
        nc = int(sizes[c])
        for p in range(P):
            for t in range(B):
                if nc >= 2:
                    out[0, c, p, t] = math.sqrt(area * float(N[c, p, 0, t]) / (math.pi * nc * (nc - 1)))
                    out[1, c, p, t] = float(N[c, p, 1, t]) / nc
                if nc >= 1:
                    out[2, c, p, t] = float(N[c, p, 2, t]) / M
    return out


def mad_p(x, exact=None):
    """The global envelope test of curves x [1 + S, B]: u_i = max_t |x_i - mean_{k != i} x_k| = max_t |(S + 1) x_i - sum_k x_k| / S,
    p = #{i : u_i >= u_0} / (S + 1).  exact: the integer counts behind x (G and F are their counts over a constant), compared
    exactly; L in fp64."""
    if exact is not None:
        rows = [[int(v) for v in r] for r in np.asarray(exact)]
        tot = [sum(col) for col in zip(*rows)]
        u = [max(abs(len(rows) * v - s) for v, s in zip(r, tot)) for r in rows]
    else:
        x = np.asarray(x, dtype=np.float64)
        tot = x.sum(axis=0)
        u = [float(np.max(np.abs(x.shape[0] * r - tot))) for r in x]
    return sum(1 for v in u if v >= u[0]) / len(u)


def stats(N, sizes, area, M, alpha=0.05, modes=STATS):
    """The host statistics of one problem from its integers: a dict of
    value [3, K, 1 + S, B]; observed, sim_mean, sim_min, sim_max, p_lo, p_hi [3, K, B]; p_global, padj [3, K]; pattern [K].
    A statistic outside `modes` was not counted: NaN throughout, and without L the pattern of every domain is ''."""
    N = np.asarray(N, dtype=np.int64)
    K, P, _, B = N.shape
    S = P - 1
    x = curves(N, sizes, area, M)
    for i, name in enumerate(STATS):
        if name not in modes:
            x[i] = np.nan
    obs, sim = x[:, :, 0], x[:, :, 1:]
    out = dict(value=x, observed=obs, sim_mean=sim.mean(axis=2), sim_min=sim.min(axis=2), sim_max=sim.max(axis=2))
    p_lo, p_hi = np.full((3, K, B), np.nan), np.full((3, K, B), np.nan)
    p_global, padj = np.full((3, K), np.nan), np.full((3, K), np.nan)
    for i in range(3):
        for c in range(K):
            if np.isnan(obs[i, c, 0]):
                continue
            for t in range(B):
                p_hi[i, c, t] = (1 + int((N[c, 1:, i, t] >= N[c, 0, i, t]).sum())) / (S + 1)
                p_lo[i, c, t] = (1 + int((N[c, 1:, i, t] <= N[c, 0, i, t]).sum())) / (S + 1)
            p_global[i, c] = mad_p(x[i, c], exact=None if i == 0 else N[c, :, i, :])
        ok = ~np.isnan(p_global[i])
        if ok.any():
            padj[i, ok] = nhood_ref.bh(p_global[i, ok])
    pattern = []
    for c in range(K):
        if not padj[0, c] <= alpha:
            pattern.append("random" if "L" in modes else "")
        else:
            excess = float(np.sum(obs[0, c] - sim[0, c].mean(axis=0)))
            pattern.append("clustered" if excess > 0 else "dispersed")
    out.update(p_lo=p_lo, p_hi=p_hi, p_global=p_global, padj=padj, pattern=np.array(pattern))
    return out
