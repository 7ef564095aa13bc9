"""Inputs of the ripley tests (CPU and GPU): the windows of the generator tests, the edge call, the domains that straddle the
256-wide tile, the integer lattice, the set whose thresholds are its own nearest-neighbour distances, the planted domains of
nhood_cases, and the restatement's integers of each, computed once per process.

A problem is a dict: xy, lab, r2, K, S, M, null (and g, the problem number it draws under, where a test fixes one)."""
import functools

import numpy as np

import cooccur_cases
import nhood_cases
import ripley_ref as ref

SEED = 7


def _readonly(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def windows():
    """{name: vertices}: a triangle, a square, a regular 37-gon and the hull of a jittered 20 x 20 grid."""
    rng = np.random.default_rng(3)
    ang = 2 * np.pi * np.arange(37) / 37
    grid = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0)), -1).reshape(-1, 2) + rng.uniform(-0.4, 0.4, (400, 2))
    return {"triangle": np.array([[0.0, 0.0], [7.0, 1.0], [2.0, 5.0]]),
            "square": np.array([[-1.0, -1.0], [3.0, -1.0], [3.0, 3.0], [-1.0, 3.0]]),
            "gon37": np.stack([10 + 6 * np.cos(ang), -4 + 6 * np.sin(ang)], axis=1),
            "jittered": ref.hull(grid)}


def problem(xy, lab, r2, K, S, M, null, g=0):
    return dict(xy=np.asarray(xy, dtype=np.float64), lab=np.asarray(lab, dtype=np.int64), r2=np.asarray(r2, dtype=np.float64),
                K=int(K), S=int(S), M=int(M), null=null, g=int(g))


@functools.lru_cache(maxsize=None)
def edge_call():
    """Four problems over the sets of cooccur_cases.edge_call(), drawing under g = 0 .. 3: n = 1 (B = 1, S = 1, M = 1); two
    coincident spots of one domain with a threshold 0 (B = 16, S = 19, M = 257, csr); n = 37 with K = 3 and the label value 1
    without spots (B = 17, S = 19, M = 1, labels); n = 300 with K = 32 (B = 64, S = 1, M = 257, csr)."""
    c = cooccur_cases.edge_call()
    return [problem(c[0][0], c[0][1], c[0][2], 1, 1, 1, "labels", 0),
            problem(c[1][0], [0, 0], c[1][2], 1, 19, 257, "csr", 1),
            problem(c[2][0], c[2][1], c[2][2], 3, 19, 1, "labels", 2),
            problem(c[3][0], c[3][1], c[3][2], 32, 1, 257, "csr", 3)]


TILE_SIZES = (255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def tile_case(m, null="labels"):
    """A problem whose domain 1 has exactly m spots (domains 0 and 2: 40 and 23), B = 7, S = 2, M = 100."""
    rng = np.random.default_rng(2000 + m)
    lab = rng.permutation(np.repeat([0, 1, 2], [40, m, 23]))
    r2 = np.sort(rng.uniform(0.0, 6.0, 7)) ** 2
    return problem(rng.uniform(0, 25, (m + 63, 2)), lab, r2, 3, 2, 100, null)


@functools.lru_cache(maxsize=None)
def lattice(null="labels"):
    """The 12 x 12 integer lattice of cooccur_cases with K = 3: every squared distance between spots is an integer, every pair
    and every nearest neighbour exactly on or off a threshold.  S = 3, M = 64."""
    xy, lab, r2, K = cooccur_cases.lattice()
    return problem(xy, lab, r2, K, 3, 64, null)


@functools.lru_cache(maxsize=None)
def on_threshold():
    """(problem, pairs): the jittered grid of cooccur_cases.on_threshold() with K = 4 and 64 thresholds taken from the set's own
    unfused squared nearest-neighbour distances inside the domains, at evenly spaced ranks of the distinct values.  pairs[t] =
    (i, j): spot i and its nearest spot j of the same domain lie exactly on threshold t.  S = 1, M = 16, labels."""
    xy, lab, _, K, _ = cooccur_cases.on_threshold()
    d2 = ref.d2_cross(xy, xy)
    d2[lab[:, None] != lab[None, :]] = np.inf
    d2[np.arange(289), np.arange(289)] = np.inf
    near, who = d2.min(axis=1), d2.argmin(axis=1)
    vals, first = np.unique(near, return_index=True)
    ranks = np.round(np.linspace(0.0, 1.0, 64) * (vals.shape[0] - 1)).astype(np.int64)
    assert np.all(np.diff(ranks) > 0) and np.all(np.isfinite(vals))
    pairs = [(int(first[r]), int(who[first[r]])) for r in ranks]
    return problem(xy, lab, vals[ranks], K, 1, 16, "labels"), pairs


PLANTED_S, PLANTED_M, PLANTED_BINS = 39, 200, 20


@functools.lru_cache(maxsize=None)
def planted(null="labels", scattered=False):
    """The 45 x 45 planted set of nhood_cases (7 Voronoi domains) under the stage's radii (20 of them), S = 39, M = 200; scattered:
    300 spots drawn at random receive the new label 7, a domain that is a random sample of the spots."""
    xy, lab, _, _, K = nhood_cases.planted(45)
    if scattered:
        lab = lab.copy()
        lab[np.random.default_rng(17).choice(lab.shape[0], 300, replace=False)] = K
        K += 1
    return problem(xy, lab, cooccur_cases.ref.default_radii(xy, PLANTED_BINS) ** 2, K, PLANTED_S, PLANTED_M, null)


def counts_of(p, seed=SEED, **kw):
    return ref.counts(p["xy"], p["lab"], p["r2"], p["K"], p["S"], p["M"], p["null"], seed, p["g"], **kw)


@functools.lru_cache(maxsize=None)
def want(name):
    """The restatement's integers [K, 1 + S, 3, B] of a named case under SEED, computed once: 'edge<i>', 'tile<m>_<null>',
    'lattice_<null>', 'on_threshold', 'planted_<null>', 'scattered'."""
    if name.startswith("edge"):
        p = edge_call()[int(name[4:])]
    elif name.startswith("tile"):
        m, null = name[4:].split("_")
        p = tile_case(int(m), null)
    elif name.startswith("lattice_"):
        p = lattice(name[8:])
    elif name == "on_threshold":
        p = on_threshold()[0]
    elif name.startswith("planted_"):
        p = planted(name[8:])
    elif name == "scattered":
        p = planted("labels", True)
    else:
        raise KeyError(name)
    return _readonly(counts_of(p))


def stats_of(p, N, alpha=0.05):
    """The restatement's statistics of a problem from integers N."""
    _, area = ref.fan(ref.hull(p["xy"]))
    return ref.stats(N, np.bincount(p["lab"], minlength=p["K"]), area, p["M"], alpha)


STAGE = dict(bins=50, n_sim=99, n_probes=1000, seed=0)


@functools.lru_cache(maxsize=None)
def stage_want():
    """{tp: (counts, radii, K, sizes, vertices, area)} of nhood_cases.stage_table() under the stage's defaults (null labels, the
    hull, time point number g in sorted order)."""
    df = nhood_cases.stage_table()
    out = {}
    for g, tp in enumerate(sorted(set(df["timepoint"]))):
        m = np.asarray(df["timepoint"]) == tp
        xy = np.stack([df["pixel_x"][m], df["pixel_y"][m]], axis=1)
        lab = np.asarray(df["kmeans"])[m]
        K = int(lab.max()) + 1
        radii = cooccur_cases.ref.default_radii(xy, STAGE["bins"])
        v = ref.hull(xy)
        N = ref.counts(xy, lab, radii * radii, K, STAGE["n_sim"], STAGE["n_probes"], "labels", STAGE["seed"], g)
        out[tp] = (_readonly(N), radii, K, np.bincount(lab, minlength=K), v, ref.fan(v)[1])
    return out
