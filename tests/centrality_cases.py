"""Inputs of the centrality tests (CPU and GPU), all seeded and small, with the restatement's answers computed once per
process: the tiny graphs, K = 1 and K = 32, duplicates, a self loop, components and isolated spots, the star, the 1000-spot
path in three edge orders (the shuffled one is what an update in place gets wrong), the lattice with its closed form, the sizes
around the widths of the 1024-thread workgroup (which loads four classes a thread: 4096 a pass), the 32-source block edges of
the source items and the planted stripe maps of the territories tests."""
import functools

import numpy as np

import hops_ref as ref
from nhood_cases import random_edges
from territories_cases import WIDTH_SIZES, _lattice, jittered_grid, knn_edges, stage_table, stripes  # noqa: F401

SEED = 321
SOURCE_SIZES = (31, 32, 33, 65, 300, 2025)


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: (src, dst, labelings int64 [L, n], K)}."""
    rng = np.random.default_rng(29)
    none = np.zeros(0, np.int32)
    out = {"n1": (none, none, np.zeros((1, 1), np.int64), 1),
           "n2": (np.array([0], np.int32), np.array([1], np.int32), np.array([[0, 0], [0, 1], [1, 0]], np.int64), 2)}
    src, dst = random_edges(rng, 50, 60)
    out["K1"] = (src, dst, np.zeros((1, 50), np.int64), 1)
    src, dst = random_edges(rng, 300, 900)
    out["K32_unused"] = (src, dst, np.asarray([0, 5, 31])[rng.integers(0, 3, (2, 300))].astype(np.int64), 32)
    src, dst = random_edges(rng, 200, 260)
    out["K32_all"] = (src, dst, np.stack([rng.permutation(np.arange(200) % 32), np.arange(200) % 32]).astype(np.int64), 32)
    src, dst = random_edges(rng, 37, 40)
    src, dst = np.concatenate([src, src[:9], dst[5:20]]), np.concatenate([dst, dst[:9], src[5:20]])   # duplicates and two-way edges
    out["dup_twoway"] = (src.astype(np.int32), dst.astype(np.int32), rng.integers(0, 3, (3, 37)).astype(np.int64), 3)
    out["self_loop"] = (np.array([0, 1, 1, 2, 3], np.int32), np.array([1, 1, 2, 3, 3], np.int32),
                        np.array([[0, 0, 1, 1], [0, 1, 2, 2]], np.int64), 3)
    # two components (a path of 5 and a triangle) and two isolated spots
    out["components"] = (np.array([0, 1, 2, 3, 5, 6, 7], np.int32), np.array([1, 2, 3, 4, 6, 7, 5], np.int32),
                         np.array([[0, 0, 1, 1, 1, 2, 2, 0, 1, 2], [0, 1, 1, 1, 1, 1, 1, 1, 1, 1]], np.int64), 3)
    star = np.ones((1, 300), np.int64)
    star[0, 299] = 0
    out["star_hub_last"] = (np.arange(299, dtype=np.int32), np.full(299, 299, np.int32), star, 2)
    a = np.arange(999, dtype=np.int32)
    one = np.ones((1, 1000), np.int64)
    one[0, 0] = 0                                                     # the set {spot 0}: distances 1 .. 999 along the path
    out["path_ascending"] = (a, a + 1, one, 2)
    out["path_descending"] = ((a + 1)[::-1].copy(), a[::-1].copy(), one, 2)
    order = rng.permutation(999)
    out["path_shuffled"] = (a[order], (a + 1)[order], one, 2)
    src, dst = _lattice(20)
    out["lattice_stripes"] = (src, dst, (np.arange(400) % 20 // 4)[None].astype(np.int64), 5)       # columns 0-3, 4-7, ..
    for n in WIDTH_SIZES:
        r = np.random.default_rng(n)
        src, dst = random_edges(r, n, 2 * n + (n % 3) - 1)
        out[f"width_n{n}"] = (src, dst, r.integers(0, 5, (1, n)).astype(np.int64), 5)
    for side in (20, 45):
        _, plant, lab, src, dst, K = stripes(side)
        out[f"stripes{side}"] = (src, dst, np.stack([lab, plant]), K)
    return out


NAMES = ("n1", "n2", "K1", "K32_unused", "K32_all", "dup_twoway", "self_loop", "components", "star_hub_last", "path_ascending",
         "path_descending", "path_shuffled", "lattice_stripes") + tuple(f"width_n{n}" for n in WIDTH_SIZES) + ("stripes20", "stripes45")
SMALL = ("n1", "n2", "K1", "dup_twoway", "self_loop", "components", "star_hub_last", "lattice_stripes")


@functools.lru_cache(maxsize=None)
def want(name):
    """The restatement's answer of a case: (sums int64 [L, K, K, 3], ecc int64 [L, K], hops int64 [n, K] of the first
    labeling)."""
    src, dst, labs, K = all_cases()[name]
    D = ref.dist_matrix(src, dst, labs.shape[1])
    got = [ref.integers(D, lab, K) for lab in labs]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), got[0][2]


@functools.lru_cache(maxsize=None)
def source_cases():
    """{n: (src, dst, labels int64 [n], K)} of the source items: n around the 32-source blocks."""
    out = {}
    for n in SOURCE_SIZES:
        if n == 2025:
            _, _, lab, src, dst, K = stripes(45)
        else:
            r = np.random.default_rng(1000 + n)
            src, dst = random_edges(r, n, (3 * n) // 2)                # sparse: several components and isolated spots
            lab, K = r.integers(0, 4, n).astype(np.int64), 4
        out[n] = (src, dst, lab, K)
    return out


@functools.lru_cache(maxsize=None)
def source_want(n):
    """(reached_by, sumdist_by, degree, ecc) of source case n and its all-pairs distance matrix."""
    src, dst, lab, K = source_cases()[n]
    D = ref.dist_matrix(src, dst, n)
    return ref.spot_integers(D, lab, K) + (D,)


@functools.lru_cache(maxsize=None)
def perm_problems():
    """The permuted problems: the 45 x 45 stripe map (graph 0), n = 37 (graph 1) and n = 300 (graph 2), P = 200 under SEED:
    [(src, dst, base labels, K, the restatement's sums [200, K, K, 3], its eccentricities [200, K])]."""
    c = all_cases()
    graphs = [(c["stripes45"][0], c["stripes45"][1], c["stripes45"][2][0], 7),
              (c["dup_twoway"][0], c["dup_twoway"][1], c["dup_twoway"][2][0], 3),
              (c["K32_unused"][0], c["K32_unused"][1], c["K32_unused"][2][0], 32)]
    out = []
    for g, (s, d, lab, K) in enumerate(graphs):
        D = ref.dist_matrix(s, d, lab.shape[0])
        out.append((s, d, lab, K) + ref.perm_integers(D, lab, K, 200, SEED, g))
    return out
