"""Inputs of the neighbourhood-enrichment tests (CPU and GPU): planted Voronoi domains on jittered grids with their k-nearest-
neighbour graphs, the edge call, the graphs that straddle the 256-thread workgroup, and the restatement's permuted count stacks,
computed once per process."""
import functools

import numpy as np

import nhood_ref as ref

SEED = 123
PLANTED = {20: 4, 45: 7}                      # grid side -> planted domains


def knn_edges(xy, k):
    """Directed k-nearest-neighbour edges by brute force in fp64, neighbours ordered by (distance, index), self dropped."""
    xy = np.asarray(xy, dtype=np.float64)
    n = xy.shape[0]
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    d2[np.arange(n), np.arange(n)] = -1.0                          # the spot itself sorts first
    idx = np.argsort(d2, axis=1, kind="stable")[:, 1:min(k, n - 1) + 1]
    return np.repeat(np.arange(n), idx.shape[1]).astype(np.int32), idx.reshape(-1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _planted_all():
    rng = np.random.default_rng(0)
    out = {}
    for side, K in PLANTED.items():
        xy = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2) + rng.uniform(-.3, .3, (side * side, 2))
        cen = rng.uniform(0, side, (K, 2))
        lab = np.argmin(((xy[:, None] - cen[None]) ** 2).sum(-1), 1).astype(np.int64)
        src, dst = knn_edges(xy, 6)
        out[side] = (xy, lab, src, dst, K)
    return out


def planted(side):
    """(xy [n, 2], labels int64 [n], src, dst int32 [6 n], K) of the side x side jittered grid with K Voronoi domains, k = 6."""
    return _planted_all()[side]


@functools.lru_cache(maxsize=None)
def planted_perm_counts(side, n_perms=1000):
    """The restatement's [n_perms, K, K] stack of the planted set under (SEED, graph 0)."""
    _, lab, src, dst, K = planted(side)
    return ref.perm_counts(src, dst, lab, K, n_perms, SEED, 0)


def random_edges(rng, n, E):
    """E random directed edges over n >= 2 nodes without self loops (duplicates may occur)."""
    src = rng.integers(0, n, E)
    dst = (src + rng.integers(1, n, E)) % n
    return src.astype(np.int32), dst.astype(np.int32)


@functools.lru_cache(maxsize=None)
def edge_call():
    """Four graphs with three labelings each: [(src, dst, labelings int64 [3, n], K)].  n = 1 without edges; n = 2; n = 37 with
    K = 3, a duplicate edge and one labeling in which the value 2 has no spots; n = 300 with K = 32."""
    rng = np.random.default_rng(11)
    out = [(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((3, 1), np.int64), 1),
           (np.array([0, 1], np.int32), np.array([1, 0], np.int32), np.array([[0, 1], [1, 0], [0, 0]], np.int64), 2)]
    src, dst = random_edges(rng, 37, 37 * 4)
    src, dst = np.append(src, src[5]), np.append(dst, dst[5])                  # the duplicate edge: counted twice
    labs = np.stack([rng.integers(0, 3, 37), rng.integers(0, 2, 37), rng.integers(0, 3, 37)])
    assert 2 not in labs[1] and set(labs[0]) == {0, 1, 2}
    out.append((src, dst, labs.astype(np.int64), 3))
    src, dst = random_edges(rng, 300, 300 * 6)
    labs = np.stack([rng.integers(0, 32, 300), rng.permutation(300) % 32, np.full(300, 31)])
    out.append((src, dst, labs.astype(np.int64), 32))
    return out


TILE_CASES = [(f"n{n}_E{E}", n, E) for n in (255, 256, 257) for E in (255 * 6, 256 * 6 + 1)] + [("n257_E0", 257, 0)]


def tile_case(name):
    """(src, dst, labels int64 [n], K = 5) of a graph whose n and E straddle the 256-thread workgroup."""
    _, n, E = next(c for c in TILE_CASES if c[0] == name)
    rng = np.random.default_rng(n * 100003 + E)
    src, dst = random_edges(rng, n, E)
    return src, dst, rng.integers(0, 5, n).astype(np.int64), 5


def planted_points(rng, n, K):
    """n uniform points in a square with K Voronoi domains: (xy, labels)."""
    side = np.sqrt(n)
    xy = rng.uniform(0, side, (n, 2))
    cen = rng.uniform(0, side, (K, 2))
    return xy, np.argmin(((xy[:, None] - cen[None]) ** 2).sum(-1), 1).astype(np.int64)


def stage_table():
    """A domains.csv of three planted time points (400, 500 and 600 spots; 4, 5 and 6 domains), the time points interleaved
    so that the table's order is not the time points' order."""
    import pandas as pd
    rng = np.random.default_rng(5)
    parts = []
    for tp, n, K in (("E10", 400, 4), ("E12", 500, 5), ("E14", 600, 6)):
        xy, lab = planted_points(rng, n, K)
        parts.append(pd.DataFrame({"timepoint": tp, "kmeans": lab, "pixel_x": xy[:, 0], "pixel_y": xy[:, 1]}))
    df = pd.concat(parts, ignore_index=True)
    df = df.iloc[rng.permutation(len(df))].reset_index(drop=True)
    df.insert(0, "row", np.arange(len(df)))
    return df
