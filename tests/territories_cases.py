"""Inputs of the territories tests (CPU and GPU), all seeded and small, with the restatement's answers computed once per
process: the tiny graphs, the paths, the star, the checkerboard, the one-label grid, the sizes around the widths of the
1024-thread workgroup (which loads four labels a thread: 4096 a pass) and the planted stripe maps."""
import functools

import numpy as np
from scipy.spatial import cKDTree

import territories_ref as ref
from nhood_cases import random_edges

SEED = 123
STRIPES = {20: (3, 0.05), 45: (7, 0.03)}          # grid side -> (stripes, share of the labels flipped)
STRIPE_SEED = {20: 1, 45: 0}                      # chosen so that the planted properties of test_territories_cpu.py hold
WIDTH_SIZES = (255, 256, 257, 1023, 1024, 1025, 4095, 4097)


def knn_edges(xy, k):
    """Directed k-nearest-neighbour edges (a kd-tree; the spot itself dropped), int32."""
    n = xy.shape[0]
    idx = cKDTree(xy).query(xy, k=min(k, n - 1) + 1)[1][:, 1:]
    return np.repeat(np.arange(n), idx.shape[1]).astype(np.int32), idx.reshape(-1).astype(np.int32)


def jittered_grid(side, rng):
    return np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2) + rng.uniform(-.3, .3, (side * side, 2))


@functools.lru_cache(maxsize=None)
def stripes(side):
    """(xy, planted labels, labels with a share flipped to another value, src, dst, K) of the side x side jittered grid cut
    into K vertical stripes, k = 6."""
    K, share = STRIPES[side]
    rng = np.random.default_rng(STRIPE_SEED[side])
    xy = jittered_grid(side, rng)
    plant = np.minimum((np.arange(side * side) % side) * K // side, K - 1).astype(np.int64)
    lab = plant.copy()
    flip = rng.choice(side * side, int(round(share * side * side)), replace=False)
    lab[flip] = (plant[flip] + rng.integers(1, K, flip.shape[0])) % K
    src, dst = knn_edges(xy, 6)
    return xy, plant, lab, src, dst, K


def _lattice(side):
    """The 4-neighbour lattice, every edge once."""
    i = np.arange(side * side).reshape(side, side)
    src = np.concatenate([i[:, :-1].reshape(-1), i[:-1, :].reshape(-1)])
    dst = np.concatenate([i[:, 1:].reshape(-1), i[1:, :].reshape(-1)])
    return src.astype(np.int32), dst.astype(np.int32)


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: (src, dst, labelings int64 [L, n], K)}."""
    rng = np.random.default_rng(17)
    none = np.zeros(0, np.int32)
    out = {"n1": (none, none, np.zeros((1, 1), np.int64), 1),
           "n2": (np.array([0], np.int32), np.array([1], np.int32), np.array([[0, 0], [0, 1], [1, 1]], np.int64), 2)}
    src, dst = random_edges(rng, 50, 60)
    out["K1"] = (src, dst, np.zeros((1, 50), np.int64), 1)
    src, dst = random_edges(rng, 300, 900)
    out["K32_unused"] = (src, dst, np.asarray([0, 5, 31])[rng.integers(0, 3, (2, 300))].astype(np.int64), 32)
    src, dst = random_edges(rng, 37, 40)
    src, dst = np.concatenate([src, src[:9], dst[5:20]]), np.concatenate([dst, dst[:9], src[5:20]])   # duplicates and two-way edges
    out["dup_twoway"] = (src.astype(np.int32), dst.astype(np.int32), rng.integers(0, 3, (3, 37)).astype(np.int64), 3)
    a = np.arange(999, dtype=np.int32)
    one = np.zeros((1, 1000), np.int64)
    out["path_ascending"] = (a, a + 1, one, 1)
    out["path_descending"] = ((a + 1)[::-1].copy(), a[::-1].copy(), one, 1)
    pi = rng.permutation(1000).astype(np.int32)
    order = rng.permutation(999)
    out["path_shuffled"] = (pi[a][order], pi[a + 1][order], one, 1)
    out["star_hub_last"] = (np.arange(299, dtype=np.int32), np.full(299, 299, np.int32), np.zeros((1, 300), np.int64), 1)
    src, dst = _lattice(20)
    ij = np.arange(400)
    out["checkerboard"] = (src, dst, ((ij // 20 + ij % 20) % 2)[None].astype(np.int64), 2)
    src, dst = knn_edges(jittered_grid(64, rng), 6)
    out["grid64_one_label"] = (src, dst, np.zeros((1, 4096), np.int64), 1)
    for n in WIDTH_SIZES:
        r = np.random.default_rng(n)
        src, dst = random_edges(r, n, 6 * n + (n % 3) - 1)
        out[f"width_n{n}"] = (src, dst, r.integers(0, 5, (1, n)).astype(np.int64), 5)
    for side in STRIPES:
        _, plant, lab, src, dst, K = stripes(side)
        out[f"stripes{side}"] = (src, dst, np.stack([lab, plant]), K)
    return out


NAMES = ("n1", "n2", "K1", "K32_unused", "dup_twoway", "path_ascending", "path_descending", "path_shuffled", "star_hub_last",
         "checkerboard", "grid64_one_label") + tuple(f"width_n{n}" for n in WIDTH_SIZES) + tuple(f"stripes{s}" for s in STRIPES)


@functools.lru_cache(maxsize=None)
def want(name):
    """The restatement's answer of a case: (integers int64 [L, K, 4], ids [n] and sizes [n] of the first labeling)."""
    src, dst, labs, K = all_cases()[name]
    ids, sizes = ref.components(src, dst, labs[0])
    return np.stack([ref.integers(src, dst, lab, K) for lab in labs]), ids, sizes


@functools.lru_cache(maxsize=None)
def perm_problems():
    """The permuted problems: the 45 x 45 stripe map (graph 0), n = 37 (graph 1) and n = 300 (graph 2), P = 200 under SEED:
    [(src, dst, base labels, K, the restatement's [200, K, 4])]."""
    c = all_cases()
    graphs = [(c["stripes45"][0], c["stripes45"][1], c["stripes45"][2][0], 7),
              (c["dup_twoway"][0], c["dup_twoway"][1], c["dup_twoway"][2][0], 3),
              (c["K32_unused"][0], c["K32_unused"][1], c["K32_unused"][2][0], 32)]
    return [(s, d, lab, K, ref.perm_integers(s, d, lab, K, 200, SEED, g)) for g, (s, d, lab, K) in enumerate(graphs)]


def agreement(lab, plant):
    return float((np.asarray(lab) == np.asarray(plant)).mean())


def stage_table():
    """A domains.csv of two stripe maps as time points (400 and 2025 spots), the rows interleaved so that the table's order is
    not the time points' order."""
    import pandas as pd
    parts = []
    for tp, side in (("E10", 20), ("E12", 45)):
        xy, _, lab, _, _, _ = stripes(side)
        parts.append(pd.DataFrame({"timepoint": tp, "kmeans": lab, "pixel_x": xy[:, 0], "pixel_y": xy[:, 1]}))
    df = pd.concat(parts, ignore_index=True)
    df = df.iloc[np.random.default_rng(5).permutation(len(df))].reset_index(drop=True)
    df.insert(0, "row", np.arange(len(df)))
    return df
