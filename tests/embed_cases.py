"""The inputs of the embed tests, from fixed seeds (numpy only)."""
import numpy as np

# (name, d, n, perplexity): what each exercises is said beside it
NEIGHBOR_CASES = [
    ("dense", 20, 91, 30.0),             # k = n - 1: P is dense
    ("padded", 3, 257, 5.0),             # padding of d, one point past a tile
    ("smallest", 1, 256, 2.0),           # smallest d and perplexity
    ("largest", 32, 513, 50.0),          # k = 150, the largest d
    ("lattice", 2, 400, 4.0),            # the 20 x 20 integer lattice: exact distance ties, broken by index
    ("duplicates", 8, 130, 10.0),        # 40 rows are copies of row 0: more duplicates than the perplexity
    ("uniform", 4, 34, 10.0),            # all rows equal: the uniform rule
]

# (d, n, perplexity) of the optimiser cases: Gaussian blobs, six centres three standard deviations apart
OPTIMISER_CASES = [(20, 300, 30.0), (20, 91, 30.0), (8, 513, 5.0), (20, 255, 30.0), (20, 256, 30.0)]

BATCH_SIZES = (91, 257, 513)             # d = 20: three problems of one neighbour launch


def blobs(d, n, seed, centres=6, spread=3.0):
    """n points with unit normal scatter around `centres` centres that lie `spread` standard deviations apart per coordinate (the
    centres are spread * normal draws)."""
    rng = np.random.default_rng(seed)
    c = spread * rng.normal(size=(centres, d))
    return c[rng.integers(0, centres, n)] + rng.normal(size=(n, d))


def neighbor_case(name):
    """(X fp64 [n, d], perplexity) of a neighbour and affinity case."""
    _name, d, n, u = next(c for c in NEIGHBOR_CASES if c[0] == name)
    seed = 7000 + [c[0] for c in NEIGHBOR_CASES].index(name)
    if name == "lattice":
        g = np.arange(20, dtype=np.float64)
        X = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(400, 2)
    elif name == "uniform":
        X = np.tile(np.random.default_rng(seed).normal(size=(1, d)), (n, 1))
    else:
        X = blobs(d, n, seed)
        if name == "duplicates":
            rows = np.random.default_rng(seed + 1).choice(np.arange(1, n), 39, replace=False)
            X[rows] = X[0]
    return np.ascontiguousarray(X), u


def optimiser_case(d, n):
    """The points of the optimiser case (d, n, .)."""
    return np.ascontiguousarray(blobs(d, n, 9000 + 7 * d + n))


def stage_latents(seed=4242):
    """A latent file's arrays for the stage tests: three time points of 120, 257 and 300 spots (d = 20), the rows shuffled and with
    row ids of their own, and a domains table of its rows: (X, timepoint, spatial, rows, kmeans)."""
    rng = np.random.default_rng(seed)
    sizes, names = (120, 257, 300), ("E1", "E2", "E3")
    X = np.concatenate([blobs(20, n, seed + i, centres=4) for i, n in enumerate(sizes)])
    tp = np.concatenate([[t] * n for t, n in zip(names, sizes)])
    lab = np.concatenate([rng.integers(0, 4, n) for n in sizes])
    for t in names:                                              # every domain occurs in every time point
        lab[np.flatnonzero(tp == t)[:4]] = np.arange(4)
    order = rng.permutation(X.shape[0])
    rows = 1000 + rng.permutation(X.shape[0])
    return (np.ascontiguousarray(X[order]), tp[order], rng.uniform(0, 100, size=(X.shape[0], 2)), rows.astype(np.int64),
            lab[order].astype(np.int64))
