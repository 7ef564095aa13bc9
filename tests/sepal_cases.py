"""Inputs of the sepal tests (CPU and GPU).  A case is a list of time points (src, dst, V fp32 [n, genes]) and a dt; its genes are
GENES: one without a stored entry, one with a single positive spot, a constant one, one stored in every spot and a sparse one.
Every value is an fp32 that a log-normalised count could be: not negative, many zeros."""
import functools

import numpy as np

import nhood_cases as nc
import sepal_ref as ref

W = 1024                                       # the workgroup (spadot_amd.stage_ops.SEPAL_THREADS)
SIZES = (1, 2, 3, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1)
GENES = ("empty", "single", "constant", "dense", "sparse")
RAGGED = (65, 257, 513)
DT, THRESH, N_ITER = 0.1, 1e-8, 30000          # the defaults of the stage
HUB_DT = 0.02                                  # the hub's largest degree admits no more than 0.0232..
STEPS = 50
PLANTED = dict(spots_per_tp=(400,), n_genes=200, n_modules=4, genes_per_module=10, n_rare=5, seed=3)
PLANTED_GENES = tuple(range(0, 10)) + tuple(range(20, 30)) + tuple(range(40, 60))      # modules 0 and 2 (bumps) and 20 null genes


def knn(xy, k):
    """Directed k-nearest-neighbour edges (ties by index), k cut to n - 1; no edges for one spot."""
    n = xy.shape[0]
    if n < 2:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    return nc.knn_edges(xy, min(k, n - 1))


def genes(rng, n):
    """V fp32 [n, 5] in the order of GENES."""
    V = np.zeros((n, len(GENES)))
    V[n // 2, 1] = 1.5
    V[:, 2] = 0.7
    V[:, 3] = 0.25 + rng.gamma(2.0, 0.5, n)
    V[:, 4] = rng.gamma(2.0, 0.5, n) * (rng.uniform(size=n) < 0.3)
    return V.astype(np.float32)


def points(rng, n):
    return rng.uniform(0.0, np.sqrt(n), (n, 2))


@functools.lru_cache(maxsize=None)
def size_case(n):
    """One time point of n random spots on its 6-nearest-neighbour graph."""
    rng = np.random.default_rng(1000 + n)
    return [knn(points(rng, n), 6) + (genes(rng, n),)], DT


def lattice_edges(side=12):
    ii, jj = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    return knn(np.stack([ii.reshape(-1), jj.reshape(-1)], axis=1).astype(np.float64), 4)


@functools.lru_cache(maxsize=None)
def lattice():
    """A 12 x 12 square lattice, k = 4, no jitter: the spots two or more steps from the border have their four lattice
    neighbours as their row, each twice (the spots of the border reach further, by index where distances tie)."""
    return [lattice_edges() + (genes(np.random.default_rng(12), 144),)], DT


@functools.lru_cache(maxsize=None)
def ragged():
    """Three time points of 65, 257 and 513 spots in one call."""
    rng = np.random.default_rng(77)
    return [knn(points(rng, n), 6) + (genes(rng, n),) for n in RAGGED], DT


@functools.lru_cache(maxsize=None)
def hub():
    """A caller's graph: a ring of 300 spots in which spot 0 also points at 118 others (degree 120)."""
    n = 300
    rng = np.random.default_rng(5)
    far = 2 + rng.permutation(n - 3)[:118]                                   # neither itself nor its ring neighbours
    src = np.concatenate([np.arange(n), np.zeros(118, np.int64)]).astype(np.int32)
    dst = np.concatenate([(np.arange(n) + 1) % n, far]).astype(np.int32)
    rowptr, _ = ref.sym_csr(src, dst, n)
    assert np.diff(rowptr).max() == 120 and np.diff(rowptr)[0] == 120
    return [(src, dst, genes(rng, n))], HUB_DT


@functools.lru_cache(maxsize=None)
def loose():
    """A caller's graph of 40 spots: spot 7 has no edge at all, spot 5 has a self-loop and the edge 3 -> 4 stands twice."""
    n = 40
    rng = np.random.default_rng(9)
    src, dst = nc.random_edges(rng, n, 5 * n)
    keep = (src != 7) & (dst != 7)
    src = np.concatenate([src[keep], [5, 3, 3]]).astype(np.int32)
    dst = np.concatenate([dst[keep], [5, 4, 4]]).astype(np.int32)
    V = genes(rng, n)
    V[7, 4] = 1.25                                                           # the lone spot keeps a value of its own
    return [(src, dst, V)], DT


CASES = {"lattice": lattice, "ragged": ragged, "hub": hub, "loose": loose}
CASES.update({f"n{n}": functools.partial(size_case, n) for n in SIZES})


def graph_numbers(src, dst, n):
    """(rowptr, col, E, the largest degree) of one time point."""
    rowptr, col = ref.sym_csr(src, dst, n)
    return rowptr, col, int(len(src)), int(np.diff(rowptr).max()) if n else 0


@functools.lru_cache(maxsize=None)
def want_diffuse(name, steps=STEPS):
    """The restatement of diffuse on a case: [t] -> (images fp64 [n, genes], parts [genes][steps + 1] of (H, S, A))."""
    problems, dt = CASES[name]()
    out = []
    for src, dst, V in problems:
        n = V.shape[0]
        rowptr, col, E, _ = graph_numbers(src, dst, n)
        a = ref.rate(dt, n, E) if E else 0.0
        res = [ref.diffuse(V[:, g].astype(np.float64), rowptr, col, a, steps) for g in range(V.shape[1])]
        out.append((np.stack([r[0] for r in res], axis=1), [r[1] for r in res]))
    return out


def want_runs(problems, dt, thresh=THRESH, n_iter=N_ITER):
    """The restatement of sepal on the time points of a case: [t] -> [gene] -> sepal_ref.Run."""
    out = []
    for src, dst, V in problems:
        n = V.shape[0]
        rowptr, col, E, _ = graph_numbers(src, dst, n)
        out.append(ref.run_genes(V.astype(np.float64), rowptr, col, ref.rate(dt, n, E) if E else 0.0, dt, thresh, n_iter))
    return out


@functools.lru_cache(maxsize=None)
def want_ragged_runs():
    return want_runs(*ragged())


@functools.lru_cache(maxsize=None)
def planted_raw():
    from spadot_amd.synthetic import make_raw_counts
    return make_raw_counts(**PLANTED)


def host_lognorm(X):
    """fp32 log1p(count * 1e4 / row total) of dense counts, 0 where the count is 0 (the values of trends.lognorm_values up to
    the rounding of the device's fp32 logarithm; the CPU test runs on these, the GPU test on the device's own)."""
    X = np.asarray(X, dtype=np.float64)
    total = X.sum(axis=1, keepdims=True)
    return np.log1p(X * 1e4 / np.where(total > 0, total, 1.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def planted_scores():
    """The restatement's runs of all 200 genes of the planted data set on its 6-nearest-neighbour graph, from host_lognorm."""
    raw = planted_raw()
    src, dst = knn(np.asarray(raw.obsm["spatial"], dtype=np.float64), 6)
    return want_runs([(src, dst, host_lognorm(raw.X))], DT)[0]
