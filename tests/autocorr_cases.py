"""Inputs of the spatial-autocorrelation tests (CPU and GPU), built on nhood_cases: six test genes on the 20 x 20 planted grid with
the restatement's sums under 200 permutations, the edge call, the graphs that straddle the workgroup, genes whose stored counts
straddle a wavefront and the workgroup, the host-side CSC of a set of time points and the counts file of the stage.  Every value
is an fp32 that a log-normalised count could be: not negative, many zeros."""
import functools

import numpy as np

import autocorr_ref as ref
import nhood_cases as nc

SEED = nc.SEED
GS, THREADS = 2, 1024                          # the library's genes per group and workgroup (spadot_amd.stage_ops.AUTOCORR_*)
PLANTED_GENES = ("gradient", "marker", "noise_a", "noise_b", "checkerboard", "single")
PLANTED_PERMS = 200
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def planted_genes():
    """(src, dst, V fp32 [400, 6]) on nhood_cases.planted(20): a gradient along x and a domain marker under noise, two noise
    genes (one with zeros), a checkerboard on the grid cells and a single nonzero."""
    xy, lab, src, dst, _ = nc.planted(20)
    n = xy.shape[0]
    rng = np.random.default_rng(7)
    cell = np.rint(xy).astype(np.int64)
    V = np.zeros((n, 6))
    V[:, 0] = np.maximum(0.0, 1.5 + xy[:, 0] / 10.0 + 0.95 * rng.normal(size=n))
    V[:, 1] = np.maximum(0.0, 1.0 + (lab == 1) + 0.68 * rng.normal(size=n))
    V[:, 2] = rng.gamma(2.0, 0.5, n)
    V[:, 3] = rng.uniform(0.0, 2.0, n) * (rng.uniform(size=n) < 0.7)
    V[:, 4] = (cell[:, 0] + cell[:, 1]) % 2
    V[137, 5] = 1.5
    return src, dst, V.astype(np.float32)


def centres(V):
    """The fp64 mean of every fp32 column."""
    return np.asarray(V).astype(np.float64).mean(axis=0)


def bound_N(E, A):
    """|N_a - N_b| of two fp64 evaluations of the same E terms in any order (tests/test_autocorr_gpu.py, Tolerance)."""
    return 4.0 * (E + 2) * U * A


@functools.lru_cache(maxsize=None)
def planted_sums():
    """The restatement's N, D, A [6, 1 + 200] of planted_genes under (SEED, graph 0), and the genes whose p_sim the device must
    reproduce: those whose smallest |N_p - N_0| and |D_p - D_0| exceed the rounding bound of the comparison.  Asserted here:
    that rule keeps every gene but the single nonzero (whose permuted sums tie with the observed one exactly)."""
    src, dst, V = planted_genes()
    N, D, A = ref.all_sums_genes(src, dst, V, centres(V), PLANTED_PERMS, SEED, 0)
    E = src.shape[0]
    clear = np.array([np.abs(N[g, 1:] - N[g, 0]).min() > bound_N(E, A[g].max()) and
                      np.abs(D[g, 1:] - D[g, 0]).min() > bound_N(E, D[g].max()) for g in range(V.shape[1])])
    assert clear.tolist() == [True, True, True, True, True, False], clear
    return N, D, A, clear


def random_values(rng, n, G, density=0.3):
    """fp32 [n, G] with about `density` of the entries nonzero."""
    return (rng.gamma(2.0, 0.5, (n, G)) * (rng.uniform(size=(n, G)) < density)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def edge_call():
    """Four time points of one call, [(src, dst, V fp32 [n, 4])]: n = 1 without edges, n = 2, n = 37 with a duplicate and a
    reciprocal edge, n = 300.  Gene 0 is all zero in time point 2 only, gene 1 nonzero in every spot, gene 2 a single nonzero,
    gene 3 a constant nonzero gene (m2 = 0)."""
    rng = np.random.default_rng(21)
    graphs = nc.edge_call()
    out = []
    for t, (src, dst, _, _) in enumerate(graphs):
        n = (1, 2, 37, 300)[t]
        if t == 2:
            src, dst = np.append(src, dst[9]), np.append(dst, src[9])            # the reciprocal of edge 9
        V = np.zeros((n, 4), dtype=np.float32)
        V[:, 0] = 0.0 if t == 2 else rng.gamma(2.0, 0.5, n) * (rng.uniform(size=n) < 0.6) + (np.arange(n) == 0)
        V[:, 1] = 0.25 + rng.gamma(2.0, 0.5, n)
        V[n // 2, 2] = 2.0
        V[:, 3] = 0.7
        out.append((src.astype(np.int32), dst.astype(np.int32), V))
    return out


TILE_CASES = ([(f"n{n}_E{E}", n, E) for w in (256, THREADS) for n in (w - 1, w, w + 1) for E in ((w - 1) * 6, w * 6 + 1)]
              + [("n257_E0", 257, 0), (f"n{THREADS + 1}_E0", THREADS + 1, 0)])
GROUP_SIZES = (1, GS - 1, GS, GS + 1, 2 * GS + 1)


def tile_case(name, G=3):
    """(src, dst, V fp32 [n, G]) of a graph whose n and E straddle the wavefront-multiple workgroup sizes."""
    _, n, E = next(c for c in TILE_CASES if c[0] == name)
    rng = np.random.default_rng(n * 100003 + E + G)
    src, dst = nc.random_edges(rng, n, E) if E else (np.zeros(0, np.int32), np.zeros(0, np.int32))
    return src, dst, random_values(rng, n, G)


STORED = (0, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, THREADS + 76)


@functools.lru_cache(maxsize=None)
def stored_case():
    """Two time points (n = 300 and n = THREADS + 76) whose gene k has STORED[k] stored entries in the second one: the stored
    count straddles the wavefront and the workgroup, and every ridx segment of the second time point starts mid-column."""
    rng = np.random.default_rng(33)
    n0, n1 = 300, THREADS + 76
    V0 = random_values(rng, n0, len(STORED))
    V1 = np.zeros((n1, len(STORED)), dtype=np.float32)
    for k, cnt in enumerate(STORED):
        V1[rng.permutation(n1)[:cnt], k] = (0.1 + rng.gamma(2.0, 0.5, cnt)).astype(np.float32)
    assert [(V1[:, k] != 0).sum() for k in range(len(STORED))] == list(STORED)
    return [nc.random_edges(rng, n0, 6 * n0) + (V0,), nc.random_edges(rng, n1, 6 * n1) + (V1,)]


@functools.lru_cache(maxsize=None)
def perm_case():
    """Three graphs under 200 permutations: the 45 x 45 planted grid, n = 37 and n = 300, three genes each (dense, sparse and
    very sparse), with the restatement's N, D, A [3, 201] per graph under (SEED, graph index)."""
    rng = np.random.default_rng(44)
    call = edge_call()
    _, _, s45, d45, _ = nc.planted(45)
    graphs = []
    for g, (src, dst) in enumerate(((s45, d45), call[2][:2], call[3][:2])):
        n = (2025, 37, 300)[g]
        V = np.stack([0.2 + rng.gamma(2.0, 0.5, n), rng.gamma(2.0, 0.5, n) * (rng.uniform(size=n) < 0.3),
                      rng.gamma(2.0, 0.5, n) * (rng.uniform(size=n) < 0.08) + (np.arange(n) == 1)], axis=1).astype(np.float32)
        graphs.append((src, dst, V))
    want = [ref.all_sums_genes(s, d, V, centres(V), 200, SEED, g) for g, (s, d, V) in enumerate(graphs)]
    return graphs, want


def csc(Vs):
    """The host-side CSC of time points stacked row-wise, zeros not stored: colptr int64 [G + 1], ridx int32, vals fp32, tp_off
    int64 [T + 1] (the layout of a DeviceCounts)."""
    X = np.concatenate(Vs, axis=0)
    cols, rows = np.nonzero(X.T)
    colptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=X.shape[1]))]).astype(np.int64)
    tp_off = np.concatenate([[0], np.cumsum([V.shape[0] for V in Vs])]).astype(np.int64)
    return colptr, rows.astype(np.int32), X.T[cols, rows].astype(np.float32), tp_off


def stage_counts(path):
    """Writes the counts .npz of the stage test: three planted time points (400, 500 and 600 spots, interleaved), 40 genes:
    ten follow a domain, ten a gradient, the rest are noise; gene 39 is never counted."""
    rng = np.random.default_rng(6)
    parts, tps, xys = [], [], []
    for tp, n, K in (("E10", 400, 4), ("E12", 500, 5), ("E14", 600, 6)):
        xy, lab = nc.planted_points(rng, n, K)
        rate = np.full((n, 40), 0.5)
        for g in range(10):
            rate[:, g] += 4.0 * (lab == g % K)
            rate[:, 10 + g] += 4.0 * xy[:, g % 2] / np.sqrt(n)
        rate[:, 39] = 0.0
        parts.append(rng.poisson(rate).astype(np.float32))
        tps += [tp] * n
        xys.append(xy)
    order = rng.permutation(len(tps))
    np.savez(path, X=np.concatenate(parts)[order], timepoint=np.asarray(tps)[order], spatial=np.concatenate(xys)[order],
             genes=np.asarray([f"g{g:02d}" for g in range(40)]))
    return path
