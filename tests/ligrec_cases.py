"""Inputs of the ligand-receptor tests (CPU and GPU): the planted 20 x 20 grid with two raised genes, the problems whose p-values
the device must reproduce, the launch of four small time points, the shapes that straddle the wavefront and the gene chunk, and
the files of the stage.  Every value is a continuous draw, fp32(log1p(gamma)) with many zeros, as a log-normalised count could
be: different subsets of spots do not tie mathematically."""
import functools
import os

import numpy as np

import ligrec_ref as ref
import nhood_cases as nc
from autocorr_cases import csc  # noqa: F401  (the host-side CSC of time points stacked row-wise)

SEED = nc.SEED
GC, THREADS = 128, 512                         # the library's genes per chunk and workgroup (spadot_amd.stage_ops.LIGREC_*)


def values(rng, n, G, density=0.3):
    """fp32 [n, G] log1p(gamma) draws with about `density` of the entries nonzero."""
    return (np.log1p(rng.gamma(2.0, 1.0, (n, G))) * (rng.uniform(size=(n, G)) < density)).astype(np.float32)


def all_pairs(G, M, rng):
    """M distinct (source, target) pairs over G genes, (0, 1) first and one pair with source == target."""
    pairs = [(0, 1), (2, 2)] if G > 2 else [(0, G - 1), (0, 0)]
    while len(pairs) < M:
        p = (int(rng.integers(G)), int(rng.integers(G)))
        if p not in pairs:
            pairs.append(p)
    return np.asarray(pairs[:M], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def planted():
    """(V fp32 [400, 12], lab int64 [400], K = 4, pairs [6, 2]) on nhood_cases.planted(20): gene 0 is raised in domain 0 and gene 1
    in domain 1, gene 2 is stored in 5 % of the spots (below the threshold of 0.1 in most domains), the rest is noise."""
    _, lab, _, _, K = nc.planted(20)
    rng = np.random.default_rng(17)
    V = values(rng, 400, 12, density=0.6).astype(np.float64)
    V[:, 0] += np.log1p(rng.gamma(4.0, 1.0, 400)) * (lab == 0)
    V[:, 1] += np.log1p(rng.gamma(4.0, 1.0, 400)) * (lab == 1)
    V[:, 2] = np.log1p(rng.gamma(2.0, 1.0, 400)) * (rng.uniform(size=400) < 0.05)
    pairs = np.asarray([(0, 1), (2, 3), (3, 3), (4, 5), (1, 0), (6, 2)], dtype=np.int64)
    return V.astype(np.float32), lab, K, pairs


PVALUE_CASES = (("n300_K4", 300, 4, 8, 8, 200), ("n257_K7", 257, 7, 9, 10, 200), ("n64_K3", 64, 3, 6, 16, 200),
                ("n1025_K32", 1025, 32, 10, 12, 100))          # name, n, K, genes, interactions, permutations


@functools.lru_cache(maxsize=None)
def pvalue_case(name):
    """(V fp32 [n, G], lab int64 [n], K, pairs [M, 2], P) of one entry of PVALUE_CASES; every label 0 .. K-1 occurs."""
    _, n, K, G, M, P = next(c for c in PVALUE_CASES if c[0] == name)
    rng = np.random.default_rng(1000 + n)
    lab = rng.integers(K, size=n)
    lab[:K] = np.arange(K)
    return values(rng, n, G, density=0.5), lab.astype(np.int64), K, all_pairs(G, M, rng), P


@functools.lru_cache(maxsize=None)
def pvalue_ref(name, reverse=False):
    """The restatement of pvalue_case(name) under (SEED, graph 0) at threshold 0.1: (S [1 + P, G, K], c, sizes, the dict of
    ligrec_ref.all_cells, near bool [M, K, K]: the cells a rounding could flip)."""
    V, lab, K, pairs, P = pvalue_case(name)
    S = ref.sums(V, ref.labelings(lab, P, SEED, 0), K, reverse=reverse)
    c, sizes = ref.positive_counts(V, lab, K), np.bincount(lab, minlength=K)
    return S, c, sizes, ref.all_cells(S, c, sizes, pairs, 0.1), ref.near_ties(S, ref.stored(V), sizes, pairs)


@functools.lru_cache(maxsize=None)
def call4():
    """Four time points of one launch, [(V fp32 [n, 5], lab int64 [n])], K = 4: n = 1, n = 2, n = 37 with domain 2 empty, n = 300.
    Gene 0 is all zero in time point 2 only, gene 1 is stored in every spot, gene 2 is a single nonzero, genes 3 and 4 are
    noise."""
    rng = np.random.default_rng(29)
    out = []
    for t, n in enumerate((1, 2, 37, 300)):
        V = values(rng, n, 5, density=0.6)
        V[:, 0] = 0.0 if t == 2 else V[:, 0] + np.float32(0.5) * (np.arange(n) == 0)
        V[:, 1] = np.log1p(0.25 + rng.gamma(2.0, 1.0, n)).astype(np.float32)
        V[:, 2] = 0.0
        V[n // 2, 2] = 1.75
        lab = rng.integers(4, size=n)
        if t == 2:
            lab[lab == 2] = 3
        if t == 3:
            lab[:4] = np.arange(4)
        out.append((V, lab.astype(np.int64)))
    return out


CALL4_PAIRS = np.asarray([(0, 1), (1, 2), (2, 2), (2, 0), (3, 4), (1, 1)], dtype=np.int64)
SPOTS = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
STORED = (0, 1, 63, 64, 65, 129)


def spots_case(n, K=5, G=3):
    """(V fp32 [n, G], lab int64 [n], K) of a time point whose n straddles the label words, the wavefront and the workgroup.  The
    last gene spans 40 binary orders of magnitude: its fp64 sums are not exact, so their bits depend on the order of the
    additions (the sums of the other genes, fp32 values of one magnitude, are exact in fp64 in any order)."""
    rng = np.random.default_rng(7000 + 31 * n + K + G)
    V = values(rng, n, G, density=0.5)
    V[:, -1] *= (2.0 ** -rng.integers(0, 40, n)).astype(np.float32)
    return V, rng.integers(K, size=n).astype(np.int64), K


@functools.lru_cache(maxsize=None)
def stored_case():
    """Two time points (n = 150 and n = 200), K = 6, whose gene k has STORED[k] stored entries in the second one: every ridx
    segment of the second time point starts mid-column."""
    rng = np.random.default_rng(35)
    V0 = values(rng, 150, len(STORED), density=0.4)
    V1 = np.zeros((200, len(STORED)), dtype=np.float32)
    for k, cnt in enumerate(STORED):
        V1[rng.permutation(200)[:cnt], k] = np.log1p(0.1 + rng.gamma(2.0, 1.0, cnt)).astype(np.float32)
    assert [(V1[:, k] != 0).sum() for k in range(len(STORED))] == list(STORED)
    return [(V0, rng.integers(6, size=150).astype(np.int64)), (V1, rng.integers(6, size=200).astype(np.int64))]


def want_sums(problems, K, n_perms, seed=SEED, first=0, genes=None):
    """The restatement of a launch: [t] -> (S [1 + P, genes, K], c [genes, K], m [genes])."""
    out = []
    for t, (V, lab) in enumerate(problems):
        W = V if genes is None else V[:, np.asarray(genes)]
        out.append((ref.sums(W, ref.labelings(lab, n_perms, seed, t, first), K), ref.positive_counts(W, lab, K), ref.stored(W)))
    return out


STAGE_TPS = (("E10", 300, 4), ("E12", 400, 5), ("E14", 500, 6))
STAGE_GENES = 24


def stage_files(out):
    """Writes counts.npz, domains.csv and pairs.csv of the stage test into `out` and returns their paths: three planted time
    points (300, 400 and 500 spots; 4, 5 and 6 domains), interleaved, 24 genes of which gene g < 6 is raised in domain g % K; the
    pairs name 10 genes, one pair twice and one with a gene that the data does not have."""
    import pandas as pd
    rng = np.random.default_rng(8)
    parts, tps, xys, labs = [], [], [], []
    for tp, n, K in STAGE_TPS:
        xy, lab = nc.planted_points(rng, n, K)
        rate = np.full((n, STAGE_GENES), 0.4)
        for g in range(6):
            rate[:, g] += 3.0 * (lab == g % K)
        rate[:, STAGE_GENES - 1] = 0.0
        parts.append(rng.poisson(rate).astype(np.float32))
        tps += [tp] * n
        xys.append(xy)
        labs.append(lab)
    order = rng.permutation(len(tps))
    names = np.asarray([f"g{g:02d}" for g in range(STAGE_GENES)])
    counts = os.path.join(out, "counts.npz")
    np.savez(counts, X=np.concatenate(parts)[order], timepoint=np.asarray(tps)[order], spatial=np.concatenate(xys)[order],
             genes=names)
    domains = os.path.join(out, "domains.csv")
    pd.DataFrame({"row": np.arange(len(tps)), "timepoint": np.asarray(tps)[order],
                  "kmeans": np.concatenate(labs)[order]}).to_csv(domains, index=False)
    pairs = os.path.join(out, "pairs.csv")
    rows = [("g00", "g01"), ("g01", "g00"), ("g02", "g03"), ("g00", "g01"), ("g04", "g04"), ("g05", "g10"), ("g11", "nope"),
            ("g12", "g13"), ("g14", "g23"), ("g02", "g12")]
    pd.DataFrame(rows, columns=["source", "target"]).to_csv(pairs, index=False)
    return counts, domains, pairs
