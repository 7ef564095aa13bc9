"""The ligand-receptor definition of DESIGN 7k restated in numpy: the per-domain sums of every gene under the labelings of
nhood_ref.perm, the statistic of a cell with its roundings, the tested cells, the p-values and the rounding bound that says which
comparisons the device must reproduce.  Independent of the package (Benjamini-Hochberg from nhood_ref)."""
import numpy as np

import nhood_ref

U = 2.0 ** -53


def labelings(lab, n_perms, seed, g, first=0):
    """int64 [1 + n_perms, n]: lab, then lab[pi_p] for p = first .. first + n_perms - 1 of graph g under seed."""
    lab = np.asarray(lab, dtype=np.int64)
    return np.stack([lab] + [lab[nhood_ref.perm(lab.shape[0], seed, g, first + p)] for p in range(n_perms)])


def sums(V, labs, K, reverse=False):
    """S fp64 [L, G, K] of dense fp32 values V [n, G] (0 = nothing stored) under the labelings labs [L, n]: per gene
    np.bincount(labels, weights=v) over the stored entries in row order (reverse: in descending row order)."""
    V = np.asarray(V)
    assert V.dtype == np.float32
    S = np.zeros((labs.shape[0], V.shape[1], K))
    for g in range(V.shape[1]):
        rows = np.flatnonzero(V[:, g])
        if reverse:
            rows = rows[::-1]
        v = V[rows, g].astype(np.float64)
        for l in range(labs.shape[0]):
            S[l, g] = np.bincount(labs[l, rows], weights=v, minlength=K)[:K]
    return S


def positive_counts(V, lab, K):
    """c int64 [G, K]: the entries with v > 0 per gene and label."""
    V, lab = np.asarray(V), np.asarray(lab, dtype=np.int64)
    return np.stack([np.bincount(lab[V[:, g] > 0], minlength=K)[:K] for g in range(V.shape[1])]).astype(np.int64)


def stored(V):
    """m [G]: the stored entries of every gene."""
    return (np.asarray(V) != 0).sum(axis=0)


def weights(sizes):
    nk = np.asarray(sizes, dtype=np.float64)
    return np.array([1.0 / v if v > 0 else 0.0 for v in nk])


def stat(S, w, pairs):
    """stat [L, M, K, K] = 0.5 (S[l, src, a] w_a + S[l, tgt, b] w_b): two products and one sum, each rounded once."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    x = S * w[None, None, :]
    return 0.5 * (x[:, pairs[:, 0], :, None] + x[:, pairs[:, 1], None, :])


def tested_cells(S0, c, sizes, pairs, threshold):
    """(tested bool [M, K, K], held bool [K, K], mean [G, K], pct [G, K]) of the definition."""
    nk = np.asarray(sizes, dtype=np.float64)
    w = weights(sizes)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    G, K = S0.shape
    mean = S0 * w[None, :]
    pct = np.zeros((G, K))
    for k in range(K):
        if nk[k] > 0:
            pct[:, k] = c[:, k] / nk[k]
    M = pairs.shape[0]
    tested = np.zeros((M, K, K), dtype=bool)
    for m, (s, t) in enumerate(pairs):
        for a in range(K):
            for b in range(K):
                tested[m, a, b] = (nk[a] > 0 and nk[b] > 0 and pct[s, a] >= threshold and pct[t, b] >= threshold
                                   and mean[s, a] > 0 and mean[t, b] > 0)
    return tested, (nk[:, None] > 0) & (nk[None, :] > 0), mean, pct


def all_cells(S, c, sizes, pairs, threshold):
    """The whole host definition from the sums S [1 + P, G, K] and the counts c [G, K]: a dict of mean, pvalue, padj [M, K, K]
    (NaN as the definition says), tested, ge, gene_mean, gene_pct and stat [1 + P, M, K, K]."""
    P = S.shape[0] - 1
    tested, held, mean, pct = tested_cells(S[0], c, sizes, pairs, threshold)
    st = stat(S, weights(sizes), pairs)
    ge = (st[1:] >= st[:1]).sum(axis=0).astype(np.int64)
    out_mean = np.where(tested, st[0], np.where(held[None], 0.0, np.nan))
    pvalue, padj = np.full(tested.shape, np.nan), np.full(tested.shape, np.nan)
    if P >= 1:
        pvalue[tested] = (1.0 + ge[tested]) / (P + 1.0)
        if tested.any():
            padj[tested] = nhood_ref.bh(pvalue[tested])
    return dict(mean=out_mean, pvalue=pvalue, padj=padj, tested=tested, ge=np.where(tested, ge, 0), gene_mean=mean, gene_pct=pct,
                stat=st)


def sum_bound(S, m):
    """|S_a - S_b| of two fp64 evaluations of the same m non-negative terms in any order: 2 (m + 2) 2^-53 S (the argument of
    tests/test_trends_gpu.py with all terms >= 0).  S [L, G, K], m [G]."""
    return 2.0 * (np.asarray(m, dtype=np.float64)[None, :, None] + 2.0) * U * S


def near_ties(S, m, sizes, pairs):
    """bool [M, K, K]: the cells where some 0 < |stat_p - stat_0| lies within the bound propagated from the sums (the bounds of
    both sums of both statistics, and four roundings of each statistic): there another order of summation may compare the other
    way."""
    w = weights(sizes)
    st = stat(S, w, pairs)
    tol = stat(sum_bound(S, m), w, pairs) + 4.0 * U * st
    d = np.abs(st[1:] - st[:1])
    return ((d > 0) & (d <= tol[1:] + tol[:1])).any(axis=0)
