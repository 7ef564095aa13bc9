"""The local Moran's I definition of DESIGN 7l restated in numpy: the CSR of a stable sort by source, the sequential neighbour
sums, the conditional permutation (pi_p of nhood_ref composed with the transposition (i, pi_p^-1(i))), the two counts and the
host statistics.  Independent of the package; the permutation and Benjamini-Hochberg are those of nhood_ref."""
import numpy as np

from nhood_ref import bh, perm


def csr(src, dst, n):
    """(rowptr int64 [n + 1], col int64 [E]): the edges sorted stably by source."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.argsort(src, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    return rowptr, dst[order]


def inverse(pi):
    inv = np.empty_like(pi)
    inv[pi] = np.arange(pi.shape[0], dtype=pi.dtype)
    return inv


def conditional_map(pi, i):
    """What every spot shows while spot i is evaluated: pi with the entries of i and j* = pi^-1(i) exchanged (int64 [n])."""
    m = pi.copy()
    j = int(inverse(pi)[i])
    m[i], m[j] = pi[j], pi[i]
    return m


def lag_rows(rowptr, col, x, c, swap=None):
    """lag [n] in fp64: slot s = 0, 1, ... of every row with more than s neighbours is added in turn, so every row adds its
    neighbours in row order from 0.0.  x fp64 [n]: what every spot shows; swap int64 [n] or None: the neighbour swap[i] of
    row i shows x[i] instead (the conditional draw)."""
    n = rowptr.shape[0] - 1
    deg = np.diff(rowptr)
    lag = np.zeros(n, dtype=np.float64)
    for s in range(int(deg.max()) if n and deg.size else 0):
        rows = np.flatnonzero(deg > s)
        j = col[rowptr[rows] + s]
        val = x[j]
        if swap is not None:
            hit = j == swap[rows]
            val = np.where(hit, x[rows], val)
        lag[rows] = lag[rows] + (val - c)
    return lag


def local_counts(src, dst, n, v, c, n_perms, seed, g, first=0, replace=True):
    """(lag fp64 [n], ge int64 [n], le int64 [n]) of one gene: v fp32 [n], c its centre, graph g under seed.  replace=False drops
    the j* replacement (the unconditional permutation: what the kernel must NOT compute)."""
    rowptr, col = csr(src, dst, n)
    c = np.float64(c)
    v64 = np.asarray(v).astype(np.float64)
    lag = lag_rows(rowptr, col, v64, c)
    ge, le = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for p in range(n_perms):
        pi = perm(n, seed, g, first + p)
        lp = lag_rows(rowptr, col, v64[pi], c, inverse(pi) if replace else None)
        ge += lp >= lag
        le += lp <= lag
    return lag, ge, le


def local_counts_genes(src, dst, n, V, c, n_perms, seed, g, first=0, replace=True):
    """local_counts of every column of V [n, G] with centres c [G]: [G, n] arrays."""
    out = [local_counts(src, dst, n, V[:, k], c[k], n_perms, seed, g, first, replace) for k in range(V.shape[1])]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def jstar_hits(src, dst, n, n_perms, seed, g, first=0):
    """How many (spot, permutation) have j* = pi_p^-1(i) among the neighbours of i."""
    rowptr, col = csr(src, dst, n)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    hits = 0
    for p in range(n_perms):
        inv = inverse(perm(n, seed, g, first + p))
        hits += np.unique(rows[col == inv[rows]]).size
    return hits


def stats(lag, ge, le, v, c, n, E, P, has_neighbours):
    """The statistics of one gene, spot by spot: dict of I, p_sim, padj fp64 [n] and quadrant int64 [n]."""
    v = np.asarray(v).astype(np.float64)
    z = v - np.float64(c)
    m2, sumsq = float((z * z).sum()), float((v * v).sum())
    out = {"I": np.full(n, np.nan), "p_sim": np.full(n, np.nan), "padj": np.full(n, np.nan), "quadrant": np.zeros(n, dtype=np.int64)}
    if n < 3 or E == 0 or m2 <= n * 2.0 ** -50 * sumsq:
        return out
    for i in range(n):
        if not has_neighbours[i]:
            out["I"][i] = 0.0
            continue
        out["I"][i] = n * z[i] * lag[i] / m2
        if z[i] > 0 and lag[i] > 0:
            out["quadrant"][i] = 1
        elif z[i] < 0 and lag[i] > 0:
            out["quadrant"][i] = 2
        elif z[i] < 0 and lag[i] < 0:
            out["quadrant"][i] = 3
        elif z[i] > 0 and lag[i] < 0:
            out["quadrant"][i] = 4
        larger = ge[i] if z[i] > 0 else (le[i] if z[i] < 0 else P)
        smaller = le[i] if z[i] > 0 else (ge[i] if z[i] < 0 else P)
        out["p_sim"][i] = (1 + min(int(larger), int(smaller))) / (P + 1)
    fam = np.asarray(has_neighbours, dtype=bool)
    if fam.any():
        out["padj"][fam] = bh(out["p_sim"][fam])
    return out
