"""The bivariate Moran's I between genes of DESIGN 7m restated in numpy: the centred values, the sequential lag over the CSR of a
stable sort by source, the cross sums of the identity and of the relabelings (the permuted gene against the FIXED lag of the other
one), the symmetrised statistic, the two-sided permutation null and the host statistics.  Independent of the package; the CSR and
the lag are those of hotspots_ref, the permutation and Benjamini-Hochberg those of nhood_ref."""
import numpy as np

from hotspots_ref import csr, lag_rows
from nhood_ref import bh, perm

U = 2.0 ** -53


def centred(V, c):
    """Z [n, G]: the fp32 columns promoted to fp64 minus their centres."""
    return np.asarray(V).astype(np.float64) - np.asarray(c, dtype=np.float64)[None, :]


def lag(src, dst, V, c):
    """Y [n, G]: per gene the sequential fp64 sum of z over the row of every spot, in row order (hotspots_ref.lag_rows)."""
    V = np.asarray(V)
    n, G = V.shape
    rowptr, col = csr(src, dst, n)
    Y = np.zeros((n, G), dtype=np.float64)
    for k in range(G):
        Y[:, k] = lag_rows(rowptr, col, V[:, k].astype(np.float64), np.float64(c[k]))
    return Y


def lag_dense(src, dst, Z):
    """A z with A the dense n x n matrix of edge multiplicities (another order of the same additions)."""
    n = Z.shape[0]
    A = np.zeros((n, n), dtype=np.float64)
    np.add.at(A, (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)), 1.0)
    return A @ Z


def labelings(n, n_perms, seed, g, first=0, observed=True):
    return ([np.arange(n)] if observed else []) + [perm(n, seed, g, first + p) for p in range(n_perms)]


def cross_sums(src, dst, V, c, n_perms, seed, g, first=0, observed=True):
    """(M, A) fp64 [L, G, G]: M[l, g, h] = sum_i z_g[pi_l(i)] Y[i, h] and A, the same sum over the absolute values of its terms
    (the size behind the rounding bound of a comparison).  Labeling 0 is the identity (if observed), then the permutations
    first .. first + n_perms - 1 of graph g under seed."""
    Z, Y = centred(V, c), lag(src, dst, V, c)
    maps = labelings(Z.shape[0], n_perms, seed, g, first, observed)
    M = np.stack([Z[m].T @ Y for m in maps]) if maps else np.zeros((0, Z.shape[1], Z.shape[1]))
    A = np.stack([np.abs(Z[m]).T @ np.abs(Y) for m in maps]) if maps else np.zeros_like(M)
    return M, A


def bound_M(n, A):
    """|M_a - M_b| of two fp64 evaluations of the same n products in any order, fused or not: each within (n + 2) 2^-53 A of the
    exact sum (n - 1 additions and one rounding per product, first order, with a factor 2 for the higher orders), so the two
    within 4 (n + 2) 2^-53 A of one another -- the argument of autocorr_cases.bound_N with n terms."""
    return 4.0 * (n + 2) * U * A


def symmetrised(M):
    """B[l] = (M[l] + M[l]^T) / 2."""
    M = np.asarray(M, dtype=np.float64)
    return 0.5 * (M + np.swapaxes(M, -1, -2))


def counts(M):
    """ge [G, G] int64 = #{p : |B[1 + p]| >= |B[0]|} of sums whose labeling 0 is the observed one."""
    B = symmetrised(M)
    return (np.abs(B[1:]) >= np.abs(B[:1])).sum(axis=0).astype(np.int64)


def spread(V, c):
    """(m2, sumsq) [G]: sum (v - c)^2 and sum v^2 in fp64."""
    Z, V64 = centred(V, c), np.asarray(V).astype(np.float64)
    return (Z * Z).sum(axis=0), (V64 * V64).sum(axis=0)


def degenerate(n, E, m2, sumsq):
    m2, sumsq = np.asarray(m2, dtype=np.float64), np.asarray(sumsq, dtype=np.float64)
    return np.full(m2.shape, True) if n < 3 or E == 0 else ~(m2 > n * 2.0 ** -50 * sumsq)


def stats(M, n, E, m2, sumsq):
    """The statistics of one time point from M [1 + P, G, G] (labeling 0 observed): dict of R, z_sim, p_sim, padj fp64 [G, G], ge
    int64 [G, G] and `degenerate` [G]; NaN in the row and column of a degenerate gene, padj over the pairs g < h of the others."""
    M = np.asarray(M, dtype=np.float64)
    P, G = M.shape[0] - 1, M.shape[1]
    bad = degenerate(n, E, m2, sumsq)
    B = symmetrised(M)
    out = {k: np.full((G, G), np.nan) for k in ("R", "z_sim", "p_sim", "padj")}
    out["degenerate"], out["ge"] = bad, counts(M) if P >= 1 else np.zeros((G, G), dtype=np.int64)
    for g in range(G):
        for h in range(G):
            if bad[g] or bad[h]:
                continue
            scale = n / (E * np.sqrt(m2[g] * m2[h]))
            out["R"][g, h] = scale * B[0, g, h]
            if P >= 1:
                sims = scale * B[1:, g, h]
                sd = sims.std()
                if sd > 0:
                    out["z_sim"][g, h] = (out["R"][g, h] - sims.mean()) / sd
                out["p_sim"][g, h] = (1 + int(out["ge"][g, h])) / (P + 1)
    pairs = [(g, h) for g in range(G) for h in range(g + 1, G) if not bad[g] and not bad[h]]
    if P >= 1 and pairs:
        adj = bh([out["p_sim"][g, h] for g, h in pairs])
        for (g, h), v in zip(pairs, adj):
            out["padj"][g, h] = out["padj"][h, g] = v
    return out


def margin_share(M, A, n):
    """(close, total): the (pair g <= h, permutation) comparisons whose ||B_p| - |B_0|| lies inside the rounding bound of the
    comparison -- bound_M of the larger A of the four sums involved -- and all of them."""
    B = symmetrised(M)
    S = np.maximum(A, np.swapaxes(A, -1, -2))
    bound = bound_M(n, np.maximum(S[1:], S[:1]))
    iu = np.triu_indices(M.shape[1])
    close = (np.abs(np.abs(B[1:]) - np.abs(B[:1])) <= bound)[:, iu[0], iu[1]]
    return close, close.size


def scores(Z, m2, n, labels):
    """The module scores [modules, n]: the mean over the module's genes (ascending) of z_g / sqrt(m2_g / n)."""
    labels = np.asarray(labels)
    K = int(labels.max()) + 1 if labels.size else 0
    out = np.zeros((K, Z.shape[0]))
    for k in range(K):
        members = np.flatnonzero(labels == k)
        for g in members:
            out[k] = out[k] + Z[:, g] / np.sqrt(m2[g] / n)
        out[k] = out[k] / members.size
    return out


def jaccard(a, b):
    """The Jaccard index of every (module of a, module of b) from sets of gene positions."""
    a, b = np.asarray(a), np.asarray(b)
    Ka, Kb = int(a.max()) + 1 if a.size else 0, int(b.max()) + 1 if b.size else 0
    out = np.zeros((Ka, Kb))
    for i in range(Ka):
        for j in range(Kb):
            sa, sb = set(np.flatnonzero(a == i).tolist()), set(np.flatnonzero(b == j).tolist())
            out[i, j] = len(sa & sb) / max(len(sa | sb), 1)
    return out
