"""The definition of the correlogram stage, restated in numpy: what csrc/correlogram.hip and spadot_amd.correlogram are
held to.  It forms the n x n matrix of squared distances, which the device never does.

    band(i, j) = #{t : r2[t] < d2(i, j)}  for i != j  (B: beyond the last threshold, in no band), d2 the unfused squared distance of
                 cooccur_ref.d2_matrix
    cnt_b(i) = #{j : band(i, j) = b},   W[b] = sum_i cnt_b(i),   S2c[b] = sum_i cnt_b(i)^2
    N[g, b] = sum over the pairs of band b of x_i x_j,   Q[g, b] = sum_i cnt_b(i) x_i^2       (x: centred values, fp64)
Labeling 1 + p shows spot i the row pi_p(i) of the centred values, pi_p = nhood_ref.perm(n, seed, g, p)."""
import numpy as np

import cooccur_ref
import nhood_ref


def bands(xy, r2):
    """int64 [n, n]: the band of every ordered pair; B on the diagonal and beyond the last threshold."""
    r2 = np.asarray(r2, dtype=np.float64).reshape(-1)
    d2 = cooccur_ref.d2_matrix(xy)
    band = (r2[None, None, :] < d2[:, :, None]).sum(axis=2).astype(np.int64)
    band[np.eye(d2.shape[0], dtype=bool)] = r2.shape[0]
    return band


def partner_counts(band, B):
    """int64 [n, B]: cnt_b(i)."""
    return np.stack([(band == b).sum(axis=1) for b in range(B)], axis=1).astype(np.int64)


def integers(xy, r2):
    """(W, S2c), int64 [B] each."""
    B = np.asarray(r2).reshape(-1).shape[0]
    cnt = partner_counts(bands(xy, r2), B)
    return cnt.sum(axis=0), (cnt * cnt).sum(axis=0)


def sums(xy, X, r2):
    """(W, S2c int64 [B]; N, Q fp64 [G, B]; AN, AQ fp64 [G, B]: the sums of the absolute values of N's and Q's terms, for the
    rounding bound of a comparison) of the centred values X fp64 [n, G] under the identity labeling."""
    X = np.asarray(X, dtype=np.float64)
    B = np.asarray(r2).reshape(-1).shape[0]
    band = bands(xy, r2)
    cnt = partner_counts(band, B)
    G = X.shape[1]
    N, Q, AN, AQ = (np.zeros((G, B)) for _ in range(4))
    for b in range(B):
        M = (band == b).astype(np.float64)
        N[:, b] = (X * (M @ X)).sum(axis=0)
        AN[:, b] = (np.abs(X) * (M @ np.abs(X))).sum(axis=0)
        Q[:, b] = (cnt[:, b].astype(np.float64)[:, None] * (X * X)).sum(axis=0)
        AQ[:, b] = Q[:, b]
    return cnt.sum(axis=0), (cnt * cnt).sum(axis=0), N, Q, AN, AQ


def shown(X, n_perms, seed, g, first=0, observed=True):
    """[L] -> the centred values every labeling shows: X itself (if observed), then X[pi_p] for p = first .. first + n_perms - 1."""
    X = np.asarray(X, dtype=np.float64)
    out = [X] if observed else []
    for p in range(first, first + n_perms):
        out.append(X[nhood_ref.perm(X.shape[0], seed, g, p)])
    return out


def all_sums(xy, X, r2, n_perms, seed, g, first=0, observed=True):
    """(W, S2c [B]; N, Q, AN, AQ [G, L, B]) over the labelings of `shown`."""
    per = [sums(xy, Xl, r2) for Xl in shown(X, n_perms, seed, g, first, observed)]
    return (per[0][0], per[0][1]) + tuple(np.stack([p[k] for p in per], axis=1) for k in (2, 3, 4, 5))


def direct_D(xy, X, r2):
    """fp64 [G, B]: sum over the ordered pairs of band b of (x_i - x_j)^2, term by term."""
    X = np.asarray(X, dtype=np.float64)
    B = np.asarray(r2).reshape(-1).shape[0]
    band = bands(xy, r2)
    D = np.zeros((X.shape[1], B))
    for b in range(B):
        i, j = np.nonzero(band == b)
        D[:, b] = ((X[i] - X[j]) ** 2).sum(axis=0)
    return D


def pair_graph(xy, r2_max):
    """(src, dst) int64: the directed graph of all ordered pairs i != j with d2 <= r2_max, by source then target."""
    d2 = cooccur_ref.d2_matrix(xy)
    ok = (d2 <= r2_max) & ~np.eye(d2.shape[0], dtype=bool)
    src, dst = np.nonzero(ok)
    return src.astype(np.int64), dst.astype(np.int64)


def tolerance(n, A):
    """The bound of a comparison of a device sum with the restatement: 4 n 2^-53 times the sum of the absolute values of its
    terms (a sequential sum of <= n terms per thread, then a tree over <= n threads and blocks: (n + log2 n) u to first order;
    the factor 4 covers the restatement's own rounding)."""
    return 4.0 * n * 2.0 ** -53 * np.asarray(A, dtype=np.float64)
