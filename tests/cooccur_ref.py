"""The definition of the cooccurrence stage, restated in numpy: what csrc/cooccur.hip and spadot_amd.cooccurrence are
held to.  It forms the n x n matrix of squared distances, which the device never does.

    N[a, b, t] = #{ordered pairs (i, j), i != j : lab[i] = a, lab[j] = b, d2(i, j) <= r2[t]}
    d2 = dx * dx + dy * dy in fp64, as numpy evaluates it: two rounded products and one rounded sum, no fused multiply-add."""
import numpy as np


def d2_matrix(xy):
    """The unfused squared distances of all ordered pairs, fp64 [n, n]."""
    xy = np.asarray(xy, dtype=np.float64)
    dx = xy[:, 0][:, None] - xy[:, 0][None, :]
    dy = xy[:, 1][:, None] - xy[:, 1][None, :]
    return dx * dx + dy * dy


def counts(xy, lab, r2, K):
    """int64 [K, K, B] of one problem; r2: the squared thresholds."""
    lab = np.asarray(lab, dtype=np.int64)
    r2 = np.asarray(r2, dtype=np.float64).reshape(-1)
    n = lab.shape[0]
    d2 = d2_matrix(xy)
    other = ~np.eye(n, dtype=bool)                                  # a spot is never its own neighbour
    pair = lab[:, None] * K + lab[None, :]
    N = np.zeros((K, K, r2.shape[0]), dtype=np.int64)
    for t, r in enumerate(r2):
        N[:, :, t] = np.bincount(pair[(d2 <= r) & other], minlength=K * K).reshape(K, K)
    return N


def stats(N, ring=False):
    """cond [K, K, B], marg [K, B], ratio [K, K, B] in fp64 from the integers; ring: from the differences along t."""
    N = np.asarray(N, dtype=np.int64)
    if ring:
        N = np.concatenate([N[:, :, :1], N[:, :, 1:] - N[:, :, :-1]], axis=2)
    K, _, B = N.shape
    cond, marg, ratio = np.full((K, K, B), np.nan), np.full((K, B), np.nan), np.full((K, K, B), np.nan)
    for t in range(B):
        M = N[:, :, t]
        tot = int(M.sum())
        for b in range(K):
            if tot > 0:
                marg[b, t] = float(M[:, b].sum()) / float(tot)
        for a in range(K):
            row = int(M[a].sum())
            for b in range(K):
                if row > 0:
                    cond[a, b, t] = float(M[a, b]) / float(row)
                    if M[:, b].sum() > 0:
                        ratio[a, b, t] = cond[a, b, t] / marg[b, t]
    return dict(cond=cond, marg=marg, ratio=ratio)


def default_radii(xy, bins=50):
    xy = np.asarray(xy, dtype=np.float64)
    w, h = xy[:, 0].max() - xy[:, 0].min(), xy[:, 1].max() - xy[:, 1].min()
    return 0.25 * np.hypot(w, h) * np.arange(1, bins + 1) / bins
