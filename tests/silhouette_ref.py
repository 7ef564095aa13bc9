"""The silhouette coefficient's definition (spadot_amd/silhouette.py) restated in numpy fp64 with a full distance
matrix, which is fine at test sizes.  Pinned to sklearn.metrics.silhouette_samples by tests/test_silhouette_cpu.py; the device
kernel is compared with this restatement on the same values."""
import numpy as np


def silhouette(X, labels, K=None):
    """X [n, d] (converted to fp64), labels in 0 .. K-1 (K: default the largest label + 1).  Returns a dict: a, b, samples (fp64
    [n]), nearest (int32 [n], -1 where no other non-empty cluster exists), sizes (int64 [K]), means ([n, K]: S_i(k) / n_k, inf
    for the own and the empty clusters) and score (NaN unless 2 <= non-empty clusters <= n - 1)."""
    X = np.asarray(X, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    n = X.shape[0]
    K = int(lab.max()) + 1 if K is None else int(K)
    diff = X[:, None, :] - X[None, :, :]
    D = np.sqrt((diff * diff).sum(-1))                                  # the direct form
    sizes = np.bincount(lab, minlength=K).astype(np.int64)
    S = np.stack([D[:, lab == k].sum(1) for k in range(K)], axis=1)     # [n, K]
    own = sizes[lab]
    a = np.where(own > 1, S[np.arange(n), lab] / np.maximum(own - 1, 1), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = np.where(sizes[None, :] > 0, S / sizes[None, :], np.inf)
    means[np.arange(n), lab] = np.inf
    nearest = means.argmin(1).astype(np.int32)                          # first minimum
    b = means[np.arange(n), nearest]
    nearest[np.isinf(b)] = -1
    m = np.maximum(a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(m > 0, (b - a) / m, 0.0)
    s[own == 1] = 0.0
    nonempty = int((sizes > 0).sum())
    score = float(np.mean(s)) if 2 <= nonempty <= n - 1 else float("nan")
    return dict(a=a, b=b, samples=s, nearest=nearest, sizes=sizes, means=means, score=score)


def min_gap(means):
    """Per row, the relative gap between the smallest and the second-smallest finite cluster mean (inf with fewer than two):
    how far the choice of `nearest` is from a tie."""
    srt = np.sort(means, axis=1)
    if srt.shape[1] < 2:
        return np.full(srt.shape[0], np.inf)
    lo, hi = srt[:, 0], srt[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(np.isfinite(hi), (hi - lo) / np.maximum(hi, np.finfo(np.float64).tiny), np.inf)
    return gap
