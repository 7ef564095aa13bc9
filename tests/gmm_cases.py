"""Inputs shared by tests/test_gmm_cpu.py (the restatement against sklearn) and tests/test_gmm_gpu.py (the kernels against the
restatement).  Every value is exactly representable in fp32, so the fp32 and the fp64 upload hold the same numbers."""
import numpy as np


def blobs(rng, n, d, k, spread=3.0, noise=1.0):
    cen = spread * rng.normal(size=(k, d))
    which = rng.integers(0, k, n)
    x = cen[which] + noise * rng.normal(size=(n, d))
    return x.astype(np.float32).astype(np.float64), which


def nearest_labels(X, K, rng):
    """The labels a K-means start would give: nearest of K data points drawn without replacement (first minimum)."""
    c = X[rng.choice(X.shape[0], K, replace=False)]
    d2 = ((X[:, None, :] - c[None, :, :]) ** 2).sum(2)
    return np.argmin(d2, axis=1).astype(np.int64)


def edge_call():
    """One call: sets of 37 and 300 points in d = 3 with three labelings each (the sets of a call share d; 300 x 20 with a
    component of fewer than d + 1 points is the fit case `few_d20`).  Returns (sets, labelings, Ks).
    Set 0: rows 5, 6, 7 are identical; labeling 1 has a component of one point (label 2 = the last row); labeling 2 has K = 5
    with a label value (2) that no point carries.  Set 1: labeling 1 has a component of 3 < d + 1 points."""
    rng = np.random.default_rng(20271)
    a, _ = blobs(rng, 37, 3, 2)
    a[6] = a[5]
    a[7] = a[5]
    b, _ = blobs(rng, 300, 3, 4)
    la0 = nearest_labels(a, 2, rng)
    la1 = la0.copy()
    la1[36] = 2
    la2 = np.array([0, 1, 3, 4])[nearest_labels(a, 4, rng)]
    for lab in (la0, la1, la2):
        lab[6] = lab[7] = lab[5]
    lb0 = nearest_labels(b, 2, rng)
    lb1 = lb0.copy()
    lb1[[3, 120, 299]] = 2
    lb2 = nearest_labels(b, 4, rng)
    return [a, b], [[la0, la1, la2], [lb0, lb1, lb2]], [[2, 3, 5], [2, 3, 4]]


# (name, n, d, K, blobs in the data, spread): n around the 256-point block, the smallest and the largest d and K, the largest
# parameter block (d = 20, K = 32), an overlapping set that takes about 50 iterations and a separated one that stops at 2
FIT_CASES = [("n255", 255, 20, 3, 3, 3.0), ("n256", 256, 20, 3, 3, 3.0), ("n257", 257, 20, 3, 3, 3.0),
             ("n770", 770, 20, 4, 4, 3.0),
             ("d1", 513, 1, 3, 3, 3.0), ("d3", 513, 3, 4, 4, 3.0), ("d19", 513, 19, 3, 3, 3.0),
             ("k1", 300, 20, 1, 3, 3.0), ("k2", 513, 20, 2, 4, 3.0), ("k20", 1100, 20, 20, 20, 3.0), ("k32_d3", 770, 3, 32, 8, 3.0),
             ("k32_d20", 1500, 20, 32, 32, 3.0), ("slow", 770, 20, 7, 7, 1.2), ("fast", 513, 20, 4, 4, 4.0),
             ("few_d20", 300, 20, 3, 4, 3.0)]
CAPPED = ("slow", 10)        # the overlapping set again with max_iter = 10: a fit that ends without converging


def fit_case(name):
    """(X [n, d] fp64, labels int64 [n], K) of a FIT_CASES entry.  `fast` starts from the planted labels, the others from the
    nearest of K drawn points; `few_d20` from the nearest of 2 with five rows moved to a third component (fewer than d + 1)."""
    i = [c[0] for c in FIT_CASES].index(name)
    _, n, d, K, kb, spread = FIT_CASES[i]
    rng = np.random.default_rng(1977 + i)
    X, which = blobs(rng, n, d, kb, spread=spread)
    if name == "few_d20":
        lab = nearest_labels(X, 2, rng)
        lab[[3, 50, 120, 200, 299]] = 2
    else:
        lab = which.astype(np.int64) if name == "fast" else nearest_labels(X, K, rng)
    return X, lab, K


def planted(counts=(1500, 2000, 2500), k0s=(5, 6, 7)):
    """Three time points of planted blobs, d = 20: centres normal * 4, unit noise (the silhouette test's sets, with more spots:
    at 500 .. 700 spots the 210 covariance parameters per component make BIC prefer k = 4)."""
    rng = np.random.default_rng(1993)
    X, truth = [], []
    for n, k0 in zip(counts, k0s):
        cen = rng.normal(size=(k0, 20)) * 4
        which = rng.integers(0, k0, n)
        X.append((cen[which] + rng.normal(size=(n, 20))).astype(np.float32))
        truth.append(which)
    return X, truth


def write_latent(path, X, seed=3):
    """latent.npz as train writes it, the rows numbered 0 .. N-1 (what trends.read_lineage matches memberships.npz against)."""
    rng = np.random.default_rng(seed)
    n = sum(x.shape[0] for x in X)
    tp = np.repeat(np.array(["E1", "E2", "E3"]), [x.shape[0] for x in X])
    rows = np.arange(n)
    np.savez_compressed(path, X=np.concatenate(X), rows=rows, timepoint=tp, spatial=rng.uniform(0, 100, size=(n, 2)))
    return tp, rows
