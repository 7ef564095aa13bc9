"""Inputs shared by tests/test_silhouette_cpu.py (the restatement against sklearn) and tests/test_silhouette_gpu.py (the kernel
against the restatement).  Every value is exactly representable in fp32, so the fp32 and the fp64 upload hold the same numbers."""
import numpy as np


def _points(rng, n, d, k=4):
    cen = 3.0 * rng.normal(size=(k, d))
    x = cen[rng.integers(0, k, n)] + rng.normal(size=(n, d))
    return x.astype(np.float32).astype(np.float64)


def _labelings(rng, n, same=()):
    """K = 2 (random), K = 3 (label 2 is a singleton), K = 5 (label 2 has no points); the rows `same` share a label."""
    l2 = rng.integers(0, 2, n)
    l3 = rng.integers(0, 2, n)
    l5 = rng.choice(np.array([0, 1, 3, 4]), n)
    for lab in (l2, l3, l5):
        if same:
            lab[list(same)] = lab[same[0]]
        lab[:4] = [0, 1, 0, 1]
    l3[n - 1] = 2
    l5[[8, 9, 10, 11]] = [0, 1, 3, 4]
    return [l2.astype(np.int64), l3.astype(np.int64), l5.astype(np.int64)]


def edge_call():
    """One call: two random sets of 37 and 300 points (d = 20) with three labelings each, a set whose points are all equal and
    a set of two point masses.  Returns (sets, labelings, random): random[t] says whether set t is a random one (its `nearest`
    is compared after the tie condition on the reference), the others are compared exactly."""
    rng = np.random.default_rng(20261)
    a, b = _points(rng, 37, 20), _points(rng, 300, 20)
    a[6] = a[5]
    a[7] = a[5]                                                      # three identical points, in one cluster
    # the two degenerate sets have small integer coordinates: sklearn forms distances as |x|^2 + |y|^2 - 2 x.y, which is exact
    # (0 between equal points) only where those products are; the definition's direct form is exact for any values
    equal = np.tile(np.round(_points(rng, 1, 20)), (40, 1))
    masses = np.round(_points(rng, 2, 20))[np.arange(40) % 2]
    lab_equal = [np.arange(40) % 2, np.arange(40) % 3, (np.arange(40) // 8)]
    lab_masses = [np.arange(40) % 2] * 3
    sets = [a, b, equal, masses]
    labelings = [_labelings(rng, 37, same=(5, 6, 7)), _labelings(rng, 300), [np.asarray(v, dtype=np.int64) for v in lab_equal],
                 [np.asarray(v, dtype=np.int64) for v in lab_masses]]
    return sets, labelings, [True, True, False, False]


# (name, n, d, K): n around the 256-point tile, cluster boundaries on and across tile edges, the smallest and the largest d and K
TILE_CASES = [("n255", 255, 20, 3), ("n256", 256, 20, 3), ("n257", 257, 20, 3), ("n770", 770, 20, 5),
              ("sizes_256_256_1", 513, 20, 3), ("k2", 513, 20, 2), ("k32", 513, 20, 32), ("d1", 513, 1, 4), ("d30", 513, 30, 4),
              ("d32", 513, 32, 4), ("d32_k32", 257, 32, 32)]


def tile_case(name):
    """(X [n, d] fp64, labels int64 [n]) of a TILE_CASES entry; the labels are not sorted, so the clusters' tiles mix rows."""
    i = [c[0] for c in TILE_CASES].index(name)
    _, n, d, K = TILE_CASES[i]
    rng = np.random.default_rng(977 + i)
    X = _points(rng, n, d, k=min(K, 6))
    if name == "sizes_256_256_1":
        lab = rng.permutation(np.repeat(np.array([0, 1, 2]), [256, 256, 1]))
    else:
        lab = rng.integers(0, K, n)
        lab[:K] = np.arange(K)                                        # every label value occurs: K is the largest label + 1
    return X, lab.astype(np.int64)
