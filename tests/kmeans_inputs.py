"""Inputs of the K-means kernel tests, shared by tests/test_kmeans_ref_cpu.py (which proves their preconditions on the host
reference) and tests/test_kmeans_kernels_gpu.py (which runs them on the device).  Everything comes from fixed seeds.

Two regimes.  LATTICE inputs have small-integer coordinates: every sum of both kernels is then exact in fp64 in any order, so
device and reference must agree bit for bit, ties included.  GENERAL inputs are Gaussian blobs; the CPU test asserts that on
them no decision of the reference (nearest centre, stopping test, seeding draw, best candidate) lies within 1e-9 of a tie,
which rounding (~1e-13) cannot bridge, so the GPU tests exclude nothing."""
import numpy as np

import kmeans_ref

F64 = np.float64
COND = 1e-9                      # the smallest relative margin a decision of a general input may have
LDS_DOUBLES = 7936               # (K_max + 256) * D <= 7936: the Lloyd launch's LDS rule


def blobs(rng, n, k, d, spread=3.0, noise=0.5):
    cen = spread * rng.normal(size=(k, d))
    return cen[rng.integers(0, k, n)] + noise * rng.normal(size=(n, d))


def tol_of(Xc, tol=1e-4):
    """sklearn's rule (and _Plan._seed's): tol * mean feature variance of the centred data."""
    return tol * float((Xc * Xc).sum() / Xc.size)


# ------------------------------------------------------------------------------------------------ Lloyd, general regime
#           name        seed   n     k   d  spread noise
GENERAL = (("separated", 101, 700, 10, 20, 3.0, 0.5),
           ("overlap", 102, 2300, 20, 20, 1.0, 1.0),
           ("d1", 103, 255, 2, 1, 3.0, 0.5),
           ("d2", 104, 1500, 6, 2, 2.0, 0.7),
           ("k32", 105, 1200, 32, 20, 2.0, 0.7),
           ("d30", 106, 513, 8, 30, 3.0, 0.5))
GENERAL_RESTARTS = 3


def general_case(name):
    """(Xc [n, d] centred blobs, tol, C0 [R, k, d] start centres = distinct random data rows)."""
    _, seed, n, k, d, spread, noise = next(c for c in GENERAL if c[0] == name)
    rng = np.random.default_rng(seed)
    X = blobs(rng, n, k, d, spread, noise)
    Xc = X - X.mean(0)
    C0 = np.stack([Xc[rng.choice(n, k, replace=False)] for _ in range(GENERAL_RESTARTS)])
    return Xc, tol_of(Xc), C0


# ------------------------------------------------------------------------------------------------ Lloyd, exact regime
LLOYD_NPTS = (1, 2, 255, 256, 257, 511, 513, 2300)
LLOYD_DIMS = (1, 2, 3, 20, 27, 30)
FAR = 40.0                       # a centre out there owns no point


def lattice_set(rng, n, d):
    """n points with integer coordinates in [-8, 8], drawn from a pool of n / 3 of them: many duplicates."""
    pool = rng.integers(-8, 9, size=(max(1, n // 3), d))
    return pool[rng.integers(0, pool.shape[0], n)].astype(F64)


def lattice_centres(rng, X, K):
    """Integer start centres: every other one a data row; C[1] = C[0] (the second must stay empty and keep its centre);
    C[2] far away (owns nothing); C[3], C[4] at distance 1 on either side of a data point (it is half-way: goes to 3)."""
    n, d = X.shape
    C = rng.integers(-8, 9, size=(K, d)).astype(F64)
    for j in range(0, K, 2):
        C[j] = X[rng.integers(n)]
    if K >= 2:
        C[1] = C[0]
    if K >= 3:
        C[2] = FAR
    if K >= 5:
        p = X[rng.integers(n)]
        C[3], C[4] = p.copy(), p.copy()
        C[3, 0] -= 1.0
        C[4, 0] += 1.0
    return C


def lloyd_k_max(d):
    return 32 if (32 + 256) * d <= LDS_DOUBLES else LDS_DOUBLES // d - 256


def lattice_lloyd(d):
    """One launch of the exact regime in d dimensions: (sets, restarts [(set index, C0 [Kr, d])], K_max).  Sets of LLOYD_NPTS
    points and one of 7 distinct points; 2 or 3 restarts (70 at least in all) per (set, Kr) with Kr in {1, 2, 7, 20, 32} up
    to K_max, and one with K = npts = 7 whose centres are the points themselves (inertia 0, done at once)."""
    rng = np.random.default_rng(1000 + d)
    K_max = lloyd_k_max(d)
    krs = [k for k in (1, 2, 7, 20, 32) if k <= K_max]
    if K_max not in krs:
        krs.append(K_max)
    sets = [lattice_set(rng, n, d) for n in LLOYD_NPTS]
    variants = 2 if 2 * len(sets) * len(krs) >= 70 else 3
    restarts = [(g, lattice_centres(rng, sets[g], k)) for _ in range(variants) for g in range(len(sets)) for k in krs]
    own = np.zeros((7, d))
    own[:, 0] = rng.permutation(np.arange(-8, 9))[:7]
    sets.append(own)
    restarts.append((len(sets) - 1, own.copy()))
    return sets, restarts, K_max


def exact_tols(sets, restarts):
    """A threshold per set that separates its restarts' reference shifts by a wide margin where they differ (the geometric
    mean of the two adjacent shifts furthest apart in ratio), else 0: `done` is then decided far from rounding."""
    tols = np.zeros(len(sets))
    for g in range(len(sets)):
        sh = sorted({kmeans_ref.lloyd_step(sets[g], C, 0.0)[3] for gg, C in restarts if gg == g})
        sh = [s for s in sh if s > 0]
        pairs = [(sh[i + 1] / sh[i], np.sqrt(sh[i] * sh[i + 1])) for i in range(len(sh) - 1)]
        if pairs and max(pairs)[0] > 1.001:
            tols[g] = max(pairs)[1]
    return tols


# ------------------------------------------------------------------------------------------------ seeding, exact regime
SEED_NPTS = (1, 2, 255, 256, 257, 1000, 50000)
SEED_KS = (1, 2, 3, 7, 8, 20, 21, 32)
SEED_DIMS = (1, 3, 20, 32)
BELOW_ONE = float(np.nextafter(1.0, 0.0))
MIRROR = np.array([-5.0, -3.0, -1.0, 0.0, 1.0, 3.0, 5.0])


def exact_prefix_draw(X, first):
    """(u, i): a draw whose product fl(u * pot) EQUALS the prefix sum of row i in round 1 from `first`, with row i weighing
    something (side left picks i; side right, or `>` in place of `>=`, the next row that weighs something)."""
    d0 = ((X - X[first]) ** 2).sum(1)
    cum, pot = np.cumsum(d0), d0.sum()
    for i in range(1, X.shape[0] - 1):
        if d0[i] > 0 and cum[-1] > cum[i]:
            for u in (cum[i] / pot, np.nextafter(cum[i] / pot, 0.0), np.nextafter(cum[i] / pot, 1.0)):
                if u * pot == cum[i]:
                    return float(u), i
    raise AssertionError("no exact prefix draw")


def lattice_seeding(d):
    """(sets, problems [dict(g, k, first, U [(k - 1) * trials], tag)]) of the exact regime in d dimensions: every k of
    SEED_KS that fits on sets of SEED_NPTS lattice points (the 50 000-point set with k = 3 and 21 only), a set of identical
    points, a mirror-symmetric set, and the hand-made draws."""
    rng = np.random.default_rng(2000 + d)
    sets = [lattice_set(rng, n, d) for n in SEED_NPTS]
    probs = []
    rand = lambda g, k, tag="random": dict(g=g, k=k, first=int(rng.integers(sets[g].shape[0])),
                                           U=rng.uniform(size=(k - 1) * kmeans_ref.trials_of(k)), tag=tag)
    for g, n in enumerate(SEED_NPTS):
        for k in SEED_KS:
            if k <= n and (n < 50000 or k in (3, 21)):
                probs.append(rand(g, k))
    g1000 = SEED_NPTS.index(1000)
    for k, u, tag in ((7, 0.0, "u=0"), (8, BELOW_ONE, "below one"), (21, 1.5, "past the last prefix")):
        p = rand(g1000, k, tag)
        p["U"][::3] = u
        p["U"][:kmeans_ref.trials_of(k)] = u                          # round 1: every candidate from this draw
        probs.append(p)
    p = rand(g1000, 3, "exact prefix")
    p["U"][0], p["row"] = exact_prefix_draw(sets[g1000], p["first"])
    probs.append(p)
    sets.append(np.repeat(sets[0][:1], 300, axis=0))                 # identical points: pot = 0 from round 1 on
    probs.append(rand(len(sets) - 1, 7, "zero potential"))
    mirror = np.zeros((7, d))
    mirror[:, 0] = MIRROR
    sets.append(mirror)
    # from the middle point the closest distances are 25 9 1 0 1 9 25 (prefix 25 34 35 35 36 45 70): 40 / 70 draws row 5
    # (+3), 30 / 70 row 1 (-3); their potentials tie by symmetry and the FIRST candidate (row 5) wins
    probs.append(dict(g=len(sets) - 1, k=2, first=3, U=np.array([40.0 / 70.0, 30.0 / 70.0]), tag="mirror tie"))
    return sets, probs


def invalid_seeding():
    """(sets, n_max, K_max, problems): valid problems with invalid ones between them (k = 0, k > K_max, first >= n,
    first < 0, a set larger than n_max); `valid` says which."""
    rng = np.random.default_rng(2500)
    sets = [lattice_set(rng, 1000, 3), lattice_set(rng, 1001, 3)]
    mk = lambda g, k, first, valid: dict(g=g, k=k, first=first, valid=valid,
                                         U=rng.uniform(size=max(k - 1, 0) * kmeans_ref.trials_of(max(k, 1))))
    probs = [mk(0, 7, 5, True), mk(0, 0, 5, False), mk(0, 20, 999, True), mk(0, 21, 5, False), mk(0, 3, 1000, False),
             mk(0, 3, 0, True), mk(0, 3, -1, False), mk(1, 3, 5, False), mk(0, 8, 77, True)]
    return sets, 1000, 20, probs


# ------------------------------------------------------------------------------------------------ seeding, general regime
SEED_GENERAL_N = (3, 40, 255, 256, 700, 2300)
SEED_GENERAL_R = 2


def seed_general_ks(n):
    if n == 3:
        return (2, 3)
    return tuple(range(4, 33)) if n in (40, 700) else (4, 7, 8, 20, 21, 32)


def seed_general_sets():
    rng = np.random.default_rng(3000)
    # (the small sets are one blob: two points alone in a blob tie as candidates, whichever enters first leaves the same potential)
    Xs = [blobs(rng, n, 10 if n > 40 else 1, 20) for n in SEED_GENERAL_N]
    return [x - x.mean(0) for x in Xs]


def seed_general_problems(sets):
    """[dict(g, k, first, U)]: the draws of KMeans(k, random_state=1993, n_init=R) for every set and k."""
    from spadot_amd.kmeans import sweep_draws
    probs = []
    for g, x in enumerate(sets):
        for k in seed_general_ks(x.shape[0]):
            first, U = sweep_draws(x.shape[0], k, 1993, SEED_GENERAL_R)
            probs += [dict(g=g, k=k, first=int(first[r]), U=U[r]) for r in range(SEED_GENERAL_R)]
    return probs


# ------------------------------------------------------------------------------------------------ the whole fit
FIT_SIZES = (300, 700, 1201)
FIT_KS = (1, 5, 10, 20, 32)
FIT_RESTARTS = 4
FIT_SEED = 1993


def fit_sets():
    """Three ragged sets of blobs in 20 dimensions, away from the origin (the driver centres them)."""
    rng = np.random.default_rng(4000)
    return [blobs(rng, n, 10, 20) + 5.0 for n in FIT_SIZES]


# ------------------------------------------------------------------------------------------------ spadot_kmeans_assign
ASSIGN_N, ASSIGN_K, ASSIGN_D = (1, 255, 256, 257), (1, 2, 32, 64), (1, 20, 64)
ASSIGN_LARGE = ((10000, 1, 1), (10000, 2, 20), (10000, 32, 64), (10000, 64, 20))
ASSIGN_GAP32 = 1e-6


def assign_shapes():
    return [(n, k, d) for n in ASSIGN_N for k in ASSIGN_K for d in ASSIGN_D] + list(ASSIGN_LARGE)


def assign_case(n, k, d, lattice):
    """(X [n, d], C [k, d]) fp64: lattice points and centres (duplicate centres, exact ties) or blobs and centres near them."""
    rng = np.random.default_rng(5000 + 7 * n + 131 * k + 17 * d + lattice)
    if lattice:
        X = lattice_set(rng, n, d)
        C = rng.integers(-8, 9, size=(k, d)).astype(F64)
        if k >= 2:
            C[k - 1] = C[0]
        return X, C
    X = blobs(rng, n, min(k, 10), d)
    return X, X[rng.integers(0, n, k)] + 0.3 * rng.normal(size=(k, d))
