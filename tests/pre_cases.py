"""Inputs of the preprocess / SCTransform edge tests (CPU and GPU): small crafted counts that reach the paths of
csrc/preprocess.hip and csrc/sctransform.hip which the synthetic data of the stage tests never reaches.

    segments()         202 spots x 24 genes in three time points of 70, 1 and 131 spots: column segments of 0, 1, 5, 63, 64, 65,
                       N-1 and N nonzeros, zero-total spots at both ends and at a time-point boundary, rows interleaved
    tiny()             7 + 3 spots: a time point that keeps 5 spots
    fit()              40 genes of negative-binomial / Poisson counts over 150 and 40 kept spots
    resid_tiles()      three time points that keep 4096, 4097 and 8193 spots: one, two and three tiles of k_sct_resid_write
    scale_tiles(S)     6 spots x (S + 7) genes, S = 15360, 15361, 30721: one, two and three tiles of k_pre_scale_write
    pvalue_rows()      crafted moments, one row per branch of k_sparkx_pvals

Every builder returns a Case: the counts in INPUT row order (scipy CSR float32), the time point label and coordinates of every
input row, and, for the checks, B (the same counts as fp64 CSR in the device's row order: time point blocks in order of first
appearance, input order inside a block), perm (the input row of each device row), tp_off, and `facts`, what the case is
meant to have (tests/test_preprocess_edges_cpu.py checks the counts against them).  Values are integer counts."""
import functools
import types

import numpy as np
import scipy.sparse as sp

PRE_TILE = 15360               # csrc/preprocess.hip
SCT_TILE = 4096                # csrc/sctransform.hip
WAVE = 64


def tile_rule(n, tile):
    """The host rule of both tiled writers: equal tiles, each at most `tile` wide.  Returns (ntile, width)."""
    ntile = -(-n // tile)
    return ntile, -(-n // ntile)


def _interleave(sizes):
    """Block rows in an input order that takes the time points in turn: the order inside a time point is kept, the first
    appearances are in block order, and the rows of a time point are not contiguous."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    nxt = [0] * len(sizes)
    out = []
    while len(out) < off[-1]:
        for t, s in enumerate(sizes):
            if nxt[t] < s:
                out.append(off[t] + nxt[t])
                nxt[t] += 1
    return np.asarray(out, dtype=np.int64)


def _case(B, sizes, labels, rng, interleave=True, **facts):
    """A Case from the block-ordered dense or sparse counts B."""
    B = sp.csr_matrix(B, dtype=np.float64)
    B.eliminate_zeros()
    B.sort_indices()
    n = B.shape[0]
    assert n == sum(sizes)
    rows = _interleave(sizes) if interleave else np.arange(n)      # block row of each input row
    tp_block = np.repeat(np.asarray(labels), sizes)
    spatial_block = rng.uniform(0.0, 100.0, (n, 2))
    return types.SimpleNamespace(X=sp.csr_matrix(B[rows], dtype=np.float32), timepoint=tp_block[rows], spatial=spatial_block[rows],
                                 B=B, perm=np.argsort(rows), tp_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                                 labels=list(labels), sizes=tuple(sizes), spatial_block=spatial_block, facts=facts)


def raw_counts(case):
    """The case as the stage reads it (spadot_amd's RawCounts)."""
    from spadot_amd.utils._preprocess_utils import RawCounts
    names = np.array([f"g{j}" for j in range(case.X.shape[1])])
    return RawCounts(case.X, case.timepoint, case.spatial, names)


def kept_rows(case, t, cols=None):
    """The device rows of time point t with a non-zero total over the columns `cols` (all when None)."""
    lo, hi = int(case.tp_off[t]), int(case.tp_off[t + 1])
    M = case.B[lo:hi] if cols is None else case.B[lo:hi][:, cols]
    return lo + np.flatnonzero(np.asarray(M.sum(1)).ravel() > 0)


def _counts(rng, size, big=0.1):
    """Integer counts >= 1: mostly below 20, a share `big` of them between 1000 and 60000."""
    v = rng.integers(1, 20, size).astype(np.float64)
    b = rng.uniform(size=size) < big
    v[b] = rng.integers(1000, 60001, int(b.sum()))
    return v


# ---------------------------------------------------------------- segments
SEG_SIZES = (70, 1, 131)
SEG_G = 24
SEG_ZERO_ROWS = (0, 69, 71, 201)      # device rows: first of time point 0, both sides of the boundaries 70 | 71, last of 2
SEG_KEPT = (68, 1, 129)
SEG_CONSTANT = (10, 2, 3.0)           # gene 10 is 3 at every kept spot of time point 2
SEG_MIDDLE_ONLY = 9
SEG_ALL_ZERO = 1
SEG_COLS = (23, 0, 7, 1, 10, 5, 2, 9, 14, 3, 8, 12)       # a non-monotone subset: the columns of the scaling checks
# nonzeros per (time point, gene) of genes 0 .. 10 and 23; genes 11 .. 22 are random
SEG_NNZ = {0: (68, 1, 0), 1: (0, 0, 0), 2: (1, 0, 1), 3: (5, 0, 5), 4: (63, 0, 63), 5: (64, 1, 64), 6: (65, 0, 65),
           7: (67, 0, 128), 8: (68, 1, 129), 9: (0, 1, 0), 10: (5, 0, 129), 23: (0, 1, 65)}


@functools.lru_cache(maxsize=None)
def segments():
    rng = np.random.default_rng(5)
    n = sum(SEG_SIZES)
    off = np.concatenate([[0], np.cumsum(SEG_SIZES)])
    D = np.zeros((n, SEG_G))
    kept = [np.setdiff1d(np.arange(off[t], off[t + 1]), SEG_ZERO_ROWS) for t in range(3)]
    assert tuple(k.size for k in kept) == SEG_KEPT
    nnz = dict(SEG_NNZ)
    for g in range(11, 23):
        nnz[g] = tuple(int(rng.integers(2, k.size)) if k.size > 1 else int(rng.integers(0, 2)) for k in kept)
    for g, per in nnz.items():
        for t, c in enumerate(per):
            K = kept[t]
            if c == 1:
                rows = K[-1:] if t == 2 else K[:1]                 # the very first / last kept row of the time point
            elif c == 5:
                rows = np.concatenate([K[:1], K[-1:], rng.choice(K[1:-1], 3, replace=False)])
            else:
                rows = rng.choice(K, c, replace=False)
            D[rows, g] = _counts(rng, c)
    g, t, v = SEG_CONSTANT
    D[kept[t], g] = v
    D[kept[0][np.flatnonzero(D[kept[0], 4])[0]], 4] = 1.0          # both ends of the value range are present
    D[kept[2][np.flatnonzero(D[kept[2], 6])[0]], 6] = 60000.0
    return _case(D, SEG_SIZES, ("b", "a", "c"), rng, nnz=nnz, zero_rows=SEG_ZERO_ROWS, kept=SEG_KEPT)


@functools.lru_cache(maxsize=None)
def tiny():
    """Two time points of 7 and 3 spots, 6 genes; time point 0 keeps 5 spots (rows 1 and 6 are zero)."""
    rng = np.random.default_rng(6)
    D = np.zeros((10, 6))
    D[np.ix_([0, 2, 3, 4, 5], [0, 2, 5])] = _counts(rng, (5, 3), big=0.0)
    D[[0, 4], 1] = (7.0, 2.0)
    D[3, 3] = 41.0                                                 # gene 4 stays empty
    D[7:, :] = _counts(rng, (3, 6), big=0.0) * (rng.uniform(size=(3, 6)) < 0.6)
    D[[7, 8, 9], [0, 1, 5]] = (1.0, 2.0, 3.0)
    return _case(D, (7, 3), ("x", "y"), rng, zero_rows=(1, 6), kept=(5, 3))


# ---------------------------------------------------------------- fit
FIT_SIZES = (151, 41)
FIT_KEPT = (150, 40)                  # 40: fewer than one wavefront
FIT_G = 40
FIT_ZERO_ROWS = (75, 151 + 20)
FIT_POISSON = (38, 39)


@functools.lru_cache(maxsize=None)
def fit():
    """Negative-binomial counts y ~ NB(mean m_g s_j, theta_g) with planted theta in [0.5, 50], m_g in [0.3, 30] and a
    log-normal spot depth s_j; the last two genes are Poisson.  One spot per time point has no counts."""
    rng = np.random.default_rng(9)
    n = sum(FIT_SIZES)
    depth = np.exp(rng.normal(0.0, 0.5, n))
    m = rng.permutation(np.geomspace(0.3, 30.0, FIT_G))
    theta = rng.permutation(np.geomspace(0.5, 50.0, FIT_G))
    mu = depth[:, None] * m[None, :]
    lam = rng.gamma(theta[None, :], mu / theta[None, :])
    lam[:, FIT_POISSON] = mu[:, FIT_POISSON]
    D = rng.poisson(lam).astype(np.float64)
    D[list(FIT_ZERO_ROWS)] = 0.0
    return _case(D, FIT_SIZES, ("late", "early"), rng, zero_rows=FIT_ZERO_ROWS, kept=FIT_KEPT, theta=theta)


# ---------------------------------------------------------------- tiles of k_sct_resid_write
RT_KEPT = (4096, 4097, 8193)          # one full tile, two tiles of 2049, three tiles of 2731
RT_GENES = ("boundary", "no_middle", "last_only", "dense")
RT_THETA = (1e8, 0.05, 2.0, 10.0)
RT_SLOPE = (1.0, 0.9, 1.1, 1.0)       # in units of ln 10: mu ~ umi ** slope
RT_CENTER = (0.0, -0.01, 0.1, -0.3)


def _rt_block(rng, N):
    """Counts of one time point that keeps N spots, and the kept position before which each zero-total row stands."""
    ntile, w = tile_rule(N, SCT_TILE)
    before = {0}                                                   # a zero-total row opens the time point
    for j in range(1, ntile):
        before |= {j * w - 1, j * w, j * w + 1}                    # inside the left tile, on the boundary, inside the right
    before |= set(rng.choice(np.arange(2, N - 2), 8, replace=False).tolist())
    before = np.asarray(sorted(before))
    krow = np.arange(N) + np.searchsorted(before, np.arange(N), side="right")
    n = int(krow[-1]) + 2                                          # and one closes it
    Y = np.zeros((N, 4))
    edge = sorted({0, N - 1} | {j * w - 1 for j in range(1, ntile)} | {j * w for j in range(1, ntile)})
    Y[edge, 0] = rng.integers(1, 30, len(edge))
    tile_of = np.arange(N) // w
    mid = ntile // 2 if ntile > 1 else -1                          # two tiles: the second one counts as the middle
    Y[:, 1] = rng.integers(1, 30, N) * (rng.uniform(size=N) < 0.3) * (tile_of != mid)
    Y[:, 2] = rng.integers(1, 30, N) * (rng.uniform(size=N) < 0.5) * (tile_of == ntile - 1)
    Y[:, 3] = rng.integers(1, 50, N)
    D = np.zeros((n, 4))
    D[krow] = Y
    return D, before


@functools.lru_cache(maxsize=None)
def resid_tiles():
    rng = np.random.default_rng(12)
    blocks, befores = zip(*[_rt_block(rng, N) for N in RT_KEPT])
    sizes = tuple(b.shape[0] for b in blocks)
    return _case(np.concatenate(blocks), sizes, ("t0", "t1", "t2"), rng, kept=RT_KEPT, zero_before=befores)


def model_pars(case, t, theta, slope):
    """Given (theta, b0, b1) rows [G, 3] for the genes of time point t: b1 = slope ln 10 (mu ~ umi ** slope) and b0 so that
    sum mu = sum y + 1 (finite for an empty gene too)."""
    rows = kept_rows(case, t)
    umi = np.asarray(case.B[rows].sum(1)).ravel()
    sy = np.asarray(case.B[rows].sum(0)).ravel()
    theta, slope = np.asarray(theta, dtype=np.float64), np.asarray(slope, dtype=np.float64)
    b0 = np.log((sy + 1.0) / np.power(umi[:, None], slope[None, :]).sum(0))
    return np.stack([theta, b0, slope * np.log(10.0)], axis=1)


def rt_pars(case, t):
    """The parameters [4, 3] and centres [4] of time point t of resid_tiles()."""
    return model_pars(case, t, RT_THETA, RT_SLOPE), np.asarray(RT_CENTER)


def cycled_pars(case, t):
    """Parameters and centres for every gene of a small case: theta cycles through 1e8, 0.05, 2, 10, 0.7, the slope through
    0.8 .. 1.2, the centres through a few values of either sign."""
    G = case.B.shape[1]
    g = np.arange(G)
    theta = np.asarray([1e8, 0.05, 2.0, 10.0, 0.7])[g % 5]
    slope = np.asarray([1.0, 0.8, 1.2])[g % 3]
    return model_pars(case, t, theta, slope), np.asarray([0.0, -0.01, 0.1, -0.3])[g % 4]


# ---------------------------------------------------------------- tiles of k_pre_scale_write
ST_S = (PRE_TILE, PRE_TILE + 1, 2 * PRE_TILE + 1)      # one tile (the largest LDS request), two of 7681, three of 10241
ST_EXTRA = 7
ST_SIZES = (3, 3)
ST_EMPTY_ROW, ST_ZERO_TOTAL_ROW = 1, 3


def st_edges(S):
    """The output columns at the tile edges."""
    ntile, w = tile_rule(S, PRE_TILE)
    return sorted({j for j in (0, w - 1, w, 2 * w - 1, 2 * w, S - 1) if j < S})


@functools.lru_cache(maxsize=None)
def scale_tiles(S):
    """6 spots in two time points over G = S + 7 genes; `cols` (in facts) selects S of them in a shuffled order.  Rows 0, 2,
    4 and 5 have nonzeros at every tile-edge output column and at about 300 others, row 1 has none, row 3 only at the genes
    outside cols (its total over cols is zero)."""
    rng = np.random.default_rng(S)
    G = S + ST_EXTRA
    order = rng.permutation(G)
    cols, rest = order[:S], order[S:]
    D = sp.lil_matrix((6, G))
    for r in (0, 2, 4, 5):
        j = np.union1d(st_edges(S), rng.choice(S, 300, replace=False))
        D[r, cols[j]] = rng.integers(1, 100, j.size)
        D[r, rest[:3]] = (5.0, 1.0, 9.0)
    D[ST_ZERO_TOTAL_ROW, rest] = rng.integers(1, 100, rest.size)
    return _case(D, ST_SIZES, (0, 1), rng, interleave=False, cols=cols, zero_rows=(ST_EMPTY_ROW,), kept=(2, 3))


# ---------------------------------------------------------------- p-values
PV_N = 1000
PV_LAM = np.array([[[1.0, 1.0], [2.0, 0.5], [1.3, 0.9], [0.5, 2.0], [3.0, 1.0], [1.0, 0.25], [0.8, 0.8], [1.5, 1.2], [0.6, 1.1],
                    [2.5, 0.4], [1.0, 4.0]], [[1.0, 1.0]] * 11])     # time point 0: unequal weights; 1: unit weights
PV_ROWS = ("ylam_zero", "all_zero", "q_zero", "equal_weights", "underflow", "zero_and_one", "one_small_cct", "one_small_atan",
           "three_small", "all_small", "small_among_unequal", "one_only") + ("ordinary",) * 8


@functools.lru_cache(maxsize=None)
def pvalue_rows():
    """mom [P, 24], pair_t [P], the row names, for nkeep = (PV_N, PV_N), inv = identity and lam = PV_LAM.  With sum y^2 = n the
    statistic of kernel k is q = e1^2 + e2^2 of its two moments."""
    rng = np.random.default_rng(3)
    P = len(PV_ROWS)
    mom = np.zeros((P, 24))
    pt = np.zeros(P, dtype=np.int32)

    def put(i, q, t, sy=0.0):
        q = np.asarray(q, dtype=np.float64)
        a = rng.uniform(0.0, 2 * np.pi, 11)
        mom[i, 0], mom[i, 1], pt[i] = sy, PV_N, t
        mom[i, 2::2], mom[i, 3::2] = np.sqrt(q) * np.cos(a), np.sqrt(q) * np.sin(a)

    ordinary = lambda: rng.uniform(0.5, 9.0, 11)
    for i, name in enumerate(PV_ROWS):
        if name == "ylam_zero":                    # a constant count of 3 in all n spots: n ybar^2 / sum y^2 == 1 exactly
            put(i, ordinary(), 0)
            mom[i, 0], mom[i, 1] = 3.0 * PV_N, 9.0 * PV_N
        elif name == "all_zero":
            pt[i] = 1
        elif name == "q_zero":
            put(i, np.zeros(11), 0, sy=5.0)
        elif name == "equal_weights":
            put(i, ordinary(), 1, sy=17.0)
        elif name == "underflow":
            put(i, np.full(11, 2000.0), 1)
        elif name == "zero_and_one":
            put(i, np.concatenate([[1e4, 0.0], ordinary()[2:]]), 1)
        elif name == "one_small_cct":              # p = exp(-40) = 4e-18: 1 / (11 pi p) > 1e15
            put(i, np.concatenate([ordinary()[:4], [80.0], ordinary()[5:]]), 1)
        elif name == "one_small_atan":             # p = exp(-37.5) = 5e-17 < 1e-16, 1 / (11 pi p) = 5.6e14 < 1e15
            put(i, np.concatenate([[75.0], ordinary()[1:]]), 1)
        elif name == "three_small":
            put(i, np.concatenate([[80.0], ordinary()[1:5], [200.0], ordinary()[6:10], [600.0]]), 1)
        elif name == "all_small":
            put(i, np.linspace(80.0, 600.0, 11), 1)
        elif name == "small_among_unequal":        # kernel 0 of time point 0 has equal weights
            put(i, np.concatenate([[80.0], ordinary()[1:]]), 0, sy=12.0)
        elif name == "one_only":
            put(i, np.concatenate([ordinary()[:7], [0.0], ordinary()[8:]]), 0, sy=3.0)
        else:
            put(i, ordinary(), 0, sy=float(rng.uniform(0.0, 40.0)))
    return mom, pt, PV_ROWS
