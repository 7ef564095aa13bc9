"""Inputs of the co-occurrence tests (CPU and GPU): the edge call, the sets that straddle the 256-wide tile, the integer lattice,
the on-threshold set, the planted domains of nhood_cases, and the restatement's counts of each, computed once per process."""
import functools
from fractions import Fraction

import numpy as np

import cooccur_ref as ref
import nhood_cases


def _readonly(a):
    a.setflags(write=False)
    return a


def _thresholds(rng, B, r_max):
    """B strictly increasing squared thresholds up to r_max^2."""
    return np.sort(rng.uniform(0.0, r_max, B)) ** 2


@functools.lru_cache(maxsize=None)
def edge_call():
    """[(xy, labels, r2, K)]: n = 1 (B = 1); two coincident spots with a threshold 0 (B = 16); n = 37 with K = 3 and the label
    value 1 without spots (B = 17); n = 300 with K = 32 (B = 64)."""
    rng = np.random.default_rng(21)
    out = [(np.array([[3.5, -2.0]]), np.zeros(1, np.int64), np.array([4.0]), 1)]
    r2 = np.concatenate([[0.0], _thresholds(rng, 15, 2.0) + 0.01])
    out.append((np.array([[1.25, 7.5], [1.25, 7.5]]), np.array([0, 1]), r2, 2))
    lab = rng.integers(0, 2, 37) * 2
    assert set(lab) == {0, 2}
    out.append((rng.uniform(0, 10, (37, 2)), lab, _thresholds(rng, 17, 8.0), 3))
    lab = rng.permutation(300) % 32
    out.append((rng.uniform(0, 30, (300, 2)), lab, _thresholds(rng, 64, 20.0), 32))
    assert all(np.all(np.diff(c[2]) > 0) for c in out)
    return out


TILE_SIZES = (255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def tile_case(n):
    """(xy, labels, r2, K = 5) with B = 7: n straddles the 256 sorted positions of a workgroup and of a tile."""
    rng = np.random.default_rng(1000 + n)
    return rng.uniform(0, 25, (n, 2)), rng.integers(0, 5, n), _thresholds(rng, 7, 12.0), 5


@functools.lru_cache(maxsize=None)
def lattice():
    """The 12 x 12 integer lattice with K = 3: every squared distance is an integer, every pair exactly on or off a threshold."""
    xy = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0)), -1).reshape(-1, 2)
    lab = np.random.default_rng(4).integers(0, 3, 144)
    return xy, lab, np.array([0.0, 1.0, 2.0, 4.0, 5.0, 25.0]), 3


@functools.lru_cache(maxsize=None)
def on_threshold():
    """(xy, labels, r2, K = 4, pairs): a 17 x 17 grid of spacing 10 with jitter +-3 and 64 thresholds taken from the set's own
    unfused squared distances, at evenly spaced ranks between 2 % and 50 % of the distinct values.  pairs[t] = (i, j): a pair
    that lies exactly on threshold t."""
    rng = np.random.default_rng(11)
    xy = 10.0 * np.stack(np.meshgrid(np.arange(17.0), np.arange(17.0)), -1).reshape(-1, 2) + rng.uniform(-3, 3, (289, 2))
    lab = rng.integers(0, 4, 289)
    d2 = ref.d2_matrix(xy)
    iu = np.triu_indices(289, 1)
    vals, first = np.unique(d2[iu], return_index=True)
    ranks = np.round(np.linspace(0.02, 0.5, 64) * (vals.shape[0] - 1)).astype(np.int64)
    assert np.all(np.diff(ranks) > 0)
    pairs = [(int(iu[0][first[r]]), int(iu[1][first[r]])) for r in ranks]
    return xy, lab, vals[ranks], 4, pairs


def fused_misses(xy, r2, pairs):
    """Of the on-threshold pairs, how many a contracted evaluation would lose: with exact rational arithmetic, the pairs whose
    fma(dx, dx, dy * dy) or fma(dy, dy, dx * dx) -- one rounding of the exact dx^2 + fl(dy^2) -- comes out above the threshold
    that their unfused d2 equals."""
    lost = 0
    for (i, j), r in zip(pairs, r2):
        dx, dy = float(xy[i, 0] - xy[j, 0]), float(xy[i, 1] - xy[j, 1])
        assert dx * dx + dy * dy == r
        fx = float(Fraction(dx) * Fraction(dx) + Fraction(dy * dy))          # float(Fraction) rounds correctly, once
        fy = float(Fraction(dy) * Fraction(dy) + Fraction(dx * dx))
        lost += fx > r or fy > r
    return lost


def planted_xy():
    """(xy, labels, K) of the 45 x 45 planted set of nhood_cases."""
    xy, lab, _, _, K = nhood_cases.planted(45)
    return xy, lab, K


@functools.lru_cache(maxsize=None)
def want(name):
    """The restatement's counts of a named case, computed once: 'edge<i>', 'tile<n>', 'lattice', 'on_threshold', 'planted'
    (default radii, B = 50), 'planted_far' (one radius above the diameter)."""
    if name.startswith("edge"):
        xy, lab, r2, K = edge_call()[int(name[4:])]
    elif name.startswith("tile"):
        xy, lab, r2, K = tile_case(int(name[4:]))
    elif name == "lattice":
        xy, lab, r2, K = lattice()
    elif name == "on_threshold":
        xy, lab, r2, K, _ = on_threshold()
    elif name == "planted":
        xy, lab, K = planted_xy()
        r2 = ref.default_radii(xy, 50) ** 2
    else:
        raise KeyError(name)
    return _readonly(ref.counts(xy, lab, r2, K))


@functools.lru_cache(maxsize=None)
def stage_want(bins=50):
    """{tp: (counts, radii, K)} of nhood_cases.stage_table() under the stage's default radii."""
    df = nhood_cases.stage_table()
    out = {}
    for tp in sorted(set(df["timepoint"])):
        m = np.asarray(df["timepoint"]) == tp
        xy = np.stack([df["pixel_x"][m], df["pixel_y"][m]], axis=1)
        lab = np.asarray(df["kmeans"])[m]
        K = int(lab.max()) + 1
        radii = ref.default_radii(xy, bins)
        out[tp] = (_readonly(ref.counts(xy, lab, radii * radii, K)), radii, K)
    return out
