"""Inputs of the correlogram tests (CPU and GPU): the sets around the 256-wide tile of csrc/correlogram.hip with 1, 7 and 16 bands,
the integer lattice, the on-threshold set of cooccur_cases, two coincident spots, the sparse set on which tiles are culled, the
planted lattice with a smooth, a white and a checkerboard gene, and the restatement's sums of each, computed once per process."""
import functools

import numpy as np

import cooccur_cases as cc
import correlogram_ref as ref

SIZES = (1, 2, 255, 256, 257, 513)
BAND_COUNTS = (1, 7, 16)
SEED = 5
PLANTED_RADII = (1.3, 2.5, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0, 16.0)


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def centred(V):
    """The columns of V minus their means, fp64."""
    V = np.asarray(V, dtype=np.float64)
    return V - V.mean(axis=0, keepdims=True)


@functools.lru_cache(maxsize=None)
def sized(n, B, G=3):
    """(xy, X fp64 [n, G] centred, r2 [B]) of n spots uniform over 25 x 25, thresholds up to 12^2."""
    rng = np.random.default_rng(3000 + 17 * n + B)
    xy = rng.uniform(0, 25, (n, 2))
    r2 = np.sort(rng.uniform(0.5, 12.0, B)) ** 2
    assert np.all(np.diff(r2) > 0)
    return _readonly(xy, centred(rng.standard_normal((n, G))), r2)


@functools.lru_cache(maxsize=None)
def lattice():
    """The 12 x 12 integer lattice: every squared distance is an integer, every pair exactly on or off a threshold."""
    xy, _, r2, _ = cc.lattice()
    X = centred(np.random.default_rng(12).standard_normal((144, 3)))
    return _readonly(np.array(xy), X, np.array(r2))


@functools.lru_cache(maxsize=None)
def on_threshold():
    """The on-threshold set of cooccur_cases with 16 of its 64 thresholds: each is the unfused squared distance of one of the
    set's own pairs."""
    xy, _, r2, _, pairs = cc.on_threshold()
    X = centred(np.random.default_rng(13).standard_normal((xy.shape[0], 2)))
    return _readonly(np.array(xy), X, np.array(r2[::4])) + (pairs[::4],)


@functools.lru_cache(maxsize=None)
def coincident():
    """Two coincident spots and a third, thresholds 0 and 4: the coincident pair is in band 0."""
    xy = np.array([[1.25, 7.5], [1.25, 7.5], [2.25, 7.5]])
    return _readonly(xy, centred(np.array([[1.0, 2.0], [3.0, -1.0], [-2.0, 0.5]])), np.array([0.0, 4.0]))


@functools.lru_cache(maxsize=None)
def sparse(G=17):
    """(xy, X [1100, G], r2 [5]): 1100 spots over 40 x 40 with r_max = 3: most tiles of 256 Morton-ordered spots lie out of
    reach of most query blocks."""
    rng = np.random.default_rng(1100)
    xy = rng.uniform(0, 40, (1100, 2))
    return _readonly(xy, centred(rng.standard_normal((1100, G))), np.array([0.6, 1.2, 1.8, 2.4, 3.0]) ** 2)


@functools.lru_cache(maxsize=None)
def planted():
    """(xy [1024, 2], V fp64 [1024, 3]): the 32 x 32 unit lattice with jitter +-0.2 and three genes: white noise convolved with a
    Gaussian of sigma = 3, white noise, and the checkerboard (x + y) mod 2."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(7)
    gx, gy = np.meshgrid(np.arange(32.0), np.arange(32.0), indexing="ij")
    xy = np.stack([gx, gy], -1).reshape(-1, 2) + rng.uniform(-0.2, 0.2, (1024, 2))
    smooth = gaussian_filter(rng.standard_normal((32, 32)), 3.0)
    noise = rng.standard_normal((32, 32))
    checker = (gx + gy) % 2
    return _readonly(xy, np.stack([smooth.reshape(-1), noise.reshape(-1), checker.reshape(-1)], axis=1))


@functools.lru_cache(maxsize=None)
def want(name, n_perms=0, seed=SEED, g=0, first=0, observed=True):
    """(W, S2c, N, Q, AN, AQ) of the restatement for a named case ('sized<n>_<B>', 'lattice', 'on_threshold', 'coincident',
    'sparse', 'planted') over the labelings asked for, computed once."""
    xy, X, r2 = problem(name)
    return _readonly(*ref.all_sums(xy, X, r2, n_perms, seed, g, first, observed))


def problem(name):
    if name.startswith("sized"):
        n, B = (int(v) for v in name[5:].split("_"))
        return sized(n, B)
    if name == "planted":
        xy, V = planted()
        return xy, centred(V), np.asarray(PLANTED_RADII) ** 2
    return {"lattice": lattice, "on_threshold": on_threshold, "coincident": coincident, "sparse": sparse}[name]()[:3]


def stage_counts(path):
    """Writes the counts .npz of the stage test: the planted lattice as one time point 'P0' with five genes -- smooth, noise and
    checker as counts, `flat`, the same count in every spot (degenerate), and `rest`, which fills every spot up to the same total
    of 1000.  The stage takes log1p(10 count) of them: the counts are round(expm1(6 + z / 4) / 10), z the standardised planted
    values, so that the values the stage sees are 6 + z / 4 up to the rounding of the counts."""
    xy, V = planted()
    z = (V - V.mean(axis=0)) / V.std(axis=0)
    counts = np.round(np.expm1(6.0 + 0.25 * z) / 10.0)
    flat = np.full((1024, 1), 7.0)
    rest = 1000.0 - counts.sum(axis=1, keepdims=True) - flat
    assert rest.min() > 0
    X = np.concatenate([counts, flat, rest], axis=1).astype(np.float32)
    order = np.random.default_rng(8).permutation(1024)
    np.savez(path, X=X[order], timepoint=np.asarray(["P0"] * 1024), spatial=xy[order],
             genes=np.asarray(["smooth", "noise", "checker", "flat", "rest"]))
    return path
