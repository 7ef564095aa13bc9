"""Inputs of the tests of the co-occurrence null (CPU and GPU): the sets of cooccur_cases and nhood_cases under relabelings, and
the restatement's integers of each (tests/cooccur_null_ref.py), computed once per process."""
import functools

import numpy as np

import cooccur_cases
import cooccur_null_ref as ref
import cooccur_ref
import nhood_cases

PLANTED = dict(bins=20, S=39, seed=7, g=0)      # the planted verdicts: 45 x 45 planted set, 20 default radii
ATTRACT = {(0, 6), (1, 2), (1, 5), (3, 6)}       # the off-diagonal pairs of the planted set that read `attract` (and their transposes)


def _readonly(a):
    a.setflags(write=False)
    return a


def problem(name):
    """(xy, labels, r2, K) of a named case of cooccur_cases: 'edge<i>', 'tile<n>', 'lattice', 'on_threshold'."""
    if name.startswith("edge"):
        return cooccur_cases.edge_call()[int(name[4:])]
    if name.startswith("tile"):
        return cooccur_cases.tile_case(int(name[4:]))
    if name == "lattice":
        return cooccur_cases.lattice()
    if name == "on_threshold":
        return cooccur_cases.on_threshold()[:4]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def want(name, S, seed=0, g=0):
    """The restatement's int64 [1 + S, K, K, B] of a named case under (seed, g)."""
    xy, lab, r2, K = problem(name)
    return _readonly(ref.counts(xy, lab, r2, K, S, seed, g))


@functools.lru_cache(maxsize=None)
def planted():
    """(xy, labels, K, radii, N) of the planted set under PLANTED."""
    xy, lab, K = cooccur_cases.planted_xy()
    radii = cooccur_ref.default_radii(xy, PLANTED["bins"])
    return xy, lab, K, radii, _readonly(ref.counts(xy, lab, radii * radii, K, PLANTED["S"], PLANTED["seed"], PLANTED["g"]))


@functools.lru_cache(maxsize=None)
def caveat():
    """The planted set with an eighth label dealt to 300 spots chosen at random, independently of everything:
    (xy, labels, K = 8, radii, N) under PLANTED."""
    xy, lab, K = cooccur_cases.planted_xy()
    lab = lab.copy()
    lab[np.random.default_rng(5).choice(lab.shape[0], 300, replace=False)] = K
    radii = cooccur_ref.default_radii(xy, PLANTED["bins"])
    return xy, lab, K + 1, radii, _readonly(ref.counts(xy, lab, radii * radii, K + 1, PLANTED["S"], PLANTED["seed"], PLANTED["g"]))


@functools.lru_cache(maxsize=None)
def small_sizes():
    """(xy, labels, r2, K = 4) of 40 spots: the label value 1 has no spots, the label value 3 one spot."""
    rng = np.random.default_rng(77)
    lab = rng.integers(0, 2, 40) * 2
    lab[17] = 3
    return rng.uniform(0, 10, (40, 2)), lab, np.sort(rng.uniform(0.5, 8.0, 9)) ** 2, 4


@functools.lru_cache(maxsize=None)
def stage_want(S, seed, bins=50):
    """{tp: (N, radii, K)} of nhood_cases.stage_table() under the stage's default radii: time point number g in sorted order
    draws under problem number g."""
    df = nhood_cases.stage_table()
    out = {}
    for g, tp in enumerate(sorted(set(df["timepoint"]))):
        m = np.asarray(df["timepoint"]) == tp
        xy = np.stack([df["pixel_x"][m], df["pixel_y"][m]], axis=1)
        lab = np.asarray(df["kmeans"])[m]
        K = int(lab.max()) + 1
        radii = cooccur_ref.default_radii(xy, bins)
        out[tp] = (_readonly(ref.counts(xy, lab, radii * radii, K, S, seed, g)), radii, K)
    return out
