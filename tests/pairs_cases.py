"""Inputs of the tests of what the pair-counting stages share (CPU and GPU): the 257-spot tile cases of cooccur_cases and
ripley_cases under B = 17 and B = 33 thresholds, which the shared dispatch pads to 32 and 48 columns, and the restatements'
integers of each, computed once per process."""
import functools

import numpy as np

import cooccur_cases
import cooccur_null_ref
import cooccur_ref
import ripley_cases

BINS = (17, 33)                    # padded to 32 and 48: the two widths of the dispatch that no other GPU test of cooccur runs
N, S, SEED = 257, 2, ripley_cases.SEED


def _drawn(seed, B, r_max):
    r2 = cooccur_cases._thresholds(np.random.default_rng(seed), B, r_max)
    assert r2.shape == (B,) and np.all(np.diff(r2) > 0) and r2[0] >= 0
    r2.setflags(write=False)
    return r2


@functools.lru_cache(maxsize=None)
def cooccur_problem(B):
    """(xy, labels, r2, K) of cooccur_cases.tile_case(257) with B thresholds."""
    xy, lab, _, K = cooccur_cases.tile_case(N)
    return xy, lab, _drawn(3000 + B, B, 12.0), K


@functools.lru_cache(maxsize=None)
def ripley_problem(B, null):
    """The problem of ripley_cases.tile_case(257, null) (S = 2, M = 100) with B thresholds."""
    return dict(ripley_cases.tile_case(N, null), r2=_drawn(3100 + B, B, 6.0))


@functools.lru_cache(maxsize=None)
def want(kind, B):
    """The restatement's integers: 'cooccur' [K, K, B], 'null' [1 + S, K, K, B] (seed SEED, g = 0), 'labels' and 'csr'
    [K, 1 + S, 3, B] (ripley under SEED)."""
    if kind == "cooccur":
        xy, lab, r2, K = cooccur_problem(B)
        out = cooccur_ref.counts(xy, lab, r2, K)
    elif kind == "null":
        xy, lab, r2, K = cooccur_problem(B)
        out = cooccur_null_ref.counts(xy, lab, r2, K, S, seed=SEED, g=0)
    else:
        out = ripley_cases.counts_of(ripley_problem(B, kind))
    out.setflags(write=False)
    return out
