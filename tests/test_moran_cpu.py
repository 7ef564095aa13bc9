"""What the Moran stages share on the host (spadot_amd/moran.py), numpy only: the degeneracy rule against both restatements of it,
the Moran ordering and the union of the top genes against the stage restatement of tests/modules_cases.py, and the refusals of a
gene selection."""
import numpy as np
import pytest

import autocorr_ref as aref
import modules_cases as mcases
import modules_ref as mref
from spadot_amd import moran


def _rule_cases():
    """(what, n, E, m2 [4], sumsq [4]): around every clause of the rule.  The floor n 2^-50 sumsq is exact in fp64 for these
    n and sumsq (a product of a small integer, a power of two and a short mantissa), so `at` and `above` sit exactly on it and
    one ulp past it."""
    sumsq = np.array([3.0, 0.75, 1e6, 5.0])
    ok = np.array([1.0, 0.5, 2.0, 4.0])
    at = 37 * 2.0 ** -50 * sumsq
    return [("n = 2", 2, 5, ok, sumsq), ("E = 0", 37, 0, ok, sumsq), ("m2 = 0", 37, 150, np.array([0.0, 0.5, 0.0, 4.0]), sumsq),
            ("at the floor", 37, 150, at, sumsq), ("one ulp above", 37, 150, np.nextafter(at, np.inf), sumsq),
            ("mixed", 37, 150, np.array([at[0], np.nextafter(at[1], np.inf), 0.0, 4.0]), sumsq)]


@pytest.mark.parametrize("what,n,E,m2,sumsq", _rule_cases(), ids=[c[0] for c in _rule_cases()])
def test_degenerate_is_the_rule_of_both_restatements(what, n, E, m2, sumsq):
    got = moran.degenerate(n, E, m2, sumsq)
    assert got.dtype == bool and got.shape == (4,)
    assert got.tolist() == [bool(aref.is_degenerate(n, E, a, b)) for a, b in zip(m2, sumsq)]
    assert got.tolist() == mref.degenerate(n, E, m2, sumsq).tolist()
    want = {"n = 2": [True] * 4, "E = 0": [True] * 4, "m2 = 0": [True, False, True, False], "at the floor": [True] * 4,
            "one ulp above": [False] * 4, "mixed": [True, False, True, False]}[what]
    assert got.tolist() == want


def test_degenerate_without_the_sum_of_squares_asks_for_a_positive_spread():
    m2 = np.array([0.0, 1e-300, 1.0, -0.0])
    assert moran.degenerate(37, 150, m2).tolist() == [True, False, False, True]
    assert moran.degenerate(37, 150, m2).tolist() == mref.degenerate(37, 150, m2, np.zeros(4)).tolist()
    assert moran.degenerate(2, 150, m2).tolist() == [True] * 4 and moran.degenerate(37, 0, m2).tolist() == [True] * 4
    from spadot_amd.autocorr import autocorr_stats
    N = np.ones((4, 1))
    assert autocorr_stats(N, N, 37, 150, m2, (150, 300, 3600))["degenerate"].tolist() == [True, False, False, True]


class _R:
    def __init__(self, I):
        self.I = np.asarray(I, dtype=np.float64)


def test_the_moran_ordering_and_the_top_genes_match_the_stage_restatement():
    nan = np.nan
    Is = [np.array([0.3, nan, 0.7, 0.3, -0.1, 0.7, nan]), np.array([nan, 0.2, 0.2, nan, 0.9, -0.5, 0.2]), np.full(7, nan)]
    assert moran.moran_order(Is[0]).tolist() == [2, 5, 0, 3, 4, 1, 6]                # descending, ties by index, NaN last
    assert moran.moran_order(Is[1]).tolist() == [4, 1, 2, 6, 5, 0, 3]
    assert moran.moran_order(Is[2]).tolist() == list(range(7))
    for I in Is:
        np.testing.assert_array_equal(moran.moran_order(I), np.lexsort((np.arange(7), -np.where(np.isnan(I), -np.inf, I))))
    for top in (1, 2, 3, 6, 7, 50):                                                  # 50: larger than G
        got = moran.top_genes([_R(I) for I in Is], top)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, mcases.top_union(Is, top))
    assert moran.top_genes([_R(Is[0])], 3).tolist() == [0, 2, 5]
    assert moran.top_genes([_R(I) for I in Is], 50).tolist() == [0, 1, 2, 3, 4, 5, 6]
    empty = moran.top_genes([_R(Is[2]), _R(Is[2])], 4)                                # all NaN: nothing is picked
    assert empty.dtype == np.int32 and empty.size == 0 and mcases.top_union([Is[2]], 4).size == 0


def test_a_gene_selection_keeps_repeats_and_order_and_refuses_the_rest():
    sel = moran.gene_selection([4, 1, 1, 0], 5)
    assert sel.dtype == np.int32 and sel.tolist() == [4, 1, 1, 0]
    assert moran.gene_selection(np.array([[3, 2], [1, 0]], dtype=np.uint8), 4).tolist() == [3, 2, 1, 0]
    assert moran.gene_selection(range(3), 3).tolist() == [0, 1, 2]
    for genes in ([], np.zeros(0, dtype=np.int64), [0.0, 1.0], np.array([1.5]), [True, False]):
        with pytest.raises(ValueError, match="at least one integer gene index"):
            moran.gene_selection(genes, 5)
    for genes, what in (([0, 5], r"selected genes 0 \.\. 5 must lie in 0 \.\. 4"), ([-1, 2], r"selected genes -1 \.\. 2")):
        with pytest.raises(ValueError, match=what):
            moran.gene_selection(genes, 5)


def test_the_stage_modules_hand_on_the_shared_names():
    from spadot_amd import hotspots
    assert hotspots.read_genes is moran.read_genes
    assert moran.read_genes("b, a,b", ["a", "b", "a"]).tolist() == [1, 0, 1]         # the first gene of a repeated name
