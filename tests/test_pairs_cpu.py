"""What the pair-counting stages share on the host (spadot_amd/pairs.py and the helpers of stage_ops), without a GPU:
the thresholds of a call, the global envelope test against both copies it replaced and against Python integers, the threshold
and cluster-offset helpers of the checks, the names the stage modules hand on, and that the restatements run the inputs of
tests/test_pairs_gpu.py."""
import numpy as np
import pytest

import pairs_cases
import ripley_ref
from spadot_amd import pairs


def test_thresholds_take_exactly_one_of_radii_and_their_squares():
    for radii, radii_sq in (([[1.0]], [[1.0]]), (None, None)):
        with pytest.raises(ValueError, match="some_call takes exactly one of radii and radii_sq"):
            pairs.thresholds("some_call", 1, radii, radii_sq)
    got = pairs.thresholds("some_call", 2, [[0.1, 0.3], np.array([3.0])], None)
    assert [t.dtype for t in got] == [np.float64, np.float64]
    assert got[0].tolist() == [0.1 * 0.1, 0.3 * 0.3] and got[1].tolist() == [9.0]      # r * r in fp64
    assert pairs.thresholds("some_call", 1, None, [[0.0, 0.5]])[0].tolist() == [0.0, 0.5]


def test_thresholds_refuse_a_wrong_count_of_sets_or_of_radii():
    for P, given, labelings in ((2, [[1.0]], None), (0, [], None), (1, [[1.0]], 2)):
        with pytest.raises(ValueError, match="one labeling and one set of radii per problem"):
            pairs.thresholds("some_call", P, None, given, labelings=labelings)
    with pytest.raises(ValueError, match="at most 65535 per call"):
        pairs.thresholds("some_call", 65536, None, [[1.0]] * 65536)
    for bad in ([], np.arange(65.0)):
        with pytest.raises(ValueError, match="thresholds: the device takes 1 to 64"):
            pairs.thresholds("some_call", 1, None, [bad])
        with pytest.raises(ValueError, match="radii: the device takes 1 to 64"):
            pairs.thresholds("some_call", 1, [bad], None)
    assert pairs.thresholds("some_call", 1, [np.arange(64.0)], None)[0].shape == (64,)


def test_thresholds_refuse_a_ladder_that_is_not_finite_positive_and_increasing():
    for bad in ([-1.0, 2.0], [1.0, np.inf], [1.0, np.nan], [1.0, 1.0], [2.0, 1.0]):
        with pytest.raises(ValueError, match="squared thresholds of problem 1 must be finite, >= 0 and strictly increasing"):
            pairs.thresholds("some_call", 2, None, [[1.0], bad])
        with pytest.raises(ValueError, match="radii of problem 1 must be finite, >= 0 and strictly increasing"):
            pairs.thresholds("some_call", 2, [[1.0], bad], None)
    a = 1.0
    b = np.nextafter(a, 2.0)
    tiny = [1e-200, 2e-200]                                                              # two radii, one square: both squares are 0
    assert tiny[0] < tiny[1] and tiny[0] * tiny[0] == tiny[1] * tiny[1]
    with pytest.raises(ValueError, match="squared thresholds of problem 0 must be finite, >= 0 and strictly increasing"):
        pairs.thresholds("some_call", 1, [tiny], None)
    assert pairs.thresholds("some_call", 1, [[a, b]], None)[0].tolist() == [a * a, b * b]


def _former_cooccur_mad_p(T):
    """The copy that cooccurrence.py held: curves along axis 0."""
    n = T.shape[0]
    if T.size and int(T.max()) * n >= 2 ** 62:
        T = T.astype(object)
    dev = np.abs(n * T - T.sum(axis=0, keepdims=True)).max(axis=-1)
    return np.asarray((dev >= dev[:1]).sum(axis=0), dtype=np.float64) / n


def _former_ripley_mad_p(x, exact):
    """The copy that ripley.py held: curves along axis -2, no guard against int64 overflow."""
    n = x.shape[-2]
    if exact:
        dev = np.abs(n * x.astype(np.int64) - x.astype(np.int64).sum(axis=-2, keepdims=True)).max(axis=-1)
    else:
        dev = np.abs(n * x - x.sum(axis=-2, keepdims=True)).max(axis=-1)
    return (dev >= dev[..., :1]).sum(axis=-1) / float(n)


def test_mad_p_is_the_cooccurrence_copy_on_counts_near_two_to_the_62():
    """The inputs of test_the_global_test_is_exact_on_counts_near_two_to_the_62 (tests/test_cooccur_null_cpu.py)."""
    big = 2 ** 62
    rows = np.array([big + 1, 0, big, 1], dtype=np.int64).reshape(4, 1, 1, 1)
    T = np.cumsum(np.random.default_rng(3).integers(big // 8, big // 4, (8, 2, 2, 5)), axis=3)
    T = T + T.transpose(0, 2, 1, 3)
    for x in (rows, T):
        got = pairs.mad_p(x)
        assert got.dtype == np.float64 and got.shape == x.shape[1:3]
        np.testing.assert_array_equal(got, _former_cooccur_mad_p(x))
        moved = np.ascontiguousarray(np.moveaxis(x, 0, -2))                              # ripley's layout of the same curves: guarded too
        np.testing.assert_array_equal(pairs.mad_p(moved, axis=-2), got)
        for a in range(x.shape[1]):
            for b in range(x.shape[2]):
                assert got[a, b] == ripley_ref.mad_p(None, exact=x[:, a, b, :])
    assert pairs.mad_p(rows)[0, 0] == 0.5


def test_mad_p_is_the_ripley_copy_on_a_ripley_array():
    rng = np.random.default_rng(11)
    K, S, B = 4, 19, 9
    N = np.cumsum(rng.integers(0, 50, (3, K, 1 + S, B)), axis=-1)                       # [3, K, 1 + S, B] integers
    L = np.sqrt(7.25 * N[0] / np.pi)                                                    # fp64 curves
    for i in range(3):
        got = pairs.mad_p(N[i], axis=-2)
        assert got.dtype == np.float64 and got.shape == (K,)
        np.testing.assert_array_equal(got, _former_ripley_mad_p(N[i], exact=True))
        np.testing.assert_array_equal(got, _former_cooccur_mad_p(np.moveaxis(N[i], -2, 0)))
        np.testing.assert_array_equal(got, [ripley_ref.mad_p(None, exact=N[i, c]) for c in range(K)])
    got = pairs.mad_p(L, axis=-2)
    np.testing.assert_array_equal(got, _former_ripley_mad_p(L, exact=False))
    np.testing.assert_array_equal(got, [ripley_ref.mad_p(L[c]) for c in range(K)])
    np.testing.assert_array_equal(pairs.mad_p(N, axis=-2), np.stack([pairs.mad_p(N[i], axis=-2) for i in range(3)]))


def test_the_integer_path_and_the_float_path_agree_on_small_integers():
    T = np.cumsum(np.random.default_rng(5).integers(0, 1000, (40, 3, 3, 12)), axis=-1)
    np.testing.assert_array_equal(pairs.mad_p(T), pairs.mad_p(T.astype(np.float64)))    # exact in fp64 below 2^53
    np.testing.assert_array_equal(pairs.mad_p(T.astype(np.int32)), pairs.mad_p(T))
    moved = np.moveaxis(T, 0, -2)
    np.testing.assert_array_equal(pairs.mad_p(moved, axis=-2), pairs.mad_p(moved.astype(np.float64), axis=-2))
    np.testing.assert_array_equal(pairs.mad_p(moved, axis=2), pairs.mad_p(T))


def test_the_threshold_helper_of_the_checks_takes_the_padded_form_and_refuses_bad_padding():
    from spadot_amd import stage_ops as ops
    assert [ops.cooccur_padded(B) for B in (1, 16, 17, 32, 33, 48, 49, 64)] == [16, 16, 32, 32, 48, 48, 64, 64]
    t = np.array([0.0, 0.5, 2.0])

    def padded(row, B=3, width=16):
        pad = np.full((2, width), -1.0)
        ops._padded_thresholds(pad, 1, row, B)
        assert np.all(pad[0] == -1.0)
        return pad[1]

    want = np.concatenate([t, np.full(13, -1.0)])
    np.testing.assert_array_equal(padded(t), want)
    np.testing.assert_array_equal(padded(want), want)                                   # the padded form itself
    np.testing.assert_array_equal(padded(list(t)), want)
    for bad in (np.concatenate([t, np.full(13, -2.0)]), np.concatenate([t, [5.0], np.full(12, -1.0)]),
                np.concatenate([t, np.full(12, -1.0), [np.nan]])):
        with pytest.raises(ValueError, match="problem 1 has 16 thresholds and its descriptor says 3"):
            padded(bad)
    with pytest.raises(ValueError, match="problem 1 has 3 thresholds and its descriptor says 2"):
        padded(t, B=2)
    full = np.arange(16.0)                                                              # B = BP: nothing is padding
    np.testing.assert_array_equal(padded(full, B=16), full)
    for bad in ([-1.0, 0.5, 2.0], [0.0, np.inf, np.inf], [0.0, np.nan, 2.0], [0.0, 0.5, 0.5], [0.0, 2.0, 0.5]):
        with pytest.raises(ValueError, match="squared thresholds of problem 1 must be finite, >= 0 and strictly increasing"):
            padded(np.array(bad))


def test_the_offset_helper_of_the_checks_wants_offsets_that_ascend_from_0_to_n():
    from spadot_amd import stage_ops as ops
    assert ops._cluster_offsets_ok([0, 20, 20, 36], 36) and ops._cluster_offsets_ok([0, 5], 5)
    assert ops._cluster_offsets_ok([0, 0, 0, 7], 7)
    for coff, n in (([1, 20, 36], 36), ([0, 20, 35], 36), ([0, 20, 16, 36], 36), ([0, 40, 36], 36)):
        assert not ops._cluster_offsets_ok(coff, n), coff


def test_the_ripley_limits_are_the_cooccurrence_limits():
    from spadot_amd import stage_ops as ops
    assert (ops.RIPLEY_MAX_K, ops.RIPLEY_MAX_B, ops.RIPLEY_MAX_N, ops.RIPLEY_MAX_P, ops.RIPLEY_MAX_Y, ops.RIPLEY_MAX_G) == \
        (32, 64, 2147483391, 65535, 65535, 2147483647)
    assert (ops.COOCCUR_MAX_K, ops.COOCCUR_MAX_B, ops.COOCCUR_MAX_N, ops.COOCCUR_MAX_P, ops.COOCCUR_MAX_Y, ops.COOCCUR_MAX_G) == \
        (32, 64, 2147483391, 65535, 65535, 2147483647)
    assert (pairs.MAX_CLUSTERS, pairs.MAX_BINS, pairs.MAX_SPOTS, pairs.MAX_PROBLEMS) == (32, 64, 2147483391, 65535)


def test_the_stage_modules_hand_on_the_shared_names():
    from spadot_amd import cooccurrence, ripley
    for name in ("default_radii", "ladder", "sorted_problems", "MAX_CLUSTERS", "MAX_BINS", "MAX_SPOTS", "MAX_PROBLEMS"):
        assert getattr(cooccurrence, name) is getattr(pairs, name), name
    for name in ("default_radii", "ladder", "MAX_BINS"):
        assert getattr(ripley, name) is getattr(pairs, name), name
    assert not hasattr(cooccurrence, "_mad_p") and not hasattr(ripley, "_mad_p")
    assert pairs.ladder(2.0, 4).tolist() == [0.5, 1.0, 1.5, 2.0]


@pytest.mark.parametrize("B", pairs_cases.BINS)
def test_the_restatements_run_the_inputs_of_the_gpu_test(B):
    xy, lab, r2, K = pairs_cases.cooccur_problem(B)
    assert xy.shape == (257, 2) and r2.shape == (B,) and np.all(np.diff(r2) > 0)
    plain, null = pairs_cases.want("cooccur", B), pairs_cases.want("null", B)
    assert plain.shape == (K, K, B) and null.shape == (3, K, K, B) and plain.dtype == np.int64
    np.testing.assert_array_equal(null[0], plain)                                       # pattern 0 is the observed labeling
    assert plain[:, :, 0].sum() < plain[:, :, -1].sum() and np.all(np.diff(plain, axis=2) >= 0)
    np.testing.assert_array_equal(null.sum(axis=(1, 2)), np.tile(plain.sum(axis=(0, 1)), (3, 1)))     # a relabelling keeps the pairs
    for kind in ("labels", "csr"):
        p, N = pairs_cases.ripley_problem(B, kind), pairs_cases.want(kind, B)
        assert p["r2"].shape == (B,) and N.shape == (3, 3, 3, B) and N.any(axis=(0, 1, 3)).all()
        sizes = np.bincount(p["lab"], minlength=3)
        assert sizes.tolist() == [40, 257, 23] and np.all(N[:, :, 1, :] <= sizes[:, None, None]) and np.all(N[:, :, 2, :] <= p["M"])
    np.testing.assert_array_equal(pairs_cases.want("labels", B)[:, 0], pairs_cases.want("csr", B)[:, 0])
