"""The host K-means reference (tests/kmeans_ref.py) and the inputs of the GPU kernel tests (tests/kmeans_inputs.py), settled
without a device: the reference against sklearn with an explicit init and against the same rules in integer arithmetic on the
lattice inputs, and, for every general input, the margins that leave the GPU tests nothing to exclude."""
import warnings
from fractions import Fraction

import numpy as np
import pytest

import kmeans_inputs as ki
import kmeans_ref as ref

I64 = np.int64


def test_longdouble_is_wide_or_fsum_is_used():
    assert ref.WIDE == (np.finfo(np.longdouble).nmant >= 63)
    x = np.array([1.0, 2.0 ** -60, -1.0])
    assert float(ref._sum0(x)) == 2.0 ** -60                    # either way the accumulation is wider than fp64


# ---------------------------------------------------------------------------------------------- against sklearn
@pytest.mark.parametrize("n,k,d", [(700, 10, 20), (2300, 20, 20), (1500, 6, 3)])
def test_reference_matches_sklearn_with_explicit_init(n, k, d):
    """sklearn centres the data and the init itself; the reference runs on the centred data and the mean is added back.
    1e-12 relative to the largest |centre| (sklearn's chunked fp64 sums over <= 2300 points are within ~n 2^-53)."""
    from sklearn.cluster import KMeans
    rng = np.random.default_rng(n + k)
    X = ki.blobs(rng, n, k, d, 2.0, 0.8) + 1.0
    mean = X.mean(0)
    Xc = X - mean
    tol = ki.tol_of(Xc)
    C0 = X[rng.choice(n, k, replace=False)]
    scale = np.abs(X).max()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = KMeans(k, init=C0, n_init=1, algorithm="lloyd", max_iter=1).fit(X)
        full = KMeans(k, init=C0, n_init=1, algorithm="lloyd").fit(X)
    labels, C1, _, _, _, _, _ = ref.lloyd_step(Xc, C0 - mean, tol)
    assert np.bincount(labels, minlength=k).min() > 0            # (sklearn relocates empty clusters: not comparable)
    inertia1 = float(ref._sum0(ref.assign(Xc, C1)[1]))
    assert np.abs(one.cluster_centers_ - (C1 + mean)).max() <= 1e-12 * scale
    assert abs(one.inertia_ - inertia1) <= 1e-12 * inertia1
    C, lab, inertia, n_iter, min_gap, _, emptied, _ = ref.fit(Xc, C0 - mean, tol)
    assert min_gap >= ki.COND and not emptied
    assert n_iter == full.n_iter_
    assert np.abs(full.cluster_centers_ - (C + mean)).max() <= 1e-12 * scale
    assert abs(full.inertia_ - inertia) <= 1e-12 * inertia
    np.testing.assert_array_equal(full.labels_, lab)


# ---------------------------------------------------------------------------------------------- the lattice, in integers
def _int_lloyd(X, C):
    """The Lloyd step in integers: labels, member sums and counts, inertia; every distance an exact int64."""
    Xi, Ci = X.astype(I64), C.astype(I64)
    d2 = np.stack([((Xi - c) ** 2).sum(1) for c in Ci], axis=1)
    labels = d2.argmin(1)
    sums = np.stack([Xi[labels == k].sum(0) for k in range(C.shape[0])])
    return labels, sums, np.bincount(labels, minlength=C.shape[0]), int(d2.min(1).sum()), d2


@pytest.mark.parametrize("d", ki.LLOYD_DIMS)
def test_lattice_lloyd_reference_equals_integer_arithmetic(d):
    sets, restarts, K_max = ki.lattice_lloyd(d)
    assert (K_max + 256) * d <= ki.LDS_DOUBLES < (K_max + 257) * d or K_max == 32
    assert len(restarts) >= 70
    tols = ki.exact_tols(sets, restarts)
    saw = dict(empty=0, twin=0, tie=0, far=0, done=0, live=0)
    for r, (g, C) in enumerate(restarts):
        X = sets[g]
        assert np.array_equal(X, np.round(X)) and np.abs(X).max() <= 8 and np.array_equal(C, np.round(C))
        labels, C_new, inertia, shift, done, gap, _ = ref.lloyd_step(X, C, tols[g])
        il, sums, cnt, iin, d2 = _int_lloyd(X, C)
        np.testing.assert_array_equal(labels, il)
        assert inertia == float(iin) and iin < 2 ** 53
        for k in range(C.shape[0]):
            if cnt[k] == 0:
                assert np.array_equal(C_new[k], C[k])             # kept
            else:
                want = [float(Fraction(int(s), int(cnt[k]))) for s in sums[k]]      # the correctly rounded quotient
                assert C_new[k].tolist() == want
        assert tols[g] == 0 or abs(shift - tols[g]) > 1e-4 * tols[g]
        assert done == (shift <= tols[g])
        saw["done" if done else "live"] += 1
        saw["empty"] += int((cnt == 0).any())
        if C.shape[0] >= 3 and r < len(restarts) - 1:
            assert np.array_equal(C[1], C[0]) and cnt[1] == 0 and cnt[2] == 0
            saw["twin"] += int(cnt[0] > 0)
            saw["far"] += 1
        # a point at the same distance from two DIFFERENT centres, nearest to both: it went to the lower index
        two = np.sort(d2, axis=1)[:, :2] if C.shape[0] >= 2 else None
        if two is not None:
            for i in np.flatnonzero(two[:, 0] == two[:, 1]):
                ks = np.flatnonzero(d2[i] == two[i, 0])
                if not np.array_equal(C[ks[0]], C[ks[1]]):
                    assert labels[i] == ks[0] and gap[i] == 0
                    saw["tie"] += 1
                    break
    assert all(v > 0 for v in saw.values()), saw
    g, C = restarts[-1]                                           # K = npts: every point its own cluster
    _, C_new, inertia, shift, done, _, _ = ref.lloyd_step(sets[g], C, 0.0)
    assert inertia == 0 and shift == 0 and done and np.array_equal(C_new, C)


def _int_seed_rows(X, k, first, U):
    """The k-means++ rounds in integers (distances as sums of squared differences, which on integers equal the expanded
    form); the one rounding of the rule, fl(u * pot), is taken from the exact product."""
    Xi = X.astype(I64)
    n = Xi.shape[0]
    d2 = lambda j: ((Xi - Xi[j]) ** 2).sum(1)
    trials = ref.trials_of(k)
    U = np.asarray(U).reshape(max(k - 1, 0), trials)
    rows, closest = [int(first)], d2(first)
    for c in range(1, k):
        pot = int(closest.sum())
        cum = np.cumsum(closest)
        assert pot < 2 ** 53
        cands = []
        for u in U[c - 1]:
            rv = float(Fraction(float(u)) * pot)
            hit = np.flatnonzero(cum.astype(np.float64) >= rv)
            cands.append(int(hit[0]) if hit.size else n - 1)
        pots = [int(np.minimum(d2(j), closest).sum()) for j in cands]
        best = pots.index(min(pots))
        rows.append(cands[best])
        closest = np.minimum(d2(cands[best]), closest)
    return rows


@pytest.mark.parametrize("d", ki.SEED_DIMS)
def test_lattice_seeding_reference_equals_integer_arithmetic(d):
    sets, probs = ki.lattice_seeding(d)
    tags = set()
    for p in probs:
        X = sets[p["g"]]
        rows, draw_dist, cand_gap = ref.seed_rows(X, p["k"], p["first"], p["U"])
        assert rows.tolist() == _int_seed_rows(X, p["k"], p["first"], p["U"]), p["tag"]
        tags.add(p["tag"])
        if p["tag"] == "exact prefix":
            assert draw_dist[0, 0] == 0
            cum = np.cumsum(((X - X[p["first"]]) ** 2).sum(1))
            assert p["U"][0] * cum[-1] == cum[p["row"]] and cum[p["row"]] > cum[p["row"] - 1]
            assert np.searchsorted(cum, p["U"][0] * cum[-1], side="right") > p["row"]        # side right differs
        if p["tag"] == "zero potential":
            assert rows.tolist() == [p["first"]] + [0] * (p["k"] - 1) and np.isinf(draw_dist).all()
        if p["tag"] == "mirror tie":
            assert cand_gap[0] == 0 and rows.tolist() == [3, 5]                              # the first candidate
        if p["tag"] == "past the last prefix":
            assert rows[1] == X.shape[0] - 1                                                 # the clamp
        if p["tag"] == "u=0":
            assert rows[1] == (1 if p["first"] == 0 else 0) or ((X[0] == X[p["first"]]).all())
    assert tags == {"random", "u=0", "below one", "past the last prefix", "exact prefix", "zero potential", "mirror tie"}
    assert {ref.trials_of(p["k"]) for p in probs} == {2, 3, 4, 5}


def test_invalid_seeding_problems_are_invalid_for_the_stated_reason():
    sets, n_max, K_max, probs = ki.invalid_seeding()
    for p in probs:
        n = sets[p["g"]].shape[0]
        assert p["valid"] == (1 <= p["k"] <= K_max and 0 <= p["first"] < n and n <= n_max)
        if p["valid"]:
            rows = ref.seed_rows(sets[p["g"]], p["k"], p["first"], p["U"])[0]
            assert rows.tolist() == _int_seed_rows(sets[p["g"]], p["k"], p["first"], p["U"])
    assert sum(p["valid"] for p in probs) == 4 and probs[0]["valid"] and probs[-1]["valid"]


# ---------------------------------------------------------------------------------------------- the general inputs' margins
@pytest.mark.parametrize("name", [c[0] for c in ki.GENERAL])
def test_general_lloyd_inputs_decide_nothing_within_rounding(name):
    Xc, tol, C0 = ki.general_case(name)
    for r in range(C0.shape[0]):
        _, _, _, n_iter, min_gap, min_tol, _, _ = ref.fit(Xc, C0[r], tol)
        assert 2 <= n_iter < 300
        assert min_gap >= ki.COND and min_tol >= ki.COND, (name, r, min_gap, min_tol)


def test_general_seeding_inputs_decide_nothing_within_rounding():
    sets = ki.seed_general_sets()
    probs = ki.seed_general_problems(sets)
    assert {p["k"] for p in probs} >= set(range(4, 33))
    for p in probs:
        _, draw_dist, cand_gap = ref.seed_rows(sets[p["g"]], p["k"], p["first"], p["U"])
        assert draw_dist.min() >= ki.COND and cand_gap.min() >= ki.COND, (p["g"], p["k"], draw_dist.min(), cand_gap.min())


def test_fit_inputs_decide_nothing_within_rounding():
    from spadot_amd.kmeans import sweep_draws
    empties = 0
    for X in ki.fit_sets():
        Xc = X - X.mean(0)
        tol = ki.tol_of(Xc)
        for k in ki.FIT_KS:
            first, U = sweep_draws(X.shape[0], k, ki.FIT_SEED, ki.FIT_RESTARTS)
            for r in range(ki.FIT_RESTARTS):
                rows, draw_dist, cand_gap = ref.seed_rows(Xc, k, int(first[r]), U[r])
                assert min(draw_dist.min(initial=np.inf), cand_gap.min(initial=np.inf)) >= ki.COND, (X.shape[0], k, r)
                _, _, _, n_iter, min_gap, min_tol, emptied, _ = ref.fit(Xc, Xc[rows], tol)
                assert min_gap >= ki.COND and min_tol >= ki.COND and n_iter < 300, (X.shape[0], k, r, min_gap, min_tol)
                empties += int(emptied)
    print("restarts that end with an empty cluster:", empties)


def test_assign_inputs_have_ties_on_the_lattice_and_margins_elsewhere():
    ties = 0
    for n, k, d in ki.assign_shapes():
        X, C = ki.assign_case(n, k, d, lattice=True)
        assert np.array_equal(X, np.round(X)) and np.array_equal(C, np.round(C))
        labels, _, gap = ref.assign(X, C)
        np.testing.assert_array_equal(labels, _int_lloyd(X, C)[0])
        ties += int(k >= 2 and (gap == 0).any())
        X, C = ki.assign_case(n, k, d, lattice=False)
        assert ref.assign(X, C)[2].min() >= ki.COND, (n, k, d)
        gap32 = ref.assign(X.astype(np.float32), C.astype(np.float32))[2].min()
        assert gap32 >= ki.ASSIGN_GAP32, (n, k, d, gap32)
    assert ties >= 20
