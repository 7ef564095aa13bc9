"""utils._stage_utils.labeling_runs by enumeration: the runs of a call hold the observed labeling at most once and first, then
the permutation indices first .. first + n_perms - 1 without gap or overlap, and agree with the arithmetic the stages spelt out by
hand before they shared it.  A wrong index here would not fail anywhere else: it would draw other permutations."""
import itertools

from spadot_amd.utils._stage_utils import labeling_runs

GRID = [(n_perms, observed, first, per, budget)
        for n_perms, observed, first, per in itertools.product(range(7), (False, True), (0, 5), (0, 1, 3))
        if observed + n_perms >= 1
        for budget in range(1, per * (observed + n_perms) + 2)]


def _old_runs(n_perms, observed, first, per, budget):
    """ligrec._runs and the index arithmetic of its callers (and of autocorr.autocorr_sums), as they stood."""
    L = int(observed) + n_perms
    step = L if per * L <= budget else max(1, budget // per)
    runs = [(l, min(step, L - l), bool(observed) and l == 0) for l in range(0, L, step)]
    return [(obs, first + (l - int(observed) if l else 0), take - int(obs)) for l, take, obs in runs]


def test_grid_is_the_one_asked_for():
    assert len(GRID) == len(set(GRID)) == 470           # 13 (n_perms, observed) x 2 firsts x budgets 1 .. per L + 1 of 3 pers
    assert {g[3] for g in GRID} == {0, 1, 3} and {g[2] for g in GRID} == {0, 5} and {g[0] for g in GRID} == set(range(7))


def test_labeling_runs_cover_every_labeling_once_in_order():
    for n_perms, observed, first, per, budget in GRID:
        runs = labeling_runs(n_perms, observed, first, per, budget)
        what = (n_perms, observed, first, per, budget, runs)
        flat = []
        for obs, p0, n in runs:
            assert int(obs) + n >= 1, what                                  # no empty run
            assert n >= 0 and isinstance(obs, bool), what
            flat += ["observed"] * int(obs) + list(range(p0, p0 + n))
        assert flat == ["observed"] * int(observed) + list(range(first, first + n_perms)), what
        L = int(observed) + n_perms
        if per == 0 or per * L <= budget:
            assert len(runs) == 1, what
        else:
            assert all(int(obs) + n <= max(1, budget // per) for obs, _, n in runs), what
            assert all(int(obs) + n == max(1, budget // per) for obs, _, n in runs[:-1]), what      # only the last run is short


def test_labeling_runs_equal_the_old_arithmetic():
    for args in GRID:
        assert labeling_runs(*args) == _old_runs(*args), args
