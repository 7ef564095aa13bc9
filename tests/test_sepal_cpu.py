"""CPU: the numpy restatement of the sepal stage (tests/sepal_ref.py) against what can be known without it -- conservation of mass,
the five-point stencil on the lattice, the constant gene, the growth of the entropy, the stability limit, the planted data set --
and the host side of spadot_amd.sepal: the rate and the largest dt, the command line and the frame of the driver."""
import argparse
import functools
import math

import numpy as np
import pytest

import autocorr_cases as ac
import sepal_cases as cases
import sepal_ref as ref

U = ref.U
LONG = 200                                     # the steps of the mass and entropy tests


@functools.lru_cache(maxsize=None)
def _long(name):
    """[t] -> (V, largest degree, [gene] -> [(H, S, A)] over LONG steps) of a case."""
    problems, dt = cases.CASES[name]()
    out = []
    for src, dst, V in problems:
        n = V.shape[0]
        rowptr, col, E, deg = cases.graph_numbers(src, dst, n)
        a = ref.rate(dt, n, E) if E else 0.0
        out.append((V, deg, [ref.diffuse(V[:, g].astype(np.float64), rowptr, col, a, LONG)[1] for g in range(V.shape[1])]))
    return out


def _step_rounding(deg):
    """The relative rounding of one new value: c' = c + a (s - deg c) with a deg < 1.  s is a sum of deg_i terms (gamma_deg s),
    deg c, the subtraction, the product with a and the addition are rounded once each: in all at most (deg + 4) u (s + deg c) a +
    u c', and summed over the spots (sum_i s_i = sum_i deg_i c_i <= max deg S, a max deg < 1) at most (2 deg + 9) u S per step."""
    return (2 * deg + 9) * U


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_mass_is_conserved_to_rounding(name):
    for V, deg, parts in _long(name):
        for g in range(V.shape[1]):
            S = np.array([p[1] for p in parts[g]])
            if math.isnan(parts[g][0][0]):
                continue
            # W is symmetric: sum_i l_i = 0 exactly, and a deg_i < 1 keeps every exact c'_i >= 0, so a clamp removes rounding
            # only (counted twice here); each S is an fsum (u S)
            bound = (2 * LONG * _step_rounding(deg) + 2 * U) * S[0]
            print(name, cases.GENES[g], "largest drift", np.abs(S - S[0]).max(), "bound", bound)
            assert np.abs(S - S[0]).max() <= bound


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_entropy_does_not_decrease_beyond_rounding(name):
    for V, deg, parts in _long(name):
        n = V.shape[0]
        for g in range(V.shape[1]):
            if math.isnan(parts[g][0][0]):
                continue
            H = np.array([p[0] for p in parts[g]])
            # I - a L is doubly stochastic with entries >= 0: the exact step cannot lower the entropy.  Each H is within half
            # of entropy_bound of its exact value, and the rounding e of a step moves n H by at most e (2 + 2 A / S)
            half = np.array([ref.entropy_bound(n, p[1], p[2]) / 2 for p in parts[g]])
            step = np.array([_step_rounding(deg) * (2 + 2 * p[2] / p[1]) / n for p in parts[g]])
            assert np.all(H[1:] - H[:-1] >= -(half[1:] + half[:-1] + step[1:])), (name, cases.GENES[g])
            assert H[-1] > H[0] or cases.GENES[g] == "constant"


def test_the_vectorised_row_sums_are_the_sequential_loop():
    for name in ("n65", "loose", "hub", "lattice"):
        (src, dst, V), = cases.CASES[name]()[0]
        rowptr, col, _, _ = cases.graph_numbers(src, dst, V.shape[0])
        C = V.astype(np.float64)
        np.testing.assert_array_equal(ref.row_sums(C, rowptr, col), ref.row_sums_loop(C, rowptr, col))
        np.testing.assert_array_equal(ref.row_sums(C[:, 3], rowptr, col), ref.row_sums_loop(C, rowptr, col)[:, 3])


def test_the_symmetric_rows_list_own_targets_first_then_the_sources():
    src, dst = np.array([0, 0, 2, 1, 2]), np.array([1, 2, 0, 0, 0])
    rowptr, col = ref.sym_csr(src, dst, 4)
    assert rowptr.tolist() == [0, 5, 7, 10, 10]
    assert col[0:5].tolist() == [1, 2, 2, 1, 2] and col[5:7].tolist() == [0, 0] and col[7:10].tolist() == [0, 0, 0]


def test_the_lattice_interior_is_the_five_point_stencil_at_a_quarter_of_the_rate():
    src, dst = cases.lattice_edges(12)
    n, side, dt = 144, 12, 0.125                                                     # a power of two: a = dt / 8 exactly
    rowptr, col, E, _ = cases.graph_numbers(src, dst, n)
    assert E == 4 * n and ref.rate(dt, n, E) == dt / 8
    c = np.random.default_rng(3).integers(0, 1000, n).astype(np.float64)            # integers: every sum below is exact
    new = ref.step(c, rowptr, col, ref.rate(dt, n, E))
    grid, got, inner = c.reshape(side, side), new.reshape(side, side), 0
    for i in range(side):
        for j in range(side):
            row = sorted(col[rowptr[i * side + j]:rowptr[i * side + j + 1]].tolist())
            cross = sorted(2 * [(i - 1) * side + j, (i + 1) * side + j, i * side + j - 1, i * side + j + 1])
            if 2 <= i < side - 2 and 2 <= j < side - 2:
                assert row == cross                                                  # the four lattice neighbours, each twice
            if row == cross:
                inner += 1
                want = grid[i, j] + (dt / 4) * (grid[i - 1, j] + grid[i + 1, j] + grid[i, j - 1] + grid[i, j + 1] - 4 * grid[i, j])
                assert got[i, j] == want
    assert inner >= (side - 4) ** 2


@pytest.mark.parametrize("name", ["lattice", "ragged", "hub", "n65", "n1025"])
def test_the_constant_gene_stops_at_the_first_step(name):
    problems, dt = cases.CASES[name]()
    g = cases.GENES.index("constant")
    for src, dst, V in problems:
        n = V.shape[0]
        rowptr, col, E, _ = cases.graph_numbers(src, dst, n)
        r = ref.run(V[:, g].astype(np.float64), rowptr, col, ref.rate(dt, n, E), dt, cases.THRESH, cases.N_ITER)
        assert (r.iterations, r.converged, r.degenerate, r.score) == (1, True, False, dt)
        # the image stays constant up to the rounding of a step, where the entropy is stationary: what is left is the evaluation
        H, S, A = r.parts[-1]
        assert abs(H - math.log(n) / n) <= ref.entropy_bound(n, S, A)


def test_degenerate_genes_and_time_points():
    (src, dst, V), = cases.size_case(65)[0]
    rowptr, col, E, _ = cases.graph_numbers(src, dst, 65)
    r = ref.run(V[:, 0].astype(np.float64), rowptr, col, ref.rate(0.1, 65, E), 0.1, 1e-8, 100)
    assert r.degenerate and math.isnan(r.score) and (r.iterations, r.converged) == (0, False)
    (src, dst, V), = cases.size_case(1)[0]
    assert len(src) == 0
    for g in range(V.shape[1]):                                                      # n < 2 and E = 0: every gene
        r = ref.run(V[:, g].astype(np.float64), *ref.sym_csr(src, dst, 1), 0.0, 0.1, 1e-8, 100)
        assert r.degenerate and math.isnan(r.score) and r.iterations == 0
    (src, dst, V), = cases.CASES["n65"]()[0]
    r = ref.run(V[:, 1].astype(np.float64), rowptr, col, ref.rate(0.1, 65, E), 0.1, 1e-8, 7)      # a cap that bites
    assert (r.iterations, r.converged, r.degenerate) == (7, False, False) and r.score == 0.1 * 7


@pytest.mark.parametrize("name", ["hub", "lattice", "ragged", "n2049"])
def test_dt_at_the_stability_limit_is_refused_and_just_below_it_is_not(name):
    from spadot_amd import stage_ops as ops
    for src, dst, V in cases.CASES[name]()[0]:
        n = V.shape[0]
        _, _, E, deg = cases.graph_numbers(src, dst, n)
        top = ref.max_dt(n, E, deg)
        assert top == ops.sepal_max_dt(n, 2 * E, deg) and abs(top - 2 * E / (n * deg)) <= 4 * U * top
        over = float(np.nextafter(top, np.inf))
        assert ref.stable(top, n, E, deg) and not ref.stable(over, n, E, deg)
        assert ops.sepal_rate(top, n, 2 * E) == ref.rate(top, n, E) and ops.sepal_rate(top, n, 2 * E) * deg < 1.0
        assert not ops.sepal_rate(over, n, 2 * E) * deg < 1.0
    assert ops.sepal_rate(0.1, 5, 0) == 0.0 and ops.sepal_max_dt(5, 0, 0) == float("inf")
    assert cases.HUB_DT < ref.max_dt(300, 418, 120) < cases.DT                       # why the hub has a dt of its own


def test_the_planted_bumps_outlast_the_null_genes():
    """On the 400-spot planted data set the median score of module 0 (a Gaussian bump) exceeds the largest score of every null
    gene that is detected in at least 5 spots.  It does NOT hold against all 200 genes: the five rare genes (the last n_rare,
    detected in 3 spots each) are a few isolated spots, which diffuse as slowly as the `single` gene of the cases and outrank
    every pattern (232 to 358 against a median of 131) -- that is the statistic, a ranking by scale, and the reason why the
    stage is run on genes that a detection filter has passed.  So the assertion is the planted separation without them."""
    raw, runs = cases.planted_raw(), cases.planted_scores()
    module, detected = np.asarray(raw.uns["module"]), (np.asarray(raw.X) > 0).sum(axis=0)
    score = np.array([r.score for r in runs])
    assert all(r.converged or r.degenerate for r in runs)
    null = np.flatnonzero((module == -1) & (detected >= 5))
    rare = np.flatnonzero((module == -1) & (detected > 0) & (detected < 5))
    print("module medians", [float(np.median(score[module == m])) for m in range(4)], "largest null", score[null].max(),
          "rare", score[rare], "iterations", min(r.iterations for r in runs if not r.degenerate), max(r.iterations for r in runs))
    assert null.size == 154 and rare.size == 5
    assert np.median(score[module == 0]) > score[null].max()
    assert score[rare].min() > np.median(score[module == 0])                        # the exception the docstring names
    assert np.isnan(score[(module == -1) & (detected == 0)]).all() and ((module == -1) & (detected == 0)).sum() == 1


def test_the_table_orders_by_score_with_nan_last():
    from spadot_amd.sepal import SepalResult, sepal_table, TABLE_COLUMNS
    it, done = np.array([5, 0, 9, 5, 30], dtype=np.int32), np.array([1, 2, 1, 1, 0], dtype=np.int32)
    H = np.arange(5, dtype=np.float64)
    r = SepalResult(it, done, H, H + 1, np.zeros((3, 5)), np.array([4, 3, 2, 1, 0]), 3, 6, 0.1, 1e-8, 30)
    assert r.converged.tolist() == [True, False, True, True, False] and r.degenerate.tolist() == [False, True, False, False, False]
    assert np.isnan(r.score[1]) and r.score[4] == 0.1 * 30
    tab = sepal_table(r, np.array(["a", "b", "c", "d", "e"]))
    assert tuple(tab.columns) == TABLE_COLUMNS
    assert tab["gene"].tolist() == ["a", "c", "e", "b", "d"]                         # 30, 9, 5 (index 0 before 3), NaN
    assert tab["rank"].tolist() == [1, 2, 3, 4, 0] and tab["converged"].tolist() == [0, 1, 1, 1, 0]
    assert tab["iterations"].tolist() == [30, 9, 5, 5, 0]
    np.testing.assert_array_equal(ref.order(r.score), [4, 2, 0, 3, 1])


def test_the_lds_formula_and_the_stride():
    from spadot_amd import stage_ops as ops
    assert cases.W == ops.SEPAL_THREADS and ops.SEPAL_LDS_BYTES == 512 + 8 * 12 * 1024 == 98816
    assert ops.sepal_lds_bytes(12288) == ops.SEPAL_LDS_BYTES < ops.sepal_lds_bytes(12289)
    desc = np.array([[0, 65, 0, 0, 0, 0, 0, 0], [0, 513, 0, 65, 1, 66, 0, 0]], dtype=np.int64)
    assert ops.sepal_stride(desc) == 513 and ops.sepal_stride(desc, lds_limit=0) == 1026
    assert ops.sepal_stride(desc, lds_limit=512 + 8 * 65) == 513 + 513


def test_command_line_parsing_and_refusals(tmp_path):
    from spadot_amd.cli import build_parser, main
    from spadot_amd.sepal import sepal_stage
    a = build_parser().parse_args(["sepal", "-i", "counts.npz"])
    assert (a.cmd_choice, a.k, a.dt, a.thresh, a.n_iter, a.genes, a.prefix, a.output_dir, a.device) == (
        "sepal", 6, 0.1, 1e-8, 30000, None, "", None, "cuda:0")
    a = build_parser().parse_args(["sepal", "-i", "c.npz", "--genes", "a,b", "--k", "4", "--dt", "0.05", "--thresh", "1e-6",
                                   "--n_iter", "99", "-o", "out", "--prefix", "p_", "--device", "cuda:1"])
    assert (a.genes, a.k, a.dt, a.thresh, a.n_iter, a.output_dir, a.prefix, a.device) == ("a,b", 4, 0.05, 1e-6, 99, "out", "p_",
                                                                                          "cuda:1")
    with pytest.raises(SystemExit) as e:
        main(["sepal", "-i", str(tmp_path / "missing.npz")])
    assert e.value.code == 2
    path = ac.stage_counts(str(tmp_path / "counts.npz"))

    def ns(**kw):
        base = dict(data=path, output_dir=str(tmp_path), prefix="", k=6, dt=0.1, thresh=1e-8, n_iter=100, genes=None,
                    device="cuda:0")
        base.update(kw)
        return argparse.Namespace(**base)

    for kw in (dict(k=0), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("inf")), dict(thresh=-1e-9), dict(thresh=float("nan")),
               dict(n_iter=0)):
        with pytest.raises(ValueError, match="the sepal stage takes"):
            sepal_stage(ns(**kw))
    with pytest.raises(RuntimeError, match="MI355X only"):
        sepal_stage(ns(device="cpu"))


def test_sepal_refuses_host_tensors_without_a_gpu():
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.sepal import diffuse, sepal
    t = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.sepal_steps(t, t, t.long(), t, t.float(), t, np.zeros((1, 8), np.int64), 0.1)
    for call in (sepal, diffuse):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call([(t, t)], [torch.zeros((4, 2))])
