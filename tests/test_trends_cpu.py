"""CPU: the restatement of the trends stage (tests/trends_ref.py) against scipy.stats.pearsonr and numpy.average, its edge
cases, and the host logic of spadot_amd.trends (row matching, the files, the parser) with the device calls replaced by the
restatement."""
import argparse
import os

import numpy as np
import pytest
import scipy.sparse as sp

import trends_ref as ref


def _small():
    """The recipe of the markers tests: 37 + 300 spots, 40 genes, Poisson 0.6 thinned by half, a filler gene that makes the row
    totals equal; F random with every 7th row zero."""
    rng = np.random.default_rng(1993)
    n0, n1, G = 37, 300, 40
    n = n0 + n1
    X = rng.poisson(0.6, size=(n, G)).astype(np.float32) * (rng.random((n, G)) < 0.5)
    tp = np.repeat(np.array(["d0", "d1"]), [n0, n1])
    X[:, 8] = 0                                            # all zero everywhere
    X[:, 39] = 0
    X[:, 39] = 200 - X.sum(1)
    assert X.min() >= 0
    F = rng.random((n, 4))
    F[::7] = 0.0
    return X, tp, F


def _values(X, tp):
    V = ref.lognorm(X, np.asarray(X, dtype=np.float64).sum(1))
    return [V[tp == t] for t in dict.fromkeys(tp.tolist())]


def _split(M, tp):
    return [M[tp == t] for t in dict.fromkeys(tp.tolist())]


def test_restatement_against_scipy_pearsonr_and_numpy_average():
    from scipy.stats import pearsonr
    X, tp, F = _small()
    Vs, Fs = _values(X, tp), _split(F, tp)
    got = ref.fate_drivers(Vs, Fs)
    dr, dp, ratio, checked = 0.0, 0.0, np.inf, 0
    for t, (V, Ft) in enumerate(zip(Vs, Fs)):
        valid = Ft.sum(1) != 0
        assert got["n_valid"][t] == valid.sum()
        Vd = V[valid].astype(np.float64)
        for g in range(V.shape[1]):
            x = Vd[:, g]
            if np.ptp(x) == 0:                             # scipy: NaN; here the zero-variance rule
                assert np.all(got["r"][t, g] == 0) and np.all(got["pval"][t, g] == 1)
                continue
            ratio = min(ratio, ((x - x.mean()) ** 2).sum() / (x * x).sum())
            for k in range(Ft.shape[1]):
                want = pearsonr(x, Ft[valid, k])
                dr = max(dr, abs(got["r"][t, g, k] - want[0]))
                dp = max(dp, abs(got["pval"][t, g, k] - want[1]) / want[1])
                checked += 1
    print(f"max |dr| = {dr:.3g}, max rel dp = {dp:.3g}, smallest SSv / M2 = {ratio:.3g} over {checked} tests")
    assert checked >= 2 * 38 * 4
    assert dr <= 1e-10 and dp <= 1e-8

    W = np.random.default_rng(5).random((X.shape[0], 3))
    W[::5] = 0.0
    Ws = _split(W, tp)
    tr = ref.gene_trends(Vs, Ws)
    for t, (V, Wt) in enumerate(zip(Vs, Ws)):
        Vd = V.astype(np.float64)
        for c in range(3):
            mean = np.average(Vd, axis=0, weights=Wt[:, c])
            var = np.average((Vd - mean) ** 2, axis=0, weights=Wt[:, c])
            np.testing.assert_allclose(tr["mean"][t, :, c], mean, rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(tr["var"][t, :, c], var, rtol=1e-9, atol=1e-13)
            np.testing.assert_allclose(tr["pct"][t, :, c], np.average(Vd > 0, axis=0, weights=Wt[:, c]), rtol=1e-12)
        np.testing.assert_allclose(tr["baseline"][t], Vd.mean(0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(tr["change"], tr["mean"][1] - tr["mean"][0], rtol=0, atol=0)


def test_zero_variance_small_time_points_and_bh_families():
    rng = np.random.default_rng(3)
    n, G = 50, 6
    V = rng.random((n, G)).astype(np.float32)
    F = rng.random((n, 2))
    F[::7] = 0.0
    valid = F.sum(1) != 0
    V[valid, 0] = np.float32(1.25)                         # constant over the valid spots, not over all
    V[~valid, 0] = np.float32(3.0)
    V[:, 1] = 0                                            # unexpressed
    V[valid, 2] = 0                                        # expressed only where no fate is defined
    V[:, 3] = (F[:, 0] * 2 + 1).astype(np.float32)         # r = 1 up to the rounding of v
    got = ref.fate_drivers([V], [F])
    for g in (0, 1, 2):
        assert np.all(got["r"][0, g] == 0) and np.all(got["pval"][0, g] == 1)
    assert np.all(got["padj"][0, [1, 2]] == 1)
    assert got["r"][0, 3, 0] > 1 - 1e-6 and got["pval"][0, 3, 0] < 1e-100
    fam = np.array([0, 3, 4, 5])                           # genes with a nonzero among the valid spots: one BH family
    for k in range(2):
        np.testing.assert_allclose(got["padj"][0, fam, k], ref.bh(got["pval"][0, fam, k]), rtol=1e-14)
    # a fate column that is constant over the valid spots
    Fc = F.copy()
    Fc[valid, 1] = 0.5
    got = ref.fate_drivers([V], [Fc])
    assert np.all(got["r"][0, :, 1] == 0) and np.all(got["pval"][0, :, 1] == 1)
    # n' < 3
    Fs = np.zeros((n, 2))
    Fs[[4, 9]] = [[0.5, 0.5], [1.0, 0.0]]
    got = ref.fate_drivers([V], [Fs])
    assert got["n_valid"][0] == 2
    assert np.all(got["r"] == 0) and np.all(got["pval"] == 1) and np.all(got["padj"] == 1)
    # a column of W without mass: NaN, and change skips it
    W = rng.random((n, 2))
    tr = ref.gene_trends([V, V], [W * [1, 0], W])
    assert np.all(np.isnan(tr["mean"][0, :, 1])) and np.all(np.isnan(tr["var"][0, :, 1])) and np.all(np.isnan(tr["pct"][0, :, 1]))
    assert np.all(tr["change"][:, 1] == 0) and np.all(np.isfinite(tr["change"][:, 0]))


# ---------------------------------------------------------------------------------------------------------------- host logic
def _stub(monkeypatch, seen):
    """gene_trends / fate_drivers replaced by the restatement on the host: what the stage hands over is kept in `seen`."""
    from spadot_amd import trends as tr
    from spadot_amd.utils._preprocess_utils import timepoint_order

    def pieces(raw):
        tp = np.asarray(raw.obs["timepoint"]).astype(str)
        tps = timepoint_order(tp)
        X = np.asarray(raw.X.todense(), dtype=np.float64)
        V = ref.lognorm(X, X.sum(1))
        return tp, tps, [V[tp == t] for t in tps]

    def gene_trends(raw, W, names=None, device="cuda:0"):
        seen["W"] = np.array(W)
        tp, tps, Vs = pieces(raw)
        out = ref.gene_trends(Vs, [W[tp == t] for t in tps])
        out.update(names=np.asarray(names), genes=raw.var_names, timepoints=tps, timings={})
        return out

    def fate_drivers(raw, F, names=None, device="cuda:0"):
        seen["F"] = np.array(F)
        tp, tps, Vs = pieces(raw)
        out = ref.fate_drivers(Vs, [F[tp == t] for t in tps])
        out.update(names=np.asarray(names), genes=raw.var_names, timepoints=tps, timings={})
        return out

    monkeypatch.setattr(tr, "gene_trends", gene_trends)
    monkeypatch.setattr(tr, "fate_drivers", fate_drivers)
    return tr


def _files(d, tp_rows, rows=None, tp_file=None, seed=0):
    """counts.npz with the time points `tp_rows`, and a trajectories / fates pair whose `rows` is `rows` (default: analyze's
    order, the time points sorted)."""
    rng = np.random.default_rng(seed)
    tp_rows = np.asarray(tp_rows)
    n, G = tp_rows.size, 7
    X = sp.csr_matrix(rng.poisson(1.0, size=(n, G)).astype(np.float32))
    counts = str(d / "counts.npz")
    np.savez(counts, X_data=X.data, X_indices=X.indices, X_indptr=X.indptr, X_shape=np.asarray(X.shape), timepoint=tp_rows,
             spatial=rng.random((n, 2)), genes=np.array([f"g{i}" for i in range(G)]))
    Wfull, Ffull = rng.random((n, 3)), rng.random((n, 2))
    if rows is None:
        rows = np.concatenate([np.flatnonzero(tp_rows == t) for t in sorted(set(tp_rows.tolist()))])
    rows = np.asarray(rows)
    ok = np.clip(rows, 0, n - 1)
    tpf = tp_rows[ok] if tp_file is None else np.asarray(tp_file)
    traj, fates = str(d / "trajectories.npz"), str(d / "fates.npz")
    np.savez_compressed(traj, X=Wfull[ok], rows=rows, timepoint=tpf, names=np.array(["a_0", "a_1", "b_0"]))
    np.savez_compressed(fates, X=Ffull[ok], rows=rows, timepoint=tpf, names=np.array(["b_0", "b_1"]))
    return counts, traj, fates, Wfull, Ffull


TP = np.array(["late"] * 4 + ["early"] * 5 + ["late"] * 3)       # first appearance: late, early; sorted: early, late


def test_rows_are_matched_by_id_not_by_position(tmp_path, monkeypatch):
    import pandas as pd
    seen = {}
    tr = _stub(monkeypatch, seen)
    counts, traj, fates, W, F = _files(tmp_path, TP)
    out = str(tmp_path / "out")
    res = tr.trends(argparse.Namespace(data=counts, trajectories=traj, fates=fates, output_dir=out, prefix="p_", top=3,
                                       device="cuda:0"))
    np.testing.assert_array_equal(seen["W"], W)            # analyze's sorted order undone
    np.testing.assert_array_equal(seen["F"], F)
    assert [str(t) for t in res["timepoints"]] == ["late", "early"]
    assert set(os.listdir(out)) == {"p_trends.npz", "p_trends_top.csv", "p_drivers.npz", "p_drivers_late.csv",
                                    "p_drivers_early.csv"}
    z = np.load(os.path.join(out, "p_trends.npz"), allow_pickle=False)
    assert set(z.files) == {"mean", "var", "pct", "delta", "baseline", "change", "names", "genes", "timepoints"}
    assert z["mean"].shape == (2, 7, 3) and z["baseline"].shape == (2, 7) and z["change"].shape == (7, 3)
    assert z["names"].tolist() == ["a_0", "a_1", "b_0"] and z["timepoints"].tolist() == ["late", "early"]
    d = np.load(os.path.join(out, "p_drivers.npz"), allow_pickle=False)
    assert set(d.files) == {"r", "pval", "padj", "n_valid", "names", "genes", "timepoints"}
    assert d["r"].shape == (2, 7, 2) and d["n_valid"].tolist() == [7, 5]
    top = pd.read_csv(os.path.join(out, "p_trends_top.csv"))
    assert list(top.columns) == ["trajectory", "gene", "change", "mean_late", "mean_early"] and len(top) == 3 * 3
    for c, name in enumerate(["a_0", "a_1", "b_0"]):
        part = top[top["trajectory"] == name]
        want = np.lexsort((np.arange(7), -np.abs(res["change"][:, c])))[:3]
        assert part["gene"].tolist() == [f"g{i}" for i in want]
        np.testing.assert_allclose(part["change"].to_numpy(), res["change"][want, c], rtol=1e-15)
    drv = pd.read_csv(os.path.join(out, "p_drivers_early.csv"))
    assert list(drv.columns) == ["gene", "fate", "r", "pval", "padj"] and len(drv) == 2 * 3
    for k, name in enumerate(["b_0", "b_1"]):
        part = drv[drv["fate"] == name]
        want = np.lexsort((np.arange(7), -res["r"][1][:, k]))[:3]
        assert part["gene"].tolist() == [f"g{i}" for i in want]

    # a shuffled `rows` gives the same arrays
    rng = np.random.default_rng(1)
    d2 = tmp_path / "shuffled"
    d2.mkdir()
    counts2, traj2, fates2, _, _ = _files(d2, TP, rows=rng.permutation(TP.size))
    again = tr.trends(argparse.Namespace(data=counts2, trajectories=traj2, fates=fates2, output_dir=str(d2 / "out"), prefix="",
                                         top=0, device="cuda:0"))
    for key in ("mean", "var", "pct", "delta", "baseline", "change", "r", "pval", "padj", "n_valid"):
        assert again[key].tobytes() == res[key].tobytes(), key
    assert len(pd.read_csv(str(d2 / "out" / "trends_top.csv"))) == 3 * 7          # top = 0: all genes


def test_only_one_of_the_two_inputs(tmp_path, monkeypatch):
    seen = {}
    tr = _stub(monkeypatch, seen)
    counts, traj, fates, W, F = _files(tmp_path, TP)
    res = tr.trends(argparse.Namespace(data=counts, trajectories=None, fates=fates, output_dir=str(tmp_path / "f"), prefix="",
                                       top=100, device="cuda:0"))
    assert "F" in seen and "W" not in seen and "r" in res and "mean" not in res
    assert set(os.listdir(tmp_path / "f")) == {"drivers.npz", "drivers_late.csv", "drivers_early.csv"}


@pytest.mark.parametrize("case,match", [("missing", "row 11 of the data is missing"), ("duplicate", "row 2 appears more than once"),
                                        ("mismatch", "time point mismatch at row 4"), ("range", "names row 12")])
def test_bad_rows_are_refused_with_the_first_offender(tmp_path, monkeypatch, case, match):
    seen = {}
    tr = _stub(monkeypatch, seen)
    n = TP.size
    rows, tp_file = np.arange(n), None
    if case == "missing":
        rows = np.arange(n - 1)
    elif case == "duplicate":
        rows = np.concatenate([np.arange(n), [2]])
    elif case == "mismatch":
        tp_file = TP.copy()
        tp_file[4] = "late"                                # row 4 is `early` in the data
    else:
        rows = np.concatenate([np.arange(n - 1), [12]])
    counts, traj, fates, _, _ = _files(tmp_path, TP, rows=rows, tp_file=tp_file)
    with pytest.raises(ValueError, match=match):
        tr.trends(argparse.Namespace(data=counts, trajectories=traj, fates=None, output_dir=str(tmp_path / "o"), prefix="",
                                     top=100, device="cuda:0"))
    with pytest.raises(ValueError, match=match):
        tr.trends(argparse.Namespace(data=counts, trajectories=None, fates=fates, output_dir=str(tmp_path / "o"), prefix="",
                                     top=100, device="cuda:0"))
    assert seen == {}


def test_numeric_time_points_are_compared_as_strings(tmp_path, monkeypatch):
    seen = {}
    tr = _stub(monkeypatch, seen)
    tp = np.array([2, 2, 0, 0, 0, 1, 1])
    counts, traj, fates, W, _ = _files(tmp_path, tp, tp_file=np.array(["0", "0", "0", "1", "1", "2", "2"]))
    res = tr.trends(argparse.Namespace(data=counts, trajectories=traj, fates=None, output_dir=str(tmp_path / "o"), prefix="",
                                       top=100, device="cuda:0"))
    np.testing.assert_array_equal(seen["W"], W)
    assert [str(t) for t in res["timepoints"]] == ["2", "0", "1"]


def test_parser_and_argument_checks(tmp_path, monkeypatch):
    from spadot_amd.cli import build_parser
    a = build_parser().parse_args(["trends", "-i", "counts.npz"])
    assert a.cmd_choice == "trends" and a.data == "counts.npz" and a.trajectories is None and a.fates is None
    assert a.top == 100 and a.prefix == "" and a.device == "cuda:0" and a.output_dir is None
    a = build_parser().parse_args(["trends", "-i", "c.npz", "--trajectories", "t.npz", "--fates", "f.npz", "--top", "0", "-o", "d",
                                   "--prefix", "x_", "--device", "cuda:1"])
    assert (a.trajectories, a.fates, a.top, a.output_dir, a.prefix, a.device) == ("t.npz", "f.npz", 0, "d", "x_", "cuda:1")
    seen = {}
    tr = _stub(monkeypatch, seen)
    counts, traj, fates, _, _ = _files(tmp_path, TP)
    with pytest.raises(ValueError, match="trajectories.npz and / or fates.npz"):
        tr.trends(argparse.Namespace(data=counts, trajectories=None, fates=None, output_dir=str(tmp_path), prefix="", top=100,
                                     device="cuda:0"))
    with pytest.raises(ValueError, match="top must be 0"):
        tr.trends(argparse.Namespace(data=counts, trajectories=traj, fates=None, output_dir=str(tmp_path), prefix="", top=-1,
                                     device="cuda:0"))
    assert seen == {}


def test_command_line_reports_a_missing_file(tmp_path, capsys):
    from spadot_amd.cli import main
    counts, traj, _, _, _ = _files(tmp_path, TP)
    for argv in (["trends", "-i", str(tmp_path / "nothing.npz"), "--trajectories", traj],
                 ["trends", "-i", counts, "--fates", str(tmp_path / "nothing.npz")]):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2
        assert "does not exist" in capsys.readouterr().err


def test_planted_modules_are_recovered_by_the_restatement():
    """The expectations of the end-to-end GPU tests, on the host.  With this draw the smallest planted r is 0.517 and the largest
    other r 0.121, every planted padj is below 1e-26, the smallest planted delta is 1.27 and the largest other delta 0.27."""
    X, tp, F, W = ref.planted()
    Vs = _values(X, tp)
    dr = ref.fate_drivers(Vs, _split(F, tp))
    tr = ref.gene_trends(Vs, _split(W, tp))
    for t in range(2):
        for k, module in ((0, range(0, 10)), (1, range(10, 20))):
            module = list(module)
            rest = [g for g in range(60) if g not in module]
            assert sorted(np.argsort(-dr["r"][t, :, k])[:10].tolist()) == module
            assert dr["r"][t, module, k].min() > 0.5 and dr["r"][t, rest, k].max() < 0.15
            assert dr["padj"][t, module, k].max() < 1e-25
            assert sorted(np.argsort(-tr["delta"][t, :, k])[:10].tolist()) == module
            assert tr["delta"][t, module, k].min() > 1.2 and tr["delta"][t, rest, k].max() < 0.3
