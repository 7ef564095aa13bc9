"""CPU: the markers stage's definition (tests/markers_ref.py) against scipy.stats.mannwhitneyu, Benjamini-Hochberg against a
direct restatement, the stage's loader and its refusals, and the command line's new subcommand."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.stats import mannwhitneyu

import markers_ref as ref


def _cases():
    """~200 small two-group cases: heavy ties (few distinct values, many zeros), all-distinct values, and the degenerate
    ones (all values equal, an empty side, a symmetric split with U1 = mu)."""
    rng = np.random.default_rng(20260)
    out = []
    for i in range(192):
        n = int(rng.integers(3, 60))
        if i % 3 == 0:
            v = rng.permutation(n).astype(np.float32) / 7.0 + 0.125                 # all distinct, no zeros
        elif i % 3 == 1:
            v = rng.integers(0, 4, size=n).astype(np.float32)                        # heavy ties, zeros among them
        else:
            v = np.where(rng.random(n) < 0.7, 0.0, rng.integers(1, 3, size=n) * 0.693).astype(np.float32)
        lab = (rng.random(n) < rng.uniform(0.1, 0.9)).astype(np.int64)
        out.append((v, lab))
    out.append((np.full(9, 1.5, dtype=np.float32), np.arange(9) % 2))               # var = 0
    out.append((np.zeros(7, dtype=np.float32), np.arange(7) % 2))                   # all zero
    out.append((np.arange(6, dtype=np.float32), np.zeros(6, dtype=np.int64)))       # n1 = 0 for domain 1, n2 = 0 for domain 0
    out.append((np.array([1, 2, 3, 4], dtype=np.float32), np.array([1, 0, 0, 1])))  # d = 0
    out.append((np.array([0, 0, 5, 5], dtype=np.float32), np.array([1, 0, 1, 0])))  # d = 0 with ties
    return out


def test_the_restatement_is_scipys_mannwhitneyu():
    worst, checked, degenerate = 0.0, 0, 0
    for v, lab in _cases():
        r = ref.ranksum_timepoint(v[:, None], lab, 2)
        n = v.size
        for k in (0, 1):
            x, y = v[lab == k], v[lab != k]
            u1, score, p = r["U1"][0, k], r["score"][0, k], r["pval"][0, k]
            if x.size == 0 or y.size == 0:
                assert (score, p) == (0.0, 1.0)
                degenerate += 1
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                want = mannwhitneyu(x.astype(np.float64), y.astype(np.float64), alternative="two-sided", method="asymptotic",
                                    use_continuity=True)
            assert u1 == want.statistic
            assert r["r2"][0, k] == 2 * want.statistic + x.size * (x.size + 1)
            d = u1 - x.size * y.size / 2.0
            if np.isnan(want.pvalue) or d == 0 or np.unique(v).size == 1:
                assert (score, p) == (0.0, 1.0)
                degenerate += 1
                continue
            np.testing.assert_allclose(p, want.pvalue, rtol=1e-12, atol=0)
            worst = max(worst, abs(p - want.pvalue) / want.pvalue)
            checked += 1
        assert sum(r["r2"][0]) == n * (n + 1)                     # the ranks 1 .. n, twice
    assert checked >= 350 and degenerate >= 8, (checked, degenerate, worst)


def test_ties_and_twice_ranks_by_hand():
    v = np.array([0, 0, 0, 2, 2, 5, 7, 7, 7, 7], dtype=np.float32)
    tw, ties = ref.twice_ranks(v[:, None])
    np.testing.assert_array_equal(tw[:, 0], [4, 4, 4, 9, 9, 12, 17, 17, 17, 17])
    assert ties == [(27 - 3) + (8 - 2) + (64 - 4)] and isinstance(ties[0], int)


def test_bh_matches_the_direct_form():
    from spadot_amd.markers import bh_adjust
    rng = np.random.default_rng(3)
    for m in (1, 2, 17, 200):
        p = rng.random(m) ** 3
        p[rng.integers(m)] = 1.0
        if m > 2:
            p[:2] = p[2]                                           # equal p-values
        np.testing.assert_allclose(bh_adjust(p), ref.bh(p), rtol=1e-15, atol=0)
        assert np.all(bh_adjust(p) <= 1.0) and np.all(bh_adjust(p) >= p)
    assert bh_adjust(np.zeros(0)).size == 0
    np.testing.assert_allclose(bh_adjust([0.01, 0.04, 0.03, 0.005]), [0.02, 0.04, 0.04, 0.02], rtol=1e-15)


# ---------------------------------------------------------------------------------------------------------------- loader
def _write_inputs(tmp_path, K=3):
    import pandas as pd
    rng = np.random.default_rng(5)
    n, G = 30, 12
    X = sp.random(n, G, density=0.4, random_state=7, format="csr", dtype=np.float32)
    X.data = np.ceil(X.data * 5).astype(np.float32)
    tp = np.repeat(np.array(["E10", "E12"]), [12, 18])
    spatial = rng.random((n, 2))
    path = os.path.join(str(tmp_path), "preprocessed_data.npz")
    np.savez(path, X=rng.standard_normal((n, G)).astype(np.float32), timepoint=tp, spatial=spatial,
             genes=np.array([f"g{i}" for i in range(G)]), counts_data=X.data, counts_indices=X.indices, counts_indptr=X.indptr,
             counts_shape=np.asarray(X.shape, dtype=np.int64))
    order = rng.permutation(n)                                     # the table need not be in row order
    df = pd.DataFrame({"row": order, "timepoint": tp[order], "kmeans": (order * 7 + 1) % K, "pixel_x": spatial[order, 0],
                       "pixel_y": spatial[order, 1]})
    return path, df, X, tp


def test_loader_reads_the_counts_of_a_preprocess_npz(tmp_path):
    from spadot_amd.markers import load_marker_counts, read_domains
    path, df, X, tp = _write_inputs(tmp_path)
    raw, p = load_marker_counts(path)
    assert p == path
    np.testing.assert_array_equal(raw.X.toarray(), X.toarray())    # the raw counts, not the scaled X
    np.testing.assert_array_equal(raw.obs["timepoint"], tp)
    assert raw.var_names[3] == "g3" and raw.obsm["spatial"].shape == (30, 2)
    csv = os.path.join(str(tmp_path), "domains.csv")
    df.to_csv(csv, index=False)
    labels = read_domains(csv, raw.obs["timepoint"])
    np.testing.assert_array_equal(labels, (np.arange(30) * 7 + 1) % 3)
    assert labels.dtype == np.int32
    # a raw-counts npz (X_* keys) still goes through load_counts
    rawp = os.path.join(str(tmp_path), "raw.npz")
    np.savez(rawp, X_data=X.data, X_indices=X.indices, X_indptr=X.indptr, X_shape=np.asarray(X.shape), timepoint=tp,
             spatial=raw.obsm["spatial"])
    np.testing.assert_array_equal(load_marker_counts(rawp)[0].X.toarray(), X.toarray())


def test_loader_refusals(tmp_path):
    import pandas as pd
    from spadot_amd.markers import read_domains
    _, df, _, tp = _write_inputs(tmp_path)
    bad = df.copy()
    bad.loc[bad["row"] == 3, "timepoint"] = "E12"
    with pytest.raises(ValueError, match="time point mismatch at row 3"):
        read_domains(bad, tp)
    with pytest.raises(ValueError, match="more than once"):
        read_domains(pd.concat([df, df.iloc[:1]], ignore_index=True), tp)
    with pytest.raises(ValueError, match="has no label"):
        read_domains(df.iloc[1:], tp)
    with pytest.raises(ValueError, match="names row 30"):
        read_domains(df.assign(row=df["row"] + 1), tp)
    with pytest.raises(ValueError, match="no `kmeans` column"):
        read_domains(df.drop(columns="kmeans"), tp)
    many = df.copy()
    many["kmeans"] = np.where(many["timepoint"] == "E12", many["row"] - 12, 0)      # rows 12 .. 29 -> only 18 domains
    read_domains(many, tp)
    tp33 = np.repeat(np.array(["a"]), 40)
    df33 = pd.DataFrame({"row": np.arange(40), "timepoint": tp33, "kmeans": np.arange(40) % 33})
    with pytest.raises(ValueError, match="33 domains"):
        read_domains(df33, tp33)
    read_domains(df33.assign(kmeans=np.arange(40) % 32), tp33)                      # 32 is admitted
    with pytest.raises(ValueError, match="non-negative"):
        read_domains(df33.assign(kmeans=-1), tp33)


def test_find_markers_refuses_a_cpu_device_before_touching_the_data():
    from spadot_amd.markers import find_markers
    with pytest.raises(ValueError, match="cuda device"):
        find_markers(object(), [0], device="cpu")


# ---------------------------------------------------------------------------------------------------------------- parser
def test_parser_takes_the_markers_subcommand_and_keeps_the_others():
    from spadot_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(["markers", "-i", "c.npz", "--domains", "d.csv"])
    assert (a.cmd_choice, a.data, a.domains, a.output_dir, a.prefix, a.top, a.device) == \
        ("markers", "c.npz", "d.csv", None, "", 100, "cuda:0")
    a = p.parse_args(["markers", "-i", "c.npz", "--domains", "d.csv", "-o", "out", "--prefix", "p_", "--top", "0",
                      "--device", "cuda:1"])
    assert (a.output_dir, a.prefix, a.top, a.device) == ("out", "p_", 0, "cuda:1")
    with pytest.raises(SystemExit):
        p.parse_args(["markers", "-i", "c.npz"])                                    # --domains is required
    a = p.parse_args(["preprocess", "-i", "x.npz"])
    assert (a.cmd_choice, a.prefix, a.feature_selection, a.gene_clusters, a.device) == \
        ("preprocess", "preprocessed_", True, "kmeans", "cuda:0")
    a = p.parse_args(["train", "-i", "x.npz", "--save_model"])
    assert (a.cmd_choice, a.prefix, a.save_model, a.config) == ("train", "", True, None)
    a = p.parse_args(["analyze", "-i", "latent.npz", "--n_clusters", "5,7", "--lineage"])
    assert (a.cmd_choice, a.n_clusters, a.lineage, a.write_tmaps) == ("analyze", [5, 7], True, False)
    assert not hasattr(a, "domains")


def test_cli_reports_a_missing_file(tmp_path, capsys):
    from spadot_amd.cli import main
    with pytest.raises(SystemExit) as e:
        main(["markers", "-i", os.path.join(str(tmp_path), "nope.npz"), "--domains", os.path.join(str(tmp_path), "d.csv")])
    assert e.value.code == 2
    assert "does not exist" in capsys.readouterr().err
