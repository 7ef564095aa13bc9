"""CPU: the silhouette definition (tests/silhouette_ref.py) against sklearn.metrics.silhouette_samples / silhouette_score on the
GPU test's shapes and edge cases, the silhouette rule for k, the command line's `score` subcommand and `analyze --criterion`,
and the refusals that come before any device work."""
import os

import numpy as np
import pytest

import silhouette_cases as cases
import silhouette_ref as ref

ATOL = 1e-12      # the restatement and sklearn differ by <= 6e-16 on these shapes (both fp64, sums in another order)


def _against_sklearn(X, lab):
    from sklearn.metrics import silhouette_samples, silhouette_score
    r = ref.silhouette(X, lab)
    np.testing.assert_allclose(r["samples"], silhouette_samples(X, lab), rtol=0, atol=ATOL)
    assert abs(r["score"] - silhouette_score(X, lab)) <= ATOL
    return r


def test_the_restatement_is_sklearns_silhouette_on_the_edge_call():
    sets, labelings, random = cases.edge_call()
    assert [x.shape for x in sets[:2]] == [(37, 20), (300, 20)]
    for x, ls, rnd in zip(sets, labelings, random):
        assert len(ls) == 3
        for lab in ls:
            r = _against_sklearn(x, lab)
            if rnd:
                assert ref.min_gap(r["means"]).min() > 1e-9
    # what the labelings hold
    r3, r5 = ref.silhouette(sets[0], labelings[0][1]), ref.silhouette(sets[0], labelings[0][2])
    assert r3["sizes"][2] == 1 and r3["samples"][36] == 0.0 and r3["a"][36] == 0.0               # a singleton: s = 0
    assert r5["sizes"][2] == 0 and not np.any(r5["nearest"] == 2)                                   # a label value without points
    assert np.array_equal(sets[0][5], sets[0][6]) and np.array_equal(sets[0][5], sets[0][7])     # three identical points ...
    assert all(l[5] == l[6] == l[7] for l in labelings[0])                                          # ... in one cluster
    for lab in labelings[2]:                                                                        # all points equal
        r = ref.silhouette(sets[2], lab)
        assert not r["a"].any() and not r["b"].any() and not r["samples"].any()
    r = ref.silhouette(sets[3], labelings[3][0])                                                    # two point masses
    assert np.all(r["samples"] == 1.0) and not r["a"].any() and r["score"] == 1.0


@pytest.mark.parametrize("name", [c[0] for c in cases.TILE_CASES])
def test_the_restatement_is_sklearns_silhouette_on_the_tile_cases(name):
    X, lab = cases.tile_case(name)
    _, n, d, K = cases.TILE_CASES[[c[0] for c in cases.TILE_CASES].index(name)]
    assert X.shape == (n, d) and int(lab.max()) + 1 == K and np.array_equal(X, X.astype(np.float32).astype(np.float64))
    if name == "sizes_256_256_1":
        assert np.bincount(lab).tolist() == [256, 256, 1]
    r = _against_sklearn(X, lab)
    assert ref.min_gap(r["means"]).min() > 1e-9


def test_undefined_labelings_have_no_score():
    X = np.arange(12, dtype=np.float64).reshape(6, 2)
    assert np.isnan(ref.silhouette(X, np.zeros(6, dtype=int), K=3)["score"])             # one non-empty cluster
    assert np.isnan(ref.silhouette(X, np.arange(6))["score"])                            # n clusters of one point
    assert np.isfinite(ref.silhouette(X, np.array([0, 0, 1, 1, 4, 4]))["score"])


def test_select_k_silhouette():
    from spadot_amd.utils._analyze_utils import select_k_silhouette, silhouette_table
    s = np.linspace(0.1, 0.2, 17)
    assert select_k_silhouette(s) == 20
    s[3] = s[9] = 0.9                                                 # a tie: the first maximum
    assert select_k_silhouette(s) == 7
    s[3] = np.nan                                                     # NaN is skipped, not propagated
    assert select_k_silhouette(s) == 13
    only = np.full(17, np.nan)
    only[16] = -0.25
    assert select_k_silhouette(only) == 20
    with pytest.raises(ValueError, match="time point E12"):
        select_k_silhouette(np.full(17, np.nan), timepoint="E12")
    with pytest.raises(ValueError, match="one score per k"):
        select_k_silhouette(np.zeros(5))
    tab = silhouette_table(s, 13)
    assert list(tab.columns) == ["clusters", "silhouette", "selected"]
    assert tab["clusters"].tolist() == list(range(4, 21)) and tab["clusters"][tab["selected"]].tolist() == [13]
    assert np.isnan(tab["silhouette"][3])


# ---------------------------------------------------------------------------------------------------------------- parser
def test_parser_takes_score_and_criterion_and_keeps_the_others():
    from spadot_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(["score", "-i", "latent.npz", "--domains", "d.csv"])
    assert (a.cmd_choice, a.data, a.domains, a.output_dir, a.prefix, a.device) == ("score", "latent.npz", "d.csv", None, "", "cuda:0")
    a = p.parse_args(["score", "-i", "latent.npz", "--domains", "d.csv", "-o", "out", "--prefix", "p_", "--device", "cuda:1"])
    assert (a.output_dir, a.prefix, a.device) == ("out", "p_", "cuda:1")
    with pytest.raises(SystemExit):
        p.parse_args(["score", "-i", "latent.npz"])                                  # --domains is required
    a = p.parse_args(["analyze", "-i", "latent.npz"])
    assert (a.criterion, a.n_clusters, a.lineage) == ("elbow", None, False)
    assert p.parse_args(["analyze", "-i", "latent.npz", "--criterion", "silhouette"]).criterion == "silhouette"
    with pytest.raises(SystemExit):
        p.parse_args(["analyze", "-i", "latent.npz", "--criterion", "gap"])
    a = p.parse_args(["markers", "-i", "c.npz", "--domains", "d.csv"])
    assert (a.cmd_choice, a.top) == ("markers", 100) and not hasattr(a, "criterion")


def test_cli_score_reports_a_missing_file(tmp_path, capsys):
    from spadot_amd.cli import main
    latent = os.path.join(str(tmp_path), "latent.npz")
    with pytest.raises(SystemExit) as e:
        main(["score", "-i", latent, "--domains", os.path.join(str(tmp_path), "d.csv")])
    assert e.value.code == 2 and "latent representations does not exist" in capsys.readouterr().err
    np.savez(latent, X=np.zeros((4, 3), dtype=np.float32), timepoint=np.array(["a"] * 4), spatial=np.zeros((4, 2)))
    with pytest.raises(SystemExit) as e:
        main(["score", "-i", latent, "--domains", os.path.join(str(tmp_path), "d.csv")])
    assert e.value.code == 2 and "domains table does not exist" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------- refusals
class _Args:
    def __init__(self, **kw):
        self.__dict__.update(dict(output_dir=None, prefix="", device="cuda:0"), **kw)


def test_analyze_refuses_the_silhouette_criterion_with_given_cluster_counts(tmp_path):
    from spadot_amd.analyze import analyze
    missing = os.path.join(str(tmp_path), "never_read.npz")            # refused before the data is read or a device is asked for
    with pytest.raises(ValueError, match="cannot be combined with --n_clusters"):
        analyze(_Args(data=missing, n_clusters=[5, 6], criterion="silhouette"))
    with pytest.raises(ValueError, match="criterion must be"):
        analyze(_Args(data=missing, n_clusters=None, criterion="gap"))


def _latent_and_table(tmp_path):
    import pandas as pd
    rng = np.random.default_rng(8)
    n = 30
    tp = np.repeat(np.array(["E10", "E12"]), [12, 18])
    rows = rng.permutation(n) + 500                                    # the latents' own row ids, as train writes them
    path = os.path.join(str(tmp_path), "latent.npz")
    np.savez(path, X=rng.standard_normal((n, 6)).astype(np.float32), rows=rows, timepoint=tp, spatial=rng.random((n, 2)))
    order = rng.permutation(n)
    df = pd.DataFrame({"row": rows[order], "timepoint": tp[order], "kmeans": order % 3})
    return path, df, rows, tp


def test_score_refuses_a_malformed_domains_table_before_the_device(tmp_path, monkeypatch):
    import pandas as pd
    import torch
    from spadot_amd.silhouette import _positions, score

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch, "device", no_device)
    path, df, rows, tp = _latent_and_table(tmp_path)
    with pytest.raises(ValueError, match="needs the domains table"):
        score(_Args(data=path, domains=None))
    with pytest.raises(ValueError, match="more than once"):
        score(_Args(data=path, domains=pd.concat([df, df.iloc[:1]], ignore_index=True)))
    with pytest.raises(ValueError, match="has no label"):
        score(_Args(data=path, domains=df.iloc[1:]))
    with pytest.raises(ValueError, match="which the latents do not have"):
        score(_Args(data=path, domains=df.assign(row=df["row"] + 1000)))
    with pytest.raises(ValueError, match="no `kmeans` column"):
        score(_Args(data=path, domains=df.drop(columns="kmeans")))
    bad = df.copy()
    bad.loc[bad["row"] == rows[3], "timepoint"] = "E12"
    with pytest.raises(ValueError, match="time point mismatch at row 3"):
        score(_Args(data=path, domains=bad))
    with pytest.raises(ValueError, match="33 domains"):
        many = os.path.join(str(tmp_path), "many.npz")
        np.savez(many, X=np.zeros((40, 3), dtype=np.float32), timepoint=np.array(["a"] * 40), spatial=np.zeros((40, 2)))
        score(_Args(data=many, domains=pd.DataFrame({"row": np.arange(40), "timepoint": "a", "kmeans": np.arange(40) % 33})))
    csv = os.path.join(str(tmp_path), "domains.csv")
    df.to_csv(csv, index=False)
    with pytest.raises(AssertionError, match="the device was asked for"):      # a well-formed table gets as far as the device
        score(_Args(data=path, domains=csv))
    pos = _positions(df, rows, 30)                                             # row ids -> positions
    np.testing.assert_array_equal(rows[pos["row"].to_numpy()], df["row"].to_numpy())


def test_a_cpu_tensor_is_refused():
    import torch
    from spadot_amd.silhouette import silhouette_many, silhouette_samples
    X = torch.zeros((6, 3))
    with pytest.raises(RuntimeError, match="MI355X only"):
        silhouette_samples(X, np.arange(6) % 2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        silhouette_many([X], [[np.arange(6) % 2]])
