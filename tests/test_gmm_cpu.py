"""CPU: the Gaussian-mixture definition (tests/gmm_ref.py) against sklearn.mixture.GaussianMixture on every fit case of the GPU
test (same centred values, same starts: weights_init / means_init / precisions_init from the one-hot M-step), the BIC formula,
the BIC rule for k, the command line's `--method` and `--criterion bic`, and the refusals that come before any device work."""
import os
import warnings

import numpy as np
import pytest

import gmm_cases as cases
import gmm_ref as ref

TOL = 1e-3
ATOL = 1e-9       # the restatement and sklearn differ by <= 6.1e-13 on converged fits (both fp64, sums in another order)


def _all_cases():
    sets, labelings, Ks = cases.edge_call()
    out = [(f"edge{t}{l}", sets[t], labelings[t][l], Ks[t][l], 100) for t in range(2) for l in range(3)]
    out += [(c[0],) + cases.fit_case(c[0]) + (100,) for c in cases.FIT_CASES]
    out.append(("capped",) + cases.fit_case(cases.CAPPED[0]) + (cases.CAPPED[1],))
    return out


CASES = {c[0]: c[1:] for c in _all_cases()}


def _sklearn(Xc, lab, K, max_iter):
    from sklearn.mixture import GaussianMixture
    p0 = ref.m_step(Xc, ref.one_hot(lab, K))
    prec = np.stack([pc @ pc.T for pc in p0["precisions_cholesky"]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # the capped fit warns that it did not converge
        return GaussianMixture(K, covariance_type="full", reg_covar=1e-6, tol=TOL, max_iter=max_iter, n_init=1,
                               weights_init=p0["weights"] / p0["weights"].sum(), means_init=p0["means"],
                               precisions_init=prec).fit(Xc)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_restatement_is_sklearns_gaussian_mixture(name):
    X, lab, K, max_iter = CASES[name]
    assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
    r = ref.fit(X, lab, K, max_iter=max_iter)
    Xc = r["Xc"]
    g = _sklearn(Xc, lab, K, max_iter)
    assert (r["n_iter"], r["converged"]) == (g.n_iter_, g.converged_)
    assert r["converged"] == (name != "capped")
    diffs = dict(weights=np.abs(g.weights_ - r["weights"]).max(), means=np.abs(g.means_ - r["means_c"]).max(),
                 covariances=np.abs(g.covariances_ - r["covariances"]).max(),
                 resp=np.abs(g.predict_proba(Xc) - r["resp"]).max(), lower_bound=abs(g.lower_bound_ - r["lower_bound"]),
                 labels=int((g.predict(Xc) != r["labels"]).sum()))
    print(name, r["n_iter"], diffs)
    assert max(diffs.values()) <= ATOL, diffs
    # rounding cannot move the stop: the last two |lb - lb_prev| stay clear of tol
    dl = np.abs(np.diff(np.concatenate([[-np.inf], r["lbs"]])))[-2:]
    assert np.min(np.abs(dl - TOL)) >= 1e-6 * TOL, dl
    # the GPU test compares labels where the two largest responsibilities differ by more than 1e-6: at most 1 % are left out
    assert np.mean(ref.label_margin(r["resp"]) <= 1e-6) <= 0.01
    # the BIC / AIC formulas
    assert abs(r["bic"] - g.bic(Xc)) <= 1e-9 * abs(r["bic"]) and abs(r["aic"] - g.aic(Xc)) <= 1e-9 * abs(r["aic"])
    # the rounding bound that the GPU test holds the reported factor to holds for the restatement's own (LAPACK's) factor
    d = X.shape[1]
    res = np.stack([np.abs(pc.T @ c @ pc - np.eye(d)) for c, pc in zip(r["covariances"], r["precisions_cholesky"])])
    bound = np.stack([ref.factor_bound(c, pc) for c, pc in zip(r["covariances"], r["precisions_cholesky"])])
    print(name, "factor: largest residual", res.max(), "largest residual / bound", (res / np.maximum(bound, 1e-300)).max())
    assert np.all(res <= bound)


def test_what_the_cases_hold():
    sets, labelings, Ks = cases.edge_call()
    assert [x.shape for x in sets] == [(37, 3), (300, 3)] and Ks == [[2, 3, 5], [2, 3, 4]]
    assert np.array_equal(sets[0][5], sets[0][6]) and np.array_equal(sets[0][5], sets[0][7])         # three identical points
    assert np.bincount(labelings[0][1], minlength=3)[2] == 1                                             # a component of one point
    assert np.bincount(labelings[0][2], minlength=5)[2] == 0                                             # a label value without points
    assert np.bincount(labelings[1][1], minlength=3)[2] == 3                                             # fewer than d + 1 points
    X, lab, K = cases.fit_case("few_d20")
    assert X.shape == (300, 20) and np.bincount(lab, minlength=3)[2] == 5                               # and in d = 20
    r = ref.fit(sets[0], labelings[0][2], 5)
    assert r["weights"][2] < 1e-15 and np.allclose(r["means"][2], r["mean"])          # its mean is the set's mean (sklearn: the origin)
    assert [cases.fit_case(n)[0].shape[0] for n in ("n255", "n256", "n257", "n770")] == [255, 256, 257, 770]
    assert sorted({cases.fit_case(c[0])[0].shape[1] for c in cases.FIT_CASES}) == [1, 3, 19, 20]
    assert {1, 2, 20, 32} <= {c[3] for c in cases.FIT_CASES}
    iters = {n: ref.fit(*cases.fit_case(n))["n_iter"] for n in ("slow", "fast")}
    assert iters["fast"] == 2 and 40 <= iters["slow"] <= 60, iters


def test_select_k_bic():
    from spadot_amd.utils._analyze_utils import bic_table, select_k_bic
    b = np.linspace(200.0, 100.0, 17)
    assert select_k_bic(b) == 20
    b[3] = b[9] = 5.0                                                 # a tie: the first minimum
    assert select_k_bic(b) == 7
    b[3] = np.nan                                                     # NaN is skipped, not propagated
    assert select_k_bic(b) == 13
    only = np.full(17, np.nan)
    only[16] = 1e9
    assert select_k_bic(only) == 20
    with pytest.raises(ValueError, match="time point E12"):
        select_k_bic(np.full(17, np.nan), timepoint="E12")
    with pytest.raises(ValueError, match="one BIC per k"):
        select_k_bic(np.zeros(5))

    class Fit:
        def __init__(self, k):
            self.bic_, self.aic_, self.log_likelihood_, self.n_iter_, self.converged_ = 10.0 * k, 9.0 * k, -k, k, k != 6
    tab = bic_table([Fit(k) for k in range(4, 21)], 13)
    assert list(tab.columns) == ["clusters", "bic", "aic", "log_likelihood", "n_iter", "converged", "selected"]
    assert tab["clusters"].tolist() == list(range(4, 21)) and tab["clusters"][tab["selected"]].tolist() == [13]
    assert tab["converged"].tolist() == [k != 6 for k in range(4, 21)] and tab["bic"][2] == 60.0


def test_parser_takes_method_and_bic_and_keeps_the_defaults():
    from spadot_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(["analyze", "-i", "latent.npz"])
    assert (a.criterion, a.method, a.n_clusters, a.lineage) == ("elbow", "kmeans", None, False)
    a = p.parse_args(["analyze", "-i", "latent.npz", "--method", "gmm", "--criterion", "bic"])
    assert (a.criterion, a.method) == ("bic", "gmm")
    assert p.parse_args(["analyze", "-i", "latent.npz", "--criterion", "silhouette"]).criterion == "silhouette"
    for bad in (["--criterion", "gap"], ["--method", "dbscan"]):
        with pytest.raises(SystemExit):
            p.parse_args(["analyze", "-i", "latent.npz"] + bad)
    assert not hasattr(p.parse_args(["markers", "-i", "c.npz", "--domains", "d.csv"]), "method")


class _Args:
    def __init__(self, **kw):
        self.__dict__.update(dict(output_dir=None, prefix="", device="cuda:0"), **kw)


def test_analyze_refuses_the_combinations_that_make_no_sense_before_any_device_work(tmp_path):
    from spadot_amd.analyze import analyze
    missing = os.path.join(str(tmp_path), "never_read.npz")            # refused before the data is read or a device is asked for
    with pytest.raises(ValueError, match="needs --method gmm"):
        analyze(_Args(data=missing, n_clusters=None, criterion="bic"))
    with pytest.raises(ValueError, match="needs --method gmm"):
        analyze(_Args(data=missing, n_clusters=None, criterion="bic", method="kmeans"))
    with pytest.raises(ValueError, match="has no WSS"):
        analyze(_Args(data=missing, n_clusters=None, method="gmm"))
    with pytest.raises(ValueError, match="cannot be combined with --n_clusters"):
        analyze(_Args(data=missing, n_clusters=[5, 6], criterion="bic", method="gmm"))
    with pytest.raises(ValueError, match="cannot be combined with --n_clusters"):
        analyze(_Args(data=missing, n_clusters=[5, 6], criterion="silhouette", method="gmm"))
    with pytest.raises(ValueError, match="criterion must be"):
        analyze(_Args(data=missing, n_clusters=None, criterion="gap", method="gmm"))
    with pytest.raises(ValueError, match="method must be"):
        analyze(_Args(data=missing, n_clusters=None, method="dbscan"))


def test_a_shape_outside_the_limits_and_a_cpu_tensor_are_refused():
    import torch
    from spadot_amd import gmm
    for d, K in ((20, 32), (24, 32), (28, 29), (32, 24), (1, 1)):
        gmm.check_shape(d, K)
    for d, K in ((33, 2), (20, 33), (28, 30), (32, 25), (0, 1), (3, 0)):
        with pytest.raises(ValueError, match="outside the limits.*163840 bytes of LDS"):
            gmm.check_shape(d, K)
    X = torch.zeros((6, 3))
    with pytest.raises(RuntimeError, match="MI355X only"):
        gmm.fit_sweep([X], [[np.arange(6) % 2]])
    with pytest.raises(RuntimeError, match="MI355X only"):
        gmm.GaussianMixtureDevice(2).fit(X)


def test_the_restatement_picks_the_planted_k_by_bic():
    """K-means labels from sklearn on the host (the device draws differ; the planted blobs are far apart).  k = 4 .. 9 here: past
    the planted k every further component costs 231 log n more than it gains (measured once over 4 .. 20: the BIC rises
    monotonically from the planted k on, by 1200 to 1500 per component)."""
    from sklearn.cluster import KMeans
    from spadot_amd.utils._analyze_utils import select_k_bic
    X, _ = cases.planted()
    picked = []
    for x in X:
        x = x.astype(np.float64)
        bics = [ref.fit(x, KMeans(k, random_state=1993, n_init=10).fit(x).labels_, k)["bic"] for k in range(4, 10)]
        assert all(b1 > b0 for b0, b1 in zip(bics[int(np.argmin(bics)):], bics[int(np.argmin(bics)) + 1:]))
        picked.append(select_k_bic(bics, 4, 9))
    assert picked == [5, 6, 7]


def test_memberships_written_by_a_stubbed_run_are_read_by_trends(tmp_path, monkeypatch):
    """analyze --method gmm with the device stages replaced by host stand-ins: the files it writes and their layout."""
    import sys
    import types
    import torch
    import spadot_amd.analyze                                              # (the package exports the function under this name)
    from spadot_amd import analyze_ot, gmm, kmeans
    an = sys.modules["spadot_amd.analyze"]
    from spadot_amd.trends import read_lineage
    rng = np.random.default_rng(5)
    X = [x[:60] for x in cases.planted((60, 60, 60), (2, 3, 2))[0]]
    f = tmp_path / "latent.npz"
    tp, rows = cases.write_latent(f, X)

    class KM:
        def __init__(self, lab):
            self.labels_, self.inertia_, self.cluster_centers_, self.n_iter_ = lab, 1.0, None, 1

    def km_sweep(Xs, ks, **kw):
        return [{k: KM(np.arange(x.shape[0]) % k) for k in kt} for x, kt in zip(Xs, ks)]

    def gm_sweep(Xs, labelings, n_components=None, resp_for=None, **kw):
        out = []
        for x, ls, kt in zip(Xs, labelings, n_components):
            fits = []
            for lab, k in zip(ls, kt):
                r = ref.fit(np.asarray(x.cpu(), dtype=np.float64), lab, k)
                fits.append(gmm.GMMResult(weights_=r["weights"], means_=r["means"], covariances_=r["covariances"],
                                          precisions_cholesky_=r["precisions_cholesky"], bic_=r["bic"], aic_=r["aic"],
                                          log_likelihood_=r["log_likelihood"], n_iter_=r["n_iter"], converged_=r["converged"],
                                          labels_=r["labels"], resp_=r["resp"] if resp_for else None))
            out.append(fits)
        return out

    monkeypatch.setattr(torch, "device", lambda s: types.SimpleNamespace(type="cuda"))
    monkeypatch.setattr(torch, "as_tensor", lambda x, device=None, **kw: torch.from_numpy(np.asarray(x)))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(an._analyze_utils, "have_matplotlib", lambda: False)    # the plots are not what this test is about
    monkeypatch.setattr(kmeans, "fit_sweep", km_sweep)
    monkeypatch.setattr(gmm, "fit_sweep", gm_sweep)
    monkeypatch.setattr(analyze_ot, "write_transition_tables",
                        lambda out, latents, labels, tps, **kw: [np.eye(int(a.max()) + 1, int(b.max()) + 1)
                                                                  for a, b in zip(labels[:-1], labels[1:])])
    res = an.analyze(_Args(data=str(f), output_dir=str(tmp_path / "out"), method="gmm", n_clusters=[2, 3, 2]))
    assert res["method"] == "gmm" and res["n_clusters"] == [2, 3, 2] and set(res["bic"]) == {"E1", "E2", "E3"}
    files = set(os.listdir(tmp_path / "out"))
    assert {"domains.csv", "memberships.npz", "gmm.npz"} <= files and not any("BIC" in n or "WSS" in n for n in files)
    M, names = read_lineage(str(tmp_path / "out" / "memberships.npz"), tp)
    assert names.tolist() == ["E1_0", "E1_1", "E2_0", "E2_1", "E2_2", "E3_0", "E3_1"] and M.shape == (180, 7)
    np.testing.assert_allclose(M.sum(1), 1.0, rtol=0, atol=1e-12)
    assert not M[tp == "E1", 2:].any() and not M[tp == "E2", :2].any() and not M[tp == "E2", 5:].any() and not M[tp == "E3", :5].any()
    np.testing.assert_array_equal(M, res["memberships"]["X"])
    import pandas as pd
    dom = pd.read_csv(tmp_path / "out" / "domains.csv")
    assert list(dom.columns) == ["row", "timepoint", "kmeans", "pixel_x", "pixel_y"]
    np.testing.assert_array_equal(dom["kmeans"].to_numpy(), np.concatenate([M[tp == t].argmax(1) - o for t, o in
                                                                             (("E1", 0), ("E2", 2), ("E3", 5))]))
    z = np.load(tmp_path / "out" / "gmm.npz")
    assert z["timepoints"].tolist() == ["E1", "E2", "E3"] and z["means_E2"].shape == (3, 20) and z["covariances_E3"].shape == (2, 20, 20)
    assert abs(z["weights_E1"].sum() - 1.0) < 1e-12
