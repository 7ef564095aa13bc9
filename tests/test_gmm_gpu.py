"""The Gaussian-mixture kernels on the MI355X against the numpy restatement of their definition (tests/gmm_ref.py, pinned to
sklearn by tests/test_gmm_cpu.py): one M-step from given responsibilities and one E-step from given parameters with rounding
bounds, whole fits, bitwise repeatability, the refusals, and `analyze --method gmm` end to end (`--criterion bic`, and
`--criterion silhouette --lineage`).

Bounds (u = 2^-53, n_blk = the number of 256-point blocks, whose partial sums are added in ascending order):
  moment sums   |delta| <= 4 (256 + n_blk + 4) u sum_i r_ik |x_ia x_ib|   (one or no coordinate factor for sum r x and sum r)
  covariance    the same constant times sum r |x_a x_b| / nk + |mu_a mu_b|
  lp_ik         |delta| <= 4 (d + 4)^2 u A_ik, A_ik = sum_j (sum_a |x_ia - mu_ka| |P_k,aj|)^2 / 2 + sum_j |log P_k,jj| + d log(2 pi) / 2
                + |log w_k|;  norm_i is held to the largest bound of its row
Whole fits: n_iter_, converged_ and labels_ (where the restatement's two largest responsibilities differ by more than 1e-6) are
equal; lower_bound_, weights, means (relative to the data's scale), covariances (relative to max |Sigma|), responsibilities and the
relative BIC are held to 1e-9.  A fit that ends at max_iter without converging is held to 100 x the difference between the
restatement on the rows as given and on the rows reversed (a pure change of summation order), at least 1e-9.
The sets of one call share their dimension, so the edge call holds 37 x 3 and 300 x 3; 300 x 20 with a component of fewer than
d + 1 points is the fit case few_d20."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gmm_cases as cases
import gmm_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
FIELDS = ("weights_", "means_", "covariances_", "precisions_cholesky_", "labels_", "resp_")
SCALARS = ("lower_bound_", "n_iter_", "converged_", "log_likelihood_", "bic_", "aic_")


def _dev(x, dtype=torch.float64):
    return torch.as_tensor(x, dtype=dtype, device=DEV)


def _same_bits(r, q):
    return all(np.array_equal(getattr(r, f), getattr(q, f)) for f in FIELDS if getattr(r, f) is not None) \
        and all(getattr(r, f) == getattr(q, f) for f in SCALARS) and (r.resp_ is None) == (q.resp_ is None)


def _metrics(got, want):
    """The normalised differences of a fit (dict `got` in the restatement's keys) from the restatement `want`."""
    scale = max(float(np.abs(want["Xc"]).max()), 1.0)
    return dict(lower_bound=abs(got["lower_bound"] - want["lower_bound"]) / max(1.0, abs(want["lower_bound"])),
                weights=float(np.abs(got["weights"] - want["weights"]).max()),
                means=float(np.abs(got["means"] - want["means"]).max()) / scale,
                covariances=float(np.abs(got["covariances"] - want["covariances"]).max()) / float(np.abs(want["covariances"]).max()),
                resp=float(np.abs(got["resp"] - want["resp"]).max()),
                bic=abs(got["bic"] - want["bic"]) / abs(want["bic"]))


def _as_dict(r):
    return dict(lower_bound=r.lower_bound_, weights=r.weights_, means=r.means_, covariances=r.covariances_, resp=r.resp_,
                bic=r.bic_)


def _compare_fit(name, got, want, tol=1e-9):
    m = _metrics(_as_dict(got), want)
    print(f"{name}: n_iter {got.n_iter_} / {want['n_iter']}  " + "  ".join(f"{k} {v:.2e}" for k, v in m.items()) + f"  tol {tol:.1e}")
    assert (got.n_iter_, got.converged_) == (want["n_iter"], want["converged"])
    assert max(m.values()) <= tol, m
    sure = ref.label_margin(want["resp"]) > 1e-6
    assert sure.mean() >= 0.99
    np.testing.assert_array_equal(got.labels_[sure], want["labels"][sure])
    assert got.labels_.dtype == np.int32 and got.resp_.dtype == np.float64
    n, (K, d) = want["Xc"].shape[0], got.means_.shape
    assert got.log_likelihood_ == pytest.approx(want["log_likelihood"], rel=1e-9)
    assert got.aic_ == -2.0 * got.log_likelihood_ + 2.0 * ref.n_parameters(K, d)
    assert got.bic_ == -2.0 * got.log_likelihood_ + ref.n_parameters(K, d) * np.log(n)
    np.testing.assert_allclose(got.resp_.sum(1), 1.0, rtol=0, atol=1e-12)
    res, bound = np.empty((K, d, d)), np.empty((K, d, d))
    for k in range(K):                                   # the factor that is reported is the factor of the covariance that is,
        pc, cov = got.precisions_cholesky_[k], got.covariances_[k]                  # within gmm_ref.factor_bound's rounding bound
        res[k], bound[k] = np.abs(pc.T @ cov @ pc - np.eye(d)), ref.factor_bound(cov, pc)
        assert not np.tril(pc, -1).any()
    print(f"{name}: largest |P^T Sigma P - I| {res.max():.2e}, / bound {np.max(res / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(res <= bound)                          # a bound of exactly 0 (a diagonal Sigma) admits only an exact 0


@pytest.fixture(scope="module")
def edge():
    """The edge call, fitted once: (sets, labelings, Ks, results, references)."""
    from spadot_amd.gmm import fit_sweep
    sets, labelings, Ks = cases.edge_call()
    res = fit_sweep([_dev(x) for x in sets], labelings, Ks, resp_for=True)
    want = [[ref.fit(x, lab, K) for lab, K in zip(ls, kt)] for x, ls, kt in zip(sets, labelings, Ks)]
    return sets, labelings, Ks, res, want


# ---------------------------------------------------------------------------------------------------------------- single steps
STEP_CASES = ["edge01", "edge02", "edge11", "few_d20", "n255", "n256", "n257", "n770", "d1", "d19", "k1", "k32_d20", "k32_d3"]


def _step_case(name):
    if name.startswith("edge"):
        sets, labelings, Ks = cases.edge_call()
        t, l = int(name[4]), int(name[5])
        return sets[t], labelings[t][l], Ks[t][l]
    return cases.fit_case(name)


@pytest.mark.parametrize("name", STEP_CASES)
def test_one_m_step_and_one_e_step_within_their_rounding_bounds(name):
    from spadot_amd.gmm import GMMResult, estep_many, m_step_many
    X, lab, K = _step_case(name)
    w3 = ref.fit(X, lab, K, stop_after=3)                # the restatement's parameters and responsibilities after 3 iterations
    Xc, n, d = w3["Xc"], X.shape[0], X.shape[1]
    n_blk = (n + 255) // 256
    assert n_blk <= 8
    cm = 4.0 * (256 + n_blk + 4) * U
    # M-step from the responsibilities, on identical centred inputs (the restatement's mean is handed over)
    want = ref.m_step(Xc, w3["resp"])
    got = m_step_many([_dev(X)], [[w3["resp"]]], centers=[w3["mean"]])[0][0]
    tiny = 1e-300                                        # a bound of exactly 0 (no mass at all) admits only an exact 0
    ratios = dict(s0=np.max(np.abs(got["s0"] - want["s0"]) / (cm * want["s0"] + tiny)),
                  s1=np.max(np.abs(got["s1"] - want["s1"]) / (cm * want["a1"] + tiny)),
                  s2=np.max(np.abs(got["s2"] - want["s2"]) / (cm * want["a2"] + tiny)))
    mumu = np.abs(want["means"][:, :, None] * want["means"][:, None, :])
    ratios["cov"] = np.max(np.abs(got["covariances"] - want["covariances"]) / (cm * (want["a2"] / want["nk"][:, None, None] + mumu) + tiny))
    ratios["mean"] = np.max(np.abs(got["means_c"] - want["means"]) / (cm * want["a1"] / want["nk"][:, None] + tiny))
    ratios["weight"] = np.max(np.abs(got["weights"] - want["weights"]) / (cm * want["weights"]))
    # E-step from the restatement's parameters
    lp, norm, log_resp, A = ref.e_step(Xc, w3["weights"], w3["means_c"], w3["precisions_cholesky"])
    model = GMMResult(weights_=w3["weights"], means_centred_=w3["means_c"], center_=w3["mean"],
                      precisions_cholesky_=w3["precisions_cholesky"])
    e = estep_many([_dev(X)], [[model]], resp=True, lp=True)[0][0]
    bound = 4.0 * (d + 4) ** 2 * U * A
    ratios["lp"] = np.max(np.abs(e["lp"] - lp) / bound)
    ratios["norm"] = np.max(np.abs(e["norm"] - norm) / bound.max(1))
    print(name, "largest |delta| / bound:", "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    np.testing.assert_allclose(e["resp"], np.exp(log_resp), rtol=0, atol=1e-9)
    sure = ref.label_margin(np.exp(log_resp)) > 1e-6
    np.testing.assert_array_equal(e["labels"][sure], np.argmax(log_resp, axis=1)[sure])


# ---------------------------------------------------------------------------------------------------------------- whole fits
def test_edge_call_matches_the_restatement(edge):
    sets, labelings, Ks, res, want = edge
    assert [len(r) for r in res] == [3, 3]
    for t in range(2):
        for l in range(3):
            _compare_fit(f"edge{t}{l}", res[t][l], want[t][l])
    empty = res[0][2]                                    # the label value without points: weight 10 eps / n, mean = the set's mean
    assert empty.weights_[2] < 1e-15 and np.array_equal(empty.means_[2], empty.center_) and not empty.resp_[:, 2].any()
    np.testing.assert_allclose(empty.covariances_[2], 1e-6 * np.eye(3), rtol=0, atol=1e-18)
    one = res[0][1]                                      # the component of one point keeps it
    assert one.labels_[36] == 2 and (one.labels_ == 2).sum() == 1


@pytest.mark.parametrize("name", [c[0] for c in cases.FIT_CASES])
def test_fit_cases_match_the_restatement(name):
    from spadot_amd.gmm import fit_sweep
    X, lab, K = cases.fit_case(name)
    got = fit_sweep([_dev(X)], [[lab]], [[K]], resp_for=True)[0][0]
    _compare_fit(name, got, ref.fit(X, lab, K))


def test_a_fit_that_ends_at_max_iter_is_held_to_the_reordering_difference():
    from spadot_amd.gmm import fit_sweep
    name, max_iter = cases.CAPPED
    X, lab, K = cases.fit_case(name)
    want = ref.fit(X, lab, K, max_iter=max_iter)
    rev = ref.fit(X[::-1], lab[::-1], K, max_iter=max_iter)
    rev = dict(rev, resp=rev["resp"][::-1])
    reorder = max(_metrics(rev, want).values())
    tol = max(1e-9, 100.0 * reorder)
    print(f"capped: reversed-row difference {reorder:.3e}, tolerance {tol:.3e}")
    got = fit_sweep([_dev(X)], [[lab]], [[K]], max_iter=max_iter, resp_for=True)[0][0]
    assert not want["converged"] and want["n_iter"] == max_iter
    _compare_fit("capped", got, want, tol=tol)


def test_a_slow_and_a_fast_fit_side_by_side_and_check_every(edge):
    """One call with the set that takes about 50 iterations next to the one that stops at 2: each is the fit it is alone, and
    the grouping of the iterations into calls (check_every 1, 4, 8) does not move a bit."""
    from spadot_amd.gmm import fit_sweep
    (Xs, ls, Ks), (Xf, lf, Kf) = cases.fit_case("slow"), cases.fit_case("fast")
    both = fit_sweep([_dev(Xs), _dev(Xf)], [[ls], [lf]], [[Ks], [Kf]], resp_for=True)
    assert 40 <= both[0][0].n_iter_ <= 60 and both[1][0].n_iter_ == 2 and both[0][0].converged_ and both[1][0].converged_
    alone = [fit_sweep([_dev(Xs)], [[ls]], [[Ks]], resp_for=True, check_every=1)[0][0],
             fit_sweep([_dev(Xf)], [[lf]], [[Kf]], resp_for=True, check_every=8)[0][0]]
    assert _same_bits(both[0][0], alone[0]) and _same_bits(both[1][0], alone[1])
    sets, labelings, Ks_e, res, _ = edge
    for ce in (1, 8):
        again = fit_sweep([_dev(x) for x in sets], labelings, Ks_e, resp_for=True, check_every=ce)
        assert all(_same_bits(again[t][l], res[t][l]) for t in range(2) for l in range(3)), ce


def test_alone_in_a_batch_again_and_fp32_give_the_same_bits(edge):
    from spadot_amd.gmm import fit_sweep
    sets, labelings, Ks, res, _ = edge
    for t, l in ((1, 2), (0, 1), (0, 2)):
        alone = fit_sweep([_dev(sets[t])], [[labelings[t][l]]], [[Ks[t][l]]], resp_for=True)[0][0]
        assert _same_bits(alone, res[t][l]), (t, l)
    again = fit_sweep([_dev(x) for x in sets], labelings, Ks, resp_for=True)
    res32 = fit_sweep([_dev(x, torch.float32) for x in sets], labelings, Ks, resp_for=True)
    for t in range(2):
        for l in range(3):
            assert _same_bits(again[t][l], res[t][l]) and _same_bits(res32[t][l], res[t][l]), (t, l)
    some = fit_sweep([_dev(x) for x in sets], labelings, Ks, resp_for=[(1, 0)])       # responsibilities only where asked for
    assert [[r.resp_ is not None for r in rt] for rt in some] == [[False] * 3, [True, False, False]]
    assert np.array_equal(some[1][0].resp_, res[1][0].resp_)


def test_a_converged_problem_is_untouched_by_later_steps():
    from spadot_amd.gmm import _as_sets, _Batch, _labels_on_device
    (Xs, ls, Ks), (Xf, lf, Kf) = cases.fit_case("slow"), cases.fit_case("fast")
    sets = _as_sets([_dev(Xs), _dev(Xf)])
    _, _, Kl, labels = _labels_on_device(sets, [[ls], [lf]], [[Ks], [Kf]])
    b = _Batch(sets, [0, 1], Kl)
    onehot = torch.zeros((b.total, b.K_max), dtype=torch.float64, device=DEV).scatter_(1, labels[:, None], 1.0)
    b.em(4, 1e-6, 1e-3, resp_init=onehot)
    assert b.done.tolist() == [0, 1] and b.n_iter.tolist() == [4, 2]
    snap = [x[1].clone() for x in (b.par, b.w, b.cov, b.lb, b.n_iter)]
    b.em(5, 1e-6, 1e-3)
    assert b.n_iter.tolist() == [9, 2] and b.done.tolist() == [0, 1]
    assert all(torch.equal(s, x[1]) for s, x in zip(snap, (b.par, b.w, b.cov, b.lb, b.n_iter)))


def test_the_estimator_follows_sklearns_definitions():
    from spadot_amd.gmm import GaussianMixtureDevice
    X, lab, K = cases.fit_case("n257")
    want = ref.fit(X, lab, K)
    g = GaussianMixtureDevice(K).fit(_dev(X), labels=lab)
    assert (g.n_iter_, g.converged_) == (want["n_iter"], want["converged"])
    np.testing.assert_array_equal(g.predict(_dev(X)), g.labels_)
    np.testing.assert_allclose(g.predict_proba(_dev(X)), want["resp"], rtol=0, atol=1e-9)
    assert g.score(_dev(X)) == pytest.approx(want["log_likelihood"] / 257, rel=1e-9)
    assert g.bic(_dev(X)) == pytest.approx(want["bic"], rel=1e-9) and g.aic(_dev(X)) == pytest.approx(want["aic"], rel=1e-9)
    new = X[:40] + 0.25                                   # other points: the fit's own centring is applied to them
    _, norm, log_resp, _ = ref.e_step(new - want["mean"], want["weights"], want["means_c"], want["precisions_cholesky"])
    np.testing.assert_allclose(g.score_samples(_dev(new)), norm, rtol=1e-9, atol=0)
    h = GaussianMixtureDevice(K, random_state=1993).fit(_dev(X, torch.float32))          # started from KMeansDevice's labels
    assert h.weights_.shape == (K,) and abs(h.weights_.sum() - 1.0) < 1e-12 and h.n_iter_ >= 1 and np.isfinite(h.lower_bound_)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(monkeypatch):
    from spadot_amd import gmm, stage_ops as ops
    # the library's own refusals (-7 -> ValueError): nothing is launched, the outputs keep their fill
    for d, K in ((33, 2), (3, 33), (32, 25)):
        S = gmm._dims(d)[2]
        X = _dev(np.zeros((40, d)))
        prob = torch.tensor([[0, 0, 40, min(K, 2)]], dtype=torch.int64, device=DEV)
        par = torch.full((1, K, S), 7.0, dtype=torch.float64, device=DEV)
        norm = torch.full((40,), 7.0, dtype=torch.float64, device=DEV)
        w, cov = torch.full((1, K), 7.0, dtype=torch.float64, device=DEV), torch.full((1, K, d, d), 7.0, dtype=torch.float64, device=DEV)
        flags = [torch.full((1,), 7, dtype=torch.int32, device=DEV) for _ in range(2)]
        lb, part = torch.full((1,), 7.0, dtype=torch.float64, device=DEV), torch.full((4096,), 7.0, dtype=torch.float64, device=DEV)
        with pytest.raises(ValueError, match="outside its limits"):
            ops.gmm_estep(X, prob, 40, par, norm)
        with pytest.raises(ValueError, match="outside its limits"):
            ops.gmm_em_steps(X, prob, 40, par, w, cov, part, flags[0], flags[1], lb, 1e-6, 1e-3, 1)
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in [par, norm, w, cov, lb, part] + flags)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(ops, "gmm_em_steps", no_launch)
    monkeypatch.setattr(ops, "gmm_estep", no_launch)
    X = _dev(np.zeros((40, 3)))
    two = np.arange(40) % 2
    with pytest.raises(ValueError, match="outside the limits"):
        gmm.fit_sweep([_dev(np.zeros((40, 33)))], [[two]])
    with pytest.raises(ValueError, match="33 components"):
        gmm.fit_sweep([X], [[np.arange(40) % 33]])
    with pytest.raises(ValueError, match="outside the limits"):
        gmm.fit_sweep([_dev(np.zeros((40, 32)))], [[two]], [[25]])
    with pytest.raises(ValueError, match="labels must lie in 0 .. 1"):
        gmm.fit_sweep([X], [[np.where(np.arange(40) == 7, -1, two)]], [[2]])
    with pytest.raises(ValueError, match="labels must lie in 0 .. 2"):
        gmm.fit_sweep([X], [[np.arange(40) % 4]], [[3]])
    with pytest.raises(ValueError, match="labels must be integers"):
        gmm.fit_sweep([X], [[np.zeros(40)]])
    with pytest.raises(ValueError, match="one label per point"):
        gmm.fit_sweep([X], [[np.arange(39) % 2]])
    with pytest.raises(ValueError, match="share their dimension, their dtype"):
        gmm.fit_sweep([X, _dev(np.zeros((40, 4)))], [[two], [two]])
    with pytest.raises(ValueError, match="share their dimension, their dtype"):
        gmm.fit_sweep([X, _dev(np.zeros((40, 3)), torch.float32)], [[two], [two]])
    with pytest.raises(RuntimeError, match="MI355X only"):
        gmm.fit_sweep([X.cpu()], [[two]])
    with pytest.raises(AssertionError, match="launched"):                           # the patch is what a valid call would reach
        gmm.fit_sweep([X], [[two]])


# ---------------------------------------------------------------------------------------------------------------- the stage
class _Args:
    def __init__(self, **kw):
        self.__dict__.update(dict(output_dir=None, prefix="", n_clusters=None, device=DEV, write_tmaps=False), **kw)


def test_analyze_picks_the_planted_k_by_bic_and_leaves_the_default_alone(tmp_path):
    import pandas as pd
    from spadot_amd import analyze
    from spadot_amd.trends import read_lineage
    from spadot_amd.utils._analyze_utils import have_matplotlib
    X, _ = cases.planted()
    f = tmp_path / "latent.npz"
    tp_all, _ = cases.write_latent(f, X)
    tps = ["E1", "E2", "E3"]
    gmm_dir, cli_dir = tmp_path / "gmm", tmp_path / "cli"
    out = analyze(_Args(data=str(f), output_dir=str(gmm_dir), method="gmm", criterion="bic"))
    assert out["n_clusters"] == [5, 6, 7] and out["method"] == "gmm" and out["criterion"] == "bic"
    for t, (tp, x) in enumerate(zip(tps, X)):
        tab = pd.read_csv(gmm_dir / f"adaptive_{tp}_BIC.csv", float_precision="round_trip")
        assert list(tab.columns) == ["clusters", "bic", "aic", "log_likelihood", "n_iter", "converged", "selected"]
        assert tab["clusters"].tolist() == list(range(4, 21)) and tab["clusters"][tab["selected"]].tolist() == [5 + t]
        np.testing.assert_array_equal(tab["bic"].to_numpy(), np.asarray(out["bic"][tp]))
        assert int(np.argmin(out["bic"][tp])) == 1 + t                             # k = 5, 6, 7 at index 1, 2, 3
    M, names = read_lineage(str(gmm_dir / "adaptive_memberships.npz"), tp_all)      # what `trends --trajectories` reads
    assert names.tolist() == [f"{tp}_{c}" for tp, k in zip(tps, (5, 6, 7)) for c in range(k)] and M.shape == (6000, 18)
    np.testing.assert_allclose(M.sum(1), 1.0, rtol=0, atol=1e-12)
    off = 0
    dom = pd.read_csv(gmm_dir / "adaptive_domains.csv")
    assert list(dom.columns) == ["row", "timepoint", "kmeans", "pixel_x", "pixel_y"]
    for tp, k in zip(tps, (5, 6, 7)):
        m = tp_all == tp
        assert not np.delete(M[m], np.arange(off, off + k), axis=1).any()           # 0 outside the time point's own columns
        sure = ref.label_margin(M[m][:, off:off + k]) > 1e-6
        np.testing.assert_array_equal(dom["kmeans"].to_numpy()[m][sure], M[m][:, off:off + k].argmax(1)[sure])
        np.testing.assert_array_equal(dom["kmeans"].to_numpy()[m], out["labels"][tp])
        off += k
    z = np.load(gmm_dir / "adaptive_gmm.npz")
    assert z["means_E1"].shape == (5, 20) and z["covariances_E3"].shape == (7, 20, 20) and abs(z["weights_E2"].sum() - 1) < 1e-12
    new = {"adaptive_memberships.npz", "adaptive_gmm.npz"} | {f"adaptive_{t}_BIC.csv" for t in tps}
    if have_matplotlib():
        new |= {f"adaptive_{t}_BIC_vs_Clusters.png" for t in tps}
    assert new <= set(os.listdir(gmm_dir)) and not any("WSS" in n for n in os.listdir(gmm_dir))
    # the command line writes the same tables
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "spadot_amd", "analyze", "-i", str(f), "-o", str(cli_dir), "--method", "gmm",
                        "--criterion", "bic"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for name in ["adaptive_domains.csv"] + [f"adaptive_{t}_BIC.csv" for t in tps]:
        assert (cli_dir / name).read_bytes() == (gmm_dir / name).read_bytes(), name
    assert np.array_equal(np.load(cli_dir / "adaptive_memberships.npz")["X"], np.load(gmm_dir / "adaptive_memberships.npz")["X"])
    # the default run, in the same directory: it writes none of the new files (those there stay as they are), no new keys
    held = {n: ((gmm_dir / n).read_bytes(), os.stat(gmm_dir / n).st_mtime_ns) for n in new}
    before = set(os.listdir(gmm_dir))
    a = _Args(data=str(f), output_dir=str(gmm_dir))
    res = analyze(a)
    made = set(os.listdir(gmm_dir)) - before
    assert not any("BIC" in n or "memberships" in n or "gmm" in n for n in made) and "adaptive_E1_WSS.csv" in made
    assert all(((gmm_dir / n).read_bytes(), os.stat(gmm_dir / n).st_mtime_ns) == v for n, v in held.items())
    assert not {"method", "bic", "memberships", "criterion"} & set(res) and not hasattr(a, "method")
    kcol = pd.read_csv(gmm_dir / "adaptive_domains.csv")["kmeans"].to_numpy()         # its own domains replace the mixtures'
    np.testing.assert_array_equal(kcol, np.concatenate([res["labels"][tp] for tp in tps]))


def test_analyze_gmm_by_silhouette_with_lineage(tmp_path):
    """The other adaptive rule on mixtures: the silhouette of every mixture's labels picks k, the BIC tables are still written
    (with that k selected), and --lineage chains the plans over the mixtures' domains."""
    import pandas as pd
    from sklearn.metrics import silhouette_score
    from spadot_amd import analyze
    X, _ = cases.planted(counts=(500, 600, 700))
    f = tmp_path / "latent.npz"
    tp_all, rows = cases.write_latent(f, X)
    tps = ["E1", "E2", "E3"]
    out = analyze(_Args(data=str(f), output_dir=str(tmp_path / "out"), method="gmm", criterion="silhouette", lineage=True))
    assert out["method"] == "gmm" and out["criterion"] == "silhouette" and {"silhouette", "bic", "memberships", "lineage"} <= set(out)
    ks = out["n_clusters"]
    files = set(os.listdir(tmp_path / "out"))
    assert {"adaptive_domains.csv", "adaptive_memberships.npz", "adaptive_gmm.npz", "adaptive_trajectories.npz",
            "adaptive_fates.npz", "adaptive_transition_table_0_2.csv"} <= files and not any("WSS" in n for n in files)
    for tp, x, k in zip(tps, X, ks):
        s = np.asarray(out["silhouette"][tp])
        assert len(s) == 17 and k == 4 + int(np.nanargmax(s))                      # the largest score, the first of equals
        lab = out["labels"][tp]
        assert s[k - 4] == pytest.approx(silhouette_score(x.astype(np.float64), lab), rel=1e-9, abs=1e-12)   # of the mixture's labels
        for name in ("silhouette", "BIC"):
            tab = pd.read_csv(tmp_path / "out" / f"adaptive_{tp}_{name}.csv")
            assert tab["clusters"].tolist() == list(range(4, 21)) and tab["clusters"][tab["selected"]].tolist() == [k]
        np.testing.assert_array_equal(pd.read_csv(tmp_path / "out" / f"adaptive_{tp}_BIC.csv", float_precision="round_trip")["bic"],
                                      np.asarray(out["bic"][tp]))
    M = out["memberships"]["X"]
    assert M.shape == (1800, sum(ks)) and out["memberships"]["names"].tolist() == [f"{tp}_{c}" for tp, k in zip(tps, ks) for c in range(k)]
    np.testing.assert_allclose(M.sum(1), 1.0, rtol=0, atol=1e-12)
    off = 0
    for tp, k in zip(tps, ks):
        own = M[tp_all == tp][:, off:off + k]
        sure = ref.label_margin(own) > 1e-6
        np.testing.assert_array_equal(out["labels"][tp][sure], own.argmax(1)[sure])
        off += k
    tr, fa = np.load(tmp_path / "out" / "adaptive_trajectories.npz"), np.load(tmp_path / "out" / "adaptive_fates.npz")
    assert tr["names"].tolist() == out["memberships"]["names"].tolist() and tr["X"].shape == M.shape and np.isfinite(tr["X"]).all()
    np.testing.assert_array_equal(tr["rows"], rows)
    assert fa["X"].shape == (1800, ks[2]) and np.isfinite(fa["X"]).all()
    np.testing.assert_array_equal(fa["X"][tp_all == "E3"], np.eye(ks[2])[out["labels"]["E3"]])
