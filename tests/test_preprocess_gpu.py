"""The preprocess stage on the MI355X against the fp64 restatement of tests/preprocess_ref.py: SPARK-X moments, statistics,
p-values and ACAT, the per-time-point SVG lists, the scaled output, determinism, the K-means gene clusters, preprocess(args)
end to end into train, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import preprocess_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (400, 1200, 2000)


@pytest.fixture(scope="module")
def data():
    from spadot_amd.synthetic import make_raw_counts
    return make_raw_counts(SIZES, n_genes=1500)


@pytest.fixture(scope="module")
def run(data):
    from spadot_amd.preprocess import preprocess_counts
    from spadot_amd.utils._preprocess_utils import load_counts
    raw, _ = load_counts(data)
    return preprocess_counts(raw, device=DEV)


@pytest.fixture(scope="module")
def restated(data):
    X = sp.csr_matrix(data.X, dtype=np.float64)
    tp = data.obs["timepoint"]
    out = []
    for t in range(len(SIZES)):
        B = X[tp == t]
        vst = ref.gene_filter(B)
        r = ref.sparkx(B[:, vst], data.obsm["spatial"][tp == t])
        r["genes"] = vst[r["genes"]]
        r["selected"] = vst[r["selected"]]
        out.append(r)
    return out


def _close(got, want, rtol):
    scale = np.abs(want).max() if want.size else 1.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * scale)


def test_sparkx_matches_the_restatement(run, restated):
    for t, (g, w) in enumerate(zip(run["sparkx"], restated)):
        off = sum(SIZES[:t])
        np.testing.assert_array_equal(g["spots"] - off, w["spots"])
        np.testing.assert_array_equal(g["genes"], w["genes"])
        _close(g["mom"][:, 0], w["sy"], 1e-12)
        _close(g["mom"][:, 1], w["syy"], 1e-12)
        for k in range(11):     # column-wise: each kernel's coordinates have their own scale (sums of centred values cancel)
            _close(g["mom"][:, 2 + 2 * k:4 + 2 * k], w["ehl"][:, 2 * k:2 * k + 2], 1e-10)
        _close(g["stat"], w["stat"], 1e-10)
        np.testing.assert_allclose(g["pval"], w["pval"], rtol=1e-10, atol=1e-15)
        # ACAT's 1 - cauchy.cdf(cct) cancels for large cct: an absolute floor of 1e-15 below which rounding decides
        np.testing.assert_allclose(g["combined"], w["combined"], rtol=1e-10, atol=1e-15)
        # BY scales each combined p by up to n * sum(1/k): so does the absolute floor
        n = w["adjusted"].size
        np.testing.assert_allclose(g["adjusted"], w["adjusted"], rtol=1e-10, atol=1e-15 * n * np.sum(1.0 / np.arange(1, n + 1)))


def test_svg_lists_match_and_planted_genes_are_selected(run, restated, data):
    mod = data.uns["module"]
    planted = np.flatnonzero(mod >= 0)
    for g, w in zip(run["sparkx"], restated):
        # the same genes; the order too, except inside a run of equal adjusted p, where the tie-break by combined p can see
        # p-values that differ only by the rounding of ACAT's cancellation (< 1e-15 absolute)
        np.testing.assert_array_equal(np.sort(g["selected"]), np.sort(w["selected"]))
        adj = dict(zip(g["genes"].tolist(), g["adjusted"].tolist()))
        a_g = np.array([adj[c] for c in g["selected"]])
        assert np.all(np.diff(a_g) >= 0)
        np.testing.assert_allclose(a_g, [adj[c] for c in w["selected"]], rtol=1e-10, atol=1e-10)
        assert np.isin(planted, g["selected"]).mean() >= 0.95
        null = g["genes"][mod[g["genes"]] == -1]
        assert np.isin(null, g["selected"]).mean() < 0.5
    names = data.var_names
    for t, (gn, comb, adj, clus) in enumerate(run["tables"]):
        np.testing.assert_array_equal(np.sort(gn), np.sort(names[restated[t]["selected"]]))


def test_gene_clusters_recover_the_planted_modules(run, data):
    from sklearn.metrics import adjusted_rand_score
    mod = data.uns["module"]
    for r in run["sparkx"]:
        m = mod[r["selected"]]
        assert len(set(r["cluster"].tolist())) == 10
        assert adjusted_rand_score(m[m >= 0], r["cluster"][m >= 0]) >= 0.8


def _restated_output(data, cols):
    X = sp.csr_matrix(data.X, dtype=np.float64)
    tp = data.obs["timepoint"]
    return np.concatenate([ref.normalize_log_scale(X[tp == t][:, cols]) for t in range(len(SIZES))])


def test_scaled_output_matches_the_restatement(run, data):
    want = _restated_output(data, run["cols"])
    np.testing.assert_allclose(run["X"], want.astype(np.float32), rtol=2e-6, atol=2e-6)
    assert run["X"].dtype == np.float32
    # the svgs are the sorted union of gene names
    assert list(run["genes"]) == sorted(run["genes"])


def test_no_feature_selection_dense_and_csr_agree(data):
    from spadot_amd.preprocess import preprocess_counts
    from spadot_amd.synthetic import SpatialData
    from spadot_amd.utils._preprocess_utils import load_counts
    raw_d, _ = load_counts(data)
    csr = SpatialData(sp.csr_matrix(data.X), data.obs["timepoint"], data.obsm["spatial"])
    csr.X = sp.csr_matrix(data.X)
    csr.var_names = data.var_names
    raw_s, _ = load_counts(csr)
    a = preprocess_counts(raw_d, feature_selection=False, device=DEV)
    b = preprocess_counts(raw_s, feature_selection=False, device=DEV)
    np.testing.assert_array_equal(a["X"], b["X"])
    want = _restated_output(data, np.arange(data.X.shape[1]))
    np.testing.assert_allclose(a["X"], want.astype(np.float32), rtol=2e-6, atol=2e-6)
    zero_gene = data.X.shape[1] - 6                             # zero in the first time point: std 0 -> 1, output 0
    assert np.all(a["X"][:SIZES[0], zero_gene] == 0)
    tp0 = data.X[:SIZES[0]]
    zero_spot = np.flatnonzero(tp0.sum(1) == 0)[0]              # a zero-total spot: every entry is -mean / std
    np.testing.assert_allclose(a["X"][zero_spot], want[zero_spot].astype(np.float32), rtol=2e-6, atol=2e-6)


def test_two_runs_are_bitwise_identical(run, data):
    from spadot_amd.preprocess import preprocess_counts
    from spadot_amd.utils._preprocess_utils import load_counts
    raw, _ = load_counts(data)
    again = preprocess_counts(raw, device=DEV)
    np.testing.assert_array_equal(again["X"], run["X"])
    for a, b in zip(again["sparkx"], run["sparkx"]):
        for k in ("mom", "stat", "pval", "combined", "cluster"):
            np.testing.assert_array_equal(a[k], b[k])


class _Args:
    def __init__(self, **kw):
        self.__dict__.update(dict(output_dir=None, prefix="preprocessed_", feature_selection=True, device=DEV), **kw)


def _write_counts(path, data, csr=False):
    if csr:
        C = sp.csr_matrix(data.X)
        np.savez(path, X_data=C.data, X_indices=C.indices, X_indptr=C.indptr, X_shape=np.array(C.shape),
                 timepoint=np.array([f"E{t + 1}" for t in data.obs["timepoint"]]), spatial=data.obsm["spatial"],
                 genes=data.var_names)
    else:
        np.savez(path, X=data.X, timepoint=np.array([f"E{t + 1}" for t in data.obs["timepoint"]]),
                 spatial=data.obsm["spatial"], genes=data.var_names)


def test_preprocess_end_to_end_into_train(tmp_path, data, run):
    import yaml
    from spadot_amd import preprocess, train
    from spadot_amd.utils._utils import load_data
    f = tmp_path / "counts.npz"
    _write_counts(f, data, csr=True)
    a = _Args(data=str(f))
    res = preprocess(a)
    assert a.output_dir == str(tmp_path)
    files = set(os.listdir(tmp_path))
    want = {"preprocessed_counts.npz", "SVG_genes.txt"} | {f"E{t}_SVG_sparkx_clustered_louvain.csv" for t in (1, 2, 3)}
    assert want <= files, want - files
    np.testing.assert_array_equal(res["X"], run["X"])
    svg = open(tmp_path / "SVG_genes.txt").read().split()
    assert svg == list(run["genes"])
    import pandas as pd
    df = pd.read_csv(tmp_path / "E1_SVG_sparkx_clustered_louvain.csv", header=0, index_col=0)
    assert list(df.columns) == ["combinedPval", "adjustedPval", "cluster"]
    assert df.index.tolist() == list(run["tables"][0][0])
    d, _ = load_data(str(tmp_path / "preprocessed_counts.npz"))
    assert d.X.shape == run["X"].shape
    z = np.load(tmp_path / "preprocessed_counts.npz")
    counts = sp.csr_matrix((z["counts_data"], z["counts_indices"], z["counts_indptr"]), shape=tuple(z["counts_shape"]))
    np.testing.assert_array_equal(counts.toarray(), data.X[:, run["cols"]])     # rows already in time point order here
    cfg = dict(yaml.safe_load(open(os.path.join(ROOT, "spadot_amd", "config.yaml"))))
    cfg.update(maxiter=2, ot_epoch=1, batch_size=256, inducing_point_nums=50, svgp_encoder_layers=[32, 16],
               gat_encoder_hidden=16, decoder_layers=[16, 32])
    cfg["ot_config"] = dict(cfg["ot_config"], ot_epochs=1)
    cfg_path = tmp_path / "small.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    targs = type("A", (), {})()
    targs.__dict__.update(data=str(tmp_path / "preprocessed_counts.npz"), output_dir=str(tmp_path / "train"), prefix="",
                          config=str(cfg_path), device=DEV, save_model=False)
    os.makedirs(targs.output_dir, exist_ok=True)
    train(targs)
    assert any(n.startswith("latent") for n in os.listdir(targs.output_dir))


def test_command_line_preprocess(tmp_path, data):
    f = tmp_path / "counts.npz"
    _write_counts(f, data)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "spadot_amd", "preprocess", "-i", str(f), "-o", str(tmp_path / "out")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    files = set(os.listdir(tmp_path / "out"))
    assert {"preprocessed_counts.npz", "SVG_genes.txt", "E1_SVG_sparkx_clustered_louvain.csv"} <= files


def test_pvalue_kernel_with_unequal_weights_matches_quadrature():
    # k_sparkx_pvals on crafted moments: SPARK-X's own weights are (1, 1) up to rounding, so this is where the kernel's
    # trapezoid over an integrand that is far from constant is compared with adaptive quadrature
    from spadot_amd._lib import model_lib
    rng = np.random.default_rng(7)
    P, n = 64, 1000
    lam = np.array([[1.0, 1.0], [2.0, 0.5], [1.3, 0.9], [0.5, 2.0], [3.0, 1.0], [1.0, 0.25], [0.8, 0.8], [1.5, 1.2],
                    [0.6, 1.1], [2.5, 0.4], [1.0, 4.0]])
    inv = np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (11, 1))
    mom = np.zeros((P, 24))
    mom[:, 0] = rng.uniform(0, 40, P)                      # sum y: ylam = 1 - n ybar^2 / sum y^2 in (0.998, 1]
    mom[:, 1] = n                                          # sum y^2 = n: stat = e1^2 + e2^2
    mom[:, 2:] = rng.uniform(0.05, 3.8, (P, 22)) * rng.choice([-1, 1], (P, 22))
    d = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)
    mom_d, pt_d, nk_d, inv_d, lam_d = d(mom), d(np.zeros(P), torch.int32), d([n], torch.int32), d(inv), d(lam)
    stat = torch.empty((P, 11), dtype=torch.float64, device=DEV)
    pval = torch.empty((P, 11), dtype=torch.float64, device=DEV)
    comb = torch.empty(P, dtype=torch.float64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    rc = model_lib().spadot_sparkx_pvals(mom_d.data_ptr(), P, pt_d.data_ptr(), nk_d.data_ptr(), inv_d.data_ptr(),
                                         lam_d.data_ptr(), 256, stat.data_ptr(), pval.data_ptr(), comb.data_ptr(), s)
    assert rc == 0
    stat, pval, comb = stat.cpu().numpy(), pval.cpu().numpy(), comb.cpu().numpy()
    ylam = 1 - n * (mom[:, 0] / n) ** 2 / n
    for i in range(P):
        for k in range(11):
            q = mom[i, 2 + 2 * k] ** 2 + mom[i, 3 + 2 * k] ** 2
            assert stat[i, k] == pytest.approx(q, rel=1e-13)
            assert pval[i, k] == pytest.approx(ref.sf_two_term(q, ylam[i] * lam[k, 0], ylam[i] * lam[k, 1]), rel=1e-10)
        assert comb[i] == pytest.approx(ref.acat(pval[i]), rel=1e-10, abs=1e-15)


def _shuffled(data, seed=11):
    """The same spots with rows shuffled and time point 2 appearing first: returns (object for load_counts, original row
    of each shuffled row)."""
    rng = np.random.default_rng(seed)
    tp = data.obs["timepoint"]
    first = int(np.flatnonzero(tp == 2)[0])
    rest = rng.permutation(np.setdiff1d(np.arange(tp.size), [first]))
    sh = np.concatenate([[first], rest])
    while tp[sh[1:]][np.argmax(tp[sh[1:]] != 2)] != 0:     # then time point 0, then 1
        rest = rng.permutation(rest)
        sh = np.concatenate([[first], rest])
    obj = type("Obj", (), {})()
    obj.X, obj.obs, obj.obsm = sp.csr_matrix(data.X[sh]), {"timepoint": tp[sh]}, {"spatial": data.obsm["spatial"][sh]}
    obj.var_names = data.var_names
    return obj, sh


def test_shuffled_rows_and_time_point_order(data, run):
    from spadot_amd.preprocess import preprocess_counts
    from spadot_amd.utils._preprocess_utils import load_counts
    obj, sh = _shuffled(data)
    raw, _ = load_counts(obj)
    # without feature selection the output does not depend on the gene clusters: every row must be the block-ordered
    # run's row of the same spot
    s = preprocess_counts(raw, feature_selection=False, device=DEV)
    b = preprocess_counts(load_counts(data)[0], feature_selection=False, device=DEV)
    assert s["tps"] == [2, 0, 1] and b["tps"] == [0, 1, 2]
    orig = sh[s["perm"]]                                   # original row of each output row
    tp = data.obs["timepoint"]
    np.testing.assert_array_equal(s["timepoint"], tp[orig])
    np.testing.assert_array_equal(s["timepoint"], np.repeat([2, 0, 1], [SIZES[2], SIZES[0], SIZES[1]]))
    for t in (0, 1, 2):                                    # input order kept inside a time point block
        rows = s["perm"][s["timepoint"] == t]
        assert np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(s["spatial"], data.obsm["spatial"][orig])
    np.testing.assert_array_equal(s["counts"].toarray(), data.X[orig][:, s["cols"]])
    np.testing.assert_allclose(s["X"], b["X"][orig], rtol=1e-6, atol=1e-6)
    # with feature selection: the same SPARK-X results per time point, now in the order 2, 0, 1
    f = preprocess_counts(raw, device=DEV)
    for i, t in enumerate(f["tps"]):
        g, w = f["sparkx"][i], run["sparkx"][t]
        np.testing.assert_array_equal(g["genes"], w["genes"])
        np.testing.assert_array_equal(np.sort(g["selected"]), np.sort(w["selected"]))
        np.testing.assert_allclose(g["combined"], w["combined"], rtol=1e-10, atol=1e-15)
        np.testing.assert_array_equal(np.sort(sh[f["perm"]][g["spots"]]), w["spots"])     # block run: row = original row
    np.testing.assert_array_equal(f["timepoint"], tp[sh[f["perm"]]])
    np.testing.assert_array_equal(f["counts"].toarray(), data.X[sh[f["perm"]]][:, f["cols"]])
