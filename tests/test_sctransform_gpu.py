"""SCTransform and the Louvain gene clusters on the MI355X against the fp64 restatement of tests/sct_ref.py: Poisson fits,
theta.ml, regularisation, Pearson residual statistics and scale.data per time point, the device digamma / trigamma, the
step-1 draw, determinism, the clusters, and preprocess with gene_clusters='louvain' end to end and from the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sct_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (400, 1200, 2000)


@pytest.fixture(scope="module")
def data():
    from spadot_amd.synthetic import make_raw_counts
    return make_raw_counts(SIZES, n_genes=1500)


@pytest.fixture(scope="module")
def dc(data):
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.utils._preprocess_utils import load_counts
    raw, _ = load_counts(data)
    return DeviceCounts(raw, DEV)


@pytest.fixture(scope="module")
def sct(dc):
    from spadot_amd.sctransform import sctransform
    return [sctransform(dc, t) for t in range(dc.T)]


@pytest.fixture(scope="module")
def restated(data):
    X = sp.csr_matrix(data.X, dtype=np.float64)
    tp = data.obs["timepoint"]
    return [ref.sctransform(X[tp == t]) for t in range(len(SIZES))]


def test_fits_match_the_restatement(sct, restated):
    for t, (g, w) in enumerate(zip(sct, restated)):
        off = sum(SIZES[:t])
        np.testing.assert_array_equal(g.spots - off, w["spots"])
        np.testing.assert_array_equal(g.genes, w["genes"])
        np.testing.assert_allclose(g.log_umi, w["log_umi"], rtol=1e-14)
        np.testing.assert_allclose(g.log_gmean, w["log_gmean"], rtol=1e-12, atol=1e-13)
        np.testing.assert_array_equal(g.step1, w["step1"])
        np.testing.assert_allclose(g.model_pars[:, 1:], w["coef"], rtol=0, atol=1e-9)
        th, tw = g.model_pars[:, 0], w["theta"]
        small = tw < 1e3
        assert small.sum() > 0.5 * tw.size
        np.testing.assert_allclose(th[small], tw[small], rtol=1e-6)
        disp = np.log10(1 + 10 ** g.log_gmean[g.step1] / th)
        np.testing.assert_allclose(disp, w["disp"], rtol=0, atol=1e-9)


def test_regularisation_matches_the_restatement(sct, restated):
    for g, w in zip(sct, restated):
        np.testing.assert_array_equal(g.outliers, w["outliers"])
        np.testing.assert_allclose(g.model_pars_fit[:, 1], w["fit_intercept"], rtol=0, atol=1e-8)
        np.testing.assert_allclose(g.model_pars_fit[:, 2], w["fit_slope"], rtol=0, atol=1e-8)
        np.testing.assert_allclose(np.log10(1 + 10 ** g.log_gmean / g.model_pars_fit[:, 0]),
                                   np.log10(1 + 10 ** w["log_gmean"] / w["fit_theta"]), rtol=0, atol=1e-8)


def test_residuals_and_scale_data_match_the_restatement(sct, restated):
    for g, w in zip(sct, restated):
        np.testing.assert_allclose(g.gene_attr["residual_mean"], w["residual_mean"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(g.gene_attr["residual_variance"], w["residual_variance"], rtol=1e-9)
        np.testing.assert_allclose(g.gene_attr["amean"], w["amean"], rtol=1e-12)
        np.testing.assert_allclose(g.gene_attr["variance"], w["variance"], rtol=1e-10)
        rows = np.arange(0, g.genes.size, 7)
        blk = g.scale_data(g.genes[rows]).cpu().numpy()
        np.testing.assert_allclose(blk, w["scale"][rows], rtol=0, atol=1e-9)


def test_device_polygamma_matches_scipy():
    from scipy.special import digamma, polygamma
    from spadot_amd._lib import model_lib
    x = np.concatenate([np.geomspace(1e-8, 1e10, 4000), np.arange(1, 200) + 0.5, [1.4616321449683622]])
    xd = torch.as_tensor(x, device=DEV)
    psi = torch.empty_like(xd)
    psi1 = torch.empty_like(xd)
    rc = model_lib().spadot_sct_polygamma(xd.data_ptr(), x.size, psi.data_ptr(), psi1.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    # relative 1e-14, with an absolute floor of 1e-15 where digamma crosses zero (x ~ 1.46)
    np.testing.assert_allclose(psi.cpu().numpy(), digamma(x), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(psi1.cpu().numpy(), polygamma(1, x), rtol=1e-14, atol=0)


def test_step1_draw_with_more_than_2000_genes():
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.sctransform import sctransform
    from spadot_amd.synthetic import make_raw_counts
    from spadot_amd.utils._preprocess_utils import load_counts
    d = make_raw_counts((300,), n_genes=2600, seed=7)
    raw, _ = load_counts(d)
    g = sctransform(DeviceCounts(raw, DEV), 0)
    assert g.genes.size > 2000 and g.step1.size == 2000
    X = sp.csr_matrix(d.X, dtype=np.float64)
    keep, _ = ref.cell_attr(X)
    genes = ref.kept_genes(X)
    np.testing.assert_array_equal(g.genes, genes)
    np.testing.assert_array_equal(g.step1, ref.step1_set(ref.log_gmean(ref.dense_y(X, keep, genes))))


def test_two_runs_are_bitwise_identical(dc, sct):
    from spadot_amd.preprocess import cluster_genes_louvain
    from spadot_amd.sctransform import sctransform
    t = 1
    a, b = sct[t], sctransform(dc, t)
    np.testing.assert_array_equal(a.model_pars, b.model_pars)
    np.testing.assert_array_equal(a.fit_info, b.fit_info)
    np.testing.assert_array_equal(a.model_pars_fit, b.model_pars_fit)
    for k in a.gene_attr:
        np.testing.assert_array_equal(a.gene_attr[k], b.gene_attr[k])
    cols = a.genes[:300]
    assert torch.equal(a.scale_data(cols), b.scale_data(cols))
    np.testing.assert_array_equal(cluster_genes_louvain(dc, t, cols, a), cluster_genes_louvain(dc, t, cols, b))


@pytest.fixture(scope="module")
def louvain_run(data):
    from spadot_amd.preprocess import preprocess_counts
    from spadot_amd.utils._preprocess_utils import load_counts
    raw, _ = load_counts(data)
    return preprocess_counts(raw, device=DEV, gene_clusters="louvain")


def test_louvain_clusters_recover_the_planted_modules(louvain_run, data):
    from sklearn.metrics import adjusted_rand_score
    mod = data.uns["module"]
    for r in louvain_run["sparkx"]:
        assert np.unique(r["cluster"]).size >= 10
        sel = mod[r["selected"]] >= 0
        assert sel.sum() >= 100
        assert adjusted_rand_score(mod[r["selected"]][sel], r["cluster"][sel]) >= 0.8


def _write_counts(path, data):
    np.savez(path, X=data.X, timepoint=np.array([f"E{t + 1}" for t in data.obs["timepoint"]]),
             spatial=data.obsm["spatial"], genes=data.var_names)


class _Args:
    def __init__(self, **kw):
        self.output_dir, self.prefix, self.feature_selection, self.device = None, "preprocessed_", True, DEV
        self.__dict__.update(kw)


def test_preprocess_with_louvain_end_to_end(tmp_path, data):
    import pandas as pd
    from spadot_amd import preprocess
    from spadot_amd.utils._utils import load_data
    f = tmp_path / "counts.npz"
    _write_counts(f, data)
    km = tmp_path / "km"
    lv = tmp_path / "lv"
    preprocess(_Args(data=str(f), output_dir=str(km)))
    res = preprocess(_Args(data=str(f), output_dir=str(lv), gene_clusters="louvain"))
    for t in (1, 2, 3):
        a = pd.read_csv(km / f"E{t}_SVG_sparkx_clustered_louvain.csv", header=0, index_col=0)
        b = pd.read_csv(lv / f"E{t}_SVG_sparkx_clustered_louvain.csv", header=0, index_col=0)
        assert a.index.tolist() == b.index.tolist()
        pd.testing.assert_frame_equal(a.drop(columns="cluster"), b.drop(columns="cluster"))
        assert b["cluster"].nunique() >= 10
    svg = open(lv / "SVG_genes.txt").read().split()
    assert svg == list(res["genes"])
    d, _ = load_data(str(lv / "preprocessed_counts.npz"))
    assert d.X.shape == res["X"].shape


def test_command_line_louvain(tmp_path, data):
    import pandas as pd
    f = tmp_path / "counts.npz"
    _write_counts(f, data)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "spadot_amd", "preprocess", "-i", str(f), "-o", str(tmp_path / "out"),
                        "--gene_clusters", "louvain"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    df = pd.read_csv(tmp_path / "out" / "E1_SVG_sparkx_clustered_louvain.csv", header=0, index_col=0)
    assert df["cluster"].nunique() >= 10
