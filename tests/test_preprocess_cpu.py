"""CPU: the host helpers of the preprocess stage (ACAT, Benjamini-Yekutieli, the two-term survival function against Liu and
quadrature, the balancing rule select_svgs, the raw-count loader and its checks) and the preprocess command line."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import preprocess_ref as ref
from spadot_amd.utils import _preprocess_utils as pu


def test_acat_branches():
    p = np.array([0.2, 0.5, 0.9])
    w = 1 / 3
    want = 0.5 - np.arctan(sum(w * np.tan((0.5 - v) * np.pi) for v in p)) / np.pi
    assert pu.acat(p) == pytest.approx(want, rel=1e-12)
    assert pu.acat(np.array([0.0, 0.3])) == 0.0
    assert pu.acat(np.array([1.0, 0.3])) == 1.0
    with pytest.raises(ValueError):
        pu.acat(np.array([0.0, 1.0]))
    with pytest.raises(ValueError):
        pu.acat(np.array([np.nan, 0.1]))
    # the p < 1e-16 branch: w / (pi p) in place of the tangent
    p = np.array([1e-18, 0.4])
    cct = 0.5 / (np.pi * 1e-18) + 0.5 * np.tan(0.1 * np.pi)
    assert cct > 1e15
    assert pu.acat(p) == pytest.approx(1 / (cct * np.pi), rel=1e-12)       # and the cct > 1e15 branch
    p = np.array([1e-17, 0.5, 0.5, 0.5] + [0.5] * 1000)
    cct = (1 / p.size) / (np.pi * 1e-17)
    assert cct < 1e15
    assert pu.acat(p) == pytest.approx(1 - (0.5 + np.arctan(cct) / np.pi), rel=1e-9)
    for q in (np.array([0.01, 0.02, 0.5]), np.array([1e-20, 0.3, 0.7]), np.array([1e-3] * 11)):
        assert pu.acat(q) == pytest.approx(ref.acat(q), rel=1e-12)


def test_by_adjustment_hand_computed():
    p = np.array([0.01, 0.04, 0.03, 0.5])
    cm = 1 + 1 / 2 + 1 / 3 + 1 / 4                       # 25 / 12
    # sorted 0.01, 0.03, 0.04, 0.5: raw p * n * cm / rank, then the running minimum from the top, capped at 1
    raw = np.array([0.01 * 4 * cm / 1, 0.03 * 4 * cm / 2, 0.04 * 4 * cm / 3, 0.5 * 4 * cm / 4])
    want_sorted = np.minimum(np.minimum.accumulate(raw[::-1])[::-1], 1)
    want = want_sorted[[0, 2, 1, 3]]
    np.testing.assert_allclose(pu.by_adjust(p), want, rtol=1e-14)
    np.testing.assert_allclose(want, [1 / 12, 1 / 9, 1 / 9, 1.0], rtol=1e-12)   # 0.03 -> 0.125 takes the 1/9 below it
    rng = np.random.default_rng(0)
    q = rng.uniform(size=300) ** 3
    np.testing.assert_allclose(pu.by_adjust(q), ref.fdr_by(q), rtol=1e-14)


@pytest.mark.parametrize("l1,l2", [(1.0, 1.0), (0.7, 0.7), (2.0, 0.5), (1.3, 0.9)])
def test_two_term_survival_against_liu_and_quadrature(l1, l2):
    from scipy import integrate
    for q in (0.01, 0.5, 2.0, 7.5, 30.0):
        f = lambda th: np.exp(-q / (2 * (l1 * np.cos(th) ** 2 + l2 * np.sin(th) ** 2)))
        quad = integrate.quad(f, 0, np.pi, epsabs=0, epsrel=1e-13)[0] / np.pi
        exact = ref.sf_two_term(q, l1, l2)
        assert exact == pytest.approx(quad, rel=1e-10)
        # the rule k_sparkx_pvals applies (256 equispaced nodes), restated in numpy, is exact to rounding here; the kernel
        # itself meets quadrature with unequal weights in tests/test_preprocess_gpu.py
        th = np.pi * np.arange(256) / 256
        trap = np.mean(np.exp(-q / (2 * (l1 * np.cos(th) ** 2 + l2 * np.sin(th) ** 2))))
        assert trap == pytest.approx(quad, rel=1e-12)
        lu = ref.liu(q, [l1, l2])
        if l1 == l2:
            assert lu == pytest.approx(np.exp(-q / (2 * l1)), rel=1e-9)      # Liu is exact for equal weights
            assert exact == pytest.approx(np.exp(-q / (2 * l1)), rel=1e-14)
        else:
            assert lu == pytest.approx(exact, rel=0.1, abs=1e-3)            # an approximation otherwise


def test_kernel_coordinates_match_the_restatement():
    rng = np.random.default_rng(3)
    loc = rng.uniform(0, 30, size=(200, 2))
    xt, inv, lam = pu.kernel_coordinates(loc)
    sets = [loc] + [ref.transloc_func_vec(loc, k, "gaussian") for k in range(5)] + \
        [ref.transloc_func_vec(loc, k, "cosine") for k in range(5)]
    for k, s in enumerate(sets):
        xc = s - s.mean(0)
        np.testing.assert_allclose(xt[:, 2 * k:2 * k + 2], xc, rtol=0, atol=1e-12 * np.abs(xc).max())
        np.testing.assert_allclose(inv[k].reshape(2, 2), np.linalg.inv(xc.T @ xc), rtol=1e-10)
        np.testing.assert_allclose(lam[k], [1.0, 1.0], rtol=1e-10)


def _tab(genes, adj, cluster):
    return np.asarray(genes), np.asarray(adj, dtype=float), np.asarray(cluster)


def test_select_svgs_rule():
    # time point 1 has the fewest SVGs (ties with 2: the first one wins) and is taken whole
    a = _tab([f"a{i:03d}" for i in range(300)], np.linspace(0, 1, 300), np.arange(300) % 3)
    b = _tab([f"b{i:03d}" for i in range(250)], np.linspace(0, 1, 250), np.zeros(250))
    c = _tab([f"c{i:03d}" for i in range(250)], np.linspace(0, 1, 250), np.zeros(250))
    got = pu.select_svgs([a, b, c])
    # quota max(100, round(250 / 3)) = 100 per cluster of a, and max(100, round(250 / 1)) = 250 of c
    want = set(b[0]) | set(c[0]) | {f"a{i:03d}" for i in range(300)}
    assert got == sorted(want)
    # quota: 250 / 100 = 2.5 rounds half to even -> 2, so max(100, 2) = 100; check with a larger min list
    big = _tab([f"d{i:04d}" for i in range(2500)], np.linspace(0, 1, 2500), np.arange(2500) % 10)
    small = _tab([f"s{i:04d}" for i in range(2250)], np.linspace(0, 1, 2250), np.zeros(2250))
    got = pu.select_svgs([big, small])          # round(2250 / 10) = 225 per cluster of `big`
    assert len([g for g in got if g.startswith("d")]) == 2250
    small = _tab([f"s{i:04d}" for i in range(1250)], np.linspace(0, 1, 1250), np.zeros(1250))
    got = pu.select_svgs([big, small])          # round(1250 / 10) = round(125.0) = 125
    assert len([g for g in got if g.startswith("d")]) == 1250
    odd = _tab([f"s{i:04d}" for i in range(1250)], np.linspace(0, 1, 1250), np.zeros(1250))
    big4 = _tab([f"d{i:04d}" for i in range(2500)], np.linspace(0, 1, 2500), np.arange(2500) % 4)
    got = pu.select_svgs([big4, odd])           # round(1250 / 4) = round(312.5) = 312 (half to even), not 313
    assert len([g for g in got if g.startswith("d")]) == 4 * 312
    # within a cluster the lowest adjusted p are taken; the result is sorted and duplicates merge
    x = _tab(["g2", "g1", "g3"], [0.3, 0.1, 0.2], [0, 0, 0])
    y = _tab(["g1", "g9"], [0.5, 0.5], [0, 1])
    assert pu.select_svgs([x, y]) == ["g1", "g2", "g3", "g9"]


def test_rank_genes_tie_order_and_count():
    adj = np.array([0.5, 0.01, 0.01, 0.01, 0.9])
    comb = np.array([0.4, 0.002, 0.001, 0.002, 0.8])
    order, n_keep = pu.rank_genes(adj, comb)
    assert order.tolist() == [2, 1, 3, 0, 4]
    assert n_keep == 5                            # min(G, max(#sig, 500))
    order, n_keep = pu.rank_genes(np.full(800, 0.01), np.full(800, 0.001))
    assert n_keep == 800 and order.tolist() == list(range(800))
    order, n_keep = pu.rank_genes(np.linspace(0, 1, 1000), np.linspace(0, 1, 1000))
    assert n_keep == 500


def _raw(n=30, g=12, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.poisson(1.0, size=(n, g)).astype(np.float32)
    tp = np.array(["b"] * (n // 2) + ["a"] * (n - n // 2))
    xy = rng.uniform(size=(n, 2))
    return X, tp, xy


def test_loader_dense_and_csr_npz_agree(tmp_path):
    X, tp, xy = _raw()
    np.savez(tmp_path / "dense.npz", X=X, timepoint=tp, spatial=xy, genes=np.array([f"g{i}" for i in range(12)]))
    C = sp.csr_matrix(X)
    np.savez(tmp_path / "csr.npz", X_data=C.data, X_indices=C.indices, X_indptr=C.indptr, X_shape=np.array(C.shape),
             timepoint=tp, spatial=xy)
    d, pd_ = pu.load_counts(str(tmp_path / "dense.npz"))
    c, pc = pu.load_counts(str(tmp_path / "csr.npz"))
    assert pd_ == os.path.abspath(tmp_path / "dense.npz")
    assert sp.isspmatrix_csr(d.X) and d.X.dtype == np.float32
    assert (d.X != c.X).nnz == 0
    np.testing.assert_array_equal(d.obs["timepoint"], c.obs["timepoint"])
    assert d.var_names.tolist() == [f"g{i}" for i in range(12)]
    assert c.var_names.tolist() == [str(i) for i in range(12)]
    assert pu.timepoint_order(d.obs["timepoint"]) == ["b", "a"]

    class Obj:
        pass
    o = Obj()
    o.X, o.obs, o.obsm = sp.csc_matrix(X), {"timepoint": tp}, {"spatial": xy}
    m, path = pu.load_counts(o)
    assert path is None and (m.X != d.X).nnz == 0


def test_loader_input_checks(tmp_path):
    X, tp, xy = _raw()
    np.savez(tmp_path / "no_tp.npz", X=X, spatial=xy)
    with pytest.raises(ValueError, match="`timepoint` column is not found"):
        pu.load_counts(str(tmp_path / "no_tp.npz"))
    np.savez(tmp_path / "no_sp.npz", X=X, timepoint=tp)
    with pytest.raises(ValueError, match="`spatial` key is not found"):
        pu.load_counts(str(tmp_path / "no_sp.npz"))
    np.savez(tmp_path / "sp1d.npz", X=X, timepoint=tp, spatial=xy[:, 0])
    with pytest.raises(ValueError, match="not a 2D numpy array"):
        pu.load_counts(str(tmp_path / "sp1d.npz"))

    class Obj:
        pass
    o = Obj()
    o.X, o.obs, o.obsm = X, {"timepoint": tp}, {"spatial": xy.tolist()}
    with pytest.raises(ValueError, match="not a 2D numpy array"):
        pu.load_counts(o)


def test_cli_preprocess_options():
    from spadot_amd import cli
    a = cli.parse_args(["preprocess", "-i", "x.npz"])
    assert a.feature_selection is True and a.device == "cuda:0" and a.prefix == "preprocessed_"
    a = cli.parse_args(["preprocess", "-i", "x.npz", "--no_feature_selection", "--device", "cuda:1"])
    assert a.feature_selection is False and a.device == "cuda:1"
    a = cli.parse_args(["preprocess", "-i", "x.npz", "--feature_selection"])
    assert a.feature_selection is True


def test_cli_preprocess_missing_input_message(capsys):
    from spadot_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["preprocess", "-i", "does_not_exist.npz"])
    assert e.value.code == 2
    assert "the data does not exist: does_not_exist.npz" in capsys.readouterr().err


def test_raw_count_generator_shape():
    from spadot_amd.synthetic import make_raw_counts
    d = make_raw_counts((50, 80), n_genes=200, n_modules=2, genes_per_module=10)
    assert d.X.shape == (130, 200) and d.X.dtype == np.float32
    assert (d.X.sum(1) == 0).sum() >= 2                           # one zero-total spot per time point
    det = (d.X[:50] >= 0.01).sum(0)
    assert (det[-5:] < 5).all()                                   # rarely detected genes
    assert d.X[:50, 200 - 6].sum() == 0                           # zero in the first time point
    assert (d.uns["module"][:20] >= 0).all() and (d.uns["module"][20:] == -1).all()
