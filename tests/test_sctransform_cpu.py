"""CPU: the SCTransform host helpers (bw.SJ, ksmooth, outliers, the step-1 draw) against the restatement of tests/sct_ref.py,
the Louvain gene clusters, the Gaussian gene graph and the --gene_clusters option."""
import numpy as np
import pytest
import scipy.sparse as sp

import sct_ref as ref
from spadot_amd.utils import _sctransform_utils as su


@pytest.mark.parametrize("n", [60, 500, 501, 3000])
def test_bw_sj_both_paths_match_the_restatement(n):
    rng = np.random.default_rng(n)
    x = np.concatenate([rng.normal(-1.0, 0.4, n - n // 5), rng.normal(0.5, 0.2, n // 5)])
    np.testing.assert_allclose(su.bw_sj(x), ref.bw_sj(x), rtol=1e-12)


def test_ksmooth_matches_a_direct_windowed_sum():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, 700)
    y = np.cos(2 * x) + 0.1 * rng.normal(size=x.size)
    xp = np.concatenate([rng.uniform(-3, 3, 400), [-10.0, 10.0]])      # two points with an empty window
    bw = 0.4
    got = su.ksmooth(x, y, xp, bw)
    xs, want = ref.ksmooth(x, y, xp, bw)
    o = np.argsort(xp, kind="stable")
    np.testing.assert_allclose(got[o], want, rtol=0, atol=1e-12)
    b = bw * 0.3706506
    for j in (0, 17, 399):                                                # a plain windowed sum at a few points
        m = np.abs(x - xp[j]) <= 4 * b
        w = np.exp(-0.5 * ((x[m] - xp[j]) / b) ** 2)
        assert abs(got[j] - (w * y[m]).sum() / w.sum()) <= 1e-12
    assert got[-1] == 0.0 and got[-2] == 0.0


def test_is_outlier_flags_crafted_outliers():
    rng = np.random.default_rng(5)
    x = np.sort(rng.normal(-1, 0.5, 900))
    y = 0.3 * x + 0.05 * rng.normal(size=x.size)
    bad = np.array([10, 300, 450, 801])
    y[bad] += np.array([3.0, -4.0, 5.0, 2.5])
    got = su.is_outlier(y, x)
    np.testing.assert_array_equal(got, ref.is_outlier(y, x))
    assert set(bad) <= set(np.flatnonzero(got))
    assert got.sum() <= bad.size + 5


def test_step1_draw_is_deterministic_and_matches_the_restatement():
    rng = np.random.default_rng(9)
    lg = np.concatenate([rng.normal(-1.5, 0.3, 2600), rng.normal(0.2, 0.4, 400)])
    a = su.sample_step1(lg, 2000, 1448145)
    b = su.sample_step1(lg, 2000, 1448145)
    np.testing.assert_array_equal(a, b)
    assert a.size == 2000 and np.all(np.diff(a) > 0)
    np.testing.assert_array_equal(a, ref.step1_set(lg, 2000, 1448145))
    np.testing.assert_array_equal(su.sample_step1(lg[:1500], 2000), np.arange(1500))


def _planted(sizes, p_in, p_out, seed):
    rng = np.random.default_rng(seed)
    lab = np.repeat(np.arange(len(sizes)), sizes)
    n = lab.size
    P = np.where(lab[:, None] == lab[None, :], p_in, p_out)
    U = np.triu(rng.uniform(size=(n, n)) < P, 1)
    W = rng.uniform(0.5, 1.5, size=(n, n)) * U
    return sp.csr_matrix(W + W.T), lab


def test_louvain_recovers_planted_cliques():
    blocks = [sp.csr_matrix(np.ones((s, s)) - np.eye(s)) for s in (8, 7, 6, 5)]
    W = sp.block_diag(blocks).tolil()
    W[7, 8] = W[8, 7] = 0.1                      # weak bridges between the cliques
    W[14, 15] = W[15, 14] = 0.1
    W[20, 21] = W[21, 20] = 0.1
    lab = su.louvain(W.tocsr(), 1.0, seed=0)
    want = np.repeat(np.arange(4), (8, 7, 6, 5))  # renumbered by size, descending
    np.testing.assert_array_equal(lab, want)


@pytest.mark.parametrize("gamma", [1.0, 1.5])
def test_louvain_modularity_matches_networkx(gamma):
    import networkx as nx
    W, _ = _planted([40, 35, 30, 25, 20], 0.3, 0.02, seed=11)
    G = nx.from_scipy_sparse_array(W)
    ours, theirs = [], []
    for s in range(5):                           # both are randomised local searches: compare their means over seeds
        lab = su.louvain(W, gamma, seed=s)
        ours.append(su.modularity(W, lab, gamma))
        groups = [set(np.flatnonzero(lab == c)) for c in np.unique(lab)]
        np.testing.assert_allclose(ours[-1], nx.community.modularity(G, groups, weight="weight", resolution=gamma), rtol=1e-12)
        theirs.append(nx.community.modularity(G, nx.community.louvain_communities(G, weight="weight", resolution=gamma,
                                                                                  seed=s), weight="weight", resolution=gamma))
    assert np.mean(ours) >= np.mean(theirs) - 1e-3


def test_louvain_is_deterministic_per_seed():
    W, _ = _planted([30, 30, 30], 0.2, 0.05, seed=2)
    np.testing.assert_array_equal(su.louvain(W, 1.0, seed=4), su.louvain(W, 1.0, seed=4))


def test_resolution_loop_stops_at_the_first_gamma_with_enough_communities():
    W, _ = _planted([25] * 12, 0.5, 0.03, seed=4)
    lab, gamma = su.cluster_by_resolution(W, k=10)
    assert np.unique(lab).size >= 10
    g, seen = 1.0, []
    while True:                                  # the same float accumulation: every earlier gamma has < 10 communities
        n = np.unique(su.louvain(W, g, 0)).size
        seen.append(n)
        if n >= 10:
            break
        g += 0.1
    assert g == gamma and all(n < 10 for n in seen[:-1])
    small, _ = _planted([3, 3], 1.0, 0.0, seed=1)
    lab, _ = su.cluster_by_resolution(small, k=10)            # S = 6 < 10: the target becomes S
    assert np.unique(lab).size == 6
    with pytest.raises(RuntimeError, match="fewer than"):
        su.cluster_by_resolution(W, k=300, gamma_max=1.3)


def test_gauss_graph_is_symmetric_without_self_loops_and_uses_the_median_rule():
    rng = np.random.default_rng(8)
    pcs = rng.normal(size=(150, 5))
    k = 20
    W = su.gauss_knn_graph(pcs, k=k)
    assert (abs(W - W.T)).max() < 1e-15
    assert W.diagonal().max() == 0.0
    D2 = ((pcs[:, None, :] - pcs[None, :, :]) ** 2).sum(-1)
    order = np.argsort(D2, axis=1, kind="stable")
    nbr = [o[o != i][:k - 1] for i, o in enumerate(order)]
    sig2 = np.array([np.median(D2[i, nbr[i]]) for i in range(150)])
    for i in (0, 33, 149):
        for j in nbr[i][:5]:
            den = sig2[i] + sig2[j]
            want = np.sqrt(2 * np.sqrt(sig2[i] * sig2[j]) / den) * np.exp(-D2[i, j] / den)
            np.testing.assert_allclose(W[i, j], want, rtol=1e-10)
    far = [j for j in range(150) if j not in nbr[0] and 0 not in nbr[j] and j != 0]
    assert all(W[0, j] == 0 for j in far)


def test_cli_gene_clusters_option():
    from spadot_amd import cli
    assert cli.parse_args(["preprocess", "-i", "x.npz"]).gene_clusters == "kmeans"
    assert cli.parse_args(["preprocess", "-i", "x.npz", "--gene_clusters", "louvain"]).gene_clusters == "louvain"
    with pytest.raises(SystemExit):
        cli.parse_args(["preprocess", "-i", "x.npz", "--gene_clusters", "leiden"])


def test_sctransform_wrapper_refuses_what_the_reference_does_not_do():
    from spadot_amd.sctransform import SCTransform
    X = sp.csr_matrix(np.ones((5, 4)))
    with pytest.raises(NotImplementedError):
        SCTransform(X, np.arange(5), np.arange(4), reference_sct_model=object())
    with pytest.raises(NotImplementedError):
        SCTransform(X, np.arange(5), np.arange(4), method="glmGamPoi")
