"""CPU: the numpy restatement of the embed stage (tests/embed_ref.py) against sklearn's own pieces, pca_start against sklearn's
PCA, the command line's `embed` sub-command, and the refusals that come before the device."""
import argparse
import os

import numpy as np
import pytest

import embed_cases as cases
import embed_ref as ref


def _sk(name):
    """A private piece of sklearn 1.7's t-SNE, or a skip that says why."""
    try:
        if name == "_binary_search_perplexity":
            from sklearn.manifold import _utils
            return _utils._binary_search_perplexity
        from sklearn.manifold import _t_sne
        return getattr(_t_sne, name)
    except (ImportError, AttributeError) as e:
        pytest.skip(f"sklearn's {name} is not importable here: {e}")


# ------------------------------------------------------------------------------------------------ the restatement against sklearn
@pytest.mark.parametrize("d,n,u", [(20, 91, 30.0), (20, 300, 30.0), (8, 257, 5.0)])
def test_conditional_affinities_against_sklearns_binary_search(d, n, u):
    search = _sk("_binary_search_perplexity")
    X = cases.blobs(d, n, 100 + n)
    _idx, d2 = ref.knn(X, ref.n_neighbors(n, u))
    cond, beta = ref.conditional(d2, u)
    want = np.asarray(search(np.ascontiguousarray(d2, dtype=np.float32), u, 0), dtype=np.float64)
    gap = float(np.max(np.abs(cond - want)))
    print(f"conditional P against sklearn at ({d}, {n}, {u}): largest gap {gap:.3g}")
    assert gap <= 5e-5                                   # sklearn stops at an entropy tolerance of 1e-5 on float32 distances
    assert np.all(beta > 0)
    np.testing.assert_allclose(cond.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    H = -np.sum(np.where(cond > 0, cond * np.log(np.where(cond > 0, cond, 1.0)), 0.0), axis=1)
    np.testing.assert_allclose(H, np.log(u), rtol=0, atol=1e-9)


def test_joint_affinities_against_sklearns_dense_ones():
    from scipy.spatial.distance import squareform
    joint = _sk("_joint_probabilities")
    d, n, u = 20, 91, 30.0
    X = cases.blobs(d, n, 100 + n)
    idx, d2 = ref.knn(X, ref.n_neighbors(n, u))          # k = n - 1: every pair is stored
    cond, _beta = ref.conditional(d2, u)
    rowptr, col, val = ref.joint_csr(idx, cond)
    assert rowptr[-1] == n * (n - 1) and np.all(np.diff(rowptr) == n - 1)
    P = ref.dense(rowptr, col, val, n)
    want = squareform(np.asarray(joint(ref.sq_dists(X), u, 0), dtype=np.float64))
    gap = float(np.max(np.abs(P - want)))
    print(f"joint P against sklearn: largest gap {gap:.3g}")
    assert gap <= 1e-7
    np.testing.assert_array_equal(P, P.T)
    assert abs(P.sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("scale", [1e-4, 1.0, 10.0])
def test_gradient_and_kl_against_sklearns_kl_divergence(scale):
    from scipy.spatial.distance import squareform
    kl_div = _sk("_kl_divergence")
    d, n, u = 20, 91, 30.0
    X = cases.blobs(d, n, 100 + n)
    idx, d2 = ref.knn(X, ref.n_neighbors(n, u))
    rowptr, col, val = ref.joint_csr(idx, ref.conditional(d2, u)[0])
    Y = np.random.default_rng(5).normal(size=(n, 2)) * scale
    f = ref.forces(Y, rowptr, col, val, 1.0, 1)
    kl, grad = kl_div(Y.ravel().copy(), squareform(ref.dense(rowptr, col, val, n), checks=False), 1.0, n, 2)
    grad = grad.reshape(n, 2)
    top = float(np.max(np.abs(grad)))
    gap = float(np.max(np.abs(f["g"] - grad)))
    print(f"scale {scale}: gradient gap {gap / top:.3g} of the largest entry, KL gap {abs(f['kl'] - kl):.3g}")
    assert gap <= 1e-12 * top
    assert abs(f["kl"] - kl) <= 1e-12


def test_the_update_rule_is_sklearns_gradient_descent():
    """Three iterations of sklearn's _gradient_descent on the restatement's own gradient give the restatement's run."""
    gd = _sk("_gradient_descent")
    d, n, u = 20, 91, 30.0
    X = cases.blobs(d, n, 100 + n)
    idx, d2 = ref.knn(X, ref.n_neighbors(n, u))
    rowptr, col, val = ref.joint_csr(idx, ref.conditional(d2, u)[0])
    Y0 = ref.pca_start(X)
    lr = ref.default_learning_rate(n)

    def objective(p, *_a, **_k):
        f = ref.forces(p.reshape(n, 2), rowptr, col, val, 12.0, 1)
        return f["kl"], f["g"].ravel()

    want, _err, _it = gd(objective, Y0.ravel().copy(), it=0, max_iter=3, n_iter_check=10, momentum=0.5, learning_rate=lr,
                         min_gain=0.01, min_grad_norm=0.0)
    got, _u, _g, _kl = ref.run(Y0, rowptr, col, val, 3, early=250, lr=lr, slices=1)
    np.testing.assert_array_equal(got.ravel(), want)


def test_pca_start_against_sklearns_pca():
    from sklearn.decomposition import PCA
    from spadot_amd.embed import pca_start
    for d, n in ((20, 300), (8, 513), (3, 257)):
        X = cases.optimiser_case(d, n) if d > 3 else cases.neighbor_case("padded")[0]
        pca = PCA(n_components=2, svd_solver="full")
        want = pca.fit_transform(X)
        for c in range(2):                               # the stated sign rule: the entry of largest magnitude is positive
            if pca.components_[c, np.argmax(np.abs(pca.components_[c]))] < 0:
                want[:, c] = -want[:, c]
        want = want / np.std(want[:, 0]) * 1e-4
        got = pca_start(X)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * 1e-4 * 10)
        np.testing.assert_array_equal(got, ref.pca_start(X))
        assert abs(np.std(got[:, 0]) - 1e-4) <= 1e-18


def test_host_joint_csr_is_the_restatements():
    from spadot_amd.embed import joint_csr
    for name in ("dense", "padded", "duplicates", "uniform", "lattice"):
        X, u = cases.neighbor_case(name)
        idx, d2 = ref.knn(X, ref.n_neighbors(X.shape[0], u))
        cond, _beta = ref.conditional(d2, u)
        rowptr, col, val = joint_csr(idx, cond)
        rp, cj, v = ref.joint_csr(idx, cond)
        np.testing.assert_array_equal(rowptr, rp)
        np.testing.assert_array_equal(col, cj)
        np.testing.assert_allclose(val, v, rtol=1e-14, atol=0)
        assert col.dtype == np.int32 and rowptr.dtype == np.int64
        lens = np.diff(rowptr)
        assert lens.min() >= idx.shape[1] and lens.max() <= X.shape[0] - 1


def test_the_restatement_on_the_degenerate_cases():
    X, u = cases.neighbor_case("uniform")
    idx, d2 = ref.knn(X, ref.n_neighbors(X.shape[0], u))
    assert np.all(d2 == 0.0)
    np.testing.assert_array_equal(idx[0], np.arange(1, 31))      # ties broken by index, self left out by index
    np.testing.assert_array_equal(idx[5, :6], [0, 1, 2, 3, 4, 6])
    cond, beta = ref.conditional(d2, u)
    assert np.all(beta == 0.0) and np.all(cond == 1.0 / 30)
    X, u = cases.neighbor_case("duplicates")
    idx, d2 = ref.knn(X, 30)
    cond, beta = ref.conditional(d2, u)
    dup = np.flatnonzero(np.all(X == X[0], axis=1))
    assert dup.shape[0] == 40
    assert np.all(beta[dup] == 0.0) and np.all(cond[dup] == 1.0 / 30)       # 39 neighbours at distance 0: uniform
    assert np.all(np.isfinite(cond)) and np.all(np.isfinite(beta))
    X, u = cases.neighbor_case("lattice")
    idx, d2 = ref.knn(X, 12)
    np.testing.assert_array_equal(d2[0], [1, 1, 2, 4, 4, 5, 5, 8, 9, 9, 10, 10])
    np.testing.assert_array_equal(idx[0], [1, 20, 21, 2, 40, 22, 41, 42, 3, 60, 23, 61])


def test_slice_rule_and_table():
    from spadot_amd import stage_ops as so
    assert [so.embed_slices(n) for n in (91, 256, 257, 513, 10000, 50000, 10 ** 6)] == [1, 1, 2, 3, 26, 6, 1]
    assert [ref.default_slices(n) for n in (91, 256, 257, 513, 10000, 50000, 10 ** 6)] == [1, 1, 2, 3, 26, 6, 1]
    assert -(-50000 // 256) * so.embed_slices(50000) >= 4 * 256             # four workgroups per CU at 50 000 points
    desc, perp = so.embed_table([300, 91, 513], [30.0, 30.0, 5.0], nnz=[10, 20, 30])
    assert desc.tolist() == [[0, 300, 90, 0, 2, 0, 0, 0, 0, 10], [300, 91, 90, 27000, 1, 600, 301, 10, 2, 20],
                             [391, 513, 15, 35190, 3, 691, 393, 30, 3, 30]]
    assert perp.tolist() == [30.0, 30.0, 5.0]
    with pytest.raises(ValueError, match="slices"):
        so.embed_table([513], 5.0, slices=0)
    with pytest.raises(ValueError, match="1 GiB"):
        so.embed_table([2 ** 24], 30.0, slices=3)


# ------------------------------------------------------------------------------------------------------------ parser and CLI
def test_parser_takes_the_embed_subcommand_and_keeps_the_others():
    from spadot_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(["embed", "-i", "latent.npz"])
    assert (a.cmd_choice, a.data, a.domains, a.output_dir, a.prefix, a.perplexity, a.n_iter, a.early, a.learning_rate,
            a.per_timepoint, a.device) == ("embed", "latent.npz", None, None, "", 30.0, 1000, 250, None, False, "cuda:0")
    a = p.parse_args(["embed", "-i", "l.npz", "--domains", "d.csv", "-o", "out", "--prefix", "p_", "--perplexity", "12.5",
                      "--n_iter", "50", "--early", "20", "--learning_rate", "80", "--per_timepoint", "--device", "cuda:1"])
    assert (a.domains, a.output_dir, a.prefix, a.perplexity, a.n_iter, a.early, a.learning_rate, a.per_timepoint, a.device) == \
        ("d.csv", "out", "p_", 12.5, 50, 20, 80.0, True, "cuda:1")
    assert not hasattr(a, "seed")                                            # nothing is random
    with pytest.raises(SystemExit):
        p.parse_args(["embed"])                                              # -i is required
    for cmd, argv in (("preprocess", ["-i", "x"]), ("train", ["-i", "x"]), ("analyze", ["-i", "x"]),
                      ("markers", ["-i", "x", "--domains", "d"]), ("score", ["-i", "x", "--domains", "d"]), ("trends", ["-i", "x"]),
                      ("neighbors", ["--domains", "d"]), ("cooccurrence", ["--domains", "d"]), ("autocorr", ["-i", "x"]),
                      ("hotspots", ["-i", "x"]), ("modules", ["-i", "x"]), ("ripley", ["--domains", "d"]),
                      ("correlogram", ["-i", "x"]), ("ligrec", ["-i", "x", "--domains", "d", "--interactions", "c"])):
        assert p.parse_args([cmd] + argv).cmd_choice == cmd


def test_cli_reports_a_missing_file(tmp_path, capsys):
    from spadot_amd.cli import main
    with pytest.raises(SystemExit) as e:
        main(["embed", "-i", os.path.join(str(tmp_path), "nope.npz")])
    assert e.value.code == 2
    assert "does not exist" in capsys.readouterr().err
    np.savez(os.path.join(str(tmp_path), "latent.npz"), X=np.zeros((4, 2)), timepoint=np.zeros(4), spatial=np.zeros((4, 2)))
    with pytest.raises(SystemExit) as e:
        main(["embed", "-i", os.path.join(str(tmp_path), "latent.npz"), "--domains", os.path.join(str(tmp_path), "d.csv")])
    assert e.value.code == 2
    assert "domains table does not exist" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------- refusals before the device
def _args(data, **kw):
    base = dict(data=data, domains=None, output_dir=None, prefix="", perplexity=30.0, n_iter=10, early=5, learning_rate=None,
                per_timepoint=False, device="cuda:0")
    base.update(kw)
    return argparse.Namespace(**base)


def _latents(sizes=(60, 70), d=20, seed=3):
    from spadot_amd.synthetic import SpatialData
    X = np.random.default_rng(seed).normal(size=(sum(sizes), d))
    tp = np.concatenate([[f"T{t}"] * n for t, n in enumerate(sizes)])
    return SpatialData(X, tp, np.zeros((sum(sizes), 2)))


def test_refusals_before_the_device(tmp_path):
    import pandas as pd
    import torch
    from spadot_amd.embed import embed, latent_knn, tsne, tsne_many
    out = str(tmp_path)
    for u in (1.5, 50.5, float("nan")):
        with pytest.raises(ValueError, match="perplexity"):
            embed(_args(_latents(), perplexity=u, output_dir=out))
        with pytest.raises(ValueError, match="perplexity"):
            tsne(torch.zeros((200, 4), dtype=torch.float64), perplexity=u)
    with pytest.raises(ValueError, match="needs at least 32"):
        embed(_args(_latents((15, 16)), output_dir=out))                     # 31 spots in all at perplexity 30
    with pytest.raises(ValueError, match="problem 0 has 31 points.*time points"):
        embed(_args(_latents((31, 70)), per_timepoint=True, output_dir=out))  # one time point is too small; jointly it is not
    with pytest.raises(ValueError, match="needs at least 32"):
        tsne_many([torch.zeros((40, 4), dtype=torch.float64), torch.zeros((31, 4), dtype=torch.float64)])
    with pytest.raises(ValueError, match="33 dimensions"):
        embed(_args(_latents(d=33), output_dir=out))
    with pytest.raises(ValueError, match="1 to 32 dimensions"):
        tsne(torch.zeros((100, 33), dtype=torch.float64))
    bad = _latents()
    bad.X[17, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        embed(_args(bad, output_dir=out))
    data = _latents()
    table = pd.DataFrame({"row": np.arange(129), "timepoint": data.obs["timepoint"][:129], "kmeans": np.zeros(129, dtype=int)})
    with pytest.raises(ValueError, match="has no label in the domains table"):
        embed(_args(data, domains=table, output_dir=out))                    # a domains table that misses a row
    table = pd.DataFrame({"row": np.arange(130), "timepoint": data.obs["timepoint"][::-1], "kmeans": np.zeros(130, dtype=int)})
    with pytest.raises(ValueError, match="time point mismatch"):
        embed(_args(data, domains=table, output_dir=out))
    assert os.listdir(out) == []                                             # nothing was written
    with pytest.raises(RuntimeError, match="MI355X only"):
        tsne(torch.zeros((100, 4), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="MI355X only"):
        latent_knn(torch.zeros((100, 4), dtype=torch.float64), 5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        embed(_args(_latents(), device="cpu", output_dir=out))
    with pytest.raises(ValueError, match="min\\(n - 1, 150\\)"):
        latent_knn(torch.zeros((100, 4), dtype=torch.float64), 151)
