"""GPU: the embed stage (csrc/embed.hip, spadot_amd/embed.py) against the numpy restatement of tests/embed_ref.py:
the neighbours exactly, the affinities and every sum of one iteration within the stated rounding bounds, the update rule bit for
bit, the bitwise invariances, one run against sklearn's exact t-SNE, and the stage's files."""
import functools
import os

import numpy as np
import pytest

import embed_cases as cases
import embed_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
C = 8                                    # roundings per term: the subtraction, pc_d2 (3), 1 + d2, the division, the products


def _dev(X):
    import torch
    return torch.as_tensor(np.ascontiguousarray(X), device="cuda:0")


@functools.lru_cache(maxsize=None)
def _neighbor_run(name):
    """(X, u, the device's affinities, the restatement's idx, d2, cond, beta) of a neighbour case, computed once."""
    from spadot_amd.embed import tsne_affinities
    X, u = cases.neighbor_case(name)
    got = tsne_affinities(_dev(X), u)
    idx, d2 = ref.knn(X, ref.n_neighbors(X.shape[0], u))
    cond, beta = ref.conditional(d2, u)
    return X, u, got, idx, d2, cond, beta


@functools.lru_cache(maxsize=None)
def _optimiser_run(d, n, u):
    """(X, the device's joint CSR, {state name: (Y, update, gains, iteration number, early)}) of an optimiser case: the start, the
    restatement's state after 60 iterations and, for n = 300, after 300 iterations with early = 250."""
    from spadot_amd.embed import tsne_affinities
    X = cases.optimiser_case(d, n)
    aff = tsne_affinities(_dev(X), u)
    csr = (aff["rowptr"], aff["col"], aff["val"])
    Y0 = ref.pca_start(X)
    states = {"start": (Y0, np.zeros((n, 2)), np.ones((n, 2)), 0, 250)}
    Y, upd, gains, _kl = ref.run(Y0, *csr, 60, early=250)
    states["after60"] = (Y, upd, gains, 60, 250)
    if n == 300:
        Y, upd, gains, _kl = ref.run(Y, *csr, 240, early=250, it0=60, update=upd, gains=gains)
        states["after300"] = (Y, upd, gains, 300, 250)
    return X, csr, states


# --------------------------------------------------------------------------------------------------------------- neighbours
@pytest.mark.parametrize("name", [c[0] for c in cases.NEIGHBOR_CASES])
def test_neighbours_equal_the_restatement(name):
    X, u, got, idx, d2, _cond, _beta = _neighbor_run(name)
    assert got["idx"].dtype == np.int32 and got["idx"].shape == idx.shape
    np.testing.assert_array_equal(got["idx"], idx)                           # ties and duplicates included
    gap = np.abs(got["d2"] - d2)
    print(f"{name}: largest relative gap of d2 {float(np.max(gap / np.where(d2 > 0, d2, 1.0))):.3g}")
    assert np.all(gap <= X.shape[1] * 2.0 ** -52 * d2)
    assert not np.any(got["idx"] == np.arange(X.shape[0])[:, None])          # self is left out by index


def test_latent_knn_alone_and_for_any_k():
    from spadot_amd.embed import latent_knn
    X, _u = cases.neighbor_case("largest")
    for k in (1, 7, 150):
        idx, d2 = latent_knn(_dev(X), k)
        want_idx, want_d2 = ref.knn(X, k)
        np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
        np.testing.assert_array_equal(d2.cpu().numpy(), want_d2)             # unfused on both sides: the same bits


def test_three_problems_in_one_launch_give_the_bits_of_each_alone():
    from spadot_amd.embed import TsneBatch
    Xs = [cases.blobs(20, n, 300 + n) for n in cases.BATCH_SIZES]
    batch = TsneBatch([_dev(x) for x in Xs], 30.0, n_iter=0)
    idx, d2, cond, beta = (t.cpu().numpy() for t in (batch.idx, batch.d2, batch.cond, batch.beta))
    for p, x in enumerate(Xs):
        alone = TsneBatch([_dev(x)], 30.0, n_iter=0)
        off, n, k, koff = (int(v) for v in batch.desc[p, :4])
        np.testing.assert_array_equal(idx[koff:koff + n * k], alone.idx.cpu().numpy())
        np.testing.assert_array_equal(d2[koff:koff + n * k], alone.d2.cpu().numpy())
        np.testing.assert_array_equal(cond[koff:koff + n * k], alone.cond.cpu().numpy())
        np.testing.assert_array_equal(beta[off:off + n], alone.beta.cpu().numpy())
        np.testing.assert_array_equal(idx[koff:koff + n * k].reshape(n, k), ref.knn(x, k)[0])
        for a, b in zip(batch.csr_host[p], alone.csr_host[0]):
            np.testing.assert_array_equal(a, b)


# --------------------------------------------------------------------------------------------------------------- affinities
@pytest.mark.parametrize("name", [c[0] for c in cases.NEIGHBOR_CASES])
def test_affinities_against_the_restatement(name):
    X, u, got, idx, d2, cond, beta = _neighbor_run(name)
    n, k = idx.shape
    top = cond.max(axis=1, keepdims=True)
    gap = float(np.max(np.abs(got["cond"] - cond) / top))
    print(f"{name}: conditional P within {gap:.3g} of the row's largest entry")
    assert gap <= 1e-9
    np.testing.assert_allclose(got["cond"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    e = d2 - d2.min(axis=1, keepdims=True)
    regular = (e == 0.0).sum(axis=1) < u                 # fewer neighbours at the smallest distance than the perplexity
    p = got["cond"]
    H = -np.sum(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0), axis=1)
    if regular.any():
        print(f"{name}: entropy within {float(np.max(np.abs(H[regular] - np.log(u)))):.3g} of log u on {int(regular.sum())} rows")
        assert np.all(np.abs(H[regular] - np.log(u)) <= 1e-9)
    flat = e.max(axis=1) == 0.0                          # the uniform rule
    assert np.all(got["beta"][flat] == 0.0) and np.all(got["cond"][flat] == 1.0 / k)
    np.testing.assert_array_equal(got["beta"] == 0.0, beta == 0.0)
    if name == "uniform":
        assert flat.all()
    if name == "duplicates":
        assert flat.sum() >= 40
        np.testing.assert_array_equal(got["cond"][flat], cond[flat])
    rowptr, col, val = got["rowptr"], got["col"], got["val"]
    P = ref.dense(rowptr, col, val, n)
    np.testing.assert_array_equal(P, P.T)
    assert abs(val.sum() - 1.0) <= 1e-12
    lens = np.diff(rowptr)
    assert lens.min() >= k and lens.max() <= n - 1
    assert all(np.all(np.diff(col[rowptr[i]:rowptr[i + 1]]) > 0) for i in range(n))      # columns ascending


def test_beta_runs_to_the_end_of_the_search_where_the_entropy_is_out_of_reach():
    """Twelve copies of a point among k = 30 neighbours at perplexity 10: the entropy stays above log 10 and beta doubles 200 times."""
    from spadot_amd.embed import tsne_affinities
    X = cases.blobs(8, 130, 77)
    X[1:12] = X[0]
    got = tsne_affinities(_dev(X), 10.0)
    _idx, d2 = ref.knn(X, 30)
    cond, beta = ref.conditional(d2, 10.0)
    assert np.all(beta[:12] == 2.0 ** 200)
    np.testing.assert_array_equal(got["beta"][:12], beta[:12])
    np.testing.assert_array_equal(got["cond"][:12], cond[:12])               # 1 / 11 on the copies, exact zeros elsewhere
    assert np.all(np.isfinite(got["cond"])) and np.all(np.isfinite(got["val"]))


# ----------------------------------------------------------------------------------------------------------------- one step
def _one_step(X, u, state, slices, two=False):
    from spadot_amd.embed import TsneBatch
    Y, upd, gains, it, early = state
    batch = TsneBatch([_dev(X)], u, n_iter=it + 1, early=early, slices=slices, start=[(Y, upd, gains)], it0=it, two=two)
    batch.steps(1)
    out = batch.download("Y", "zr", "att", "grad", "Z", "gains", "upd", "kl")[0]
    out["lr"] = batch.learning_rate[0]
    out["it_kl"] = out["kl"][it]
    return out


@pytest.mark.parametrize("d,n,u", cases.OPTIMISER_CASES)
def test_one_step_against_the_restatement(d, n, u):
    X, csr, states = _optimiser_run(d, n, u)
    rows = np.diff(csr[0])
    for which, state in states.items():
        Y, upd, gains, it, early = state
        for slices in ((1, 2, 3, 4) if n == 513 else (1, 2)):
            eps, mu = ref.phase(it, early)
            f = ref.forces(Y, *csr, eps, slices)
            got = _one_step(X, u, state, slices)
            z, r, a, g, Z = got["zr"][:, 0], got["zr"][:, 1:], got["att"], got["grad"], float(got["Z"])
            bz = C * (n - 1) * U * f["z_abs"]
            br = C * (n - 1) * U * f["r_abs"]
            bZ = C * (2 * n) * U * f["Z"]
            ba = C * rows[:, None] * U * f["a_abs"]
            print(f"({d}, {n}, {u}) {which} slices {slices}: z {float(np.max(np.abs(z - f['z']) / bz)):.3g}, "
                  f"r {float(np.max(np.abs(r - f['r']) / br)):.3g}, Z {abs(Z - f['Z']) / bZ:.3g}, "
                  f"a {float(np.max(np.abs(a - f['a']) / ba)):.3g} of their bounds; kl gap {abs(got['it_kl'] - f['kl']):.3g}")
            assert np.all(np.abs(z - f["z"]) <= bz)
            assert np.all(np.abs(r - f["r"]) <= br)
            assert abs(Z - f["Z"]) <= bZ
            assert np.all(np.abs(a - f["a"]) <= ba)
            bg = (4.0 * (ba + br / f["Z"] + np.abs(f["r"]) * bZ / f["Z"] ** 2)
                  + C * U * 4.0 * (np.abs(f["a"]) + np.abs(f["r"]) / f["Z"]))
            assert np.all(np.abs(g - f["g"]) <= bg)
            assert abs(got["it_kl"] - f["kl"]) <= 1e-12
            Yn, un, gn = ref.apply_update(Y, upd, gains, g, mu, got["lr"])   # numpy's update rule on the device's own gradient
            np.testing.assert_array_equal(got["gains"], gn)
            np.testing.assert_array_equal(got["upd"], un)
            np.testing.assert_array_equal(got["Y"], Yn)
            if which == "after60":
                assert np.unique(gains).size > n                  # mixed gains: raised here, lowered there
    if n == 513:                                          # an empty slice adds exact zeros: four slices of three tiles
        one, four = _one_step(X, u, states["start"], 3), _one_step(X, u, states["start"], 4)
        np.testing.assert_array_equal(one["zr"], four["zr"])


def test_two_query_points_per_thread_give_the_same_bits():
    X, _csr, states = _optimiser_run(8, 513, 5.0)
    for slices in (1, 3):
        a, b = _one_step(X, 5.0, states["after60"], slices), _one_step(X, 5.0, states["after60"], slices, two=True)
        for key in ("zr", "att", "grad", "Y", "kl"):
            np.testing.assert_array_equal(a[key], b[key])


# ------------------------------------------------------------------------------------------------------ bitwise invariances
def test_bitwise_invariances_of_a_run():
    from spadot_amd.embed import TsneBatch, tsne
    X = cases.optimiser_case(20, 300)
    once = tsne(_dev(X), 30.0, n_iter=120, early=40)
    assert np.all(np.isfinite(once.embedding)) and np.all(np.isfinite(once.kl)) and once.kl.shape == (120,)
    batch = TsneBatch([_dev(X)], 30.0, n_iter=120, early=40)
    for _ in range(120):
        batch.steps(1)
    single = batch.results()[0]
    np.testing.assert_array_equal(single.embedding, once.embedding)
    np.testing.assert_array_equal(single.kl, once.kl)
    again = tsne(_dev(X), 30.0, n_iter=120, early=40)
    np.testing.assert_array_equal(again.embedding, once.embedding)
    np.testing.assert_array_equal(again.kl, once.kl)
    two = TsneBatch([_dev(X)], 30.0, n_iter=120, early=40, two=True)
    two.steps(120)
    np.testing.assert_array_equal(two.results()[0].embedding, once.embedding)


def test_a_problem_in_a_batch_has_the_bits_of_the_problem_alone():
    """(20, 300, 30) beside (20, 91, 30) and (8, 513, 5): one launch per kernel, the bits of every problem alone."""
    from spadot_amd.embed import tsne, tsne_many
    X = cases.optimiser_case(20, 300)
    a, b = cases.optimiser_case(20, 91), cases.optimiser_case(8, 513)
    once = tsne(_dev(X), 30.0, n_iter=120, early=40)
    res = tsne_many([_dev(a), _dev(X), _dev(b)], [30.0, 30.0, 5.0], n_iter=120, early=40)
    np.testing.assert_array_equal(res[1].embedding, once.embedding)
    np.testing.assert_array_equal(res[1].kl, once.kl)
    np.testing.assert_array_equal(res[1].beta, once.beta)
    assert [r.slices for r in res] == [1, 2, 3] and [r.n_neighbors for r in res] == [90, 90, 15]
    alone = tsne(_dev(b), 5.0, n_iter=120, early=40)     # the narrower set was padded with zero coordinates
    np.testing.assert_array_equal(res[2].embedding, alone.embedding)
    np.testing.assert_array_equal(res[2].kl, alone.kl)


# --------------------------------------------------------------------------------------------------------------- end to end
def test_a_run_with_the_defaults_against_sklearns_exact_tsne():
    from sklearn.manifold import TSNE, trustworthiness
    from spadot_amd.embed import tsne
    X = cases.optimiser_case(20, 300)
    got = tsne(_dev(X))
    assert got.n_iter == 1000 and got.early == 250 and got.learning_rate == 50.0 and got.kl.shape == (1000,)
    kls, trusts = [], []
    for init, seed in (("pca", 0), ("random", 1)):
        sk = TSNE(perplexity=30, method="exact", init=init, random_state=seed)
        trusts.append(trustworthiness(X, sk.fit_transform(X), n_neighbors=10))
        kls.append(float(sk.kl_divergence_))
    trust = trustworthiness(X, got.embedding, n_neighbors=10)
    print(f"device: KL {got.kl[-1]:.4f}, trustworthiness {trust:.4f}; sklearn exact: KL {kls}, trustworthiness {trusts}")
    assert got.kl[-1] <= 1.05 * max(kls)
    assert trust >= min(trusts) - 0.01
    assert got.kl[-1] < got.kl[250]


# ---------------------------------------------------------------------------------------------------------------- the stage
def test_the_stage_writes_its_files_joint_and_per_time_point(tmp_path):
    import pandas as pd
    from spadot_amd.cli import main
    from spadot_amd.embed import tsne
    from spadot_amd.utils._analyze_utils import have_matplotlib
    X, tp, spatial, rows, lab = cases.stage_latents()
    out = str(tmp_path)
    latent = os.path.join(out, "latent.npz")
    np.savez(latent, X=X, timepoint=tp, spatial=spatial, rows=rows)
    shuffle = np.random.default_rng(1).permutation(X.shape[0])               # the table has an order of its own
    pd.DataFrame({"row": rows[shuffle], "timepoint": tp[shuffle], "kmeans": lab[shuffle]}).to_csv(
        os.path.join(out, "domains.csv"), index=False)
    main(["embed", "-i", latent, "--domains", os.path.join(out, "domains.csv"), "--n_iter", "50", "--prefix", "joint_"])
    main(["embed", "-i", latent, "--n_iter", "50", "--per_timepoint", "-o", os.path.join(out, "per"), "--prefix", "tp_"])
    joint = pd.read_csv(os.path.join(out, "joint_embedding.csv"), float_precision="round_trip")
    assert list(joint.columns) == ["row", "timepoint", "tsne_1", "tsne_2", "kmeans"]
    np.testing.assert_array_equal(joint["row"], rows)                        # input order, the latents' own ids
    np.testing.assert_array_equal(joint["timepoint"], tp)
    np.testing.assert_array_equal(joint["kmeans"], lab)
    z = np.load(os.path.join(out, "joint_embedding.npz"))
    assert sorted(z.files) == sorted(["Y", "kl", "beta", "perplexity", "n_iter", "early", "learning_rate", "slices", "offsets",
                                      "per_timepoint", "timepoints"])
    want = tsne(_dev(X), n_iter=50)
    np.testing.assert_array_equal(z["Y"], want.embedding)                    # the joint one: tsne of the stacked latents
    np.testing.assert_array_equal(z["kl"], want.kl[None])
    np.testing.assert_array_equal(z["beta"], want.beta)
    np.testing.assert_array_equal(np.asarray(joint[["tsne_1", "tsne_2"]]), want.embedding)
    assert z["offsets"].tolist() == [0, 677] and int(z["n_iter"]) == 50 and int(z["early"]) == 250 and z["slices"].tolist() == [3]
    per = pd.read_csv(os.path.join(out, "per", "tp_embedding.csv"), float_precision="round_trip")
    assert list(per.columns) == ["row", "timepoint", "tsne_1", "tsne_2"]
    np.testing.assert_array_equal(per["row"], rows)
    zp = np.load(os.path.join(out, "per", "tp_embedding.npz"))
    assert zp["timepoints"].tolist() == ["E1", "E2", "E3"] and zp["offsets"].tolist() == [0, 120, 377, 677]
    assert zp["kl"].shape == (3, 50) and zp["slices"].tolist() == [1, 2, 2]
    for t, name in enumerate(("E1", "E2", "E3")):
        m = tp == name
        alone = tsne(_dev(X[m]), n_iter=50)
        np.testing.assert_array_equal(zp["Y"][m], alone.embedding)           # bit for bit the time point alone
        np.testing.assert_array_equal(zp["kl"][t], alone.kl)
    np.testing.assert_array_equal(np.asarray(per[["tsne_1", "tsne_2"]]), zp["Y"])
    if have_matplotlib():
        assert os.path.getsize(os.path.join(out, "joint_embedding.png")) > 0
        assert os.path.getsize(os.path.join(out, "per", "tp_embedding.png")) > 0


def test_refusals_on_the_device():
    import torch
    from spadot_amd import stage_ops as so
    from spadot_amd.embed import tsne
    X = cases.optimiser_case(20, 91)
    bad = X.copy()
    bad[5, 2] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        tsne(_dev(bad), n_iter=1)
    desc, _perp = so.embed_table([4], 2.0, nnz=[4])
    rowptr = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int64, device="cuda:0")
    col = torch.tensor([1, 0, 3, 2], dtype=torch.int32, device="cuda:0")
    val = torch.full((4,), 0.25, dtype=torch.float64, device="cuda:0")
    so.tsne_csr_check(desc, rowptr, col, val)
    with pytest.raises(ValueError, match="columns 0 .. 4"):
        so.tsne_csr_check(desc, rowptr, torch.tensor([1, 0, 4, 2], dtype=torch.int32, device="cuda:0"), val)
    with pytest.raises(ValueError, match="must ascend"):
        so.tsne_csr_check(desc, torch.tensor([0, 2, 1, 3, 4], dtype=torch.int64, device="cuda:0"), col, val)
    with pytest.raises(ValueError, match="do not fit"):
        so.tsne_steps_launch(desc, None, rowptr, col, val, so.tsne_state(desc, 3, "cuda:0"), 2, 2, 250)
