"""The analyze stage on the MI355X: the k-means++ seeding kernel against the torch rounds of tests/kmeans_ref.py, the Lloyd
launch with mixed cluster counts against the same launch with one K, kmeans.fit_sweep against KMeansDevice.fit and sklearn,
analyze(args) end to end and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kmeans_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blobs(rng, n, k, d=20, spread=3.0, noise=0.5):
    cen = spread * rng.normal(size=(k, d))
    return cen[rng.integers(0, k, n)] + noise * rng.normal(size=(n, d))


def _centred_sets(sizes, seed=4):
    rng = np.random.default_rng(seed)
    Xs = [torch.as_tensor(_blobs(rng, n, 10), device=DEV) for n in sizes]
    Xc = [x - x.mean(0) for x in Xs]
    return Xs, Xc


def _seed_all(Xc, ks, R=10):
    from spadot_amd.kmeans import sweep_draws
    from spadot_amd.ops import kmeanspp_seed
    ns = [x.shape[0] for x in Xc]
    pset, pK, pfirst, puoff, Us = [], [], [], [], []
    off = 0
    for t, n in enumerate(ns):
        for k in ks:
            first, U = sweep_draws(n, k, 1993, R)
            for r in range(R):
                pset.append(t); pK.append(k); pfirst.append(int(first[r])); puoff.append(off); Us.append(U[r])
                off += U.shape[1]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    xoff = i32(np.concatenate([[0], np.cumsum(ns)[:-1]]).tolist())
    args = (torch.cat(Xc).contiguous(), xoff, i32(ns), max(ns), i32(pset), i32(pK), i32(pfirst), i32(puoff),
            torch.as_tensor(np.concatenate(Us), device=DEV), max(ks))
    return args, kmeanspp_seed(*args)


def test_seeding_kernel_matches_the_torch_path():
    sizes, ks, R = (257, 700, 1500, 2300), list(range(4, 21)), 10
    _, Xc = _centred_sets(sizes)
    args, (idx, C) = _seed_all(Xc, ks, R)
    idx2, C2 = __import__("spadot_amd.ops", fromlist=["x"]).kmeanspp_seed(*args)
    assert torch.equal(idx, idx2) and torch.equal(C, C2)            # bitwise reproducible
    seeds = np.random.RandomState(1993).randint(np.iinfo(np.int32).max, size=R)
    p = 0
    for t, x in enumerate(Xc):
        xsq = (x * x).sum(1)
        for k in ks:
            want = kmeans_ref.init_centers(x, xsq, seeds, k)                       # [R, k, d]
            got_i = idx[p:p + R]
            assert bool((got_i[:, k:] == -1).all()) and bool((C[p:p + R, k:] == 0).all())
            assert torch.equal(x[got_i[:, :k].long()], want), (sizes[t], k)       # the same rows were chosen
            assert torch.equal(C[p:p + R, :k], want)                              # centres bit for bit
            p += R


def test_lloyd_sweep_matches_the_uniform_launch():
    from spadot_amd.ops import lloyd_steps
    sizes, R, d = (257, 700, 1500, 2300), 10, 20
    _, Xc = _centred_sets(sizes, seed=7)
    ks = [6, 10]
    (Xall, xoff, npts, n_max, pset, pK, *_), (idx, C) = _seed_all(Xc, ks, R)
    T = len(sizes)
    tol = torch.full((T,), 1e-6, dtype=torch.float64, device=DEV)
    Cv = C.view(T, len(ks), R, max(ks), d)
    rg = torch.arange(T, device=DEV, dtype=torch.int32).repeat_interleave(R)
    for skip, steps in ((False, 12), (True, 9)):
        # mixed K (6 and 10 in one launch, padded to 10): each restart as the launch with K_max = its own K (no padding)
        Cs = C.clone()
        done = torch.zeros(C.shape[0], dtype=torch.int32, device=DEV)
        inert = torch.zeros(C.shape[0], dtype=torch.float64, device=DEV)
        part = torch.empty(C.shape[0] * ((n_max + 255) // 256) * (10 * (d + 1) + 1), dtype=torch.float64, device=DEV)
        lloyd_steps(Xall, Cs, xoff, npts, n_max, pset, pK, tol, done, inert, part, steps, skip_done=skip)
        Csv = Cs.view(T, len(ks), R, 10, d)
        for j, K in enumerate(ks):
            Cg = Cv[:, j, :, :K].reshape(T * R, K, d).contiguous()
            dg = torch.zeros(T * R, dtype=torch.int32, device=DEV)
            ig = torch.zeros(T * R, dtype=torch.float64, device=DEV)
            pg = torch.empty(T * R * ((n_max + 255) // 256) * (K * (d + 1) + 1), dtype=torch.float64, device=DEV)
            Kr = torch.full((T * R,), K, dtype=torch.int32, device=DEV)
            lloyd_steps(Xall, Cg, xoff, npts, n_max, rg, Kr, tol, dg, ig, pg, steps, skip_done=skip)
            assert torch.equal(Csv[:, j, :, :K].reshape(T * R, K, d), Cg), (skip, K)
            assert torch.equal(inert.view(T, len(ks), R)[:, j].reshape(-1), ig), (skip, K)
            assert torch.equal(done.view(T, len(ks), R)[:, j].reshape(-1), dg), (skip, K)
            assert bool((Csv[:, j, :, K:] == 0).all())                            # padding untouched


def test_fit_sweep_matches_kmeansdevice_for_every_set_and_k():
    from spadot_amd.kmeans import KMeansDevice, fit_sweep
    Xs, _ = _centred_sets((257, 700, 1500), seed=11)
    ks = [list(range(4, 21)), list(range(4, 21)), [3, 10, 17]]
    res = fit_sweep(Xs, ks, labels_for=True)
    again = fit_sweep(Xs, ks, labels_for=True)
    for t, X in enumerate(Xs):
        assert sorted(res[t]) == sorted(ks[t])
        Xh = X.cpu().numpy()
        for k in ks[t]:
            km, km2 = res[t][k], again[t][k]
            one = KMeansDevice(k, random_state=1993, n_init=10).fit(X)
            assert km.cluster_centers_.shape == (k, 20) and km.labels_.dtype == np.int32
            assert km.inertia_ == one.inertia_, (t, k)
            np.testing.assert_array_equal(km.labels_, one.labels_)
            np.testing.assert_array_equal(km.cluster_centers_, one.cluster_centers_)
            dd = ((Xh[:, None, :] - km.cluster_centers_[None]) ** 2).sum(-1)
            np.testing.assert_array_equal(km.labels_, dd.argmin(1).astype(np.int32))
            np.testing.assert_array_equal(km.labels_, km2.labels_)
            np.testing.assert_array_equal(km.cluster_centers_, km2.cluster_centers_)
            assert km.inertia_ == km2.inertia_ and km.n_iter_ >= 1
    only = fit_sweep(Xs[:1], [[5, 6]], labels_for=[(0, 6)])
    assert only[0][5].labels_ is None and only[0][6].labels_ is not None


def test_fit_sweep_elbow_agrees_with_sklearn():
    from sklearn.cluster import KMeans
    from sklearn.metrics import adjusted_rand_score
    from spadot_amd.kmeans import fit_sweep
    from spadot_amd.utils._analyze_utils import select_k
    rng = np.random.default_rng(3)
    true_k = (5, 7, 9)
    Xh = [_blobs(rng, n, k, spread=8.0, noise=0.5) for n, k in zip((900, 1200, 1500), true_k)]
    ks = list(range(4, 21))
    res = fit_sweep([torch.as_tensor(x, device=DEV) for x in Xh], [ks] * 3)
    for t, (x, k_true) in enumerate(zip(Xh, true_k)):
        sk = [KMeans(n_clusters=k, random_state=1993, n_init=10).fit(x) for k in ks]
        k_dev = select_k([res[t][k].inertia_ for k in ks])
        assert k_dev == k_true
        assert select_k([m.inertia_ for m in sk]) == k_true
        assert res[t][k_true].inertia_ == pytest.approx(sk[k_true - 4].inertia_, rel=1e-6)
        lab = fit_sweep([torch.as_tensor(x, device=DEV)], [[k_true]], labels_for=True)[0][k_true].labels_
        assert adjusted_rand_score(sk[k_true - 4].labels_, lab) > 0.999


def _write_latent(path, counts=(600, 500, 700), true_k=(5, 6, 7), seed=5):
    rng = np.random.default_rng(seed)
    X = np.concatenate([_blobs(rng, n, k, spread=6.0) for n, k in zip(counts, true_k)]).astype(np.float32)
    tp = np.repeat(np.array(["E1", "E2", "E3"]), counts)
    rows = rng.permutation(X.shape[0]) + 1000
    np.savez_compressed(path, X=X, rows=rows, timepoint=tp, spatial=rng.uniform(0, 100, size=(X.shape[0], 2)))
    return X, tp, rows


class _Args:
    def __init__(self, **kw):
        self.__dict__.update(dict(output_dir=None, prefix="", n_clusters=None, device=DEV, write_tmaps=False), **kw)


@pytest.mark.parametrize("mode", ["fixed", "adaptive"])
def test_analyze_end_to_end(tmp_path, mode):
    import pandas as pd
    from spadot_amd import analyze, analyze_ot
    from spadot_amd.kmeans import fit_sweep
    from spadot_amd.utils._analyze_utils import have_matplotlib
    f = tmp_path / "latent.npz"
    X, tp, rows = _write_latent(f)
    a = _Args(data=str(f), n_clusters=[5, 6, 7] if mode == "fixed" else None)
    out = analyze(a)
    pre = "" if mode == "fixed" else "adaptive_"
    assert a.prefix == pre and a.output_dir == str(tmp_path)
    tps = ["E1", "E2", "E3"]
    assert out["timepoints"] == tps and out["n_clusters"] == [5, 6, 7]
    files = set(os.listdir(tmp_path))
    want = {pre + "domains.csv", "OT_g.txt"} | {f"{pre}transition_table_{d}_{d + 1}.{e}" for d in (0, 1) for e in ("csv", "npz")}
    if mode == "adaptive":
        want |= {f"{pre}{t}_WSS.csv" for t in tps}
    if have_matplotlib():
        want |= {f"{pre}{t}_domains.png" for t in tps} | {f"{pre}transition_dotplot_{d}_{d + 1}.png" for d in (0, 1)}
        if mode == "adaptive":
            want |= {f"{pre}{t}_WSS_vs_Clusters.png" for t in tps}
    assert want <= files, want - files
    dom = pd.read_csv(tmp_path / (pre + "domains.csv"))
    assert list(dom.columns) == ["row", "timepoint", "kmeans", "pixel_x", "pixel_y"]
    np.testing.assert_array_equal(dom["row"].to_numpy(), rows)
    np.testing.assert_array_equal(dom["timepoint"].astype(str).to_numpy(), tp)
    Xs = [torch.as_tensor(X[tp == t], device=DEV) for t in tps]
    res = fit_sweep(Xs, [[k] for k in (5, 6, 7)], labels_for=True)
    labels = []
    for i, (t, k) in enumerate(zip(tps, (5, 6, 7))):
        np.testing.assert_array_equal(dom["kmeans"].to_numpy()[tp == t], res[i][k].labels_)
        np.testing.assert_array_equal(out["labels"][t], res[i][k].labels_)
        labels.append(res[i][k].labels_)
    if mode == "adaptive":
        w = pd.read_csv(tmp_path / f"{pre}E2_WSS.csv")
        assert list(w.columns) == ["clusters", "wss", "wss_diff", "wss_diff_ratio", "selected"]
        assert w["clusters"][w["selected"]].tolist() == [6]
    tabs = analyze_ot.transition_tables([X[tp == t] for t in tps], labels, device=DEV)
    for d, (tab, _) in enumerate(tabs):
        z = np.load(tmp_path / f"{pre}transition_table_{d}_{d + 1}.npz")
        np.testing.assert_allclose(z["X"], tab, rtol=1e-12, atol=0)
        np.testing.assert_allclose(out["tables"][d], tab, rtol=1e-12, atol=0)
        assert z["obs_names"].tolist() == [f"{tps[d]}_{c}" for c in range(tab.shape[0])]


def test_command_line_analyze(tmp_path):
    f = tmp_path / "latent.npz"
    _write_latent(f)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "spadot_amd", "analyze", "-i", str(f), "--n_clusters", "5,6,7", "-o",
                        str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    files = set(os.listdir(tmp_path / "out"))
    assert {"domains.csv", "transition_table_0_1.csv", "transition_table_1_2.npz"} <= files
