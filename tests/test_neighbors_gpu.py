"""The neighbourhood-enrichment kernel on the MI355X against the numpy restatement of its definition (tests/nhood_ref.py, held to
its own conditions by tests/test_neighbors_cpu.py): the edge call, graphs that straddle the 256-thread workgroup, the permuted
labelings from the seed alone, the path that reads its labels from global memory, repeatability, the test's statistics, the
spatial graph, the refusals and the stage.

Everything the device computes is an integer, so every comparison of counts is assert_array_equal.  The host statistics are
fp64 arithmetic on the same integers: z, expected and sd within 1e-12 relative, the p-values exactly."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nhood_cases as cases
import nhood_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


def _edges(src, dst):
    return _dev(src, torch.int32), _dev(dst, torch.int32)


def _given_want(src, dst, labs, K):
    return np.stack([ref.count_matrix(src, dst, lab, K) for lab in labs])


@pytest.fixture(scope="module")
def perm_problems():
    """The PERM problems: the 45 x 45 planted grid (graph 0), n = 37 (graph 1) and n = 300 (graph 2), P = 200 under
    cases.SEED, with the restatement's stacks."""
    from spadot_amd.neighbors import Permuted
    _, lab45, s45, d45, K45 = cases.planted(45)
    call = cases.edge_call()
    graphs = [(s45, d45, lab45, K45), (call[2][0], call[2][1], call[2][2][0], 3), (call[3][0], call[3][1], call[3][2][0], 32)]
    want = [cases.planted_perm_counts(45)[:200]] + [ref.perm_counts(s, d, lab, K, 200, cases.SEED, g)
                                                    for g, (s, d, lab, K) in enumerate(graphs) if g > 0]
    edges = [_edges(s, d) for s, d, _, _ in graphs]
    specs = [Permuted(_dev(lab), 200, seed=cases.SEED, graph=g) for g, (_, _, lab, _) in enumerate(graphs)]
    return graphs, edges, specs, want


def test_edge_call_matches_the_restatement():
    from spadot_amd.neighbors import nhood_counts
    call = cases.edge_call()
    got = nhood_counts([_edges(s, d) for s, d, _, _ in call], [_dev(labs) for _, _, labs, _ in call],
                       n_clusters=[K for *_, K in call])
    assert [g.shape for g in got] == [(3, 1, 1), (3, 2, 2), (3, 3, 3), (3, 32, 32)]
    for g, (src, dst, labs, K) in zip(got, call):
        assert g.dtype == np.int32
        np.testing.assert_array_equal(g, _given_want(src, dst, labs, K))
        assert np.all(g.sum(axis=(1, 2)) == src.shape[0])
    assert not got[0].any()                                                          # n = 1: no edges
    np.testing.assert_array_equal(got[1], [[[0, 1], [1, 0]], [[0, 1], [1, 0]], [[2, 0], [0, 0]]])
    assert not got[2][1][2].any() and not got[2][1][:, 2].any()                      # the label value without spots
    assert got[3][2][31, 31] == 1800 and got[3][2].sum() == 1800                     # one domain holds every spot
    src, dst = call[2][0], call[2][1]                                                # the duplicate edge counts twice
    lab = call[2][2][0]
    once = ref.count_matrix(src[:-1], dst[:-1], lab, 3)
    assert got[2][0][lab[src[-1]], lab[dst[-1]]] == once[lab[src[-1]], lab[dst[-1]]] + 1


@pytest.mark.parametrize("name", [c[0] for c in cases.TILE_CASES])
def test_tile_edges_match_the_restatement(name):
    from spadot_amd.neighbors import Permuted, nhood_counts
    src, dst, lab, K = cases.tile_case(name)
    got = nhood_counts([_edges(src, dst)] * 2, [_dev(lab), Permuted(_dev(lab), 3, seed=5, graph=2)], n_clusters=[K, K])
    np.testing.assert_array_equal(got[0], ref.count_matrix(src, dst, lab, K)[None])
    np.testing.assert_array_equal(got[1], ref.perm_counts(src, dst, lab, K, 3, 5, 2))
    if src.shape[0] == 0:
        assert not got[0].any() and not got[1].any()


def test_permuted_labelings_match_the_restatement_from_the_seed_alone(perm_problems):
    from spadot_amd.neighbors import Permuted, nhood_counts
    graphs, edges, specs, want = perm_problems
    got = nhood_counts(edges, specs, n_clusters=[K for *_, K in graphs])
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_array_equal(g, w)
    tail = nhood_counts(edges, [Permuted(s.base, 50, seed=cases.SEED, graph=s.graph, first=150) for s in specs],
                        n_clusters=[K for *_, K in graphs])
    for t, g in zip(tail, got):
        np.testing.assert_array_equal(t, g[150:200])
    other = nhood_counts(edges[:1], [Permuted(specs[0].base, 2, seed=cases.SEED + 1, graph=0)], n_clusters=[graphs[0][3]])[0]
    assert not np.array_equal(other, got[0][:2])                                     # another seed: other permutations


def test_labels_read_from_global_memory_give_the_same_integers(perm_problems):
    from spadot_amd.neighbors import nhood_counts
    graphs, edges, specs, want = perm_problems
    Ks = [K for *_, K in graphs]
    for limit in (36, 16 * 32 * 32 + 299, 0):            # below n = 37 at K = 3; just below n = 300 beside 16 K^2; nothing at all
        got = nhood_counts(edges, specs, n_clusters=Ks, lds_limit=limit)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
    call = cases.edge_call()
    given = nhood_counts([_edges(s, d) for s, d, _, _ in call], [_dev(labs) for _, _, labs, _ in call],
                         n_clusters=[K for *_, K in call], lds_limit=16)
    for g, (src, dst, labs, K) in zip(given, call):
        np.testing.assert_array_equal(g, _given_want(src, dst, labs, K))


def test_a_problem_alone_in_a_batch_and_run_twice_gives_the_same_integers(perm_problems):
    from spadot_amd.neighbors import nhood_counts
    graphs, edges, specs, want = perm_problems
    call = cases.edge_call()
    alone = nhood_counts(edges[1:2], specs[1:2], n_clusters=[3])[0]
    np.testing.assert_array_equal(alone, want[1])
    batch = nhood_counts([_edges(call[3][0], call[3][1]), edges[0], edges[1], _edges(call[1][0], call[1][1])],
                         [_dev(call[3][2]), specs[0], specs[1], _dev(call[1][2])], n_clusters=[32, graphs[0][3], 3, 2])
    np.testing.assert_array_equal(batch[2], alone)
    np.testing.assert_array_equal(batch[1], want[0])
    again = nhood_counts(edges[1:2], specs[1:2], n_clusters=[3])[0]
    np.testing.assert_array_equal(again, alone)
    wide = nhood_counts(edges[1:2], specs[1:2], n_clusters=[9])[0]                   # a larger K: the same corner, zeros around
    np.testing.assert_array_equal(wide[:, :3, :3], alone)
    assert wide[:, 3:, :].sum() == 0 and wide[:, :, 3:].sum() == 0


def test_nhood_enrichment_on_the_planted_grid():
    from spadot_amd.neighbors import nhood_enrichment
    _, lab, src, dst, K = cases.planted(45)
    r = nhood_enrichment([_edges(src, dst)], [_dev(lab)], n_perms=1000, seed=cases.SEED)[0]
    counts, perms = ref.count_matrix(src, dst, lab, K), cases.planted_perm_counts(45)
    np.testing.assert_array_equal(r.counts, counts)
    np.testing.assert_array_equal(r.perm_counts, perms)
    np.testing.assert_array_equal(r.sizes, np.bincount(lab, minlength=K))
    want = ref.stats(counts, perms, r.sizes)
    for name in ("zscore", "expected", "sd", "share", "coherence"):
        np.testing.assert_allclose(getattr(r, name), want[name], rtol=1e-12, atol=0, err_msg=name)
    for name in ("p_enriched", "p_depleted"):
        np.testing.assert_array_equal(getattr(r, name), want[name])
    np.testing.assert_allclose(r.padj, want["padj"], rtol=1e-12, atol=0)
    print("diagonal z", np.round(np.diagonal(r.zscore), 1), "coherence", np.round(r.coherence, 3))
    assert np.all(np.diagonal(r.zscore) > 0)                                         # planted compact domains
    assert np.all(r.p_enriched[np.diag_indices(K)] == 1 / 1001)


def test_spatial_edges_against_sklearn():
    from sklearn.neighbors import NearestNeighbors
    from spadot_amd.neighbors import spatial_edges
    xy = cases.planted(20)[0]
    n, k = xy.shape[0], 6
    dist, idx = NearestNeighbors(n_neighbors=k + 2).fit(xy).kneighbors(xy)
    assert np.all(idx[:, 0] == np.arange(n))
    gaps = np.diff(dist[:, 1:], axis=1) / dist[:, 2:]                 # on the reference: no two candidate distances of a spot tie
    assert gaps.min() > 1e-9, gaps.min()
    src, dst = spatial_edges(xy, k, DEV)
    assert src.dtype == torch.int32 and dst.dtype == torch.int32 and src.is_cuda
    np.testing.assert_array_equal(src.cpu().numpy(), np.repeat(np.arange(n), k))
    np.testing.assert_array_equal(dst.cpu().numpy().reshape(n, k), idx[:, 1:k + 1])
    src, dst = spatial_edges(xy[:1], k, DEV)                                         # one spot: no edges
    assert src.numel() == 0 and dst.numel() == 0 and src.dtype == torch.int32
    src, dst = spatial_edges(xy[:k], k, DEV)                                         # n = k: n - 1 neighbours per spot
    np.testing.assert_array_equal(src.cpu().numpy(), np.repeat(np.arange(k), k - 1))
    want = NearestNeighbors(n_neighbors=k).fit(xy[:k]).kneighbors(xy[:k])[1][:, 1:]
    np.testing.assert_array_equal(dst.cpu().numpy().reshape(k, k - 1), want)


SENTINEL = -77


def _desc(n=37, E=148, K=3, L=3, p0=-1, gid=0):
    return np.array([[0, n, E, K, 0, L, p0, gid, 0, 0, 0, 0]], dtype=np.int64)


def test_refusals_come_before_any_launch():
    from spadot_amd import stage_ops as ops
    from spadot_amd.neighbors import Permuted, nhood_counts
    src, dst, labs, K = cases.edge_call()[2]
    e, lab = _edges(src, dst), _dev(labs)
    out = torch.full((3, 3, 3), SENTINEL, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="1 to 32"):
        nhood_counts([e], [lab], n_clusters=[33], out=out)
    with pytest.raises(ValueError, match="1 to 32"):
        nhood_counts([e], [lab], n_clusters=[0], out=out)
    with pytest.raises(ValueError, match=r"labels must lie in 0 \.\. 1"):
        nhood_counts([e], [lab], n_clusters=[2], out=out)                            # a label >= K
    with pytest.raises(ValueError, match="labels must lie in"):
        nhood_counts([e], [lab - 1], n_clusters=[3], out=out)                        # a negative label
    bad = dst.copy()
    bad[7] = 37
    with pytest.raises(ValueError, match=r"edge ends 0 \.\. 37: they must lie in 0 \.\. 36"):
        nhood_counts([_edges(src, bad)], [lab], n_clusters=[3], out=out)
    bad[7] = -1
    with pytest.raises(ValueError, match="edge ends -1"):
        nhood_counts([_edges(src, bad)], [lab], n_clusters=[3], out=out)
    with pytest.raises(ValueError, match="must form an"):
        nhood_counts([e], [lab[None]], n_clusters=[3], out=out)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nhood_counts([(torch.as_tensor(src), torch.as_tensor(dst))], [lab], n_clusters=[3], out=out)
    s32, d32, l8 = e[0], e[1], lab.to(torch.uint8).reshape(-1)
    for desc, what in ((_desc(n=2 ** 31), "nodes"), (_desc(E=2 ** 31), "edges"), (_desc(K=33), "label values"),
                       (_desc(L=2 ** 31, p0=0), "more than 2147483647 labelings"), (_desc(p0=2 ** 32 - 1, L=3), "below")):
        with pytest.raises(ValueError, match=what):
            ops.nhood_counts(s32, d32, l8, desc, 32 if what != "label values" else 33, out=out)
    with pytest.raises(ValueError, match="1 to 32"):
        ops.nhood_counts(s32, d32, l8, _desc(K=33), 33, out=out)
    with pytest.raises(ValueError):
        Permuted(lab[0], 0)
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)                                                # nothing was launched
    lib = ops.model_lib()                                                            # the library's own checks, from the host descriptor
    import ctypes
    for desc in (_desc(n=2 ** 31), _desc(E=2 ** 31), _desc(K=33), _desc(K=0), _desc(L=2 ** 31, p0=0),
                 np.array([[0, 37, 149, 3, 0, 3, -1, 0, 0, 0, 0, 37]], dtype=np.int64),
                 np.array([[0, 37, 149, 3, 0, 3, -1, 0, 0, 0, -1, 36]], dtype=np.int64)):
        ddev = _dev(desc)
        rc = lib.spadot_nhood_counts(s32.data_ptr(), d32.data_ptr(), l8.data_ptr(), ctypes.c_void_p(desc.ctypes.data),
                                     ddev.data_ptr(), 1, 32, 163840, out.data_ptr(), None)
        assert rc == -7, (rc, desc.tolist())
    assert lib.spadot_nhood_counts(s32.data_ptr(), d32.data_ptr(), l8.data_ptr(), ctypes.c_void_p(_desc().ctypes.data),
                                   _dev(_desc()).data_ptr(), 1, 33, 163840, out.data_ptr(), None) == -7
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)
    got = nhood_counts([e], [lab], n_clusters=[3], out=out)[0]                       # and the same tensor is written by a valid call
    np.testing.assert_array_equal(got, _given_want(src, dst, labs, 3))
    np.testing.assert_array_equal(out.cpu().numpy(), got)


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from spadot_amd.neighbors import neighbors
    out = tmp_path_factory.mktemp("neighbors")
    df = cases.stage_table()
    path = os.path.join(out, "domains.csv")
    df.to_csv(path, index=False)
    res = neighbors(argparse.Namespace(domains=path, output_dir=str(out), prefix="s_", k=6, n_perms=200, seed=3, device=DEV))
    return df, path, str(out), res


def test_the_stage_writes_its_files(stage):
    import pandas as pd
    from spadot_amd.neighbors import MATRICES, SPOT_COLUMNS, TABLE_COLUMNS, nhood_enrichment, spatial_edges
    df, path, out, res = stage
    tps = ["E10", "E12", "E14"]
    assert res["timepoints"] == tps and set(res["timings"]) == {"read_s", "graph_s", "device_s", "write_s", "total_s"}
    masks = [np.asarray(df["timepoint"]) == tp for tp in tps]
    xy = np.stack([df["pixel_x"], df["pixel_y"]], axis=1)
    edges = [spatial_edges(xy[m], 6, DEV) for m in masks]
    labs = [np.asarray(df["kmeans"])[m] for m in masks]
    want = nhood_enrichment(edges, [_dev(l) for l in labs], n_perms=200, seed=3, n_clusters=[int(l.max()) + 1 for l in labs])
    z = np.load(os.path.join(out, "s_nhood.npz"))
    assert z["timepoints"].tolist() == tps and int(z["seed"]) == 3 and int(z["k"]) == 6 and int(z["n_perms"]) == 200
    same = np.empty(len(df))
    for tp, m, (src, dst), lab, w in zip(tps, masks, edges, labs, want):
        for name in MATRICES:
            np.testing.assert_array_equal(z[f"{tp}_{name}"], getattr(w, name), err_msg=f"{tp}_{name}")
        s, d = src.cpu().numpy(), dst.cpu().numpy()
        np.testing.assert_array_equal(w.counts, ref.count_matrix(s, d, lab, w.counts.shape[0]))
        np.testing.assert_array_equal(w.perm_counts, ref.perm_counts(s, d, lab, w.counts.shape[0], 200, 3, tps.index(tp)))
        same[m] = ref.same_share(s, d, lab, lab.shape[0])
        tab = pd.read_csv(os.path.join(out, f"s_nhood_{tp}.csv"))
        K = w.counts.shape[0]
        assert tuple(tab.columns) == TABLE_COLUMNS and len(tab) == K * K
        np.testing.assert_array_equal(tab["count"], w.counts.reshape(-1))
        np.testing.assert_array_equal(tab["domain"] * K + tab["neighbor"], np.arange(K * K))
        np.testing.assert_allclose(tab["zscore"], w.zscore.reshape(-1), rtol=1e-12)
        if os.path.exists(os.path.join(out, f"s_{tp}_nhood.png")):
            assert os.path.getsize(os.path.join(out, f"s_{tp}_nhood.png")) > 0
    spots = pd.read_csv(os.path.join(out, "s_nhood_spots.csv"), float_precision="round_trip")
    assert tuple(spots.columns) == SPOT_COLUMNS and len(spots) == len(df)
    np.testing.assert_array_equal(spots["row"], df["row"])
    np.testing.assert_array_equal(spots["kmeans"], df["kmeans"])
    np.testing.assert_array_equal(np.asarray(spots["same"]), same)
    from spadot_amd.utils._analyze_utils import have_matplotlib
    assert all(os.path.exists(os.path.join(out, f"s_{tp}_nhood.png")) for tp in tps) == have_matplotlib()


def test_a_second_run_and_the_sub_command_write_the_same_bytes(stage, tmp_path):
    from spadot_amd.neighbors import neighbors
    df, path, out, res = stage
    names = ["s_nhood_spots.csv"] + [f"s_nhood_{tp}.csv" for tp in res["timepoints"]]
    neighbors(argparse.Namespace(domains=path, output_dir=str(tmp_path), prefix="s_", k=6, n_perms=200, seed=3, device=DEV))
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(tmp_path, name), "rb").read(), name
    sub = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "spadot_amd", "neighbors", "--domains", path, "-o", str(sub), "--prefix", "s_",
                        "--n_perms", "200", "--seed", "3", "--device", DEV], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(sub, name), "rb").read(), name
    other = neighbors(argparse.Namespace(domains=path, output_dir=str(tmp_path / "seed4"), prefix="", k=6, n_perms=200, seed=4,
                                         device=DEV))
    assert not np.array_equal(other["results"]["E12"].perm_counts, res["results"]["E12"].perm_counts)
    np.testing.assert_array_equal(other["results"]["E12"].counts, res["results"]["E12"].counts)
