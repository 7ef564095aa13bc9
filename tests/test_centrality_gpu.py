"""The hops kernel on the MI355X against the scipy restatement of its definition (tests/hops_ref.py, held to hand-worked
answers and to networkx by tests/test_centrality_cpu.py): every case alone and in one batch, the per-spot distances, the
permuted labelings from the seed alone, the scratch path, the source items, depth against the boundary of territories,
repeatability, the stage and the refusals.

Everything the device computes is an integer, the round counts included (two mask arrays: a round reads only what the round
before left), so every comparison of integers is assert_array_equal.  The host statistics are fp64 arithmetic on the same
integers: within 1e-12 relative.  No test provokes the round cap on the device; its host path is tested on the CPU."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

import centrality_cases as cases
import hops_ref as ref
import nhood_ref
from spadot_amd import centrality as _stage_module  # noqa: F401  (the whole file is about this stage: no stage, no test)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


def _edges(src, dst):
    return _dev(src, torch.int32), _dev(dst, torch.int32)


def _check(name, got):
    """One HopSums against the restatement of case `name`."""
    sums, ecc, hops = cases.want(name)
    assert got.sums.dtype == np.int64 and got.sums.shape == sums.shape and got.ecc.dtype == np.int32
    np.testing.assert_array_equal(got.sums, sums, err_msg=name)
    np.testing.assert_array_equal(got.ecc, ecc, err_msg=name)
    np.testing.assert_array_equal(got.hops, hops, err_msg=name)
    np.testing.assert_array_equal(got.rounds, ecc.max(axis=1) + 1, err_msg=name)          # the largest distance and the closing round


def _call(names, **kw):
    from spadot_amd.centrality import hop_sums
    c = cases.all_cases()
    return hop_sums([_edges(c[n][0], c[n][1]) for n in names], [_dev(c[n][2]) for n in names],
                    n_clusters=[c[n][3] for n in names], hops=True, **kw)


@pytest.fixture(scope="module")
def batch():
    """Every case in one call."""
    return dict(zip(cases.NAMES, _call(cases.NAMES)))


@pytest.fixture(scope="module")
def perm_problems():
    from spadot_amd.neighbors import Permuted
    probs = cases.perm_problems()
    edges = [_edges(s, d) for s, d, *_ in probs]
    specs = [Permuted(_dev(p[2]), 200, seed=cases.SEED, graph=g) for g, p in enumerate(probs)]
    return probs, edges, specs


@pytest.fixture(scope="module")
def sources():
    """The source items of every source case in one call."""
    from spadot_amd.centrality import spot_hop_sums
    c = cases.source_cases()
    got = spot_hop_sums([_edges(c[n][0], c[n][1]) for n in cases.SOURCE_SIZES], [_dev(c[n][2]) for n in cases.SOURCE_SIZES],
                        n_clusters=[c[n][3] for n in cases.SOURCE_SIZES])
    return dict(zip(cases.SOURCE_SIZES, got))


@pytest.mark.parametrize("name", cases.NAMES)
def test_a_case_alone_matches_the_restatement_and_the_batch(name, batch):
    alone = _call([name])[0]
    _check(name, alone)
    _check(name, batch[name])


def test_the_shuffled_path_takes_one_round_per_hop(batch):
    for name in ("path_ascending", "path_descending", "path_shuffled"):
        got = batch[name]
        assert got.rounds.tolist() == [1000]                                              # 999 rounds and the closing one: cap 1001
        assert got.sums[0, 0, 1].tolist() == [999, 499500, 1] and got.ecc[0].tolist() == [999, 1]
        np.testing.assert_array_equal(got.hops[:, 0], np.arange(1000))
    assert batch["n1"].rounds.tolist() == [1] and batch["K1"].rounds.tolist() == [1]       # nothing to reach: the closing round alone


def test_permuted_labelings_match_explicit_ones_from_the_seed_alone(perm_problems):
    from spadot_amd.centrality import hop_sums
    from spadot_amd.neighbors import Permuted
    probs, edges, specs = perm_problems
    Ks = [p[3] for p in probs]
    got = hop_sums(edges, specs, n_clusters=Ks)
    for g, (s, d, lab, K, sums, ecc) in zip(got, probs):
        assert g.sums.shape == sums.shape and g.hops is None
        np.testing.assert_array_equal(g.sums, sums)
        np.testing.assert_array_equal(g.ecc, ecc)
        np.testing.assert_array_equal(g.rounds, ecc.max(axis=1) + 1)
    explicit = [np.stack([p[2][nhood_ref.perm(p[2].shape[0], cases.SEED, g, i)] for i in range(200)]) for g, p in enumerate(probs)]
    given = hop_sums(edges, [_dev(b) for b in explicit], n_clusters=Ks)
    for a, b in zip(given, got):
        np.testing.assert_array_equal(a.sums, b.sums)
        np.testing.assert_array_equal(a.ecc, b.ecc)
    tail = hop_sums(edges, [Permuted(s.base, 50, seed=cases.SEED, graph=s.graph, first=150) for s in specs], n_clusters=Ks)
    for t, g in zip(tail, got):
        np.testing.assert_array_equal(t.sums, g.sums[150:200])
        np.testing.assert_array_equal(t.ecc, g.ecc[150:200])
    other = hop_sums(edges[:1], [Permuted(specs[0].base, 2, seed=cases.SEED + 1, graph=0)], n_clusters=Ks[:1])[0]
    assert not np.array_equal(other.sums, got[0].sums[:2])                                # another seed: other relabelings


def test_the_scratch_path_gives_the_integers_of_the_lds_path(perm_problems, batch):
    from spadot_amd import stage_ops as ops
    from spadot_amd.centrality import hop_sums
    probs, edges, specs = perm_problems
    Ks = [p[3] for p in probs]
    # nothing at all; just below the need of n = 300 (n = 37 stays in LDS, n = 300 and n = 2025 leave it); just below n = 37
    for limit in (0, ops.hop_lds_bytes(300) - 1, ops.hop_lds_bytes(37) - 1):
        got = hop_sums(edges, specs, n_clusters=Ks, lds_limit=limit)
        for g, p in zip(got, probs):
            np.testing.assert_array_equal(g.sums, p[4])
            np.testing.assert_array_equal(g.ecc, p[5])
    assert ops.hop_lds_bytes(37) <= ops.hop_lds_bytes(300) - 1 < ops.hop_lds_bytes(2025)
    for limit in (0, ops.hop_lds_bytes(1024) - 1):                                        # LDS and scratch problems mixed in one call
        for name, got in zip(cases.NAMES, _call(cases.NAMES, lds_limit=limit)):
            _check(name, got)


@pytest.mark.parametrize("n", cases.SOURCE_SIZES)
def test_source_items_equal_the_all_pairs_sums(n, sources):
    from spadot_amd.centrality import spot_hop_sums
    src, dst, lab, K = cases.source_cases()[n]
    reached_by, sumdist_by, degree, ecc, D = cases.source_want(n)
    alone = spot_hop_sums([_edges(src, dst)], [_dev(lab)], n_clusters=[K])[0]
    for got in (alone, sources[n]):
        assert got.reached_by.shape == (n, K) and got.rounds.shape == ((n + 31) // 32,)
        np.testing.assert_array_equal(got.reached_by, reached_by)
        np.testing.assert_array_equal(got.sumdist_by, sumdist_by)
        np.testing.assert_array_equal(got.degree, degree)
        np.testing.assert_array_equal(got.ecc, ecc)
        np.testing.assert_array_equal(got.reached, reached_by.sum(axis=1))
        np.testing.assert_array_equal(got.rounds, [ecc[i:i + 32].max() + 1 for i in range(0, n, 32)])
        # summed over the graph the sums are symmetric: sum of d(u, v) over u of class a' and v of class a, both ways
        by = np.stack([got.sumdist_by[lab == a].sum(axis=0) for a in range(K)])
        np.testing.assert_array_equal(by, by.T)
        assert got.sumdist.sum() == int(np.where(D == ref.FAR, 0, D).astype(np.int64).sum())
    scratch = spot_hop_sums([_edges(src, dst)], [_dev(lab)], n_clusters=[K], lds_limit=0)[0]
    np.testing.assert_array_equal(scratch.sumdist_by, sumdist_by)
    np.testing.assert_array_equal(scratch.ecc, ecc)


def test_depth_one_is_the_boundary_of_territories(batch):
    from spadot_amd.centrality import spot_depth
    from spadot_amd.territories import boundary_spots
    for name in ("stripes20", "stripes45", "dup_twoway", "components", "K32_all", "width_n1025"):
        src, dst, labs, K = cases.all_cases()[name]
        depth = spot_depth(batch[name].hops, labs[0])
        np.testing.assert_array_equal(depth, ref.depth(cases.want(name)[2], labs[0]), err_msg=name)
        border = boundary_spots(*_edges(src, dst), _dev(labs[0])).cpu().numpy()
        np.testing.assert_array_equal(depth == 1, border, err_msg=name)


def test_two_runs_are_bitwise_equal_and_a_larger_k_pads_with_zeros(batch):
    from spadot_amd.centrality import hop_sums
    for name, got in zip(cases.NAMES, _call(cases.NAMES)):
        for field in ("sums", "ecc", "hops", "rounds"):
            assert getattr(got, field).tobytes() == getattr(batch[name], field).tobytes(), (name, field)
    c = cases.all_cases()["dup_twoway"]
    more = hop_sums([_edges(c[0], c[1])], [_dev(c[2])], n_clusters=[9], hops=True)[0]      # a larger K: the same numbers, zeros beyond
    np.testing.assert_array_equal(more.sums[:, :3, :3], batch["dup_twoway"].sums)
    np.testing.assert_array_equal(more.ecc[:, :3], batch["dup_twoway"].ecc)
    assert not more.sums[:, 3:].any() and not more.sums[:, :, 3:].any() and not more.ecc[:, 3:].any()
    np.testing.assert_array_equal(more.hops[:, :3], batch["dup_twoway"].hops)
    assert np.all(more.hops[:, 3:] == -1)


def test_centrality_and_its_statistics_on_the_stripe_maps():
    from spadot_amd.centrality import centrality
    s45, s20 = cases.stripes(45), cases.stripes(20)
    graphs = [(s45[3], s45[4], s45[2], s45[5]), (s20[3], s20[4], s20[2], s20[5])]
    res = centrality([_edges(s, d) for s, d, _, _ in graphs], [_dev(l) for _, _, l, _ in graphs], n_perms=40, seed=cases.SEED,
                     n_clusters=[k for *_, k in graphs], spots=True)
    for g, (r, (s, d, l, k)) in enumerate(zip(res, graphs)):
        n = l.shape[0]
        D = ref.dist_matrix(s, d, n)
        sums, ecc, hops = ref.integers(D, l, k)
        perm, _ = ref.perm_integers(D, l, k, 40, cases.SEED, g)
        np.testing.assert_array_equal(r.sums, sums)
        np.testing.assert_array_equal(r.ecc, ecc)
        np.testing.assert_array_equal(r.perm_sums, perm)
        np.testing.assert_array_equal(r.hops, hops)
        np.testing.assert_array_equal(r.depth, ref.depth(hops, l))
        np.testing.assert_array_equal(r.sizes, np.bincount(l, minlength=k))
        assert r.rounds == ecc.max() + 1 and r.n == n
        for name, v in ref.stats(sums, ecc, perm, r.sizes, n).items():
            np.testing.assert_allclose(getattr(r, name), v, rtol=1e-12, atol=0, err_msg=name)
        rb, sb, deg, secc = ref.spot_integers(D, l, k)
        close, wf, diameter, radius, centre = ref.spot_stats(rb.sum(axis=1), sb.sum(axis=1), secc)
        np.testing.assert_array_equal(r.spot_reached_by, rb)
        np.testing.assert_array_equal(r.spot_sumdist_by, sb)
        np.testing.assert_array_equal(r.spot_eccentricity, secc)
        np.testing.assert_allclose(r.spot_closeness, close, rtol=1e-15)
        np.testing.assert_allclose(r.spot_closeness_wf, wf, rtol=1e-15)
        assert (int(r.diameter), int(r.radius), r.centre.tolist()) == (diameter, radius, centre)
        print("graph", g, "closeness z", np.round(r.closeness_z, 1), "diameter", diameter, "radius", radius, "centre", centre)
        assert np.all(r.p_lower == 1 / 41)                                               # what the docstring says of the null
    none = centrality([_edges(*graphs[0][:2])], [_dev(graphs[0][2])], n_perms=0, n_clusters=[7])[0]
    np.testing.assert_array_equal(none.sums, res[0].sums)
    assert none.perm_sums.shape == (0, 7, 7, 3) and np.all(np.isnan(none.padj)) and none.spots is None


# ------------------------------------------------------------------------------------- the stage
@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from spadot_amd.centrality import centrality_stage
    out = tmp_path_factory.mktemp("centrality")
    df = cases.stage_table()
    path = os.path.join(out, "domains.csv")
    df.to_csv(path, index=False)
    res = centrality_stage(argparse.Namespace(domains=path, output_dir=str(out), prefix="s_", k=6, n_perms=30, seed=3, spots=True,
                                              device=DEV))
    return df, path, str(out), res


def test_the_stage_writes_its_files(stage):
    import pandas as pd
    from spadot_amd.centrality import (MATRICES, PAIR_COLUMNS, SPOT_COLUMNS, SPOT_EXTRA, SPOT_MATRICES, SPOT_TABLE_COLUMN,
                                       TABLE_COLUMNS)
    from spadot_amd.neighbors import spatial_edges
    from spadot_amd.utils._analyze_utils import have_matplotlib
    df, path, out, res = stage
    tps = ["E10", "E12"]
    assert res["timepoints"] == tps and set(res["timings"]) == {"read_s", "graph_s", "device_s", "write_s", "total_s"}
    masks = [np.asarray(df["timepoint"]) == tp for tp in tps]
    xy = np.stack([df["pixel_x"], df["pixel_y"]], axis=1)
    z = np.load(os.path.join(out, "s_centrality.npz"))
    assert z["timepoints"].tolist() == tps and (int(z["seed"]), int(z["k"]), int(z["n_perms"]), bool(z["spots"])) == (3, 6, 30, True)
    spots = pd.read_csv(os.path.join(out, "s_centrality_spots.csv"))
    K_all = int(df["kmeans"].max()) + 1
    assert tuple(spots.columns) == SPOT_COLUMNS + tuple(f"hops_to_{a}" for a in range(K_all)) + SPOT_EXTRA and len(spots) == len(df)
    np.testing.assert_array_equal(spots["row"], df["row"])                               # the input order
    np.testing.assert_array_equal(spots["kmeans"], df["kmeans"])
    for t, (tp, m) in enumerate(zip(tps, masks)):
        src, dst = (e.cpu().numpy() for e in spatial_edges(xy[m], 6, DEV))
        lab = np.asarray(df["kmeans"])[m]
        K, n = int(lab.max()) + 1, int(m.sum())
        D = ref.dist_matrix(src, dst, n)
        sums, ecc, hops = ref.integers(D, lab, K)
        perm, _ = ref.perm_integers(D, lab, K, 30, 3, t)
        sizes = np.bincount(lab, minlength=K)
        want = ref.stats(sums, ecc, perm, sizes, n)
        for name in MATRICES + SPOT_MATRICES:
            assert f"{tp}_{name}" in z.files, name
        np.testing.assert_array_equal(z[f"{tp}_sums"], sums)
        np.testing.assert_array_equal(z[f"{tp}_perm_sums"], perm)
        np.testing.assert_array_equal(z[f"{tp}_hops"], hops)
        np.testing.assert_allclose(z[f"{tp}_separation_z"], want["separation_z"], rtol=1e-12)
        tab = pd.read_csv(os.path.join(out, f"s_centrality_{tp}.csv"))
        assert tuple(tab.columns) == TABLE_COLUMNS + (SPOT_TABLE_COLUMN,) and len(tab) == K
        np.testing.assert_array_equal(tab["size"], sizes)
        np.testing.assert_array_equal(tab["eccentricity"], ecc)
        for col in ("closeness", "degree", "reached_share", "closeness_expected", "closeness_z", "p_lower", "p_higher", "padj"):
            np.testing.assert_allclose(tab[col], want[col], rtol=1e-12, err_msg=col)
        pairs = pd.read_csv(os.path.join(out, f"s_centrality_pairs_{tp}.csv"))
        assert tuple(pairs.columns) == PAIR_COLUMNS and len(pairs) == K * K
        np.testing.assert_array_equal(pairs["sumdist"], sums[:, :, 1].reshape(-1))
        for col in ("separation", "separation_expected", "separation_z"):
            np.testing.assert_allclose(pairs[col], want[col].reshape(-1), rtol=1e-12, err_msg=col)
        np.testing.assert_array_equal(np.asarray(spots["depth"])[m], ref.depth(hops, lab))
        for a in range(K):
            np.testing.assert_array_equal(np.asarray(spots[f"hops_to_{a}"])[m], hops[:, a])
        rb, sb, deg, secc = ref.spot_integers(D, lab, K)
        close, wf, diameter, radius, centre = ref.spot_stats(rb.sum(axis=1), sb.sum(axis=1), secc)
        np.testing.assert_array_equal(np.asarray(spots["reached"])[m], rb.sum(axis=1))
        np.testing.assert_array_equal(np.asarray(spots["eccentricity"])[m], secc)
        np.testing.assert_allclose(np.asarray(spots["closeness"])[m], close, rtol=1e-12)
        np.testing.assert_allclose(np.asarray(spots["closeness_wf"])[m], wf, rtol=1e-12)
        assert np.flatnonzero(np.asarray(spots["centre"])[m]).tolist() == centre
        assert (int(z[f"{tp}_diameter"]), int(z[f"{tp}_radius"]), z[f"{tp}_centre"].tolist()) == (diameter, radius, centre)
        np.testing.assert_allclose(tab[SPOT_TABLE_COLUMN], [wf[lab == a].mean() for a in range(K)], rtol=1e-12)
        assert os.path.exists(os.path.join(out, f"s_{tp}_centrality.png")) == have_matplotlib()


# ------------------------------------------------------------------------------------- the refusals
def _desc(n=37, E=64, K=3, L=3, p0=-1, gid=0, hops=-1, kind=0):
    return np.array([[0, n, E, K, 0, L, p0, gid, 0, 0, 0, 0, hops, 0, kind]], dtype=np.int64)


def test_refusals_come_before_any_launch(monkeypatch):
    from spadot_amd import stage_ops as ops
    from spadot_amd.centrality import hop_sums, spot_hop_sums
    src, dst, labs, K = cases.all_cases()["dup_twoway"]
    e, lab = _edges(src, dst), _dev(labs)
    E = src.shape[0]
    lib = ops.model_lib()
    calls = []
    real = lib.spadot_hop_sums
    monkeypatch.setattr(lib, "spadot_hop_sums", lambda *a: calls.append(a) or real(*a))
    with pytest.raises(ValueError, match="1 to 32"):
        hop_sums([e], [lab], n_clusters=[33])
    with pytest.raises(ValueError, match=r"labels must lie in 0 \.\. 1"):
        hop_sums([e], [lab], n_clusters=[2])                                             # a label >= K
    with pytest.raises(ValueError, match="labels must lie in"):
        spot_hop_sums([e], [lab[0] - 1], n_clusters=[3])
    with pytest.raises(ValueError, match="must be 1-d"):
        spot_hop_sums([e], [lab], n_clusters=[3])
    bad = dst.copy()
    bad[7] = 37
    with pytest.raises(ValueError, match=r"edge ends 0 \.\. 37: they must lie in 0 \.\. 36"):
        hop_sums([_edges(src, bad)], [lab], n_clusters=[3])                              # an edge end >= n
    with pytest.raises(ValueError, match=r"edge ends 0 \.\. 37"):
        spot_hop_sums([_edges(src, bad)], [lab[0]], n_clusters=[3])
    with pytest.raises(ValueError, match="no nodes"):
        hop_sums([e], [_dev(np.zeros((1, 0), np.int64))], n_clusters=[3])
    s32, d32, l8 = e[0], e[1], lab.to(torch.uint8).reshape(-1)
    for desc, what in ((_desc(E=E, n=2 ** 31), "spadot_hop_sums takes 1 to 2147483647"), (_desc(E=2 ** 31), "edges"),
                       (_desc(E=E, K=33), "label values"), (_desc(E=E, L=2 ** 31, p0=0), "more than 2147483647 labelings"),
                       (_desc(E=E, hops=-2), "column 12"), (_desc(E=E, kind=2), "column 14"),
                       (_desc(E=E, kind=1), "a source problem has one explicit"), (_desc(E=E, L=2, kind=1, hops=0), "a source problem")):
        with pytest.raises(ValueError, match=what):
            ops.hop_sums(s32, d32, l8, desc, 32)
    with pytest.raises(ValueError, match="K_max = 32 only"):
        ops.hop_sums(s32, d32, l8, _desc(E=E, L=2, kind=1), 3)
    assert not calls                                                                     # the library was not reached
    out = torch.full((3, 32, 32, 3), -77, dtype=torch.int64, device=DEV)                 # the library's own checks, from the host descriptor
    ecc = torch.full((3, 32), -77, dtype=torch.int32, device=DEV)
    status = torch.full((3, 2), -77, dtype=torch.int32, device=DEV)

    def direct(desc, K_max=32, limit=163840):
        return real(s32.data_ptr(), d32.data_ptr(), l8.data_ptr(), ctypes.c_void_p(desc.ctypes.data), _dev(desc).data_ptr(), 1, K_max,
                    limit, out.data_ptr(), ecc.data_ptr(), None, 0, status.data_ptr(), None, 0, None)
    for desc, rc_want in ((_desc(E=E, n=2 ** 31), -7), (_desc(E=2 ** 31), -7), (_desc(E=E, K=33), -7), (_desc(E=E, K=0), -7),
                          (_desc(E=E, L=2 ** 31, p0=0), -7), (_desc(E=E, hops=-2), -22), (_desc(E=E, hops=0), -22),
                          (_desc(E=E, kind=2), -22), (_desc(E=E, kind=1), -22), (_desc(E=E, L=2, kind=1, p0=0), -22),
                          (np.array([[0, 37, E, 3, 0, 3, -1, 0, 0, 0, 0, 37, -1, 0, 0]], dtype=np.int64), -7)):
        assert direct(desc) == rc_want, desc.tolist()
    good = np.array([[0, 37, E, 3, 0, 3, -1, 0, 0, 0, 0, 36, -1, 0, 0]], dtype=np.int64)
    assert direct(good, K_max=33) == -7
    assert direct(good, limit=0) == -22                                                  # the scratch path without scratch
    source = np.array([[0, 37, E, 3, 0, 2, -1, 0, 0, 0, 0, 36, -1, 0, 1]], dtype=np.int64)
    assert direct(source, K_max=3) == -7                                                 # source items need the 32-wide tables
    torch.cuda.synchronize()
    assert torch.all(out == -77) and torch.all(ecc == -77) and torch.all(status == -77)  # nothing was launched
    got = hop_sums([e], [lab], n_clusters=[3])[0]                                        # and a valid call goes through
    np.testing.assert_array_equal(got.sums, cases.want("dup_twoway")[0])
    assert len(calls) == 1
