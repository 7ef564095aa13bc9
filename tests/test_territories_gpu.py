"""The territories kernel on the MI355X against the scipy restatement of its definition (tests/territories_ref.py, held to
hand-worked answers by tests/test_territories_cpu.py): every case alone and in one batch, the per-spot ids and sizes, the
permuted labelings from the seed alone, the scratch path, repeatability, the refinement, the stage and the refusals.

Everything the device computes is an integer, so every comparison of integers and ids is assert_array_equal.  The host
statistics are fp64 arithmetic on the same integers: within 1e-12 relative, the p-values exactly.  The round counts are never
compared: they may depend on the order in which atomics retire; only the results do not."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

import nhood_ref
import territories_cases as cases
import territories_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


def _edges(src, dst):
    return _dev(src, torch.int32), _dev(dst, torch.int32)


def _check(name, got):
    """One TerritoryCounts against the restatement of case `name`."""
    ints, ids, sizes = cases.want(name)
    n = cases.all_cases()[name][2].shape[1]
    assert got.counts.dtype == np.int64 and got.counts.shape == ints.shape
    np.testing.assert_array_equal(got.counts, ints, err_msg=name)
    np.testing.assert_array_equal(got.ids, ids, err_msg=name)
    np.testing.assert_array_equal(got.sizes, sizes, err_msg=name)
    assert got.rounds.shape == (ints.shape[0],) and np.all(got.rounds >= 1) and np.all(got.rounds <= n + 1), (name, got.rounds)


def _call(names, **kw):
    from spadot_amd.territories import territory_counts
    c = cases.all_cases()
    return territory_counts([_edges(c[n][0], c[n][1]) for n in names], [_dev(c[n][2]) for n in names],
                            n_clusters=[c[n][3] for n in names], ids=True, **kw)


@pytest.fixture(scope="module")
def batch():
    """Every case in one call."""
    return dict(zip(cases.NAMES, _call(cases.NAMES)))


@pytest.fixture(scope="module")
def perm_problems():
    from spadot_amd.neighbors import Permuted
    probs = cases.perm_problems()
    edges = [_edges(s, d) for s, d, *_ in probs]
    specs = [Permuted(_dev(lab), 200, seed=cases.SEED, graph=g) for g, (_, _, lab, _, _) in enumerate(probs)]
    return probs, edges, specs


@pytest.mark.parametrize("name", cases.NAMES)
def test_a_case_alone_matches_the_restatement_and_the_batch(name, batch):
    alone = _call([name])[0]
    _check(name, alone)
    _check(name, batch[name])
    np.testing.assert_array_equal(alone.counts, batch[name].counts)
    np.testing.assert_array_equal(alone.ids, batch[name].ids)
    np.testing.assert_array_equal(alone.sizes, batch[name].sizes)


def test_the_rounds_are_reported_and_no_hook_means_one_round(batch):
    r = {n: int(batch[n].rounds[0]) for n in ("path_ascending", "path_descending", "path_shuffled")}
    print("rounds", r, {n: batch[n].rounds.tolist() for n in ("star_hub_last", "grid64_one_label", "checkerboard", "n1")})
    assert batch["n1"].rounds.tolist() == [1] and batch["checkerboard"].rounds.tolist() == [1]     # no same-label edge: no hook


def test_permuted_labelings_match_explicit_ones_from_the_seed_alone(perm_problems):
    from spadot_amd.neighbors import Permuted
    from spadot_amd.territories import territory_counts
    probs, edges, specs = perm_problems
    Ks = [K for *_, K, _ in probs]
    got = territory_counts(edges, specs, n_clusters=Ks)
    for g, (s, d, lab, K, want) in zip(got, probs):
        assert g.counts.shape == want.shape and g.ids is None
        np.testing.assert_array_equal(g.counts, want)
        assert np.all(g.rounds <= lab.shape[0] + 1)
    explicit = [np.stack([lab[nhood_ref.perm(lab.shape[0], cases.SEED, g, p)] for p in range(200)])
                for g, (_, _, lab, _, _) in enumerate(probs)]
    given = territory_counts(edges, [_dev(b) for b in explicit], n_clusters=Ks)
    for a, b in zip(given, got):
        np.testing.assert_array_equal(a.counts, b.counts)
    tail = territory_counts(edges, [Permuted(s.base, 50, seed=cases.SEED, graph=s.graph, first=150) for s in specs], n_clusters=Ks)
    for t, g in zip(tail, got):
        np.testing.assert_array_equal(t.counts, g.counts[150:200])
    other = territory_counts(edges[:1], [Permuted(specs[0].base, 2, seed=cases.SEED + 1, graph=0)], n_clusters=Ks[:1])[0]
    assert not np.array_equal(other.counts, got[0].counts[:2])                           # another seed: other relabelings


def test_the_scratch_path_gives_the_bits_of_the_lds_path(perm_problems, batch):
    from spadot_amd import stage_ops as ops
    from spadot_amd.territories import territory_counts
    probs, edges, specs = perm_problems
    Ks = [K for *_, K, _ in probs]
    # nothing at all; just below the need of n = 300 (n = 37 stays in LDS, n = 300 and n = 2025 leave it); just below n = 37
    for limit in (0, ops.territory_lds_bytes(300) - 1, ops.territory_lds_bytes(37) - 1):
        got = territory_counts(edges, specs, n_clusters=Ks, lds_limit=limit)
        for g, (*_, want) in zip(got, probs):
            np.testing.assert_array_equal(g.counts, want)
    assert ops.territory_lds_bytes(37) <= ops.territory_lds_bytes(300) - 1 < ops.territory_lds_bytes(2025)
    for limit in (0, ops.territory_lds_bytes(1024) - 1):
        for name, got in zip(cases.NAMES, _call(cases.NAMES, lds_limit=limit)):
            _check(name, got)
            np.testing.assert_array_equal(got.counts, batch[name].counts)
            np.testing.assert_array_equal(got.ids, batch[name].ids)


def test_two_runs_are_identical(batch):
    for name, got in zip(cases.NAMES, _call(cases.NAMES)):
        np.testing.assert_array_equal(got.counts, batch[name].counts)
        np.testing.assert_array_equal(got.ids, batch[name].ids)
        np.testing.assert_array_equal(got.sizes, batch[name].sizes)
    wide = _call(["dup_twoway"])[0]
    from spadot_amd.territories import territory_counts
    c = cases.all_cases()["dup_twoway"]
    more = territory_counts([_edges(c[0], c[1])], [_dev(c[2])], n_clusters=[9])[0]       # a larger K: the same rows, zeros below
    np.testing.assert_array_equal(more.counts[:, :3], wide.counts)
    assert not more.counts[:, 3:].any()


def test_the_test_and_its_statistics_on_the_stripe_map():
    from spadot_amd.territories import territories
    _, plant, lab, src, dst, K = cases.stripes(45)
    s20 = cases.stripes(20)
    res = territories([_edges(src, dst), _edges(s20[3], s20[4])], [_dev(lab), _dev(s20[2])], n_perms=200, seed=cases.SEED,
                      n_clusters=[K, s20[5]])
    for g, (r, (s, d, l, k)) in enumerate(zip(res, [(src, dst, lab, K), (s20[3], s20[4], s20[2], s20[5])])):
        obs = ref.integers(s, d, l, k)
        perm = cases.perm_problems()[0][4] if g == 0 else ref.perm_integers(s, d, l, k, 200, cases.SEED, g)
        ids, sizes = ref.components(s, d, l)
        np.testing.assert_array_equal(r.counts, obs)
        np.testing.assert_array_equal(r.perm_counts, perm)
        np.testing.assert_array_equal(r.sizes, np.bincount(l, minlength=k))
        np.testing.assert_array_equal(r.territory, ids)
        np.testing.assert_array_equal(r.territory_size, sizes)
        np.testing.assert_array_equal(r.boundary, ref.boundary(s, d, l))
        want = ref.stats(obs, perm, r.sizes, 0.05)
        for name in ("largest_share", "contiguity", "count_expected", "count_sd", "count_z", "contiguity_expected",
                     "contiguity_sd", "contiguity_z", "padj"):
            np.testing.assert_allclose(getattr(r, name), want[name], rtol=1e-12, atol=0, err_msg=name)
        for name in ("p_fewer", "p_more"):
            np.testing.assert_array_equal(getattr(r, name), want[name])
        assert r.verdict.tolist() == want["verdict"].tolist()
        print("graph", g, "count z", np.round(r.count_z, 1), "contiguity z", np.round(r.contiguity_z, 1), r.verdict.tolist())
        assert r.verdict.tolist() == ["contiguous"] * k and np.all(r.p_fewer == 1 / 201)   # what the docstring says of the null
    none = territories([_edges(src, dst)], [_dev(lab)], n_perms=0, n_clusters=[K])[0]
    np.testing.assert_array_equal(none.counts, res[0].counts)
    assert none.perm_counts.shape == (0, K, 4) and none.verdict.tolist() == [""] * K and np.all(np.isnan(none.padj))


def test_refinement_equals_the_restatement():
    from spadot_amd.territories import refine_labels
    for side, s in ((20, 4), (45, 5), (45, 2)):
        _, plant, lab, src, dst, K = cases.stripes(side)
        want, rounds, moved, _ = ref.refine(src, dst, lab, K, s)
        got = refine_labels(_edges(src, dst), _dev(lab), s, n_clusters=K)
        assert got[0].dtype == np.int64 and (got[1], got[2]) == (rounds, moved), (side, s, got[1:], rounds, moved)
        np.testing.assert_array_equal(got[0], want)
        again = refine_labels(_edges(src, dst), got[0], s, n_clusters=K)                 # a refined map stays
        assert again[1:] == (0, 0) and np.array_equal(again[0], got[0])
    path = _edges([0, 1, 2], [1, 2, 3])
    got = refine_labels(path, np.array([0, 0, 1, 1]), 3)
    assert got[0].tolist() == [0, 0, 1, 1] and got[1:] == (0, 0)                         # A A B B, s = 3
    got = refine_labels(_edges([0, 1, 3, 4, 2, 2], [1, 5, 4, 6, 5, 6]), np.array([0, 0, 2, 1, 1, 0, 1]), 3)
    assert got[0].tolist() == [0, 0, 0, 1, 1, 0, 1] and got[1:] == (1, 1)                # a tie goes to the smallest label
    got = refine_labels(_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 5]), np.array([2, 1, 0, 0, 0, 0]), 2)
    assert got[0].tolist() == [0] * 6 and got[1:] == (2, 2)                              # a small piece among small ones waits
    got = refine_labels(_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 5]), np.array([2, 1, 0, 0, 0, 0]), 2, max_rounds=1)
    assert got[0].tolist() == [2, 0, 0, 0, 0, 0] and got[1:] == (1, 1)


# ------------------------------------------------------------------------------------- the stage
@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from spadot_amd.territories import territories_stage
    out = tmp_path_factory.mktemp("territories")
    df = cases.stage_table()
    path = os.path.join(out, "domains.csv")
    df.to_csv(path, index=False)
    res = territories_stage(argparse.Namespace(domains=path, output_dir=str(out), prefix="s_", k=6, n_perms=50, seed=3, min_size=4,
                                               alpha=0.05, device=DEV))
    return df, path, str(out), res


def test_the_stage_writes_its_files(stage):
    import pandas as pd
    from spadot_amd.neighbors import spatial_edges
    from spadot_amd.territories import DOMAIN_COLUMNS, MATRICES, SPOT_COLUMNS, TABLE_COLUMNS
    from spadot_amd.utils._analyze_utils import have_matplotlib
    df, path, out, res = stage
    tps = ["E10", "E12"]
    assert res["timepoints"] == tps and set(res["timings"]) == {"read_s", "graph_s", "device_s", "write_s", "total_s"}
    masks = [np.asarray(df["timepoint"]) == tp for tp in tps]
    xy = np.stack([df["pixel_x"], df["pixel_y"]], axis=1)
    z = np.load(os.path.join(out, "s_territories.npz"))
    assert z["timepoints"].tolist() == tps and (int(z["seed"]), int(z["k"]), int(z["n_perms"]), int(z["min_size"])) == (3, 6, 50, 4)
    assert float(z["alpha"]) == 0.05
    spots = pd.read_csv(os.path.join(out, "s_territories_spots.csv"))
    assert tuple(spots.columns) == SPOT_COLUMNS + ("refined",) and len(spots) == len(df)
    np.testing.assert_array_equal(spots["row"], df["row"])
    np.testing.assert_array_equal(spots["kmeans"], df["kmeans"])
    refined = pd.read_csv(os.path.join(out, "s_refined_domains.csv"), float_precision="round_trip")
    assert tuple(refined.columns) == DOMAIN_COLUMNS == tuple(df.columns)
    for col in ("row", "timepoint", "pixel_x", "pixel_y"):                               # the coordinates as the stage read them
        np.testing.assert_array_equal(refined[col], pd.read_csv(path)[col])
    np.testing.assert_array_equal(refined["kmeans"], spots["refined"])
    for t, (tp, m) in enumerate(zip(tps, masks)):
        src, dst = (e.cpu().numpy() for e in spatial_edges(xy[m], 6, DEV))
        lab = np.asarray(df["kmeans"])[m]
        K = int(lab.max()) + 1
        obs, perm = ref.integers(src, dst, lab, K), ref.perm_integers(src, dst, lab, K, 50, 3, t)
        ids, sizes = ref.components(src, dst, lab)
        want = ref.stats(obs, perm, np.bincount(lab, minlength=K), 0.05)
        for name in MATRICES:
            assert f"{tp}_{name}" in z.files, name
        np.testing.assert_array_equal(z[f"{tp}_counts"], obs)
        np.testing.assert_array_equal(z[f"{tp}_perm_counts"], perm)
        np.testing.assert_allclose(z[f"{tp}_contiguity_z"], want["contiguity_z"], rtol=1e-12)
        tab = pd.read_csv(os.path.join(out, f"s_territories_{tp}.csv"))
        assert tuple(tab.columns) == TABLE_COLUMNS and len(tab) == K
        for c, col in enumerate(("count", "largest", "singletons")):
            np.testing.assert_array_equal(tab[col], obs[:, c])
        np.testing.assert_array_equal(tab["size"], np.bincount(lab, minlength=K))
        np.testing.assert_allclose(tab["contiguity"], want["contiguity"], rtol=1e-12)
        np.testing.assert_allclose(tab["count_z"], want["count_z"], rtol=1e-12)
        assert tab["verdict"].tolist() == want["verdict"].tolist()
        np.testing.assert_array_equal(np.asarray(spots["territory"])[m], ids)
        np.testing.assert_array_equal(np.asarray(spots["territory_size"])[m], sizes)
        np.testing.assert_array_equal(np.asarray(spots["boundary"])[m], ref.boundary(src, dst, lab))
        new, rounds, moved, _ = ref.refine(src, dst, lab, K, 4)
        np.testing.assert_array_equal(np.asarray(spots["refined"])[m], new)
        np.testing.assert_array_equal(z[f"{tp}_refined"], new)
        assert (int(z["refine_rounds"][t]), int(z["refine_moved"][t])) == (rounds, moved)
        assert os.path.exists(os.path.join(out, f"s_{tp}_territories.png")) == have_matplotlib()


def test_the_refined_table_feeds_the_other_stages(stage, tmp_path):
    from spadot_amd.neighbors import neighbors, spatial_edges
    from spadot_amd.territories import territories_stage
    from spadot_amd.utils._stage_utils import read_domains_table
    df, path, out, res = stage
    refined = os.path.join(out, "s_refined_domains.csv")
    tab = read_domains_table(argparse.Namespace(domains=refined), "territories")
    np.testing.assert_array_equal(tab.labels, res["refined"])
    nb = neighbors(argparse.Namespace(domains=refined, output_dir=str(tmp_path / "nb"), prefix="", k=6, n_perms=20, seed=0, device=DEV))
    assert nb["timepoints"] == ["E10", "E12"]
    again = territories_stage(argparse.Namespace(domains=refined, output_dir=str(tmp_path / "again"), prefix="", k=6, n_perms=0,
                                                 seed=0, min_size=0, alpha=0.05, device=DEV))
    assert not os.path.exists(tmp_path / "again" / "refined_domains.csv")
    for tp, m in zip(tab.tps, tab.masks):
        src, dst = (e.cpu().numpy() for e in spatial_edges(tab.coords[m], 6, DEV))
        want = ref.integers(src, dst, tab.labels[m], int(tab.labels[m].max()) + 1)
        np.testing.assert_array_equal(again["results"][tp].counts, want)
        assert again["results"][tp].counts[:, 0].sum() < res["results"][tp].counts[:, 0].sum()
        assert again["results"][tp].verdict.tolist() == [""] * want.shape[0]


# ------------------------------------------------------------------------------------- the refusals
def _desc(n=37, E=64, K=3, L=3, p0=-1, gid=0, ids=-1):
    return np.array([[0, n, E, K, 0, L, p0, gid, 0, 0, 0, 0, ids, 0]], dtype=np.int64)


def test_refusals_come_before_any_launch(monkeypatch):
    from spadot_amd import stage_ops as ops
    from spadot_amd.territories import territory_counts
    src, dst, labs, K = cases.all_cases()["dup_twoway"]
    e, lab = _edges(src, dst), _dev(labs)
    E = src.shape[0]
    lib = ops.model_lib()
    calls = []
    real = lib.spadot_territory_counts
    monkeypatch.setattr(lib, "spadot_territory_counts", lambda *a: calls.append(a) or real(*a))
    with pytest.raises(ValueError, match="1 to 32"):
        territory_counts([e], [lab], n_clusters=[33])
    with pytest.raises(ValueError, match=r"labels must lie in 0 \.\. 1"):
        territory_counts([e], [lab], n_clusters=[2])                                     # a label >= K
    with pytest.raises(ValueError, match="labels must lie in"):
        territory_counts([e], [lab - 1], n_clusters=[3])
    bad = dst.copy()
    bad[7] = 37
    with pytest.raises(ValueError, match=r"edge ends 0 \.\. 37: they must lie in 0 \.\. 36"):
        territory_counts([_edges(src, bad)], [lab], n_clusters=[3])                      # an edge end >= n
    with pytest.raises(ValueError, match="no nodes"):
        territory_counts([e], [_dev(np.zeros((1, 0), np.int64))], n_clusters=[3])
    s32, d32, l8 = e[0], e[1], lab.to(torch.uint8).reshape(-1)
    for desc, what in ((_desc(E=E, n=2 ** 31), "nodes"), (_desc(E=2 ** 31), "edges"), (_desc(E=E, K=33), "label values"),
                       (_desc(E=E, L=2 ** 31, p0=0), "more than 2147483647 labelings"), (_desc(E=E, ids=-2), "column 12")):
        with pytest.raises(ValueError, match=what):
            ops.territory_counts(s32, d32, l8, desc, 32)
    assert not calls                                                                     # the library was not reached
    out = torch.full((3, 32, 4), -77, dtype=torch.int64, device=DEV)                     # the library's own checks, from the host descriptor
    status = torch.full((3, 2), -77, dtype=torch.int32, device=DEV)
    for desc, rc_want in ((_desc(E=E, n=2 ** 31), -7), (_desc(E=2 ** 31), -7), (_desc(E=E, K=33), -7), (_desc(E=E, K=0), -7),
                          (_desc(E=E, L=2 ** 31, p0=0), -7), (_desc(E=E, ids=-2), -22), (_desc(E=E, ids=0), -22),
                          (np.array([[0, 37, E, 3, 0, 3, -1, 0, 0, 0, 0, 37, -1, 0]], dtype=np.int64), -7)):
        rc = real(s32.data_ptr(), d32.data_ptr(), l8.data_ptr(), ctypes.c_void_p(desc.ctypes.data), _dev(desc).data_ptr(), 1, 32,
                  163840, out.data_ptr(), None, None, 0, status.data_ptr(), None, 0, None)
        assert rc == rc_want, (rc, desc.tolist())
    good = np.array([[0, 37, E, 3, 0, 3, -1, 0, 0, 0, 0, 36, -1, 0]], dtype=np.int64)
    assert real(s32.data_ptr(), d32.data_ptr(), l8.data_ptr(), ctypes.c_void_p(good.ctypes.data), _dev(good).data_ptr(), 1, 33,
                163840, out.data_ptr(), None, None, 0, status.data_ptr(), None, 0, None) == -7
    assert real(s32.data_ptr(), d32.data_ptr(), l8.data_ptr(), ctypes.c_void_p(good.ctypes.data), _dev(good).data_ptr(), 1, 32,
                0, out.data_ptr(), None, None, 0, status.data_ptr(), None, 0, None) == -22     # the scratch path without scratch
    torch.cuda.synchronize()
    assert torch.all(out == -77) and torch.all(status == -77)                            # nothing was launched
    got = territory_counts([e], [lab], n_clusters=[3])[0]                                # and a valid call goes through
    np.testing.assert_array_equal(got.counts, cases.want("dup_twoway")[0])
    assert len(calls) == 1
