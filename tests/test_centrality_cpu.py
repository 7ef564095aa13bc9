"""The centrality stage without a device: the scipy restatement (tests/hops_ref.py) against answers worked by hand and
against networkx, depth 1 against the boundary of the territories restatement, centrality_stats on integers written by hand and
against the restated statistics, the host layer's refusals, the round cap's host path and the sub-command's defaults."""
import argparse
import os

import numpy as np
import pytest

import centrality_cases as cases
import hops_ref as ref
import territories_ref
from spadot_amd import centrality as _stage_module  # noqa: F401  (the whole file is about this stage: no stage, no test)
from test_stage_frame_cpu import DEVICE, Inputs


# ------------------------------------------------------------------------------------- the restatement against hand-worked answers
def test_the_tiny_cases_by_hand():
    sums, ecc, hops = cases.want("n1")
    assert not sums.any() and not ecc.any() and hops.tolist() == [[0]]
    sums, ecc, hops = cases.want("n2")
    assert not sums[0].any() and ecc[0].tolist() == [0, 0]                                # both spots in domain 0: nothing to reach
    np.testing.assert_array_equal(sums[1], [[[0, 0, 0], [1, 1, 1]], [[1, 1, 1], [0, 0, 0]]])
    np.testing.assert_array_equal(sums[2], sums[1])                                       # the labels swapped: the same by symmetry
    assert ecc[1].tolist() == [1, 1] and hops.tolist() == [[0, -1], [0, -1]]
    sums, ecc, _ = cases.want("K1")
    assert not sums.any() and not ecc.any()
    sums, ecc, _ = cases.want("K32_unused")
    used = np.zeros(32, dtype=bool)
    used[[0, 5, 31]] = True
    assert not sums[:, ~used].any() and not sums[:, :, ~used].any() and not ecc[:, ~used].any()   # an empty set: all zeros
    assert np.all(sums[:, used][:, :, used][:, ~np.eye(3, dtype=bool), 0] > 0)
    sums, ecc, _ = cases.want("K32_all")
    assert np.all(ecc > 0) and np.all(sums[:, :, :, 0].sum(axis=2) > 0)


def test_the_paths_the_star_and_the_lattice_by_hand():
    for name in ("path_ascending", "path_descending", "path_shuffled"):
        sums, ecc, hops = cases.want(name)
        np.testing.assert_array_equal(sums[0, 0], [[0, 0, 0], [999, 499500, 1]], err_msg=name)   # 1 + 2 + .. + 999
        np.testing.assert_array_equal(sums[0, 1], [[1, 1, 1], [0, 0, 0]], err_msg=name)
        assert ecc[0].tolist() == [999, 1]
        np.testing.assert_array_equal(hops[:, 0], np.arange(1000))
    sums, ecc, hops = cases.want("star_hub_last")                                         # domain 0 = the hub, domain 1 = the 299 leaves
    np.testing.assert_array_equal(sums[0], [[[0, 0, 0], [299, 299, 299]], [[1, 1, 1], [0, 0, 0]]])
    assert ecc[0].tolist() == [1, 1]
    sums, ecc, hops = cases.want("lattice_stripes")                                       # stripes of 4 columns, 20 rows
    for a in range(5):
        for b in range(5):
            if a != b:                                                                    # the distance is the column difference
                gaps = [abs(col - (4 * a + (3 if b > a else 0))) for col in range(4 * b, 4 * b + 4)]
                assert sums[0, a, b].tolist() == [80, 20 * sum(gaps), 20 if abs(a - b) == 1 else 0], (a, b)
                assert sums[0, a, b, 1] / sums[0, a, b, 0] == 4 * abs(a - b) - 1.5
        assert ecc[0, a] == 4 * max(a, 4 - a)
    np.testing.assert_array_equal(hops[:, 0], np.maximum(np.arange(400) % 20 - 3, 0))


def test_two_components_and_isolated_spots_by_hand():
    sums, ecc, hops = cases.want("components")       # a path 0-1-2-3-4 (0 0 1 1 1), a triangle 5-6-7 (2 2 0), 8 (1) and 9 (2) alone
    np.testing.assert_array_equal(sums[0, 0], [[0, 0, 0], [3, 6, 1], [2, 2, 2]])          # {0, 1, 7}: 2, 3, 4 at 1, 2, 3; 5, 6 at 1
    np.testing.assert_array_equal(sums[0, 1], [[2, 3, 1], [0, 0, 0], [0, 0, 0]])          # {2, 3, 4, 8}: 1 at 1, 0 at 2
    np.testing.assert_array_equal(sums[0, 2], [[1, 1, 1], [0, 0, 0], [0, 0, 0]])          # {5, 6, 9}: 7 at 1
    assert ecc[0].tolist() == [3, 2, 1]
    assert hops[8].tolist() == [-1, 0, -1] and hops[9].tolist() == [-1, -1, 0] and hops[4].tolist() == [3, 0, -1]
    assert ref.depth(hops, cases.all_cases()["components"][2][0]).tolist() == [2, 1, 1, 2, 3, 1, 1, 1, -1, -1]
    st = ref.stats(sums[0], ecc[0], np.zeros((0, 3, 3, 3)), [3, 4, 3], 10)
    np.testing.assert_array_equal(st["closeness"], [7 / 8, 6 / 3, 7 / 1])                 # unreached spots count in the numerator only
    np.testing.assert_array_equal(st["degree"], [3 / 7, 1 / 6, 1 / 7])
    np.testing.assert_array_equal(st["reached_share"], [5 / 7, 2 / 6, 1 / 7])
    assert st["separation"][0, 1] == 2.0 and st["separation"][1, 0] == 1.5 and np.isnan(st["separation"][1, 2])
    assert np.all(np.isnan(np.diag(st["separation"])))
    src, dst, labs, K = cases.all_cases()["self_loop"]
    D = ref.dist_matrix(src, dst, 4)
    np.testing.assert_array_equal(D, ref.dist_matrix([0, 1, 2], [1, 2, 3], 4))            # the loops change nothing
    np.testing.assert_array_equal(D, np.abs(np.arange(4)[:, None] - np.arange(4)[None]))


def test_direction_and_duplicates_change_nothing():
    src, dst, labs, K = cases.all_cases()["dup_twoway"]
    once = np.unique(np.stack([np.minimum(src, dst), np.maximum(src, dst)]), axis=1)
    D = ref.dist_matrix(src, dst, 37)
    np.testing.assert_array_equal(D, ref.dist_matrix(once[0], once[1], 37))
    np.testing.assert_array_equal(D, ref.dist_matrix(dst, src, 37))
    np.testing.assert_array_equal(D, D.T)


# ------------------------------------------------------------------------------------- the restatement against networkx
def _nx_graph(src, dst, n):
    nx = pytest.importorskip("networkx")
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from((int(s), int(d)) for s, d in zip(src, dst) if s != d)
    return nx, g


def test_the_networkx_examples_of_the_issue():
    nx, g = _nx_graph([0, 1, 2, 3], [1, 2, 3, 4], 5)
    assert nx.group_closeness_centrality(g, [0]) == 0.4
    D = ref.dist_matrix([0, 1, 2, 3], [1, 2, 3, 4], 5)
    lab = [0, 1, 1, 1, 1]
    sums, ecc, _ = ref.integers(D, lab, 2)
    assert ref.stats(sums, ecc, [], [1, 4], 5)["closeness"][0] == 0.4
    nx, g = _nx_graph([0, 1, 2, 3], [1, 2, 3, 4], 6)                                      # an extra isolated spot
    assert nx.group_closeness_centrality(g, [0]) == 0.5
    sums, ecc, _ = ref.integers(ref.dist_matrix([0, 1, 2, 3], [1, 2, 3, 4], 6), lab + [1], 2)
    assert ref.stats(sums, ecc, [], [1, 5], 6)["closeness"][0] == 0.5


@pytest.mark.parametrize("name", cases.SMALL + ("stripes20",))
def test_the_restatement_equals_networkx(name):
    src, dst, labs, K = cases.all_cases()[name]
    n = labs.shape[1]
    nx, g = _nx_graph(src, dst, n)
    D = ref.dist_matrix(src, dst, n)
    lab = labs[0]
    sums, ecc, _ = ref.integers(D, lab, K)
    sizes = np.bincount(lab, minlength=K)
    st = ref.stats(sums, ecc, [], sizes, n)
    for a in range(K):
        members = np.flatnonzero(lab == a).tolist()
        if not members:
            continue
        if len(members) < n:                                                              # networkx divides by zero on V = S
            np.testing.assert_allclose(st["closeness"][a], nx.group_closeness_centrality(g, members), rtol=1e-15)
            np.testing.assert_allclose(st["degree"][a], nx.group_degree_centrality(g, members), rtol=1e-15)
        else:
            assert st["closeness"][a] == 0.0 and np.isnan(st["degree"][a])
    reached_by, sumdist_by, degree, secc = ref.spot_integers(D, lab, K)
    close, wf, diameter, radius, centre = ref.spot_stats(reached_by.sum(axis=1), sumdist_by.sum(axis=1), secc)
    plain, improved = nx.closeness_centrality(g, wf_improved=False), nx.closeness_centrality(g, wf_improved=True)
    np.testing.assert_allclose(close, [plain[i] for i in range(n)], rtol=1e-14)
    np.testing.assert_allclose(wf, [improved[i] for i in range(n)], rtol=1e-14)
    assert degree.tolist() == [g.degree(i) for i in range(n)]
    pieces = list(nx.connected_components(g))
    for piece in pieces:                                                                  # the eccentricity within the component
        e = nx.eccentricity(g.subgraph(piece))
        assert all(secc[i] == e[i] for i in piece)
    largest = max(pieces, key=len)
    if sum(len(p) == len(largest) for p in pieces) == 1:
        sub = g.subgraph(largest)
        assert (diameter, radius, centre) == (nx.diameter(sub), nx.radius(sub), sorted(nx.center(sub)))


def test_depth_one_is_the_boundary_of_territories():
    for name in cases.NAMES:
        if name.startswith("width_n40"):
            continue                                                                      # the python loop of the boundary is slow there
        src, dst, labs, K = cases.all_cases()[name]
        hops = cases.want(name)[2]
        np.testing.assert_array_equal(ref.depth(hops, labs[0]) == 1, territories_ref.boundary(src, dst, labs[0]), err_msg=name)


# ------------------------------------------------------------------------------------- centrality_stats
def _hand():
    """n = 20, four domains of 6, 8, 6, 0 spots, P = 4.  Domain 0 is less close than every relabeling, domain 1 the same in all
    (sd = 0, exactly: the values are dyadic), domain 3 empty."""
    obs = np.zeros((4, 4, 3), dtype=np.int64)
    obs[0, 1], obs[0, 2] = [8, 20, 3], [6, 36, 0]                   # closeness 14 / 56 = 0.25
    obs[1, 0], obs[1, 2] = [6, 12, 4], [6, 12, 2]                   # 12 / 24 = 0.5
    obs[2, 0], obs[2, 1] = [3, 8, 1], [8, 20, 2]                    # 14 / 28 = 0.5; three spots of domain 0 out of reach
    perm = np.zeros((4, 4, 4, 3), dtype=np.int64)
    for p, total in enumerate((16, 14, 28, 14)):                   # domain 0: 0.875, 1, 0.5, 1
        perm[p, 0, 1], perm[p, 0, 2] = [8, total - 6, 6], [6, 6, 6]
    perm[:, 1, 0], perm[:, 1, 2] = [6, 12, 4], [6, 12, 4]           # always 0.5
    for p, total in enumerate((28, 56, 14, 28)):                   # domain 2: 0.5, 0.25, 1, 0.5
        perm[p, 2, 0], perm[p, 2, 1] = [6, total - 8, 6], [8, 8, 8]
    return obs, np.array([5, 2, 3, 0]), perm, np.array([6, 8, 6, 0], dtype=np.int64), 20


def test_centrality_stats_by_hand():
    from spadot_amd.centrality import NULL_COLUMNS, PAIR_NULL, centrality_stats
    obs, ecc, perm, sizes, n = _hand()
    got = centrality_stats(obs, ecc, perm, sizes, n)
    np.testing.assert_array_equal(got["closeness"][:3], [0.25, 0.5, 0.5])
    np.testing.assert_array_equal(got["degree"][:3], [3 / 14, 6 / 12, 3 / 14])
    np.testing.assert_array_equal(got["reached_share"][:3], [1.0, 1.0, 11 / 14])
    assert got["eccentricity"].tolist() == [5, 2, 3, 0] and got["eccentricity"].dtype == np.int64
    for name in ("closeness", "degree", "reached_share", "p_lower", "p_higher", "padj", "closeness_z"):
        assert np.isnan(got[name][3]), name                                               # a domain without spots
    np.testing.assert_array_equal(got["separation"][0, :3], [np.nan, 2.5, 6.0])
    np.testing.assert_array_equal(got["separation"][2, :3], [8 / 3, 2.5, np.nan])
    assert np.all(np.isnan(got["separation"][3])) and np.all(np.isnan(got["separation"][:, 3]))
    np.testing.assert_array_equal(got["closeness_expected"][:3], [0.84375, 0.5, 0.5625])
    assert got["closeness_sd"][1] == 0.0 and np.isnan(got["closeness_z"][1])              # sd = 0
    np.testing.assert_allclose(got["closeness_z"][0], (0.25 - 0.84375) / np.std([0.875, 1, 0.5, 1]), rtol=1e-15)
    np.testing.assert_array_equal(got["p_lower"][:3], [0.2, 1.0, 0.8])
    np.testing.assert_array_equal(got["p_higher"][:3], [1.0, 1.0, 0.8])
    np.testing.assert_allclose(got["padj"][:3], [1.0, 1.0, 1.0], rtol=1e-15)              # raw 0.4, 1, 1 over three domains
    np.testing.assert_array_equal(got["separation_expected"][1, 0], 2.0)
    assert got["separation_sd"][1, 0] == 0.0 and np.isnan(got["separation_z"][1, 0])
    want = ref.stats(obs, ecc, perm, sizes, n)
    assert set(want) == set(got)
    for name, v in want.items():
        np.testing.assert_allclose(got[name], v, rtol=1e-12, atol=0, err_msg=name)
    none = centrality_stats(obs, ecc, perm[:0], sizes, n)                                 # P = 0: no null
    want = ref.stats(obs, ecc, perm[:0], sizes, n)
    for name in NULL_COLUMNS + PAIR_NULL:
        assert np.all(np.isnan(none[name])) and np.all(np.isnan(want[name])), name
    np.testing.assert_array_equal(none["closeness"], got["closeness"])
    whole = centrality_stats(np.zeros((1, 1, 3), np.int64), [0], np.zeros((2, 1, 1, 3), np.int64), [7], 7)   # size_a = n
    assert whole["closeness"][0] == 0.0 and np.isnan(whole["degree"][0]) and np.isnan(whole["reached_share"][0])


@pytest.mark.parametrize("name", ["stripes20", "components", "K32_unused"])
def test_centrality_stats_equal_the_restated_statistics(name):
    from spadot_amd.centrality import centrality_stats, spot_depth, spot_stats, SpotHops
    src, dst, labs, K = cases.all_cases()[name]
    n = labs.shape[1]
    D = ref.dist_matrix(src, dst, n)
    sums, ecc, hops = ref.integers(D, labs[0], K)
    perm, _ = ref.perm_integers(D, labs[0], K, 12, cases.SEED, 0)
    sizes = np.bincount(labs[0], minlength=K)
    got, want = centrality_stats(sums, ecc, perm, sizes, n), ref.stats(sums, ecc, perm, sizes, n)
    for key, v in want.items():
        np.testing.assert_allclose(got[key], v, rtol=1e-12, atol=0, err_msg=key)
    np.testing.assert_array_equal(spot_depth(hops, labs[0]), ref.depth(hops, labs[0]))
    rb, sb, deg, secc = ref.spot_integers(D, labs[0], K)
    st = spot_stats(SpotHops(rb, sb, deg, secc.astype(np.int32), None), labs[0], K)
    close, wf, diameter, radius, centre = ref.spot_stats(rb.sum(axis=1), sb.sum(axis=1), secc)
    np.testing.assert_allclose(st["spot_closeness"], close, rtol=1e-15)
    np.testing.assert_allclose(st["spot_closeness_wf"], wf, rtol=1e-15)
    assert (int(st["diameter"]), int(st["radius"]), st["centre"].tolist()) == (diameter, radius, centre)
    for a in range(K):
        if sizes[a]:
            np.testing.assert_allclose(st["domain_spot_closeness"][a], wf[labs[0] == a].mean(), rtol=1e-12)
        else:
            assert np.isnan(st["domain_spot_closeness"][a])


def test_the_null_is_one_or_two_hops_from_everything():
    """What the docstring says of the null, at the size of the suite: a real domain reads far less close than chance."""
    _, plant, lab, src, dst, K = cases.stripes(45)
    D = ref.dist_matrix(src, dst, 2025)
    sums, ecc, _ = ref.integers(D, lab, K)
    perm, pecc = ref.perm_integers(D, lab, K, 5, 0, 0)
    st = ref.stats(sums, ecc, perm, np.bincount(lab, minlength=K), 2025)
    sums_p, ecc_p, _ = ref.integers(D, plant, K)
    print("closeness", np.round(st["closeness"], 3), "expected", np.round(st["closeness_expected"], 3), "ecc under the null",
          pecc.max(), "planted separation 0 -> 6", sums_p[0, 6, 1] / sums_p[0, 6, 0])
    assert np.all(st["closeness_expected"] > 0.5)                                         # under two hops on average
    assert np.all(st["closeness"] < 0.5 * st["closeness_expected"]) and np.all(st["p_lower"] == 1 / 6)
    assert np.nanmax(st["separation_expected"]) < 2.0
    assert sums_p[0, 6, 1] / sums_p[0, 6, 0] > 10 * np.nanmax(st["separation_expected"])  # the separation is the finding


# ------------------------------------------------------------------------------------- the round cap's host path
def test_a_capped_status_raises_on_the_host():
    from spadot_amd.centrality import _run
    ok = np.array([[0, 3], [0, 1000]], dtype=np.int32)
    assert _run(None, None, status=ok)[3] is not None
    with pytest.raises(RuntimeError, match=r"spadot_hop_sums: item 1 of the call reached its round cap after 1001 rounds"):
        _run(None, None, status=np.array([[0, 3], [1, 1001], [1, 5]], dtype=np.int32))


# ------------------------------------------------------------------------------------- the driver's refusals
def _stage():
    from spadot_amd.centrality import centrality_stage
    return centrality_stage


CASES = [
    ("no domains", dict(domains=None), ValueError, "the centrality stage needs the domains table of analyze (--domains)", False),
    ("bad k", dict(k=0), ValueError, "the centrality stage takes k >= 1 and n_perms = 0 .. 9999 (got k = 0, n_perms = 200)", False),
    ("too many relabelings", dict(n_perms=10000), ValueError, "n_perms = 0 .. 9999 (got k = 6, n_perms = 10000)", False),
    ("negative relabelings", dict(n_perms=-1), ValueError, "n_perms = 0 .. 9999 (got k = 6, n_perms = -1)", False),
    ("33 domains", lambda i: dict(domains=i.table.assign(kmeans=np.r_[np.arange(12) % 3, [40] * 18])), ValueError,
     "at most 32 per time point", False),
    ("bad k and a bad device", dict(k=0, device="cpu"), ValueError, "the centrality stage takes k >= 1", False),
    ("well-formed", {}, AssertionError, DEVICE, True),
    ("well-formed, with spots and without a null", dict(spots=True, n_perms=0), AssertionError, DEVICE, True),
]


def _refused(tmp_path, change, exc, fragment, made):
    inp = Inputs(tmp_path)
    kw = dict(domains=inp.table, output_dir=inp.out, device="cuda:0")
    kw.update(change(inp) if callable(change) else change)
    with pytest.raises(exc) as e:
        _stage()(argparse.Namespace(**kw))
    assert type(e.value) is exc and fragment in str(e.value), str(e.value)
    assert os.path.isdir(inp.out) == made
    if made:
        assert not os.listdir(inp.out)                                                   # refused before anything is written


@pytest.mark.parametrize("case,change,exc,fragment,made", CASES, ids=[c[0] for c in CASES])
def test_the_driver_refuses_before_it_asks_for_the_device(tmp_path, monkeypatch, case, change, exc, fragment, made):
    import torch

    def no_device(*a, **k):
        raise AssertionError(DEVICE)
    monkeypatch.setattr(torch, "device", no_device)
    _refused(tmp_path, change, exc, fragment, made)


def test_the_driver_refuses_a_cpu_device(tmp_path):
    _refused(tmp_path, dict(device="cpu"), RuntimeError,
             "spadot_amd measures hop distances on the MI355X only (device 'cuda:N'); there is no CPU path", True)


def test_the_library_calls_refuse_without_a_device():
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.centrality import centrality, hop_sums, spot_hop_sums
    e = (torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32))
    lab = np.zeros(2, np.int64)
    for call in (lambda: hop_sums([e], [lab]), lambda: spot_hop_sums([e], [lab]), lambda: centrality([e], [lab])):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    with pytest.raises(ValueError, match="hop_sums takes one labeling block per graph"):
        hop_sums([e], [])
    with pytest.raises(ValueError, match="spot_hop_sums takes one labeling per graph"):
        spot_hop_sums([e, e], [lab])
    with pytest.raises(ValueError, match="centrality takes one labeling per graph"):
        centrality([], [])
    with pytest.raises(ValueError, match="n_clusters holds 2 cluster counts for 1 graphs"):
        hop_sums([e], [lab], n_clusters=[1, 1])
    with pytest.raises(ValueError, match="n_perms is a number of relabelings"):
        centrality([e], [lab], n_perms=-1)
    # the descriptor's own refusals come before the tensors are looked at
    s, d, l8 = e[0], e[1], torch.zeros(2, dtype=torch.uint8)
    row = [0, 2, 1, 1, 0, 1, -1, 0, 0, 0, 0, 0, -1, 0, 0]
    for change, what in (({12: -2}, "column 12"), ({14: 2}, "column 14"), ({14: 1, 5: 2}, "a source problem has one explicit"),
                         ({14: 1, 6: 0}, "a source problem has one explicit"), ({14: 1, 12: 0}, "a source problem has one explicit")):
        desc = np.array([[change.get(i, v) for i, v in enumerate(row)]], dtype=np.int64)
        with pytest.raises(ValueError, match=what):
            ops.hop_check(s, d, l8, desc, 32)
    with pytest.raises(ValueError, match="source problems with K_max = 32 only"):
        ops.hop_check(s, d, l8, np.array([[v if i != 14 else 1 for i, v in enumerate(row)]], dtype=np.int64), 7)
    with pytest.raises(ValueError, match="15 numbers per problem"):
        ops.hop_check(s, d, l8, np.zeros((1, 14), dtype=np.int64), 1)
    with pytest.raises(RuntimeError):                                                     # a well-formed descriptor: CPU tensors raise
        ops.hop_check(s, d, l8, np.array([row], dtype=np.int64), 1)


# ------------------------------------------------------------------------------------- the sub-command and the limits
def test_the_sub_command_and_its_defaults():
    from spadot_amd.cli import build_parser
    a = build_parser().parse_args(["centrality", "--domains", "d.csv"])
    assert a.cmd_choice == "centrality" and a.domains == "d.csv" and a.output_dir is None
    assert (a.k, a.n_perms, a.seed, a.spots, a.prefix, a.device) == (6, 200, 0, False, "", "cuda:0")
    a = build_parser().parse_args(["centrality", "--domains", "d.csv", "--spots", "--n_perms", "0", "--k", "8", "--seed", "3",
                                   "--prefix", "c_", "-o", "out", "--device", "cuda:1"])
    assert (a.k, a.n_perms, a.seed, a.spots, a.prefix, a.device, a.output_dir) == (8, 0, 3, True, "c_", "cuda:1", "out")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["centrality"])


def test_the_limits_the_library_states():
    from spadot_amd import stage_ops as ops
    assert ops.hop_lds_bytes(16354) == 163840 and ops.hop_lds_bytes(16355) > ops.HOP_LDS_BYTES
    assert ops.hop_lds_bytes(10000) <= ops.HOP_LDS_BYTES                                   # 10 000 spots with K = 32 run in LDS
    assert ops.hop_slab_ints(5) == 12 and ops.HOP_DESC == 15 and ops.HOP_FIXED == 16640
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spadot_model.h")).read()
    assert "16 354" in text and "desc [G, 15]" in text and "spadot_hop_sums" in text
    kernel = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spadot_amd", "csrc", "hops.hip")).read()
    assert "#define HP_FIXED 16640" in kernel and "#define HP_DESC 15" in kernel
