"""The territories stage without a device: the scipy restatement (tests/territories_ref.py) against answers worked by hand,
the planted properties on the restatement alone, territory_stats on integers written by hand, the driver's refusals in the
manner of test_stage_frame_cpu.py, and the sub-command's defaults."""
import argparse
import os

import numpy as np
import pytest

import territories_cases as cases
import territories_ref as ref
from test_stage_frame_cpu import DEVICE, Inputs


# ------------------------------------------------------------------------------------- the restatement against hand-worked answers
def test_the_tiny_cases_by_hand():
    c = cases.all_cases()
    np.testing.assert_array_equal(cases.want("n1")[0], [[[1, 1, 1, 1]]])
    ints, ids, sizes = cases.want("n2")
    np.testing.assert_array_equal(ints[0], [[1, 2, 0, 4], [0, 0, 0, 0]])                # both ends in domain 0: one piece of two
    np.testing.assert_array_equal(ints[1], [[1, 1, 1, 1], [1, 1, 1, 1]])                # unequal labels: the edge joins nothing
    np.testing.assert_array_equal(ints[2], [[0, 0, 0, 0], [1, 2, 0, 4]])
    assert ids.tolist() == [0, 0] and sizes.tolist() == [2, 2]
    for name in ("path_ascending", "path_descending", "path_shuffled", "grid64_one_label"):
        n = c[name][2].shape[1]
        ints, ids, sizes = cases.want(name)
        np.testing.assert_array_equal(ints, [[[1, n, 0, n * n]]], err_msg=name)          # one territory: sumsq = n^2
        assert not ids.any() and np.all(sizes == n)
    ints, ids, sizes = cases.want("star_hub_last")
    np.testing.assert_array_equal(ints, [[[1, 300, 0, 90000]]])
    assert not ids.any()                                                                 # the id is the smallest spot, not the hub
    ints, ids, sizes = cases.want("checkerboard")
    np.testing.assert_array_equal(ints, [[[200, 1, 200, 200], [200, 1, 200, 200]]])      # every territory is a singleton
    np.testing.assert_array_equal(ids, np.arange(400))
    ints = cases.want("K32_unused")[0]
    used = np.zeros(32, dtype=bool)
    used[[0, 5, 31]] = True
    assert not ints[:, ~used].any() and np.all(ints[:, used, 0] > 0)                     # a label value without spots: 0, 0, 0, 0


def test_direction_duplicates_and_self_loops_change_nothing():
    src, dst, labs, K = cases.all_cases()["dup_twoway"]
    once = np.unique(np.stack([np.minimum(src, dst), np.maximum(src, dst)]), axis=1)
    for lab, w in zip(labs, cases.want("dup_twoway")[0]):
        np.testing.assert_array_equal(ref.integers(once[0], once[1], lab, K), w)
        np.testing.assert_array_equal(ref.integers(dst, src, lab, K), w)
        np.testing.assert_array_equal(ref.integers(np.r_[src, 3], np.r_[dst, 3], lab, K), w)
    # a path 0 - 1 - 2 - 3 labelled A A B A by hand: {0, 1}, {2}, {3}
    ids, sizes = ref.components([0, 1, 2], [1, 2, 3], [0, 0, 1, 0])
    assert ids.tolist() == [0, 0, 2, 3] and sizes.tolist() == [2, 2, 1, 1]
    np.testing.assert_array_equal(ref.integers([0, 1, 2], [1, 2, 3], [0, 0, 1, 0], 2), [[2, 2, 1, 5], [1, 1, 1, 1]])
    assert ref.boundary([0, 1, 2], [1, 2, 3], [0, 0, 1, 0]).tolist() == [False, True, True, True]


def test_the_integers_are_consistent_on_every_case():
    for name in cases.NAMES:
        src, dst, labs, K = cases.all_cases()[name]
        ints, ids, sizes = cases.want(name)
        for lab, w in zip(labs, ints):
            size = np.bincount(lab, minlength=K)
            assert np.all(w[:, 1] <= size) and np.all(w[:, 0] <= size) and np.all(w[:, 2] <= w[:, 0])
            assert np.all(w[:, 3] <= size * size) and np.all(w[:, 3] >= size)
            assert np.all((w[:, 0] == 0) == (size == 0))
        assert np.all(ids <= np.arange(ids.shape[0])) and np.all(ids[ids] == ids) and np.all(labs[0][ids] == labs[0])
        np.testing.assert_array_equal(np.bincount(ids, minlength=ids.shape[0])[ids], sizes)


# ------------------------------------------------------------------------------------- the planted properties
@pytest.mark.parametrize("side,s", [(20, 4), (45, 5)])
def test_refinement_recovers_the_planted_stripes(side, s):
    _, plant, lab, src, dst, K = cases.stripes(side)
    before = ref.integers(src, dst, lab, K)
    assert before[:, 0].sum() > K and before[:, 2].sum() > 0                             # more territories than domains
    np.testing.assert_array_equal(ref.integers(src, dst, plant, K)[:, :3], np.stack([np.ones(K), np.bincount(plant), np.zeros(K)], 1))
    one, _ = ref.refine_round(src, dst, lab, K, s)
    np.testing.assert_array_equal(ref.integers(src, dst, one, K)[:, 0], np.ones(K))      # one round: exactly the K stripes
    assert cases.agreement(one, plant) > cases.agreement(lab, plant)
    new, rounds, moved, smalls = ref.refine(src, dst, lab, K, s)
    assert rounds == 1 and moved == int((one != lab).sum()) and np.array_equal(new, one)
    assert all(a > b for a, b in zip(smalls, smalls[1:]))                                # small spots fall strictly per round
    again, rounds2, moved2, _ = ref.refine(src, dst, new, K, s)
    assert rounds2 == 0 and moved2 == 0 and np.array_equal(again, new)                   # a refined map stays


def test_refinement_rules_by_hand():
    path = ([0, 1, 2], [1, 2, 3])
    new, rounds, moved, _ = ref.refine(*path, [0, 0, 1, 1], 2, 3)
    assert new.tolist() == [0, 0, 1, 1] and rounds == 0 and moved == 0                   # A A B B, s = 3: small ones never swap
    new, rounds, moved, _ = ref.refine(*path, [0, 0, 0, 1], 2, 3)
    assert new.tolist() == [0, 0, 0, 0] and rounds == 1 and moved == 1
    # the spot 2 (label 2) between a piece of three 0s and a piece of three 1s, one edge to each: the tie goes to label 0
    src, dst = [0, 1, 3, 4, 2, 2], [1, 5, 4, 6, 5, 6]
    new, rounds, moved, _ = ref.refine(src, dst, [0, 0, 2, 1, 1, 0, 1], 3, 3)
    assert new.tolist() == [0, 0, 0, 1, 1, 0, 1] and rounds == 1
    new, _, _, _ = ref.refine(src + [2], dst + [6], [0, 0, 2, 1, 1, 0, 1], 3, 3)         # a duplicate edge counts: label 1 wins
    assert new[2] == 1
    # a small piece that touches only a small piece waits: 0 - 1 - 2 - 3 - 4 - 5 labelled C B A A A A, s = 2
    src, dst = [0, 1, 2, 3, 4], [1, 2, 3, 4, 5]
    one, _ = ref.refine_round(src, dst, [2, 1, 0, 0, 0, 0], 3, 2)
    assert one.tolist() == [2, 0, 0, 0, 0, 0]
    new, rounds, moved, smalls = ref.refine(src, dst, [2, 1, 0, 0, 0, 0], 3, 2)
    assert new.tolist() == [0] * 6 and rounds == 2 and moved == 2 and smalls == [2, 1, 0]


# ------------------------------------------------------------------------------------- territory_stats
def _hand():
    """Four domains, P = 4: domain 0 in fewer pieces than every relabeling, 1 in more, 2 always the same (sd = 0), 3 empty."""
    obs = np.array([[1, 10, 0, 100], [9, 2, 8, 12], [2, 3, 1, 10], [0, 0, 0, 0]], dtype=np.int64)
    perm = np.empty((4, 4, 4), dtype=np.int64)
    perm[:, 0] = [[6, 3, 4, 22], [7, 2, 5, 18], [8, 2, 6, 16], [7, 3, 5, 20]]
    perm[:, 1] = [[4, 5, 2, 32], [5, 4, 3, 26], [3, 6, 1, 44], [4, 5, 2, 34]]
    perm[:, 2] = [[2, 3, 1, 10]] * 4
    perm[:, 3] = 0
    return obs, perm, np.array([10, 10, 4, 0], dtype=np.int64)


def test_territory_stats_by_hand():
    from spadot_amd.territories import territory_stats
    obs, perm, sizes = _hand()
    got = territory_stats(obs, perm, sizes, alpha=0.7)
    np.testing.assert_array_equal(got["largest_share"][:3], [1.0, 0.2, 0.75])
    np.testing.assert_array_equal(got["contiguity"][:3], [1.0, 0.12, 0.625])
    assert np.isnan(got["largest_share"][3]) and np.isnan(got["contiguity"][3])
    np.testing.assert_array_equal(got["count_expected"], [7.0, 4.0, 2.0, 0.0])
    np.testing.assert_allclose(got["count_sd"], [np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.0], rtol=1e-15)
    np.testing.assert_allclose(got["count_z"][:2], [-6 / np.sqrt(0.5), 5 / np.sqrt(0.5)], rtol=1e-15)
    assert np.isnan(got["count_z"][2]) and np.isnan(got["count_z"][3]) and np.isnan(got["contiguity_z"][2])     # sd = 0
    np.testing.assert_allclose(got["contiguity_expected"][:3], [0.19, 0.34, 0.625], rtol=1e-15)
    np.testing.assert_array_equal(got["p_fewer"], [0.2, 1.0, 1.0, 1.0])
    np.testing.assert_array_equal(got["p_more"], [1.0, 0.2, 1.0, 1.0])
    # the BH family is the three domains that hold spots: raw 0.4, 0.4, 1 -> 0.6, 0.6, 1; the empty one gets NaN
    np.testing.assert_allclose(got["padj"][:3], [0.6, 0.6, 1.0], rtol=1e-15)
    assert np.isnan(got["padj"][3])
    assert got["verdict"].tolist() == ["contiguous", "fragmented", "random", "random"]
    assert territory_stats(obs, perm, sizes, alpha=0.05)["verdict"].tolist() == ["random"] * 4
    want = ref.stats(obs, perm, sizes, alpha=0.7)
    for name, v in want.items():
        if name == "verdict":
            assert got[name].tolist() == v.tolist()
        else:
            np.testing.assert_allclose(got[name], v, rtol=1e-12, atol=0, err_msg=name)
    none = territory_stats(obs, perm[:0], sizes)                                         # P = 0: no null, no verdict
    assert none["verdict"].tolist() == [""] * 4 and none["contiguity"][0] == 1.0
    for name in ("count_expected", "count_sd", "count_z", "contiguity_expected", "contiguity_sd", "contiguity_z", "p_fewer",
                 "p_more", "padj"):
        assert np.all(np.isnan(none[name])), name
    assert ref.stats(obs, perm[:0], sizes)["verdict"].tolist() == [""] * 4


def test_the_null_lies_far_below_percolation():
    """What the docstring says of the null, at the size of the suite: labels dealt at random break into many small pieces."""
    _, plant, lab, src, dst, K = cases.stripes(45)
    dealt = ref.integers(src, dst, np.random.default_rng(0).permutation(lab), K)
    flipped = ref.integers(src, dst, lab, K)
    print("dealt at random:", dealt[:, 0].sum(), "territories, the largest of", dealt[:, 1].max(), "spots; flipped stripes:",
          flipped[:, 0].sum())
    assert dealt[:, 0].sum() > 10 * flipped[:, 0].sum() and dealt[:, 1].max() < 0.1 * np.bincount(lab).min()


# ------------------------------------------------------------------------------------- the driver's refusals
def _stage():
    from spadot_amd.territories import territories_stage
    return territories_stage


CASES = [
    ("no domains", dict(domains=None), ValueError, "the territories stage needs the domains table of analyze (--domains)", False),
    ("bad k", dict(k=0), ValueError, "the territories stage takes k >= 1 and n_perms = 0 .. 9999 (got k = 0, n_perms = 1000)", False),
    ("too many relabelings", dict(n_perms=10000), ValueError, "n_perms = 0 .. 9999 (got k = 6, n_perms = 10000)", False),
    ("min_size 1", dict(min_size=1), ValueError, "min_size is 0 (no refinement) or at least 2 (got 1)", False),
    ("alpha 0", dict(alpha=0.0), ValueError, "alpha is a level in (0, 1] (got 0.0)", False),
    ("33 domains", lambda i: dict(domains=i.table.assign(kmeans=np.r_[np.arange(12) % 3, [40] * 18])), ValueError,
     "at most 32 per time point", False),
    ("bad k and a bad device", dict(k=0, device="cpu"), ValueError, "the territories stage takes k >= 1", False),
    ("well-formed", {}, AssertionError, DEVICE, True),
    ("well-formed, refining without a test", dict(min_size=3, n_perms=0), AssertionError, DEVICE, True),
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
             "spadot_amd finds territories on the MI355X only (device 'cuda:N'); there is no CPU path", True)


def test_the_library_calls_refuse_cpu_tensors():
    import torch
    from spadot_amd.territories import refine_labels, territories, territory_counts
    e = (torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32))
    for call in (lambda: territory_counts([e], [np.zeros(2, np.int64)]), lambda: territories([e], [np.zeros(2, np.int64)]),
                 lambda: refine_labels(e, np.zeros(2, np.int64), 2)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    with pytest.raises(ValueError, match="min_size >= 2"):
        refine_labels(e, np.zeros(2, np.int64), 1)
    with pytest.raises(ValueError, match="one labeling block per graph"):
        territory_counts([e], [])


# ------------------------------------------------------------------------------------- the sub-command
def test_the_sub_command_and_its_defaults():
    from spadot_amd.cli import build_parser
    a = build_parser().parse_args(["territories", "--domains", "d.csv"])
    assert a.cmd_choice == "territories" and a.domains == "d.csv" and a.output_dir is None
    assert (a.k, a.n_perms, a.seed, a.min_size, a.alpha, a.prefix, a.device) == (6, 1000, 0, 0, 0.05, "", "cuda:0")
    a = build_parser().parse_args(["territories", "--domains", "d.csv", "--min_size", "5", "--n_perms", "0", "--alpha", "0.1",
                                   "--k", "8", "--seed", "3", "--prefix", "t_", "-o", "out", "--device", "cuda:1"])
    assert (a.k, a.n_perms, a.seed, a.min_size, a.alpha, a.prefix, a.device, a.output_dir) == (8, 0, 3, 5, 0.1, "t_", "cuda:1", "out")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["territories"])


def test_the_limits_the_library_states():
    from spadot_amd import stage_ops as ops
    assert ops.territory_lds_bytes(18090) == 163840 and ops.territory_lds_bytes(18091) > ops.TERRITORY_LDS_BYTES
    assert ops.territory_slab_ints(5) == 12 and ops.TERRITORY_DESC == 14
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spadot_model.h")).read()
    assert "18 090" in text and "desc [G, 14]" in text
