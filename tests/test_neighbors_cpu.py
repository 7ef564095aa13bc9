"""CPU: the definition of the neighbors stage.  The restatement's permutation is a bijection and a sound generator
(its count means against the analytic expectation, its spreads against numpy's own permutations), the host statistics of
spadot_amd.neighbors against the restatement on hand-made count stacks, the host post-processing of the k-nearest-neighbour
rows, the parser and the exit status of a missing table.

Bounds (set by the definition's issue, from the Monte-Carlo error at P = 1000): every cell's permutation mean within 4.5 standard
errors of E n_a n_b / (n (n - 1)) (diagonal: E n_a (n_a - 1) / (n (n - 1))) -- over fewer than 100 cells a one-in-10^4 event for
a sound generator; every cell's sd within 15 % of the sd under numpy.random.default_rng(0).permutation, 4.7 times the 3.2 %
Monte-Carlo sd of such a ratio.  The tests print the figures."""
import numpy as np
import pytest

import nhood_cases as cases
import nhood_ref as ref


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 257, 1000, 4097])
def test_the_permutation_is_a_bijection(n):
    for seed, g, p in ((7, 1, 0), (7, 1, 1), (0, 0, 0), (-3, 4, 2 ** 32 - 1)):
        np.testing.assert_array_equal(np.sort(ref.perm(n, seed, g, p)), np.arange(n))


def test_the_permutation_differs_with_seed_graph_and_index():
    base = ref.perm(1000, 7, 1, 0)
    for other in ((8, 1, 0), (7, 2, 0), (7, 1, 1)):
        assert not np.array_equal(ref.perm(1000, *other), base), other
    np.testing.assert_array_equal(ref.perm(1000, 7, 1, 0), base)                   # a pure function of its arguments
    np.testing.assert_array_equal(ref.perm(1000, 7 + 2 ** 64, 1, 0), base)         # the seed is taken modulo 2^64
    assert ref.domain_bits(1) == ref.domain_bits(4) == 2 and ref.domain_bits(5) == 4 and ref.domain_bits(2 ** 31 - 1) == 32


@pytest.mark.parametrize("side", sorted(cases.PLANTED))
def test_the_generator_is_sound_on_planted_domains(side):
    _, lab, src, dst, K = cases.planted(side)
    n, E, P = lab.shape[0], src.shape[0], 1000
    cf = cases.planted_perm_counts(side, P)
    assert cf.shape == (P, K, K) and np.all(cf.sum(axis=(1, 2)) == E)
    sizes = np.bincount(lab, minlength=K)
    dev =(cf.mean(0) - ref.analytic_expectation(E, sizes)) / (cf.std(0) / np.sqrt(P))
    rng = np.random.default_rng(0)
    cn = np.stack([ref.count_matrix(src, dst, rng.permutation(lab), K) for _ in range(P)])
    ratio = cf.std(0) / cn.std(0)
    print(f"side {side}: n {n}, K {K}, max |mean - analytic| / se {np.abs(dev).max():.2f}, sd ratio {ratio.min():.3f} .. "
          f"{ratio.max():.3f}")
    assert np.abs(dev).max() <= 4.5
    assert ratio.min() >= 0.85 and ratio.max() <= 1.15


def test_count_matrix_counts_duplicates_and_its_rows_sum_to_the_out_degrees():
    src, dst = np.array([0, 0, 1, 2, 2, 2]), np.array([1, 1, 2, 0, 1, 3])
    lab = np.array([0, 1, 1, 2])
    C = ref.count_matrix(src, dst, lab, 3)
    np.testing.assert_array_equal(C, [[0, 2, 0], [1, 2, 1], [0, 0, 0]])          # 0 -> 1 twice; nodes 1 and 2 form domain 1
    np.testing.assert_array_equal(C.sum(axis=1), [2, 4, 0])


def _hand_made():
    """K = 3 with an empty domain 2, P = 4: a cell that never varies (sd = 0), ties with the observed count, a zero row."""
    counts = np.array([[5, 3, 0], [2, 0, 0], [0, 0, 0]], dtype=np.int64)
    perms = np.array([[[4, 4, 0], [2, 0, 0], [0, 0, 0]],
                      [[5, 3, 0], [2, 0, 0], [0, 0, 0]],
                      [[6, 2, 0], [1, 1, 0], [0, 0, 0]],
                      [[3, 5, 0], [2, 0, 0], [0, 0, 0]]], dtype=np.int32)
    return counts, perms, np.array([6, 2, 0], dtype=np.int64)


def test_statistics_on_hand_made_stacks():
    from spadot_amd.neighbors import NhoodResult, enrichment_stats
    counts, perms, sizes = _hand_made()
    got, want = enrichment_stats(counts, perms, sizes), ref.stats(counts, perms, sizes)
    for name in ("expected", "sd", "zscore", "p_enriched", "p_depleted", "padj", "share", "coherence"):
        np.testing.assert_allclose(got[name], want[name], rtol=1e-15, atol=0, equal_nan=True, err_msg=name)
    assert got["expected"][0, 0] == 4.5 and got["sd"][0, 0] == np.sqrt(1.25)
    assert got["zscore"][0, 0] == 0.5 / np.sqrt(1.25)
    assert np.isnan(got["zscore"][0, 2]) and np.isnan(got["zscore"][2, 2]) and got["sd"][0, 2] == 0      # sd = 0 -> NaN
    assert got["p_enriched"][0, 0] == 3 / 5 and got["p_depleted"][0, 0] == 4 / 5                       # ties count on both sides
    assert got["p_enriched"][1, 1] == 1.0 and got["p_depleted"][1, 1] == 4 / 5
    assert np.all(np.isnan(got["padj"][2, :])) and np.all(np.isnan(got["padj"][:, 2]))                 # the empty domain is left out
    raw = np.minimum(1.0, 2 * np.minimum(got["p_enriched"], got["p_depleted"]))[:2, :2].reshape(-1)
    np.testing.assert_allclose(got["padj"][:2, :2].reshape(-1), ref.bh(raw), rtol=1e-15)                # a family of 4, not of 9
    assert np.all(got["padj"][:2, :2] <= 1.0) and np.all(got["padj"][:2, :2] >= raw.reshape(2, 2))
    np.testing.assert_array_equal(got["share"][0], [5 / 8, 3 / 8, 0.0])
    assert np.all(np.isnan(got["share"][2])) and np.isnan(got["coherence"][2]) and got["coherence"][1] == 0.0
    r = NhoodResult(counts, perms, sizes)
    np.testing.assert_array_equal(r.zscore, got["zscore"])
    assert r.perm_counts is perms and r.counts is counts


def test_bh_of_the_restatement_against_a_known_family():
    np.testing.assert_allclose(ref.bh([0.01, 0.04, 0.03, 0.5]), [0.04, 0.04 * 4 / 3, 0.04 * 4 / 3, 0.5], rtol=1e-15)
    from spadot_amd.markers import bh_adjust
    p = np.random.default_rng(3).uniform(size=50)
    np.testing.assert_allclose(bh_adjust(p), ref.bh(p), rtol=1e-15)


def test_knn_rows_drop_the_spot_wherever_it_stands():
    import torch
    from spadot_amd.neighbors import knn_rows_to_edges
    # spots 0, 1, 2 share their coordinates: ordered by (distance, index) spot 1 stands in column 1 of its row and spot 2 in
    # column 2 of its; with k = 2 spot 3 (three duplicates below it) would not stand in its own row at all
    idx = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 5]], dtype=torch.int32)
    src, dst = knn_rows_to_edges(idx, 3)
    np.testing.assert_array_equal(src.numpy(), [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3])
    np.testing.assert_array_equal(dst.numpy(), [1, 2, 3, 0, 2, 3, 0, 1, 4, 0, 1, 2])
    assert src.dtype == torch.int32 and dst.dtype == torch.int32
    src, dst = knn_rows_to_edges(idx[:, :3], 2)                              # rows of k + 1 = 3; row 3 holds three others
    np.testing.assert_array_equal(src.numpy(), [0, 0, 1, 1, 2, 2, 3, 3])
    np.testing.assert_array_equal(dst.numpy(), [1, 2, 0, 2, 0, 1, 0, 1])
    src, dst = knn_rows_to_edges(torch.tensor([[0, 1], [1, 0]], dtype=torch.int32), 6)      # n = 2 <= k: n - 1 neighbours
    np.testing.assert_array_equal(src.numpy(), [0, 1])
    np.testing.assert_array_equal(dst.numpy(), [1, 0])


def test_same_share_of_the_restatement():
    src, dst = np.array([0, 0, 1, 3]), np.array([1, 3, 0, 0])
    got = ref.same_share(src, dst, np.array([0, 0, 1, 1]), 4)
    np.testing.assert_array_equal(got[[0, 1, 3]], [0.5, 1.0, 0.0])
    assert np.isnan(got[2])


def test_the_parser_takes_the_neighbors_sub_command():
    from spadot_amd.cli import build_parser
    a = build_parser().parse_args(["neighbors", "--domains", "d.csv"])
    assert (a.cmd_choice, a.domains, a.output_dir, a.prefix, a.k, a.n_perms, a.seed, a.device) == \
        ("neighbors", "d.csv", None, "", 6, 1000, 0, "cuda:0")
    a = build_parser().parse_args(["neighbors", "--domains", "d.csv", "-o", "out", "--prefix", "p_", "--k", "8", "--n_perms", "50",
                                   "--seed", "9", "--device", "cuda:1"])
    assert (a.output_dir, a.prefix, a.k, a.n_perms, a.seed, a.device) == ("out", "p_", 8, 50, 9, "cuda:1")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["neighbors"])                            # --domains is required
    import spadot_amd.cli as cli
    assert "neighbors --domains CSV" in cli.__doc__


def test_a_missing_domains_table_exits_with_status_2(tmp_path, capsys):
    from spadot_amd.cli import main
    with pytest.raises(SystemExit) as e:
        main(["neighbors", "--domains", str(tmp_path / "nothing.csv")])
    assert e.value.code == 2
    assert "SpaDOT neighbors: the domains table does not exist" in capsys.readouterr().err


def test_the_stage_refuses_a_table_without_coordinates_and_a_cpu_device(tmp_path):
    import argparse
    from spadot_amd.neighbors import neighbors
    df = cases.stage_table()
    with pytest.raises(ValueError, match="pixel_x"):
        neighbors(argparse.Namespace(domains=df.drop(columns=["pixel_x"]), output_dir=str(tmp_path)))
    with pytest.raises(RuntimeError, match="MI355X only"):
        neighbors(argparse.Namespace(domains=df, output_dir=str(tmp_path), device="cpu"))
    with pytest.raises(ValueError, match="more than once|domains"):
        neighbors(argparse.Namespace(domains=df.assign(kmeans=40), output_dir=str(tmp_path), device="cpu"))
