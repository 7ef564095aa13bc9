"""CPU: the definition of the cooccurrence stage.  The restatement against its own conditions (symmetry, monotony,
the saturated counts, an independent pair count, hand-made exact ties), the condition on the on-threshold input that makes the
GPU test of the unfused distance meaningful, the host statistics of spadot_amd.cooccurrence against the restatement on
hand-made counts, the default radii, the parser, the exit status of a missing table and the stage's refusals."""
import argparse

import numpy as np
import pytest

import cooccur_cases as cases
import cooccur_ref as ref
import nhood_cases


@pytest.mark.parametrize("name", ["edge2", "edge3", "tile257", "lattice", "on_threshold"])
def test_counts_are_symmetric_and_do_not_decrease_with_the_radius(name):
    N = cases.want(name)
    np.testing.assert_array_equal(N, N.transpose(1, 0, 2))
    assert np.all(np.diff(N, axis=2) >= 0) and N.dtype == np.int64 and N.min() >= 0


def test_at_the_diameter_every_pair_counts():
    xy, lab, _, K = cases.tile_case(257)
    far = ref.d2_matrix(xy).max()
    N = ref.counts(xy, lab, [far, 2 * far], K)
    sizes = np.bincount(lab, minlength=K)
    full = np.outer(sizes, sizes) - np.diag(sizes)
    np.testing.assert_array_equal(N[:, :, 0], full)
    np.testing.assert_array_equal(N[:, :, 1], full)


def test_the_total_equals_an_independent_pair_count():
    xy, lab, r2, K = cases.tile_case(255)
    N = cases.want("tile255")
    total = np.zeros(r2.shape[0], dtype=np.int64)
    for i in range(xy.shape[0]):                                     # spot by spot, without the label bookkeeping
        dx, dy = xy[i, 0] - xy[:, 0], xy[i, 1] - xy[:, 1]
        d2 = np.delete(dx * dx + dy * dy, i)
        total += (d2[:, None] <= r2[None, :]).sum(axis=0)
    np.testing.assert_array_equal(N.sum(axis=(0, 1)), total)
    assert total[0] > 0 and total[-1] < 255 * 254


def test_exact_ties_count_on_the_threshold_and_not_below_it():
    xy, lab = np.array([[0.0, 0.0], [3.0, 4.0]]), np.array([0, 1])
    N = ref.counts(xy, lab, [24.0, 25.0], 2)
    np.testing.assert_array_equal(N[:, :, 0], [[0, 0], [0, 0]])
    np.testing.assert_array_equal(N[:, :, 1], [[0, 1], [1, 0]])
    same = ref.counts(np.array([[1.5, 2.5], [1.5, 2.5]]), np.array([0, 0]), [0.0], 1)     # coincident spots: a pair at distance 0
    np.testing.assert_array_equal(same, [[[2]]])
    np.testing.assert_array_equal(ref.counts(np.array([[1.0, 1.0]]), np.array([0]), [0.0, 9.0], 1), [[[0, 0]]])
    np.testing.assert_array_equal(cases.want("edge1")[:, :, 0], [[0, 1], [1, 0]])
    assert not cases.want("edge0").any()
    lat = cases.want("lattice")                                      # 12 x 12: ordered pairs at distance^2 0, <= 1, <= 2
    np.testing.assert_array_equal(lat.sum(axis=(0, 1))[:3], [0, 2 * 2 * 12 * 11, 2 * 2 * 12 * 11 + 2 * 2 * 11 * 11])


def test_a_contracted_distance_would_lose_on_threshold_pairs():
    xy, lab, r2, K, pairs = cases.on_threshold()
    assert r2.shape == (64,) and np.all(np.diff(r2) > 0) and len(set(pairs)) == 64
    lost = cases.fused_misses(xy, r2, pairs)
    print(f"on-threshold pairs above their threshold under fma: {lost} of 64")
    assert lost >= 3
    N = cases.want("on_threshold")
    d2 = ref.d2_matrix(xy)
    for t, (i, j) in enumerate(pairs):                               # the pair counts at its own threshold and not one below
        assert d2[i, j] == r2[t] and (t == 0 or d2[i, j] > r2[t - 1])
    assert N[:, :, 0].sum() >= 2


def _hand_made():
    """K = 3, B = 3: domain 2 has no pairs at all (a zero row and a zero column), domain 1 none at the first radius."""
    return np.array([[[2, 6, 10], [0, 3, 4], [0, 0, 0]],
                     [[0, 3, 4], [0, 2, 2], [0, 0, 0]],
                     [[0, 0, 0], [0, 0, 0], [0, 0, 0]]], dtype=np.int64)


@pytest.mark.parametrize("ring", [False, True])
def test_statistics_on_hand_made_counts(ring):
    from spadot_amd.cooccurrence import CooccurResult, cooccurrence_stats
    N = _hand_made()
    got, want = cooccurrence_stats(N, ring=ring), ref.stats(N, ring=ring)
    for name in ("cond", "marg", "ratio"):
        assert got[name].dtype == np.float64
        np.testing.assert_allclose(got[name], want[name], rtol=1e-15, atol=0, equal_nan=True, err_msg=name)
        np.testing.assert_array_equal(np.isnan(got[name]), np.isnan(want[name]))
    assert np.all(np.isnan(got["ratio"][2])) and np.all(np.isnan(got["ratio"][:, 2]))              # zero row, zero column
    assert np.all(np.isnan(got["cond"][2])) and np.all(got["cond"][0, 2] == 0) and np.all(got["marg"][2] == 0)
    assert np.all(np.isnan(got["ratio"][1, :, 0])) and np.all(np.isnan(got["ratio"][:, 1, 0]))     # domain 1 at the first radius
    if ring:                                                          # the annulus (r_0, r_1]: N[.., 1] - N[.., 0]
        assert got["cond"][0, 0, 1] == 4 / 7 and got["marg"][0, 1] == 7 / 12
        assert got["ratio"][0, 0, 1] == (4 / 7) / (7 / 12)
        np.testing.assert_array_equal(got["cond"][:, :, 0], cooccurrence_stats(N)["cond"][:, :, 0])
    else:
        assert got["cond"][0, 0, 1] == 6 / 9 and got["marg"][0, 1] == 9 / 14
        assert got["ratio"][0, 0, 1] == (6 / 9) / (9 / 14)
        assert got["ratio"][0, 0, 0] == 1.0
    r = CooccurResult(N, np.array([1.0, 2.0, 3.0]), np.array([3, 2, 1]), ring=ring)
    np.testing.assert_array_equal(r.ratio, got["ratio"])
    assert r.counts is N and r.ring == ring
    with pytest.raises(ValueError, match=r"\[K, K, B\]"):
        cooccurrence_stats(np.zeros((2, 3, 4), dtype=np.int64))


def test_default_radii_on_a_known_bounding_box():
    from spadot_amd.cooccurrence import default_radii, ladder
    xy = np.array([[10.0, 5.0], [13.0, 6.0], [40.0, 45.0], [12.0, 44.0]])            # 30 x 40: diagonal 50, r_max 12.5
    np.testing.assert_array_equal(default_radii(xy, 5), [2.5, 5.0, 7.5, 10.0, 12.5])
    r = default_radii(xy)
    assert r.shape == (50,) and r[-1] == 12.5 and r[0] == 0.25 and np.all(np.diff(r) > 0)
    np.testing.assert_array_equal(r, ref.default_radii(xy, 50))
    np.testing.assert_array_equal(ladder(8.0, 4), [2.0, 4.0, 6.0, 8.0])
    with pytest.raises(ValueError, match="coincide"):
        default_radii(np.array([[2.0, 3.0], [2.0, 3.0], [2.0, 3.0]]), 10)
    with pytest.raises(ValueError, match="1 to 64"):
        default_radii(xy, 65)
    with pytest.raises(ValueError, match="1 to 64"):
        default_radii(xy, 0)
    with pytest.raises(ValueError, match="finite"):
        default_radii(np.array([[0.0, 0.0], [np.inf, 1.0]]), 10)


def test_the_parser_takes_the_cooccurrence_sub_command():
    from spadot_amd.cli import build_parser
    a = build_parser().parse_args(["cooccurrence", "--domains", "d.csv"])
    assert (a.cmd_choice, a.domains, a.output_dir, a.prefix, a.bins, a.radius, a.ring, a.device) == \
        ("cooccurrence", "d.csv", None, "", 50, None, False, "cuda:0")
    a = build_parser().parse_args(["cooccurrence", "--domains", "d.csv", "-o", "out", "--prefix", "p_", "--bins", "20",
                                   "--radius", "150.5", "--ring", "--device", "cuda:1"])
    assert (a.output_dir, a.prefix, a.bins, a.radius, a.ring, a.device) == ("out", "p_", 20, 150.5, True, "cuda:1")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["cooccurrence"])                         # --domains is required
    import spadot_amd.cli as cli
    assert "cooccurrence --domains CSV" in cli.__doc__ and "DESIGN 7i" in cli.__doc__


def test_a_missing_domains_table_exits_with_status_2(tmp_path, capsys):
    from spadot_amd.cli import main
    with pytest.raises(SystemExit) as e:
        main(["cooccurrence", "--domains", str(tmp_path / "nothing.csv")])
    assert e.value.code == 2
    assert "SpaDOT cooccurrence: the domains table does not exist" in capsys.readouterr().err


def test_the_stage_refuses_a_table_without_coordinates_and_a_cpu_device(tmp_path):
    from spadot_amd.cooccurrence import cooccur
    df = nhood_cases.stage_table()
    with pytest.raises(ValueError, match="pixel_x"):
        cooccur(argparse.Namespace(domains=df.drop(columns=["pixel_x"]), output_dir=str(tmp_path)))
    with pytest.raises(RuntimeError, match="MI355X only"):
        cooccur(argparse.Namespace(domains=df, output_dir=str(tmp_path), device="cpu"))
    with pytest.raises(ValueError, match="more than once|domains"):
        cooccur(argparse.Namespace(domains=df.assign(kmeans=40), output_dir=str(tmp_path), device="cpu"))
    with pytest.raises(ValueError, match="1 to 64"):
        cooccur(argparse.Namespace(domains=df, output_dir=str(tmp_path), bins=65, device="cpu"))
    same = df.assign(pixel_x=1.0, pixel_y=2.0)
    with pytest.raises(ValueError, match="coincide"):
        cooccur(argparse.Namespace(domains=same, output_dir=str(tmp_path), device="cuda:0"))


def test_the_library_takes_cpu_tensors_nowhere():
    import torch
    from spadot_amd.cooccurrence import cooccurrence, cooccurrence_counts
    xy, lab, r2, K = cases.edge_call()[2]
    with pytest.raises(RuntimeError, match="MI355X only.*no CPU path"):
        cooccurrence_counts([torch.as_tensor(xy)], [lab], radii_sq=[r2])
    with pytest.raises(RuntimeError, match="MI355X only.*no CPU path"):
        cooccurrence([torch.as_tensor(xy)], [lab])
    with pytest.raises(ValueError, match="exactly one"):
        cooccurrence_counts([torch.as_tensor(xy)], [lab])
