"""CPU: the correlogram stage without a device.  The numpy restatement against itself and against the restatement of
the co-occurrence counts; the host statistics on the planted lattice (signs and ranges); the frame of the driver in the manner of
test_stage_frame_cpu.py; the command line, the ladder of bands and the layout helpers of the launch."""
import argparse
import os

import numpy as np
import pytest

import cooccur_ref
import correlogram_cases as cg
import correlogram_ref as ref


# ------------------------------------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("name", ["sized257_7", "sized255_16", "lattice", "on_threshold", "coincident"])
def test_the_bands_partition_the_pairs_within_the_last_radius(name):
    xy, X, r2 = cg.problem(name)
    n, B = xy.shape[0], r2.shape[0]
    band = ref.bands(xy, r2)
    d2 = cooccur_ref.d2_matrix(xy)
    off = ~np.eye(n, dtype=bool)
    assert np.all(band[~off] == B) and band.min() >= 0 and band.max() <= B
    np.testing.assert_array_equal(band[off] < B, d2[off] <= r2[-1])                  # in a band exactly when within r_{B-1}
    lo = np.concatenate([[-1.0], r2[:-1]])
    for b in range(B):
        np.testing.assert_array_equal((band == b) & off, (d2 > lo[b]) & (d2 <= r2[b]) & off)
    np.testing.assert_array_equal(band, band.T)                                     # a band is a symmetric graph
    W = cg.want(name)[0]
    assert int(W.sum()) == int((band < B).sum())


@pytest.mark.parametrize("name", ["sized513_7", "sized256_1", "lattice", "on_threshold", "coincident"])
def test_the_cumulated_pair_counts_are_the_cooccurrence_counts_of_one_label(name):
    xy, X, r2 = cg.problem(name)
    W, S2c = ref.integers(xy, r2)
    np.testing.assert_array_equal(np.cumsum(W), cooccur_ref.counts(xy, np.zeros(xy.shape[0], np.int64), r2, 1)[0, 0])
    np.testing.assert_array_equal(W, cg.want(name)[0])
    assert np.all(S2c >= W) and np.all(S2c * xy.shape[0] >= W * W)                  # Cauchy-Schwarz on the partner counts


def test_the_coincident_pair_lies_in_band_zero_and_on_threshold_pairs_in_their_own():
    xy, X, r2 = cg.coincident()
    band = ref.bands(xy, r2)
    assert band[0, 1] == band[1, 0] == 0 and band[0, 2] == 1
    xy, X, r2, pairs = cg.on_threshold()
    band = ref.bands(xy, r2)
    for t, (i, j) in enumerate(pairs):
        assert band[i, j] == t and cooccur_ref.d2_matrix(xy)[i, j] == r2[t]


@pytest.mark.parametrize("name", ["sized257_7", "lattice", "planted"])
def test_geary_sum_from_the_two_device_sums_is_the_direct_one(name):
    xy, X, r2 = cg.problem(name)
    W, S2c, N, Q, AN, AQ = cg.want(name)
    D = ref.direct_D(xy, X, r2)
    assert np.all(np.abs(2.0 * Q[:, 0] - 2.0 * N[:, 0] - D) <= 8.0 * ref.tolerance(xy.shape[0], AQ[:, 0] + AN[:, 0]))
    assert D.max() > 0


def test_a_labeling_shows_the_permuted_rows():
    import nhood_ref
    xy, X, r2 = cg.problem("sized255_16")
    both = ref.all_sums(xy, X, r2, 2, cg.SEED, 3, first=4)
    alone = ref.sums(xy, X[nhood_ref.perm(255, cg.SEED, 3, 5)], r2)
    np.testing.assert_array_equal(both[2][:, 2], alone[2])
    np.testing.assert_array_equal(both[2][:, 0], ref.sums(xy, X, r2)[2])


# --------------------------------------------------------------------------------------------------------- the host part
def _planted_stats(alpha=0.05):
    from spadot_amd.correlogram import corr_stats
    xy, V = cg.planted()
    W, S2c, N, Q, _, _ = cg.want("planted")
    X = cg.centred(V)
    return corr_stats(W, S2c, N, Q, 1024, (X * X).sum(axis=0), np.asarray(cg.PLANTED_RADII), (V * V).sum(axis=0), alpha)


def test_the_planted_genes_have_their_signs_and_ranges():
    s = _planted_stats()
    smooth, noise, checker = 0, 1, 2
    assert not s["degenerate"].any()
    # the smooth gene: strongly positive up to 8, negative from 10 on; its range is 8 and it does not reach past the ladder
    assert np.all(s["z_norm"][smooth, :5] > 20) and np.all(s["z_norm"][smooth, 6:] < -5)
    assert np.all(np.diff(s["I"][smooth, :6]) < 0) and s["I"][smooth, 0] > 0.8
    assert s["range"][smooth] == 8.0 and not s["open"][smooth]
    # white noise: nothing in any band
    assert np.all(np.abs(s["z_norm"][noise]) < 3.5) and s["range"][noise] == 0.0 and not s["open"][noise]
    # the checkerboard: strongly negative among the nearest neighbours
    assert s["I"][checker, 0] < -0.5 and s["z_norm"][checker, 0] < -20 and s["range"][checker] == 0.0
    # the semivariance of the smooth gene rises to the sill; that of the noise starts there
    assert s["gamma_first"][smooth] < 0.1 * s["sill"][smooth] and abs(s["gamma_first"][noise] / s["sill"][noise] - 1) < 0.1
    assert np.all(np.diff(s["gamma"][smooth, :6]) > 0)
    assert np.all((s["padj"] >= s["p_norm"] - 1e-15) | np.isnan(s["padj"])) and np.all(np.isnan(s["z_sim"]))


def test_a_looser_level_cannot_shorten_a_range():
    tight, loose = _planted_stats(0.001), _planted_stats(0.5)
    assert np.all(loose["range"] >= tight["range"])


def test_empty_bands_and_degenerate_genes_are_nan_and_left_out_of_bh():
    from spadot_amd.correlogram import corr_stats
    from spadot_amd.markers import bh_adjust
    xy, V = cg.planted()
    r = np.array([0.3, 1.3, 2.5])                                                    # no two spots lie within 0.3
    V = np.concatenate([V, np.full((1024, 1), 2.5)], axis=1)                          # a flat gene
    X = cg.centred(V)
    W, S2c, N, Q, _, _ = ref.all_sums(xy, X, r * r, 3, 1, 0)
    assert W[0] == 0 and W[1] > 0
    s = corr_stats(W, S2c, N, Q, 1024, (X * X).sum(axis=0), r, (V * V).sum(axis=0))
    assert s["degenerate"].tolist() == [False, False, False, True]
    for name in ("I", "C", "z_norm", "p_norm", "z_sim", "p_sim", "padj", "gamma"):
        assert np.all(np.isnan(s[name][:, 0])) and np.all(np.isnan(s[name][3])), name
        assert not np.isnan(s[name][:3, 1:]).any(), name
    assert np.all(s["range"][:3] == 0.0) and np.isnan(s["range"][3]) and not s["open"].any()      # the first band holds nothing
    np.testing.assert_allclose(s["padj"][:3, 1], bh_adjust(s["p_sim"][:3, 1]))                       # three genes in the family
    assert np.all(s["p_sim"][:3, 1:] >= 0.25) and np.isnan(s["sill"][3]) and s["sill"][2] == pytest.approx(0.25)


def test_the_range_counts_the_leading_bands_only():
    from spadot_amd.correlogram import corr_stats
    xy, V = cg.planted()
    W, S2c, N, Q, _, _ = cg.want("planted")
    X = cg.centred(V)
    r = np.asarray(cg.PLANTED_RADII)
    s = corr_stats(W[:5], S2c[:5], N[:, :, :5], Q[:, :, :5], 1024, (X * X).sum(axis=0), r[:5])
    assert s["range"][0] == 8.0 and s["open"][0]                                     # every band of the shorter ladder holds
    Nz = N.copy()
    Nz[0, 0, 2] = -abs(N[0, 0, 2])                                                   # break the run at band 2
    s = corr_stats(W, S2c, Nz, Q, 1024, (X * X).sum(axis=0), r)
    assert s["range"][0] == 2.5 and not s["open"][0]
    with pytest.raises(ValueError, match="corr_stats takes"):
        corr_stats(W[:3], S2c, N, Q, 1024, (X * X).sum(axis=0), r)


# -------------------------------------------------------------------------------------------------- the frame of the driver
DEVICE = "the device was asked for"


class Inputs:
    """2 time points of 12 and 18 rows and 8 genes as counts.npz, and `out`, a directory that does not exist yet."""

    def __init__(self, root):
        rng = np.random.default_rng(5)
        self.out = str(root / "out")
        self.counts = str(root / "counts.npz")
        np.savez(self.counts, X=rng.poisson(2.0, (30, 8)).astype(np.float32), timepoint=np.repeat(np.asarray(["E10", "E12"]), (12, 18)),
                 spatial=rng.random((30, 2)) * 100.0, genes=np.asarray([f"g{i}" for i in range(8)]))
        self.missing = str(root / "nowhere.npz")


LIMITS = "the correlogram stage takes top >= 1, k >= 1, 1 <= bins <= 16, n_perms >= 0 and 0 < alpha <= 1 (got "
CASES = [
    ("bad bins and no data file", lambda i: dict(bins=17, data=i.missing), ValueError, LIMITS + "top = 50, k = 6, bins = 17", False),
    ("bad top", dict(top=0), ValueError, LIMITS + "top = 0", False),
    ("bad alpha and unordered radii", dict(alpha=0.0, radii="3,2"), ValueError, "alpha = 0.0)", False),
    ("negative permutations", dict(n_perms=-1), ValueError, "n_perms = -1", False),
    ("unordered radii and an unknown gene", dict(radii="3,2", genes="g1,nope"), ValueError, "--radii takes 1 to 16 finite radii", False),
    ("seventeen radii", dict(radii=",".join(str(i + 1) for i in range(17))), ValueError, "--radii takes 1 to 16 finite radii", False),
    ("radii that are no numbers", dict(radii="1,two"), ValueError, "--radii takes a comma-separated list of numbers", False),
    ("well-formed: the device before the genes", dict(genes="g1,nope"), AssertionError, DEVICE, False),
    ("well-formed: the device before the data", lambda i: dict(data=i.missing), AssertionError, DEVICE, False),
]
CASES_WITH_DEVICE = [
    ("an unknown gene and a bad device", dict(genes="g1,nope", device="cpu"), RuntimeError,
     "spadot_amd takes the correlogram on the MI355X only (device 'cuda:N'); there is no CPU path", False),
    ("an unknown gene", dict(genes="g1,nope"), ValueError, "--genes names 1 genes that the data does not hold: nope", False),
    ("no data file", lambda i: dict(data=i.missing), FileNotFoundError, "nowhere.npz", False),
]


def _refused(tmp_path, change, exc, fragment, made):
    from spadot_amd.correlogram import correlogram_stage
    inp = Inputs(tmp_path)
    kw = dict(data=inp.counts, output_dir=inp.out, device="cuda:0")
    kw.update(change(inp) if callable(change) else change)
    with pytest.raises(exc) as e:
        correlogram_stage(argparse.Namespace(**kw))
    assert type(e.value) is exc and fragment in str(e.value), str(e.value)
    assert os.path.isdir(inp.out) == made


@pytest.mark.parametrize("case,change,exc,fragment,made", CASES, ids=[c[0] for c in CASES])
def test_the_driver_refuses_before_it_asks_for_the_device(tmp_path, monkeypatch, case, change, exc, fragment, made):
    import torch

    def no_device(*a, **k):
        raise AssertionError(DEVICE)
    monkeypatch.setattr(torch, "device", no_device)
    _refused(tmp_path, change, exc, fragment, made)


@pytest.mark.parametrize("case,change,exc,fragment,made", CASES_WITH_DEVICE, ids=[c[0] for c in CASES_WITH_DEVICE])
def test_the_driver_refuses_with_a_device_named(tmp_path, case, change, exc, fragment, made):
    _refused(tmp_path, change, exc, fragment, made)


# ----------------------------------------------------------------------------------------------- command line and ladder
def test_the_command_line_of_the_stage():
    from spadot_amd.cli import build_parser
    a = build_parser().parse_args(["correlogram", "-i", "counts.npz"])
    assert (a.cmd_choice, a.data, a.genes, a.top, a.bins, a.radii, a.n_perms, a.alpha, a.seed, a.output_dir, a.prefix, a.device) == \
        ("correlogram", "counts.npz", None, 50, 12, None, 0, 0.05, 0, None, "", "cuda:0")
    a = build_parser().parse_args(["correlogram", "-i", "c.npz", "--genes", "a,b", "--radii", "1,2.5,4", "--n_perms", "99", "--alpha",
                                   "0.01", "--seed", "3", "-o", "out", "--prefix", "p_", "--device", "cuda:1", "--bins", "7",
                                   "--top", "5"])
    assert (a.genes, a.radii, a.n_perms, a.alpha, a.seed, a.output_dir, a.prefix, a.device, a.bins, a.top) == \
        ("a,b", "1,2.5,4", 99, 0.01, 3, "out", "p_", "cuda:1", 7, 5)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["correlogram"])


def test_a_missing_counts_file_ends_the_command(tmp_path, capsys):
    from spadot_amd.cli import main
    with pytest.raises(SystemExit) as e:
        main(["correlogram", "-i", str(tmp_path / "nowhere.npz")])
    assert e.value.code == 2 and "SpaDOT correlogram: the counts do not exist" in capsys.readouterr().err


def test_the_default_bands_and_the_radii_of_the_command_line():
    from spadot_amd.correlogram import default_bands, parse_radii
    from spadot_amd.pairs import default_radii, ladder
    xy = np.array([[0.0, 0.0], [30.0, 40.0], [3.0, 4.0]])
    np.testing.assert_array_equal(default_bands(xy), ladder(12.5, 12))
    np.testing.assert_array_equal(default_bands(xy, 16), default_radii(xy, 16))
    assert default_bands(xy, 1).tolist() == [12.5]
    for bins in (0, 17, -1):
        with pytest.raises(ValueError, match="the correlogram takes 1 to 16 distance bands"):
            default_bands(xy, bins)
    with pytest.raises(ValueError, match="the spots all coincide"):
        default_bands(np.ones((4, 2)))
    assert parse_radii("1, 2.5,4").tolist() == [1.0, 2.5, 4.0] and parse_radii("0").tolist() == [0.0]
    for bad in ("", "2,1", "1,1", "-1,2", "1,inf", "nan"):
        with pytest.raises(ValueError, match="--radii takes"):
            parse_radii(bad)


def test_the_morton_order_is_a_permutation_by_key_then_index():
    from spadot_amd.correlogram import morton_order
    from spadot_amd.graph import morton_key
    xy = cg.sparse()[0]
    order = morton_order(xy)
    assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(1100))
    key = morton_key(xy)[order]
    assert np.all(np.diff(key.astype(np.int64)) >= 0)
    same = np.array([[1.0, 1.0]] * 5 + [[2.0, 3.0]])
    assert morton_order(same).tolist() == [0, 1, 2, 3, 4, 5]                          # ties by index
    # the first quarter of the order is the quadrant of the smallest coordinates
    first = xy[order[:(key < (1 << 30)).sum()]]
    assert first.shape[0] > 200 and first.max() < 20.1


def test_the_layout_of_a_launch_and_its_refusals_without_a_device():
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.correlogram import corr_sums, correlogram
    boff, blocks = ops.corr_layout([1, 256, 257, 513])
    assert boff.tolist() == [0, 1, 2, 4] and blocks == 7
    assert ops.corr_scratch_doubles(7, 3, 6, 16) == 28 + 2 * 7 * 6 * 3 * 16
    xy = torch.zeros((4, 2), dtype=torch.float64)
    desc = np.array([[0, 4, 1, 0, 0, 0]])
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.corr_sums(xy, torch.arange(4, dtype=torch.int32), torch.zeros((4, 16), dtype=torch.float64), desc, [[1.0]], 1, True, 0, 0)
    with pytest.raises(RuntimeError, match="spadot_amd takes the correlogram on the MI355X only"):
        corr_sums([xy], Z=[torch.zeros((4, 1), dtype=torch.float64)], radii=[[1.0]])
    with pytest.raises(RuntimeError, match="spadot_amd takes the correlogram on the MI355X only"):
        correlogram([xy], [torch.zeros((4, 1))], radii=[1.0])
    with pytest.raises(ValueError, match="n_perms >= 0 and 0 < alpha <= 1"):
        correlogram([xy], [torch.zeros((4, 1))], alpha=2.0)
