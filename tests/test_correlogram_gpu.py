"""GPU: spadot_corr_sums (csrc/correlogram.hip) and the correlogram stage against the numpy restatement (tests/correlogram_ref.py;
DESIGN 7o): exact integers, the floating-point sums within the bound of their summation order, the labeling convention of
autocorr, the invariances of the fixed order (bit for bit), the stage on the planted lattice, and the refusals before any launch."""
import argparse
import os

import numpy as np
import pytest

import correlogram_cases as cg
import correlogram_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.array(a), device=DEV) if dtype is None else \
        torch.as_tensor(np.array(a), device=DEV).to(dtype)


def _sums(names, n_perms=0, seed=cg.SEED, **kw):
    """corr_sums over the named cases as one call on their centred values."""
    from spadot_amd.correlogram import corr_sums
    probs = [cg.problem(name) for name in names]
    return corr_sums([_dev(p[0]) for p in probs], Z=[_dev(p[1]) for p in probs], radii_sq=[p[2] for p in probs], n_perms=n_perms,
                     seed=seed, **kw)


def _close(got, want, A, n, what):
    tol = ref.tolerance(n, A)
    err = np.abs(got - want)
    print(f"{what}: largest error {err.max():.3e}, smallest bound {tol.min():.3e}, largest error / bound "
          f"{(err / np.maximum(tol, 1e-300)).max():.3e}")
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert np.all(err <= tol), what


# ------------------------------------------------------------------------------------------------------------ exact integers
@pytest.mark.parametrize("B", cg.BAND_COUNTS)
def test_the_integers_are_exact_around_the_tile(B):
    names = [f"sized{n}_{B}" for n in cg.SIZES]
    W, S2c, N, Q = _sums(names)
    for t, name in enumerate(names):
        want = cg.want(name)
        np.testing.assert_array_equal(W[t], want[0], err_msg=name)
        np.testing.assert_array_equal(S2c[t], want[1], err_msg=name)
        assert W[t].dtype == np.int64 and W[t].shape == (B,) and N[t].shape == (3, 1, B)


@pytest.mark.parametrize("name", ["lattice", "on_threshold", "coincident"])
def test_the_integers_are_exact_on_the_thresholds(name):
    W, S2c, N, Q = _sums([name])
    want = cg.want(name)
    np.testing.assert_array_equal(W[0], want[0])
    np.testing.assert_array_equal(S2c[0], want[1])
    if name == "coincident":
        assert W[0].tolist() == [2, 4]                                                # the coincident pair, both ways, in band 0


@pytest.mark.parametrize("name", ["sized513_7", "lattice", "on_threshold", "sparse"])
def test_the_cumulated_pairs_are_the_cooccurrence_counts_of_one_domain(name):
    import torch
    from spadot_amd.cooccurrence import cooccurrence_counts
    xy, X, r2 = cg.problem(name)
    W = _sums([name])[0][0]
    co = cooccurrence_counts([_dev(xy)], [torch.zeros(xy.shape[0], dtype=torch.int64, device=DEV)], radii_sq=[r2])[0]
    np.testing.assert_array_equal(np.cumsum(W), co[0, 0])


# ------------------------------------------------------------------------------------------------- the floating-point sums
@pytest.mark.parametrize("names", [tuple(f"sized{n}_7" for n in cg.SIZES), ("sized257_16", "sized513_1", "lattice"),
                                   ("on_threshold", "coincident")], ids=["tile sizes", "band counts", "thresholds"])
def test_the_sums_agree_with_the_restatement_on_the_devices_own_image(names):
    W, S2c, N, Q, Z = _sums(list(names), n_perms=2, images=True)
    for t, name in enumerate(names):
        xy, X, r2 = cg.problem(name)
        np.testing.assert_array_equal(Z[t], X)                                       # the image is the values that were given
        _, _, wN, wQ, AN, AQ = ref.all_sums(xy, Z[t], r2, 2, cg.SEED, t)
        _close(N[t], wN, AN, xy.shape[0], f"N of {name}")
        _close(Q[t], wQ, AQ, xy.shape[0], f"Q of {name}")


def test_the_image_of_counts_and_of_dense_columns_carries_the_sums():
    """Through moran.columns: dense fp32 columns and their centre, as the stage hands them over."""
    from spadot_amd.correlogram import corr_sums
    xy, X, r2 = cg.problem("sized257_7")
    V = (X * 3.0 + 1.0).astype(np.float32)
    W, S2c, N, Q, Z = corr_sums([_dev(xy)], [_dev(V)], genes=[2, 0], radii_sq=[r2], n_perms=1, seed=3, images=True)
    c = V.astype(np.float64).mean(axis=0)
    assert np.abs(Z[0] - (V.astype(np.float64) - c)[:, [2, 0]]).max() <= 1e-12
    _, _, wN, wQ, AN, AQ = ref.all_sums(xy, Z[0], r2, 1, 3, 0)
    _close(N[0], wN, AN, 257, "N of dense columns")
    _close(Q[0], wQ, AQ, 257, "Q of dense columns")


# ------------------------------------------------------------------------------------------------ the labeling convention
def test_one_band_is_the_edge_sum_of_autocorr_on_the_graph_of_all_pairs_within_r():
    import torch
    from spadot_amd.autocorr import autocorr_sums
    from spadot_amd.correlogram import corr_sums
    from spadot_amd.moran import centre_spread, columns
    xy, X, _ = cg.problem("sized513_7")
    V = (X * 2.0 + 0.5).astype(np.float32)
    r2 = np.array([3.0 ** 2])
    src, dst = ref.pair_graph(xy, r2[0])
    cols = columns([_dev(V)])
    centre = centre_spread(cols)[1]
    P, seed = 4, 11
    Na, _ = autocorr_sums([(_dev(src).to(torch.int32), _dev(dst).to(torch.int32))], cols, cols.values, centre, P, seed=seed)
    W, S2c, N, Q, Z = corr_sums([_dev(xy)], cols, centre=centre, radii_sq=[r2], n_perms=P, seed=seed, images=True)
    assert W[0][0] == src.shape[0] and N[0].shape == (3, 1 + P, 1)
    AN = ref.all_sums(xy, Z[0], r2, P, seed, 0)[4]
    _close(N[0][:, :, 0], Na[0], AN[:, :, 0], 513, "N against autocorr_sums")
    assert np.abs(N[0][:, 1:, 0] - N[0][:, :1, 0]).min() > 0                        # the permutations do move the values


def test_the_labelings_of_two_calls_are_those_of_one():
    whole = _sums(["sized257_7", "sized255_16"], n_perms=5)
    head = _sums(["sized257_7", "sized255_16"], n_perms=2)
    tail = _sums(["sized257_7", "sized255_16"], n_perms=3, first=2, observed=False)
    for t in range(2):
        for k in (2, 3):
            np.testing.assert_array_equal(np.concatenate([head[k][t], tail[k][t]], axis=1), whole[k][t])
        np.testing.assert_array_equal(tail[0][t], whole[0][t])
        np.testing.assert_array_equal(tail[1][t], whole[1][t])


# ------------------------------------------------------------------------------------------------------------ invariances
def test_culling_skips_tiles_and_changes_no_bit():
    on = _sums(["sparse"], n_perms=1, skipped=True)
    off = _sums(["sparse"], n_perms=1, cull=False, skipped=True)
    assert on[4] >= 1 and off[4] == 0, (on[4], off[4])
    print(f"culled {on[4]} of 25 (query block, tile) pairs")
    for k in range(4):
        np.testing.assert_array_equal(on[k][0], off[k][0])
    want = cg.want("sparse")
    np.testing.assert_array_equal(on[0][0], want[0])
    np.testing.assert_array_equal(on[1][0], want[1])
    _close(on[2][0][:, :1], want[2], want[4], 1100, "N of the sparse set")
    _close(on[3][0][:, :1], want[3], want[5], 1100, "Q of the sparse set")


def test_a_gene_alone_among_others_and_under_the_wider_chunk():
    from spadot_amd.correlogram import corr_sums
    xy, X, r2 = cg.sparse()
    coords = [_dev(xy)]
    full = corr_sums(coords, Z=[_dev(X)], radii_sq=[r2], n_perms=2, seed=9)
    assert full[2][0].shape == (17, 3, 5)
    for ng in (1, 3):
        part = corr_sums(coords, Z=[_dev(X[:, 5:5 + ng])], radii_sq=[r2], n_perms=2, seed=9)
        for k in (2, 3):
            np.testing.assert_array_equal(part[k][0], full[k][0][5:5 + ng])
        np.testing.assert_array_equal(part[0][0], full[0][0])
    four = corr_sums(coords, Z=[_dev(X)], radii_sq=[r2], n_perms=2, seed=9, cs=4)     # the default is 2
    for k in range(4):
        np.testing.assert_array_equal(four[k][0], full[k][0])


def test_four_genes_a_workgroup_give_the_bits_of_two():
    """cs = 4 against cs = 2 (the default) where the wider kernel is at its limits: 16 bands (159 744 bytes of LDS, the sums of the
    waves fill the tile's 4 KiB) and 17 genes (the last chunk holds one gene and three padded columns), in one call with the sparse
    set; then over a split of the labelings, and against the restatement."""
    from spadot_amd import stage_ops as ops
    from spadot_amd.correlogram import corr_sums
    assert ops.CORR_CS == 2
    xa, _, ra = cg.problem("sized255_16")
    xb, Xb, rb = cg.sparse()
    Xa = cg.centred(Xb[:255])
    coords, Z, r2 = [_dev(xa), _dev(xb)], [_dev(Xa), _dev(Xb)], [ra, rb]
    two = corr_sums(coords, Z=Z, radii_sq=r2, n_perms=3, seed=4, cs=2)
    four = corr_sums(coords, Z=Z, radii_sq=r2, n_perms=3, seed=4, cs=4)
    head = corr_sums(coords, Z=Z, radii_sq=r2, n_perms=1, seed=4, cs=4)
    tail = corr_sums(coords, Z=Z, radii_sq=r2, n_perms=2, seed=4, first=1, observed=False, cs=4)
    assert four[2][0].shape == (17, 4, 16) and four[2][1].shape == (17, 4, 5)
    for t in range(2):
        for k in range(4):
            np.testing.assert_array_equal(four[k][t], two[k][t])
        for k in (2, 3):
            np.testing.assert_array_equal(np.concatenate([head[k][t], tail[k][t]], axis=1), two[k][t])
        np.testing.assert_array_equal(tail[0][t], two[0][t])
        np.testing.assert_array_equal(tail[1][t], two[1][t])
    for t, (xy, X, r) in enumerate(((xa, Xa, ra), (xb, Xb, rb))):
        W, S2c, wN, wQ, AN, AQ = ref.all_sums(xy, X, r, 3, 4, t)
        np.testing.assert_array_equal(four[0][t], W)
        np.testing.assert_array_equal(four[1][t], S2c)
        _close(four[2][t], wN, AN, xy.shape[0], f"N of time point {t} with cs = 4")
        _close(four[3][t], wQ, AQ, xy.shape[0], f"Q of time point {t} with cs = 4")


def test_a_time_point_alone_in_a_batch_and_run_twice():
    names = ["sized257_7", "sized513_1", "sized255_16"]
    batch = _sums(names, n_perms=2)
    again = _sums(names, n_perms=2)
    for k in range(4):
        for t in range(3):
            np.testing.assert_array_equal(batch[k][t], again[k][t])
    for t, name in enumerate(names):
        alone = _sums([name], n_perms=2, graph_ids=[t])
        for k in range(4):
            np.testing.assert_array_equal(alone[k][0], batch[k][t])


def test_a_run_split_over_a_small_scratch_budget_has_the_bits_of_one_launch(monkeypatch):
    from spadot_amd import correlogram
    names = ["sized513_7", "sized255_16"]
    whole = _sums(names, n_perms=4, skipped=True)
    per = 2 * 4 * 3 * 16                                                            # the partials of a labeling: 4 blocks, 3 genes
    monkeypatch.setattr(correlogram, "SCRATCH_DOUBLES", 4 * 4 + 2 * per)              # boxes and two labelings a launch: three launches
    split = _sums(names, n_perms=4, skipped=True)
    for k in range(4):
        for t in range(2):
            np.testing.assert_array_equal(split[k][t], whole[k][t])
    assert split[4] == whole[4]
    with pytest.raises(ValueError, match="out is taken only by a call that is one launch"):
        _sums(names, n_perms=4, out=())
    monkeypatch.setattr(correlogram, "SCRATCH_DOUBLES", 4 * 4 + per - 1)             # not even one labeling fits
    with pytest.raises(ValueError, match="one labeling alone needs 400 doubles of scratch"):
        _sums(names, n_perms=4)


def test_the_outputs_are_written_completely():
    import torch
    names = ["sized2_1", "sized257_7"]
    out = (torch.full((2, 7), -77, dtype=torch.int64, device=DEV), torch.full((2, 7), -77, dtype=torch.int64, device=DEV),
           torch.full((2, 3, 2, 7), -77.0, dtype=torch.float64, device=DEV), torch.full((2, 3, 2, 7), -77.0, dtype=torch.float64, device=DEV))
    got = _sums(names, n_perms=1, out=out)
    fresh = _sums(names, n_perms=1)
    for k in range(4):
        assert not bool((out[k] == -77).any())
        assert bool((out[k][0][..., 1:] == 0).all())                                  # the bands a time point does not have
        for t in range(2):
            np.testing.assert_array_equal(got[k][t], fresh[k][t])


# ------------------------------------------------------------------------------------------------------------------ stage
def test_the_stage_on_the_planted_lattice(tmp_path):
    import pandas as pd
    from spadot_amd.correlogram import SUMMARY_COLUMNS, TABLE_COLUMNS, correlogram, correlogram_stage
    data = cg.stage_counts(str(tmp_path / "counts.npz"))
    radii = ",".join(str(r) for r in cg.PLANTED_RADII)
    genes = "smooth,noise,checker,flat"
    out = str(tmp_path / "out")
    res = correlogram_stage(argparse.Namespace(data=data, output_dir=out, prefix="p_", genes=genes, radii=radii, device=DEV))
    for name in ("p_correlogram_P0.csv", "p_correlogram_summary.csv", "p_correlogram.npz"):
        assert os.path.exists(os.path.join(out, name)), name
    table = pd.read_csv(os.path.join(out, "p_correlogram_P0.csv"))
    summary = pd.read_csv(os.path.join(out, "p_correlogram_summary.csv"))
    assert list(table.columns) == list(TABLE_COLUMNS) and list(summary.columns) == list(SUMMARY_COLUMNS)
    assert len(table) == 4 * 9 and summary["gene"].tolist() == ["smooth", "noise", "checker", "flat"]
    assert table["r_hi"].tolist()[:9] == list(cg.PLANTED_RADII) and table["r_lo"].tolist()[:9] == [0.0] + list(cg.PLANTED_RADII[:-1])
    np.testing.assert_array_equal(table["pairs"].to_numpy()[:9], cg.want("planted")[0])
    r = res["results"]["P0"]
    assert r.degenerate.tolist() == [False, False, False, True]
    # the ranges of the CPU test: the smooth gene reaches 8 and stops inside the ladder, noise and checkerboard reach nowhere
    assert summary["range"].tolist()[:3] == [8.0, 0.0, 0.0] and np.isnan(summary["range"][3]) and summary["open"].tolist() == [0] * 4
    assert r.I[2, 0] < -0.5 and r.z_norm[2, 0] < -20 and np.all(r.z_norm[0, :5] > 20) and np.all(r.z_norm[0, 6:] < -5)
    assert np.all(np.isnan(r.z_sim)) and np.all(np.isnan(r.padj) == r.degenerate[:, None])
    z = np.load(os.path.join(out, "p_correlogram.npz"))
    assert z["genes"].tolist() == genes.split(",") and z["P0_I"].shape == (4, 9) and z["P0_W"].dtype == np.int64
    # with permutations the simulated columns are there, for every gene but the flat one
    out5 = str(tmp_path / "out5")
    res5 = correlogram_stage(argparse.Namespace(data=data, output_dir=out5, genes=genes, radii=radii, n_perms=5, seed=2, device=DEV))
    t5 = pd.read_csv(os.path.join(out5, "correlogram_P0.csv"))
    assert not t5["z_sim"][:27].isna().any() and not t5["p_sim"][:27].isna().any() and t5["z_sim"][27:].isna().all()
    assert set(np.round(t5["p_sim"][:27] * 6).astype(int)) <= set(range(1, 7))
    np.testing.assert_array_equal(res5["results"]["P0"].N[:, 0], r.N[:, 0])          # the observed labeling is that of the first run
    # without --genes and --radii: the union of the --top genes by Moran's I of autocorr, on --bins default bands
    from spadot_amd.correlogram import default_bands
    outt = str(tmp_path / "top")
    rest = correlogram_stage(argparse.Namespace(data=data, output_dir=outt, top=2, bins=5, device=DEV))
    tt = pd.read_csv(os.path.join(outt, "correlogram_P0.csv"))
    rt = rest["results"]["P0"]
    assert rest["genes"].size == 2 and 0 in rest["genes"].tolist() and len(tt) == 2 * 5          # `smooth` leads; two genes in all
    assert np.all(np.diff(rest["genes"]) > 0) and tt["gene"].tolist()[:5] == ["smooth"] * 5
    np.testing.assert_array_equal(rt.radii, default_bands(np.load(data)["spatial"], 5))
    np.testing.assert_array_equal(tt["r_hi"].to_numpy()[:5], rt.radii)
    assert rt.I[0, 0] > 0.8 and rt.range[0] > 0 and os.path.exists(os.path.join(outt, "correlogram_summary.csv"))
    # an empty band is NaN for every gene: no two spots of the lattice lie within 0.3
    import torch
    xy, V = cg.planted()
    e = correlogram([_dev(xy)], [_dev(np.concatenate([V, np.ones((1024, 1))], axis=1), torch.float32)], radii=[0.3, 1.3])[0]
    assert e.W.tolist()[0] == 0 and np.all(np.isnan(e.padj[:, 0])) and np.all(np.isnan(e.I[:, 0]))
    np.testing.assert_array_equal(np.isnan(e.padj[:, 1]), [False, False, False, True])


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch():
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.correlogram import corr_sums
    xy, X, r2 = cg.problem("sized255_16")
    coords, Z = [_dev(xy)], [_dev(X)]
    with pytest.raises(ValueError, match="17 distance bands"):
        corr_sums(coords, Z=Z, radii=[np.arange(1.0, 18.0)])
    with pytest.raises(ValueError, match="strictly increasing"):
        corr_sums(coords, Z=Z, radii=[[1.0, 3.0, 2.0]])
    with pytest.raises(ValueError, match="exactly one of radii and radii_sq"):
        corr_sums(coords, Z=Z)
    with pytest.raises(RuntimeError, match="MI355X only"):
        corr_sums([torch.as_tensor(np.array(xy))], Z=Z, radii=[[1.0]])
    with pytest.raises(RuntimeError, match="MI355X only"):
        corr_sums(coords, Z=[torch.as_tensor(np.array(X))], radii=[[1.0]])
    V = _dev(X, torch.float32)
    for genes in ([0, 3], [-1]):
        with pytest.raises(ValueError, match="must lie in 0 .. 2"):
            corr_sums(coords, [V], genes=genes, radii=[[1.0]])
    with pytest.raises(ValueError, match="cs in"):
        corr_sums(coords, Z=Z, radii=[[1.0]], cs=3)
    # the launch wrapper itself: an order that is no permutation, a descriptor that does not add up, a short scratch buffer
    img = torch.zeros((256, 16), dtype=torch.float64, device=DEV)
    img[:255, :3] = Z[0]
    desc = np.array([[0, 255, 16, 0, 0, 0]])
    order = torch.arange(255, dtype=torch.int32, device=DEV)
    twice = order.clone()
    twice[7] = 8
    for bad in (twice, order + 1):
        with pytest.raises(ValueError, match="is not a permutation of 0 .. 254"):
            ops.corr_sums(_dev(xy), bad, img, desc, [r2], 3, True, 0, 0)
    with pytest.raises(ValueError, match="inconsistent descriptor"):
        ops.corr_sums(_dev(xy), order, img, np.array([[0, 255, 16, 0, 0, 1]]), [r2], 3, True, 0, 0)
    with pytest.raises(ValueError, match="Z holds 256 rows"):
        ops.corr_sums(_dev(xy), order, img, np.array([[0, 255, 16, 0, 4, 0]]), [r2], 3, True, 0, 0)
    with pytest.raises(ValueError, match="scratch must be"):
        ops.corr_sums(_dev(xy), order, img, desc, [r2], 3, True, 0, 0, scratch=torch.zeros(10, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="65535"):
        ops.corr_sums(_dev(xy), order, img, desc, [r2], 3, True, 0, 70000)
    # the library refuses on its own what the wrapper would: called past the check, nothing is launched
    padded = np.concatenate([[1.0, 2.0, 3.0], np.full(13, -1.0)])[None, :]              # the padding of the pair-counting stages
    with pytest.raises(RuntimeError, match="spadot_corr_sums failed with -22"):
        ops.corr_launch(_dev(xy), order, img, (np.array([[0, 255, 3, 0, 0, 0]]), padded, 3, 1, 0, 0), 3)
    unordered = np.concatenate([[1.0, 3.0, 2.0], np.full(13, np.inf)])[None, :]
    with pytest.raises(ValueError, match="spadot_corr_sums: outside its limits"):
        ops.corr_launch(_dev(xy), order, img, (np.array([[0, 255, 3, 0, 0, 0]]), unordered, 3, 1, 0, 0), 3)
    got = ops.corr_sums(_dev(xy), order, img, desc, [r2], 3, True, 0, 0)                # and a well-formed call goes through
    np.testing.assert_array_equal(got[0].cpu().numpy()[0], cg.want("sized255_16")[0])
