"""CPU: the numpy restatement of local Moran's I (tests/hotspots_ref.py) against its own conditions on the planted grid, the
conditional draw, the host statistics of spadot_amd.hotspots against the restatement's, and the command line."""
import argparse

import numpy as np
import pytest

import autocorr_cases as ac
import autocorr_ref as aref
import hotspots_cases as cases
import hotspots_ref as ref
import nhood_cases as nc
from nhood_ref import perm

U = 2.0 ** -53


def _planted_stats():
    src, dst, V = ac.planted_genes()
    lag, ge, le = cases.planted_counts()
    c = ac.centres(V)
    has = np.bincount(src, minlength=400) > 0
    return src, dst, V, c, lag, ge, le, [ref.stats(lag[g], ge[g], le[g], V[:, g], c[g], 400, 2400, cases.PLANTED_PERMS, has)
                                         for g in range(6)]


def test_the_local_statistics_add_up_to_the_global_one():
    src, dst, V, c, lag, ge, le, st = _planted_stats()
    assert (src.shape[0], V.shape) == (2400, (400, 6))
    for g, name in enumerate(ac.PLANTED_GENES):
        z = V[:, g].astype(np.float64) - c[g]
        m2 = float((z * z).sum())
        N, _, A = aref.edge_sums(src, dst, V[:, g], c[g])
        err = abs(float(st[g]["I"].sum()) - 400 * N / m2)
        print(f"{name}: |sum I_i - n N / m2| = {err:.3e}, bound {400 / m2 * 4 * 2402 * U * A:.3e}")
        assert err <= 400 / m2 * 4.0 * (2400 + 2) * U * A                            # the bound on N, scaled as I is


def test_structured_genes_light_up_and_noise_does_not():
    *_, lag, ge, le, st = _planted_stats()
    share = [float((s["p_sim"] <= 0.05).mean()) for s in st]
    ties = [(ge[g] + le[g] > cases.PLANTED_PERMS).sum() for g in range(6)]
    print("share of spots with p_sim <= 0.05:", dict(zip(ac.PLANTED_GENES, share)), "ties:", ties)
    for g in (0, 1):                                                                 # gradient and marker
        sig, q = st[g]["p_sim"] <= 0.05, st[g]["quadrant"]
        same, outlier = int((sig & ((q == 1) | (q == 3))).sum()), int((sig & ((q == 2) | (q == 4))).sum())
        print(ac.PLANTED_GENES[g], "HH + LL", same, "outliers", outlier)
        assert share[g] >= 0.25 and same >= 3 * outlier
    for g in (2, 3):                                                                 # the noise genes: the folded p doubles 0.05
        assert 0.05 <= share[g] <= 0.16
    for g in (4, 5):                                                                 # checkerboard and single nonzero: ties
        assert ties[g] >= 390


def test_the_conditional_map_is_a_bijection_that_fixes_the_spot():
    for n, p, i in ((37, 0, 0), (37, 3, 36), (37, 9, 18), (400, 1, 137), (2, 0, 1), (1, 0, 0), (300, 7, 299)):
        pi = perm(n, nc.SEED, 2, p)
        m = ref.conditional_map(pi, i)
        assert m[i] == i and sorted(m.tolist()) == list(range(n))
        j = int(ref.inverse(pi)[i])
        assert m[j] == pi[i] and np.array_equal(np.delete(m, [i, j]), np.delete(pi, [i, j]))


def test_the_replacement_branch_is_exercised_by_the_n37_graph():
    src, dst, V = ac.edge_call()[2]
    hits = ref.jstar_hits(src, dst, 37, 10, nc.SEED, 2)
    print("(spot, permutation) pairs with j* among the neighbours:", hits)
    assert hits >= 1
    c = ac.centres(V)
    a = ref.local_counts_genes(src, dst, 37, V, c, 10, nc.SEED, 2)
    b = ref.local_counts_genes(src, dst, 37, V, c, 10, nc.SEED, 2, replace=False)
    np.testing.assert_array_equal(a[0], b[0])                                        # the observed sums do not know of it
    assert not np.array_equal(a[1], b[1]) or not np.array_equal(a[2], b[2])
    i, p = 0, 0                                                                      # and the sum of one spot from the composed map
    pi = perm(37, nc.SEED, 2, p)
    rowptr, col = ref.csr(src, dst, 37)
    for i in range(37):
        x = V[:, 1].astype(np.float64)[ref.conditional_map(pi, i)]
        lag = 0.0
        for j in col[rowptr[i]:rowptr[i + 1]]:
            lag = lag + (x[j] - c[1])
        assert lag == ref.lag_rows(rowptr, col, V[:, 1].astype(np.float64)[pi], c[1], ref.inverse(pi))[i]


def test_local_stats_against_the_restatement():
    from spadot_amd.hotspots import local_stats
    src, dst, V = cases.edge_call()[3]                                               # n = 300, three spots without out-edges
    n, E, P = 300, src.shape[0], 10
    V = V.copy()
    V[5, 1] = np.float32(ac.centres(V)[1])                                           # (nearly) z = 0 is not z = 0:
    c = ac.centres(V)
    c[2] = 0.0                                                                        # a centre of 0: z = 0 wherever nothing is stored
    lag, ge, le = ref.local_counts_genes(src, dst, n, V, c, P, nc.SEED, 3)
    has = np.bincount(src, minlength=n) > 0
    assert (~has).sum() == 3
    z = V.astype(np.float64).T - c[:, None]
    m2, sumsq = (z * z).sum(1), (V.astype(np.float64) ** 2).sum(0)
    bad = np.array([aref.is_degenerate(n, E, m2[g], sumsq[g]) for g in range(4)])
    assert bad.tolist() == [False, False, False, True]                               # gene 3 is the constant one
    got = local_stats(lag, ge, le, z, m2, n, P, has, bad)
    assert got["quadrant"].dtype == np.int8
    for g in range(4):
        w = ref.stats(lag[g], ge[g], le[g], V[:, g], c[g], n, E, P, has)
        np.testing.assert_array_equal(got["quadrant"][g], w["quadrant"])
        np.testing.assert_array_equal(got["p_sim"][g], w["p_sim"])
        # m2 is a sum of n terms >= 0 taken in two orders (each within n 2^-53 of exact), then two products and a quotient
        np.testing.assert_allclose(got["I"][g], w["I"], rtol=2 * (n + 4) * U, atol=0)
        np.testing.assert_allclose(got["padj"][g], w["padj"], rtol=1e-12)
        np.testing.assert_array_equal(np.isnan(got["padj"][g]), np.isnan(w["padj"]))
    assert np.isnan(got["I"][3]).all() and np.isnan(got["p_sim"][3]).all() and not got["quadrant"][3].any()
    lone = np.flatnonzero(~has)
    assert not got["I"][:3, lone].any() and np.isnan(got["p_sim"][:3, lone]).all() and np.isnan(got["padj"][:3, lone]).all()
    assert not got["quadrant"][:, lone].any()
    zero = (z[2] == 0) & has                                                         # z = 0: quadrant 0, larger = smaller = P, p = 1
    assert zero.sum() > 100 and not got["quadrant"][2, zero].any() and np.all(got["p_sim"][2, zero] == 1.0)
    flat = (lag[0] == 0) & has & (z[0] != 0)
    assert not got["quadrant"][0, flat].any()
    for g in range(3):                                                               # the BH family: the spots with a neighbour
        from nhood_ref import bh
        np.testing.assert_allclose(got["padj"][g, has], bh(got["p_sim"][g, has]), rtol=1e-12)
    pos = z[1] > 0
    np.testing.assert_array_equal(got["larger"][1, pos], ge[1, pos])
    np.testing.assert_array_equal(got["larger"][1, ~pos & (z[1] < 0)], le[1, ~pos & (z[1] < 0)])
    np.testing.assert_array_equal(got["smaller"][1, pos], le[1, pos])
    with pytest.raises(ValueError, match="local_stats takes"):
        local_stats(lag, ge, le, z, m2, n, 0, has, bad)
    with pytest.raises(ValueError, match="local_stats takes"):
        local_stats(lag, ge, le, z[:, :-1], m2, n, P, has, bad)


def test_the_lds_formula_and_the_scratch_bytes():
    from spadot_amd import stage_ops as ops
    assert ops.local_lds_bytes(10000) == 256 + 160000 <= ops.LOCAL_LDS_BYTES < ops.local_lds_bytes(10225)
    assert ops.local_lds_bytes(10000, gs=2) == 256 + 80000
    desc = np.array([[0, 37, 0, 0, 0, 0, 0, 0], [0, 300, 0, 37, 1, 38, 0, 0]], dtype=np.int64)
    assert ops.local_scratch_bytes(desc, 5, 23) == 2 * 1 * 2 * 16 * 4 * 300                          # T x chunks x groups x state
    assert ops.local_scratch_bytes(desc, 5, 23, perm_chunk=7, gs=2) == 2 * 4 * 3 * 16 * 2 * 300
    assert ops.local_scratch_bytes(desc, 5, 23, lds_limit=0) == 2 * 2 * (16 * 4 * 300 + 4 * 1200)  # and the image of the largest


def test_command_line_parsing_and_refusals(tmp_path):
    from spadot_amd.cli import build_parser, main
    from spadot_amd.hotspots import hotspots, read_genes
    a = build_parser().parse_args(["hotspots", "-i", "counts.npz"])
    assert (a.cmd_choice, a.k, a.n_perms, a.seed, a.top, a.alpha, a.fdr, a.genes, a.domains, a.prefix, a.device) == (
        "hotspots", 6, 999, 0, 50, 0.05, False, None, None, "", "cuda:0")
    a = build_parser().parse_args(["hotspots", "-i", "c.npz", "--genes", "a,b", "--fdr", "--alpha", "0.1", "--domains", "d.csv",
                                   "--n_perms", "99", "--top", "8", "--k", "4", "--seed", "7", "-o", "out", "--prefix", "p_"])
    assert (a.genes, a.fdr, a.alpha, a.domains, a.n_perms, a.top, a.k, a.seed, a.output_dir, a.prefix) == (
        "a,b", True, 0.1, "d.csv", 99, 8, 4, 7, "out", "p_")
    with pytest.raises(SystemExit) as e:
        main(["hotspots", "-i", str(tmp_path / "missing.npz")])
    assert e.value.code == 2
    path = ac.stage_counts(str(tmp_path / "counts.npz"))
    with pytest.raises(SystemExit) as e:
        main(["hotspots", "-i", path, "--domains", str(tmp_path / "missing.csv")])
    assert e.value.code == 2
    names = [f"g{g:02d}" for g in range(40)]
    assert read_genes("g03, g12,g03", names).tolist() == [3, 12, 3]
    listing = tmp_path / "genes.txt"
    listing.write_text("g07\n\n g01 \n")
    assert read_genes(str(listing), names).tolist() == [7, 1]
    with pytest.raises(ValueError, match="does not hold: nope, g40"):
        read_genes("g01,nope,g40", names)
    with pytest.raises(ValueError, match="names no gene"):
        read_genes(" , ", names)

    def ns(**kw):
        base = dict(data=path, output_dir=str(tmp_path), prefix="", k=6, n_perms=99, seed=0, top=8, genes=None, alpha=0.05,
                    fdr=False, domains=None, device="cuda:0")
        base.update(kw)
        return argparse.Namespace(**base)

    for kw in (dict(n_perms=0), dict(k=0), dict(top=0), dict(alpha=0.0), dict(alpha=1.5)):
        with pytest.raises(ValueError, match="the hotspots stage takes"):
            hotspots(ns(**kw))
    with pytest.raises(RuntimeError, match="MI355X only"):
        hotspots(ns(device="cpu"))
    with pytest.raises(ValueError, match="does not hold"):
        hotspots(ns(genes="g01,unknown"))


def test_local_lag_refuses_host_arrays_without_a_gpu():
    from spadot_amd import stage_ops as ops
    import torch
    t = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.local_lag(t, t, t.long(), t, t.float(), t.double(), t, np.zeros((1, 8), np.int64), 0, 1)
