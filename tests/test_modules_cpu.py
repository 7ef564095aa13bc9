"""CPU: the numpy restatement of the bivariate Moran's I between genes (tests/modules_ref.py) against its own conditions on the
planted grid and on the stage's planted counts, the rounding margin that the p-value tests on the device rely on, the host parts
of spadot_amd.modules (modules, overlap, tables) on hand-made input, and the command line."""
import argparse

import numpy as np
import pytest

import autocorr_cases as ac
import autocorr_ref as aref
import modules_cases as cases
import modules_ref as ref
from hotspots_ref import csr, lag_rows


@pytest.fixture(scope="module")
def planted():
    src, dst, V = ac.planted_genes()
    c = ac.centres(V)
    M, A = ref.cross_sums(src, dst, V, c, 0, cases.SEED, 0)
    m2, sumsq = ref.spread(V, c)
    return src, dst, V, c, M, ref.stats(M, 400, 2400, m2, sumsq)


def test_R_is_symmetric_and_its_diagonal_is_morans_I(planted):
    src, dst, V, c, M, st = planted
    assert (src.shape[0], V.shape) == (2400, (400, 6)) and not st["degenerate"].any()
    np.testing.assert_array_equal(st["R"], st["R"].T)
    for g in range(6):
        m2, _ = aref.spread(V[:, g], c[g])
        I = 400 * aref.edge_sums(src, dst, V[:, g], c[g])[0] / (2400 * m2)
        assert abs(st["R"][g, g] - I) <= 1e-12, (g, st["R"][g, g], I)


def test_R_does_not_change_when_every_edge_is_also_added_reversed(planted):
    src, dst, V, c, M, st = planted
    both = ref.cross_sums(np.concatenate([src, dst]), np.concatenate([dst, src]), V, c, 0, cases.SEED, 0)[0]
    m2, sumsq = ref.spread(V, c)
    R2 = ref.stats(both, 400, 4800, m2, sumsq)["R"]
    np.testing.assert_allclose(R2, st["R"], rtol=0, atol=1e-13)
    assert not np.allclose(M[0], M[0].T, rtol=0, atol=1e-6)                          # M itself is not symmetric: B is the point


def test_the_lag_is_the_dense_product_and_the_lag_of_the_local_statistic(planted):
    src, dst, V, c, *_ = planted
    Y = ref.lag(src, dst, V, c)
    np.testing.assert_allclose(Y, ref.lag_dense(src, dst, ref.centred(V, c)), rtol=0, atol=16 * 2.0 ** -53 * np.abs(V).max() * 6)
    rowptr, col = csr(src, dst, 400)
    for g in range(6):
        np.testing.assert_array_equal(Y[:, g], lag_rows(rowptr, col, V[:, g].astype(np.float64), c[g]))


def test_the_permuted_gene_moves_against_the_fixed_lag():
    src, dst, V = cases.tile_case(17, 3)
    c = ac.centres(V)
    M, _ = ref.cross_sums(src, dst, V, c, 2, 9, 4, first=5)
    Z, Y = ref.centred(V, c), ref.lag(src, dst, V, c)
    from nhood_ref import perm
    for l, m in enumerate([np.arange(17), perm(17, 9, 4, 5), perm(17, 9, 4, 6)]):
        for g in range(3):
            for h in range(3):
                assert abs(M[l, g, h] - sum(Z[m[i], g] * Y[i, h] for i in range(17))) <= ref.bound_M(17, np.abs(Z[m, g] * Y[:, h]).sum())
    assert ref.cross_sums(src, dst, V, c, 2, 9, 4, first=5, observed=False)[0].shape == (2, 3, 3)


@pytest.mark.parametrize("top", (8, 12))
def test_the_planted_stage_data_meets_its_three_conditions(top):
    from spadot_amd.modules import gene_modules
    sel, parts = cases.stage_restatement(top)
    assert set(sel.tolist()) <= set(range(20)) and np.sum(sel < 10) >= 8
    for tp, M, A, st, m2 in parts:
        assert not st["degenerate"].any()
        labels = gene_modules(st["R"], ~st["degenerate"], cases.MIN_SIM, 2)
        bad, same, (lo, hi) = cases.broken_conditions(sel, cases.STAGE_K[tp], st["R"], st["p_sim"], labels, cases.STAGE_PERMS)
        print(f"top {top}, {tp}: genes {sel.tolist()}, modules {labels.tolist()}, smallest R of a same-domain pair {same:.3f}, R of "
              f"markers of different domains {lo:.3f} .. {hi:.3f}")
        assert not bad, "\n".join(bad)


def test_the_rounding_margin_of_the_p_values_stays_within_its_cap():
    close_all = total_all = 0
    for key, P, seed in cases.PVALUE_CASES:
        for (src, dst, V), (M, A) in zip(cases.problems(key), cases.want(key, P, seed)):
            close, total = ref.margin_share(M, A, V.shape[0])
            special = cases.single_or_degenerate(V, src.shape[0])
            iu = np.triu_indices(V.shape[1])
            involved = special[iu[0]] | special[iu[1]]
            print(f"{key}: n = {V.shape[0]}, {V.shape[1]} genes, {int(close.sum())} of {total} comparisons inside the bound")
            assert not close[:, ~involved].any()                                     # only a degenerate or single-nonzero gene ties
            close_all, total_all = close_all + int(close.sum()), total_all + total
    print(f"share inside the rounding bound: {close_all} / {total_all} = {close_all / total_all:.4f}")
    assert close_all <= 0.01 * total_all


def test_stats_leave_degenerate_genes_out_of_the_family():
    src, dst, V = ac.edge_call()[3]                                                  # gene 3 is constant
    c = ac.centres(V)
    M, _ = ref.cross_sums(src, dst, V, c, 19, cases.SEED, 3)
    m2, sumsq = ref.spread(V, c)
    st = ref.stats(M, 300, src.shape[0], m2, sumsq)
    assert st["degenerate"].tolist() == [False, False, False, True]
    for k in ("R", "z_sim", "p_sim", "padj"):
        assert np.isnan(st[k][3]).all() and np.isnan(st[k][:, 3]).all() and not np.isnan(st[k][:3, :3][np.triu_indices(3, 1)]).any()
    from nhood_ref import bh
    iu = np.triu_indices(3, 1)
    np.testing.assert_array_equal(st["padj"][:3, :3][iu], bh(st["p_sim"][:3, :3][iu]))
    assert np.isnan(np.diagonal(st["padj"])).all()


def _cross_result(R, ok=None):
    from spadot_amd.modules import CrossResult
    R = np.asarray(R, dtype=np.float64)
    G = R.shape[0]
    bad = np.zeros(G, bool) if ok is None else ~np.asarray(ok, dtype=bool)
    return CrossResult(R, np.zeros((G, G), np.int64), np.zeros((G, G)), np.ones((G, G)), np.zeros(G), np.ones(G), 1, 1, 1, bad,
                       np.arange(G), None)


def test_cross_result_against_the_restatement():
    from spadot_amd.modules import CrossResult
    src, dst, V = ac.edge_call()[3]
    c = ac.centres(V)
    P, n, E = 19, 300, src.shape[0]
    M, _ = ref.cross_sums(src, dst, V, c, P, cases.SEED, 3)
    m2, sumsq = ref.spread(V, c)
    st = ref.stats(M, n, E, m2, sumsq)
    B = ref.symmetrised(M)
    r = CrossResult(B[0], ref.counts(M), B[1:].sum(0), (B[1:] ** 2).sum(0), c, m2, n, E, P, st["degenerate"], np.arange(4), None)
    np.testing.assert_allclose(r.R, st["R"], rtol=1e-14)
    np.testing.assert_array_equal(r.p_sim, st["p_sim"])
    np.testing.assert_allclose(r.padj, st["padj"], rtol=1e-12)
    np.testing.assert_allclose(r.z_sim, st["z_sim"], rtol=1e-8)                      # the sd from the two sums, not the deviations
    np.testing.assert_array_equal(r.I, np.diagonal(r.R))
    np.testing.assert_array_equal(r.R, r.R.T)


def test_gene_modules_on_hand_made_R():
    from spadot_amd.modules import gene_modules
    R = np.full((7, 7), -0.05)
    np.fill_diagonal(R, 0.6)
    for a, b, v in ((0, 3, 0.5), (3, 5, 0.4), (0, 5, 0.3), (1, 2, 0.15), (4, 6, 0.149)):
        R[a, b] = R[b, a] = v
    ok = np.ones(7, bool)
    assert gene_modules(R, ok, 0.15, 2).tolist() == [0, 1, 1, 0, -1, 0, -1]          # a tie with the cut joins, just below does not
    assert gene_modules(R, ok, 0.15, 3).tolist() == [0, -1, -1, 0, -1, 0, -1]        # min_genes, and the numbering closes the gap
    assert gene_modules(R, ok, 0.15, 1).tolist() == [0, 1, 1, 0, 2, 0, 3]            # numbered by the smallest gene
    assert gene_modules(R, ok, 0.45, 2).tolist() == [0, -1, -1, 0, -1, -1, -1]
    assert gene_modules(R, ok, -1.0, 2).tolist() == [0] * 7
    R2 = R.copy()
    R2[3, 3] = -0.1                                                                  # no positive autocorrelation: outside
    assert gene_modules(R2, ok, 0.15, 2).tolist() == [0, 1, 1, -1, -1, 0, -1]
    off = ok.copy()
    off[0] = False
    R3 = R.copy()
    R3[0], R3[:, 0] = np.nan, np.nan                                                 # a degenerate gene: NaN row and column
    assert gene_modules(R3, off, 0.15, 2).tolist() == [-1, 0, 0, 1, -1, 1, -1]
    assert gene_modules(R[:1, :1], [True], 0.15, 2).tolist() == [-1] and gene_modules(R[:1, :1], [True], 0.15, 1).tolist() == [0]
    assert gene_modules(R, np.zeros(7, bool)).tolist() == [-1] * 7
    tie = np.array([[1.0, 0.3, 0.3], [0.3, 1.0, 0.3], [0.3, 0.3, 1.0]])              # equal distances: one module at 0.3
    assert gene_modules(tie, [True] * 3, 0.3, 2).tolist() == [0, 0, 0] and gene_modules(tie, [True] * 3, 0.31, 2).tolist() == [-1] * 3
    with pytest.raises(ValueError, match="gene_modules takes"):
        gene_modules(R, ok[:-1])
    with pytest.raises(ValueError, match="gene_modules takes"):
        gene_modules(R, ok, 0.15, 0)
    assert gene_modules(R3, ok, 0.15, 2).tolist() == [-1, 0, 0, 1, -1, 1, -1]           # a NaN diagonal is not > 0 either
    R3[1, 2] = R3[2, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        gene_modules(R3, off)


def test_module_overlap_and_the_tables_on_hand_made_labels():
    from spadot_amd.modules import OVERLAP_COLUMNS, PAIR_COLUMNS, TABLE_COLUMNS, module_overlap, module_table, overlap_table, pair_table
    a, b = np.array([0, 0, 0, 1, 1, -1, -1]), np.array([1, 1, 0, 0, -1, 0, -1])
    jac, both = module_overlap(a, b)
    np.testing.assert_array_equal(both, [[1, 2], [1, 0]])
    np.testing.assert_allclose(jac, [[1 / 5, 2 / 3], [1 / 4, 0.0]])
    np.testing.assert_allclose(jac, ref.jaccard(a, b))
    assert module_overlap([-1, -1], [0, 0])[0].shape == (0, 1)
    with pytest.raises(ValueError, match="same genes"):
        module_overlap(a, b[:-1])
    tab = overlap_table(["E10", "E12", "E14"], [a, b, a])
    assert tuple(tab.columns) == OVERLAP_COLUMNS and len(tab) == 8
    assert tab.iloc[1].tolist() == ["E10", 0, "E12", 1, 3, 2, 2, 2 / 3]
    R = np.full((4, 4), 0.1)
    np.fill_diagonal(R, 0.5)
    R[0, 1] = R[1, 0] = 0.4
    R[2, 3] = R[3, 2] = -0.3
    r = _cross_result(R)
    names = np.array(["a", "b", "c", "d"])
    labels = np.array([0, 0, 1, -1])
    mt = module_table(r, names, labels)
    assert tuple(mt.columns) == TABLE_COLUMNS and mt["gene"].tolist() == list(names) and mt["module"].tolist() == [0, 0, 1, -1]
    np.testing.assert_allclose(mt["R_own"], [0.4, 0.4, np.nan, np.nan])
    assert mt["best_other"].tolist() == [1, 1, 0, 0]
    np.testing.assert_allclose(mt["R_other"], [0.1, 0.1, 0.1, 0.1])
    pt = pair_table(r, names, labels)
    assert tuple(pt.columns) == PAIR_COLUMNS and len(pt) == 6
    assert (pt["gene_a"][0], pt["gene_b"][0], pt["same_module"][0]) == ("a", "b", 1) and (pt["gene_a"][1], pt["gene_b"][1]) == ("c", "d")
    assert pt["same_module"].tolist() == [1, 0, 0, 0, 0, 0] and np.all(np.diff(np.abs(pt["R"])) <= 0)
    assert len(pair_table(r, names, labels, 2)) == 2
    gone = _cross_result(R, ok=[True, True, False, True])
    assert len(pair_table(gone, names, labels)) == 3 and np.isnan(module_table(gone, names, labels)["I"][2])


def test_the_layout_of_the_images_and_the_runs():
    from spadot_amd import stage_ops as ops
    from spadot_amd.utils._stage_utils import labeling_runs
    assert [ops.cross_padded(g) for g in (1, 15, 16, 17, 4096)] == [16, 16, 16, 32, 4096]
    zoff, zrows = ops.cross_layout([1, 2, 37, 300, 4])
    assert zoff.tolist() == [0, 4, 8, 48, 348] and zrows == 352
    assert (cases.TILE, cases.KSTEP) == (ops.CROSS_TILE, 4)
    assert labeling_runs(23, True, 0, 8 * 25, 8 * 25 * 5) == [(True, 0, 4), (False, 4, 5), (False, 9, 5), (False, 14, 5), (False, 19, 4)]


def test_command_line_parsing_and_refusals(tmp_path):
    from spadot_amd.cli import build_parser, main
    from spadot_amd.modules import modules
    a = build_parser().parse_args(["modules", "-i", "counts.npz"])
    assert (a.cmd_choice, a.k, a.n_perms, a.seed, a.top, a.genes, a.min_sim, a.min_genes, a.alpha, a.top_pairs, a.prefix, a.device) == (
        "modules", 6, 100, 0, 100, None, 0.15, 2, 0.05, 0, "", "cuda:0")
    a = build_parser().parse_args(["modules", "-i", "c.npz", "--genes", "a,b", "--min_sim", "0.2", "--min_genes", "3", "--alpha", "0.1",
                                   "--n_perms", "99", "--top", "8", "--k", "4", "--seed", "7", "-o", "out", "--prefix", "p_",
                                   "--top_pairs", "50"])
    assert (a.genes, a.min_sim, a.min_genes, a.alpha, a.n_perms, a.top, a.k, a.seed, a.output_dir, a.prefix, a.top_pairs) == (
        "a,b", 0.2, 3, 0.1, 99, 8, 4, 7, "out", "p_", 50)
    with pytest.raises(SystemExit) as e:
        main(["modules", "-i", str(tmp_path / "missing.npz")])
    assert e.value.code == 2
    path = ac.stage_counts(str(tmp_path / "counts.npz"))

    def ns(**kw):
        base = dict(data=path, output_dir=str(tmp_path), prefix="", k=6, n_perms=99, seed=0, top=8, genes=None, min_sim=0.15,
                    min_genes=2, alpha=0.05, top_pairs=0, device="cuda:0")
        base.update(kw)
        return argparse.Namespace(**base)

    for kw in (dict(n_perms=0), dict(k=0), dict(top=0), dict(alpha=0.0), dict(min_sim=1.5), dict(min_genes=0), dict(top_pairs=-1)):
        with pytest.raises(ValueError, match="the modules stage takes"):
            modules(ns(**kw))
    with pytest.raises(RuntimeError, match="MI355X only"):
        modules(ns(device="cpu"))
    with pytest.raises(ValueError, match="does not hold"):
        modules(ns(genes="g01,unknown"))


def test_the_launches_refuse_host_arrays_without_a_gpu():
    from spadot_amd import stage_ops as ops
    import torch
    t = torch.zeros(4, dtype=torch.int32)
    desc = np.zeros((1, 9), np.int64)
    desc[0, 1] = 3
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.cross_dense(t, t, t.long(), t, t.float(), t.double(), t, desc)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.cross_sums(torch.zeros((4, 16), dtype=torch.float64), torch.zeros((4, 16), dtype=torch.float64), desc, 1, True, 0, 1)
