"""CPU: the numpy restatement of the ligand-receptor test (tests/ligrec_ref.py) held to its own conditions on planted data, the
host part of the package (ligrec_stats, read_interactions, the table, the parser) against it, and the inputs of the GPU
comparison of p-values: the cells that a rounding could flip, found from the restatement in forward and reversed summation order,
stay below the cap that tests/test_ligrec_gpu.py asserts."""
import numpy as np
import pytest

import ligrec_cases as cases
import ligrec_ref as ref


@pytest.fixture(scope="module")
def planted():
    V, lab, K, pairs = cases.planted()
    S = ref.sums(V, ref.labelings(lab, 200, cases.SEED, 0), K)
    c, sizes = ref.positive_counts(V, lab, K), np.bincount(lab, minlength=K)
    return V, lab, K, pairs, S, c, sizes


def test_planted_pair_is_found_between_its_domains_and_nowhere_else(planted):
    V, lab, K, pairs, S, c, sizes = planted
    r = ref.all_cells(S, c, sizes, pairs, 0.1)
    assert r["tested"][0].all() and sizes.min() > 0
    assert r["pvalue"][0, 0, 1] == 1 / 201 and r["padj"][0, 0, 1] < 0.05             # gene 0 in domain 0 -> gene 1 in domain 1
    assert r["pvalue"][0, 2, 3] > 0.2
    assert r["pvalue"][4, 1, 0] == 1 / 201                                           # the reversed pair, the reversed cell
    assert np.argmax(r["mean"][0]) == 0 * K + 1
    np.testing.assert_array_equal(r["mean"][0], 0.5 * (r["gene_mean"][0][:, None] + r["gene_mean"][1][None, :]))
    np.testing.assert_allclose(r["gene_mean"], np.stack([V[lab == k].astype(np.float64).mean(0) for k in range(K)], 1), rtol=1e-13)
    np.testing.assert_array_equal(r["gene_pct"], np.stack([(V[lab == k] > 0).mean(0) for k in range(K)], 1))
    fam = r["tested"]
    np.testing.assert_allclose(r["padj"][fam], ref.nhood_ref.bh(r["pvalue"][fam]), rtol=0)
    assert np.all(r["padj"][fam] >= r["pvalue"][fam]) and np.isnan(r["padj"][~fam]).all()


def test_masking_by_the_threshold_empty_domains_and_a_pair_of_one_gene(planted):
    V, lab, K, pairs, S, c, sizes = planted
    r = ref.all_cells(S, c, sizes, pairs, 0.1)
    pct = r["gene_pct"]
    low = pct[2] < 0.1
    assert low.any() and (pct[2] > 0).all()                                          # gene 2: stored in about 5 % of the spots
    for a in range(K):
        assert r["tested"][1, a].all() == (not low[a]) and r["tested"][5, :, a].all() == (not low[a])
        if low[a]:
            assert not r["tested"][1, a].any() and np.isnan(r["pvalue"][1, a]).all() and np.all(r["mean"][1, a] == 0.0)
    r0 = ref.all_cells(S, c, sizes, pairs, 0.0)
    assert r0["tested"].all() and np.isfinite(r0["pvalue"]).all()                    # threshold 0 unmasks it
    np.testing.assert_array_equal(r0["pvalue"][r["tested"]], r["pvalue"][r["tested"]])
    np.testing.assert_array_equal(np.diagonal(r["mean"][2]), r["gene_mean"][3])      # source == target: the gene's own mean
    np.testing.assert_array_equal(r["mean"][2], r["mean"][2].T)
    Vs, ls = cases.call4()[2]                                                        # n = 37, domain 2 empty
    sz = np.bincount(ls, minlength=4)
    assert sz[2] == 0
    e = ref.all_cells(ref.sums(Vs, ref.labelings(ls, 20, cases.SEED, 2), 4), ref.positive_counts(Vs, ls, 4), sz, cases.CALL4_PAIRS,
                      0.0)
    assert np.isnan(e["mean"][:, 2, :]).all() and np.isnan(e["mean"][:, :, 2]).all() and not e["tested"][:, 2].any()
    assert np.isnan(e["pvalue"][:, :, 2]).all() and np.all(e["gene_mean"][:, 2] == 0.0) and np.all(e["gene_pct"][:, 2] == 0.0)
    assert not e["tested"][0].any() and np.all(e["mean"][0][:, [0, 1, 3]][[0, 1, 3]] == 0.0)   # gene 0 is all zero there: mean 0, untested
    assert e["tested"][5][[0, 1, 3]][:, [0, 1, 3]].all()


def test_ligrec_stats_agrees_with_the_restatement_on_its_own_sums(planted):
    from spadot_amd.ligrec import ligrec_stats
    V, lab, K, pairs, S, c, sizes = planted
    problems = [(S, c, sizes, pairs)]
    Vs, ls = cases.call4()[2]
    problems.append((ref.sums(Vs, ref.labelings(ls, 20, cases.SEED, 2), 4), ref.positive_counts(Vs, ls, 4), np.bincount(ls, minlength=4),
                     cases.CALL4_PAIRS))
    for S_, c_, sz, pr in problems:
        for thr in (0.1, 0.0, 0.5):
            want = ref.all_cells(S_, c_, sz, pr, thr)
            got = ligrec_stats(S_[0], want["ge"], c_, sz, pr, S_.shape[0] - 1, thr)
            for k in ("mean", "pvalue", "padj", "tested", "gene_mean", "gene_pct"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} at threshold {thr}")
    none = ligrec_stats(S[0], None, c, sizes, pairs, 0, 0.1)                         # P = 0: the means alone
    assert np.isnan(none["pvalue"]).all() and np.isnan(none["padj"]).all()
    np.testing.assert_array_equal(none["mean"], ref.all_cells(S, c, sizes, pairs, 0.1)["mean"])


@pytest.mark.parametrize("name", [c[0] for c in cases.PVALUE_CASES])
def test_the_cells_a_rounding_could_flip_stay_below_the_cap(name):
    S, c, sizes, fwd, near = cases.pvalue_ref(name)
    Sr, _, _, rev, near_r = cases.pvalue_ref(name, reverse=True)
    V = cases.pvalue_case(name)[0]
    assert np.all(np.abs(S - Sr) <= ref.sum_bound(S, ref.stored(V)))                 # the two orders lie within the derived bound
    tested = fwd["tested"]
    np.testing.assert_array_equal(tested, rev["tested"])
    out = int((near & tested).sum())
    print(f"{name}: {out} of {int(tested.sum())} tested cells hold a comparison within the rounding bound")
    assert tested.sum() >= 50 and out <= 0.01 * tested.sum()
    keep = tested & ~near & ~near_r
    np.testing.assert_array_equal(fwd["pvalue"][keep], rev["pvalue"][keep])


def test_read_interactions_drops_duplicates_and_missing_genes(tmp_path, capsys):
    from spadot_amd.ligrec import read_interactions
    genes = np.asarray(["A", "B", "C", "a"])
    path = tmp_path / "pairs.csv"
    path.write_text("source,target,note\nA,B,x\nB,A,x\nA,B,again\nC,D,missing\na,A,case\nNA,A,a gene called NA\n")
    got = read_interactions(str(path), genes)
    assert got.tolist() == [[0, 1], [1, 0], [3, 0]] and got.dtype == np.int64
    assert "dropped 3 of 6 interactions (1 duplicates, 2 with a gene" in capsys.readouterr().err
    path.write_text("source,target\nX,Y\n")
    with pytest.raises(ValueError, match="no interaction is left"):
        read_interactions(str(path), genes)
    path.write_text("ligand,receptor\nA,B\n")
    with pytest.raises(ValueError, match="no `source` column"):
        read_interactions(str(path), genes)


def test_table_rows_are_the_tested_cells_in_order(planted):
    from spadot_amd.ligrec import TABLE_COLUMNS, LigrecResult, ligrec_stats, ligrec_table
    V, lab, K, pairs, S, c, sizes = planted
    want = ref.all_cells(S, c, sizes, pairs, 0.1)
    names = np.asarray([f"g{g}" for g in range(12)])
    r = LigrecResult(ligrec_stats(S[0], want["ge"], c, sizes, pairs, 200, 0.1), sizes, want["ge"], pairs, names)
    tab = ligrec_table(r, top=0)
    assert tuple(tab.columns) == TABLE_COLUMNS and len(tab) == int(want["tested"].sum())
    assert np.all(np.diff(tab["pvalue"]) >= 0)
    same = np.diff(tab["pvalue"]) == 0
    assert np.all(np.diff(tab["mean"])[same] <= 0)
    first = tab.iloc[0]
    assert first["pvalue"] == 1 / 201 and first["mean"] == tab["mean"][tab["pvalue"] == 1 / 201].max()
    row = tab[(tab["source"] == "g0") & (tab["target"] == "g1") & (tab["domain_source"] == 0) & (tab["domain_target"] == 1)].iloc[0]
    assert row["mean"] == want["mean"][0, 0, 1] and row["mean_source"] == want["gene_mean"][0, 0]
    assert row["pct_target"] == want["gene_pct"][1, 1] and row["padj"] == want["padj"][0, 0, 1]
    assert len(ligrec_table(r, top=7)) == 7 and ligrec_table(r, top=7).equals(tab.iloc[:7])


def test_parser_takes_the_sub_command():
    from spadot_amd.cli import build_parser
    a = build_parser().parse_args(["ligrec", "-i", "c.npz", "--domains", "d.csv", "--interactions", "p.csv"])
    assert (a.cmd_choice, a.data, a.domains, a.interactions) == ("ligrec", "c.npz", "d.csv", "p.csv")
    assert (a.output_dir, a.prefix, a.n_perms, a.seed, a.threshold, a.top, a.device) == (None, "", 1000, 0, 0.1, 100, "cuda:0")
    a = build_parser().parse_args(["ligrec", "-i", "c", "--domains", "d", "--interactions", "p", "-o", "out", "--prefix", "x_",
                                   "--n_perms", "50", "--seed", "4", "--threshold", "0", "--top", "0", "--device", "cuda:1"])
    assert (a.output_dir, a.prefix, a.n_perms, a.seed, a.threshold, a.top, a.device) == ("out", "x_", 50, 4, 0.0, 0, "cuda:1")
    for missing in (["-i", "c", "--domains", "d"], ["-i", "c", "--interactions", "p"], ["--domains", "d", "--interactions", "p"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["ligrec"] + missing)


def test_the_sub_command_names_a_file_that_does_not_exist(tmp_path, capsys):
    from spadot_amd.cli import main
    with pytest.raises(SystemExit) as e:
        main(["ligrec", "-i", str(tmp_path / "none.npz"), "--domains", str(tmp_path / "d.csv"), "--interactions",
              str(tmp_path / "p.csv")])
    assert e.value.code == 2 and "SpaDOT ligrec: the counts does not exist" in capsys.readouterr().err
