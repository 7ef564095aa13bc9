"""CPU: the numpy restatement of the spatial-autocorrelation definition (tests/autocorr_ref.py) held to its own conditions on the
20 x 20 planted grid -- the graph moments, the analytic null against the permutation null, the invariance under symmetrising the
graph, the sign of the structured and the anti-structured genes -- and the command line of the stage.  No GPU."""
import numpy as np
import pytest

import autocorr_cases as cases
import autocorr_ref as ref
import nhood_cases as nc


def _I_C(src, dst, v):
    n, E = v.shape[0], src.shape[0]
    c = v.astype(np.float64).mean()
    N, D, _ = ref.edge_sums(src, dst, v, c)
    m2, _ = ref.spread(v, c)
    return n * N / (E * m2), (n - 1.0) * D / (2.0 * E * m2)


def test_graph_moments_of_the_planted_grid():
    _, _, src, dst, _ = nc.planted(20)
    assert src.shape[0] == 2400
    assert ref.graph_moments(src, dst, 400) == (2400, 4544, 58240)
    assert ref.graph_moments_dense(src, dst, 400) == (2400, 4544, 58240)
    call = cases.edge_call()
    for (s, d, V) in call[1:]:
        assert ref.graph_moments(s, d, V.shape[0]) == ref.graph_moments_dense(s, d, V.shape[0])
    s, d, _ = call[2]                                        # the duplicate and the reciprocal edge are in the multiplicities
    pairs = list(zip(s.tolist(), d.tolist()))
    assert len(set(pairs)) < len(pairs) and any((j, i) in set(pairs) for i, j in pairs)


def test_the_analytic_null_agrees_with_the_permutation_null():
    src, dst, V = cases.planted_genes()
    EI, VI, EC, VC = ref.analytic_null(400, 2400, 4544, 58240)
    assert EI == -1.0 / 399.0 and EC == 1.0
    assert abs(np.sqrt(VI) - 0.02786) < 5e-6 and abs(np.sqrt(VC) - 0.02877) < 5e-6
    N, D, _, _ = cases.planted_sums()
    for g, name in enumerate(cases.PLANTED_GENES):
        m2, _ = ref.spread(V[:, g], cases.centres(V)[g])
        sd_I = (400 * N[g, 1:] / (2400 * m2)).std()
        sd_C = (399 * D[g, 1:] / (2 * 2400 * m2)).std()
        print(f"{name}: permutation sd of I {sd_I:.4f} (analytic {np.sqrt(VI):.4f}), of C {sd_C:.4f} ({np.sqrt(VC):.4f})")
        if name == "gradient":                               # this draw: 0.0277 and 0.0269
            assert abs(sd_I - 0.0277) < 0.0002 and abs(sd_C - 0.0269) < 0.0002
        if name == "single":                                 # one spike: as far from normal as a gene can be (0.0005 and 0.098);
            assert sd_I < 0.001 and sd_C > 0.09              # the analytic null does not hold there, the permutation null does
            continue
        assert abs(sd_I / np.sqrt(VI) - 1.0) < 0.15, (name, sd_I)
        assert abs(sd_C / np.sqrt(VC) - 1.0) < 0.15, (name, sd_C)
        assert abs((400 * N[g, 1:] / (2400 * m2)).mean() - EI) < 4 * np.sqrt(VI / 200)


def test_I_and_C_do_not_change_when_the_graph_is_symmetrised():
    src, dst, V = cases.planted_genes()
    s2, d2 = np.concatenate([src, dst]), np.concatenate([dst, src])
    for g in range(V.shape[1]):
        a, b = _I_C(src, dst, V[:, g]), _I_C(s2, d2, V[:, g])
        assert abs(a[0] - b[0]) < 1e-13 and abs(a[1] - b[1]) < 1e-13


def test_structured_genes_are_found_and_the_checkerboard_is_negative():
    src, dst, V = cases.planted_genes()
    N, D, _, _ = cases.planted_sums()
    E = src.shape[0]
    c = cases.centres(V)
    sp = np.array([ref.spread(V[:, g], c[g]) for g in range(6)])
    st = ref.stats(N, D, 400, E, sp[:, 0], sp[:, 1], (2400, 4544, 58240))
    print("I", np.round(st["I"], 3), "C", np.round(st["C"], 3), "p_sim_I", st["p_sim_I"])
    assert not st["degenerate"].any()
    # this draw of the genes (autocorr_cases.planted_genes, default_rng(7)): I = 0.300 and 0.391, C = 0.705 and 0.610
    assert abs(st["I"][0] - 0.300) < 0.002 and abs(st["I"][1] - 0.391) < 0.002
    assert abs(st["C"][0] - 0.705) < 0.002 and abs(st["C"][1] - 0.610) < 0.002
    assert st["p_sim_I"][0] == 1 / 201 and st["p_sim_I"][1] == 1 / 201
    assert st["p_sim_C"][0] == 1 / 201 and st["p_sim_C"][1] == 1 / 201
    assert st["z_norm_I"][0] > 8 and st["z_norm_C"][0] < -8 and st["p_norm_I"][0] < 1e-12
    assert abs(st["I"][4] + 0.253) < 0.002 and st["p_sim_I"][4] == 1.0 and st["C"][4] > 1.2 and st["z_norm_I"][4] < -8
    assert abs(st["I"][2]) < 0.09 and abs(st["I"][3]) < 0.09                     # noise: inside three analytic sd
    assert st["padj_I"][0] <= 6 / 201 + 1e-15 and np.all(st["padj_I"] >= st["p_sim_I"])
    for g in range(6):                                                           # the gene-wise form against the batch form
        Ng, Dg, _ = ref.all_sums(src, dst, V[:, g], c[g], 5, cases.SEED, 0)
        np.testing.assert_array_equal(Ng, N[g, :6])
        np.testing.assert_array_equal(Dg, D[g, :6])


def test_degenerate_genes_are_nan_and_leave_the_family():
    call = cases.edge_call()
    for t, (src, dst, V) in enumerate(call):
        n, E = V.shape[0], src.shape[0]
        c = cases.centres(V)
        N, D, _ = ref.all_sums_genes(src, dst, V, c, 10, 1, t)
        sp = np.array([ref.spread(V[:, g], c[g]) for g in range(4)])
        mom = ref.graph_moments(src, dst, n) if E else (0, 0, 0)
        st = ref.stats(N, D, n, E, sp[:, 0], sp[:, 1], mom)
        want = [True] * 4 if n < 3 else [t == 2, False, False, True]
        assert st["degenerate"].tolist() == want, (t, st["degenerate"])
        for k in ref.FIELDS:
            assert np.isnan(st[k][st["degenerate"]]).all(), k
        if n >= 3:
            assert np.isfinite(st["padj_I"][~st["degenerate"]]).all()
            fam = ~st["degenerate"]
            np.testing.assert_array_equal(st["padj_I"][fam], ref.bh(st["p_sim_I"][fam]))


def test_the_sub_command_parses_and_a_missing_file_exits_with_2(tmp_path, capsys):
    from spadot_amd import cli
    args = cli.build_parser().parse_args(["autocorr", "-i", "counts.npz"])
    assert (args.cmd_choice, args.data, args.k, args.n_perms, args.seed, args.top, args.prefix, args.device) == \
        ("autocorr", "counts.npz", 6, 100, 0, 100, "", "cuda:0")
    args = cli.build_parser().parse_args(["autocorr", "-i", "c.npz", "-o", "out", "--prefix", "p_", "--k", "8", "--n_perms", "0",
                                          "--seed", "9", "--top", "0", "--device", "cuda:1"])
    assert (args.output_dir, args.prefix, args.k, args.n_perms, args.seed, args.top, args.device) == \
        ("out", "p_", 8, 0, 9, 0, "cuda:1")
    with pytest.raises(SystemExit) as e:
        cli.main(["autocorr", "-i", str(tmp_path / "nothing.npz")])
    assert e.value.code == 2
    assert "SpaDOT autocorr: the counts do not exist" in capsys.readouterr().err
    assert "python -m spadot_amd autocorr -i COUNTS" in cli.__doc__


def test_the_host_statistics_of_the_package_equal_the_restatement():
    from spadot_amd.autocorr import autocorr_stats
    src, dst, V = cases.planted_genes()
    N, D, _, _ = cases.planted_sums()
    c = cases.centres(V)
    sp = np.array([ref.spread(V[:, g], c[g]) for g in range(6)])
    want = ref.stats(N, D, 400, 2400, sp[:, 0], sp[:, 1], (2400, 4544, 58240))
    got = autocorr_stats(N, D, 400, 2400, sp[:, 0], (2400, 4544, 58240), sumsq=sp[:, 1])
    for k in ref.FIELDS:
        if k.startswith("p_sim"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        else:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    got0 = autocorr_stats(N[:, :1], D[:, :1], 400, 2400, sp[:, 0], (2400, 4544, 58240), sumsq=sp[:, 1])       # P = 0: BH of p_norm
    want0 = ref.stats(N[:, :1], D[:, :1], 400, 2400, sp[:, 0], sp[:, 1], (2400, 4544, 58240))
    assert np.isnan(got0["p_sim_I"]).all() and np.isnan(got0["z_sim_C"]).all()
    np.testing.assert_allclose(got0["padj_I"], want0["padj_I"], rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(got0["padj_C"], want0["padj_C"], rtol=1e-9, atol=1e-300)
