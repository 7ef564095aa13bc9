"""The random-labelling null of the cooccurrence stage without a device: the restatement (tests/cooccur_null_ref.py) against
cooccur_ref on explicitly relabelled sets and against ripley_ref on the diagonal, its symmetry, the host statistics of
spadot_amd.cooccurrence against the restatement's, the exact global test on counts near 2^62, Benjamini-Hochberg over unordered
pairs, the refusals that need no device, the parser, the existing path under --n_perms 0 and the planted verdicts."""
import argparse
import os

import numpy as np
import pytest

import cooccur_cases
import cooccur_null_cases as cases
import cooccur_null_ref as ref
import cooccur_ref
import nhood_cases
import nhood_ref
import ripley_ref

STATS = ("sim_mean", "sim_min", "sim_max", "z", "p_lo", "p_hi", "ratio", "ratio_sim_mean", "ratio_sim_min", "ratio_sim_max",
         "p_global", "padj")


@pytest.mark.parametrize("name,S,seed,g", [("edge2", 3, 0, 0), ("tile257", 2, 5, 3), ("lattice", 3, 1, 2)])
def test_the_restatement_equals_cooccur_ref_on_explicitly_relabelled_sets(name, S, seed, g):
    xy, lab, r2, K = cases.problem(name)
    N = cases.want(name, S, seed, g)
    assert N.shape == (1 + S, K, K, r2.shape[0]) and N.dtype == np.int64
    np.testing.assert_array_equal(N[0], cooccur_cases.want(name))                     # pattern 0 is the observed labeling
    for s in range(1 + S):
        xs, ls = ref.relabelled(xy, lab, K, s, seed, g)
        np.testing.assert_array_equal(np.bincount(ls, minlength=K), np.bincount(lab, minlength=K))      # the sizes stay
        np.testing.assert_array_equal(N[s], cooccur_ref.counts(xs, ls, r2, K), err_msg=f"pattern {s}")
    assert any((N[s] != N[0]).any() for s in range(1, 1 + S))


def test_first_advances_the_relabelings():
    xy, lab, r2, K = cases.problem("edge2")
    N = cases.want("edge2", 3, 0, 0)
    np.testing.assert_array_equal(ref.counts(xy, lab, r2, K, 2, 0, 0, first=1), N[[0, 2, 3]])


def test_the_diagonal_is_ripleys_pair_count_under_the_labels_null_and_the_counts_are_symmetric():
    xy, lab, K, radii, N = cases.planted()
    S, seed, g = (cases.PLANTED[k] for k in ("S", "seed", "g"))
    L = ripley_ref.counts(xy, lab, radii * radii, K, S, 1, null="labels", seed=seed, g=g, modes=("L",))
    for c in range(K):
        np.testing.assert_array_equal(N[:, c, c, :], L[c, :, 0, :], err_msg=f"domain {c}")
    np.testing.assert_array_equal(N, N.transpose(0, 2, 1, 3))


def _same(got, want, names=STATS):
    for name in names:
        np.testing.assert_array_equal(np.isnan(got[name]), np.isnan(want[name]), err_msg=name)
        np.testing.assert_allclose(got[name], want[name], rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
    np.testing.assert_array_equal(got["count"], want["count"])
    np.testing.assert_array_equal(got["relation"], want["relation"])


@pytest.mark.parametrize("ring", [False, True])
def test_the_host_statistics_match_the_restatement(ring):
    from spadot_amd.cooccurrence import cooccurrence_null_stats
    xy, lab, r2, K = cases.small_sizes()                                               # an empty label value, a domain of one spot
    sizes = np.bincount(lab, minlength=K)
    assert sizes[1] == 0 and sizes[3] == 1
    N = ref.counts(xy, lab, r2, K, 19, seed=3, g=1)
    got, want = cooccurrence_null_stats(N, sizes, ring=ring, alpha=0.2), ref.stats(N, sizes, ring=ring, alpha=0.2)
    _same(got, want)
    for name in ("sim_mean", "sim_min", "sim_max", "z", "p_lo", "p_hi"):
        assert np.all(np.isnan(got[name][1])) and np.all(np.isnan(got[name][:, 1])) and np.all(np.isnan(got[name][3, 3]))
        assert not np.any(np.isnan(got[name][0, 2])) or name == "z"
    assert np.all(np.isnan(got["p_global"][1])) and np.isnan(got["p_global"][3, 3]) and not np.isnan(got["p_global"][0, 3])
    assert got["count"].dtype == np.int64
    np.testing.assert_array_equal(got["count"], np.diff(N[0], axis=2, prepend=0) if ring else N[0])
    name = "tile255"
    xy, lab, r2, K = cases.problem(name)
    N = cases.want(name, 3, 0, 0)
    _same(cooccurrence_null_stats(N, np.bincount(lab, minlength=K), ring=ring), ref.stats(N, np.bincount(lab, minlength=K), ring=ring))
    with pytest.raises(ValueError, match=r"\[1 \+ S, K, K, B\]"):
        cooccurrence_null_stats(N[:1], np.bincount(lab, minlength=K))
    with pytest.raises(ValueError, match="sizes holds"):
        cooccurrence_null_stats(N, np.ones(K + 1))


def test_the_global_test_is_exact_on_counts_near_two_to_the_62():
    """u of rows 0 and 1 is 2^63 + 2, of rows 2 and 3 is 2^63 - 2: p_global = 2 / 4.  Wrapped int64 arithmetic and fp64 both see
    four equal deviations and give 1."""
    from spadot_amd.cooccurrence import cooccurrence_null_stats
    big = 2 ** 62
    rows = np.array([big + 1, 0, big, 1], dtype=np.int64)
    N = rows.reshape(4, 1, 1, 1)
    assert ripley_ref.mad_p(None, exact=rows.reshape(4, 1)) == 0.5
    got = cooccurrence_null_stats(N, [3])
    assert got["p_global"][0, 0] == 0.5
    with np.errstate(over="ignore"):
        wrapped = np.abs(4 * rows - rows.sum())
    assert (wrapped >= wrapped[0]).sum() / 4 == 1.0 and len(set((4.0 * rows - float(rows.sum())).tolist())) == 2
    B = 5                                                                              # and over several radii, against Python integers
    T = np.cumsum(np.random.default_rng(3).integers(big // 8, big // 4, (8, 2, 2, B)), axis=3)
    T = T + T.transpose(0, 2, 1, 3)
    got = cooccurrence_null_stats(T, [5, 6])["p_global"]
    for a in range(2):
        for b in range(2):
            assert got[a, b] == ripley_ref.mad_p(None, exact=T[:, a, b, :])


def test_benjamini_hochberg_runs_over_the_unordered_pairs():
    from spadot_amd.cooccurrence import cooccurrence_null_stats
    xy, lab, r2, K = cases.problem("tile513")
    N = ref.counts(xy, lab, r2, K, 19, seed=11, g=0)
    got = cooccurrence_null_stats(N, np.bincount(lab, minlength=K))
    p, padj = got["p_global"], got["padj"]
    iu = np.triu_indices(K)
    np.testing.assert_allclose(padj[iu], nhood_ref.bh(p[iu]), rtol=1e-12, atol=0)       # K (K + 1) / 2 = 15 tests, not 25
    np.testing.assert_array_equal(padj, padj.T)
    assert len(set(np.round(p[iu], 12))) > 1
    assert not np.allclose(padj.reshape(-1), nhood_ref.bh(p.reshape(-1)))              # an ordered family counts every pair twice


def test_refusals_that_need_no_device(tmp_path):
    import torch
    from spadot_amd.cooccurrence import cooccur, cooccurrence_null, cooccurrence_null_counts
    xy, lab, r2, K = cases.problem("edge2")
    for fn, kw in ((cooccurrence_null_counts, dict(radii_sq=[r2])), (cooccurrence_null, {})):
        with pytest.raises(RuntimeError, match="MI355X only.*no CPU path"):
            fn([torch.as_tensor(xy)], [lab], n_perms=3, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        cooccurrence_null_counts([torch.as_tensor(xy)], [lab], n_perms=3)
    for S in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="relabelings"):
            cooccurrence_null_counts([torch.as_tensor(xy)], [lab], radii_sq=[r2], n_perms=S)
    df = nhood_cases.stage_table()
    for S in (10000, -1):
        with pytest.raises(ValueError, match="0 to 9999"):
            cooccur(argparse.Namespace(domains=df, output_dir=str(tmp_path), n_perms=S, device="cuda:0"))
    wide = df.assign(kmeans=np.arange(len(df)) % 32)                                   # K = 32, B = 64: 10000 x 1024 x 64 x 8 > 2 GiB
    with pytest.raises(ValueError, match=r"n_perms = 9999 .* K = 32 .* B = 64 .*2147483648"):
        cooccur(argparse.Namespace(domains=wide, output_dir=str(tmp_path), n_perms=9999, bins=64, device="cuda:0"))
    assert not os.listdir(tmp_path) or all(not f.endswith((".csv", ".npz")) for f in os.listdir(tmp_path))


def test_the_parser_takes_the_options_of_the_null():
    import spadot_amd.cli as cli
    a = cli.build_parser().parse_args(["cooccurrence", "--domains", "d.csv"])
    assert (a.n_perms, a.seed, a.alpha) == (0, 0, 0.05)
    a = cli.build_parser().parse_args(["cooccurrence", "--domains", "d.csv", "--n_perms", "99", "--seed", "7", "--alpha", "0.01"])
    assert (a.n_perms, a.seed, a.alpha, a.bins, a.ring) == (99, 7, 0.01, 50, False)
    assert "--n_perms 0" in cli.__doc__ and "DESIGN 7i-null" in cli.__doc__


def test_without_relabelings_the_stage_takes_the_existing_path(tmp_path, monkeypatch):
    """--n_perms 0: the stage calls cooccurrence with the arguments it always passed, never the null, and writes no new file."""
    import torch
    import spadot_amd.cooccurrence as co
    calls = []

    def observed(coords, labels, radii=None, ring=False, n_clusters=None):
        calls.append("cooccurrence")
        return [co.CooccurResult(cooccur_ref.counts(xy, lab, r * r, K), r, np.bincount(lab, minlength=K), ring)
                for xy, lab, r, K in zip(coords, labels, radii, n_clusters)]

    def null(*a, **kw):
        calls.append("cooccurrence_null")
        raise AssertionError("the null was asked for")

    monkeypatch.setattr(co, "cooccurrence", observed)
    monkeypatch.setattr(co, "cooccurrence_null", null)
    monkeypatch.setattr(torch, "as_tensor", lambda x, device=None: x)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: None)
    df = nhood_cases.stage_table()
    for sub, extra in (("a", {}), ("b", dict(n_perms=0, seed=5, alpha=0.5))):
        res = co.cooccur(argparse.Namespace(domains=df, output_dir=str(tmp_path / sub), prefix="s_", bins=6, device="cuda:0", **extra))
        assert set(res) == {"tables", "results", "timepoints", "timings"}
    assert calls == ["cooccurrence", "cooccurrence"]
    names = sorted(f for f in os.listdir(tmp_path / "a") if not f.endswith(".png"))
    assert names == ["s_cooccurrence.npz"] + [f"s_cooccurrence_{tp}.csv" for tp in ("E10", "E12", "E14")]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b"))
    for f in names:
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    with pytest.raises(AssertionError, match="the null was asked for"):
        co.cooccur(argparse.Namespace(domains=df, output_dir=str(tmp_path / "c"), bins=6, n_perms=2, device="cuda:0"))


def _verdicts(N, sizes):
    from spadot_amd.cooccurrence import cooccurrence_null_stats
    got, want = cooccurrence_null_stats(N, sizes), ref.stats(N, sizes)
    _same(got, want)
    return got


def test_the_planted_verdicts():
    xy, lab, K, radii, N = cases.planted()
    got = _verdicts(N, np.bincount(lab, minlength=K))
    np.testing.assert_array_equal(got["p_global"], np.full((K, K), 1 / 40))              # every observed curve is the most extreme
    np.testing.assert_array_equal(got["padj"], np.full((K, K), 1 / 40))
    for a in range(K):
        for b in range(K):
            want = "attract" if a == b or (a, b) in cases.ATTRACT or (b, a) in cases.ATTRACT else "avoid"
            assert got["relation"][a, b] == want, (a, b)


def test_a_compact_domain_reads_significant_against_labels_dealt_at_random():
    """The caveat of DESIGN 7i-null: label 7 is dealt to 300 spots independently of the seven planted domains.  With itself it is
    independent (p_global 0.775); with every compact domain the pair is NOT a random labelling (p_global 1 / 40), although
    nothing interacts."""
    xy, lab, K, radii, N = cases.caveat()
    got = _verdicts(N, np.bincount(lab, minlength=K))
    assert got["p_global"][7, 7] == 0.775 and got["relation"][7, 7] == "independent"
    np.testing.assert_array_equal(got["p_global"][7, :7], np.full(7, 1 / 40))
    np.testing.assert_array_equal(got["p_global"][:7, 7], np.full(7, 1 / 40))
    assert all(r != "independent" for r in got["relation"][7, :7])
