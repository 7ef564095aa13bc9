"""The co-occurrence null on the MI355X against the numpy restatement of its definition (tests/cooccur_null_ref.py, held to
cooccur_ref and ripley_ref by tests/test_cooccur_null_cpu.py): k_cooccur_null through spadot_cooccur_null, stage_ops and
spadot_amd.cooccurrence.  Everything the device computes is an integer, so every comparison of counts is assert_array_equal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cooccur_cases
import cooccur_null_cases as cases
import cooccur_null_ref as ref
import nhood_cases
import ripley_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


def _null(problems, S, **kw):
    """cooccurrence_null_counts of [(xy, labels, r2, K)] by squared thresholds."""
    from spadot_amd.cooccurrence import cooccurrence_null_counts
    return cooccurrence_null_counts([_dev(p[0]) for p in problems], [p[1] for p in problems], radii_sq=[p[2] for p in problems],
                                    n_perms=S, n_clusters=[p[3] for p in problems], **kw)


def _layout(problems, gids=None):
    """(xy device tensor, desc int64 [P, 40], [p] -> r2) of a call to stage_ops.cooccur_null_counts, laid out by hand."""
    xs, desc, first = [], np.zeros((len(problems), 40), dtype=np.int64), 0
    for p, (xy, lab, r2, K) in enumerate(problems):
        s, off = ripley_ref.by_label(xy, lab, K)
        xs.append(s)
        desc[p, :4] = (first, s.shape[0], K, len(r2))
        desc[p, 4:5 + K] = off
        desc[p, 37] = p if gids is None else gids[p]
        first += s.shape[0]
    return _dev(np.concatenate(xs)), desc, [p[2] for p in problems]


def _raw(problems, observed, first, n_perms, seed=0, gids=None, K_max=None, B_max=None, out=None):
    """stage_ops.cooccur_null_counts: int64 numpy [P, observed + n_perms, K_max, K_max, B_max]."""
    from spadot_amd import stage_ops as ops
    xy, desc, r2 = _layout(problems, gids)
    K_max = K_max or max(p[3] for p in problems)
    B_max = B_max or max(len(p[2]) for p in problems)
    return ops.cooccur_null_counts(xy, desc, r2, K_max, B_max, observed, first, n_perms, seed=seed, out=out).cpu().numpy()


@pytest.mark.parametrize("S", [1, 19])
def test_edge_call_matches_the_restatement(S):
    call = cooccur_cases.edge_call()
    got = _null(call, S)                                                             # n = 1, coincident spots, an empty label, K = 32 / B = 64
    assert [g.shape for g in got] == [(1 + S, 1, 1, 1), (1 + S, 2, 2, 16), (1 + S, 3, 3, 17), (1 + S, 32, 32, 64)]
    for i, g in enumerate(got):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, cases.want(f"edge{i}", S, 0, i), err_msg=f"problem {i}")
    assert not got[0].any()                                                          # n = 1: no pairs
    np.testing.assert_array_equal(got[1], np.broadcast_to(np.array([[0, 1], [1, 0]])[None, :, :, None], (1 + S, 2, 2, 16)))
    assert not got[2][:, 1].any() and not got[2][:, :, 1].any()                      # the label value without spots, in every pattern


@pytest.mark.parametrize("n", cooccur_cases.TILE_SIZES)
def test_sets_that_straddle_the_tile_match_the_restatement(n):
    np.testing.assert_array_equal(_null([cooccur_cases.tile_case(n)], 3)[0], cases.want(f"tile{n}", 3))


def test_the_integer_lattice_matches_the_restatement():
    got = _null([cooccur_cases.lattice()], 3)[0]
    np.testing.assert_array_equal(got, cases.want("lattice", 3))
    np.testing.assert_array_equal(got.sum(axis=(1, 2))[:, :3], np.tile([0, 528, 528 + 484], (4, 1)))      # a relabelling keeps the pairs


def test_pairs_on_their_threshold_count_in_every_pattern():
    got = _null([cases.problem("on_threshold")], 3)[0]
    want = cases.want("on_threshold", 3)
    print("ordered pairs that differ from the restatement, per pattern:", np.abs(got - want).sum(axis=(1, 2, 3)).tolist())
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got.sum(axis=(1, 2)), np.tile(got[0].sum(axis=(0, 1)), (4, 1)))


def test_pattern_0_is_cooccurrence_counts_and_the_diagonal_is_ripleys_labels_null():
    from spadot_amd.cooccurrence import cooccurrence_counts
    from spadot_amd.ripley import ripley_counts
    prob = cooccur_cases.tile_case(513)
    xy, lab, r2, K = prob
    S, seed, g = 5, 9, 4
    got = _null([prob], S, seed=seed, problem_ids=[g])[0]
    np.testing.assert_array_equal(got, cases.want("tile513", S, seed, g))
    np.testing.assert_array_equal(got[0], cooccurrence_counts([_dev(xy)], [lab], radii_sq=[r2], n_clusters=[K])[0])
    L = ripley_counts([_dev(xy)], [lab], radii_sq=[r2], n_sim=S, n_probes=1, null="labels", modes=("L",), seed=seed,
                      n_clusters=[K], problem_ids=[g])[0]
    for c in range(K):
        np.testing.assert_array_equal(got[:, c, c, :], L[c, :, 0, :], err_msg=f"domain {c}")
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1, 3))


def test_a_problem_alone_in_a_batch_and_run_twice_gives_the_same_integers():
    call = cooccur_cases.edge_call()
    prob = cooccur_cases.tile_case(257)
    S = 3
    alone = _null([prob], S)[0]
    np.testing.assert_array_equal(alone, cases.want("tile257", S))
    batch = _null([call[3], cooccur_cases.tile_case(513), prob, call[1], cooccur_cases.lattice()], S,
                  problem_ids=[7, 1, 0, 3, 2])                                        # other n, K and B around it
    np.testing.assert_array_equal(batch[2], alone)
    np.testing.assert_array_equal(batch[0], cases.want("edge3", S, 0, 7))
    np.testing.assert_array_equal(batch[1], cases.want("tile513", S, 0, 1))
    np.testing.assert_array_equal(_null([prob], S)[0], alone)                         # called twice
    wide = _null([(prob[0], prob[1], prob[2], 9)], S)[0]                              # a larger K: the same corner, zeros around
    np.testing.assert_array_equal(wide[:, :5, :5], alone)
    assert wide.shape == (1 + S, 9, 9, 7) and wide[:, 5:].sum() == 0 and wide[:, :, 5:].sum() == 0
    many = np.concatenate([prob[2], prob[2][-1] + 1.0 + np.arange(33.0)])             # a larger B: the same leading thresholds
    more = _null([(prob[0], prob[1], many, 5)], S)[0]
    assert more.shape == (1 + S, 5, 5, 40)
    np.testing.assert_array_equal(more[..., :7], alone)
    out = torch.full((2, 1 + S, 32, 32, 64), -77, dtype=torch.int64, device=DEV)      # a larger K_max and B_max, a poisoned output
    res = _raw([prob, call[3]], 1, 0, S, gids=[0, 7], K_max=32, B_max=64, out=out)
    np.testing.assert_array_equal(res, out.cpu().numpy())
    np.testing.assert_array_equal(res[0, :, :5, :5, :7], alone)
    np.testing.assert_array_equal(res[1], cases.want("edge3", S, 0, 7))
    assert res[0].sum() == alone.sum() and res.min() == 0                             # every element of the output is written


def test_any_split_of_the_relabelings_gives_the_integers_of_one_call():
    probs = [cooccur_cases.tile_case(257), cooccur_cases.edge_call()[2]]
    S, seed = 6, 3
    want = [cases.want("tile257", S, seed, 0), cases.want("edge2", S, seed, 1)]
    one = _raw(probs, 1, 0, S, seed=seed)
    for p, w in enumerate(want):
        np.testing.assert_array_equal(one[p, :, :w.shape[1], :w.shape[2], :w.shape[3]], w)
    np.testing.assert_array_equal(_raw(probs, 0, 0, S, seed=seed), one[:, 1:])        # observed = 0: the relabelings alone
    np.testing.assert_array_equal(_raw(probs, 1, 0, 0, seed=seed), one[:, :1])        # and the observed labeling alone
    two = np.concatenate([_raw(probs, 1, 0, 2, seed=seed), _raw(probs, 0, 2, 4, seed=seed)], axis=1)
    np.testing.assert_array_equal(two, one)                                           # `first` advanced across two calls
    each = np.concatenate([_raw(probs, 0, s, 1, seed=seed) for s in range(S)], axis=1)
    np.testing.assert_array_equal(each, one[:, 1:])                                   # and across S calls
    whole = _null(probs, S, seed=seed)
    small = _null(probs, S, seed=seed, max_bytes=1)                                   # one pattern per call
    for w, a, b in zip(want, whole, small):
        np.testing.assert_array_equal(a, w)
        np.testing.assert_array_equal(b, w)


def test_another_seed_and_another_problem_number_draw_other_relabelings():
    prob = cooccur_cases.tile_case(255)
    base = _null([prob], 3)[0]
    for kw, key in ((dict(seed=1), (1, 0)), (dict(problem_ids=[1]), (0, 1))):
        other = _null([prob], 3, **kw)[0]
        np.testing.assert_array_equal(other, cases.want("tile255", 3, *key))
        np.testing.assert_array_equal(other[0], base[0])
        assert all((other[s] != base[s]).any() for s in (1, 2, 3))


SENTINEL = -77


def test_refusals_come_before_any_launch():
    from spadot_amd import stage_ops as ops
    from spadot_amd.cooccurrence import cooccurrence_null_counts
    prob = cooccur_cases.edge_call()[2]
    xy, desc, r2 = _layout([prob])
    out = torch.full((1, 4, 3, 3, 17), SENTINEL, dtype=torch.int64, device=DEV)
    for kw, what in ((dict(observed=1, first=0, n_perms=65535), "patterns"), (dict(observed=0, first=0, n_perms=0), "at least one"),
                     (dict(observed=1, first=-1, n_perms=3), "first >= 0"), (dict(observed=1, first=2 ** 31 - 2, n_perms=3), "2\\^31")):
        with pytest.raises(ValueError, match=what):
            ops.cooccur_null_counts(xy, desc, r2, 3, 17, out=out, **kw)
    for g in (-1, 2 ** 31):
        bad = desc.copy()
        bad[0, 37] = g
        with pytest.raises(ValueError, match="problem number"):
            ops.cooccur_null_counts(xy, bad, r2, 3, 17, 1, 0, 3, out=out)
    with pytest.raises(ValueError, match="label values"):                             # and everything cooccur_check refuses
        ops.cooccur_null_counts(xy, desc, r2, 2, 17, 1, 0, 3, out=out)
    with pytest.raises(ValueError, match="problem_ids"):
        cooccurrence_null_counts([_dev(prob[0])], [prob[1]], radii_sq=[prob[2]], n_perms=3, problem_ids=[2 ** 31])
    with pytest.raises(ValueError, match="out must be"):
        ops.cooccur_null_counts(xy, desc, r2, 3, 17, 1, 0, 4, out=out)
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)                                                # nothing was launched
    lib = ops.model_lib()                                                            # the library's own checks, from the host copies
    pad = np.full((1, 32), -1.0)
    pad[0, :17] = r2[0]

    def call(d=desc, observed=1, first=0, n_perms=3, P=1, k_max=3, b_max=17):
        d_dev, pad_dev = _dev(d), _dev(pad)              # both alive until the call is done: a kernel may read them
        rc = lib.spadot_cooccur_null(xy.data_ptr(), ctypes.c_void_p(d.ctypes.data), d_dev.data_ptr(),
                                     ctypes.c_void_p(pad.ctypes.data), pad_dev.data_ptr(), P, k_max, b_max, observed, first,
                                     n_perms, 0, out.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    assert call(observed=2) == -22 and call(observed=-1) == -22
    assert call(observed=0, n_perms=0) == -7 and call(n_perms=65535) == -7 and call(n_perms=-1) == -7
    assert call(P=65536) == -7 and call(first=-1) == -7 and call(first=2 ** 31 - 2) == -7
    for g in (-1, 2 ** 31):
        bad = desc.copy()
        bad[0, 37] = g
        assert call(bad) == -7, g
    assert call(k_max=33) == -7 and call(b_max=65) == -7                              # what spadot_cooccur_counts refuses
    bad = desc.copy()
    bad[0, 6] = 16
    assert call(bad) == -22
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)
    assert call() == 0                                                               # and the same tensor is written by a valid call
    np.testing.assert_array_equal(out.cpu().numpy()[0], cases.want("edge2", 3))


def test_the_planted_verdicts_on_the_device():
    from spadot_amd.cooccurrence import cooccurrence_null
    xy, lab, K, radii, N = cases.planted()
    kw = {k: cases.PLANTED[k] for k in ("bins", "seed")}
    r = cooccurrence_null([_dev(xy)], [lab], n_perms=cases.PLANTED["S"], n_clusters=[K], problem_ids=[cases.PLANTED["g"]], **kw)[0]
    np.testing.assert_array_equal(r.radii, radii)
    np.testing.assert_array_equal(r.null_counts, N)
    np.testing.assert_array_equal(r.counts, N[0])
    want = ref.stats(N, np.bincount(lab, minlength=K))
    for name in ("sim_mean", "z", "p_hi", "p_lo", "ratio", "ratio_sim_min", "ratio_sim_max", "p_global", "padj"):
        np.testing.assert_allclose(getattr(r, name), want[name], rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
    np.testing.assert_array_equal(r.p_global, np.full((K, K), 1 / 40))
    for a in range(K):
        for b in range(K):
            verdict = "attract" if a == b or (a, b) in cases.ATTRACT or (b, a) in cases.ATTRACT else "avoid"
            assert r.relation[a, b] == verdict, (a, b)


OLD_FILES = ["s_cooccurrence.npz"] + [f"s_cooccurrence_{tp}.csv" for tp in ("E10", "E12", "E14")]
NEW_FILES = ["s_cooccurrence_null.npz", "s_cooccurrence_summary.csv"] + [f"s_cooccurrence_null_{tp}.csv" for tp in ("E10", "E12", "E14")]


def _stage(path, out, *options, child=True):
    """The files (but the plots) that the sub-command writes: in a child process, or through the parser in this one."""
    argv = ["cooccurrence", "--domains", path, "-o", str(out), "--prefix", "s_", "--bins", "12", "--device", DEV, *options]
    if child:
        r = subprocess.run([sys.executable, "-m", "spadot_amd"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    else:
        from spadot_amd.cli import build_parser
        from spadot_amd.cooccurrence import cooccur
        cooccur(build_parser().parse_args(argv))
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if not f.endswith(".png")}


def test_the_stage_through_its_sub_command(tmp_path):
    import pandas as pd
    from spadot_amd.cooccurrence import NULL_SUMMARY_COLUMNS, NULL_TABLE_COLUMNS
    from spadot_amd.utils._analyze_utils import have_matplotlib
    df = nhood_cases.stage_table()
    path = str(tmp_path / "domains.csv")
    df.to_csv(path, index=False)
    plain = _stage(path, tmp_path / "plain", child=False)                            # a run without the option
    zero = _stage(path, tmp_path / "zero", "--n_perms", "0", "--seed", "4", child=False)
    assert sorted(plain) == sorted(OLD_FILES) and zero == plain                      # no new file, the same bytes
    assert not [f for f in os.listdir(tmp_path / "zero") if "null" in f or "summary" in f]
    first = _stage(path, tmp_path / "first", "--n_perms", "9", "--seed", "4", "--alpha", "0.2")
    again = _stage(path, tmp_path / "again", "--n_perms", "9", "--seed", "4", "--alpha", "0.2", child=False)
    assert sorted(first) == sorted(OLD_FILES + NEW_FILES) and first == again          # two runs write the same bytes
    assert all(first[f] == plain[f] for f in OLD_FILES)                              # the existing files keep their bytes
    want = cases.stage_want(9, 4, 12)
    z = np.load(tmp_path / "first" / "s_cooccurrence_null.npz")
    assert int(z["n_perms"]) == 9 and int(z["seed"]) == 4 and float(z["alpha"]) == 0.2 and z["timepoints"].tolist() == list(want)
    summary = pd.read_csv(tmp_path / "first" / "s_cooccurrence_summary.csv", float_precision="round_trip")
    assert tuple(summary.columns) == NULL_SUMMARY_COLUMNS == ("timepoint", "domain", "neighbor", "n_domain", "n_neighbor", "p_global",
                                                              "padj", "relation")
    assert len(summary) == sum(K * K for _, _, K in want.values())
    for tp, (N, radii, K) in want.items():
        np.testing.assert_array_equal(z[f"{tp}_null_counts"], N, err_msg=tp)
        sizes = z[f"{tp}_sizes"]
        st = ref.stats(N, sizes, alpha=0.2)
        tab = pd.read_csv(tmp_path / "first" / f"s_cooccurrence_null_{tp}.csv", float_precision="round_trip")
        assert tuple(tab.columns) == NULL_TABLE_COLUMNS == ("domain", "neighbor", "radius", "count", "sim_mean", "sim_min", "sim_max",
                                                            "z", "p_lo", "p_hi", "ratio", "ratio_sim_mean", "ratio_sim_min",
                                                            "ratio_sim_max")
        np.testing.assert_array_equal((tab["domain"] * K + tab["neighbor"]) * 12 + np.tile(np.arange(12), K * K), np.arange(K * K * 12))
        np.testing.assert_array_equal(tab["radius"], np.tile(radii, K * K))
        np.testing.assert_array_equal(tab["count"], N[0].reshape(-1))
        for name in NULL_TABLE_COLUMNS[4:]:
            np.testing.assert_allclose(np.asarray(tab[name]), st[name].reshape(-1), rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
        rows = summary[summary["timepoint"] == tp]
        np.testing.assert_allclose(np.asarray(rows["padj"]), st["padj"].reshape(-1), rtol=1e-12, atol=0, equal_nan=True)
        assert rows["relation"].tolist() == st["relation"].reshape(-1).tolist()
        np.testing.assert_array_equal(rows["n_domain"], np.repeat(sizes, K))
        png = tmp_path / "first" / f"s_{tp}_cooccurrence_null.png"
        assert png.exists() == have_matplotlib() and (not png.exists() or png.stat().st_size > 0)
