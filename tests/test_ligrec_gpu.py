"""The ligand-receptor kernels on the MI355X against the numpy restatement of their definition (tests/ligrec_ref.py, held to its
own conditions by tests/test_ligrec_cpu.py): one launch of four small time points, spots, stored counts, label values and selected
genes that straddle the label words, the wavefront and the gene chunk, the permuted labelings from the seed alone, the path that
permutes per stored entry, repeatability, the p-values, the integer counts over several runs, the refusals and the stage.

Tolerance (derived, not measured; the argument of tests/test_trends_gpu.py with all terms >= 0).  A sum of m non-negative fp64
terms in any order is within (m - 1) 2^-53 S of exact; the restatement's own sum has the same bound.  Hence |S_dev - S_ref| <=
2 (m + 2) 2^-53 S_ref with m the gene's stored entries in the time point.  Every comparison prints the largest observed multiple
of 2^-53 S_ref.  The counts c are integers and must agree exactly.

p-values.  (i) pvalue equals the formula applied by numpy to the device's own sums, exactly, in every tested cell.  (ii) pvalue
equals the restatement's in every cell that stays in the comparison: a cell drops out if some 0 < |stat_p - stat_0| lies within
the tolerance propagated from the sums (ligrec_ref.near_ties); at most 1 % of the tested cells may drop out (asserted here, and
for the restatement in forward and reversed order in test_ligrec_cpu.py; observed there: 0 of 128, 490, 144 and 12 288)."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ligrec_cases as cases
import ligrec_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
OTHER_THREADS = 768 - cases.THREADS                 # the kernel instance that is not the library's default: 256 <-> 512


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


class Counts:
    """The CSC of cases.csc on the device, with what the ligrec functions read of a DeviceCounts; time point t is called 't<t>'."""

    def __init__(self, problems):
        Vs = [V for V, _ in problems]
        colptr, ridx, vals, off = cases.csc(Vs)
        self.colptr, self.ridx, self.values = _dev(colptr), _dev(ridx), _dev(vals)
        self.tp_off_host, self.T, self.G, self.n, self.device = off, len(Vs), Vs[0].shape[1], int(off[-1]), torch.device(DEV)
        self.labels = np.concatenate([lab for _, lab in problems])
        self.perm = np.arange(self.n)
        self.tps = [f"t{t}" for t in range(self.T)]
        self.timepoint = np.repeat(np.asarray(self.tps), np.diff(off))
        self.genes = np.asarray([f"g{g}" for g in range(self.G)])


def _run(problems, K, n_perms, genes=None, seed=cases.SEED, **kw):
    """problems: [(V, lab)].  Returns (S, c) of spadot_amd.ligrec.ligrec_sums over `genes` (default: all) and the Counts."""
    from spadot_amd.ligrec import ligrec_sums
    dc = Counts(problems)
    genes = np.arange(dc.G) if genes is None else genes
    return ligrec_sums(dc, dc.values, dc.labels, genes, n_perms, seed=seed, K=K, **kw) + (dc,)


def _close(got, want, what):
    """The derived bound on every (labeling, gene, domain) and the exact counts; returns the largest observed multiple."""
    (gS, gc), (wS, wc, m) = got, want
    assert gS.shape == wS.shape and gS.dtype == np.float64, (gS.shape, wS.shape)
    err = np.abs(gS - wS)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(wS > 0, err / (U * wS), 0.0), initial=0.0))
    assert np.all(err <= ref.sum_bound(wS, m)), (what, float(err.max()))
    if gc is not None:
        assert gc.dtype == np.int32
        np.testing.assert_array_equal(gc, wc, err_msg=what)
    print(f"{what}: largest |dev - ref| = {worst:.2f} x 2^-53 S (bound {2 * (int(np.max(m, initial=0)) + 2)})")
    return worst


def _check_all(S, c, want, what):
    for t in range(len(want)):
        _close((S[t], c[t] if c is not None else None), want[t], f"{what}, time point {t}")


def test_four_time_points_in_one_launch_match_the_restatement():
    from spadot_amd.ligrec import ligrec
    call = cases.call4()
    S, c, dc = _run(call, 4, 50, seed=1)
    want = cases.want_sums(call, 4, 50, seed=1)
    assert [x.shape for x in S] == [(51, 5, 4)] * 4 and [x.shape for x in c] == [(5, 4)] * 4
    _check_all(S, c, want, "four time points")
    np.testing.assert_array_equal(S[2][:, 0], 0.0)                                   # the gene that is all zero there
    for t, (V, _) in enumerate(call):                                                # the single nonzero: its value or nothing
        assert set(np.unique(S[t][:, 2])) <= {0.0, 1.75} and np.all(S[t][:, 2].sum(axis=1) == 1.75)
    for thr in (0.0, 0.1):
        res = ligrec(dc, dc.labels, cases.CALL4_PAIRS, n_perms=50, seed=1, threshold=thr, values=dc.values)
        for t, (V, lab) in enumerate(call):
            Kt = int(lab.max()) + 1
            sizes = np.bincount(lab, minlength=Kt)
            r = res[t]
            assert r.mean.shape == (6, Kt, Kt) and r.sizes.tolist() == sizes.tolist()
            own = ref.all_cells(S[t][:, :, :Kt], c[t][:, :Kt], sizes, cases.CALL4_PAIRS, thr)         # (i) the device's own sums
            w = ref.all_cells(want[t][0][:, :, :Kt], want[t][1][:, :Kt], sizes, cases.CALL4_PAIRS, thr)
            for k in ("mean", "pvalue", "padj", "tested", "ge", "gene_mean", "gene_pct"):
                np.testing.assert_array_equal(getattr(r, k), own[k], err_msg=f"{k}, time point {t}, threshold {thr}")
            np.testing.assert_array_equal(r.tested, w["tested"])
            np.testing.assert_array_equal(np.isnan(r.mean), np.isnan(w["mean"]))
            near = ref.near_ties(want[t][0][:, :, :Kt], want[t][2], sizes, cases.CALL4_PAIRS)
            keep = r.tested & ~near
            np.testing.assert_array_equal(r.pvalue[keep], w["pvalue"][keep])
            if thr == 0.0 and t >= 2:                                                # the single nonzero ties exactly: kept, equal
                assert r.tested[2].any() and not near[2].any() and (r.ge[2][r.tested[2]] > 1).all()
                np.testing.assert_array_equal(r.pvalue[2], w["pvalue"][2])
        assert np.isnan(res[2].mean[:, 2, :]).all() and not res[2].tested[:, 2].any()                 # n = 37: domain 2 is empty
        assert not res[2].tested[0].any()                                            # gene 0 is all zero there


@pytest.mark.parametrize("n", cases.SPOTS)
def test_spots_around_the_label_words_the_wavefront_and_the_workgroup(n):
    V, lab, K = cases.spots_case(n)
    S, c, _ = _run([(V, lab)], K, 3, seed=5)
    _check_all(S, c, cases.want_sums([(V, lab)], K, 3, seed=5), f"n = {n}")


def test_stored_counts_around_the_wavefront():
    prob = cases.stored_case()
    S, c, _ = _run(prob, 6, 4, seed=2)
    _check_all(S, c, cases.want_sums(prob, 6, 4, seed=2), "stored counts")
    np.testing.assert_array_equal(S[1][:, 0], 0.0)                                   # nothing stored
    assert np.all((S[1][:, 1] != 0).sum(axis=1) == 1)                                # one stored entry: one domain holds it


@pytest.mark.parametrize("K", (1, 2, 31, 32))
def test_label_values_up_to_the_cap(K):
    V, lab, _ = cases.spots_case(200, K=K)
    for threads in (256, 512):
        S, c, _ = _run([(V, lab)], K, 2, seed=3, threads=threads)
        _check_all(S, c, cases.want_sums([(V, lab)], K, 2, seed=3), f"K = {K}, {threads} threads")
        both = S if threads == 256 else both
    np.testing.assert_array_equal(both[0], S[0])                                     # the two instances: the same bits
    wide, cw, _ = _run([(V, lab)], 32, 2, seed=3)                                    # more values than occur: zeros beyond, the same bits
    np.testing.assert_array_equal(wide[0][:, :, :K], S[0])
    assert not wide[0][:, :, K:].any() and not cw[0][:, K:].any()


def test_33_label_values_are_refused():
    V, lab, _ = cases.spots_case(200, K=33)
    assert lab.max() == 32
    with pytest.raises(ValueError, match="takes 1 to 32 label values"):
        _run([(V, lab)], 33, 2)


@pytest.fixture(scope="module")
def chunk_run():
    V, lab, K = cases.spots_case(257, K=5, G=9)
    S, c, _ = _run([(V, lab)], K, 3, seed=9)
    return V, lab, K, S, c


@pytest.mark.parametrize("ng", (1, 3, 4, 5, 9))                                      # 1, GC - 1, GC, GC + 1, 2 GC + 1 at GC = 4
def test_selected_gene_counts_around_the_chunk(chunk_run, ng):
    V, lab, K, S, c = chunk_run
    gS, gc, _ = _run([(V, lab)], K, 3, genes=np.arange(ng), seed=9, gene_chunk=4)
    _check_all(gS, gc, cases.want_sums([(V, lab)], K, 3, seed=9, genes=np.arange(ng)), f"{ng} selected genes")
    np.testing.assert_array_equal(gS[0], S[0][:, :ng])                               # the chunk is not in the bits
    np.testing.assert_array_equal(gc[0], c[0][:ng])


def test_an_unsorted_gene_list_with_gaps(chunk_run):
    V, lab, K, S, c = chunk_run
    genes = np.asarray([7, 2, 8, 0, 2, 5])
    for kw in (dict(), dict(gene_chunk=4), dict(gene_chunk=1, threads=OTHER_THREADS)):
        gS, gc, _ = _run([(V, lab)], K, 3, genes=genes, seed=9, **kw)
        np.testing.assert_array_equal(gS[0], S[0][:, genes])
        np.testing.assert_array_equal(gc[0], c[0][genes])


@pytest.fixture(scope="module")
def perm_run():
    probs = [cases.spots_case(1025, K=7), cases.call4()[2] + (4,), cases.spots_case(300, K=7)]
    probs = [(V[:, :3], lab) for V, lab, _ in probs]
    S, c, _ = _run(probs, 7, 200)
    return probs, S, c


def test_permuted_labelings_match_the_restatement_from_the_seed_alone(perm_run):
    probs, S, c = perm_run
    _check_all(S, c, cases.want_sums(probs, 7, 200), "200 permutations")
    tS, tc, _ = _run(probs, 7, 50, first=150, observed=False)
    assert tc is None
    for t in range(3):
        np.testing.assert_array_equal(tS[t], S[t][151:201])
    oS, oc, _ = _run(probs[:1], 7, 2, seed=cases.SEED + 1)
    np.testing.assert_array_equal(oS[0][0], S[0][0])                                 # another seed: the same observed sums,
    np.testing.assert_array_equal(oc[0], c[0])
    assert not np.array_equal(oS[0][1:], S[0][1:3])                                  # other permutations


def test_the_case_file_holds_the_library_defaults():
    from spadot_amd import stage_ops as ops
    assert (cases.GC, cases.THREADS) == (ops.LIGREC_GC, ops.LIGREC_THREADS) and OTHER_THREADS in (256, 512)


def test_a_problem_alone_in_a_batch_run_twice_and_into_a_poisoned_output_gives_the_same_bits(perm_run):
    probs, S, c = perm_run
    V, lab = probs[2]                                                                # n = 300, graph index 2 in the batch
    again = _run(probs, 7, 200)
    for t in range(3):
        np.testing.assert_array_equal(again[0][t], S[t])
        np.testing.assert_array_equal(again[1][t], c[t])
    rng = np.random.default_rng(8)
    wide = cases.values(rng, 37, 8)
    wide[:, 2:5] = probs[1][0]                                                       # other genes around: other places in the chunk
    alone, ac, _ = _run([(probs[1][0], probs[1][1])], 7, 20)                         # n = 37 alone is graph 0; in the batch below too
    bS, bc, _ = _run([(wide, probs[1][1]), (cases.values(rng, 300, 8), lab)], 7, 20)
    np.testing.assert_array_equal(bS[0][:, 2:5], alone[0])
    np.testing.assert_array_equal(bc[0][2:5], ac[0])
    for kw in (dict(gene_chunk=3), dict(threads=OTHER_THREADS), dict(gene_chunk=1, threads=OTHER_THREADS, lds_limit=0)):
        kS, kc, _ = _run(probs, 7, 200, **kw)
        for t in range(3):
            np.testing.assert_array_equal(kS[t], S[t], err_msg=str(kw))
            np.testing.assert_array_equal(kc[t], c[t], err_msg=str(kw))
    out = (torch.full((3, 201, 3, 7), float("nan"), dtype=torch.float64, device=DEV),
           torch.full((3, 3, 7), -5, dtype=torch.int32, device=DEV))
    pS, pc, _ = _run(probs, 7, 200, out=out)
    np.testing.assert_array_equal(pS[1], S[1])
    np.testing.assert_array_equal(out[0].cpu().numpy()[2], S[2])
    np.testing.assert_array_equal(out[1].cpu().numpy()[0], c[0])
    assert not torch.isnan(out[0]).any() and not (out[1] < 0).any()


def test_permuting_per_stored_entry_gives_the_same_bits(perm_run):
    from spadot_amd import stage_ops as ops
    probs, S, c = perm_run
    need = ops.ligrec_lds_bytes(1025, 7)
    assert need == 8 * 7 * 512 + 1040 and ops.ligrec_lds_bytes(300, 7) < need - 1
    for limit in (0, need - 1):                          # nothing at all; just below the need of n = 1025 (the others stay in LDS)
        gS, gc, _ = _run(probs, 7, 200, lds_limit=limit)
        for t in range(3):
            np.testing.assert_array_equal(gS[t], S[t])
            np.testing.assert_array_equal(gc[t], c[t])
    rng = np.random.default_rng(3)                       # n = 70000: past the LDS beside 32 x 8 accumulator columns at the default limit
    big = (cases.values(rng, 70000, 2, density=0.2), rng.integers(32, size=70000))
    big[0][:, 1] *= (2.0 ** -rng.integers(0, 40, 70000)).astype(np.float32)          # sums whose bits depend on the order
    assert ops.ligrec_lds_bytes(70000, 32, 512) > ops.LIGREC_LDS_BYTES >= ops.ligrec_lds_bytes(70000, 32, 256)
    want = cases.want_sums([big], 32, 3)
    bS, bc, _ = _run([big], 32, 3, threads=512)
    _check_all(bS, bc, want, "n = 70000, per stored entry")
    lS, lc, _ = _run([big], 32, 3, threads=256)                                      # four wavefronts: the labels fit in LDS
    np.testing.assert_array_equal(lS[0], bS[0])
    np.testing.assert_array_equal(lc[0], bc[0])


def test_labelings_split_into_runs_give_the_same_sums_and_the_same_integer_counts(perm_run, monkeypatch):
    from spadot_amd import ligrec as lr
    probs, S, c = perm_run
    dc = Counts(probs)
    pairs = np.asarray([(0, 1), (1, 2), (2, 2), (2, 0)])
    one = lr.ligrec(dc, dc.labels, pairs, n_perms=200, seed=cases.SEED, values=dc.values)
    per = 8 * 3 * 3 * 7                                                              # bytes of one labeling: T x genes x K doubles
    for cap in (per, 67 * per, 200 * per + 1):                                       # runs of 1, 67 and 200 labelings
        monkeypatch.setattr(lr, "SUMS_BYTES", cap)
        gS, gc, _ = _run(probs, 7, 200)
        for t in range(3):
            np.testing.assert_array_equal(gS[t], S[t])
            np.testing.assert_array_equal(gc[t], c[t])
        with pytest.raises(ValueError, match="one launch"):
            _run(probs, 7, 200, out=(torch.empty((3, 201, 3, 7), dtype=torch.float64, device=DEV),
                                     torch.empty((3, 3, 7), dtype=torch.int32, device=DEV)))
        got = lr.ligrec(dc, dc.labels, pairs, n_perms=200, seed=cases.SEED, values=dc.values)
        for t in range(3):
            np.testing.assert_array_equal(got[t].ge, one[t].ge)
            np.testing.assert_array_equal(got[t].pvalue, one[t].pvalue)
            np.testing.assert_array_equal(got[t].mean, one[t].mean)
    assert one[0].tested.any() and one[0].ge[one[0].tested].max() > 1


@pytest.mark.parametrize("name", [c[0] for c in cases.PVALUE_CASES])
def test_p_values_follow_the_device_sums_and_equal_the_restatement_where_no_tie_is_near(name):
    from spadot_amd.ligrec import ligrec
    V, lab, K, pairs, P = cases.pvalue_case(name)
    wS, wc, sizes, want, near = cases.pvalue_ref(name)
    S, c, dc = _run([(V, lab)], K, P)
    _close((S[0], c[0]), (wS, wc, ref.stored(V)), name)
    r = ligrec(dc, lab, pairs, n_perms=P, seed=cases.SEED, threshold=0.1, values=dc.values)[0]
    own = ref.all_cells(S[0], c[0], sizes, pairs, 0.1)                               # (i) the formula on the device's own sums
    for k in ("mean", "pvalue", "padj", "tested", "ge"):
        np.testing.assert_array_equal(getattr(r, k), own[k], err_msg=k)
    np.testing.assert_array_equal(r.tested, want["tested"])                          # (ii) the restatement's, away from near ties
    out = int((near & r.tested).sum())
    print(f"{name}: {out} of {int(r.tested.sum())} tested cells left out of the comparison")
    assert out <= 0.01 * r.tested.sum()
    keep = r.tested & ~near
    np.testing.assert_array_equal(r.pvalue[keep], want["pvalue"][keep])
    assert np.all(np.abs(r.mean - want["mean"])[r.tested] <= 4 * (V.shape[0] + 2) * U * want["mean"][r.tested])


def test_refusals_come_before_any_launch():
    from spadot_amd import stage_ops as ops
    from spadot_amd.ligrec import ligrec_sums
    V, lab = cases.call4()[2]
    dc = Counts([(V, lab)])
    out = (torch.full((1, 4, 5, 4), -77.0, dtype=torch.float64, device=DEV), torch.full((1, 5, 4), -77, dtype=torch.int32, device=DEV))

    def call(counts=dc, labels=None, genes=np.arange(5), P=3, K=4, **kw):
        return ligrec_sums(counts, counts.values, dc.labels if labels is None else labels, genes, P, K=K, out=out, **kw)

    with pytest.raises(RuntimeError, match="MI355X only"):
        ligrec_sums(dc, dc.values.cpu(), dc.labels, np.arange(5), 3, K=4, out=out)
    with pytest.raises(RuntimeError, match="MI355X only"):
        call(labels=torch.as_tensor(dc.labels.astype(np.uint8)))
    with pytest.raises(ValueError, match=r"holds the label 3: labels must lie in 0 \.\. 2"):
        call(K=3)
    neg = Counts([(V, lab)])
    neg.ridx = neg.ridx.clone()
    neg.ridx[3] = 37
    with pytest.raises(ValueError, match=r"row indices 0 \.\. 37: they must lie in 0 \.\. 36"):
        call(counts=neg)
    neg.ridx[3] = -1
    with pytest.raises(ValueError, match=r"row indices -1 \.\. 36"):
        call(counts=neg)
    bad = Counts([(V, lab)])
    bad.colptr = bad.colptr.clone()
    bad.colptr[2] = bad.colptr[1] - 1
    with pytest.raises(ValueError, match="colptr must ascend"):
        call(counts=bad)
    with pytest.raises(ValueError, match="below 2\\^32"):
        call(first=2 ** 32 - 2)
    with pytest.raises(ValueError, match="must not be negative"):
        call(P=-1)
    with pytest.raises(ValueError, match="at least one labeling"):
        call(P=0, observed=False)
    with pytest.raises(ValueError, match=r"selected genes 0 \.\. 5 must lie in 0 \.\. 4"):
        call(genes=np.asarray([0, 5, 1, 2, 3]))
    with pytest.raises(ValueError, match=r"selected genes -1 \.\. 3"):
        call(genes=np.asarray([0, -1, 1, 2, 3]))
    with pytest.raises(ValueError, match="lds_limit"):
        call(lds_limit=-1)
    with pytest.raises(ValueError, match="outside its limits"):
        call(threads=1024)
    torch.cuda.synchronize()
    assert torch.all(out[0] == -77.0) and torch.all(out[1] == -77)                   # nothing was launched
    S, c = call(seed=cases.SEED)                                                     # and the same tensors are written by a valid call
    _close((S[0], c[0]), cases.want_sums([(V, lab)], 4, 3)[0], "after the refusals")
    np.testing.assert_array_equal(out[0].cpu().numpy()[0], S[0])


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from spadot_amd.ligrec import interactions
    out = str(tmp_path_factory.mktemp("ligrec"))
    counts, domains, pairs = cases.stage_files(out)
    res = interactions(argparse.Namespace(data=counts, domains=domains, interactions=pairs, output_dir=out, prefix="s_", n_perms=100,
                                          seed=3, threshold=0.1, top=20, device=DEV))
    return (counts, domains, pairs), out, res


def test_the_stage_writes_its_files(stage):
    import pandas as pd
    from spadot_amd.ligrec import FIELDS, TABLE_COLUMNS, ligrec, ligrec_sums, ligrec_table, read_interactions
    from spadot_amd.markers import load_marker_counts, read_domains
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.trends import lognorm_values
    (counts, domains, pairs_csv), out, res = stage
    spec = {tp: (n, K) for tp, n, K in cases.STAGE_TPS}
    tps = res["timepoints"]                                                          # in order of first appearance in the data
    assert sorted(tps) == sorted(spec) and set(res["timings"]) == {"read_s", "device_s", "write_s", "total_s"}
    raw = load_marker_counts(counts)[0]
    labels = read_domains(domains, raw.obs["timepoint"])
    pairs = read_interactions(pairs_csv, raw.var_names)
    assert pairs.tolist() == [[0, 1], [1, 0], [2, 3], [4, 4], [5, 10], [12, 13], [14, 23], [2, 12]]
    dc = DeviceCounts(raw, DEV)
    values = lognorm_values(dc)
    want = ligrec(dc, labels, pairs, n_perms=100, seed=3, threshold=0.1)
    sel = np.unique(pairs)
    z = np.load(os.path.join(out, "s_ligrec.npz"))
    assert z["timepoints"].tolist() == tps and z["genes"].tolist() == [f"g{g:02d}" for g in sel]
    assert z["sources"].tolist() == [f"g{g:02d}" for g in pairs[:, 0]] and z["targets"].tolist() == [f"g{g:02d}" for g in pairs[:, 1]]
    assert (int(z["n_perms"]), int(z["seed"]), float(z["threshold"])) == (100, 3, 0.1)
    lab = labels[dc.perm]
    S, c = ligrec_sums(dc, values, lab, sel, 100, seed=3)
    X = np.zeros((dc.n, dc.G), dtype=np.float32)                                     # the device's own fp32 values, dense
    colptr, ridx = dc.colptr.cpu().numpy(), dc.ridx.cpu().numpy()
    X[ridx, np.repeat(np.arange(dc.G), np.diff(colptr))] = values.cpu().numpy()
    off = dc.tp_off_host
    pos = np.searchsorted(sel, pairs)
    assert [str(t) for t in dc.tps] == tps
    for t, tp in enumerate(tps):
        n, K = spec[tp]
        w = want[t]
        assert w.mean.shape == (8, K, K) and w.sizes.sum() == n
        for name in FIELDS:
            np.testing.assert_array_equal(z[f"{tp}_{name}"], getattr(w, name), err_msg=f"{tp}_{name}")
            np.testing.assert_array_equal(getattr(res["results"][tp], name), getattr(w, name), err_msg=f"{tp}_{name}")
        V, lt = X[int(off[t]):int(off[t + 1])][:, sel], lab[int(off[t]):int(off[t + 1])]
        wS = ref.sums(V, ref.labelings(lt, 100, 3, t), K)                            # the restatement on the device's values
        _close((S[t][:, :, :K], c[t][:, :K]), (wS, ref.positive_counts(V, lt, K), ref.stored(V)), f"stage, {tp}")
        own = ref.all_cells(S[t][:, :, :K], c[t][:, :K], w.sizes, pos, 0.1)
        for name in ("mean", "pvalue", "padj", "tested", "ge"):
            np.testing.assert_array_equal(getattr(w, name), own[name], err_msg=f"{tp} {name}")
        assert w.pvalue[0, 0, 1] == 1 / 101 and w.padj[0, 0, 1] < 0.05               # g00 marks domain 0, g01 domain 1
        assert not w.tested[6].any()                                                 # g23 is never counted
        tab = pd.read_csv(os.path.join(out, f"s_ligrec_{tp}.csv"))
        assert tuple(tab.columns) == TABLE_COLUMNS and len(tab) == 20
        full = ligrec_table(w, 0)
        assert len(full) == int(w.tested.sum()) and tab["source"].tolist() == full["source"].tolist()[:20]
        np.testing.assert_allclose(tab["mean"], full["mean"][:20], rtol=1e-12)
        np.testing.assert_allclose(tab["padj"], full["padj"][:20], rtol=1e-12)
        assert np.all(np.diff(tab["pvalue"]) >= 0) and tab["pvalue"][0] == pytest.approx(1 / 101)


def test_a_second_run_and_the_sub_command_write_the_same_bytes(stage, tmp_path):
    from spadot_amd.ligrec import interactions
    (counts, domains, pairs), out, res = stage
    names = ["s_ligrec.npz"] + [f"s_ligrec_{tp}.csv" for tp in res["timepoints"]]
    interactions(argparse.Namespace(data=counts, domains=domains, interactions=pairs, output_dir=str(tmp_path), prefix="s_",
                                    n_perms=100, seed=3, threshold=0.1, top=20, device=DEV))
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(tmp_path, name), "rb").read(), name
    sub = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "spadot_amd", "ligrec", "-i", counts, "--domains", domains, "--interactions", pairs,
                        "-o", str(sub), "--prefix", "s_", "--n_perms", "100", "--seed", "3", "--top", "20", "--device", DEV],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "dropped 2 of 10 interactions (1 duplicates, 1 with a gene" in r.stderr
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(sub, name), "rb").read(), name
    other = interactions(argparse.Namespace(data=counts, domains=domains, interactions=pairs, output_dir=str(tmp_path / "seed4"),
                                            prefix="", n_perms=100, seed=4, threshold=0.1, top=0, device=DEV))
    a, b = other["results"]["E12"], res["results"]["E12"]
    np.testing.assert_array_equal(a.mean, b.mean)
    np.testing.assert_array_equal(a.tested, b.tested)
    assert not np.array_equal(a.ge, b.ge) and not np.array_equal(a.pvalue[b.tested], b.pvalue[b.tested])
    assert len(other["tables"]["E12"]) == int(b.tested.sum())                        # top = 0: every tested cell
