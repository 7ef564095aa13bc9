"""The spatial-autocorrelation kernel on the MI355X against the numpy restatement of its definition (tests/autocorr_ref.py, held to
its own conditions by tests/test_autocorr_cpu.py): the edge call, graphs, gene counts and stored counts that straddle a wavefront,
the workgroup and the gene group, the permuted labelings from the seed alone, the path that keeps its image in global memory,
repeatability, the p-values, the dense columns, the graph moments, the refusals and the stage.  The restatement is evaluated on
the values and the centre the device was given.

Tolerance (derived, not measured; the argument of tests/test_trends_gpu.py).  A sum of E fp64 terms in any order is within
(E - 1) 2^-53 A of exact, A = sum |terms|; the centring and the product (one subtraction each, one fma) add a few ulps per term;
the restatement's own sum has the same bound.  Hence |N_dev - N_ref| <= 4 (E + 2) 2^-53 sum_e |z_i z_j| and |D_dev - D_ref| <=
4 (E + 2) 2^-53 D_ref.  Every comparison prints the largest observed multiple of 2^-53 A.  The package's m2 is S2 - S1^2 / n from
fixed-order fp64 sums, within 8 n 2^-53 sum v^2 of the restatement's sum (v - c)^2, which bounds the comparison of I and C.
There is no 16-bit table in this implementation (a stored entry finds its spot by the inverse permutation), so the n = 65537
case of a table's threshold does not exist; a graph beyond the LDS image (n = 20300) is run instead."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import autocorr_cases as cases
import autocorr_ref as ref
import nhood_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


class Counts:
    """The CSC of cases.csc on the device, with what autocorr_sums reads of a DeviceCounts."""

    def __init__(self, Vs):
        colptr, ridx, vals, off = cases.csc(Vs)
        self.colptr, self.ridx, self.values = _dev(colptr), _dev(ridx), _dev(vals)
        self.tp_off_host, self.T, self.G, self.n, self.device = off, len(Vs), Vs[0].shape[1], int(off[-1]), torch.device(DEV)
        self.centre = np.stack([cases.centres(V) for V in Vs])


def _run(problems, n_perms, seed=cases.SEED, **kw):
    """problems: [(src, dst, V)].  Returns (N, D) of spadot_amd.autocorr.autocorr_sums and the Counts."""
    from spadot_amd.autocorr import autocorr_sums
    dc = Counts([V for _, _, V in problems])
    edges = [(_dev(s, torch.int32), _dev(d, torch.int32)) for s, d, _ in problems]
    return autocorr_sums(edges, dc, dc.values, dc.centre, n_perms, seed=seed, **kw) + (dc,)


def _close(got, want, E, what):
    """The derived bound on every (gene, labeling); returns the largest observed multiple of 2^-53 A."""
    (gN, gD), (wN, wD, wA) = got, want
    assert gN.shape == wN.shape and gD.shape == wD.shape and gN.dtype == np.float64
    worst = 0.0
    for g, w, A in ((gN, wN, wA), (gD, wD, wD)):
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(A > 0, err / (U * A), 0.0), initial=0.0)))
        assert np.all(err <= 4.0 * (E + 2) * U * A), (what, float(err.max()))
    print(f"{what}: largest |dev - ref| = {worst:.2f} x 2^-53 A (bound {4 * (E + 2)})")
    return worst


def _want(problems, n_perms, seed=cases.SEED, **kw):
    return [ref.all_sums_genes(s, d, V, cases.centres(V), n_perms, seed, t, **kw) for t, (s, d, V) in enumerate(problems)]


def test_edge_call_matches_the_restatement():
    from spadot_amd.autocorr import autocorr_stats
    call = cases.edge_call()
    N, D, dc = _run(call, 10, seed=1)
    want = _want(call, 10, seed=1)
    assert [x.shape for x in N] == [(4, 11)] * 4
    for t, (src, dst, V) in enumerate(call):
        n, E = V.shape[0], src.shape[0]
        _close((N[t], D[t]), want[t], E, f"edge call, time point {t}")
        sp = np.array([ref.spread(V[:, g], dc.centre[t, g]) for g in range(4)])
        mom = ref.graph_moments(src, dst, n) if E else (0, 0, 0)
        w = ref.stats(want[t][0], want[t][1], n, E, sp[:, 0], sp[:, 1], mom)
        g = autocorr_stats(N[t], D[t], n, E, sp[:, 0], mom, sumsq=sp[:, 1])
        assert g["degenerate"].tolist() == w["degenerate"].tolist() == ([True] * 4 if n < 3 else [t == 2, False, False, True])
        for k in ref.FIELDS:
            np.testing.assert_array_equal(np.isnan(g[k]), np.isnan(w[k]), err_msg=f"{t} {k}")
        fam = ~w["degenerate"]
        for s in ("I", "C"):
            assert np.isnan(g[f"padj_{s}"][~fam]).all()
            if fam.any():
                np.testing.assert_allclose(g[f"padj_{s}"][fam], ref.bh(g[f"p_sim_{s}"][fam]), rtol=1e-12)
    assert not N[0].any() and not D[0].any()                                         # n = 1: no edges
    np.testing.assert_array_equal(N[2][0], 0.0)                                      # the gene that is all zero there, c = 0
    np.testing.assert_array_equal(D[3][3], 0.0)                                      # the constant gene: no differences
    assert np.all(np.abs(N[3][3]) <= 1800 * (300 * U * 0.7) ** 2)                    # and products of the rounding residue of c


@pytest.mark.parametrize("name", [c[0] for c in cases.TILE_CASES])
def test_tile_edges_match_the_restatement(name):
    src, dst, V = cases.tile_case(name)
    N, D, _ = _run([(src, dst, V)], 3, seed=5)
    _close((N[0], D[0]), _want([(src, dst, V)], 3, seed=5)[0], src.shape[0], name)
    if src.shape[0] == 0:
        assert not N[0].any() and not D[0].any()


@pytest.mark.parametrize("G", cases.GROUP_SIZES)
def test_gene_counts_around_the_group_match_the_restatement(G):
    src, dst, V = cases.tile_case("n257_E1537", G=G)
    N, D, _ = _run([(src, dst, V)], 2, seed=9)
    assert N[0].shape == (G, 3)
    _close((N[0], D[0]), _want([(src, dst, V)], 2, seed=9)[0], src.shape[0], f"G = {G}")
    if G > 2:                                                                        # a range of genes: the same bits
        Ns, Ds, _ = _run([(src, dst, V)], 2, seed=9, genes=(1, G - 1))
        np.testing.assert_array_equal(Ns[0], N[0][1:G - 1])
        np.testing.assert_array_equal(Ds[0], D[0][1:G - 1])


def test_stored_counts_around_the_wavefront_and_the_workgroup():
    prob = cases.stored_case()
    N, D, _ = _run(prob, 4, seed=2)
    want = _want(prob, 4, seed=2)
    for t in range(2):
        _close((N[t], D[t]), want[t], prob[t][0].shape[0], f"stored counts, time point {t}")
    np.testing.assert_array_equal(N[1][0], 0.0)                                      # nothing stored: x = 0 = c everywhere
    np.testing.assert_array_equal(D[1][0], 0.0)


@pytest.fixture(scope="module")
def perm_run():
    graphs, want = cases.perm_case()
    N, D, _ = _run(graphs, 200)
    return graphs, want, N, D


def test_permuted_labelings_match_the_restatement_from_the_seed_alone(perm_run):
    graphs, want, N, D = perm_run
    for t, (src, _, _) in enumerate(graphs):
        _close((N[t], D[t]), want[t], src.shape[0], f"200 permutations, graph {t}")
    tN, tD, _ = _run(graphs, 50, first=150, observed=False)
    for t in range(3):
        np.testing.assert_array_equal(tN[t], N[t][:, 151:201])
        np.testing.assert_array_equal(tD[t], D[t][:, 151:201])
    oN, _, _ = _run(graphs[:1], 2, seed=cases.SEED + 1)
    np.testing.assert_array_equal(oN[0][:, 0], N[0][:, 0])                           # another seed: the same observed sums,
    assert not np.array_equal(oN[0][:, 1:], N[0][:, 1:3])                            # other permutations


def test_the_case_file_holds_the_library_defaults():
    from spadot_amd import stage_ops as ops
    assert (cases.GS, cases.THREADS) == (ops.AUTOCORR_GS, ops.AUTOCORR_THREADS)


def test_labelings_split_into_runs_that_share_one_scratch_buffer_give_the_same_bits(perm_run, monkeypatch):
    from spadot_amd import autocorr, stage_ops as ops
    graphs, want, N, D = perm_run
    probs = graphs[1:]                                                               # n = 37 and n = 300, graph indices 0 and 1
    one = _run(probs, 7, lds_limit=0)
    tail = _run(probs, 5, first=2, observed=False, lds_limit=0)
    per = 2 * -(-3 // cases.GS) * ((cases.GS * 300 + 3) & ~3)                                               # floats of one labeling: T x groups x slab
    desc = np.array([[0, 37, 0, 0, 0, 0, 0], [0, 300, 0, 37, 1, 0, 0]], dtype=np.int64)
    assert ops.autocorr_scratch_floats(desc, 3, 1, 0) == per
    for cap in (per, 3 * per, 8 * per - 1):                                          # runs of 1 (the first has P = 0), 3 and 7 labelings
        monkeypatch.setattr(autocorr, "SCRATCH_FLOATS", cap)
        got = _run(probs, 7, lds_limit=0)
        part = _run(probs, 5, first=2, observed=False, lds_limit=0)
        for t in range(2):
            for i in range(2):
                np.testing.assert_array_equal(got[i][t], one[i][t])
                np.testing.assert_array_equal(part[i][t], tail[i][t])
                np.testing.assert_array_equal(part[i][t], one[i][t][:, 3:8])
        with pytest.raises(ValueError, match="one launch"):
            _run(probs, 7, lds_limit=0, out=tuple(torch.empty((2, 3, 8), dtype=torch.float64, device=DEV) for _ in range(2)))


def test_the_image_in_global_memory_gives_the_same_bits(perm_run):
    graphs, want, N, D = perm_run
    for limit in (0, 2048 + 4 * cases.GS * 300 - 1):               # nothing at all; just below the need of n = 300 (n = 37 stays in LDS)
        gN, gD, _ = _run(graphs, 200, lds_limit=limit)
        for t in range(3):
            np.testing.assert_array_equal(gN[t], N[t])
            np.testing.assert_array_equal(gD[t], D[t])
    rng = np.random.default_rng(3)                       # n = 20300: past the LDS image at the default limit
    big = nc.random_edges(rng, 20300, 121800) + (cases.random_values(rng, 20300, 2),)
    assert 2048 + 4 * cases.GS * 20300 > 163840
    bN, bD, _ = _run([big], 2)
    _close((bN[0], bD[0]), _want([big], 2)[0], 121800, "n = 20300")


def test_a_problem_alone_in_a_batch_run_twice_and_into_a_poisoned_output_gives_the_same_bits(perm_run):
    graphs, want, N, D = perm_run
    src, dst, V = graphs[1]                                                          # n = 37, three genes
    aN, aD, _ = _run([(src, dst, V)], 20)
    again = _run([(src, dst, V)], 20)
    np.testing.assert_array_equal(again[0][0], aN[0])
    np.testing.assert_array_equal(again[1][0], aD[0])
    rng = np.random.default_rng(8)
    wide = cases.random_values(rng, 37, 8)
    wide[:, 2:5] = V                                                                 # other genes around: other groups
    other = nc.random_edges(rng, 300, 1800) + (cases.random_values(rng, 300, 8),)
    bN, bD, dc = _run([(src, dst, wide), other], 20)
    np.testing.assert_array_equal(bN[0][2:5], aN[0])
    np.testing.assert_array_equal(bD[0][2:5], aD[0])
    for kw in (dict(gs=6 - cases.GS), dict(gs=6 - cases.GS, lds_limit=0)):                                 # the group size is not in the bits
        kN, kD, _ = _run([(src, dst, wide), other], 20, **kw)
        np.testing.assert_array_equal(kN[0], bN[0])
        np.testing.assert_array_equal(kD[1], bD[1])
    out = tuple(torch.full((2, 8, 21), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
    pN, pD, _ = _run([(src, dst, wide), other], 20, out=out)
    np.testing.assert_array_equal(pN[1], bN[1])
    np.testing.assert_array_equal(out[1].cpu().numpy()[0], bD[0])
    assert not torch.isnan(out[0]).any() and not torch.isnan(out[1]).any()


def test_p_values_follow_the_device_sums_and_equal_the_restatement_where_no_tie_is_near():
    from spadot_amd.autocorr import autocorr_stats
    src, dst, V = cases.planted_genes()
    wN, wD, wA, clear = cases.planted_sums()
    N, D, dc = _run([(src, dst, V)], cases.PLANTED_PERMS)
    _close((N[0], D[0]), (wN, wD, wA), 2400, "planted genes")
    sp = np.array([ref.spread(V[:, g], dc.centre[0, g]) for g in range(6)])
    mom = (2400, 4544, 58240)
    got = autocorr_stats(N[0], D[0], 400, 2400, sp[:, 0], mom, sumsq=sp[:, 1])
    np.testing.assert_array_equal(got["p_sim_I"], (1 + (N[0][:, 1:] >= N[0][:, :1]).sum(1)) / 201)
    np.testing.assert_array_equal(got["p_sim_C"], (1 + (D[0][:, 1:] <= D[0][:, :1]).sum(1)) / 201)
    want = ref.stats(wN, wD, 400, 2400, sp[:, 0], sp[:, 1], mom)
    assert clear.tolist() == [True] * 5 + [False]                                    # the single nonzero ties exactly: excluded
    for k in ("p_sim_I", "p_sim_C"):
        np.testing.assert_array_equal(got[k][clear], want[k][clear], err_msg=k)
    assert np.all(np.abs(got["I"] - want["I"]) <= 400 / (2400 * sp[:, 0]) * cases.bound_N(2400, wA[:, 0]))       # the same m2


def _stat_bound(r, V, A, stat):
    """|I_dev - I_ref| (or C) from the bounds of the sums and of m2 (module docstring)."""
    n, E = r.n, r.E
    sumsq = (V.astype(np.float64) ** 2).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):                            # a degenerate gene: the caller leaves it out
        scale = n / (E * r.m2) if stat == "I" else (n - 1.0) / (2.0 * E * r.m2)
        return np.abs(getattr(r, stat)) * 2.0 * (8.0 * n * U * sumsq / r.m2) + scale * 4.0 * (E + 2) * U * A + 1e-300


def test_dense_columns_take_the_same_kernel_and_give_the_same_numbers():
    from spadot_amd.autocorr import spatial_autocorr
    src, dst, V = cases.planted_genes()
    rng = np.random.default_rng(12)
    s2, d2 = nc.random_edges(rng, 300, 1800)
    V2 = cases.random_values(rng, 300, 6, density=0.5)
    problems = [(src, dst, V), (s2, d2, V2)]
    edges = [(_dev(s, torch.int32), _dev(d, torch.int32)) for s, d, _ in problems]
    res = spatial_autocorr(edges, [_dev(V.astype(np.float64)), _dev(V2)], n_perms=30, seed=cases.SEED)
    from spadot_amd.autocorr import autocorr_sums
    dc = Counts([V, V2])                                                             # zeros not stored, the same centre
    N, D = autocorr_sums(edges, dc, dc.values, np.stack([r.mean for r in res]), 30, seed=cases.SEED)
    for t, (s, d, W) in enumerate(problems):
        r = res[t]
        np.testing.assert_array_equal(r.N, N[t])
        np.testing.assert_array_equal(r.D, D[t])
        assert (r.S0, r.S1, r.S2) == ref.graph_moments(s, d, W.shape[0]) and np.all(r.pct == 1.0)
        wN, wD, wA = ref.all_sums_genes(s, d, W, r.mean, 30, cases.SEED, t)
        _close((r.N, r.D), (wN, wD, wA), s.shape[0], f"dense columns, time point {t}")
        sp = np.array([ref.spread(W[:, g], r.mean[g]) for g in range(6)])
        np.testing.assert_allclose(r.mean, cases.centres(W), rtol=4 * W.shape[0] * U)
        assert np.all(np.abs(r.m2 - sp[:, 0]) <= 8 * W.shape[0] * U * sp[:, 1])
        want = ref.stats(wN, wD, W.shape[0], s.shape[0], sp[:, 0], sp[:, 1], (r.S0, r.S1, r.S2))
        assert not r.degenerate.any() and not want["degenerate"].any()
        assert np.all(np.abs(r.I - want["I"]) <= _stat_bound(r, W, wA[:, 0], "I"))
        assert np.all(np.abs(r.C - want["C"]) <= _stat_bound(r, W, wD[:, 0], "C"))
        np.testing.assert_allclose(r.z_norm_I, want["z_norm_I"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r.p_norm_C, want["p_norm_C"], rtol=1e-6, atol=1e-300)


def test_graph_moments_against_the_dense_form():
    from spadot_amd.autocorr import graph_moments
    call = cases.edge_call()
    for src, dst, V in call[1:]:
        n = V.shape[0]
        assert graph_moments(_dev(src, torch.int32), _dev(dst, torch.int32), n) == ref.graph_moments_dense(src, dst, n)
    _, _, src, dst, _ = nc.planted(20)
    assert graph_moments(_dev(src, torch.int32), _dev(dst, torch.int32), 400) == (2400, 4544, 58240)
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    assert graph_moments(empty, empty, 5) == (0, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        graph_moments(torch.as_tensor(src), torch.as_tensor(dst), 400)


def _desc(n=37, E=150, row0=0, gid=0, lo=0, hi=36):
    return np.array([[0, n, E, row0, gid, lo, hi]], dtype=np.int64)


def test_refusals_come_before_any_launch():
    from spadot_amd import stage_ops as ops
    from spadot_amd.autocorr import autocorr_sums
    src, dst, V = cases.edge_call()[2]
    dc = Counts([V])
    e = (_dev(src, torch.int32), _dev(dst, torch.int32))
    out = tuple(torch.full((1, 4, 4), float(-77.0), dtype=torch.float64, device=DEV) for _ in range(2))

    def call(edges=e, counts=dc, P=3, **kw):
        return autocorr_sums([edges], counts, counts.values, counts.centre, P, out=out, **kw)

    bad = dst.copy()
    bad[7] = 37
    with pytest.raises(ValueError, match=r"edge ends 0 \.\. 37: they must lie in 0 \.\. 36"):
        call(edges=(e[0], _dev(bad, torch.int32)))
    bad[7] = -1
    with pytest.raises(ValueError, match="edge ends -1"):
        call(edges=(e[0], _dev(bad, torch.int32)))
    neg = Counts([V])
    neg.ridx = neg.ridx.clone()
    neg.ridx[3] = -1
    with pytest.raises(ValueError, match=r"row indices -1 \.\. 36"):
        call(counts=neg)
    neg.ridx[3] = 37
    with pytest.raises(ValueError, match=r"row indices 0 \.\. 37: they must lie in 0 \.\. 36"):
        call(counts=neg)
    wide = torch.as_tensor(dst, dtype=torch.int64, device=DEV)
    wide[7] = 2 ** 32 + 5                                                            # would wrap to 5 as an int32
    with pytest.raises(ValueError, match=r"edge ends \d+ \.\. 4294967301: they must lie in 0 \.\. 36"):
        call(edges=(e[0].long(), wide))
    with pytest.raises(ValueError, match="must not be negative"):
        call(P=-1)
    with pytest.raises(ValueError, match="below 2\\^32"):
        call(first=2 ** 32 - 2)
    with pytest.raises(ValueError, match="at least one labeling"):
        call(P=0, observed=False)
    with pytest.raises(ValueError, match="contiguous range"):
        call(genes=(2, 5))
    with pytest.raises(RuntimeError, match="MI355X only"):
        call(edges=(torch.as_tensor(src), torch.as_tensor(dst)))
    with pytest.raises(RuntimeError, match="MI355X only"):
        autocorr_sums([e], dc, dc.values.cpu(), dc.centre, 3, out=out)
    with pytest.raises(ValueError, match="lds_limit"):
        call(lds_limit=-1)
    with pytest.raises(ValueError, match="outside its limits"):
        call(threads=128)
    cen = _dev(dc.centre)
    for desc, what in ((_desc(n=2 ** 31), "spots"), (_desc(E=2 ** 31), "edges"), (_desc(row0=-1), "inconsistent")):
        with pytest.raises(ValueError, match=what):
            ops.autocorr_sums(e[0], e[1], dc.colptr, dc.ridx, dc.values, cen, desc, 0, 4, True, 0, 3, out=out)
    torch.cuda.synchronize()
    assert all(torch.all(o == -77.0) for o in out)                                   # nothing was launched

    lib = ops.model_lib()                                                            # the library's own checks, from the host descriptor

    def raw(desc, nnz=int(dc.ridx.numel()), lo=0, hi=36, T=1, G=4, g0=0, ng=4, observed=1, first=0, P=3, lds=163840, threads=0,
            gs=0, N=out[0].data_ptr(), scratch=None, floats=0):
        ddev = _dev(desc)
        return lib.spadot_autocorr_sums(e[0].data_ptr(), e[1].data_ptr(), dc.colptr.data_ptr(), dc.ridx.data_ptr(),
                                        dc.values.data_ptr(), nnz, lo, hi, cen.data_ptr(), ctypes.c_void_p(desc.ctypes.data),
                                        ddev.data_ptr(), T, G, g0, ng, observed, first, P, 0, lds, scratch, floats, threads, gs,
                                        N, out[1].data_ptr(), None)

    for kw in (dict(desc=_desc(n=2 ** 31)), dict(desc=_desc(E=2 ** 31)), dict(desc=_desc(hi=37)), dict(desc=_desc(lo=-1)),
               dict(desc=_desc(gid=2 ** 31)), dict(desc=_desc(), hi=37), dict(desc=_desc(), lo=-1), dict(desc=_desc(), ng=5),
               dict(desc=_desc(), first=2 ** 32 - 2), dict(desc=_desc(), threads=128), dict(desc=_desc(), gs=3),
               dict(desc=_desc(), P=2 ** 31)):
        assert raw(**kw) == -7, kw
    for kw in (dict(desc=_desc(n=0)), dict(desc=_desc(E=-1)), dict(desc=_desc(row0=-1)), dict(desc=_desc(), P=-1),
               dict(desc=_desc(), observed=0, P=0), dict(desc=_desc(), N=None), dict(desc=_desc(), ng=0), dict(desc=_desc(), T=0),
               dict(desc=_desc(), lds=-1), dict(desc=_desc(), lds=0), dict(desc=_desc(), nnz=-1)):
        assert raw(**kw) == -22, kw                                                  # lds = 0 without a scratch buffer among them
    torch.cuda.synchronize()
    assert all(torch.all(o == -77.0) for o in out)
    N, D = call(seed=cases.SEED)                                                     # and the same tensors are written by a valid call
    want = ref.all_sums_genes(src, dst, V, dc.centre[0], 3, cases.SEED, 0)
    _close((N[0], D[0]), want, src.shape[0], "after the refusals")
    np.testing.assert_array_equal(out[0].cpu().numpy()[0], N[0])
    np.testing.assert_array_equal(out[1].cpu().numpy()[0], D[0])


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from spadot_amd.autocorr import autocorr
    out = tmp_path_factory.mktemp("autocorr")
    path = cases.stage_counts(os.path.join(out, "counts.npz"))
    res = autocorr(argparse.Namespace(data=path, output_dir=str(out), prefix="s_", k=6, n_perms=100, seed=3, top=15, device=DEV))
    return path, str(out), res


def test_the_stage_writes_its_files(stage):
    import pandas as pd
    from spadot_amd.autocorr import ARRAYS, TABLE_COLUMNS, spatial_autocorr
    from spadot_amd.markers import load_marker_counts
    from spadot_amd.neighbors import spatial_edges
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.trends import lognorm_values
    path, out, res = stage
    tps = ["E10", "E12", "E14"]
    assert res["timepoints"] == tps and set(res["timings"]) == {"read_s", "graph_s", "device_s", "write_s", "total_s"}
    assert TABLE_COLUMNS == ("gene", "I", "C", "z_norm_I", "p_norm_I", "z_sim_I", "p_sim_I", "padj_I", "z_norm_C", "p_norm_C",
                             "z_sim_C", "p_sim_C", "padj_C", "mean", "pct")
    dc = DeviceCounts(load_marker_counts(path)[0], DEV)
    assert [str(t) for t in dc.tps] == tps and dc.G == 40
    off = dc.tp_off_host
    edges = [spatial_edges(dc.spatial[int(off[t]):int(off[t + 1])], 6, DEV) for t in range(3)]
    values = lognorm_values(dc)
    want = spatial_autocorr(edges, dc, values, n_perms=100, seed=3)
    z = np.load(os.path.join(out, "s_autocorr.npz"))
    assert z["timepoints"].tolist() == tps and z["genes"].tolist() == [f"g{g:02d}" for g in range(40)]
    assert (int(z["k"]), int(z["n_perms"]), int(z["seed"])) == (6, 100, 3)
    X = np.zeros((dc.n, 40), dtype=np.float32)                                       # the device's own fp32 values, dense
    colptr, ridx = dc.colptr.cpu().numpy(), dc.ridx.cpu().numpy()
    X[ridx, np.repeat(np.arange(40), np.diff(colptr))] = values.cpu().numpy()
    for t, (tp, w) in enumerate(zip(tps, want)):
        n = int(off[t + 1] - off[t])
        assert (w.n, w.E) == (n, 6 * n) and w.N.shape == (40, 101)
        for name in ARRAYS:
            np.testing.assert_array_equal(z[f"{tp}_{name}"], getattr(w, name), err_msg=f"{tp}_{name}")
            np.testing.assert_array_equal(getattr(res["results"][tp], name), getattr(w, name), err_msg=f"{tp}_{name}")
        s, d = edges[t][0].cpu().numpy(), edges[t][1].cpu().numpy()
        assert (int(z[f"{tp}_S0"]), int(z[f"{tp}_S1"]), int(z[f"{tp}_S2"])) == ref.graph_moments(s, d, n)
        V = X[int(off[t]):int(off[t + 1])]
        wN, wD, wA = ref.all_sums_genes(s, d, V, w.mean, 5, 3, t)                    # the restatement on the device's values
        _close((w.N[:, :6], w.D[:, :6]), (wN, wD, wA), 6 * n, f"stage, {tp}")
        np.testing.assert_allclose(w.mean, cases.centres(V), rtol=4 * n * U, atol=0)
        np.testing.assert_array_equal(w.pct, (V != 0).mean(0))
        assert w.degenerate.tolist() == [False] * 39 + [True] and np.isnan(w.I[39]) and np.isnan(w.padj_I[39])
        sp = np.array([ref.spread(V[:, g], w.mean[g]) for g in range(40)])
        wI = n * wN[:, 0] / (6 * n * sp[:, 0].clip(1e-300))
        assert np.all(np.abs(w.I - wI)[:39] <= _stat_bound(w, V, wA[:, 0], "I")[:39])
        tab = pd.read_csv(os.path.join(out, f"s_autocorr_{tp}.csv"))
        assert tuple(tab.columns) == TABLE_COLUMNS and len(tab) == 15
        order = np.lexsort((np.arange(40), -np.where(np.isnan(w.I), -np.inf, w.I)))[:15]
        assert tab["gene"].tolist() == [f"g{g:02d}" for g in order]
        np.testing.assert_allclose(tab["I"], w.I[order], rtol=1e-12)
        np.testing.assert_allclose(tab["padj_C"], w.padj_C[order], rtol=1e-12)
        assert np.all(np.diff(tab["I"]) <= 0) and set(order) <= set(range(20))      # the planted genes lead the table
        assert np.all(w.p_sim_I[order] == 1 / 101)


def test_a_second_run_and_the_sub_command_write_the_same_bytes(stage, tmp_path):
    from spadot_amd.autocorr import autocorr
    path, out, res = stage
    names = ["s_autocorr.npz"] + [f"s_autocorr_{tp}.csv" for tp in res["timepoints"]]
    autocorr(argparse.Namespace(data=path, output_dir=str(tmp_path), prefix="s_", k=6, n_perms=100, seed=3, top=15, device=DEV))
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(tmp_path, name), "rb").read(), name
    sub = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "spadot_amd", "autocorr", "-i", path, "-o", str(sub), "--prefix", "s_",
                        "--n_perms", "100", "--seed", "3", "--top", "15", "--device", DEV], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(sub, name), "rb").read(), name
    other = autocorr(argparse.Namespace(data=path, output_dir=str(tmp_path / "seed4"), prefix="", k=6, n_perms=100, seed=4, top=0,
                                        device=DEV))
    a, b = other["results"]["E12"], res["results"]["E12"]
    np.testing.assert_array_equal(a.I, b.I)
    np.testing.assert_array_equal(a.z_norm_C, b.z_norm_C)
    assert not np.array_equal(a.N[:, 1:], b.N[:, 1:]) and not np.array_equal(a.p_sim_I[20:39], b.p_sim_I[20:39])
    assert len(other["tables"]["E12"]) == 40                                         # top = 0: every gene
