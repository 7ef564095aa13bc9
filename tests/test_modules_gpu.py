"""The cross-Moran kernels on the MI355X against the numpy restatement of their definition (tests/modules_ref.py, held to its own
conditions by tests/test_modules_cpu.py), evaluated on the values and the centre the device was given.

Tolerance.  Z and Y are subtractions and sequential additions: the device and numpy produce the same bits (assert_array_equal).
M[l, g, h] is a sum of n products in an order of the device's own (four spots per matrix-core step, fused), the restatement's in
the order of its BLAS.  Each evaluation is within (n + 2) 2^-53 A of the exact sum, A = sum_i |z_g[pi(i)]| |Y[i, h]| (one
rounding per product or none, n - 1 additions, a factor 2 for the higher orders), so
    |M_dev - M_ref| <= 4 (n + 2) 2^-53 A                       (modules_ref.bound_M; the argument of test_autocorr_gpu.py)
and every test prints the largest multiple of 2^-53 A it has seen.  The diagonal M[0, g, g] is compared with the N of
autocorr_sums (the same E terms in another order) under autocorr_cases.bound_N.  Everything about repeatability is
assert_array_equal: the order of the additions depends on n alone."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import autocorr_cases as ac
import autocorr_ref as aref
import hotspots_ref as href
import modules_cases as cases
import modules_ref as ref
import nhood_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


class Counts:
    """The CSC of autocorr_cases.csc on the device, with what cross_sums reads of a DeviceCounts."""

    def __init__(self, Vs):
        colptr, ridx, vals, off = ac.csc(Vs)
        self.colptr, self.ridx, self.values = _dev(colptr), _dev(ridx), _dev(vals)
        self.tp_off_host, self.T, self.G, self.n, self.device = off, len(Vs), Vs[0].shape[1], int(off[-1]), torch.device(DEV)
        self.centre = np.stack([ac.centres(V) for V in Vs])


def _edges(problems):
    return [(_dev(s, torch.int32), _dev(d, torch.int32)) for s, d, _ in problems]


def _run(problems, n_perms, genes=None, seed=cases.SEED, **kw):
    """problems: [(src, dst, V)].  Returns spadot_amd.modules.cross_sums on their CSC and the centres of autocorr_cases."""
    from spadot_amd.modules import cross_sums
    dc = Counts([V for _, _, V in problems])
    genes = np.arange(dc.G) if genes is None else genes
    return cross_sums(_edges(problems), dc, dc.values, dc.centre, genes, n_perms, seed=seed, **kw)


def _within(got, want, problems, what):
    """|M_dev - M_ref| <= bound_M per time point; prints the largest multiple of 2^-53 A."""
    assert len(got) == len(want) == len(problems)
    worst = 0.0
    for t, (g, (M, A), (_, _, V)) in enumerate(zip(got, want, problems)):
        assert g.dtype == np.float64 and g.shape == M.shape, (what, t, g.shape, M.shape)
        err, n = np.abs(g - M), V.shape[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(A > 0, err / (U * A), 0.0), initial=0.0)))
        assert np.all(err <= ref.bound_M(n, A)), f"{what}, time point {t}: {float((err - ref.bound_M(n, A)).max()):.3e} over the bound"
    print(f"{what}: largest |M_dev - M_ref| = {worst:.2f} x 2^-53 A (bound 4 (n + 2))")


def test_the_case_file_holds_the_library_constants():
    from spadot_amd import stage_ops as ops
    assert (cases.TILE, ops.CROSS_MAX_G, ops.CROSS_DESC) == (ops.CROSS_TILE, 4096, 9)
    assert ops.cross_padded(cases.TILE + 1) == 80 and ops.cross_layout([5])[1] == 8


@pytest.mark.parametrize("key", ((("edge",),), (("stored",),)))
def test_the_images_have_the_bits_of_numpy_and_of_the_local_lag(key):
    from spadot_amd.hotspots import local_lag
    problems = cases.problems(key)
    sel = np.array([3, 1, 1, 0, 2])
    got, images = _run(problems, 0, genes=sel, images=True)
    dc = Counts([V for _, _, V in problems])
    lag = local_lag(_edges(problems), dc, dc.values, dc.centre, sel, 1)
    for t, (src, dst, V) in enumerate(problems):
        c = ac.centres(V)[sel]
        Z, Y = images[t]
        assert Z.shape == Y.shape == (V.shape[0], sel.size)
        np.testing.assert_array_equal(Z, ref.centred(V[:, sel], c), err_msg=f"Z of time point {t}")
        np.testing.assert_array_equal(Y, ref.lag(src, dst, V[:, sel], c), err_msg=f"Y of time point {t}")
        np.testing.assert_array_equal(Y.T, lag[t][0], err_msg=f"Y against local_lag, time point {t}")


def test_the_edge_call_is_one_launch_of_four_time_points():
    key = (("edge",),)
    problems = cases.problems(key)
    got = _run(problems, 5, seed=1)
    _within(got, cases.want(key, 5, 1), problems, "edge call")
    assert [g.shape for g in got] == [(6, 4, 4)] * 4 and [p[2].shape[0] for p in problems] == [1, 2, 37, 300]
    assert not got[0].any()                                                          # one spot, no edges: every lag is 0
    assert not got[2][:, :, 0].any() and not got[2][:, 0, :].any()                   # the gene that is all zero there: z = 0 = Y


@pytest.mark.parametrize("n", cases.TILE_NS)
def test_spot_counts_around_the_step_and_the_row_block(n):
    key = (("tile", n, 5),)
    problems = cases.problems(key)
    _within(_run(problems, 3, seed=5), cases.want(key, 3, 5), problems, f"n = {n}")


@pytest.fixture(scope="module")
def wide():
    problems = cases.problems((("wide",),))
    return problems, _run(problems, 2, seed=9)


@pytest.mark.parametrize("G", cases.GENE_COUNTS)
def test_gene_counts_around_the_blocks_and_the_tile(wide, G):
    problems, full = wide
    sel = tuple(range(G))
    got = _run(problems, 2, genes=np.arange(G), seed=9)
    _within(got, cases.want((("wide",),), 2, 9, sel=sel), [(s, d, V[:, :G]) for s, d, V in problems], f"{G} genes")
    np.testing.assert_array_equal(got[0], full[0][:, :G, :G], err_msg="the bits do not depend on the other genes of the call")


def test_a_selection_that_repeats_and_descends_and_a_gene_alone(wide):
    problems, full = wide
    sel = np.array([64, 40, 40, 17, 0, 64, 3])
    got = _run(problems, 2, genes=sel, seed=9)
    np.testing.assert_array_equal(got[0], full[0][:, sel][:, :, sel])
    alone = _run(problems, 2, genes=[40], seed=9)
    np.testing.assert_array_equal(alone[0], full[0][:, 40:41, 40:41])


def test_stored_counts_around_the_wavefront_and_the_workgroup():
    key = (("stored",),)
    problems = cases.problems(key)
    got = _run(problems, 4, seed=2)
    _within(got, cases.want(key, 4, 2), problems, "stored counts")
    assert not got[1][:, 0, :].any() and not got[1][:, :, 0].any()                   # nothing stored: z = 0 - 0 everywhere


def test_the_diagonal_is_the_edge_sum_of_autocorr():
    from spadot_amd.autocorr import autocorr_sums
    src, dst, V = ac.planted_genes()
    dc = Counts([V])
    edges = _edges([(src, dst, V)])
    M = _run([(src, dst, V)], 0)[0]
    N, _ = autocorr_sums(edges, dc, dc.values, dc.centre, 0)
    for g in range(V.shape[1]):
        A = aref.edge_sums(src, dst, V[:, g], dc.centre[0, g])[2]
        err = abs(M[0, g, g] - N[0][g, 0])
        print(f"gene {g}: |M[0, g, g] - N| = {err / (U * A) if A else 0.0:.2f} x 2^-53 A (bound {4 * 2402})")
        assert err <= ac.bound_N(2400, A)


@pytest.fixture(scope="module")
def p23():
    problems = [ac.edge_call()[2], cases.tile_case(300, 5)]
    problems[0] = problems[0][:2] + (np.concatenate([problems[0][2], problems[0][2][:, :1]], axis=1),)   # five genes in both
    return problems, _run(problems, 23)


def test_p23_matches_the_restatement(p23):
    problems, got = p23
    want = [ref.cross_sums(s, d, V, ac.centres(V), 23, cases.SEED, t) for t, (s, d, V) in enumerate(problems)]
    _within(got, want, problems, "P = 23")


def test_two_runs_alone_and_in_a_batch_give_the_same_bits(p23):
    problems, got = p23
    for t in range(2):
        np.testing.assert_array_equal(_run(problems, 23)[t], got[t], err_msg="run twice")
    one = _run(problems[:1], 23)
    np.testing.assert_array_equal(one[0], got[0], err_msg="the first time point alone (the same graph index: the same draws)")
    rng = np.random.default_rng(8)
    batch = [problems[0], nc.random_edges(rng, 65, 390) + (ac.random_values(rng, 65, 5),), problems[1]]
    big = _run(batch, 23, genes=[4, 0, 1, 2, 3, 3])                                  # other n, another G, another order
    np.testing.assert_array_equal(big[0][:, 1:5, 1:5], got[0][:, :4, :4], err_msg="in a batch of other n and G")
    other = _run(problems[1:], 23)                                                   # graph index 0 now: other draws
    np.testing.assert_array_equal(other[0][0], got[1][0])
    assert not np.array_equal(other[0][1:], got[1][1:])


def test_a_run_split_over_first_and_over_launches_has_the_same_bits(p23, monkeypatch):
    from spadot_amd import modules
    problems, got = p23
    part = _run(problems, 8, first=15, observed=False)
    a = _run(problems, 15)
    for t in range(2):
        assert part[t].shape == (8, 5, 5)
        np.testing.assert_array_equal(part[t], got[t][16:24])
        np.testing.assert_array_equal(a[t], got[t][:16])
    monkeypatch.setattr(modules, "SCRATCH_BYTES", 2 * 5 * 5 * 8 * 3)                 # three labelings a launch: eight launches
    from spadot_amd.utils._stage_utils import labeling_runs
    assert len(labeling_runs(23, True, 0, 2 * 5 * 5 * 8, modules.SCRATCH_BYTES)) == 8
    split = _run(problems, 23)
    for t in range(2):
        np.testing.assert_array_equal(split[t], got[t], err_msg="several launches")
    assert not np.array_equal(_run(problems, 23, seed=cases.SEED + 1)[0][1:], got[0][1:])       # another seed: other draws
    np.testing.assert_array_equal(_run(problems, 23, seed=cases.SEED + 1)[0][0], got[0][0])


def test_dense_columns_enter_as_the_image_with_the_same_bits(p23):
    from spadot_amd.modules import cross_sums
    problems, got = p23
    dc = Counts([V for _, _, V in problems])
    sel = [4, 2, 2, 0]
    a, ia = cross_sums(_edges(problems), dc, dc.values, dc.centre, sel, 7, seed=cases.SEED, images=True)
    dense = [_dev(V.astype(np.float64) if t else V) for t, (_, _, V) in enumerate(problems)]    # float32 and float64 columns
    b, ib = cross_sums(_edges(problems), dense, None, dc.centre, sel, 7, seed=cases.SEED, images=True)
    for t in range(2):
        np.testing.assert_array_equal(a[t], b[t])
        np.testing.assert_array_equal(ia[t][0], ib[t][0])
        np.testing.assert_array_equal(ia[t][1], ib[t][1])
        np.testing.assert_array_equal(a[t], got[t][:8][:, sel][:, :, sel])


@pytest.mark.parametrize("case", range(len(cases.PVALUE_CASES)))
def test_the_counts_are_the_formula_on_the_device_sums_and_the_restatement_outside_the_margin(case):
    from spadot_amd.modules import cross_moran, cross_sums
    key, P, seed = cases.PVALUE_CASES[case]
    problems = cases.problems(key)
    dense = [_dev(V) for _, _, V in problems]
    G = problems[0][2].shape[1]
    res = cross_moran(_edges(problems), dense, np.arange(G), n_perms=P, seed=seed)
    centre = np.stack([r.mean for r in res])
    M = cross_sums(_edges(problems), dense, None, centre, np.arange(G), P, seed=seed)
    for t, ((src, dst, V), r) in enumerate(zip(problems, res)):
        n, E = V.shape[0], src.shape[0]
        assert (r.n, r.E, r.P) == (n, E, P) and r.ge.dtype == np.int64 and r.z.shape == (n, G) and r.z.is_cuda
        np.testing.assert_array_equal(r.ge, ref.counts(M[t]), err_msg="ge is the formula on the device's own M")
        np.testing.assert_allclose(r.mean, ac.centres(V), rtol=4 * n * U)
        Mr, A = ref.cross_sums(src, dst, V, r.mean, P, seed, t)
        _within([M[t]], [(Mr, A)], [problems[t]], f"{key[t]}")
        close, _ = ref.margin_share(Mr, A, n)                                        # [P, pairs g <= h]
        iu = np.triu_indices(G)
        doubt = close.sum(axis=0)
        diff = np.abs(r.ge[iu] - ref.counts(Mr)[iu])
        print(f"{key[t]}: {int((doubt > 0).sum())} of {doubt.size} pairs have a comparison inside the bound; ge differs in "
              f"{int((diff > 0).sum())}")
        assert np.all(diff <= doubt)                                                 # equal wherever the margin exceeds the bound
        m2, sumsq = ref.spread(V, r.mean)
        st = ref.stats(M[t], n, E, m2, sumsq)                                        # the host statistics on the device's sums
        np.testing.assert_array_equal(r.degenerate, st["degenerate"])
        np.testing.assert_array_equal(r.p_sim, st["p_sim"])
        np.testing.assert_allclose(r.R, st["R"], rtol=1e-9)                          # m2 from fixed-order moments, not sum z^2
        np.testing.assert_allclose(r.padj, st["padj"], rtol=1e-12)
        np.testing.assert_allclose(r.z_sim, st["z_sim"], rtol=1e-6)
        np.testing.assert_array_equal(r.R, r.R.T)


def _desc(n=37, E=0, row0=0, gid=0, lo=0, hi=36, eoff=0, roff=0, zoff=0):
    return np.array([[eoff, n, E, row0, gid, roff, lo, hi, zoff]], dtype=np.int64)


def test_refusals_come_before_any_launch():
    from spadot_amd import stage_ops as ops
    from spadot_amd.modules import cross_sums
    src, dst, V = ac.edge_call()[2]
    E = src.shape[0]
    dc = Counts([V])
    e = (_dev(src, torch.int32), _dev(dst, torch.int32))

    def call(edges=e, counts=dc, P=3, genes=(0, 1, 2, 3), **kw):
        return cross_sums([edges], counts, counts.values, counts.centre, genes, P, **kw)

    bad = dst.copy()
    bad[7] = 37
    with pytest.raises(ValueError, match=r"edge ends 0 \.\. 37: they must lie in 0 \.\. 36"):
        call(edges=(e[0], _dev(bad, torch.int32)))
    worse = Counts([V])
    worse.ridx = worse.ridx.clone()
    worse.ridx[3] = 37
    with pytest.raises(ValueError, match=r"row indices 0 \.\. 37: they must lie in 0 \.\. 36"):
        call(counts=worse)
    for genes in ((0, 4), (-1, 2)):
        with pytest.raises(ValueError, match="selected genes"):
            call(genes=genes)
    with pytest.raises(ValueError, match="at most 4096 selected genes"):
        call(genes=np.zeros(4097, dtype=np.int64))
    with pytest.raises(ValueError, match="must not be negative"):
        call(P=-1)
    with pytest.raises(ValueError, match="at least one labeling"):
        call(P=0, observed=False)
    with pytest.raises(ValueError, match="below 2\\^32"):
        call(first=2 ** 32 - 2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        call(edges=(torch.as_tensor(src), torch.as_tensor(dst)))
    with pytest.raises(RuntimeError, match="device tensor"):
        cross_sums([e], dc, dc.values.cpu().numpy(), dc.centre, [0], 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        cross_sums([e], dc, dc.values.cpu(), dc.centre, [0], 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        cross_sums([e], [torch.as_tensor(V)], None, dc.centre, [0], 3)

    rowptr, col = href.csr(src, dst, 37)                                             # the launchers themselves, into poisoned outputs
    rp, cl, cen, gsel = _dev(rowptr, torch.int32), _dev(col, torch.int32), _dev(dc.centre), _dev([0, 1, 2, 3], torch.int32)
    Z, Y = (torch.full((40, 16), -77.0, dtype=torch.float64, device=DEV) for _ in range(2))
    M = torch.full((1, 4, 4, 4), -77.0, dtype=torch.float64, device=DEV)

    def dense(rowptr=rp, col=cl, genes=gsel, desc=None, **kw):
        desc = _desc(E=E) if desc is None else desc
        return ops.cross_dense(rowptr, col, dc.colptr, dc.ridx, dc.values, cen, genes, desc, out=(Z, Y), **kw)

    c2 = cl.clone()
    c2[5] = 37
    with pytest.raises(ValueError, match=r"neighbours 0 \.\. 37 in col"):
        dense(col=c2)
    c2[5] = -1
    with pytest.raises(ValueError, match=r"neighbours -1"):
        dense(col=c2)
    for i, v in ((0, 1), (37, E - 1), (10, int(rowptr[9]) - 1)):
        r2 = rp.clone()
        r2[i] = v
        with pytest.raises(ValueError, match="must ascend from 0"):
            dense(rowptr=r2)
    with pytest.raises(ValueError, match="selected genes"):
        dense(genes=_dev([0, 4], torch.int32))
    with pytest.raises(ValueError, match="1 to 4096 selected genes"):
        dense(genes=torch.zeros(4097, dtype=torch.int32, device=DEV))
    cp2 = dc.colptr.clone()
    cp2[2] = cp2[1] - 1
    with pytest.raises(ValueError, match="colptr must ascend"):
        ops.cross_dense(rp, cl, cp2, dc.ridx, dc.values, cen, gsel, _desc(E=E), out=(Z, Y))
    for desc, what in ((_desc(n=2 ** 31, E=E), "spots"), (_desc(E=2 ** 31), "edges"), (_desc(E=E, row0=-1), "inconsistent"),
                       (_desc(E=E, gid=2 ** 31), "inconsistent"), (_desc(E=E + 1), "reach past"), (_desc(E=E, zoff=4), "rows")):
        with pytest.raises(ValueError, match=what):
            dense(desc=desc)
    with pytest.raises(ValueError, match="time points"):
        ops.cross_dense(rp, cl, dc.colptr, dc.ridx, dc.values, cen, gsel, np.repeat(_desc(E=E), 65536, axis=0), out=(Z, Y))
    with pytest.raises(RuntimeError, match="MI355X only"):
        dense(rowptr=rp.cpu())

    def sums(desc=None, ng=4, observed=True, first=0, P=3, Zin=Z, Yin=Y):
        return ops.cross_sums(Zin, Yin, _desc(E=E) if desc is None else desc, ng, observed, first, P, out=M)

    wide = torch.zeros((40, 4096), dtype=torch.float64, device=DEV)
    for kw, what in ((dict(ng=4097), "1 to 4096 selected genes"), (dict(ng=0), "1 to 4096 selected genes"),
                     (dict(desc=_desc(n=2 ** 31)), "spots"), (dict(desc=_desc(gid=2 ** 31)), "inconsistent"),
                     (dict(desc=_desc(zoff=4)), "rows"), (dict(first=2 ** 32 - 3, P=4), "below 2\\^32"),
                     (dict(P=0, observed=False), "at least one labeling"), (dict(P=-1), "P >= 0"),
                     (dict(ng=17), r"\[40, 32\]"), (dict(Zin=Z.float()), "float64"),
                     (dict(ng=4096, Zin=wide, Yin=wide, P=2 ** 19), "workgroups")):
        with pytest.raises(ValueError, match=what):
            sums(**kw)
    with pytest.raises(RuntimeError, match="MI355X only"):
        sums(Zin=Z.cpu())
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == -77)) for o in (Z, Y, M))                         # nothing was launched

    lib = ops.model_lib()                                                            # the library's own checks, from the host descriptor

    def raw_dense(desc, rowptr=rp.data_ptr(), colptr=dc.colptr.data_ptr(), nnz=int(dc.ridx.numel()), lo=0, hi=36, T=1, G=4, ng=4,
                  glo=0, ghi=3, GP=16, zrows=40, Zp=Z.data_ptr()):
        ddev = _dev(desc)
        return lib.spadot_cross_dense(rowptr, cl.data_ptr(), colptr, dc.ridx.data_ptr(), dc.values.data_ptr(), nnz, lo, hi,
                                      cen.data_ptr(), ctypes.c_void_p(desc.ctypes.data), ddev.data_ptr(), T, G, gsel.data_ptr(), ng,
                                      glo, ghi, GP, zrows, Zp, Y.data_ptr(), None)

    def raw_sums(desc, T=1, ng=4, GP=16, zrows=40, observed=1, first=0, P=3, Mp=M.data_ptr()):
        ddev = _dev(desc)
        return lib.spadot_cross_sums(Z.data_ptr(), Y.data_ptr(), zrows, GP, ctypes.c_void_p(desc.ctypes.data), ddev.data_ptr(), T,
                                     ng, observed, first, P, 0, Mp, None)

    ok = _desc(E=E)
    for kw in (dict(desc=_desc(n=2 ** 31, E=E)), dict(desc=_desc(E=2 ** 31)), dict(desc=_desc(E=E, hi=37)), dict(desc=_desc(E=E, lo=-1)),
               dict(desc=_desc(E=E, gid=2 ** 31)), dict(desc=ok, hi=37), dict(desc=ok, lo=-1), dict(desc=ok, ghi=4),
               dict(desc=ok, glo=-1), dict(desc=ok, ng=4097, GP=4112), dict(desc=ok, T=65536)):
        assert raw_dense(**kw) == -7, kw
    for kw in (dict(desc=_desc(n=0, E=E)), dict(desc=_desc(E=-1)), dict(desc=_desc(E=E, row0=-1)), dict(desc=ok, rowptr=None),
               dict(desc=ok, Zp=None), dict(desc=ok, ng=0), dict(desc=ok, T=0), dict(desc=ok, nnz=-1), dict(desc=ok, GP=32),
               dict(desc=ok, zrows=39), dict(desc=_desc(E=E, zoff=1)), dict(desc=ok, G=0)):
        assert raw_dense(**kw) == -22, kw
    for kw in (dict(desc=_desc(n=2 ** 31)), dict(desc=_desc(gid=2 ** 31)), dict(desc=ok, ng=4097, GP=4112),
               dict(desc=ok, first=2 ** 32 - 2), dict(desc=ok, ng=4096, GP=4096, P=2 ** 19)):
        assert raw_sums(**kw) == -7, kw
    for kw in (dict(desc=_desc(n=0)), dict(desc=ok, Mp=None), dict(desc=ok, ng=0), dict(desc=ok, T=0), dict(desc=ok, P=-1),
               dict(desc=ok, first=-1), dict(desc=ok, observed=0, P=0), dict(desc=ok, observed=2), dict(desc=ok, GP=32),
               dict(desc=ok, zrows=39), dict(desc=_desc(zoff=1))):
        assert raw_sums(**kw) == -22, kw
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == -77)) for o in (Z, Y, M))
    got = call(seed=cases.SEED)                                                      # and a valid call goes through
    _within(got, [ref.cross_sums(src, dst, V, ac.centres(V), 3, cases.SEED, 0)], [(src, dst, V)], "after the refusals")


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from spadot_amd.modules import modules
    out = tmp_path_factory.mktemp("modules")
    path = ac.stage_counts(os.path.join(out, "counts.npz"))
    res = modules(argparse.Namespace(data=path, output_dir=str(out), prefix="s_", k=6, n_perms=99, seed=3, top=8, genes=None,
                                     min_sim=0.15, min_genes=2, alpha=0.05, top_pairs=0, device=DEV))
    return path, str(out), res


def test_the_stage_writes_its_files(stage):
    import pandas as pd
    from spadot_amd.modules import FIELDS, OVERLAP_COLUMNS, PAIR_COLUMNS, TABLE_COLUMNS, module_overlap
    path, out, res = stage
    tps = ["E10", "E12", "E14"]
    assert res["timepoints"] == tps and set(res["timings"]) == {"read_s", "graph_s", "device_s", "write_s", "total_s"}
    assert TABLE_COLUMNS == ("gene", "module", "I", "R_own", "best_other", "R_other")
    assert PAIR_COLUMNS == ("gene_a", "gene_b", "R", "z_sim", "p_sim", "padj", "same_module")
    sel = res["genes"]
    G = sel.size
    assert 8 <= G <= 24 and np.all(np.diff(sel) > 0) and set(sel) <= set(range(20)) and np.sum(sel < 10) >= 8
    z = np.load(os.path.join(out, "s_modules.npz"))
    names = [f"g{g:02d}" for g in sel]
    assert z["timepoints"].tolist() == tps and z["genes"].tolist() == names
    assert (int(z["k"]), int(z["n_perms"]), int(z["seed"]), float(z["min_sim"]), int(z["min_genes"]), float(z["alpha"])) == (
        6, 99, 3, 0.15, 2, 0.05)
    raw = np.load(path)
    for tp, n in zip(tps, (400, 500, 600)):
        r, lab, sc = res["results"][tp], res["modules"][tp], res["scores"][tp]
        for name in FIELDS:
            assert z[f"{tp}_{name}"].shape == (G, G) and z[f"{tp}_{name}"].dtype == np.float64
            np.testing.assert_array_equal(z[f"{tp}_{name}"], getattr(r, name), err_msg=f"{tp}_{name}")
        np.testing.assert_array_equal(z[f"{tp}_module"], lab)
        np.testing.assert_array_equal(z[f"{tp}_scores"], sc)
        assert z[f"{tp}_module"].dtype == np.int64 and sc.shape == (lab.max() + 1, n) and not r.degenerate.any()
        spots = z[f"{tp}_spots"]
        assert spots.shape == (n,) and np.all(raw["timepoint"][spots] == tp)
        np.testing.assert_allclose(sc, ref.scores(r.z.cpu().numpy(), r.m2, n, lab), rtol=1e-13, atol=1e-13)
        tab = pd.read_csv(os.path.join(out, f"s_modules_{tp}.csv"))
        assert tuple(tab.columns) == TABLE_COLUMNS and tab["gene"].tolist() == names and tab["module"].tolist() == lab.tolist()
        assert tab["module"].dtype == np.int64 and tab["best_other"].dtype == np.int64 and tab["I"].dtype == np.float64
        np.testing.assert_allclose(tab["I"], np.diagonal(r.R), rtol=1e-12)
        for j in range(G):
            mates = np.flatnonzero((lab == lab[j]) & (np.arange(G) != j)) if lab[j] >= 0 else np.zeros(0, int)
            if mates.size:
                np.testing.assert_allclose(tab["R_own"][j], r.R[j, mates].mean(), rtol=1e-12)
            else:
                assert np.isnan(tab["R_own"][j])
        pt = pd.read_csv(os.path.join(out, f"s_modules_pairs_{tp}.csv"))
        assert tuple(pt.columns) == PAIR_COLUMNS and len(pt) == G * (G - 1) // 2 and np.all(np.diff(np.abs(pt["R"])) <= 0)
        where = {g: j for j, g in enumerate(names)}
        a, b = pt["gene_a"].map(where).to_numpy(), pt["gene_b"].map(where).to_numpy()
        assert np.all(a < b)
        np.testing.assert_allclose(pt["R"], r.R[a, b], rtol=1e-12)
        np.testing.assert_allclose(pt["p_sim"], r.p_sim[a, b], rtol=1e-12)
        np.testing.assert_allclose(pt["padj"], r.padj[a, b], rtol=1e-12)
        np.testing.assert_array_equal(pt["same_module"], ((lab[a] >= 0) & (lab[a] == lab[b])).astype(int))
        bad, same, (lo, hi) = cases.broken_conditions(sel, cases.STAGE_K[tp], r.R, r.p_sim, lab, 99)
        print(f"{tp}: modules {lab.tolist()}, smallest R of a same-domain pair {same:.3f}, R of markers of different domains "
              f"{lo:.3f} .. {hi:.3f}")
        assert not bad, "\n".join(bad)
    ov = pd.read_csv(os.path.join(out, "s_modules_overlap.csv"))
    assert tuple(ov.columns) == OVERLAP_COLUMNS
    for ta, tb in zip(tps, tps[1:]):
        jac, both = module_overlap(res["modules"][ta], res["modules"][tb])
        rows = ov[(ov["timepoint_a"] == ta) & (ov["timepoint_b"] == tb)]
        np.testing.assert_allclose(rows["jaccard"].to_numpy().reshape(jac.shape), jac, rtol=1e-12)
        np.testing.assert_allclose(jac, ref.jaccard(res["modules"][ta], res["modules"][tb]))


def test_a_second_run_and_the_sub_command_write_the_same_bytes(stage, tmp_path):
    from spadot_amd.modules import modules
    path, out, res = stage
    names = ["s_modules.npz", "s_modules_overlap.csv"] + [f"s_modules_{tp}.csv" for tp in res["timepoints"]] + \
            [f"s_modules_pairs_{tp}.csv" for tp in res["timepoints"]]
    modules(argparse.Namespace(data=path, output_dir=str(tmp_path), prefix="s_", k=6, n_perms=99, seed=3, top=8, genes=None,
                               min_sim=0.15, min_genes=2, alpha=0.05, top_pairs=0, device=DEV))
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(tmp_path, name), "rb").read(), name
    sub = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "spadot_amd", "modules", "-i", path, "-o", str(sub), "--prefix", "s_", "--n_perms",
                        "99", "--seed", "3", "--top", "8", "--device", DEV], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(sub, name), "rb").read(), name
    named = modules(argparse.Namespace(data=path, output_dir=str(tmp_path / "named"), prefix="", k=6, n_perms=99, seed=3, top=8,
                                       genes="g03,g12,g07", min_sim=0.15, min_genes=2, alpha=0.05, top_pairs=2, device=DEV))
    assert named["genes"].tolist() == [3, 12, 7] and all(len(t) == 2 for t in named["pair_tables"].values())
    if 3 in res["genes"] and 7 in res["genes"]:
        j3, j7 = (int(np.flatnonzero(res["genes"] == g)[0]) for g in (3, 7))
        np.testing.assert_array_equal(named["results"]["E12"].ge[0, 2], res["results"]["E12"].ge[j3, j7])
