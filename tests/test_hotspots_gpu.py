"""The local Moran's I kernel on the MI355X against the numpy restatement of its definition (tests/hotspots_ref.py, held to its own
conditions by tests/test_hotspots_cpu.py).  lag, ge and le are exact: the neighbour sums are sequential fp64 additions of fp64
differences (no product, nothing to contract), so the device and numpy produce the same bits and the comparisons the same
integers; every comparison is assert_array_equal, evaluated on the values and the centre the device was given.  The one bounded
comparison is against autocorr's N (another order of the same terms), with the bound of tests/test_autocorr_gpu.py."""
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
import hotspots_cases as cases
import hotspots_ref as ref
import nhood_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


class Counts:
    """The CSC of autocorr_cases.csc on the device, with what local_lag reads of a DeviceCounts."""

    def __init__(self, Vs):
        colptr, ridx, vals, off = ac.csc(Vs)
        self.colptr, self.ridx, self.values = _dev(colptr), _dev(ridx), _dev(vals)
        self.tp_off_host, self.T, self.G, self.n, self.device = off, len(Vs), Vs[0].shape[1], int(off[-1]), torch.device(DEV)
        self.centre = np.stack([ac.centres(V) for V in Vs])


def _run(problems, n_perms, genes=None, seed=cases.SEED, **kw):
    """problems: [(src, dst, V)].  Returns [t] -> (lag, ge, le) of spadot_amd.hotspots.local_lag."""
    from spadot_amd.hotspots import local_lag
    dc = Counts([V for _, _, V in problems])
    edges = [(_dev(s, torch.int32), _dev(d, torch.int32)) for s, d, _ in problems]
    genes = np.arange(dc.G) if genes is None else genes
    return local_lag(edges, dc, dc.values, dc.centre, genes, n_perms, seed=seed, **kw)


def _equal(got, want, what):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert g[0].dtype == np.float64 and g[1].dtype == np.int32 and g[2].dtype == np.int32
        for name, a, b in zip(("lag", "ge", "le"), g, w):
            np.testing.assert_array_equal(a, b, err_msg=f"{what}, time point {t}, {name}")


def test_the_case_file_holds_the_library_defaults():
    from spadot_amd import stage_ops as ops
    assert (cases.THREADS, cases.GS, cases.CHUNK) == (ops.LOCAL_THREADS, ops.LOCAL_GS, ops.LOCAL_CHUNK)
    assert (cases.LDS_BYTES, cases.LDS_FIXED) == (ops.LOCAL_LDS_BYTES, ops.LOCAL_LDS_FIXED)
    assert ops.local_lds_bytes(300) == 256 + 4 * 4 * 300 and ops.local_lds_bytes(300, 2) == 256 + 8 * 300


def test_edge_call_matches_the_restatement():
    call = cases.edge_call()
    got = _run(call, 10, seed=1)
    _equal(got, cases.want(call, 10, seed=1), "edge call")
    assert [g[0].shape for g in got] == [(4, 1), (4, 2), (4, 37), (4, 300)]
    assert not got[0][0].any() and got[0][1].tolist() == [[10]] * 4 and got[0][2].tolist() == [[10]] * 4      # no neighbours: 0 >= 0
    for t, lone in cases.LONE.items():
        assert not got[t][0][:, lone].any() and np.all(got[t][1][:, lone] == 10) and np.all(got[t][2][:, lone] == 10)
    assert np.all(got[2][1][0] == 10) and np.all(got[2][2][0] == 10)                  # the gene that is all zero there: ties


@pytest.mark.parametrize("n", cases.TILE_NS + (257,))
def test_tile_edges_match_the_restatement(n):
    prob = [cases.tile_case(n, 0 if n == 257 else None)]
    got = _run(prob, 3, seed=5)
    _equal(got, cases.want(prob, 3, seed=5), f"n = {n}")
    if n == 257:
        assert not got[0][0].any() and np.all(got[0][1] == 3) and np.all(got[0][2] == 3)


@pytest.fixture(scope="module")
def nine():
    prob = [cases.tile_case(257, 1537, G=2 * cases.GS + 1)]
    return prob, cases.want(prob, 2, seed=9)


@pytest.mark.parametrize("G", cases.GROUP_SIZES)
def test_gene_selections_around_the_group_match_the_restatement(nine, G):
    prob, want = nine
    got = _run(prob, 2, genes=np.arange(G), seed=9)
    _equal(got, [tuple(w[:G] for w in want[0])], f"{G} genes")


def test_a_selection_that_repeats_and_descends_and_a_gene_alone(nine):
    prob, want = nine
    sel = np.array([7, 5, 5, 2, 0, 7])
    got = _run(prob, 2, genes=sel, seed=9)
    _equal(got, [tuple(w[sel] for w in want[0])], "a repeating, descending selection")
    alone = _run(prob, 2, genes=[5], seed=9)
    _equal(alone, [tuple(g[1:2] for g in got[0])], "a gene alone")


def test_stored_counts_around_the_wavefront_and_the_workgroup():
    prob = ac.stored_case()
    got = _run(prob, 4, seed=2)
    _equal(got, cases.want(prob, 4, seed=2), "stored counts")
    assert not got[1][0][0].any()                                                    # nothing stored: x = 0 = c everywhere


@pytest.fixture(scope="module")
def p23():
    prob = [cases.edge_call()[2], cases.tile_case(300)]
    prob[1] = (prob[1][0], prob[1][1], ac.random_values(np.random.default_rng(4), 300, 4))
    return prob, _run(prob, 23)


def test_p23_matches_the_restatement(p23):
    prob, got = p23
    _equal(got, cases.want(prob, 23), "P = 23")


@pytest.mark.parametrize("gs", (2, 4))
@pytest.mark.parametrize("threads", (256, 512, 1024))
def test_chunks_threads_and_group_sizes_are_not_in_the_results(p23, threads, gs):
    prob, got = p23
    for chunk in (1, 2, 7, 23, 64):
        _equal(_run(prob, 23, threads=threads, gs=gs, perm_chunk=chunk), got, f"threads {threads}, gs {gs}, perm_chunk {chunk}")


def test_a_run_split_over_first_adds_up(p23, monkeypatch):
    from spadot_amd import hotspots
    prob, got = p23
    a, b = _run(prob, 10), _run(prob, 13, first=10)
    for t in range(2):
        np.testing.assert_array_equal(a[t][0], got[t][0])
        np.testing.assert_array_equal(b[t][0], got[t][0])
        np.testing.assert_array_equal(a[t][1] + b[t][1], got[t][1])
        np.testing.assert_array_equal(a[t][2] + b[t][2], got[t][2])
    monkeypatch.setattr(hotspots, "SCRATCH_BYTES", 1)                                 # one chunk per launch: the same integers
    _equal(_run(prob, 23, perm_chunk=5), got, "one chunk per launch")


def test_the_image_in_global_memory_gives_the_same_results(p23):
    prob, got = p23
    _equal(_run(prob, 23, lds_limit=0), got, "n = 37 and 300 outside LDS")
    _equal(_run(prob, 23, lds_limit=cases.LDS_FIXED + 4 * cases.GS * 300 - 1), got, "n = 300 outside, n = 37 inside")
    stored = ac.stored_case()
    _equal(_run(stored, 4, seed=2, lds_limit=0), _run(stored, 4, seed=2), "n = THREADS + 76 outside LDS")


def test_a_graph_beyond_the_lds_image():
    from spadot_amd import stage_ops as ops
    n = (cases.LDS_BYTES - cases.LDS_FIXED) // (4 * cases.GS) + 1
    assert ops.local_lds_bytes(n - 1) <= ops.LOCAL_LDS_BYTES < ops.local_lds_bytes(n)
    prob = [cases.tile_case(n, G=2)]
    _equal(_run(prob, 2), cases.want(prob, 2), f"n = {n}")


def test_two_runs_alone_and_in_a_batch_give_the_same_results(p23):
    prob, _ = p23
    one = [prob[0]]
    a, b = _run(one, 20), _run(one, 20)
    _equal(b, a, "two runs alone")
    rng = np.random.default_rng(8)
    batch = [prob[0], nc.random_edges(rng, 300, 1800) + (ac.random_values(rng, 300, 4),),
             nc.random_edges(rng, 65, 390) + (ac.random_values(rng, 65, 4),)]
    c, d = _run(batch, 20), _run(batch, 20)
    _equal(d, c, "two runs of a batch")
    _equal(c[:1], a, "the first time point of a batch and alone")                     # the same graph index: the same draws
    _equal(c, cases.want(batch, 20), "the batch")


def test_the_sum_of_z_times_lag_is_the_edge_sum_of_autocorr():
    from spadot_amd.autocorr import autocorr_sums
    src, dst, V = ac.planted_genes()
    dc = Counts([V])
    edges = [(_dev(src, torch.int32), _dev(dst, torch.int32))]
    lag = _run([(src, dst, V)], 1)[0][0]
    N, _ = autocorr_sums(edges, dc, dc.values, dc.centre, 0)
    z = V.astype(np.float64).T - dc.centre[0][:, None]
    for g in range(V.shape[1]):
        A = aref.edge_sums(src, dst, V[:, g], dc.centre[0, g])[2]
        err = abs(float((z[g] * lag[g]).sum()) - N[0][g, 0])
        print(f"gene {g}: |sum z lag - N| = {err / (U * A) if A else 0.0:.2f} x 2^-53 A (bound {4 * 2402})")
        assert err <= ac.bound_N(2400, A)


def test_dense_columns_take_the_same_kernel():
    from spadot_amd.hotspots import local_moran
    src, dst, V = ac.planted_genes()
    edges = [(_dev(src, torch.int32), _dev(dst, torch.int32))]
    W = V[:, :3].astype(np.float64)
    r = local_moran(edges, [_dev(W)], [0, 1, 2], n_perms=19, seed=cases.SEED)[0]
    dc = Counts([V[:, :3]])
    from spadot_amd.hotspots import local_lag
    c = r.mean[None, :]                                                              # the centre the device was given
    got = local_lag(edges, dc, dc.values, c, [0, 1, 2], 19, seed=cases.SEED)[0]
    for a, b in zip((r.lag, r.ge, r.le), got):
        np.testing.assert_array_equal(a, b)
    w = ref.local_counts_genes(src, dst, 400, V[:, :3], c[0], 19, cases.SEED, 0)
    for a, b in zip((r.lag, r.ge, r.le), w):
        np.testing.assert_array_equal(a, b)
    assert r.quadrant.dtype == np.int8 and r.I.shape == (3, 400) and not r.degenerate.any() and r.has_neighbours.all()
    np.testing.assert_allclose(c[0], ac.centres(V[:, :3]), rtol=4 * 400 * U)
    for g in range(3):
        s = ref.stats(w[0][g], w[1][g], w[2][g], V[:, g], c[0, g], 400, 2400, 19, np.ones(400, bool))
        np.testing.assert_array_equal(r.quadrant[g], s["quadrant"])
        np.testing.assert_array_equal(r.p_sim[g], s["p_sim"])
        np.testing.assert_allclose(r.padj[g], s["padj"], rtol=1e-12)
        np.testing.assert_allclose(r.I[g], s["I"], rtol=1e-9, atol=1e-12)            # m2 from fixed-order moments, not sum z^2


def _desc(n=37, E=None, row0=0, gid=0, lo=0, hi=36, eoff=0, roff=0):
    return np.array([[eoff, n, E, row0, gid, roff, lo, hi]], dtype=np.int64)


def test_refusals_come_before_any_launch():
    from spadot_amd import stage_ops as ops
    from spadot_amd.hotspots import local_lag
    src, dst, V = ac.edge_call()[2]
    E = src.shape[0]
    dc = Counts([V])
    e = (_dev(src, torch.int32), _dev(dst, torch.int32))

    def call(edges=e, counts=dc, P=3, genes=(0, 1, 2, 3), **kw):
        return local_lag([edges], counts, counts.values, counts.centre, genes, P, **kw)

    bad = dst.copy()
    bad[7] = 37
    with pytest.raises(ValueError, match=r"edge ends 0 \.\. 37: they must lie in 0 \.\. 36"):
        call(edges=(e[0], _dev(bad, torch.int32)))
    wide = torch.as_tensor(dst, dtype=torch.int64, device=DEV)
    wide[7] = 2 ** 32 + 5                                                            # would wrap to 5 as an int32
    with pytest.raises(ValueError, match=r"edge ends \d+ \.\. 4294967301"):
        call(edges=(e[0].long(), wide))
    neg = Counts([V])
    neg.ridx = neg.ridx.clone()
    neg.ridx[3] = 37
    with pytest.raises(ValueError, match=r"row indices 0 \.\. 37: they must lie in 0 \.\. 36"):
        call(counts=neg)
    for genes in ((0, 4), (-1, 2)):
        with pytest.raises(ValueError, match="selected genes"):
            call(genes=genes)
    with pytest.raises(ValueError, match="at least one permutation"):
        call(P=0)
    with pytest.raises(ValueError, match="below 2\\^32"):
        call(first=2 ** 32 - 2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        call(edges=(torch.as_tensor(src), torch.as_tensor(dst)))
    with pytest.raises(RuntimeError, match="MI355X only"):
        local_lag([e], dc, dc.values.cpu(), dc.centre, [0], 3)
    with pytest.raises(ValueError, match="lds_limit"):
        call(lds_limit=-1)
    for kw in (dict(threads=128), dict(gs=3), dict(perm_chunk=-1)):
        with pytest.raises(ValueError, match="threads in"):
            call(**kw)

    rowptr, col = ref.csr(src, dst, 37)                                               # the launcher itself, into poisoned outputs
    rp, cl, cen, gsel = _dev(rowptr, torch.int32), _dev(col, torch.int32), _dev(dc.centre), _dev([0, 1, 2, 3], torch.int32)
    out = (torch.full((4, 37), -77.0, dtype=torch.float64, device=DEV), torch.full((4, 37), -77, dtype=torch.int32, device=DEV),
           torch.full((4, 37), -77, dtype=torch.int32, device=DEV))

    def op(rowptr=rp, col=cl, genes=gsel, desc=None, first=0, P=3, **kw):
        desc = _desc(E=E) if desc is None else desc
        return ops.local_lag(rowptr, col, dc.colptr, dc.ridx, dc.values, cen, genes, desc, first, P, out=out, **kw)

    c2 = cl.clone()
    c2[5] = 37
    with pytest.raises(ValueError, match=r"neighbours 0 \.\. 37 in col"):
        op(col=c2)
    c2[5] = -1
    with pytest.raises(ValueError, match=r"neighbours -1"):
        op(col=c2)
    for i, v in ((0, 1), (37, E - 1), (10, int(rowptr[9]) - 1)):
        r2 = rp.clone()
        r2[i] = v
        with pytest.raises(ValueError, match="must ascend from 0"):
            op(rowptr=r2)
    with pytest.raises(ValueError, match="selected genes"):
        op(genes=_dev([0, 4], torch.int32))
    with pytest.raises(ValueError, match="P >= 1"):
        op(P=0)
    with pytest.raises(ValueError, match="below 2\\^32"):
        op(first=2 ** 32 - 3, P=4)
    with pytest.raises(ValueError, match="workgroups"):
        op(P=2 ** 31, perm_chunk=1)
    for desc, what in ((_desc(n=2 ** 31, E=E), "spots"), (_desc(E=2 ** 31), "edges"), (_desc(E=E, row0=-1), "inconsistent"),
                       (_desc(E=E + 1), "reach past")):
        with pytest.raises(ValueError, match=what):
            op(desc=desc)
    with pytest.raises(RuntimeError, match="MI355X only"):
        op(rowptr=rp.cpu())
    torch.cuda.synchronize()
    assert all(torch.all(o == -77) for o in out)                                     # nothing was launched

    lib = ops.model_lib()                                                            # the library's own checks, from the host descriptor
    scratch = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def raw(desc, nnz=int(dc.ridx.numel()), lo=0, hi=36, T=1, G=4, ng=4, glo=0, ghi=3, first=0, P=3, lds=163840, threads=0, gs=0,
            chunk=0, rows=37, lag=out[0].data_ptr(), sc=scratch.data_ptr(), sbytes=1 << 16):
        ddev = _dev(desc)
        return lib.spadot_local_lag(rp.data_ptr(), cl.data_ptr(), dc.colptr.data_ptr(), dc.ridx.data_ptr(), dc.values.data_ptr(),
                                    nnz, lo, hi, cen.data_ptr(), ctypes.c_void_p(desc.ctypes.data), ddev.data_ptr(), T, G,
                                    gsel.data_ptr(), ng, glo, ghi, first, P, 0, lds, sc, sbytes, threads, gs, chunk, rows, lag,
                                    out[1].data_ptr(), out[2].data_ptr(), None)

    ok = _desc(E=E)
    for kw in (dict(desc=_desc(n=2 ** 31, E=E)), dict(desc=_desc(E=2 ** 31)), dict(desc=_desc(E=E, hi=37)),
               dict(desc=_desc(E=E, lo=-1)), dict(desc=_desc(E=E, gid=2 ** 31)), dict(desc=ok, hi=37), dict(desc=ok, lo=-1),
               dict(desc=ok, ghi=4), dict(desc=ok, glo=-1), dict(desc=ok, first=2 ** 32 - 2), dict(desc=ok, threads=128),
               dict(desc=ok, gs=3), dict(desc=ok, P=0), dict(desc=ok, chunk=-1), dict(desc=ok, P=2 ** 31, chunk=1)):
        assert raw(**kw) == -7, kw
    for kw in (dict(desc=_desc(n=0, E=E)), dict(desc=_desc(E=-1)), dict(desc=_desc(E=E, row0=-1)), dict(desc=ok, lag=None),
               dict(desc=ok, ng=0), dict(desc=ok, T=0), dict(desc=ok, lds=-1), dict(desc=ok, nnz=-1), dict(desc=ok, rows=36),
               dict(desc=ok, sc=None), dict(desc=ok, sbytes=16 * 4 * 37 - 1)):
        assert raw(**kw) == -22, kw
    torch.cuda.synchronize()
    assert all(torch.all(o == -77) for o in out)
    got = call(seed=cases.SEED)                                                      # and a valid call goes through
    _equal(got, cases.want([(src, dst, V)], 3), "after the refusals")


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from spadot_amd.hotspots import hotspots
    out = tmp_path_factory.mktemp("hotspots")
    path = ac.stage_counts(os.path.join(out, "counts.npz"))
    dom = cases.stage_domains(path, os.path.join(out, "domains.csv"))
    res = hotspots(argparse.Namespace(data=path, output_dir=str(out), prefix="s_", k=6, n_perms=99, seed=3, top=8, genes=None,
                                      alpha=0.05, fdr=False, domains=dom, device=DEV))
    return path, dom, str(out), res


def test_the_stage_writes_its_files(stage):
    import pandas as pd
    from spadot_amd.hotspots import DOMAIN_COLUMNS, FIELDS, TABLE_COLUMNS
    path, dom, out, res = stage
    tps = ["E10", "E12", "E14"]
    assert res["timepoints"] == tps and set(res["timings"]) == {"read_s", "graph_s", "device_s", "write_s", "total_s"}
    assert TABLE_COLUMNS == ("gene", "I", "n_HH", "n_LL", "n_LH", "n_HL") and DOMAIN_COLUMNS == ("gene", "domain", "n_HH", "n_LL",
                                                                                               "size")
    sel = res["genes"]
    assert 8 <= sel.size <= 24 and np.all(np.diff(sel) > 0) and set(sel) <= set(range(20))
    assert np.sum(sel < 10) >= 8                                                     # the domain-following genes dominate
    z = np.load(os.path.join(out, "s_hotspots.npz"))
    assert z["timepoints"].tolist() == tps and z["genes"].tolist() == [f"g{g:02d}" for g in sel]
    assert (int(z["k"]), int(z["n_perms"]), int(z["seed"]), float(z["alpha"])) == (6, 99, 3, 0.05)
    raw = np.load(path)
    labels = pd.read_csv(dom)["kmeans"].to_numpy()
    for tp, n in zip(tps, (400, 500, 600)):
        r = res["results"][tp]
        for name in FIELDS:
            assert z[f"{tp}_{name}"].shape == (sel.size, n)
            np.testing.assert_array_equal(z[f"{tp}_{name}"], getattr(r, name), err_msg=f"{tp}_{name}")
        spots = z[f"{tp}_spots"]
        assert spots.shape == (n,) and np.all(raw["timepoint"][spots] == tp)
        assert z[f"{tp}_quadrant"].dtype == np.int8 and z[f"{tp}_ge"].dtype == np.int32
        assert np.all(r.ge + r.le >= 99) and r.has_neighbours.all() and not r.degenerate.any()
        tab = pd.read_csv(os.path.join(out, f"s_hotspots_{tp}.csv"))
        assert tuple(tab.columns) == TABLE_COLUMNS and tab["gene"].tolist() == z["genes"].tolist()
        np.testing.assert_allclose(tab["I"], r.I.sum(1) / (6 * n), rtol=1e-12)
        sig = r.p_sim <= 0.05
        np.testing.assert_array_equal(tab["n_HH"], (sig & (r.quadrant == 1)).sum(1))
        np.testing.assert_array_equal(tab["n_HL"], (sig & (r.quadrant == 4)).sum(1))
        dt = pd.read_csv(os.path.join(out, f"s_hotspots_domains_{tp}.csv"))
        K = {"E10": 4, "E12": 5, "E14": 6}[tp]
        assert tuple(dt.columns) == DOMAIN_COLUMNS and len(dt) == sel.size * K
        lab = labels[spots]
        for j, g in enumerate(sel):
            rows = dt[dt["gene"] == f"g{g:02d}"]
            assert rows["domain"].tolist() == list(range(K)) and rows["size"].tolist() == np.bincount(lab, minlength=K).tolist()
            assert rows["n_HH"].sum() == tab["n_HH"][j] and rows["n_LL"].sum() == tab["n_LL"][j]
            if g < 10 and rows["size"].iloc[g % K] >= 30:                            # a marker: its hot spots lie in its domain
                hh = rows["n_HH"].to_numpy()
                print(f"{tp} g{g:02d}: HH per domain {hh.tolist()}, marked domain {g % K}")
                # Outside its domain a marker is noise: the folded p puts about 10 % of the spots at p_sim <= 0.05 (module
                # docstring of spadot_amd.hotspots) in whichever quadrant they lie, at most a third of them HH: a density near
                # 0.03, against the interior of the marked domain, where every spot is HH.  Asserted: most HH spots lie in the
                # marked domain, at five times the density of the rest.
                size, m = rows["size"].to_numpy(), g % K
                assert 2 * hh[m] > hh.sum() and hh[m] * (n - size[m]) >= 5 * (hh.sum() - hh[m]) * size[m]


def test_a_second_run_and_the_sub_command_write_the_same_bytes(stage, tmp_path):
    from spadot_amd.hotspots import hotspots
    path, dom, out, res = stage
    names = ["s_hotspots.npz"] + [f"s_hotspots_{tp}.csv" for tp in res["timepoints"]] + \
            [f"s_hotspots_domains_{tp}.csv" for tp in res["timepoints"]]
    hotspots(argparse.Namespace(data=path, output_dir=str(tmp_path), prefix="s_", k=6, n_perms=99, seed=3, top=8, genes=None,
                                alpha=0.05, fdr=False, domains=dom, device=DEV))
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(tmp_path, name), "rb").read(), name
    sub = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "spadot_amd", "hotspots", "-i", path, "-o", str(sub), "--prefix", "s_", "--n_perms",
                        "99", "--seed", "3", "--top", "8", "--domains", dom, "--device", DEV], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(sub, name), "rb").read(), name
    named = hotspots(argparse.Namespace(data=path, output_dir=str(tmp_path / "named"), prefix="", k=6, n_perms=99, seed=3, top=8,
                                        genes="g03,g12", alpha=0.05, fdr=True, domains=None, device=DEV))
    assert named["genes"].tolist() == [3, 12] and not named["domain_tables"]
    j = int(np.flatnonzero(res["genes"] == 3)[0]) if 3 in res["genes"] else None
    if j is not None:
        np.testing.assert_array_equal(named["results"]["E12"].ge[0], res["results"]["E12"].ge[j])
    a = named["results"]["E12"]
    np.testing.assert_array_equal(named["tables"]["E12"]["n_HH"], ((a.padj <= 0.05) & (a.quadrant == 1)).sum(1))
