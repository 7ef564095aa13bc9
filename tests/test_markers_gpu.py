"""The markers stage on the MI355X against tests/markers_ref.py, computed on the device's own fp32 values: the integer outputs
(twice the rank sums, Ties, nonzeros per domain) exactly, the fp64 statistics at the tolerances of their arithmetic.  A small
shape with every edge, a shape that straddles the LDS capacity of the sort (both sort paths), K = 32, the log-normalise
kernel, determinism, the stage end to end with its command line, and the refusals."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import markers_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE_SIZES = (400, 1200, 2000)
INT_KEYS = ("r2", "nnz_k", "ties")


def _raw(X, tp, genes=None):
    from spadot_amd.utils._preprocess_utils import RawCounts
    X = sp.csr_matrix(np.asarray(X, dtype=np.float32))
    rng = np.random.default_rng(11)
    genes = np.array([f"g{i}" for i in range(X.shape[1])]) if genes is None else genes
    return RawCounts(X, np.asarray(tp), rng.random((X.shape[0], 2)), genes)


def check_against_ref(res, labels):
    """Every time point of a find_markers result against the restatement on the device's own values."""
    lab = np.asarray(labels)[res["perm"]]
    for t in range(len(res["timepoints"])):
        lo, hi = int(res["tp_off"][t]), int(res["tp_off"][t + 1])
        K = res["score"][t].shape[1]
        V = ref.dense_values(res, t)
        want = ref.ranksum_timepoint(V, lab[lo:hi], K)
        np.testing.assert_array_equal(res["r2"][t], want["r2"])
        np.testing.assert_array_equal(res["ties"][t], np.asarray(want["ties"], dtype=np.int64))
        np.testing.assert_array_equal(res["nnz_k"][t], want["nnz_k"])
        np.testing.assert_array_equal(res["n_k"][t], want["n_k"])
        np.testing.assert_allclose(res["vsum"][t], want["vsum"], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(res["U1"][t], want["U1"])
        np.testing.assert_allclose(res["score"][t], want["score"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(res["pval"][t], want["pval"], rtol=1e-10, atol=1e-300)
        # the host's columns from the same integers and sums
        n = hi - lo
        n1 = want["n_k"].astype(np.float64)[None, :]
        np.testing.assert_allclose(res["mean_in"][t], want["vsum"] / n1, rtol=1e-12)
        tot, cnt = want["vsum"].sum(1, keepdims=True), want["nnz_k"].sum(1, keepdims=True)
        if K > 1:
            np.testing.assert_allclose(res["mean_out"][t], (tot - want["vsum"]) / (n - n1), rtol=1e-11, atol=1e-14)
            np.testing.assert_allclose(res["pct_out"][t], (cnt - want["nnz_k"]) / (n - n1), rtol=1e-12)
            np.testing.assert_allclose(res["auc"][t], want["U1"] / (n1 * (n - n1)), rtol=1e-12)
        np.testing.assert_allclose(res["pct_in"][t], want["nnz_k"] / n1, rtol=1e-12)
        np.testing.assert_allclose(res["log2fc"][t], np.log2((np.expm1(res["mean_in"][t]) + 1e-9) /
                                                              (np.expm1(res["mean_out"][t]) + 1e-9)), rtol=1e-12, atol=1e-14)
        expressed = cnt[:, 0] > 0
        for k in range(K):
            np.testing.assert_allclose(res["padj"][t][expressed, k], ref.bh(res["pval"][t][expressed, k]), rtol=1e-14)
            assert np.all(res["padj"][t][~expressed, k] == 1.0) and np.all(res["pval"][t][~expressed, k] == 1.0)
            assert np.all(res["score"][t][~expressed, k] == 0.0)


# ---------------------------------------------------------------------------------------------------------------- small shape
def _small():
    """T = 2 with 37 and 300 spots, 40 genes, K = 3 and 5, with every edge of the issue."""
    rng = np.random.default_rng(1993)
    n0, n1, G = 37, 300, 40
    n = n0 + n1
    X = rng.poisson(0.6, size=(n, G)).astype(np.float32) * (rng.random((n, G)) < 0.5)
    tp = np.repeat(np.array(["d0", "d1"]), [n0, n1])
    labels = np.concatenate([rng.integers(0, 2, size=n0), rng.integers(0, 4, size=n1)])
    labels[5] = 2                      # time point 0: domain 2 has one spot
    labels[n0 + 17] = 4                # time point 1: domain 4 has one spot
    X[:n0, 3] = 0                      # all zero in time point 0 ...
    X[n0:, 3] = rng.poisson(2.0, size=n1)
    X[:, 4] = 1 + rng.poisson(1.0, size=n)                 # nonzero in every spot (Z = 0)
    X[:, 5] = 0
    X[rng.choice(n0, 11, replace=False), 5] = 2            # all nonzeros equal (per row total: see gene 39)
    X[n0 + rng.choice(n1, 90, replace=False), 5] = 2
    X[:, 6] = 0
    X[9, 6] = 3                        # a single nonzero per time point
    X[n0 + 100, 6] = 1
    X[:, 7] = np.where(labels == 1, 0, X[:, 7])            # domain 1 has no nonzero of gene 7
    X[:, 8] = 0                        # all zero everywhere
    X[:, 39] = 0
    X[:, 39] = 200 - X.sum(1)          # equal row totals: equal counts give equal v, so gene 5's nonzeros tie
    assert X.min() >= 0
    return X, tp, labels


@pytest.fixture(scope="module")
def small():
    from spadot_amd.markers import find_markers
    X, tp, labels = _small()
    return find_markers(_raw(X, tp), labels, device=DEV), X, tp, labels


def test_small_shape_with_every_edge(small):
    res, X, tp, labels = small
    assert [str(t) for t in res["timepoints"]] == ["d0", "d1"]
    assert [s.shape for s in res["score"]] == [(40, 3), (40, 5)]
    assert res["n_k"][0][2] == 1 and res["n_k"][1][4] == 1
    V0, V1 = ref.dense_values(res, 0), ref.dense_values(res, 1)
    assert not V0[:, 3].any() and (V0[:, 4] > 0).all() and (V1[:, 4] > 0).all()        # all zero; Z = 0
    assert np.unique(V1[:, 5]).size == 2 and (V1[:, 5] > 0).sum() == 90                   # all nonzeros equal
    assert (V0[:, 6] > 0).sum() == 1 and (V1[:, 6] > 0).sum() == 1
    assert res["nnz_k"][1][7, 1] == 0 and res["nnz_k"][1][7].sum() > 0
    check_against_ref(res, labels)
    # an all-zero gene: every spot tied, (0, 1) and not scipy's NaN
    assert np.all(res["score"][0][3] == 0) and np.all(res["pval"][0][3] == 1) and np.all(res["padj"][0][3] == 1)
    assert res["ties"][0][3] == 37 ** 3 - 37
    assert res["timings"]["long_segments"] == 0


def test_one_domain_time_point_gives_zero_scores():
    from spadot_amd.markers import find_markers
    X, tp, labels = _small()
    labels = np.where(tp == "d0", 0, labels)               # time point 0 is one domain: n2 = 0
    res = find_markers(_raw(X, tp), labels, device=DEV)
    assert res["score"][0].shape == (40, 1)
    assert np.all(res["score"][0] == 0) and np.all(res["pval"][0] == 1) and np.all(res["padj"][0] == 1)
    check_against_ref(res, labels)


# ---------------------------------------------------------------------------------------------------------------- both sort paths
def _straddle(cap):
    rng = np.random.default_rng(7)
    n, G = cap + 1000, 8
    X = np.zeros((n, G), dtype=np.float32)
    for g, m in ((0, cap - 1), (1, cap), (2, cap + 1), (5, cap + 500), (6, 100)):
        X[rng.choice(n, m, replace=False), g] = rng.integers(1, 3 if g == 5 else 50, size=m)
    X[:, 3] = rng.integers(1, 4, size=n)                   # dense, values from {1, 2, 3}: long tie runs
    X[:, 4] = 1 + rng.permutation(n)                       # dense, all distinct
    X[:, 7] = 20000 - X.sum(1)                             # dense; makes every row total 20000, so v is a function of the count
    assert (X[:, 7] >= 1).all()
    return X, np.zeros(n, dtype=np.int64), rng.integers(0, 4, size=n)


@pytest.fixture(scope="module")
def straddle():
    from spadot_amd._lib import model_lib
    from spadot_amd.markers import find_markers
    cap = int(model_lib().spadot_mk_lds_capacity())
    X, tp, labels = _straddle(cap)
    return find_markers(_raw(X, tp), labels, device=DEV), X, tp, labels, cap


def test_segments_on_both_sides_of_the_lds_capacity(straddle):
    res, X, tp, labels, cap = straddle
    assert cap >= 256
    nnz = (ref.dense_values(res, 0) > 0).sum(0)
    np.testing.assert_array_equal(nnz, [cap - 1, cap, cap + 1, cap + 1000, cap + 1000, cap + 500, 100, cap + 1000])
    assert res["timings"]["long_segments"] == 5 and res["timings"]["lds_capacity"] == cap     # both paths ran
    V = ref.dense_values(res, 0)
    assert np.unique(V[:, 3]).size == 3 and np.unique(V[:, 4]).size == cap + 1000
    check_against_ref(res, labels)


def test_k32():
    from spadot_amd.markers import find_markers
    rng = np.random.default_rng(32)
    n, G = 2000, 16
    X = rng.poisson(rng.uniform(0.05, 2.0, size=G)[None, :], size=(n, G)).astype(np.float32)
    labels = rng.permutation(np.arange(n) % 32)
    res = find_markers(_raw(X, np.zeros(n, dtype=np.int64)), labels, device=DEV)
    assert res["score"][0].shape == (16, 32)
    check_against_ref(res, labels)


# ---------------------------------------------------------------------------------------------------------------- lognorm
def test_lognorm_kernel_matches_numpy_to_one_ulp(small, straddle):
    for res, X, tp, labels, *_ in (small, straddle):
        Xp = np.asarray(X, dtype=np.float64)[res["perm"]]
        want = ref.lognorm(Xp, Xp.sum(1))
        for t in range(len(res["timepoints"])):
            lo, hi = int(res["tp_off"][t]), int(res["tp_off"][t + 1])
            got = ref.dense_values(res, t)
            w = want[lo:hi]
            np.testing.assert_array_equal(got > 0, w > 0)
            ulp = np.spacing(np.maximum(np.abs(w), np.float32(1e-30)).astype(np.float32))
            assert np.all(np.abs(got.astype(np.float64) - w.astype(np.float64)) <= ulp.astype(np.float64))
        assert res["values"].dtype == np.float32


# ---------------------------------------------------------------------------------------------------------------- determinism
def test_two_runs_are_bitwise_identical(small, straddle):
    from spadot_amd.markers import find_markers
    for first, X, tp, labels, *_ in (small, straddle):
        again = find_markers(_raw(X, tp), labels, device=DEV)
        assert again["values"].tobytes() == first["values"].tobytes()
        for key in ("score", "pval", "padj", "log2fc", "mean_in", "mean_out", "pct_in", "pct_out", "auc", "U1", "vsum") + INT_KEYS:
            for a, b in zip(first[key], again[key]):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), key


# ---------------------------------------------------------------------------------------------------------------- stage
@pytest.fixture(scope="module")
def stage_inputs(tmp_path_factory):
    import pandas as pd
    from spadot_amd.synthetic import make_raw_counts
    d = tmp_path_factory.mktemp("markers")
    data = make_raw_counts(STAGE_SIZES, n_genes=1500)
    X = sp.csr_matrix(data.X)
    tp = np.asarray(data.obs["timepoint"])
    xy = np.asarray(data.obsm["spatial"], dtype=np.float64)
    counts = str(d / "counts.npz")
    np.savez(counts, X_data=X.data, X_indices=X.indices, X_indptr=X.indptr, X_shape=np.asarray(X.shape), timepoint=tp,
             spatial=xy, genes=np.asarray(data.var_names))
    quad = np.empty(tp.size, dtype=np.int64)
    for t in np.unique(tp):
        m = tp == t
        u = (xy[m] - xy[m].min(0)) / np.maximum(np.ptp(xy[m], 0), 1e-12)
        quad[m] = 2 * (u[:, 0] >= 0.5) + (u[:, 1] >= 0.5)
    csv = str(d / "domains.csv")
    pd.DataFrame({"row": np.arange(tp.size), "timepoint": tp, "kmeans": quad, "pixel_x": xy[:, 0],
                  "pixel_y": xy[:, 1]}).to_csv(csv, index=False)
    return d, counts, csv, quad, data.uns["module"]


def test_stage_writes_its_files_and_finds_the_planted_modules(stage_inputs):
    import pandas as pd
    from spadot_amd.markers import CSV_COLUMNS, markers
    d, counts, csv, quad, module = stage_inputs
    out = str(d / "out")
    res = markers(argparse.Namespace(data=counts, domains=csv, output_dir=out, prefix="m_", top=30, device=DEV))
    z = np.load(os.path.join(out, "m_markers.npz"), allow_pickle=False)
    assert z["timepoints"].tolist() == ["0", "1", "2"] and z["genes"].shape == (1500,)
    assert z["domains"].tolist() == [f"{t}_{k}" for t in range(3) for k in range(4)]
    for t in range(3):
        for c in ("score", "pval", "padj", "log2fc", "mean_in", "mean_out", "pct_in", "pct_out", "auc"):
            assert z[f"{c}_{t}"].tobytes() == res[c][t].tobytes()                       # the npz round-trips
        tab = pd.read_csv(os.path.join(out, f"m_markers_{t}.csv"))
        assert tuple(tab.columns) == CSV_COLUMNS and len(tab) == 4 * 30
        assert tab["domain"].tolist() == sorted(tab["domain"].tolist())
        pos = {g: i for i, g in enumerate(res["genes"].tolist())}
        for k in range(4):
            part = tab[tab["domain"] == k]
            col = np.array([pos[g] for g in part["gene"]])
            sc = part["score"].to_numpy()
            assert np.all(np.diff(sc) <= 0)                                             # score descending ...
            same = np.diff(sc) == 0
            assert np.all(np.diff(col)[same] > 0)                                       # ... then gene column
            np.testing.assert_allclose(sc, res["score"][t][col, k], rtol=1e-15)
            want = np.lexsort((np.arange(1500), -res["score"][t][:, k]))[:30]
            np.testing.assert_array_equal(col, want)
            if k in (0, 2):                                                             # the planted module of the quadrant
                assert (module[col] == k).sum() >= 27, (t, k, module[col])
    check_against_ref(res, quad)


def test_command_line_markers(stage_inputs):
    d, counts, csv, _, _ = stage_inputs
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = str(d / "cli")
    p = subprocess.run([sys.executable, "-m", "spadot_amd", "markers", "-i", counts, "--domains", csv, "-o", out, "--top", "5"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert {"markers.npz", "markers_0.csv", "markers_1.csv", "markers_2.csv"} <= set(os.listdir(out))
    with open(os.path.join(out, "markers_2.csv")) as f:
        assert len(f.read().splitlines()) == 1 + 4 * 5


def test_stage_reads_a_preprocess_style_npz(stage_inputs, tmp_path):
    from spadot_amd.markers import markers
    d, counts, csv, quad, _ = stage_inputs
    z = np.load(counts, allow_pickle=False)
    n = int(z["X_shape"][0])
    C = sp.csr_matrix((z["X_data"], z["X_indices"], z["X_indptr"]), shape=(n, int(z["X_shape"][1])))[:, :50].tocsr()
    f = str(tmp_path / "preprocessed_counts.npz")
    np.savez(f, X=np.zeros((n, 2), dtype=np.float32), timepoint=z["timepoint"], spatial=z["spatial"], genes=z["genes"][:50],
             counts_data=C.data, counts_indices=C.indices, counts_indptr=C.indptr, counts_shape=np.asarray(C.shape))
    res = markers(argparse.Namespace(data=f, domains=csv, output_dir=str(tmp_path), prefix="", top=0, device=DEV))
    assert res["score"][2].shape == (50, 4)
    check_against_ref(res, quad)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(monkeypatch):
    from spadot_amd import markers as mk
    X, tp, labels = _small()
    calls = []
    monkeypatch.setattr(mk.MarkerKernels, "lognorm", lambda self: calls.append("lognorm"))
    monkeypatch.setattr(mk.MarkerKernels, "ranksum", lambda self: calls.append("ranksum"))
    bad = labels.copy()
    bad[40:73] = np.arange(33)                             # 33 domains in time point 1
    with pytest.raises(ValueError, match="33 domains"):
        mk.find_markers(_raw(X, tp), bad, device=DEV)
    with pytest.raises(ValueError, match="cuda device"):
        mk.find_markers(_raw(X, tp), labels, device="cpu")
    with pytest.raises(ValueError, match="one domain per row"):
        mk.find_markers(_raw(X, tp), labels[:-1], device=DEV)
    assert calls == []


def test_entry_points_refuse_what_is_over_the_limits():
    import torch
    from spadot_amd._lib import model_lib
    lib = model_lib()
    assert lib.spadot_mk_ranksum_scratch_bytes(1, 4, 2097152) == -7
    assert lib.spadot_mk_ranksum_scratch_bytes(1, 4, 2097151) > 0
    buf = torch.zeros(4096, dtype=torch.int64, device=DEV)
    p = buf.data_ptr()
    for K, nmax in ((33, 100), (4, 2097152)):              # refused before anything is launched: `buf` stays zero
        assert lib.spadot_mk_ranksum(p, p, p, p, p, p, 1, 4, K, nmax, p, 32768, p, p, p, p, None) == -7
    assert lib.spadot_mk_finish(p, p, p, p, 1, 4, 33, p, p, p, None) == -7
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0
