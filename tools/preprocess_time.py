#!/usr/bin/env python3
"""Wall time of the preprocess stage on the MI355X (DESIGN "The preprocess stage"):

    python tools/preprocess_time.py [--tps 4] [--n 12500] [--genes 20000] [--density 0.1] [--threads 16] [--skip-host]

Synthetic raw counts (per time point a jittered grid, Poisson counts whose rate gives ~density nonzeros, a spatial pattern on
the first 200 genes), then
  * device SPARK-X: gene detection, row totals, k_sparkx_moments and k_sparkx_pvals of every time point, host plumbing
    included (first call, and a second call on warm code objects and allocator);
  * the whole stage: preprocess_counts with feature selection (SPARK-X, ordering, gene clusters, scaling), and the gene
    clusters of all time points alone;
  * host: the numpy / scipy restatement of the statistic (the 11 sparse products of _sparkx_sk and the two-term p-values,
    vectorised) on `--threads` threads, for the same time points;
  * k_sparkx_moments and k_sparkx_pvals alone (device events around the launches);
  * bytes moved by k_sparkx_moments: the nonzeros of the kept genes (value + row index + row map entry) plus one 176-byte
    kernel-coordinate row gathered per nonzero, plus the 24 moments written per gene.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def raw_counts(tps, n, genes, density, seed=1993):
    import scipy.sparse as sp
    from spadot_amd.synthetic import make_timepoint
    from spadot_amd.utils._preprocess_utils import RawCounts
    rng = np.random.default_rng(seed)
    rate = -np.log1p(-density)                   # P[Poisson(rate) > 0] = density
    blocks, locs = [], []
    for t in range(tps):
        xy, _, _ = make_timepoint(n, 1, seed + 17 * t)
        u = (xy - xy.min(0)) / np.ptp(xy, 0)
        nnz_rows = rng.binomial(genes, density, size=n)
        rows = np.repeat(np.arange(n), nnz_rows)
        cols = np.concatenate([rng.choice(genes, k, replace=False) for k in nnz_rows])
        vals = 1 + rng.poisson(rate, size=rows.size)
        sel = cols < 200                                          # patterned genes: more counts in one corner
        vals[sel] += rng.poisson(3.0 * np.exp(-((u[rows[sel]] - 0.3) ** 2).sum(1) / 0.02))
        blocks.append(sp.csr_matrix((vals.astype(np.float32), (rows, cols)), shape=(n, genes)))
        locs.append(xy)
    X = sp.vstack(blocks).tocsr()
    return RawCounts(X, np.repeat(np.arange(tps), n), np.concatenate(locs), np.array([f"g{i}" for i in range(genes)]))


def host_statistic(dc, per, threads):
    """_sparkx_sk restated with numpy / scipy on the host (vectorised p-values): wall time over all time points."""
    from threadpoolctl import threadpool_limits
    from spadot_amd.utils._preprocess_utils import kernel_coordinates
    t0 = time.perf_counter()
    with threadpool_limits(threads):
        for t, r in enumerate(per):
            lo, hi = dc.tp_off_host[t], dc.tp_off_host[t + 1]
            C = dc.X[lo:hi][:, r["genes"]][r["spots"] - lo].tocsc().astype(np.float64)
            xt, inv, lam = kernel_coordinates(dc.spatial[r["spots"]])
            n = C.shape[0]
            syy = np.asarray(C.power(2).sum(0)).ravel()
            ybar = np.asarray(C.mean(0)).ravel()
            ylam = 1 - n * ybar ** 2 / syy
            for k in range(11):
                ehl = np.asarray(C.T @ xt[:, 2 * k:2 * k + 2])
                a = inv[k].reshape(2, 2)
                stat = np.einsum("ij,jk,ik->i", ehl, a, ehl) * n / syy
                np.exp(-stat / (2 * ylam * lam[k].mean()))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=4)
    ap.add_argument("--n", type=int, default=12500)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd.preprocess import DeviceCounts, preprocess_counts, sparkx
    assert torch.cuda.is_available(), "preprocess_time measures on the MI355X"
    t0 = time.perf_counter()
    raw = raw_counts(a.tps, a.n, a.genes, a.density)
    rec = {"shape": f"{a.tps} x {a.n} x {a.genes}", "density": a.density, "nnz": int(raw.X.nnz),
           "make_data_s": round(time.perf_counter() - t0, 2)}
    t0 = time.perf_counter()
    dc = DeviceCounts(raw, "cuda:0")
    torch.cuda.synchronize()
    rec["upload_s"] = round(time.perf_counter() - t0, 3)
    for name in ("device_sparkx_first_s", "device_sparkx_s"):
        t0 = time.perf_counter()
        per = sparkx(dc)
        torch.cuda.synchronize()
        rec[name] = round(time.perf_counter() - t0, 4)
    tm = {}
    sparkx(dc, timings=tm)                       # the moments and p-value launches alone, timed with events
    rec["moments_kernel_ms"] = round(tm["moments_ms"], 3)
    rec["pvals_kernel_ms"] = round(tm["pvals_ms"], 3)
    nnz_kept = 0
    for t, r in enumerate(per):
        lo, hi = dc.tp_off_host[t], dc.tp_off_host[t + 1]
        nnz_kept += int(dc.X[lo:hi][:, r["genes"]].nnz)
    n_pairs = sum(r["genes"].size for r in per)
    rec["moments_bytes"] = int(nnz_kept * (4 + 4 + 4 + 176) + n_pairs * (24 * 8 + 2 * 8 + 2 * 4))
    rec["moments_bytes_unique"] = int(nnz_kept * 12 + sum(r["spots"].size for r in per) * 176 + n_pairs * 24 * 8)
    rec["moments_nnz"] = nnz_kept
    rec["moments_gathered_TBps"] = round(rec["moments_bytes"] / (tm["moments_ms"] * 1e-3) / 1e12, 2)
    rec["moments_unique_TBps"] = round(rec["moments_bytes_unique"] / (tm["moments_ms"] * 1e-3) / 1e12, 2)
    t0 = time.perf_counter()
    res = preprocess_counts(raw, device="cuda:0")
    torch.cuda.synchronize()
    rec["device_stage_s"] = round(time.perf_counter() - t0, 3)
    rec["svgs"] = int(res["X"].shape[1])
    # the gene clusters alone (scaled block, Gram matrix, eigendecomposition and K-means per time point)
    from spadot_amd.preprocess import cluster_genes
    from spadot_amd.utils._preprocess_utils import rank_genes
    t0 = time.perf_counter()
    for t, r in enumerate(per):
        order, n_keep = rank_genes(r["adjusted"], r["combined"])
        cluster_genes(dc, t, r["genes"][order[:n_keep]], r["total"])
    torch.cuda.synchronize()
    rec["cluster_s"] = round(time.perf_counter() - t0, 3)
    rec["selected_per_tp"] = [int(r["selected"].size) for r in res["sparkx"]]
    if not a.skip_host:
        rec["host_statistic_s"] = round(host_statistic(dc, per, a.threads), 3)
        rec["host_threads"] = a.threads
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
