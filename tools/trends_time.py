#!/usr/bin/env python3
"""Time of the trends stage on the MI355X:

    python tools/trends_time.py [--tps 5] [--n 10000] [--genes 3000] [--density 0.1] [--columns 33,161] [--repeats 7]
                                [--host-tps 1] [--skip-host] [--skip-stage]

Synthetic raw counts (per time point a Bernoulli(density) mask times 1 + Poisson counts), W uniform random, every column
normalised per time point, then per column count C
  * the launch alone (spadot_weighted_moments), warm, device events, the median of `--repeats`, with its spread;
  * bytes: the rows of W the kernel gathers (stored entries x C x 8 B) per second, and what it writes (3 T G C x 8 B);
  * the whole stage: gene_trends with C - 1 columns (it appends the column of ones), first call and a warm call, split into
    upload, device and host;
  * the yardstick: the three products X_csc.T @ W with scipy on the same values, the genes cut into 16 blocks on 16 threads,
    on the first `--host-tps` time points and that time SCALED to all of them (`host_scipy_scaled_s`: not measured at full
    size unless --host-tps covers every time point).
Prints one JSON line per column count."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOST_THREADS = 16


def raw_counts(tps, n, genes, density, seed=1993):
    import scipy.sparse as sp
    from spadot_amd.utils._preprocess_utils import RawCounts
    rng = np.random.default_rng(seed)
    blocks = []
    for t in range(tps):
        rows, cols = [], []
        for lo in range(0, n, 1000):                           # the mask in slabs: a few hundred MB at most
            m = rng.random((min(1000, n - lo), genes), dtype=np.float32) < density
            r, c = np.nonzero(m)
            rows.append((r + lo).astype(np.int32)); cols.append(c.astype(np.int32))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        vals = (1 + rng.poisson(0.7, size=rows.size)).astype(np.float32)
        blocks.append(sp.csr_matrix((vals, (rows, cols)), shape=(n, genes)))
        print(f"  counts of time point {t}: {rows.size} entries", file=sys.stderr, flush=True)
    X = sp.vstack(blocks).tocsr()
    return RawCounts(X, np.repeat(np.arange(tps), n), rng.random((tps * n, 2)), np.array([f"g{i}" for i in range(genes)]))


def host_scipy(dc, values, W, tps):
    """S0, S1, S2 of the first `tps` time points with scipy, the genes in 16 blocks on 16 threads: seconds."""
    import scipy.sparse as sp
    from concurrent.futures import ThreadPoolExecutor
    colptr, ridx = dc.colptr.cpu().numpy(), dc.ridx.cpu().numpy()
    Xt = sp.csr_matrix((values.astype(np.float64), ridx, colptr), shape=(dc.G, dc.n))      # genes x spots: the CSC as a CSR
    off = dc.tp_off_host
    edges = np.linspace(0, dc.G, HOST_THREADS + 1).astype(int)
    total = 0.0
    for t in range(tps):
        lo, hi = int(off[t]), int(off[t + 1])
        Xs = Xt[:, lo:hi].tocsr()
        X2, X0 = Xs.copy(), Xs.copy()
        X2.data = X2.data * X2.data
        X0.data[:] = 1.0
        Wt = W[lo:hi]
        jobs = [(M[a:b], Wt) for M in (X0, Xs, X2) for a, b in zip(edges[:-1], edges[1:])]
        t0 = time.perf_counter()                                   # the products alone
        with ThreadPoolExecutor(max_workers=HOST_THREADS) as ex:
            list(ex.map(lambda j: j[0] @ j[1], jobs))
        total += time.perf_counter() - t0
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=3000)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--columns", type=str, default="33,161")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-tps", type=int, default=1)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-stage", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.trends import gene_trends, lognorm_values, weighted_moments
    assert torch.cuda.is_available(), "trends_time measures on the MI355X"
    t0 = time.perf_counter()
    raw = raw_counts(a.tps, a.n, a.genes, a.density)
    base = {"shape": f"{a.tps} x {a.n} x {a.genes}", "density": a.density, "nnz": int(raw.X.nnz),
            "make_data_s": round(time.perf_counter() - t0, 2)}
    t0 = time.perf_counter()
    dc = DeviceCounts(raw, "cuda:0")
    torch.cuda.synchronize()
    base["upload_s"] = round(time.perf_counter() - t0, 3)
    values = lognorm_values(dc)
    seg = np.diff(dc.colptr.cpu().numpy())
    base["mean_segment"] = round(float(seg.mean()) / a.tps, 1)
    rng = np.random.default_rng(7)
    for C in [int(c) for c in a.columns.split(",")]:
        rec = dict(base, columns=C)
        W = rng.random((dc.n, C))
        for t in range(dc.T):
            lo, hi = int(dc.tp_off_host[t]), int(dc.tp_off_host[t + 1])
            W[lo:hi] /= W[lo:hi].sum(0)
        Wd = torch.as_tensor(W, device="cuda:0")
        for _ in range(2):                                         # warm
            S = weighted_moments(dc, values, Wd)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            S = weighted_moments(dc, values, Wd)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        del S
        rec["moments_ms"] = round(statistics.median(ms), 3)
        rec["moments_spread_ms"] = [round(min(ms), 3), round(max(ms), 3)]
        rec["gathered_bytes"] = int(raw.X.nnz) * C * 8
        rec["written_bytes"] = 3 * dc.T * dc.G * C * 8
        rec["gather_TBps"] = round(rec["gathered_bytes"] / (rec["moments_ms"] * 1e-3) / 1e12, 3)
        rec["Gfma_per_s"] = round(3 * int(raw.X.nnz) * C / (rec["moments_ms"] * 1e-3) / 1e9, 1)
        if not a.skip_stage and C > 1:
            perm_inv = np.argsort(dc.perm)
            for name in ("stage_first", "stage"):
                res = gene_trends(raw, W[perm_inv][:, :C - 1], device="cuda:0")
                tm = res["timings"]
                rec[name] = {k: round(tm[k], 4) for k in ("total_s", "upload_s", "device_s", "host_s", "lognorm_ms", "moments_ms")}
            del res
        if not a.skip_host:
            tps = max(1, min(a.host_tps, dc.T))
            s = host_scipy(dc, values.cpu().numpy(), W, tps)
            rec["host_scipy_tps"] = tps
            rec["host_scipy_s"] = round(s, 2)
            rec["host_scipy_scaled_s"] = round(s * dc.T / tps, 2)  # scaled to all time points
            rec["host_threads"] = HOST_THREADS
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
