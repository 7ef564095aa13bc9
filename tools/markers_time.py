#!/usr/bin/env python3
"""Time of the markers stage on the MI355X:

    python tools/markers_time.py [--tps 5] [--n 10000] [--genes 3000] [--density 0.1] [--domains 10] [--repeats 7]
                                 [--host-genes 100] [--skip-host]

Synthetic raw counts (per time point a Bernoulli(density) mask times 1 + Poisson counts, a random domain per spot), then
  * upload: DeviceCounts (row permutation, CSR -> CSC on the host, copies);
  * the launches alone, warm, device events, the median of `--repeats`: row totals (spadot_pre_row_total), spadot_mk_lognorm,
    spadot_mk_ranksum (which sort path the segments take is printed: `long_segments` of `segments` go through global
    memory), spadot_mk_finish;
  * the whole stage: find_markers, first call and a warm call, split into upload, device and host (means, BH, copies back);
  * the yardstick: scipy.stats.mannwhitneyu in a loop over (time point, domain, gene) on the first `--host-genes` genes of the
    same values, one thread, and that time SCALED to all genes (`host_scipy_scaled_s`: not measured at full size);
  * bytes: what spadot_mk_ranksum has to read (value + row index + label per stored entry) and write.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def raw_counts(tps, n, genes, density, domains, seed=1993):
    import scipy.sparse as sp
    from spadot_amd.utils._preprocess_utils import RawCounts
    rng = np.random.default_rng(seed)
    blocks = []
    for t in range(tps):
        rows, cols = [], []
        for lo in range(0, n, 1000):                           # the mask in slabs: a few hundred MB at most
            m = rng.random((min(1000, n - lo), genes)) < density
            r, c = np.nonzero(m)
            rows.append(r + lo); cols.append(c)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        vals = (1 + rng.poisson(0.7, size=rows.size)).astype(np.float32)
        blocks.append(sp.csr_matrix((vals, (rows, cols)), shape=(n, genes)))
    X = sp.vstack(blocks).tocsr()
    labels = rng.integers(0, domains, size=tps * n)
    raw = RawCounts(X, np.repeat(np.arange(tps), n), rng.random((tps * n, 2)), np.array([f"g{i}" for i in range(genes)]))
    return raw, labels


def host_scipy(res, labels, genes):
    """The scipy loop on the first `genes` genes of the device's own values: seconds, tests."""
    from scipy.stats import mannwhitneyu
    lab = np.asarray(labels)[res["perm"]]
    colptr, ridx, val = res["colptr"], res["ridx"], res["values"]
    tests = 0
    t0 = time.perf_counter()
    for t in range(len(res["timepoints"])):
        lo, hi = int(res["tp_off"][t]), int(res["tp_off"][t + 1])
        l = lab[lo:hi]
        K = res["score"][t].shape[1]
        for g in range(genes):
            a, b = int(colptr[g]), int(colptr[g + 1])
            r = ridx[a:b]
            sel = (r >= lo) & (r < hi)
            v = np.zeros(hi - lo, dtype=np.float64)
            v[r[sel] - lo] = val[a:b][sel]
            for k in range(K):
                m = l == k
                with np.errstate(divide="ignore", invalid="ignore"):
                    mannwhitneyu(v[m], v[~m], alternative="two-sided", method="asymptotic", use_continuity=True)
                tests += 1
    return time.perf_counter() - t0, tests


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=3000)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--domains", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-genes", type=int, default=100)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd.markers import MarkerKernels, check_labels, find_markers
    from spadot_amd.preprocess import DeviceCounts
    assert torch.cuda.is_available(), "markers_time measures on the MI355X"
    t0 = time.perf_counter()
    raw, labels = raw_counts(a.tps, a.n, a.genes, a.density, a.domains)
    rec = {"shape": f"{a.tps} x {a.n} x {a.genes}", "domains": a.domains, "density": a.density, "nnz": int(raw.X.nnz),
           "make_data_s": round(time.perf_counter() - t0, 2)}

    # the whole stage: first call (code objects, allocator), then warm
    for name in ("stage_first", "stage"):
        res = find_markers(raw, labels, device="cuda:0")
        tm = res["timings"]
        rec[name] = {k: round(tm[k], 4) for k in ("total_s", "upload_s", "device_s", "host_s")}
    rec["segments"] = a.tps * a.genes
    rec["long_segments"] = tm["long_segments"]
    rec["lds_capacity"] = tm["lds_capacity"]
    seg = np.diff(np.asarray(res["colptr"]))                       # nonzeros per gene over all time points (a bound per segment)
    rec["sort_path"] = "LDS only" if tm["long_segments"] == 0 else f"{tm['long_segments']} segments through global memory"
    rec["mean_segment"] = round(float(seg.mean()) / a.tps, 1)

    # the launches alone
    lab, _, ks = check_labels(labels, raw.obs["timepoint"])
    t0 = time.perf_counter()
    dc = DeviceCounts(raw, "cuda:0")
    torch.cuda.synchronize()
    rec["upload_s"] = round(time.perf_counter() - t0, 3)
    mk = MarkerKernels(dc, lab[dc.perm], max(ks))
    steps = [("row_total_ms", mk.row_totals), ("lognorm_ms", mk.lognorm), ("ranksum_ms", mk.ranksum), ("finish_ms", mk.finish)]
    for _, fn in steps:                                            # warm
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in steps}
    for _ in range(a.repeats):
        for name, fn in steps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    for name, v in times.items():
        rec[name] = round(statistics.median(v), 3)
        rec[name.replace("_ms", "_spread_ms")] = [round(min(v), 3), round(max(v), 3)]
    rec["kernels_ms"] = round(sum(rec[name] for name, _ in steps), 3)
    nnz, TGK = int(raw.X.nnz), a.tps * a.genes * max(ks)
    rec["ranksum_bytes"] = int(nnz * 12 + TGK * (8 + 4 + 8) + a.tps * a.genes * (8 + 16))
    rec["ranksum_GBps"] = round(rec["ranksum_bytes"] / (rec["ranksum_ms"] * 1e-3) / 1e9, 1)
    rec["ranksum_Mkeys_per_s"] = round(nnz / (rec["ranksum_ms"] * 1e-3) / 1e6, 1)

    if not a.skip_host:
        hg = min(a.host_genes, a.genes)
        s, tests = host_scipy(res, labels, hg)
        rec["host_scipy_genes"] = hg
        rec["host_scipy_tests"] = tests
        rec["host_scipy_s"] = round(s, 2)
        rec["host_scipy_scaled_s"] = round(s * a.genes / hg, 1)    # scaled to all genes, not measured at full size
        rec["host_threads"] = 1
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
