#!/usr/bin/env python3
"""Wall time of SCTransform and of the Louvain gene clusters on the MI355X ("SCTransform and Louvain"):

    python tools/sctransform_time.py [--tps 4] [--n 12500] [--genes 20000] [--density 0.1] [--threads 16] [--host-genes 500]

The synthetic raw counts of tools/preprocess_time.py, then
  * device SCTransform of every time point (sctransform(dc, t): row totals, gene detection, k_sct_gene_stats, k_sct_fit,
    the host regularisation, k_sct_resid_stats), first call and a second call on warm code objects and allocator;
  * the device time of each launch (events around it): k_sct_gene_stats, k_sct_fit, k_sct_resid_stats, and
    k_sct_resid_write for the first time point's 500 genes of largest residual variance;
  * preprocess_counts with gene_clusters='louvain' end to end (SPARK-X, SCTransform, PCA, gene graph, Louvain, scaling);
  * host: the numpy / scipy restatement of the step-1 fits (tests/sct_ref.py: Poisson IRLS and theta.ml, vectorised over
    genes) on --threads threads for --host-genes step-1 genes of the first time point, scaled to all its step-1 genes;
  * the fp64 transcendental operations k_sct_fit counts (exp / log per spot per iteration, exp + digamma + trigamma per
    nonzero per theta iteration), with the least time they imply at the FP64 vector peak (a spec number, see below).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_VECTOR_TFLOPS = 78.6       # MI355X FP64 vector peak from AMD's public specification (not measured here)
FLOPS_PER_TRANSCENDENTAL = 20   # assumed cost of one fp64 exp / log / digamma step in FMA-class operations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=4)
    ap.add_argument("--n", type=int, default=12500)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-genes", type=int, default=500)
    a = ap.parse_args()
    import torch
    from preprocess_time import raw_counts
    from spadot_amd.preprocess import DeviceCounts, preprocess_counts
    from spadot_amd.sctransform import sctransform
    from spadot_amd._lib import model_lib
    raw = raw_counts(a.tps, a.n, a.genes, a.density)
    out = dict(tps=a.tps, spots_per_tp=a.n, genes=a.genes, density=a.density)
    dc = DeviceCounts(raw, "cuda:0")
    torch.cuda.synchronize()
    for key in ("sct_first_s", "sct_s"):
        t0 = time.perf_counter()
        res, tim = [], []
        for t in range(dc.T):
            d = {}
            res.append(sctransform(dc, t, timings=d))
            tim.append(d)
        torch.cuda.synchronize()
        out[key] = time.perf_counter() - t0
    out["gene_stats_ms"] = sum(d["gene_stats_ms"] for d in tim)
    out["fit_ms"] = sum(d["fit_ms"] for d in tim)
    out["resid_stats_ms"] = sum(d["resid_stats_ms"] for d in tim)
    out["kept_genes"] = [d["kept_genes"] for d in tim]
    out["step1_genes"] = [d["step1_genes"] for d in tim]
    r0 = res[0]
    cols = r0.genes[np.argsort(-r0.gene_attr["residual_variance"], kind="stable")[:500]]
    r0.scale_data(cols)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    r0.scale_data(cols)
    e[1].record()
    e[1].synchronize()
    out["resid_write_ms_500"] = e[0].elapsed_time(e[1])

    # counted transcendental operations of k_sct_fit
    ops = 0.0
    for t, r in enumerate(res):
        lo, hi = dc.tp_off_host[t], dc.tp_off_host[t + 1]
        nnz = np.diff(dc.X[lo:hi].tocsc().indptr)[r.genes[r.step1]]
        pit, tit = r.fit_info[:, 2], r.fit_info[:, 3]
        ops += float((pit * r.N + nnz + tit * (2 * r.N + 3 * nnz)).sum())
    out["fit_transcendentals"] = ops
    out["fit_least_ms_at_fp64_peak"] = ops * FLOPS_PER_TRANSCENDENTAL / (FP64_VECTOR_TFLOPS * 1e12) * 1e3
    out["fp64_vector_tflops_spec"] = FP64_VECTOR_TFLOPS
    out["flops_per_transcendental_assumed"] = FLOPS_PER_TRANSCENDENTAL

    t0 = time.perf_counter()
    preprocess_counts(raw, device="cuda:0", gene_clusters="louvain")
    torch.cuda.synchronize()
    out["preprocess_louvain_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    preprocess_counts(raw, device="cuda:0")
    torch.cuda.synchronize()
    out["preprocess_kmeans_s"] = time.perf_counter() - t0

    # host restatement of the step-1 fits of the first time point (a slice of its genes, scaled)
    import scipy.sparse as sp
    from threadpoolctl import threadpool_limits
    import sct_ref as ref
    lo, hi = dc.tp_off_host[0], dc.tp_off_host[1]
    B = sp.csr_matrix(dc.X[lo:hi], dtype=np.float64)
    keep, x = ref.cell_attr(B)
    g1 = r0.genes[r0.step1][:a.host_genes]
    Y = ref.dense_y(B, keep, g1)
    with threadpool_limits(a.threads):
        t0 = time.perf_counter()
        for s in range(0, g1.size, 125):
            _, mu, _ = ref.fit_poisson(Y[s:s + 125], x)
            ref.theta_ml(Y[s:s + 125], mu)
        host = time.perf_counter() - t0
    out["host_fit_s_per_tp"] = host * r0.step1.size / g1.size
    out["host_fit_s_all_tps"] = out["host_fit_s_per_tp"] * dc.T
    out["host_threads"] = a.threads
    print(json.dumps(out))


if __name__ == "__main__":
    main()
