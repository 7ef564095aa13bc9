#!/usr/bin/env python3
"""Time of the cross-Moran kernels on the MI355X:

    python tools/modules_time.py [--tps 5] [--n 10000] [--genes 512] [--density 0.15] [--k 6] [--perms 100] [--repeats 3]
                                 [--slice-n 2000] [--slice-genes 128] [--slice-perms 3] [--skip-call]

Synthetic time points (tools/autocorr_time.py: n spots on a jittered grid with the k-nearest-neighbour graph of spatial_edges,
sparse counts with `--density` of the entries stored) as a DeviceCounts with the values of trends.lognorm_values; the first
`--genes` genes are the selection.  Prints JSON lines:
  * {"what": "images"}:     spadot_cross_dense alone (Z from the CSC, Y from the CSR), warm, device events, the median of
                            `--repeats`;
  * {"what": "candidate"}:  spadot_cross_sums alone, the observed labeling and all permutations of all time points in the launches
                            that modules.cross_sums would make (SCRATCH_BYTES of sums each, one output buffer), warm, device
                            events around the whole run, the median of `--repeats` and the spread; fp64 multiply-adds (spots x
                            genes^2 x labelings), TFLOP/s (two per multiply-add) and its share of `--peak-tflops` if given;
  * {"what": "yardstick"}:  the numpy restatement (the gathered image transposed times the lag, fp64 BLAS on this host's cores)
                            on a slice of one time point -- `--slice-n` spots, `--slice-genes` genes, `--slice-perms` labelings
                            -- scaled up by the ratio of the multiply-adds, and the ratio of it to the candidate;
  * {"what": "call"}:       cross_moran as a user calls it: moments, the CSR, validation, the images, the launches, the fold of
                            every run on the device, download, the host statistics (host clock)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import median, timed  # noqa: E402
from autocorr_time import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=512)
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--perms", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slice-n", type=int, default=2000)
    ap.add_argument("--slice-genes", type=int, default=128)
    ap.add_argument("--slice-perms", type=int, default=3)
    ap.add_argument("--peak-tflops", type=float, default=None)
    ap.add_argument("--skip-call", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd import modules
    from spadot_amd import stage_ops as ops
    from spadot_amd.moran import centre_spread, columns, edge_csr
    from spadot_amd.neighbors import spatial_edges
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.trends import lognorm_values
    from spadot_amd.utils._stage_utils import labeling_runs
    assert torch.cuda.is_available(), "modules_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    spatial_edges(rng.uniform(size=(64, 2)), a.k, dev)                               # warm
    dc = DeviceCounts(synthetic(a.tps, a.n, a.genes, a.density, rng), dev)
    off = dc.tp_off_host.astype(np.int64)
    edges = [spatial_edges(dc.spatial[int(off[t]):int(off[t + 1])], a.k, dev) for t in range(dc.T)]
    values = lognorm_values(dc)
    centre = centre_spread(columns(dc, values))[1]
    shape = f"{a.tps} x {a.n} spots x {a.genes} genes, k = {a.k}, {a.perms} permutations"
    L = a.perms + 1
    fmas = int(dc.n) * a.genes * a.genes * L

    rowptr, col, d8 = edge_csr(edges, np.diff(off), dc.device)
    desc = np.zeros((dc.T, ops.CROSS_DESC), dtype=np.int64)
    desc[:, :8] = d8
    desc[:, 3] = off[:-1]
    desc[:, 8], zrows = ops.cross_layout(np.diff(off))
    gsel = torch.arange(a.genes, dtype=torch.int32, device=dev)
    args = (rowptr, col, dc.colptr, dc.ridx, values, centre, gsel)
    checked = ops.cross_dense_check(*args, desc)
    desc_dev = torch.as_tensor(checked[0], device=dev)
    Z, Y = ops.cross_dense_launch(*args, checked, desc_dev=desc_dev)
    ms = timed(lambda: ops.cross_dense_launch(*args, checked, out=(Z, Y), desc_dev=desc_dev), a.repeats)
    print(json.dumps(dict(what="images", shape=shape, image_bytes=2 * zrows * ops.cross_padded(a.genes) * 8, **median(ms))), flush=True)

    runs = labeling_runs(a.perms, True, 0, dc.T * a.genes * a.genes * 8, modules.SCRATCH_BYTES)
    most = max(int(obs) + npm for obs, _, npm in runs)
    buf = torch.empty(dc.T * most * a.genes * a.genes, dtype=torch.float64, device=dev)
    sums = ops.cross_check(Z, Y, checked[0], a.genes, True, 0, a.perms)

    def go():
        for obs, p0, npm in runs:
            ops.cross_launch(Z, Y, sums, a.genes, obs, p0, npm, 0, buf[:dc.T * (int(obs) + npm) * a.genes * a.genes], desc_dev)

    rec = dict(what="candidate", shape=shape, launches=len(runs), workgroups=dc.T * L * (-(-a.genes // ops.CROSS_TILE)) ** 2,
               fp64_multiply_adds=fmas, **median(timed(go, a.repeats)))
    rec["tflops"] = round(2 * fmas / (rec["median_ms"] * 1e-3) / 1e12, 2)
    if a.peak_tflops:
        rec["share_of_peak"] = round(rec["tflops"] / a.peak_tflops, 3)
    print(json.dumps(rec), flush=True)
    base = rec["median_ms"]

    sn, sg, sp = min(a.slice_n, a.n), min(a.slice_genes, a.genes), a.slice_perms
    Zs = Z[:sn, :sg].cpu().numpy().copy()
    Ys = Y[:sn, :sg].cpu().numpy().copy()
    maps = [rng.permutation(sn) for _ in range(sp)]
    (Zs[maps[0]].T @ Ys).sum()                                                       # warm
    t0 = time.perf_counter()
    for m in maps:
        (Zs[m].T @ Ys).sum()
    host_ms = (time.perf_counter() - t0) * 1e3
    scaled = host_ms * fmas / (sn * sg * sg * sp)
    print(json.dumps(dict(what="yardstick", shape=f"numpy on {sn} spots x {sg} genes x {sp} labelings, scaled to {shape}",
                          slice_ms=round(host_ms, 3), scaled_ms=round(scaled, 1), numpy_over_cross_sums=round(scaled / base, 1))),
          flush=True)
    del buf

    if not a.skip_call:
        call = []
        for _ in range(2):
            t0 = time.perf_counter()
            modules.cross_moran(edges, dc, np.arange(a.genes), values, n_perms=a.perms, seed=0)
            call.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(what="call", shape=shape, **median(call))), flush=True)


if __name__ == "__main__":
    main()
