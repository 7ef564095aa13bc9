#!/usr/bin/env python3
"""Time of the spatial-autocorrelation sums on the MI355X:

    python tools/autocorr_time.py [--tps 5] [--n 10000] [--genes 3000] [--density 0.15] [--k 6] [--perms 100] [--repeats 3]
                                  [--big 100000] [--big-genes 200] [--global-genes 200] [--skip-host] [--skip-call]

Synthetic time points: n spots on a jittered grid with the k-nearest-neighbour graph of spatial_edges, sparse counts with
`--density` of the entries stored and a third of the genes following a gradient, as a DeviceCounts with the values of
trends.lognorm_values.  Prints JSON lines:
  * {"what": "graph"}:      spatial_edges of all time points (host clock, ends in a synchronise);
  * {"what": "candidate"}:  spadot_autocorr_sums alone, the observed labeling and all permutations of all time points and genes in
                            one launch, warm, device events, the median of `--repeats` and the spread, for every workgroup size
                            and gene group the library has: how the defaults were chosen; edge terms (edges x genes x labelings)
                            per second;
  * {"what": "prologue"}:   the default configuration on the same counts with EMPTY edge lists: what a workgroup does beside the
                            edge pass (the binary searches of the segment bounds, zeroing, the scatter through the inverse
                            permutation, the reduction), device events;
  * {"what": "global"}:     the default configuration with lds_limit = 0 on the first `--global-genes` genes: every image in
                            global memory (the labelings in runs that share one scratch buffer; host clock around all of them);
  * {"what": "call"}:       spatial_autocorr as a user calls it: moments, validation, launch, download, graph moments, the host
                            statistics (host clock);
  * {"what": "big"}:        ONE time point of `--big` spots and `--big-genes` genes, whose image does not fit in LDS (host clock
                            around the runs of labelings, once warm);
  * {"what": "host"}:       the numpy restatement (tests/autocorr_ref.py) on 8 genes and 5 permutations of ONE time point, and
                            that time SCALED to all genes and labelings of all time points (`scaled_s`: not measured at full
                            size)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _timing import median, timed  # noqa: E402


def synthetic(tps, n, G, density, rng):
    """RawCounts of `tps` time points of n spots on jittered grids and G genes (float32 CSR)."""
    import scipy.sparse as sp
    from spadot_amd.utils._preprocess_utils import RawCounts
    side = int(np.ceil(np.sqrt(n)))
    xy = np.concatenate([np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:n]
                         + rng.uniform(-.3, .3, (n, 2)) for _ in range(tps)])
    blocks = []
    for g0 in range(0, G, 500):
        gc = min(500, G - g0)
        p = np.full((tps * n, gc), density, dtype=np.float32)
        p[:, ::3] *= (0.4 + 1.2 * xy[:, :1] / side).astype(np.float32)               # every third gene follows x
        hit = rng.random((tps * n, gc), dtype=np.float32) < p
        blocks.append(sp.csr_matrix(hit * rng.integers(1, 6, (tps * n, gc)).astype(np.float32)))
    X = sp.hstack(blocks, format="csr").astype(np.float32)
    return RawCounts(X, np.repeat(np.arange(tps), n), xy, np.arange(G).astype(str))


def _prepared(edges, dc, values, centre, perms):
    """The tensors and the checked descriptor of one call (as autocorr.autocorr_sums builds them)."""
    import torch
    from spadot_amd import stage_ops as ops
    src = torch.cat([s for s, _ in edges])
    dst = torch.cat([d for _, d in edges])
    eoff = np.concatenate([[0], np.cumsum([int(s.shape[0]) for s, _ in edges])])
    off = dc.tp_off_host.astype(np.int64)
    desc = np.asarray([[eoff[t], off[t + 1] - off[t], eoff[t + 1] - eoff[t], off[t], t, 0, 0] for t in range(dc.T)], dtype=np.int64)
    args = (src, dst, dc.colptr, dc.ridx, values, centre)
    checked = ops.autocorr_check(*args, desc, 0, dc.G, True, 0, perms)
    out = tuple(torch.empty((dc.T, dc.G, 1 + perms), dtype=torch.float64, device=src.device) for _ in range(2))
    return args, checked, out, torch.as_tensor(checked[0], device=src.device)


def _time_launch(prep, G, perms, repeats, threads, gs):
    from spadot_amd import stage_ops as ops
    args, checked, out, desc_dev = prep
    return timed(lambda: ops.autocorr_launch(*args, checked, 0, G, True, 0, perms, 0, None, out, None, threads, gs, desc_dev),
                 repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=3000)
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--perms", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--big", type=int, default=100000)
    ap.add_argument("--big-genes", type=int, default=200)
    ap.add_argument("--global-genes", type=int, default=200)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-call", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.autocorr import autocorr_sums, spatial_autocorr
    from spadot_amd.moran import centre_spread, columns
    from spadot_amd.neighbors import spatial_edges
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.trends import lognorm_values
    assert torch.cuda.is_available(), "autocorr_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)

    def setup(tps, n, G):
        dc = DeviceCounts(synthetic(tps, n, G, a.density, rng), dev)
        off = dc.tp_off_host
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        edges = [spatial_edges(dc.spatial[int(off[t]):int(off[t + 1])], a.k, dev) for t in range(dc.T)]
        torch.cuda.synchronize()
        graph_ms = (time.perf_counter() - t0) * 1e3
        values = lognorm_values(dc)
        centre = centre_spread(columns(dc, values))[1]
        return dc, edges, values, centre, graph_ms

    spatial_edges(rng.uniform(size=(64, 2)), a.k, dev)                               # warm
    dc, edges, values, centre, graph_ms = setup(a.tps, a.n, a.genes)
    shape = f"{a.tps} x {a.n} spots x {a.genes} genes, k = {a.k}, {a.perms} permutations"
    print(json.dumps(dict(what="graph", shape=shape, ms=round(graph_ms, 3), stored=int(dc.ridx.numel()))), flush=True)
    E = sum(int(s.shape[0]) for s, _ in edges)
    terms = E * a.genes * (a.perms + 1)

    prep = _prepared(edges, dc, values, centre, a.perms)
    for threads in (1024, 512, 256):
        for gs in (4, 2):
            rec = dict(what="candidate", shape=shape, threads=threads, gs=gs, edge_terms=terms,
                       default=(threads, gs) == (ops.AUTOCORR_THREADS, ops.AUTOCORR_GS),
                       **median(_time_launch(prep, a.genes, a.perms, a.repeats, threads, gs)))
            rec["Gterms_per_s"] = round(terms / (rec["median_ms"] * 1e-3) / 1e9, 2)
            print(json.dumps(rec), flush=True)
    del prep
    none = torch.empty(0, dtype=torch.int32, device=dev)
    prep = _prepared([(none, none)] * dc.T, dc, values, centre, a.perms)
    print(json.dumps(dict(what="prologue", shape=shape + ", no edges", threads=ops.AUTOCORR_THREADS, gs=ops.AUTOCORR_GS,
                          **median(_time_launch(prep, a.genes, a.perms, a.repeats, None, None)))), flush=True)
    del prep

    if a.global_genes > 0:
        gg = min(a.global_genes, a.genes)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        autocorr_sums(edges, dc, values, centre, a.perms, genes=(0, gg), lds_limit=0)
        ms = (time.perf_counter() - t0) * 1e3
        gt = E * gg * (a.perms + 1)
        print(json.dumps(dict(what="global", shape=f"{a.tps} x {a.n} spots x {gg} genes, {a.perms} permutations, lds_limit = 0",
                              ms=round(ms, 3), edge_terms=gt, Gterms_per_s=round(gt / (ms * 1e-3) / 1e9, 2))), flush=True)

    res = None
    if not a.skip_call:
        call = []
        for _ in range(2):
            t0 = time.perf_counter()
            res = spatial_autocorr(edges, dc, values, n_perms=a.perms, seed=0)
            call.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(what="call", shape=shape, **median(call))), flush=True)

    if not a.skip_host:
        import autocorr_ref as ref
        src, dst = (t.cpu().numpy() for t in edges[0])
        n0 = int(dc.tp_off_host[1])
        colptr, ridx, vals = dc.colptr.cpu().numpy(), dc.ridx.cpu().numpy(), values.cpu().numpy()
        V = np.zeros((n0, 8), dtype=np.float32)
        for g in range(8):
            seg = slice(int(colptr[g]), int(colptr[g + 1]))
            keep = ridx[seg] < n0
            V[ridx[seg][keep], g] = vals[seg][keep]
        c = centre[0, :8].cpu().numpy()
        t0 = time.perf_counter()
        wN, wD, wA = ref.all_sums_genes(src, dst, V, c, 5, 0, 0)
        s = time.perf_counter() - t0
        rec = dict(what="host", shape=f"1 x {a.n} spots x 8 genes, 5 permutations", numpy_s=round(s, 3),
                   scaled_s=round(s / (8 * 6) * a.genes * (a.perms + 1) * a.tps, 1),
                   scaled_to=f"{a.tps} x {a.genes} genes x {a.perms + 1} labelings, not measured")
        if res is not None:
            err = max(float(np.abs(res[0].N[:8, :6] - wN).max()), float(np.abs(res[0].D[:8, :6] - wD).max()))
            rec["within_bound_of_device"] = bool(np.all(np.abs(res[0].N[:8, :6] - wN) <= 4 * (len(src) + 2) * 2.0 ** -53 * wA))
            rec["largest_difference"] = err
        print(json.dumps(rec), flush=True)

    if a.big > 0:
        del dc, edges, values, centre, res
        torch.cuda.empty_cache()
        dc, edges, values, centre, graph_ms = setup(1, a.big, a.big_genes)
        autocorr_sums(edges, dc, values, centre, 1, genes=(0, min(4, a.big_genes)))  # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        autocorr_sums(edges, dc, values, centre, a.perms)
        ms = (time.perf_counter() - t0) * 1e3
        bt = int(edges[0][0].shape[0]) * a.big_genes * (a.perms + 1)
        print(json.dumps(dict(what="big", shape=f"1 x {a.big} spots x {a.big_genes} genes, k = {a.k}, {a.perms} permutations",
                              graph_ms=round(graph_ms, 3), ms=round(ms, 3), edge_terms=bt,
                              Gterms_per_s=round(bt / (ms * 1e-3) / 1e9, 2))), flush=True)


if __name__ == "__main__":
    main()
