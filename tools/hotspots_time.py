#!/usr/bin/env python3
"""Time of the local Moran's I kernel on the MI355X:

    python tools/hotspots_time.py [--tps 5] [--n 10000] [--genes 100] [--density 0.15] [--k 6] [--perms 999] [--repeats 3]
                                  [--skip-call] [--quick]

Synthetic time points (tools/autocorr_time.py: n spots on a jittered grid with the k-nearest-neighbour graph of spatial_edges,
sparse counts with `--density` of the entries stored) as a DeviceCounts with the values of trends.lognorm_values; the first
`--genes` genes are the selection.  Prints JSON lines:
  * {"what": "candidate"}:  spadot_local_lag alone, all permutations of all time points and selected genes in one launch into
                            zeroed outputs, warm, device events, the median of `--repeats` and the spread, for the workgroup
                            sizes, gene groups and permutation chunks tried (`--quick`: the default and its neighbours only):
                            how the defaults were chosen; neighbour terms (edges x genes x (1 + permutations)) per second;
  * {"what": "yardstick"}:  spadot_autocorr_sums at its defaults on the same genes and labelings (the observed one and the
                            permutations): the same scatter and edge stream per (gene, labeling) without the per-spot state; and
                            the ratio of the default candidate to it;
  * {"what": "global"}:     the default configuration with lds_limit = 0: every image in global memory;
  * {"what": "call"}:       local_moran as a user calls it: moments, the CSR, validation, launch, download, the host statistics
                            (host clock)."""
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
from autocorr_time import _prepared, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=100)
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--perms", type=int, default=999)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.hotspots import local_moran
    from spadot_amd.moran import centre_spread, columns, edge_csr
    from spadot_amd.neighbors import spatial_edges
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.trends import lognorm_values
    assert torch.cuda.is_available(), "hotspots_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    spatial_edges(rng.uniform(size=(64, 2)), a.k, dev)                               # warm
    dc = DeviceCounts(synthetic(a.tps, a.n, a.genes, a.density, rng), dev)
    off = dc.tp_off_host.astype(np.int64)
    edges = [spatial_edges(dc.spatial[int(off[t]):int(off[t + 1])], a.k, dev) for t in range(dc.T)]
    values = lognorm_values(dc)
    centre = centre_spread(columns(dc, values))[1]
    shape = f"{a.tps} x {a.n} spots x {a.genes} genes, k = {a.k}, {a.perms} permutations"
    E = sum(int(s.shape[0]) for s, _ in edges)
    terms = E * a.genes * (a.perms + 1)

    rowptr, col, desc = edge_csr(edges, np.diff(off), dc.device)
    desc[:, 3] = off[:-1]
    gsel = torch.arange(a.genes, dtype=torch.int32, device=dev)
    args = (rowptr, col, dc.colptr, dc.ridx, values, centre, gsel)
    checked = ops.local_check(*args, desc, 0, a.perms)
    desc_dev = torch.as_tensor(checked[0], device=dev)
    out = tuple(torch.zeros((a.genes, dc.n), dtype=dt, device=dev) for dt in (torch.float64, torch.int32, torch.int32))

    def launch(threads, gs, chunk, lds_limit=None):
        scratch = torch.empty(ops.local_scratch_bytes(checked[0], a.genes, a.perms, lds_limit, gs, chunk), dtype=torch.uint8,
                              device=dev)

        def go():
            out[1].zero_()
            out[2].zero_()
            ops.local_launch(*args, checked, 0, a.perms, 0, lds_limit, out, scratch, threads, gs, chunk, desc_dev)
        return timed(go, a.repeats)

    default = (ops.LOCAL_THREADS, ops.LOCAL_GS, ops.LOCAL_CHUNK)
    tried = [default] + [c for c in ((1024, 2, 128), (512, 4, 128), (512, 2, 128), (256, 2, 128), (1024, 4, 32), (1024, 4, 64),
                                     (1024, 4, 256), (1024, 4, 1024), (1024, 2, 64)) if c != default]
    if a.quick:
        tried = tried[:4]
    base = None
    for threads, gs, chunk in tried:
        rec = dict(what="candidate", shape=shape, threads=threads, gs=gs, perm_chunk=chunk, neighbour_terms=terms,
                   default=(threads, gs, chunk) == default, lds_bytes=ops.local_lds_bytes(a.n, gs),
                   **median(launch(threads, gs, chunk)))
        rec["Gterms_per_s"] = round(terms / (rec["median_ms"] * 1e-3) / 1e9, 2)
        base = rec["median_ms"] if rec["default"] else base
        print(json.dumps(rec), flush=True)
    ref_ge = out[1].clone()

    prep = _prepared(edges, dc, values, centre, a.perms)
    a_args, a_checked, a_out, a_desc = prep
    ms = timed(lambda: ops.autocorr_launch(*a_args, a_checked, 0, a.genes, True, 0, a.perms, 0, None, a_out, None, None, None,
                                           a_desc), a.repeats)
    rec = dict(what="yardstick", shape=shape, entry="spadot_autocorr_sums", threads=ops.AUTOCORR_THREADS, gs=ops.AUTOCORR_GS,
               **median(ms))
    rec["local_lag_over_autocorr_sums"] = round(base / rec["median_ms"], 2)
    print(json.dumps(rec), flush=True)
    del prep, a_out

    rec = dict(what="global", shape=shape + ", lds_limit = 0", **median(launch(None, None, None, 0)))
    rec["same_integers_as_lds"] = bool(torch.equal(out[1], ref_ge))
    print(json.dumps(rec), flush=True)

    if not a.skip_call:
        call = []
        for _ in range(2):
            t0 = time.perf_counter()
            local_moran(edges, dc, np.arange(a.genes), values, n_perms=a.perms, seed=0)
            call.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(what="call", shape=shape, **median(call))), flush=True)


if __name__ == "__main__":
    main()
