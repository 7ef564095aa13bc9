#!/usr/bin/env python3
"""Time of the sepal stage on the MI355X:

    python tools/sepal_time.py [--tps 5] [--n 10000] [--genes 100] [--steps 1000] [--repeats 3] [--skip-call]

Synthetic counts: synthetic.make_raw_counts with `--tps` time points of `--n` spots and `--genes` genes, of which 40 follow a
planted pattern; the log-normalised values and the 6-nearest-neighbour graphs of the stage.  Prints JSON lines:
  * {"what": "steps", "path": "lds" | "global"}:  one launch of `--steps` steps without the stop rule over the genes of the FIRST time
                                     point alone (one workgroup per gene, all resident at once), state already on the device,
                                     warm, device events, the median of `--repeats` and the spread; the steps per second of a
                                     workgroup and the spot updates per second of the launch; with the image in LDS and, under
                                     lds_limit = 0, in global memory;
  * {"what": "call"}:                sepal as a user calls it on all time points, with the stop rule and the defaults: graph,
                                     checks, launches, downloads (host clock, after one warm call); the iterations, the share of
                                     the items on each path and the (time point, gene) pairs that reached n_iter."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import median, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=100)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-call", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.neighbors import spatial_edges
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.sepal import _prepare, sepal
    from spadot_amd.synthetic import make_raw_counts
    from spadot_amd.trends import lognorm_values
    assert torch.cuda.is_available(), "sepal_time measures on the MI355X"
    dev = torch.device("cuda:0")
    raw = make_raw_counts((a.n,) * a.tps, n_genes=a.genes, n_modules=4, genes_per_module=min(10, a.genes // 8), n_rare=0, seed=1993)
    dc = DeviceCounts(raw, dev)
    values = lognorm_values(dc)
    off = dc.tp_off_host
    edges = [spatial_edges(dc.spatial[int(off[t]):int(off[t + 1])], 6, dev) for t in range(dc.T)]
    shape = f"{a.tps} x {a.n} spots, {a.genes} genes"

    first = DeviceCounts(make_raw_counts((a.n,), n_genes=a.genes, n_modules=4, genes_per_module=min(10, a.genes // 8), n_rare=0,
                                         seed=1993), dev)
    cols, _, sel, graph, gsel = _prepare([spatial_edges(first.spatial, 6, dev)], first, None, lognorm_values(first))
    one = graph.desc
    for path, lds_limit in (("lds", None), ("global", 0)):
        checked = ops.sepal_check(graph.rowptr, graph.col, cols.colptr, cols.ridx, cols.values, gsel, one, 0.1, 0.0, a.steps, a.steps)
        state = ops.sepal_state(one, sel.size, dev, lds_limit)
        fixed = dict(desc_dev=torch.as_tensor(checked[0], device=dev), rate_dev=torch.as_tensor(checked[5], device=dev))
        go = lambda: ops.sepal_launch(graph.rowptr, graph.col, cols.colptr, cols.ridx, cols.values, gsel, checked, state,  # noqa: E731
                                      True, a.steps, a.steps, 0.0, False, lds_limit, **fixed)
        rec = dict(what="steps", path=path, shape=f"1 x {a.n} spots, {a.genes} genes, {a.steps} steps",
                   in_lds=bool(ops.sepal_lds_bytes(a.n) <= ops.SEPAL_LDS_BYTES and lds_limit is None), **median(timed(go, a.repeats)))
        rec["steps_per_s_per_workgroup"] = round(a.steps / (rec["median_ms"] * 1e-3))
        rec["Gspot_updates_per_s"] = round(a.steps * a.n * sel.size / (rec["median_ms"] * 1e-3) / 1e9, 2)
        print(json.dumps(rec), flush=True)

    if not a.skip_call:
        call, res = [], None
        for i in range(1 + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = sepal(edges, dc, values=values)
            call.append((time.perf_counter() - t0) * 1e3)
        it = np.concatenate([r.iterations[~r.degenerate] for r in res])
        in_lds = sum(r.genes.size for r in res if ops.sepal_lds_bytes(r.n) <= ops.SEPAL_LDS_BYTES)
        print(json.dumps(dict(what="call", shape=shape, **median(call[1:]), iterations_min=int(it.min()),
                              iterations_median=int(np.median(it)), iterations_max=int(it.max()),
                              share_in_lds=round(in_lds / sum(r.genes.size for r in res), 3),
                              reached_n_iter=int(sum((~r.converged & ~r.degenerate).sum() for r in res)))), flush=True)


if __name__ == "__main__":
    main()
