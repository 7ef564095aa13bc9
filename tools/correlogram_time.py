#!/usr/bin/env python3
"""Time of the correlogram sums on the MI355X:

    python tools/correlogram_time.py [--tps 5] [--n 10000] [--genes 100] [--bins 12] [--n_perms 0,99] [--cs 2] [--repeats 5]
                                     [--skip-call]

Synthetic time points: n spots on a jittered grid (tools/cooccur_time.py), `--genes` columns of random centred values, the stage's
default bands.  Prints JSON lines:
  * {"what": "launch", "n_perms": P, "cull": ..}:  stage_ops.corr_launch on checked arrays with the scratch buffer, the
                                     descriptor and the thresholds already on the device: the zeroing of the integers, the boxes,
                                     the band sums and the reduction of the partials, all time points in one call, warm, device
                                     events, the median of `--repeats` and the spread; for every P of `--n_perms`, with and
                                     without tile culling; the culled share of the (query block, tile) pairs and the pairs of
                                     spots per second;
  * {"what": "call"}:                correlogram as a user calls it on dense columns: moments, image, Morton order, validation,
                                     launch, download, the host statistics (host clock), P = 0."""
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
from cooccur_time import synthetic  # noqa: E402


def _prepared(sets, X, radii, P, cs, dev):
    """The tensors and the checked arrays of one call (as correlogram.corr_sums builds them)."""
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.correlogram import morton_order
    sizes = np.asarray([xy.shape[0] for xy in sets], dtype=np.int64)
    ng = X[0].shape[1]
    zoff, zrows = ops.cross_layout(sizes)
    boff, blocks = ops.corr_layout(sizes)
    Z = torch.zeros((zrows, ops.cross_padded(ng)), dtype=torch.float64, device=dev)
    orders = [morton_order(xy) for xy in sets]
    for t, x in enumerate(X):
        Z[int(zoff[t]):int(zoff[t]) + int(sizes[t]), :ng] = torch.as_tensor(x, device=dev)
    xy = torch.as_tensor(np.ascontiguousarray(np.concatenate([p[o] for p, o in zip(sets, orders)])), device=dev)
    order = torch.as_tensor(np.concatenate(orders), device=dev)
    desc = np.zeros((len(sets), ops.CORR_DESC), dtype=np.int64)
    desc[:, 0], desc[:, 1], desc[:, 2] = np.concatenate([[0], np.cumsum(sizes)])[:-1], sizes, [r.shape[0] for r in radii]
    desc[:, 3], desc[:, 4], desc[:, 5] = np.arange(len(sets)), zoff, boff
    checked = ops.corr_check(xy, order, Z, desc, [r * r for r in radii], ng, True, 0, P, cs)
    B = checked[2]
    scratch = torch.empty(ops.corr_scratch_doubles(blocks, ng, 1 + P, B), dtype=torch.float64, device=dev)
    out = (torch.empty((len(sets), B), dtype=torch.int64, device=dev), torch.empty((len(sets), B), dtype=torch.int64, device=dev),
           torch.empty((len(sets), ng, 1 + P, B), dtype=torch.float64, device=dev),
           torch.empty((len(sets), ng, 1 + P, B), dtype=torch.float64, device=dev))
    skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    fixed = dict(out=out, scratch=scratch, skipped=skipped, desc_dev=torch.as_tensor(checked[0], device=dev),
                 r2_dev=torch.as_tensor(checked[1], device=dev))
    return (xy, order, Z, checked, ng), fixed, blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=100)
    ap.add_argument("--bins", type=int, default=12)
    ap.add_argument("--n_perms", type=str, default="0,99")
    ap.add_argument("--cs", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-call", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.correlogram import correlogram, default_bands
    assert torch.cuda.is_available(), "correlogram_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    sets = [synthetic(a.n, 7, rng)[0] for _ in range(a.tps)]
    X = [rng.standard_normal((a.n, a.genes)) for _ in range(a.tps)]
    X = [x - x.mean(axis=0) for x in X]
    radii = [default_bands(xy, a.bins) for xy in sets]
    pairs = a.tps * a.n * (a.n - 1)

    for P in [int(v) for v in a.n_perms.split(",")]:
        args, fixed, blocks = _prepared(sets, X, radii, P, a.cs, dev)
        shape = f"{a.tps} x {a.n} spots, {a.genes} genes, B = {a.bins}, P = {P}, cs = {a.cs}"
        for cull in (True, False):
            rec = dict(what="launch", n_perms=P, cull=cull, shape=shape,
                       **median(timed(lambda: ops.corr_launch(*args, 0, cull, a.cs, **fixed), a.repeats)))
            tiles = sum((-(-xy.shape[0] // 256)) ** 2 for xy in sets)
            rec["culled_share"] = round(int(fixed["skipped"].item()) / tiles, 3)
            rec["Gpairs_per_s"] = round(pairs * (1 + P) * -(-a.genes // a.cs) / (rec["median_ms"] * 1e-3) / 1e9, 2)
            print(json.dumps(rec), flush=True)
        del args, fixed
        torch.cuda.empty_cache()

    if not a.skip_call:
        coords = [torch.as_tensor(xy, device=dev) for xy in sets]
        dense = [torch.as_tensor(x.astype(np.float32), device=dev) for x in X]
        call = []
        for _ in range(3):
            t0 = time.perf_counter()
            correlogram(coords, dense, radii=radii, n_perms=0)
            call.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(what="call", shape=f"{a.tps} x {a.n} spots, {a.genes} genes, B = {a.bins}, P = 0", **median(call))),
              flush=True)


if __name__ == "__main__":
    main()
