#!/usr/bin/env python3
"""Time of the neighbourhood-enrichment counts on the MI355X:

    python tools/neighbors_time.py [--tps 5] [--n 10000] [--domains 12] [--k 6] [--perms 1000] [--repeats 7] [--big 100000]
                                   [--skip-host]

Synthetic time points: n spots on a jittered grid, `--domains` planted Voronoi domains, the k-nearest-neighbour graph of
spatial_edges.  Prints JSON lines:
  * {"what": "graph"}:    spatial_edges of all time points (host clock, ends in a synchronise);
  * {"what": "launch"}:   spadot_nhood_counts alone, the observed labelings and all permutations of all time points in one
                          launch, warm, device events, the median of `--repeats` and the spread; label pairs counted per second;
  * {"what": "global"}:   the same launch with lds_limit = 0: every label read from global memory, pi evaluated per edge end;
  * {"what": "call"}:     nhood_enrichment as a user calls it: validation, launch, download, the host statistics (host clock);
  * {"what": "big"}:      ONE time point of `--big` spots with `--perms` permutations, launch alone (device events), once warm;
  * {"what": "host"}:     the numpy bincount restatement (tests/nhood_ref.py) on 50 permutations of ONE time point, and that time
                          SCALED to all permutations of all time points (`scaled_s`: not measured at full size)."""
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


def synthetic(n, K, rng):
    side = int(np.ceil(np.sqrt(n)))
    xy = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:n] + rng.uniform(-.3, .3, (n, 2))
    cen = rng.uniform(0, side, (K, 2))
    lab = np.empty(n, dtype=np.int64)
    for lo in range(0, n, 8192):
        lab[lo:lo + 8192] = np.argmin(((xy[lo:lo + 8192, None] - cen[None]) ** 2).sum(-1), 1)
    return xy, lab


def _prepared(edges, labs, K, perms, seed=0):
    """The tensors and the checked descriptor of one enrichment call (as neighbors._run builds them)."""
    import torch
    from spadot_amd import stage_ops as ops
    src = torch.cat([s for s, _ in edges])
    dst = torch.cat([d for _, d in edges])
    labels = torch.cat([l.to(torch.uint8) for l in labs])
    eoff = np.concatenate([[0], np.cumsum([int(s.shape[0]) for s, _ in edges])])
    loff = np.concatenate([[0], np.cumsum([int(l.shape[0]) for l in labs])])
    desc, item = [], 0
    for g in range(len(edges)):
        for L, p0 in ((1, -1), (perms, 0)):
            desc.append([eoff[g], loff[g + 1] - loff[g], eoff[g + 1] - eoff[g], K, loff[g], L, p0, g, item, seed, 0, 0])
            item += L
    desc = ops.nhood_check(src, dst, labels, np.asarray(desc, dtype=np.int64), K)
    out = torch.empty((item, K, K), dtype=torch.int32, device=src.device)
    return src, dst, labels, desc, torch.as_tensor(desc, device=src.device), out


def _time_launch(prep, K, repeats, lds_limit=None):
    from spadot_amd import stage_ops as ops
    src, dst, labels, desc, desc_dev, out = prep
    return timed(lambda: ops.nhood_launch(src, dst, labels, desc, K, lds_limit, out, desc_dev), repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--domains", type=int, default=12)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--big", type=int, default=100000)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd.neighbors import nhood_enrichment, spatial_edges
    assert torch.cuda.is_available(), "neighbors_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    sets = [synthetic(a.n, a.domains, rng) for _ in range(a.tps)]
    shape = f"{a.tps} x {a.n} spots, K = {a.domains}, k = {a.k}, {a.perms} permutations"

    spatial_edges(sets[0][0], a.k, dev)                                        # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    edges = [spatial_edges(xy, a.k, dev) for xy, _ in sets]
    torch.cuda.synchronize()
    print(json.dumps(dict(what="graph", shape=shape, ms=round((time.perf_counter() - t0) * 1e3, 3))), flush=True)
    labs = [torch.as_tensor(lab, device=dev) for _, lab in sets]
    pairs = sum(int(s.shape[0]) for s, _ in edges) * (a.perms + 1)

    prep = _prepared(edges, labs, a.domains, a.perms)
    for what, limit in (("launch", None), ("global", 0)):
        rec = dict(what=what, shape=shape, label_pairs=pairs, **median(_time_launch(prep, a.domains, a.repeats, limit)))
        rec["Gpairs_per_s"] = round(pairs / (rec["median_ms"] * 1e-3) / 1e9, 2)
        print(json.dumps(rec), flush=True)

    call = []
    for _ in range(max(3, a.repeats // 2)):
        t0 = time.perf_counter()
        res = nhood_enrichment(edges, labs, n_perms=a.perms, seed=0, n_clusters=[a.domains] * a.tps)
        call.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what="call", shape=shape, **median(call))), flush=True)

    if a.big > 0:
        xy, lab = synthetic(a.big, a.domains, rng)
        t0 = time.perf_counter()
        e = spatial_edges(xy, a.k, dev)
        torch.cuda.synchronize()
        graph_ms = (time.perf_counter() - t0) * 1e3
        big = _prepared([e], [torch.as_tensor(lab, device=dev)], a.domains, a.perms)
        ms = _time_launch(big, a.domains, 1)
        bp = int(e[0].shape[0]) * (a.perms + 1)
        print(json.dumps(dict(what="big", shape=f"1 x {a.big} spots, K = {a.domains}, k = {a.k}, {a.perms} permutations",
                              graph_ms=round(graph_ms, 3), launch_ms=round(ms[0], 3), label_pairs=bp,
                              Gpairs_per_s=round(bp / (ms[0] * 1e-3) / 1e9, 2))), flush=True)

    if not a.skip_host:
        import nhood_ref as ref
        src, dst = (t.cpu().numpy() for t in edges[0])
        lab = sets[0][1]
        t0 = time.perf_counter()
        want = ref.perm_counts(src, dst, lab, a.domains, 50, 0, 0)
        s = time.perf_counter() - t0
        same = bool(np.array_equal(want, res[0].perm_counts[:50]))
        print(json.dumps(dict(what="host", shape=f"1 x {a.n} spots, 50 permutations", numpy_s=round(s, 3),
                              scaled_s=round(s / 50 * a.perms * a.tps, 2),
                              scaled_to=f"{a.tps} x {a.perms} permutations, not measured", equal_to_device=same)), flush=True)


if __name__ == "__main__":
    main()
