#!/usr/bin/env python3
"""Time of the territories kernel on the MI355X:

    python tools/territories_time.py [--tps 5] [--n 10000] [--domains 7] [--k 6] [--perms 1000] [--repeats 3] [--flip 0.03]
                                     [--host-perms 20] [--skip-host]

Synthetic time points: n spots on a jittered grid cut into `--domains` stripes with a share `--flip` of the labels flipped, the
k-nearest-neighbour graph of spatial_edges.  Prints JSON lines:
  * {"what": "graph"}:    spatial_edges of all time points (host clock, ends in a synchronise);
  * {"what": "launch"}:   stage_ops.territory_launch alone (the descriptor upload, the output tensors and the one kernel): the
                          observed labelings and all relabelings of all time points in one launch, warm, device events, the median of `--repeats` and the spread; the rounds seen per item
                          (maximum and median) and (labeling, edge) pairs per second;
  * {"what": "scratch"}:  the same launch with lds_limit = 0: parents, sizes and labels in the global scratch slabs;
  * {"what": "call"}:     territories() as a user calls it: validation, launch, download, the host statistics (host clock);
  * {"what": "host"}:     the scipy restatement (tests/territories_ref.py) on `--host-perms` relabelings of ONE time point, and
                          that time SCALED to all relabelings of all time points (`scaled_s`: not measured at full size)."""
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


def synthetic(n, K, flip, rng):
    side = int(np.ceil(np.sqrt(n)))
    xy = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:n] + rng.uniform(-.3, .3, (n, 2))
    lab = np.minimum((np.arange(n) % side) * K // side, K - 1).astype(np.int64)
    who = rng.choice(n, int(round(flip * n)), replace=False)
    lab[who] = (lab[who] + rng.integers(1, max(K, 2), who.shape[0])) % K
    return xy, lab


def _prepared(edges, labs, K, perms, seed=0):
    """The tensors and the checked descriptor of one territories call (as territories._run builds them)."""
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
            desc.append([eoff[g], loff[g + 1] - loff[g], eoff[g + 1] - eoff[g], K, loff[g], L, p0, g, item, seed, 0, 0, -1, 0])
            item += L
    return src, dst, labels, ops.territory_check(src, dst, labels, np.asarray(desc, dtype=np.int64), K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--domains", type=int, default=7)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--flip", type=float, default=0.03)
    ap.add_argument("--host-perms", type=int, default=20)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.neighbors import spatial_edges
    from spadot_amd.territories import territories
    assert torch.cuda.is_available(), "territories_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    sets = [synthetic(a.n, a.domains, a.flip, rng) for _ in range(a.tps)]
    shape = f"{a.tps} x {a.n} spots, K = {a.domains}, k = {a.k}, {a.perms} relabelings"

    spatial_edges(sets[0][0], a.k, dev)                                        # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    edges = [spatial_edges(xy, a.k, dev) for xy, _ in sets]
    torch.cuda.synchronize()
    print(json.dumps(dict(what="graph", shape=shape, ms=round((time.perf_counter() - t0) * 1e3, 3))), flush=True)
    labs = [torch.as_tensor(lab, device=dev) for _, lab in sets]
    pairs = sum(int(s.shape[0]) for s, _ in edges) * (a.perms + 1)

    src, dst, labels, desc = _prepared(edges, labs, a.domains, a.perms)
    keep = {}
    for what, limit in (("launch", None), ("scratch", 0)):
        ms = timed(lambda: keep.__setitem__(what, ops.territory_launch(src, dst, labels, desc, a.domains, limit)), a.repeats)
        out, _, _, status = keep[what]
        status = status.cpu().numpy()
        rec = dict(what=what, shape=shape, labeling_edges=pairs, **median(ms), status_max=int(status[:, 0].max()),
                   rounds_max=int(status[:, 1].max()), rounds_median=float(np.median(status[:, 1])),
                   rounds_observed=status[np.cumsum([0] + [a.perms + 1] * (a.tps - 1)), 1].tolist())
        rec["Gedges_per_s"] = round(pairs / (rec["median_ms"] * 1e-3) / 1e9, 2)
        print(json.dumps(rec), flush=True)
    same = bool(torch.equal(keep["launch"][0], keep["scratch"][0]))
    print(json.dumps(dict(what="paths", lds_equals_scratch=same)), flush=True)

    call = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = territories(edges, labs, n_perms=a.perms, seed=0, n_clusters=[a.domains] * a.tps)
        call.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what="call", shape=shape, **median(call), observed_territories=[int(r.counts[:, 0].sum()) for r in res],
                          relabeled_territories_mean=round(float(res[0].perm_counts[:, :, 0].sum(axis=1).mean()), 1))),
          flush=True)

    if not a.skip_host:
        import territories_ref as ref
        s, d = (t.cpu().numpy() for t in edges[0])
        lab = sets[0][1]
        t0 = time.perf_counter()
        want = ref.perm_integers(s, d, lab, a.domains, a.host_perms, 0, 0)
        sec = time.perf_counter() - t0
        same = bool(np.array_equal(want, res[0].perm_counts[:a.host_perms]))
        print(json.dumps(dict(what="host", shape=f"1 x {a.n} spots, {a.host_perms} relabelings", scipy_s=round(sec, 3),
                              scaled_s=round(sec / a.host_perms * a.perms * a.tps, 2),
                              scaled_to=f"{a.tps} x {a.perms} relabelings, not measured", equal_to_device=same)), flush=True)


if __name__ == "__main__":
    main()
