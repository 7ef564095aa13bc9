#!/usr/bin/env python3
"""Time of the hops kernel on the MI355X:

    python tools/centrality_time.py [--tps 5] [--n 10000] [--domains 7] [--k 6] [--perms 200,1000] [--repeats 3] [--flip 0.03]
                                    [--host-spots 200] [--skip-host]

Synthetic time points: n spots on a jittered grid cut into `--domains` stripes with a share `--flip` of the labels flipped, the
k-nearest-neighbour graph of spatial_edges.  Prints JSON lines:
  * {"what": "graph"}:    spatial_edges of all time points (host clock, ends in a synchronise);
  * {"what": "labels"}:   stage_ops.hop_launch alone (the descriptor upload, the output tensors and the one kernel) for the
                          label items: the observed labelings and P relabelings of all time points in one launch, once per
                          P of `--perms`, on the LDS path and (path = "scratch") with lds_limit = 0; warm, device events, the
                          median of `--repeats` and the spread; the rounds per item (observed, and maximum and median of all);
  * {"what": "sources"}:  the same for the source items of all time points (tps x ceil(n / 32) items), on both paths;
  * {"what": "paths"}:    whether the two paths gave the same integers;
  * {"what": "call"}:     centrality() as a user calls it, with the first P and without / with spots (host clock);
  * {"what": "host"}:     on the same host, for ONE time point: scipy's all-pairs shortest_path (tests/hops_ref.py) and
                          networkx's closeness_centrality of `--host-spots` spots, that time SCALED to all
                          spots (`networkx_scaled_s`: not measured at full size), and whether both equal the device's numbers."""
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
from territories_time import synthetic  # noqa: E402


def _prepared(edges, labs, K, perms, sources):
    """The tensors and the checked descriptor of one call (as centrality._run builds them): the label items (perms >= 0) or the
    source items."""
    import torch
    from spadot_amd import stage_ops as ops
    src = torch.cat([s for s, _ in edges])
    dst = torch.cat([d for _, d in edges])
    labels = torch.cat([l.to(torch.uint8) for l in labs])
    eoff = np.concatenate([[0], np.cumsum([int(s.shape[0]) for s, _ in edges])])
    loff = np.concatenate([[0], np.cumsum([int(l.shape[0]) for l in labs])])
    desc, item = [], 0
    for g in range(len(edges)):
        n = int(loff[g + 1] - loff[g])
        for L, p0 in (((n + 31) // 32, -1),) if sources else ((1, -1), (perms, 0))[:2 if perms else 1]:
            desc.append([eoff[g], n, eoff[g + 1] - eoff[g], K, loff[g], L, p0, g, item, 0, 0, 0, -1, 0, int(sources)])
            item += L
    K_max = ops.HOP_SETS if sources else K
    return src, dst, labels, ops.hop_check(src, dst, labels, np.asarray(desc, dtype=np.int64), K_max), K_max


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--domains", type=int, default=7)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--perms", type=str, default="200,1000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--flip", type=float, default=0.03)
    ap.add_argument("--host-spots", type=int, default=200)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    perms = [int(p) for p in a.perms.split(",")]
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.centrality import centrality
    from spadot_amd.neighbors import spatial_edges
    assert torch.cuda.is_available(), "centrality_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    sets = [synthetic(a.n, a.domains, a.flip, rng) for _ in range(a.tps)]
    shape = f"{a.tps} x {a.n} spots, K = {a.domains}, k = {a.k}"

    spatial_edges(sets[0][0], a.k, dev)                                        # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    edges = [spatial_edges(xy, a.k, dev) for xy, _ in sets]
    torch.cuda.synchronize()
    print(json.dumps(dict(what="graph", shape=shape, ms=round((time.perf_counter() - t0) * 1e3, 3))), flush=True)
    labs = [torch.as_tensor(lab, device=dev) for _, lab in sets]

    runs = [("labels", P, False) for P in perms] + [("sources", 0, True)]
    for what, P, sources in runs:
        src, dst, labels, desc, K_max = _prepared(edges, labs, a.domains, P, sources)
        keep = {}
        for path, limit in (("lds", None), ("scratch", 0)):
            ms = timed(lambda: keep.__setitem__(path, ops.hop_launch(src, dst, labels, desc, K_max, limit)), a.repeats)
            status = keep[path][3].cpu().numpy()
            rec = dict(what=what, path=path, shape=shape, relabelings=P, items=int(status.shape[0]), **median(ms),
                       status_max=int(status[:, 0].max()), rounds_max=int(status[:, 1].max()),
                       rounds_median=float(np.median(status[:, 1])))
            if not sources:
                rec["rounds_observed"] = status[np.cumsum([0] + [P + 1] * (a.tps - 1)), 1].tolist()
            print(json.dumps(rec), flush=True)
        same = all(bool(torch.equal(x, y)) for x, y in zip(keep["lds"], keep["scratch"]))
        print(json.dumps(dict(what="paths", of=what, relabelings=P, lds_equals_scratch=same)), flush=True)

    res = None
    for spots in (False, True):
        call = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = centrality(edges, labs, n_perms=perms[0], seed=0, n_clusters=[a.domains] * a.tps, spots=spots)
            call.append((time.perf_counter() - t0) * 1e3)
        rec = dict(what="call", shape=shape, relabelings=perms[0], spots=spots, **median(call),
                   closeness=np.round(res[0].closeness, 4).tolist(), closeness_z=np.round(res[0].closeness_z, 1).tolist())
        if spots:
            rec.update(diameter=[int(r.diameter) for r in res], radius=[int(r.radius) for r in res])
        print(json.dumps(rec), flush=True)

    if not a.skip_host:
        import hops_ref as ref
        s, d = (t.cpu().numpy() for t in edges[0])
        t0 = time.perf_counter()
        D = ref.dist_matrix(s, d, a.n)
        scipy_s = time.perf_counter() - t0
        same = bool(np.array_equal(np.where(D == ref.FAR, 0, D).astype(np.int64).sum(axis=1), res[0].spot_sumdist))
        rec = dict(what="host", shape=f"1 x {a.n} spots", scipy_shortest_path_s=round(scipy_s, 2), equal_to_device=same)
        try:
            import networkx as nx
            g = nx.Graph()
            g.add_nodes_from(range(a.n))
            g.add_edges_from(zip(s.tolist(), d.tolist()))
            some = np.random.default_rng(0).choice(a.n, min(a.host_spots, a.n), replace=False).tolist()
            t0 = time.perf_counter()
            got = [nx.closeness_centrality(g, u=u) for u in some]
            sec = time.perf_counter() - t0
            rec.update(networkx_closeness_s=round(sec, 2), networkx_spots=len(some),
                       networkx_scaled_s=round(sec / len(some) * a.n, 1), networkx_scaled_to=f"{a.n} spots, not measured",
                       networkx_equal_to_device=bool(np.allclose(got, res[0].spot_closeness_wf[some], rtol=1e-12, atol=0)))
        except ImportError:
            rec["networkx_closeness_s"] = None
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
