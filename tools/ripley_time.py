#!/usr/bin/env python3
"""Time of the ripley counts on the MI355X:

    python tools/ripley_time.py [--tps 5] [--n 10000] [--domains 7] [--bins 50] [--n_sim 99] [--n_probes 1000] [--repeats 7]
                                [--host-sims 3] [--skip-host]

Synthetic time points: n spots on a jittered grid, `--domains` planted Voronoi domains, the stage's default radii, all three
statistics.  Prints JSON lines:
  * {"what": "launch", "null": ..}:  stage_ops.ripley_launch on checked arrays: the four host-to-device copies of the descriptor,
                                     thresholds, vertices and areas, then spadot_ripley_counts (the zeroing of the output and
                                     the counting launch), all time points in one call, warm, device events, the median of
                                     `--repeats` and the spread, for either null; distance evaluations per second;
  * {"what": "call"}:                ripley as a user calls it: validation, the sort by label, the hulls, launch, download, the
                                     host statistics (host clock), null "labels";
  * {"what": "host"}:                the numpy restatement (tests/ripley_ref.py) on ONE time point with `--host-sims`
                                     simulations, checked against the device, for scale."""
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


def _prepared(sets, K, radii, S, M, null, dev):
    """The tensors and the checked arrays of one call (as ripley_counts builds them)."""
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.ripley import convex_window
    desc = np.zeros((len(sets), ops.RIPLEY_DESC), dtype=np.int64)
    parts, wins, first = [], [], 0
    for g, (xy, lab) in enumerate(sets):
        parts.append(xy[np.argsort(lab, kind="stable")])
        desc[g, :9] = (first, lab.shape[0], K, radii[g].shape[0], S, M, int(null == "csr"), 7, g)
        desc[g, 13:13 + K] = np.cumsum(np.bincount(lab, minlength=K))
        wins.append(convex_window(xy)[:2])
        first += lab.shape[0]
    x = torch.as_tensor(np.ascontiguousarray(np.concatenate(parts)), device=dev)
    B = max(r.shape[0] for r in radii)
    checked = ops.ripley_check(x, desc, [r * r for r in radii], wins, K, S, B)
    out = torch.empty((len(sets), K, 1 + S, 3, B), dtype=torch.int64, device=dev)
    return x, checked, K, S, B, 0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--domains", type=int, default=7)
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--n_sim", type=int, default=99)
    ap.add_argument("--n_probes", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-sims", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.cooccurrence import default_radii
    from spadot_amd.ripley import ripley, ripley_counts
    assert torch.cuda.is_available(), "ripley_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    sets = [synthetic(a.n, a.domains, rng) for _ in range(a.tps)]
    radii = [default_radii(xy, a.bins) for xy, _ in sets]
    shape = f"{a.tps} x {a.n} spots, K = {a.domains}, S = {a.n_sim}, M = {a.n_probes}, B = {a.bins}"
    sizes = np.stack([np.bincount(lab, minlength=a.domains) for _, lab in sets]).astype(np.float64)
    d2 = int((1 + a.n_sim) * (sizes * (sizes - 1) + a.n_probes * sizes).sum())

    for null in ("labels", "csr"):
        prep = _prepared(sets, a.domains, radii, a.n_sim, a.n_probes, null, dev)
        rec = dict(what="launch", null=null, shape=shape, distances=d2, **median(timed(lambda: ops.ripley_launch(*prep), a.repeats)))
        rec["Gdistances_per_s"] = round(d2 / (rec["median_ms"] * 1e-3) / 1e9, 2)
        print(json.dumps(rec), flush=True)

    coords = [torch.as_tensor(xy, device=dev) for xy, _ in sets]
    labs = [lab for _, lab in sets]
    call = []
    for _ in range(max(3, a.repeats // 2)):
        t0 = time.perf_counter()
        ripley(coords, labs, radii=radii, n_sim=a.n_sim, n_probes=a.n_probes, n_clusters=[a.domains] * a.tps)
        call.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what="call", null="labels", shape=shape, **median(call))), flush=True)

    if not a.skip_host:
        import ripley_ref as ref
        xy, lab = sets[0]
        t0 = time.perf_counter()
        want = ref.counts(xy, lab, radii[0] ** 2, a.domains, a.host_sims, a.n_probes, "labels", 0, 0)
        s = time.perf_counter() - t0
        got = ripley_counts([coords[0]], [lab], radii=[radii[0]], n_sim=a.host_sims, n_probes=a.n_probes, n_clusters=[a.domains])[0]
        print(json.dumps(dict(what="host", shape=f"1 x {a.n} spots, K = {a.domains}, S = {a.host_sims}, M = {a.n_probes}, "
                                                 f"B = {a.bins}", numpy_s=round(s, 3),
                              equal_to_device=bool(np.array_equal(want, got)))), flush=True)


if __name__ == "__main__":
    main()
