#!/usr/bin/env python3
"""Time of the co-occurrence counts on the MI355X:

    python tools/cooccur_time.py [--tps 5] [--n 10000] [--domains 12] [--bins 50] [--repeats 7] [--big 100000] [--skip-host]

Synthetic time points: n spots on a jittered grid, `--domains` planted Voronoi domains, the stage's default radii.  Prints JSON
lines:
  * {"what": "launch"}:   spadot_cooccur_counts alone (the zeroing of the output and the counting launch), all time points in one
                          call, warm, device events, the median of `--repeats` and the spread; (pair, threshold) tests per second;
  * {"what": "call"}:     cooccurrence as a user calls it: validation, the sort by label, launch, download, the host statistics
                          (host clock);
  * {"what": "big"}:      ONE time point of `--big` spots, launch alone (device events), once warm;
  * {"what": "host"}:     the numpy restatement (tests/cooccur_ref.py) on 2 000 spots of one time point, checked against the
                          device, and that time SCALED by (n / 2000)^2 to all time points (`scaled_s`: not measured at full
                          size, where the restatement's n x n matrix cannot be formed)."""
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


def _prepared(sets, K, radii, dev):
    """The tensors and the checked descriptor of one call (as cooccurrence_counts builds them)."""
    import torch
    from spadot_amd import stage_ops as ops
    desc = np.zeros((len(sets), ops.COOCCUR_DESC), dtype=np.int64)
    parts, first = [], 0
    for g, (xy, lab) in enumerate(sets):
        order = np.argsort(lab, kind="stable")
        parts.append(xy[order])
        desc[g, :4] = (first, lab.shape[0], K, radii[g].shape[0])
        desc[g, 5:5 + K] = np.cumsum(np.bincount(lab, minlength=K))
        first += lab.shape[0]
    x = torch.as_tensor(np.ascontiguousarray(np.concatenate(parts)), device=dev)
    B = max(r.shape[0] for r in radii)
    desc, pad = ops.cooccur_check(x, desc, [r * r for r in radii], K, B)
    out = torch.empty((len(sets), K, K, B), dtype=torch.int64, device=dev)
    return x, desc, pad, K, B, out, torch.as_tensor(desc, device=dev), torch.as_tensor(pad, device=dev)


def _time_launch(prep, repeats):
    from spadot_amd import stage_ops as ops
    return timed(lambda: ops.cooccur_launch(*prep), repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--domains", type=int, default=12)
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--big", type=int, default=100000)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd.cooccurrence import cooccurrence, default_radii
    assert torch.cuda.is_available(), "cooccur_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    sets = [synthetic(a.n, a.domains, rng) for _ in range(a.tps)]
    radii = [default_radii(xy, a.bins) for xy, _ in sets]
    shape = f"{a.tps} x {a.n} spots, K = {a.domains}, B = {a.bins}"
    tests = a.tps * a.n * (a.n - 1) * a.bins

    rec = dict(what="launch", shape=shape, pair_threshold_tests=tests, **median(_time_launch(_prepared(sets, a.domains, radii, dev),
                                                                                              a.repeats)))
    rec["Gtests_per_s"] = round(tests / (rec["median_ms"] * 1e-3) / 1e9, 2)
    print(json.dumps(rec), flush=True)

    coords = [torch.as_tensor(xy, device=dev) for xy, _ in sets]
    labs = [lab for _, lab in sets]
    call = []
    for _ in range(max(3, a.repeats // 2)):
        t0 = time.perf_counter()
        res = cooccurrence(coords, labs, radii=radii, n_clusters=[a.domains] * a.tps)
        call.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what="call", shape=shape, **median(call))), flush=True)

    if a.big > 0:
        xy, lab = synthetic(a.big, a.domains, rng)
        ms = _time_launch(_prepared([(xy, lab)], a.domains, [default_radii(xy, a.bins)], dev), 1)
        bt = a.big * (a.big - 1) * a.bins
        print(json.dumps(dict(what="big", shape=f"1 x {a.big} spots, K = {a.domains}, B = {a.bins}", launch_ms=round(ms[0], 3),
                              pair_threshold_tests=bt, Gtests_per_s=round(bt / (ms[0] * 1e-3) / 1e9, 2))), flush=True)

    if not a.skip_host:
        import cooccur_ref as ref
        m = min(2000, a.n)
        xy, lab = sets[0][0][:m], sets[0][1][:m]
        t0 = time.perf_counter()
        want = ref.counts(xy, lab, radii[0] ** 2, a.domains)
        s = time.perf_counter() - t0
        got = cooccurrence([torch.as_tensor(xy, device=dev)], [lab], radii=[radii[0]], n_clusters=[a.domains])[0].counts
        print(json.dumps(dict(what="host", shape=f"1 x {m} spots, B = {a.bins}", numpy_s=round(s, 3),
                              scaled_s=round(s * (a.n / m) ** 2 * a.tps, 2), scaled_to=f"{shape}, not measured",
                              equal_to_device=bool(np.array_equal(want, got)))), flush=True)
    del res


if __name__ == "__main__":
    main()
