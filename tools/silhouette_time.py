#!/usr/bin/env python3
"""Time of the device silhouette on the MI355X:

    python tools/silhouette_time.py [--tps 5] [--n 10000] [--d 20] [--repeats 7] [--skip-host]

Synthetic latents (per time point 10 planted blobs, fp32) and the adaptive sweep's labelings: per time point one labeling for
every k = 4 .. 20 (nearest of k random points of the set, which gives clusters of the sizes a K-means fit has), 5 x 17 = 85
problems.  Prints JSON lines:
  * {"what": "launch"}:   spadot_silhouette alone, all problems in one launch, warm, device events, the median of `--repeats` and
                          the spread; the point pairs it evaluates and pairs per second;
  * {"what": "prepare"}:  the stable sort and the offsets in torch on the device, ending in a synchronise (host clock, warm median);
  * {"what": "download"}: a, b, nearest, s and the cluster sizes to the host and the means (host clock, warm median);
  * {"what": "call"}:     silhouette_many as a user calls it: upload of the labels, validation, the three steps above;
  * {"what": "host"}:     sklearn.metrics.silhouette_score on ONE labeling (k = 10) of ONE time point on the host, and that time
                          SCALED to all problems (`scaled_s`: not measured at full size); the device's score of the same labeling
                          beside sklearn's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import median  # noqa: E402

KS = list(range(4, 21))


def synthetic(tps, n, d, seed=1993):
    rng = np.random.default_rng(seed)
    Xs, labelings = [], []
    for _ in range(tps):
        cen = 3.0 * rng.normal(size=(10, d))
        x = (cen[rng.integers(0, 10, n)] + rng.normal(size=(n, d))).astype(np.float32)
        labs = []
        for k in KS:
            c = x[rng.choice(n, k, replace=False)].astype(np.float64)
            d2 = ((x.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * x.astype(np.float64) @ c.T + (c ** 2).sum(1)[None, :])
            labs.append(d2.argmin(1).astype(np.int64))
        Xs.append(x)
        labelings.append(labs)
    return Xs, labelings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import torch
    from spadot_amd.silhouette import SilhouetteBatch, silhouette_many
    assert torch.cuda.is_available(), "silhouette_time measures on the MI355X"
    Xh, labelings = synthetic(a.tps, a.n, a.d)
    Xs = [torch.as_tensor(x, device="cuda:0") for x in Xh]
    ncl = [list(KS) for _ in range(a.tps)]
    shape = f"{a.tps} x {a.n} x {a.d}, {a.tps * len(KS)} labelings"
    pairs = a.tps * len(KS) * a.n * a.n

    batch = SilhouetteBatch(Xs, labelings, ncl)
    batch.prepare()
    batch.launch()                                                 # warm: code object, allocator
    batch.results()
    torch.cuda.synchronize()
    launch, prepare, download = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        batch.prepare()
        torch.cuda.synchronize()
        prepare.append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        batch.launch()
        e1.record()
        e1.synchronize()
        launch.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        res = batch.results()
        download.append((time.perf_counter() - t0) * 1e3)
    rec = dict(what="launch", shape=shape, pairs=pairs, **median(launch))
    rec["Gpairs_per_s"] = round(pairs / (rec["median_ms"] * 1e-3) / 1e9, 2)
    print(json.dumps(rec), flush=True)
    print(json.dumps(dict(what="prepare", shape=shape, **median(prepare))), flush=True)
    print(json.dumps(dict(what="download", shape=shape, **median(download))), flush=True)

    call = []
    for _ in range(max(3, a.repeats // 2)):
        t0 = time.perf_counter()
        res = silhouette_many(Xs, labelings, ncl)
        call.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what="call", shape=shape, **median(call))), flush=True)

    if not a.skip_host:
        from sklearn.metrics import silhouette_score
        x64, lab = Xh[0].astype(np.float64), labelings[0][KS.index(10)]
        t0 = time.perf_counter()
        want = float(silhouette_score(x64, lab))
        s = time.perf_counter() - t0
        print(json.dumps(dict(what="host", shape=f"1 x {a.n} x {a.d}, 1 labeling (k = 10)", sklearn_s=round(s, 3),
                              scaled_s=round(s * a.tps * len(KS), 1), scaled_to=f"{a.tps * len(KS)} labelings, not measured",
                              sklearn_score=want, device_score=res[0][KS.index(10)].score,
                              host_threads=os.environ.get("OMP_NUM_THREADS", "default"))), flush=True)


if __name__ == "__main__":
    main()
