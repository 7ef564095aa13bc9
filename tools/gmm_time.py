#!/usr/bin/env python3
"""Time of the device Gaussian mixtures on the MI355X:

    python tools/gmm_time.py [--tps 5] [--n 10000] [--d 20] [--repeats 5] [--skip-host]

Synthetic latents (per time point 10 planted blobs, fp32) and the adaptive sweep's starts: per time point one labeling for every
k = 4 .. 20 (nearest of k random points of the set, which gives clusters of the sizes a K-means fit has), 5 x 17 = 85 problems.
Prints JSON lines:
  * {"what": "iteration"}: one EM iteration of all problems (the points launch, the M-step launch, the stop launch), nothing
                           frozen, warm, device events, the median of `--repeats` and the spread;
  * {"what": "m_step"} / {"what": "e_step"}: the first M-step (from the one-hot labels) and the last E-step alone, device events;
  * {"what": "stages"}:    by a host clock: upload and validation of the labels, centring and buffers (each once, cold), and
                           fit_sweep as a user calls it (warm median: those two, the EM loop with its host round trips, the last
                           E-step and the download); the iteration counts of the problems;
  * {"what": "host"}:      sklearn.mixture.GaussianMixture with the same start on ONE problem (k = 10) of ONE time point on the
                           host, and that time SCALED to all problems (`scaled_s`: not measured at full size); the device's
                           n_iter and lower bound of the same problem beside sklearn's."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from _timing import median, timed  # noqa: E402

KS = list(range(4, 21))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import torch
    from silhouette_time import synthetic
    from spadot_amd import gmm
    assert torch.cuda.is_available(), "gmm_time measures on the MI355X"
    Xh, labelings = synthetic(a.tps, a.n, a.d)
    Xs = [torch.as_tensor(x, device="cuda:0") for x in Xh]
    ncl = [list(KS) for _ in range(a.tps)]
    shape = f"{a.tps} x {a.n} x {a.d}, {a.tps * len(KS)} mixtures"

    t0 = time.perf_counter()
    sets = gmm._as_sets(Xs)
    psets, _, Ks, labels = gmm._labels_on_device(sets, labelings, ncl)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    b = gmm._Batch(sets, psets, Ks)
    onehot = torch.zeros((b.total, b.K_max), dtype=torch.float64, device=b.dev).scatter_(1, labels[:, None], 1.0)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    validate_ms, buffers_ms = round((t1 - t0) * 1e3, 3), round((t2 - t1) * 1e3, 3)      # cold: the first touch of the device
    b.em(0, 1e-6, 1e-3, resp_init=onehot)                          # warm: code objects, allocator
    b.em(1, 1e-6, -1.0)                                            # tol < 0: nothing ever stops
    b.estep()
    torch.cuda.synchronize()
    m_step = timed(lambda: b.em(0, 1e-6, -1.0, resp_init=onehot), a.repeats, warm=False)
    print(json.dumps(dict(what="m_step", shape=shape, **median(m_step))), flush=True)
    print(json.dumps(dict(what="iteration", shape=shape, **median(timed(lambda: b.em(1, 1e-6, -1.0), a.repeats, warm=False)))), flush=True)
    print(json.dumps(dict(what="e_step", shape=shape, **median(timed(lambda: b.estep(), a.repeats, warm=False)))), flush=True)
    del b, onehot

    stages = []
    for _ in range(max(2, a.repeats // 2)):
        t0 = time.perf_counter()
        res = gmm.fit_sweep(Xs, labelings, ncl)
        stages.append((time.perf_counter() - t0) * 1e3)
    iters = [r.n_iter_ for rt in res for r in rt]
    print(json.dumps(dict(what="stages", shape=shape, validate_ms=validate_ms, buffers_ms=buffers_ms,
                          fit_sweep=median(stages), n_iter_min=min(iters), n_iter_median=int(statistics.median(iters)),
                          n_iter_max=max(iters), converged=int(sum(r.converged_ for rt in res for r in rt)))), flush=True)

    if not a.skip_host:
        import warnings
        from sklearn.mixture import GaussianMixture
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import gmm_ref as ref
        x64, lab, k = Xh[0].astype(np.float64), labelings[0][KS.index(10)], 10
        xc = x64 - x64.mean(0)
        p0 = ref.m_step(xc, ref.one_hot(lab, k))
        prec = np.stack([pc @ pc.T for pc in p0["precisions_cholesky"]])
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g = GaussianMixture(k, covariance_type="full", reg_covar=1e-6, tol=1e-3, max_iter=100, weights_init=p0["weights"] /
                                p0["weights"].sum(), means_init=p0["means"], precisions_init=prec).fit(xc)
        s = time.perf_counter() - t0
        mine = res[0][KS.index(10)]
        print(json.dumps(dict(what="host", shape=f"1 x {a.n} x {a.d}, 1 mixture (k = 10)", sklearn_s=round(s, 3),
                              scaled_s=round(s * a.tps * len(KS), 1), scaled_to=f"{a.tps * len(KS)} mixtures, not measured",
                              sklearn_n_iter=int(g.n_iter_), device_n_iter=mine.n_iter_, sklearn_lower_bound=float(g.lower_bound_),
                              device_lower_bound=mine.lower_bound_, host_threads=os.environ.get("OMP_NUM_THREADS", "default"))),
              flush=True)


if __name__ == "__main__":
    main()
