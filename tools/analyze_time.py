#!/usr/bin/env python3
"""Wall time of the analyze stage on the MI355X (DESIGN "The analyze stage's K-means sweep"):

    python tools/analyze_time.py [--n 10000] [--tps 5] [--dim 20] [--skip-sklearn] [--out DIR]

Synthetic latents (per time point well-separated blobs of 6 .. 10 clusters plus noise, seed 1993), then
  * device: kmeans.fit_sweep over k = 4 .. 20, n_init = 10, all time points at once (first call, and a second call on
    warm code objects and allocator), host clock around work that ends in a device synchronise;
  * sklearn: the reference's loop, KMeans(k, random_state=1993, n_init=10).fit per time point and k, on 16 threads;
  * analyze(args) in adaptive mode on the same latents written as latent.npz: clustering, OT and writing.
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def latents(n, tps, dim, seed=1993):
    rng = np.random.default_rng(seed)
    out = []
    for t in range(tps):
        k = 6 + t % 5
        cen = 3.0 * rng.normal(size=(k, dim))
        out.append((cen[rng.integers(0, k, n)] + rng.normal(size=(n, dim))).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--dim", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-sklearn", action="store_true")
    ap.add_argument("--out", default=None, help="directory for analyze's outputs (default: a temporary one)")
    a = ap.parse_args()
    import torch
    from spadot_amd import analyze
    from spadot_amd.kmeans import fit_sweep
    from spadot_amd.utils._analyze_utils import select_k
    assert torch.cuda.is_available(), "analyze_time measures on the MI355X"
    Ls = latents(a.n, a.tps, a.dim)
    ks = list(range(4, 21))
    rec = {"shape": f"{a.tps} x {a.n} x {a.dim}", "ks": "4..20", "n_init": 10}
    Xs = [torch.as_tensor(x, device="cuda:0") for x in Ls]
    torch.cuda.synchronize()
    for name in ("device_sweep_first_s", "device_sweep_s"):
        t0 = time.perf_counter()
        res = fit_sweep(Xs, [ks] * a.tps)
        torch.cuda.synchronize()
        rec[name] = round(time.perf_counter() - t0, 4)
    rec["device_k"] = [select_k([res[t][k].inertia_ for k in ks]) for t in range(a.tps)]
    rec["device_iters_max"] = int(max(r.n_iter_ for d in res for r in d.values()))
    if not a.skip_sklearn:
        import contextlib
        from sklearn.cluster import KMeans
        try:
            from threadpoolctl import threadpool_limits
            lim = threadpool_limits(limits=a.threads)
        except ImportError:
            lim = contextlib.nullcontext()
        with lim:
            t0 = time.perf_counter()
            sk = [[KMeans(n_clusters=k, random_state=1993, n_init=10).fit(x).inertia_ for k in ks] for x in Ls]
            rec["sklearn_sweep_s"] = round(time.perf_counter() - t0, 3)
        rec["sklearn_threads"] = a.threads
        rec["sklearn_k"] = [select_k(w) for w in sk]
        rec["inertia_rel_dev_vs_sklearn_max"] = float(max(abs(res[t][k].inertia_ - sk[t][i]) / sk[t][i]
                                                          for t in range(a.tps) for i, k in enumerate(ks)))
    out = a.out or tempfile.mkdtemp(prefix="analyze_time_")
    os.makedirs(out, exist_ok=True)
    n_all = a.n * a.tps
    rng = np.random.default_rng(0)
    np.savez_compressed(os.path.join(out, "latent.npz"), X=np.concatenate(Ls), rows=np.arange(n_all),
                        timepoint=np.repeat(np.arange(a.tps), a.n), spatial=rng.uniform(0, 100, size=(n_all, 2)))

    class Args:
        data = os.path.join(out, "latent.npz")
        output_dir = out
        prefix = ""
        n_clusters = None
        device = "cuda:0"
    t0 = time.perf_counter()
    r = analyze(Args())
    rec["analyze_total_s"] = round(time.perf_counter() - t0, 3)
    rec["analyze_s"] = {k: round(v, 3) for k, v in r["timings"].items()}
    rec["analyze_k"] = r["n_clusters"]
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
