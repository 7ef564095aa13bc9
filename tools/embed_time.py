#!/usr/bin/env python3
"""Time of the device t-SNE on the MI355X:

    python tools/embed_time.py [--tps 5] [--n 10000] [--d 20] [--perplexity 30] [--n_iter 1000] [--repeats 3] [--slices S]
                               [--two] [--only joint|per|host] [--cpu]

Synthetic latents (per time point 10 planted blobs in d dimensions, fp64), embedded jointly (one problem of tps x n points) and per
time point (tps problems of one launch).  Prints JSON lines, one per phase and mode:
  * {"what": "knn"}:         spadot_latent_knn alone, warm, device events, the median of `--repeats` and the spread; the ordered pairs
                             it evaluates and pairs per second;
  * {"what": "affinities"}:  spadot_tsne_affinities alone, likewise;
  * {"what": "symmetrise"}:  the download of idx and the conditionals, joint_csr on the host and the upload (host clock, one run);
  * {"what": "iterations"}:  `--n_iter` iterations queued in one call between two events: milliseconds per iteration and the ordered
                             pairs of the repulsion per second (ripley's 3.2e11 distances per second is the yardstick for this
                             kind of kernel); `--slices` overrides the slice rule and `--two` gives a thread two query points;
  * {"what": "host"} with --cpu: sklearn.manifold.TSNE(method="barnes_hut") on the same data on this machine's host, as context
                             (`--only host`: that alone)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import median, timed  # noqa: E402


def synthetic(tps, n, d, seed=1993):
    rng = np.random.default_rng(seed)
    Xs = []
    for _ in range(tps):
        cen = 3.0 * rng.normal(size=(10, d))
        Xs.append(cen[rng.integers(0, 10, n)] + rng.normal(size=(n, d)))
    return Xs


def measure(mode, Xh, a):
    import torch
    from spadot_amd import stage_ops as so
    from spadot_amd.embed import TsneBatch, joint_csr
    Xs = [torch.as_tensor(x, device="cuda:0") for x in Xh]
    sizes = [int(x.shape[0]) for x in Xs]
    shape = f"{mode}: {len(Xs)} x {sizes[0]} x {a.d}, perplexity {a.perplexity}"
    pairs = sum(n * (n - 1) for n in sizes)
    desc, perp = so.embed_table(sizes, a.perplexity, a.slices)
    desc_dev = torch.as_tensor(desc, device="cuda:0")
    X = torch.cat(Xs).contiguous()
    out = so.latent_knn_launch(X, desc, desc_dev)
    rec = dict(what="knn", shape=shape, pairs=pairs, **median(timed(lambda: so.latent_knn_launch(X, desc, desc_dev, out=out), a.repeats)))
    rec["Gpairs_per_s"] = round(pairs / (rec["median_ms"] * 1e-3) / 1e9, 2)
    print(json.dumps(rec), flush=True)
    idx, d2 = out
    rec = dict(what="affinities", shape=shape, rows=sum(sizes),
               **median(timed(lambda: so.tsne_affinities_launch(d2, desc, perp, desc_dev), a.repeats)))
    print(json.dumps(rec), flush=True)
    cond, _beta = so.tsne_affinities_launch(d2, desc, perp, desc_dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx_h, cond_h = idx.cpu().numpy(), cond.cpu().numpy()
    csr = [joint_csr(idx_h[koff:koff + n * k].reshape(n, k), cond_h[koff:koff + n * k].reshape(n, k))
           for _off, n, k, koff, *_rest in desc.tolist()]
    dev = [torch.as_tensor(np.concatenate([c[i] for c in csr]), device="cuda:0") for i in range(3)]
    torch.cuda.synchronize()
    print(json.dumps(dict(what="symmetrise", shape=shape, stored=int(dev[1].numel()), longest_row=int(max(np.diff(c[0]).max()
                          for c in csr)), host_ms=round((time.perf_counter() - t0) * 1e3, 1))), flush=True)
    del dev
    ms = []
    for _ in range(a.repeats):
        batch = TsneBatch(Xs, a.perplexity, n_iter=a.n_iter, slices=a.slices, two=a.two)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        batch.steps(a.n_iter)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    res = batch.results()
    rec = dict(what="iterations", shape=shape, n_iter=a.n_iter, slices=[r.slices for r in res], two=bool(a.two), **median(ms))
    rec["ms_per_iteration"] = round(rec["median_ms"] / max(a.n_iter, 1), 4)
    rec["Gpairs_per_s"] = round(pairs * a.n_iter / (rec["median_ms"] * 1e-3) / 1e9, 2)
    rec["kl_first_last"] = [[float(r.kl[0]), float(r.kl[-1])] for r in res] if a.n_iter else []
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--n_iter", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slices", type=int, default=None)
    ap.add_argument("--two", action="store_true")
    ap.add_argument("--only", choices=("joint", "per", "host"), default=None)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    Xh = synthetic(a.tps, a.n, a.d)
    if a.only != "host":
        import torch
        assert torch.cuda.is_available(), "embed_time measures on the MI355X"
        if a.only != "per":
            measure("joint", [np.concatenate(Xh)], a)
        if a.only != "joint":
            measure("per time point", Xh, a)
    if a.cpu or a.only == "host":
        from sklearn.manifold import TSNE
        X = np.concatenate(Xh)
        t0 = time.perf_counter()
        sk = TSNE(perplexity=a.perplexity, method="barnes_hut", init="pca", max_iter=a.n_iter, random_state=0)
        sk.fit_transform(X)
        print(json.dumps(dict(what="host", shape=f"joint: 1 x {X.shape[0]} x {a.d}", sklearn_barnes_hut_s=round(time.perf_counter()
                              - t0, 1), n_iter=int(sk.n_iter_), kl=float(sk.kl_divergence_),
                              host_threads=os.environ.get("OMP_NUM_THREADS", "default"))), flush=True)


if __name__ == "__main__":
    main()
