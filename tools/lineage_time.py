#!/usr/bin/env python3
"""Device time of the plan-apply kernels and wall time of the lineage part of the analyze stage on the MI355X (DESIGN 7b,
"Domain lineages"):

    python tools/lineage_time.py [--n 10000] [--tps 5] [--dim 20] [--alternations 7] [--skip-analyze] [--out DIR]

Seeded synthetic latents (those of tools/analyze_time.py), no files read.
  * apply: one n x n pair in f32 storage, solved once with the analyze stage's configuration; for nrhs = 1, 10, 64 and both
    directions OTSolver.apply against the only route there was before it, OTSolver.plan("torch", dtype=float64) followed by
    torch.matmul.  Both are warmed up for every shape, then timed alternately with device events (one event pair around one
    call of each, `--alternations` times); reported: median, minimum and maximum per variant, the algorithmic bytes
    (I * ld * 4 for K plus the fp64 P and Q) and fp64 operations (2 * I * J * nrhs) of apply over its median time.
    The fp64 vector peak quoted beside them (78.6 TFLOP/s) is AMD's published figure, not a measurement of this script.
  * analyze(args) in adaptive mode on tps x n x dim latents written as latent.npz, without and with lineage: both timings dicts.
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

PEAK_FP64_VECTOR_TFLOPS = 78.6       # AMD's published MI355X figure; not measured here
PEAK_HBM_TBS = 8.0                   # likewise


def latents(n, tps, dim, seed=1993):
    rng = np.random.default_rng(seed)
    out = []
    for t in range(tps):
        k = 6 + t % 5
        cen = 3.0 * rng.normal(size=(k, dim))
        out.append((cen[rng.integers(0, k, n)] + rng.normal(size=(n, dim))).astype(np.float32))
    return out


def event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1)


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4)}


def time_apply(Ls, alternations):
    import torch
    from spadot_amd import analyze_ot
    n = Ls[0].shape[0]
    solver, _ = analyze_ot.spot_transport(Ls[0], Ls[1], which="first", storage="f32")
    rows = []
    try:
        I, J, ld = solver.I, solver.J, solver.ld
        rng = np.random.default_rng(0)
        for nrhs in (1, 10, 64):
            for transpose in (False, True):
                P = torch.as_tensor(rng.uniform(size=(I if transpose else J, nrhs)), device="cuda:0")
                ours = lambda: solver.apply(P, transpose=transpose)

                def parent():
                    plan = solver.plan("torch", dtype=torch.float64)
                    return torch.matmul(plan.T if transpose else plan, P)
                for _ in range(2):                                   # warm-up of this shape, both variants
                    a, b = ours(), parent()
                torch.cuda.synchronize()
                rel = float(((a - b).abs().max() / b.abs().max()).item())
                del a, b
                t_ours, t_parent = [], []
                for _ in range(alternations):
                    t_ours.append(event_ms(ours))
                    t_parent.append(event_ms(parent))
                so, sp = stats(t_ours), stats(t_parent)
                nbytes = I * ld * 4 + 8 * nrhs * (I + J)
                flops = 2.0 * I * J * nrhs
                sec = so["median_ms"] * 1e-3
                tbs, tfl = nbytes / sec / 1e12, flops / sec / 1e12
                rows.append({"nrhs": nrhs, "direction": "push" if transpose else "pull", "apply": so, "plan_matmul": sp,
                             "speedup_median": round(sp["median_ms"] / so["median_ms"], 2),
                             "apply_TB_s": round(tbs, 3), "apply_TFLOP_s": round(tfl, 3),
                             "share_of_hbm_peak": round(tbs / PEAK_HBM_TBS, 3),
                             "share_of_fp64_vector_peak": round(tfl / PEAK_FP64_VECTOR_TFLOPS, 3),
                             "nearer_bound": "fp64" if tfl / PEAK_FP64_VECTOR_TFLOPS > tbs / PEAK_HBM_TBS else "hbm",
                             "max_rel_diff_vs_plan_matmul": rel})
    finally:
        solver.close()
    return {"shape": f"{n} x {n}", "storage": "f32", "alternations": alternations, "rows": rows}


def time_analyze(Ls, out):
    from spadot_amd import analyze
    n_all = sum(x.shape[0] for x in Ls)
    rng = np.random.default_rng(0)
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, "latent.npz"), X=np.concatenate(Ls), rows=np.arange(n_all),
                        timepoint=np.repeat(np.arange(len(Ls)), [x.shape[0] for x in Ls]),
                        spatial=rng.uniform(0, 100, size=(n_all, 2)))
    rec = {}
    for name, flag in (("warm_up", False), ("without_lineage", False), ("with_lineage", True)):
        class Args:
            data = os.path.join(out, "latent.npz")
            output_dir = os.path.join(out, name)
            prefix = ""
            n_clusters = None
            device = "cuda:0"
            lineage = flag
        t0 = time.perf_counter()
        r = analyze(Args())
        rec[name] = {"total_s": round(time.perf_counter() - t0, 3), "timings_s": {k: round(v, 3) for k, v in r["timings"].items()},
                     "n_clusters": r["n_clusters"]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--dim", type=int, default=20)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--skip-analyze", action="store_true")
    ap.add_argument("--out", default=None, help="directory for analyze's outputs (default: a temporary one)")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "lineage_time measures on the MI355X"
    assert a.alternations >= 5 and a.tps >= 2
    Ls = latents(a.n, a.tps, a.dim)
    rec = {"device": torch.cuda.get_device_name(0), "apply": time_apply(Ls, a.alternations)}
    if not a.skip_analyze:
        rec["analyze"] = dict(time_analyze(Ls, a.out or tempfile.mkdtemp(prefix="lineage_time_")), shape=f"{a.tps} x {a.n} x {a.dim}")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
