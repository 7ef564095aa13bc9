#!/usr/bin/env python3
"""Time of the ligand-receptor sums and comparisons on the MI355X:

    python tools/ligrec_time.py [--tps 5] [--n 10000] [--genes 3000] [--density 0.15] [--domains 10] [--pairs 1000]
                                [--named 1000] [--perms 1000] [--repeats 3] [--skip-host] [--skip-call]

Synthetic time points (tools/autocorr_time.py: sparse counts with `--density` of the entries stored) as a DeviceCounts with the
values of trends.lognorm_values, `--domains` random domains per time point and `--pairs` interactions that name `--named` genes.
Prints JSON lines:
  * {"what": "candidate"}:  spadot_ligrec_sums alone, the observed labeling and all permutations of all time points and named
                            genes in one launch, warm, device events, the median of `--repeats` and the spread, for every gene
                            chunk in (64, 128, 256) and workgroup size in (256, 512): how the defaults were chosen; entry terms
                            (stored entries of the named genes x labelings) per second;
  * {"what": "prologue"}:   the default configuration with P = 0: the observed labeling alone (label bytes, searches, one pass
                            with the counts), device events;
  * {"what": "count"}:      spadot_ligrec_count on the sums of the last launch with every cell tested, device events;
  * {"what": "call"}:       ligrec as a user calls it: values, validation, both launches, the mask's round trip, download, the host
                            statistics (host clock), and the device milliseconds of its launches;
  * {"what": "host"}:       the numpy restatement (tests/ligrec_ref.py) on 8 genes and 5 permutations of ONE time point, and that
                            time SCALED to all named genes and labelings of all time points (`scaled_s`: not measured at full
                            size)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from _timing import median, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=3000)
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--domains", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--named", type=int, default=1000)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-call", action="store_true")
    a = ap.parse_args()
    import torch
    from autocorr_time import synthetic
    from spadot_amd import stage_ops as ops
    from spadot_amd.ligrec import _device_args, ligrec
    from spadot_amd.preprocess import DeviceCounts
    from spadot_amd.trends import lognorm_values
    assert torch.cuda.is_available(), "ligrec_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    dc = DeviceCounts(synthetic(a.tps, a.n, a.genes, a.density, rng), dev)
    values = lognorm_values(dc)
    K, T = a.domains, dc.T
    lab = rng.integers(K, size=dc.n)
    named = np.sort(rng.choice(a.genes, size=min(a.named, a.genes), replace=False))
    ends = np.concatenate([named, rng.choice(named, size=max(0, 2 * a.pairs - named.size))])[:2 * a.pairs]
    pairs = rng.permutation(ends).reshape(-1, 2)
    sel = np.unique(pairs)
    ns, M = int(sel.size), int(pairs.shape[0])
    colptr = dc.colptr.cpu().numpy()
    stored = int((colptr[sel + 1] - colptr[sel]).sum())
    terms = stored * (a.perms + 1)
    shape = (f"{T} x {a.n} spots x {a.genes} genes, {K} domains, {M} interactions over {ns} genes ({stored} stored entries), "
             f"{a.perms} permutations")

    args, desc, K = _device_args(dc, values, lab, sel, K)
    checked = ops.ligrec_check(*args, desc, K, True, 0, a.perms)
    desc_dev = torch.as_tensor(checked[0], device=dev)
    out = (torch.empty((T, 1 + a.perms, ns, K), dtype=torch.float64, device=dev), torch.empty((T, ns, K), dtype=torch.int32, device=dev))
    for gc in (64, 128, 256):
        for threads in (256, 512):
            ms = timed(lambda: ops.ligrec_launch(*args, checked, K, True, 0, a.perms, 0, None, out, threads, gc, desc_dev), a.repeats)
            rec = dict(what="candidate", shape=shape, threads=threads, gene_chunk=gc, entry_terms=terms,
                       default=(threads, gc) == (ops.LIGREC_THREADS, ops.LIGREC_GC), **median(ms))
            rec["Gterms_per_s"] = round(terms / (rec["median_ms"] * 1e-3) / 1e9, 2)
            print(json.dumps(rec), flush=True)
    out0 = (torch.empty((T, 1, ns, K), dtype=torch.float64, device=dev), out[1])
    ms = timed(lambda: ops.ligrec_launch(*args, checked, K, True, 0, 0, 0, None, out0, None, None, desc_dev), a.repeats)
    print(json.dumps(dict(what="prologue", shape=shape + ", P = 0", threads=ops.LIGREC_THREADS, gene_chunk=ops.LIGREC_GC,
                          **median(ms))), flush=True)

    sizes = np.stack([np.bincount(lab[int(dc.tp_off_host[t]):int(dc.tp_off_host[t + 1])], minlength=K) for t in range(T)])
    wk = torch.as_tensor(1.0 / np.maximum(sizes, 1), device=dev)
    S0 = out[0][:, 0].clone()
    mask = torch.ones((T, M, K, K), dtype=torch.uint8, device=dev)
    ge = torch.zeros((T, M, K, K), dtype=torch.int32, device=dev)
    pos = torch.as_tensor(np.searchsorted(sel, pairs).astype(np.int32), device=dev)
    ms = timed(lambda: ops.ligrec_count(S0, out[0], wk, pos, (0, ns - 1), mask, 1, ge), a.repeats)
    print(json.dumps(dict(what="count", shape=shape, comparisons=T * M * K * K * a.perms, **median(ms))), flush=True)
    S_first = out[0][0, :6].cpu().numpy()
    del out, out0, S0, mask, ge
    torch.cuda.empty_cache()

    if not a.skip_call:
        call, launches = [], {}
        for _ in range(2):
            t0 = time.perf_counter()
            ligrec(dc, lab[np.argsort(dc.perm)], pairs, n_perms=a.perms, seed=0, values=values, timings=launches)
            call.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(what="call", shape=shape, launch_ms=[round(v, 3) for v in launches["launch_ms"]], **median(call))),
              flush=True)

    if not a.skip_host:
        import ligrec_ref as ref
        n0 = int(dc.tp_off_host[1])
        ridx, vals = dc.ridx.cpu().numpy(), values.cpu().numpy()
        V = np.zeros((n0, 8), dtype=np.float32)
        for j, g in enumerate(sel[:8]):
            seg = slice(int(colptr[g]), int(colptr[g + 1]))
            keep = ridx[seg] < n0
            V[ridx[seg][keep], j] = vals[seg][keep]
        t0 = time.perf_counter()
        wS = ref.sums(V, ref.labelings(lab[:n0], 5, 0, 0), K)
        s = time.perf_counter() - t0
        rec = dict(what="host", shape=f"1 x {a.n} spots x 8 genes, 5 permutations", numpy_s=round(s, 4),
                   scaled_s=round(s / (8 * 6) * ns * (a.perms + 1) * T, 1),
                   scaled_to=f"{T} x {ns} genes x {a.perms + 1} labelings, not measured")
        if a.perms >= 5:
            rec["within_bound_of_device"] = bool(np.all(np.abs(S_first[:, :8] - wS) <= ref.sum_bound(wS, ref.stored(V))))
            rec["largest_difference"] = float(np.abs(S_first[:, :8] - wS).max())
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
