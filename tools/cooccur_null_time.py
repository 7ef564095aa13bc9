#!/usr/bin/env python3
"""Time of the co-occurrence null on the MI355X, on the workload of tools/cooccur_time.py:

    python tools/cooccur_null_time.py [--tps 5] [--n 10000] [--domains 12] [--bins 50] [--n_perms 99] [--repeats 7]

Prints JSON lines, both from the same run on the same inputs, warm, device events around the library call, the median of
`--repeats` and the spread:
  * {"what": "counts"}:  spadot_cooccur_counts (the zeroing of the output and the counting launch): one pattern;
  * {"what": "null"}:    spadot_cooccur_null with the observed labeling and `--n_perms` relabelings in one call, and
                         `per_pattern_ratio` = null / counts / (1 + n_perms): what the inverse-Feistel gather costs per pattern
                         (1: nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import median, timed  # noqa: E402
from cooccur_time import _prepared, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--domains", type=int, default=12)
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--n_perms", type=int, default=99)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from spadot_amd import stage_ops as ops
    from spadot_amd.cooccurrence import default_radii
    assert torch.cuda.is_available(), "cooccur_null_time measures on the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(1993)
    sets = [synthetic(a.n, a.domains, rng) for _ in range(a.tps)]
    radii = [default_radii(xy, a.bins) for xy, _ in sets]
    shape = f"{a.tps} x {a.n} spots, K = {a.domains}, B = {a.bins}"
    x, desc, pad, K, B, out, desc_dev, pad_dev = prep = _prepared(sets, a.domains, radii, dev)
    counts = median(timed(lambda: ops.cooccur_launch(*prep), a.repeats))
    print(json.dumps(dict(what="counts", shape=shape, **counts)), flush=True)

    desc[:, ops.COOCCUR_DESC_G] = np.arange(a.tps)
    checked = ops.cooccur_null_check(x, desc, pad, K, B, 1, 0, a.n_perms)
    desc_dev = torch.as_tensor(checked[0], device=dev)
    big = torch.empty((a.tps, 1 + a.n_perms, K, K, B), dtype=torch.int64, device=dev)
    null = median(timed(lambda: ops.cooccur_null_launch(x, checked, K, B, 0, big, desc_dev, pad_dev), a.repeats))
    same = bool(torch.equal(big[:, 0], out))
    print(json.dumps(dict(what="null", shape=shape, n_perms=a.n_perms, **null, pattern_0_equals_counts=same,
                          per_pattern_ratio=round(null["median_ms"] / counts["median_ms"] / (1 + a.n_perms), 3))), flush=True)


if __name__ == "__main__":
    main()
