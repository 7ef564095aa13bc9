"""The ligrec stage: which domains signal to which inside a time point, and through which ligand-receptor pair.  The CellPhoneDB
permutation test between the domains of every time point (squidpy's gr.ligrec; csrc/ligrec.hip).  The reference has no
such stage; the definition is restated in numpy in tests/ligrec_ref.py.

    ligrec_sums(dc, values, labels, genes, n_perms)     the device primitive: S and c of every (time point, labeling, gene, domain)
    ligrec_stats(S0, ge, c, sizes, pairs, n_perms, threshold)     the host part: means, pct, the tested cells, pvalue, padj
    ligrec(counts | dc, labels, interactions, n_perms=1000)       the test of every interaction between every pair of domains
    read_interactions(path, genes)                      the pairs of a csv `source,target` as gene indices
    interactions(args)    the stage.  args: data, domains, interactions, output_dir, prefix (''), n_perms (1000), seed (0),
                          threshold (0.1), top (100; 0 = all), device

One time point: n spots with domain labels lab in 0 .. K-1 (K <= 32) and domain sizes n_k, per gene g the fp32 values v of
trends.lognorm_values (0 where nothing is stored) promoted to fp64, and M interactions (src gene, tgt gene).  Labeling 0 is lab;
labeling 1 + p gives spot i the label lab[pi_p(i)], pi_p the permutation of neighbors.py's docstring under (seed, index of the
time point, p, n): one seed means the same relabelings as in neighbors and autocorr.  The device computes, in fp64 and a fixed
order,
    S[l, g, k] = sum of v_r over the stored entries r of gene g with label k under labeling l
and, for labeling 0, the integer c[g, k] = the number of those entries with v > 0.  With w_k = 1 / n_k (0 where n_k = 0):
    mean[g, k] = S[0, g, k] w_k,     pct[g, k] = c[g, k] / n_k,
    stat_l(m, a, b) = 0.5 (S[l, src_m, a] w_a + S[l, tgt_m, b] w_b)
(two products and one sum, each rounded once: numpy reproduces the device's statistic bit for bit from the device's sums).
A cell (m, a, b) is tested iff n_a > 0, n_b > 0, pct[src, a] >= threshold, pct[tgt, b] >= threshold, mean[src, a] > 0 and
mean[tgt, b] > 0.  Tested cells: mean = stat_0 and
    pvalue = (1 + #{p : stat_{1 + p} >= stat_0}) / (P + 1)
(the project's convention; squidpy divides the bare count by P); padj: Benjamini-Hochberg of pvalue over the tested cells of one
time point.  Untested cells: mean = 0 where both domains hold spots and NaN otherwise, pvalue = padj = NaN.  With P = 0 pvalue
and padj are NaN everywhere and only the means are reported.

The device sums and compares; the host validates, masks, adjusts and writes the files.  Only genes named by some interaction are
summed.  Out of scope: complexes and their min rule, interaction databases, restricting to bordering domains, a z-score of the
null, pairs across time points.  Limits: at most 32 domains and 2147483647 spots per time point; permutation indices below 2^32."""
import os
import sys
import time

import numpy as np

from .utils._stage_utils import (cuda_device, labeling_runs, load_marker_counts, open_output, read_domains, savez_pinned, timings,
                                 top_setting, write_timepoints)

FIELDS = ("mean", "pvalue", "padj", "gene_mean", "gene_pct", "sizes", "tested", "ge")
TABLE_COLUMNS = ("source", "target", "domain_source", "domain_target", "mean", "pvalue", "padj", "mean_source", "mean_target",
                 "pct_source", "pct_target")
SUMS_BYTES = 2 ** 30               # the sums of one launch: the labelings are split into runs that share one buffer beyond that


class LigrecResult:
    """One time point: mean, pvalue, padj fp64 [M, K, K] (cell (m, a, b): interaction m from domain a to domain b), gene_mean,
    gene_pct fp64 [G_sel, K] of the selected genes, sizes int64 [K], tested bool [M, K, K], ge int64 [M, K, K] (the permutations
    whose statistic reached the observed one; 0 in untested cells), sources, targets (gene names per interaction), genes (the
    selected genes' names), pairs int64 [M, 2] (positions in `genes`)."""

    def __init__(self, stats, sizes, ge, pairs, genes):
        for name, v in stats.items():
            setattr(self, name, v)
        self.sizes, self.ge, self.pairs, self.genes = np.asarray(sizes, dtype=np.int64), ge, pairs, genes
        self.sources, self.targets = genes[pairs[:, 0]], genes[pairs[:, 1]]


def _tested(S0, c, sizes, pairs, threshold):
    """gene_mean, gene_pct [G_sel, K], w [K], stat_0 and tested [M, K, K] of one time point (module docstring)."""
    S0, c = np.asarray(S0, dtype=np.float64), np.asarray(c, dtype=np.float64)
    nk = np.asarray(sizes, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    with np.errstate(divide="ignore"):
        w = np.where(nk > 0, 1.0 / np.where(nk > 0, nk, 1.0), 0.0)
    mean = S0 * w[None, :]
    pct = np.where(nk[None, :] > 0, c / np.where(nk > 0, nk, 1.0)[None, :], 0.0)
    src, tgt = pairs[:, 0], pairs[:, 1]
    stat0 = 0.5 * (mean[src][:, :, None] + mean[tgt][:, None, :])
    held = (nk[:, None] > 0) & (nk[None, :] > 0)
    ok = (pct >= threshold) & (mean > 0)
    tested = held[None] & ok[src][:, :, None] & ok[tgt][:, None, :]
    return mean, pct, w, stat0, tested, held


def ligrec_stats(S0, ge, c, sizes, pairs, n_perms, threshold):
    """The host part of one time point (module docstring).  S0 fp64 [G_sel, K]: the sums of labeling 0; ge [M, K, K]: the
    permutations whose statistic reached the observed one (None with n_perms = 0); c [G_sel, K]; sizes [K]; pairs [M, 2]:
    positions in the selected genes.  Returns a dict: mean, pvalue, padj fp64 [M, K, K], tested bool [M, K, K], gene_mean,
    gene_pct fp64 [G_sel, K]."""
    from .markers import bh_adjust
    mean, pct, _, stat0, tested, held = _tested(S0, c, sizes, pairs, threshold)
    n_perms = int(n_perms)
    out_mean = np.where(tested, stat0, np.where(held[None], 0.0, np.nan))
    pvalue, padj = np.full(stat0.shape, np.nan), np.full(stat0.shape, np.nan)
    if n_perms >= 1:
        pvalue[tested] = (1.0 + np.asarray(ge)[tested]) / (n_perms + 1.0)
        padj[tested] = bh_adjust(pvalue[tested])
    return dict(mean=out_mean, pvalue=pvalue, padj=padj, tested=tested, gene_mean=mean, gene_pct=pct)


def _device_args(dc, values, labels, genes, K):
    """The prepared tensors of a launch: (colptr, ridx, values, labels uint8, genes int32), desc int64 [T, 3] and K."""
    import torch
    from . import stage_ops as ops
    if not isinstance(values, torch.Tensor):
        raise RuntimeError("ligrec_sums takes the values as a device tensor (torch), not a host array")
    dev = dc.device
    if isinstance(labels, torch.Tensor):
        if not labels.is_cuda:
            raise RuntimeError("spadot_amd ops run on the MI355X only (got a CPU tensor); there is no CPU path")
        if K is None:
            K = int(labels.max().item()) + 1 if labels.numel() else 1
    else:
        labels = np.asarray(labels)
        if labels.dtype.kind not in "iu" or labels.ndim != 1:
            raise ValueError("labels must be one integer domain id per row")
        lo, hi = (int(labels.min()), int(labels.max())) if labels.size else (0, 0)
        if lo < 0 or hi > 255:
            raise ValueError(f"labels holds the labels {lo} .. {hi}: labels must lie in 0 .. {ops.LIGREC_MAX_K - 1}")
        if K is None:
            K = hi + 1
        labels = torch.as_tensor(labels.astype(np.uint8), device=dev)
    if not isinstance(genes, torch.Tensor):
        genes = torch.as_tensor(np.asarray(genes, dtype=np.int64).reshape(-1), device=dev)
    if genes.dtype != torch.int32:                           # a gene outside int32 stays outside the genes: refused by the check
        genes = genes.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    off = np.asarray(dc.tp_off_host, dtype=np.int64)
    T = int(dc.T)
    desc = np.stack([off[1:] - off[:-1], off[:-1], np.arange(T, dtype=np.int64)], axis=1)
    return (dc.colptr, dc.ridx, values, labels.contiguous(), genes.contiguous()), desc, int(K)


def ligrec_sums(dc, values, labels, genes, n_perms, seed=0, first=0, observed=True, lds_limit=None, gene_chunk=None, out=None,
                threads=None, K=None):
    """S and c of every (time point, labeling, selected gene, domain) (module docstring).  dc: a DeviceCounts (its colptr, ridx,
    tp_off); values: fp32 device tensor, one per stored entry in CSC order; labels: one domain id per row of dc (its row order),
    integers on the host or a uint8 device tensor; genes: the selected genes, any order, repeats allowed.  Labelings: lab itself
    first (observed), then the permutations first .. first + n_perms - 1 under seed, time point t as graph index t.  K: the label
    values (default: the largest label + 1).  lds_limit: the LDS bytes a workgroup may use (default 163840): a time point whose
    labels do not fit beside the accumulators permutes per stored entry, with the same bits.  gene_chunk, threads: the selected
    genes per workgroup and its size (defaults of the library).  One launch (several only where the sums of all labelings would
    pass 1 GiB).  Returns (S, c): [t] -> fp64 numpy [labelings, genes, K] and [t] -> int32 numpy [genes, K] (None without the
    observed labeling).  ValueError / RuntimeError before any launch; out: a pair of device tensors (fp64 [T, labelings, genes,
    K], int32 [T, genes, K]) to write into."""
    import torch
    from . import stage_ops as ops
    n_perms, first, observed = int(n_perms), int(first), bool(observed)
    if n_perms < 0:
        raise ValueError(f"the number of permutations must not be negative (got n_perms = {n_perms})")
    with torch.cuda.device(dc.device):
        args, desc, K = _device_args(dc, values, labels, genes, K)
        checked = ops.ligrec_check(*args, desc, K, observed, first, n_perms, gene_chunk)
        T, ng, L = int(dc.T), int(args[4].numel()), int(observed) + n_perms
        runs = labeling_runs(n_perms, observed, first, 8 * T * ng * K, SUMS_BYTES)
        if len(runs) == 1:
            S, c = ops.ligrec_launch(*args, checked, K, observed, first, n_perms, seed, lds_limit, out, threads, gene_chunk)
            S, c = S.reshape(T, L, ng, K).cpu().numpy(), (c.reshape(T, ng, K).cpu().numpy() if observed else None)
        else:                                                # the labelings in runs that share one buffer
            if out is not None:
                raise ValueError("out is taken only by a call that is one launch")
            buf = torch.empty(T * (runs[0][0] + runs[0][2]) * ng * K, dtype=torch.float64, device=dc.device)
            cnt = torch.empty((T, ng, K), dtype=torch.int32, device=dc.device) if observed else None
            parts, c = [], None
            for obs, p0, n in runs:
                view = buf[:T * (obs + n) * ng * K].view(T, obs + n, ng, K)
                ops.ligrec_launch(*args, checked, K, obs, p0, n, seed, lds_limit, (view, cnt if obs else None), threads,
                                  gene_chunk)
                parts.append(view.to("cpu", copy=True).numpy())
                if obs:
                    c = cnt.cpu().numpy()
            S = np.concatenate(parts, axis=1)
    return [S[t] for t in range(T)], ([c[t] for t in range(T)] if observed else None)


def _pairs(interactions, genes):
    """interactions as int64 [M, 2] gene indices: an integer array [M, 2], or pairs of gene names looked up in `genes`."""
    arr = np.asarray(interactions)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.shape[0] < 1:
        raise ValueError(f"interactions must be M >= 1 pairs (source gene, target gene) (got an array of shape {arr.shape})")
    if arr.dtype.kind in "iu":
        if arr.min() < 0 or arr.max() >= len(genes):
            raise ValueError(f"the interactions name the genes {int(arr.min())} .. {int(arr.max())}: the data has the genes 0 .. "
                             f"{len(genes) - 1}")
        return arr.astype(np.int64)
    pos = {g: i for i, g in enumerate(np.asarray(genes).astype(str).tolist())}
    missing = sorted({g for g in arr.astype(str).reshape(-1).tolist() if g not in pos})
    if missing:
        raise ValueError(f"the interactions name genes that the data does not have: {missing[:5]} ({len(missing)} genes)")
    return np.asarray([[pos[s], pos[t]] for s, t in arr.astype(str).tolist()], dtype=np.int64)


def ligrec(counts, labels, interactions, n_perms=1000, seed=0, threshold=0.1, device="cuda:0", values=None, lds_limit=None,
           gene_chunk=None, threads=None, timings=None):
    """The permutation test of every interaction between every ordered pair of domains of every time point (module docstring).
    counts: a DeviceCounts, or anything load_counts accepts in memory; labels: one non-negative domain id per row of the input
    data (a domain inside the row's time point); interactions: int [M, 2] gene indices or pairs of gene names (read_interactions);
    values: the fp32 values of a DeviceCounts in CSC order (default: trends.lognorm_values).
    The sums of all labelings of all time points are one launch and the comparisons another (several runs of the two only where
    the sums would pass 1 GiB); the observed sums come to the host once, for the mask.  Returns [t] -> LigrecResult, its arrays
    [M, K_t, K_t] with K_t the domains of the time point.  timings: a dict that receives the device milliseconds of the
    launches."""
    import torch
    from . import stage_ops as ops
    from .markers import check_labels
    from .preprocess import DeviceCounts
    from .trends import lognorm_values
    from .utils._preprocess_utils import RawCounts, load_counts
    n_perms, threshold = int(n_perms), float(threshold)
    if n_perms < 0 or not 0.0 <= threshold <= 1.0:
        raise ValueError(f"ligrec takes n_perms >= 0 and 0 <= threshold <= 1 (got n_perms = {n_perms}, threshold = {threshold})")
    if hasattr(counts, "colptr"):
        dc = counts
    else:
        if torch.device(device).type != "cuda":
            raise RuntimeError("spadot_amd takes the ligand-receptor test on the MI355X only (device 'cuda:N'); there is no CPU "
                               "path")
        dc = DeviceCounts(counts if isinstance(counts, RawCounts) else load_counts(counts)[0], device)
    perm = np.asarray(dc.perm)
    tp_in = np.empty(dc.n, dtype=np.asarray(dc.timepoint).dtype)
    tp_in[perm] = np.asarray(dc.timepoint)
    lab, tps, ks = check_labels(labels, tp_in)
    if [str(a) for a in dc.tps] != [str(a) for a in tps]:
        raise ValueError(f"the labels' time points {[str(a) for a in tps]} are not the data's {[str(a) for a in dc.tps]}")
    lab = lab[perm]
    gene_names = np.asarray(dc.genes).astype(str)
    pairs_abs = _pairs(interactions, gene_names)
    sel, pos = np.unique(pairs_abs.reshape(-1), return_inverse=True)
    pairs = pos.reshape(-1, 2).astype(np.int64)
    T, K, M, ns = int(dc.T), max(ks), int(pairs.shape[0]), int(sel.shape[0])
    off = np.asarray(dc.tp_off_host, dtype=np.int64)
    sizes = np.stack([np.bincount(lab[off[t]:off[t + 1]], minlength=K) for t in range(T)]).astype(np.int64)
    ev = []

    def stamp():
        ev.append(torch.cuda.Event(enable_timing=True))
        ev[-1].record()

    with torch.cuda.device(dc.device):
        if values is None:
            values = lognorm_values(dc)
        args, desc, K = _device_args(dc, values, lab, sel, K)
        checked = ops.ligrec_check(*args, desc, K, True, 0, n_perms, gene_chunk)
        dev = dc.device
        runs = labeling_runs(n_perms, True, 0, 8 * T * ns * K, SUMS_BYTES)
        buf = torch.empty(T * (runs[0][0] + runs[0][2]) * ns * K, dtype=torch.float64, device=dev)
        cnt = torch.empty((T, ns, K), dtype=torch.int32, device=dev)
        ge = torch.zeros((T, M, K, K), dtype=torch.int32, device=dev)
        pairs_dev = torch.as_tensor(pairs.astype(np.int32), device=dev)
        S0 = wk = mask = None
        for obs, p0, n in runs:
            view = buf[:T * (obs + n) * ns * K].view(T, obs + n, ns, K)
            stamp()
            ops.ligrec_launch(*args, checked, K, obs, p0, n, seed, lds_limit, (view, cnt if obs else None), threads, gene_chunk)
            stamp()
            if obs:                                          # the observed sums, once: the mask is the host's
                S0 = view[:, 0].clone()                      # its own buffer: the runs after this one reuse `buf`
                S0_host, c_host = S0.cpu().numpy(), cnt.cpu().numpy()
                parts = [_tested(S0_host[t], c_host[t], sizes[t], pairs, threshold) for t in range(T)]
                wk = torch.as_tensor(np.stack([p[2] for p in parts]), device=dev)
                mask = torch.as_tensor(np.stack([p[4] for p in parts]).astype(np.uint8), device=dev)
            if n > 0:
                stamp()
                ops.ligrec_count(S0, view, wk, pairs_dev, (int(pairs.min()), int(pairs.max())), mask, int(obs), ge)
                stamp()
        ge_host = ge.cpu().numpy().astype(np.int64)
    if timings is not None:
        timings["launch_ms"] = [ev[i].elapsed_time(ev[i + 1]) for i in range(0, len(ev), 2)]
    names = gene_names[sel]
    res = []
    for t, Kt in enumerate(ks):
        st = ligrec_stats(S0_host[t][:, :Kt], ge_host[t][:, :Kt, :Kt], c_host[t][:, :Kt], sizes[t][:Kt], pairs, n_perms, threshold)
        res.append(LigrecResult(st, sizes[t][:Kt], ge_host[t][:, :Kt, :Kt].copy(), pairs, names))
    return res


def read_interactions(path, genes):
    """The interactions of a csv with the header `source,target` (gene names, case-sensitive) as int64 [M, 2] indices into
    `genes`.  An exact duplicate pair is dropped (the first occurrence is kept), a pair with a gene missing from the data is
    dropped; the number of dropped pairs goes to stderr.  ValueError for a table without the two columns or without a pair
    left."""
    import pandas as pd
    df = pd.read_csv(path, dtype=str, keep_default_na=False) if isinstance(path, (str, os.PathLike)) else path
    for col in ("source", "target"):
        if col not in df.columns:
            raise ValueError(f"the interactions table has no `{col}` column (expected a csv with the header source,target)")
    pos = {g: i for i, g in enumerate(np.asarray(genes).astype(str).tolist())}
    seen, out, dup, missing = set(), [], 0, 0
    for s, t in zip(df["source"].astype(str).tolist(), df["target"].astype(str).tolist()):
        if (s, t) in seen:
            dup += 1
            continue
        seen.add((s, t))
        if s not in pos or t not in pos:
            missing += 1
            continue
        out.append((pos[s], pos[t]))
    if dup or missing:
        print(f"ligrec: dropped {dup + missing} of {len(df)} interactions ({dup} duplicates, {missing} with a gene that the data "
              f"does not have)", file=sys.stderr)
    if not out:
        raise ValueError(f"no interaction is left: none of the {len(df)} pairs names two genes of the data")
    return np.asarray(out, dtype=np.int64)


def ligrec_table(r, top=100):
    """The rows of {prefix}ligrec_{tp}.csv: the tested cells by ascending pvalue, then descending mean, then interaction,
    source domain, target domain; the first `top` of them (0 = all)."""
    import pandas as pd
    m, a, b = np.nonzero(r.tested)
    p = np.where(np.isnan(r.pvalue[m, a, b]), 0.0, r.pvalue[m, a, b])
    order = np.lexsort((b, a, m, -r.mean[m, a, b], p))
    if top:
        order = order[:top]
    m, a, b = m[order], a[order], b[order]
    src, tgt = r.pairs[m, 0], r.pairs[m, 1]
    return pd.DataFrame({"source": r.sources[m], "target": r.targets[m], "domain_source": a, "domain_target": b,
                         "mean": r.mean[m, a, b], "pvalue": r.pvalue[m, a, b], "padj": r.padj[m, a, b],
                         "mean_source": r.gene_mean[src, a], "mean_target": r.gene_mean[tgt, b],
                         "pct_source": r.gene_pct[src, a], "pct_target": r.gene_pct[tgt, b]}, columns=list(TABLE_COLUMNS))


def interactions(args):
    """Reads args.data (counts) and args.domains as the markers stage does and args.interactions (read_interactions), and runs
    one ligrec call.  Writes {prefix}ligrec_{tp}.csv (TABLE_COLUMNS; the tested cells, args.top rows, 0 = all) and
    {prefix}ligrec.npz ('{tp}_{field}' for FIELDS, plus sources, targets, genes, timepoints, n_perms, seed, threshold; pinned time
    stamps: two runs with one seed write the same bytes).  Returns {'tables', 'results' (per time point), 'timepoints',
    'timings'}."""
    import torch
    from .preprocess import DeviceCounts
    t_start = time.perf_counter()
    top = top_setting(args, 100)
    n_perms, seed = int(getattr(args, "n_perms", 1000)), int(getattr(args, "seed", 0))
    threshold = float(getattr(args, "threshold", 0.1))
    if top < 0 or n_perms < 0 or not 0.0 <= threshold <= 1.0:
        raise ValueError(f"the ligrec stage takes top >= 0, n_perms >= 0 and 0 <= threshold <= 1 (got top = {top}, n_perms = "
                         f"{n_perms}, threshold = {threshold})")
    dev = cuda_device(args, "takes the ligand-receptor test")
    if not getattr(args, "domains", None):
        raise ValueError("the ligrec stage needs the domains table of analyze (--domains)")
    if not getattr(args, "interactions", None):
        raise ValueError("the ligrec stage needs a csv of ligand-receptor pairs with the header source,target (--interactions)")
    raw, path = load_marker_counts(args.data)
    labels = read_domains(args.domains, raw.obs["timepoint"])
    pairs = read_interactions(args.interactions, raw.var_names)
    out_file = open_output(args, path)
    dc = DeviceCounts(raw, dev)
    tps = [str(t) for t in dc.tps]
    t_read = time.perf_counter()
    res = ligrec(dc, labels, pairs, n_perms=n_perms, seed=seed, threshold=threshold)
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter()
    arrays = dict(sources=res[0].sources, targets=res[0].targets, genes=res[0].genes, timepoints=np.asarray(tps),
                  n_perms=np.int64(n_perms), seed=np.int64(seed), threshold=np.float64(threshold))
    tables, arrays = write_timepoints(out_file, "ligrec", tps, res, lambda t, r: ligrec_table(r, top), FIELDS, arrays)
    savez_pinned(out_file("ligrec.npz"), arrays)
    t_end = time.perf_counter()
    print(f"ligrec: {pairs.shape[0]} interactions over {res[0].genes.shape[0]} genes x {dc.n} spots of {dc.T} time points, "
          f"{n_perms} permutations, written to {args.output_dir}", file=sys.stderr)
    return {"tables": tables, "results": dict(zip(tps, res)), "timepoints": tps, "timings": timings(t_start, t_read, t_dev, t_end)}
