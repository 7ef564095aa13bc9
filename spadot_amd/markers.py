"""The markers stage: which genes mark each spatial domain.  Per (time point, domain, gene) a Wilcoxon rank-sum test of the
domain's spots against the rest of the time point on the MI355X (csrc/markers.hip).  The reference has no such stage;
the definition is scipy.stats.mannwhitneyu(x_in, x_out, alternative='two-sided', method='asymptotic', use_continuity=True) on
v = float32(log1p(count * 1e4 / row_total)), all spots of a time point ranked together with average ranks.

    find_markers(counts, labels, device='cuda:0')    the arrays
    markers(args)    args: data, domains ({prefix}domains.csv of analyze), output_dir, prefix (''), top (100; 0 = all), device

Per (time point t, gene g, domain k), with n1 the domain's size, n2 = n - n1, R the domain's rank sum and Ties the sum of
t^3 - t over the tie runs (the zeros included):
    U1 = R - n1 (n1 + 1) / 2,  d = U1 - n1 n2 / 2,  var = n1 n2 ((n + 1) n (n - 1) - Ties) / (12 n (n - 1)),
    score = (d - sign(d) / 2) / sqrt(var),  pval = min(1, erfc(|score| / sqrt 2)),
and score = 0, pval = 1 where var <= 0, n1 = 0, n2 = 0 or d = 0 (scipy: NaN or a clipped 1).  Also mean_in / mean_out (means
of v), pct_in / pct_out (share of spots with v > 0), log2fc = log2((expm1(mean_in) + 1e-9) / (expm1(mean_out) + 1e-9)) (scanpy's
form), auc = U1 / (n1 n2) and padj: Benjamini-Hochberg within one (time point, domain) over the genes with a nonzero in that
time point (the others: score 0, pval = padj = 1).

The device ranks; the host does the plumbing (row permutation, CSR -> CSC, domain sizes, means from the device's sums, BH,
ordering and the files)."""
import sys
import time

import numpy as np

from ._call import launched, ptr as _p, stream as _stream
from .utils._preprocess_utils import RawCounts, load_counts, timepoint_order
from .utils._stage_utils import load_marker_counts, read_domains  # noqa: F401  (handed on: they were first written for this stage)
from .utils._stage_utils import open_output, top_setting

TARGET_SUM = 1e4
MAX_DOMAINS = 32               # the cap of analyze; the kernel's accumulators are sized for it
MAX_SPOTS = 2097151            # per time point: n^3 < 2^63
COLUMNS = ("score", "pval", "padj", "log2fc", "mean_in", "mean_out", "pct_in", "pct_out", "auc")
CSV_COLUMNS = ("gene", "domain") + COLUMNS


def bh_adjust(p):
    """Benjamini-Hochberg adjusted p-values (step-up, capped at 1)."""
    p = np.asarray(p, dtype=np.float64)
    m = p.size
    if m == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    adj = np.minimum.accumulate((p[order] * m / np.arange(1, m + 1))[::-1])[::-1]
    out = np.empty(m, dtype=np.float64)
    out[order] = np.minimum(adj, 1.0)
    return out


def check_labels(labels, timepoint):
    """labels: one non-negative integer per row, the domain inside the row's time point.  Returns (int32 labels, the time
    points in order of first appearance, the domain count of each).  ValueError on anything else, before device work."""
    tp = np.asarray(timepoint)
    if tp.dtype == object:
        tp = tp.astype(str)
    lab = np.asarray(labels)
    if lab.shape != tp.shape:
        raise ValueError(f"labels must hold one domain per row: {tp.shape[0]} rows, labels of shape {lab.shape}")
    if lab.dtype.kind not in "iu":
        if lab.dtype.kind != "f" or not np.all(np.isfinite(lab)) or np.any(lab != np.floor(lab)):
            raise ValueError("labels must be integers (a domain id per row)")
    if lab.size and lab.min() < 0:
        raise ValueError("labels must be non-negative domain ids")
    lab = lab.astype(np.int64)
    tps = timepoint_order(tp)
    ks = [int(lab[tp == t].max()) + 1 for t in tps]
    for t, k in zip(tps, ks):
        if k > MAX_DOMAINS:
            raise ValueError(f"time point {t} has {k} domains: the markers stage takes at most {MAX_DOMAINS} per time point")
    return lab.astype(np.int32), tps, ks


def _check(rc, name):
    if rc == -7:
        raise ValueError(f"{name}: more than {MAX_DOMAINS} domains or more than {MAX_SPOTS} spots in a time point")
    launched(rc, name)


class MarkerKernels:
    """The three launches on a DeviceCounts.  labels: int32 per permuted row, K: the widest time point's domain count."""

    def __init__(self, dc, labels, K):
        import torch
        from ._lib import model_lib
        self.dc, self.K, self.lib = dc, int(K), model_lib()
        sizes = np.diff(dc.tp_off_host)
        self.nmax = int(sizes.max())
        if self.K > MAX_DOMAINS:
            raise ValueError(f"{self.K} domains: the markers stage takes at most {MAX_DOMAINS} per time point")
        if self.nmax > MAX_SPOTS:
            raise ValueError(f"a time point has {self.nmax} spots: the markers stage takes at most {MAX_SPOTS}")
        nk = np.zeros((dc.T, self.K), dtype=np.int32)
        for t in range(dc.T):
            lo, hi = dc.tp_off_host[t], dc.tp_off_host[t + 1]
            nk[t] = np.bincount(labels[lo:hi], minlength=self.K)[:self.K]
        self.nk_host = nk
        d = dc.device
        self.nk = torch.as_tensor(nk, device=d)
        self.labels = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.int32), device=d)
        self.nnz = int(dc.cval.numel())
        self.cap = int(self.lib.spadot_mk_lds_capacity())
        nbytes = int(self.lib.spadot_mk_ranksum_scratch_bytes(dc.T, dc.G, self.nmax))
        if nbytes < 0:
            _check(nbytes, "spadot_mk_ranksum_scratch_bytes")
        self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=d)
        T, G, K = dc.T, dc.G, self.K
        self.values = torch.empty(self.nnz, dtype=torch.float32, device=d)
        self.r2 = torch.zeros((T, G, K), dtype=torch.int64, device=d)
        self.ties = torch.zeros((T, G), dtype=torch.int64, device=d)
        self.nnz_k = torch.zeros((T, G, K), dtype=torch.int32, device=d)
        self.vsum = torch.zeros((T, G, K), dtype=torch.float64, device=d)
        self.u1 = torch.empty((T, G, K), dtype=torch.float64, device=d)
        self.score = torch.empty((T, G, K), dtype=torch.float64, device=d)
        self.pval = torch.empty((T, G, K), dtype=torch.float64, device=d)
        self.total = None

    def row_totals(self):
        import torch
        mask = torch.ones((self.dc.T, self.dc.G), dtype=torch.uint8, device=self.dc.device)
        self.total = self.dc.row_total(mask)
        return self.total

    def lognorm(self):
        dc = self.dc
        _check(self.lib.spadot_mk_lognorm(_p(dc.ridx), _p(dc.cval), _p(self.total), self.nnz, TARGET_SUM, _p(self.values),
                                          _stream()), "spadot_mk_lognorm")

    def ranksum(self):
        dc = self.dc
        _check(self.lib.spadot_mk_ranksum(_p(dc.colptr), _p(dc.ridx), _p(self.values), _p(dc.tp_off), _p(self.labels),
                                          _p(self.nk), dc.T, dc.G, self.K, self.nmax, _p(self.scratch),
                                          int(self.scratch.numel()), _p(self.r2), _p(self.ties), _p(self.nnz_k), _p(self.vsum),
                                          _stream()), "spadot_mk_ranksum")

    def finish(self):
        dc = self.dc
        _check(self.lib.spadot_mk_finish(_p(self.r2), _p(self.ties), _p(dc.tp_off), _p(self.nk), dc.T, dc.G, self.K,
                                         _p(self.u1), _p(self.score), _p(self.pval), _stream()), "spadot_mk_finish")


def find_markers(counts, labels, device="cuda:0"):
    """Rank-sum tests of every (time point, gene, domain).  counts: anything load_counts accepts in memory (.X, .obs['timepoint'],
    .obsm['spatial'], optionally .var_names); labels: one non-negative int per row, a domain id within the row's time point.

    Returns a dict.  Lists with one entry per time point (in order of first appearance, `timepoints`): score, pval, padj,
    log2fc, mean_in, mean_out, pct_in, pct_out, auc, U1, vsum (fp64 [G, K_t]), r2 (int64 [G, K_t], TWICE the rank sums), nnz_k
    (int32 [G, K_t]), ties (int64 [G]), n_k (int64 [K_t]).  `values`: the fp32 v the device ranked, in the CSC order of the
    permuted rows (`colptr`, `ridx`, `perm`: input row of each permuted row, `tp_off`).  `genes`, `timings` (seconds; the
    three kernels in device milliseconds)."""
    import torch
    from .preprocess import DeviceCounts
    if torch.device(device).type != "cuda":
        raise ValueError(f"the markers stage runs on the MI355X (a cuda device), not on {device!r}")
    t_start = time.perf_counter()
    raw = counts if isinstance(counts, RawCounts) else load_counts(counts)[0]
    lab, tps, ks = check_labels(labels, raw.obs["timepoint"])
    dc = DeviceCounts(raw, device)
    assert [str(a) for a in dc.tps] == [str(a) for a in tps]
    mk = MarkerKernels(dc, lab[dc.perm], max(ks))
    torch.cuda.synchronize(dc.device)
    t_up = time.perf_counter()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    with torch.cuda.device(dc.device):
        ev[0].record()
        mk.row_totals()
        ev[1].record()
        mk.lognorm()
        ev[2].record()
        mk.ranksum()
        ev[3].record()
        mk.finish()
        ev[4].record()
        ev[4].synchronize()
    t_dev = time.perf_counter()
    r2, ties, nnz_k, vsum, u1, score, pval = (x.cpu().numpy() for x in (mk.r2, mk.ties, mk.nnz_k, mk.vsum, mk.u1, mk.score,
                                                                        mk.pval))
    out = {c: [] for c in COLUMNS + ("U1", "vsum", "r2", "nnz_k", "ties", "n_k")}
    for t, K in enumerate(ks):
        n = float(dc.tp_off_host[t + 1] - dc.tp_off_host[t])
        n1 = mk.nk_host[t, :K].astype(np.float64)[None, :]
        n2 = n - n1
        s_in, c_in = vsum[t, :, :K], nnz_k[t, :, :K].astype(np.float64)
        s_all, c_all = vsum[t].sum(1, keepdims=True), nnz_k[t].astype(np.float64).sum(1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean_in = np.where(n1 > 0, s_in / n1, 0.0)
            mean_out = np.where(n2 > 0, (s_all - s_in) / n2, 0.0)
            pct_in = np.where(n1 > 0, c_in / n1, 0.0)
            pct_out = np.where(n2 > 0, (c_all - c_in) / n2, 0.0)
            auc = np.where(n1 * n2 > 0, u1[t, :, :K] / (n1 * n2), 0.5)
        expressed = c_all[:, 0] > 0
        padj = np.ones_like(pval[t, :, :K])
        for k in range(K):
            padj[expressed, k] = bh_adjust(pval[t, expressed, k])
        out["score"].append(score[t, :, :K].copy()); out["pval"].append(pval[t, :, :K].copy()); out["padj"].append(padj)
        out["log2fc"].append(np.log2((np.expm1(mean_in) + 1e-9) / (np.expm1(mean_out) + 1e-9)))
        out["mean_in"].append(mean_in); out["mean_out"].append(mean_out)
        out["pct_in"].append(pct_in); out["pct_out"].append(pct_out); out["auc"].append(auc)
        out["U1"].append(u1[t, :, :K].copy()); out["vsum"].append(s_in.copy()); out["r2"].append(r2[t, :, :K].copy())
        out["nnz_k"].append(nnz_k[t, :, :K].copy()); out["ties"].append(ties[t].copy())
        out["n_k"].append(mk.nk_host[t, :K].astype(np.int64))
    t_end = time.perf_counter()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]
    out.update(values=mk.values.cpu().numpy(), colptr=dc.colptr.cpu().numpy(), ridx=dc.ridx.cpu().numpy(), perm=dc.perm,
               tp_off=dc.tp_off_host.astype(np.int64), genes=dc.genes, timepoints=list(dc.tps),
               timings=dict(upload_s=t_up - t_start, device_s=t_dev - t_up, host_s=t_end - t_dev, total_s=t_end - t_start,
                            row_total_ms=ms[0], lognorm_ms=ms[1], ranksum_ms=ms[2], finish_ms=ms[3],
                            long_segments=int(mk.scratch[:4].view(torch.int32).item()), lds_capacity=mk.cap))
    return out


def marker_table(res, t, top=100):
    """The rows of {prefix}markers_{tp}.csv: per domain the `top` highest scores (0 = all), ordered by domain, then score
    descending, then gene column."""
    import pandas as pd
    score = res["score"][t]
    G, K = score.shape
    frames = []
    for k in range(K):
        order = np.lexsort((np.arange(G), -score[:, k]))
        if top:
            order = order[:top]
        cols = {"gene": np.asarray(res["genes"])[order], "domain": np.full(order.size, k, dtype=np.int64)}
        cols.update({c: res[c][t][order, k] for c in COLUMNS})
        frames.append(pd.DataFrame(cols, columns=list(CSV_COLUMNS)))
    return pd.concat(frames, ignore_index=True) if frames else pd.DataFrame(columns=list(CSV_COLUMNS))


def markers(args):
    """Reads args.data (counts) and args.domains (the domains.csv of analyze), writes {prefix}markers_{tp}.csv per time point
    and {prefix}markers.npz (per time point t: score_t, pval_t, ... [G, K_t]; genes, timepoints, domains '<tp>_<domain>').
    Returns the dict of find_markers."""
    raw, path = load_marker_counts(args.data)
    if not getattr(args, "domains", None):
        raise ValueError("the markers stage needs the domains table of analyze (--domains)")
    labels = read_domains(args.domains, raw.obs["timepoint"])
    out_file = open_output(args, path)
    top = top_setting(args, 100, least=0)
    res = find_markers(raw, labels, device=getattr(args, "device", None) or "cuda:0")
    arrays = dict(genes=np.asarray(res["genes"]).astype(str), timepoints=np.asarray([str(t) for t in res["timepoints"]]))
    names = []
    for t, tp in enumerate(res["timepoints"]):
        marker_table(res, t, top).to_csv(out_file(f"markers_{tp}.csv"), index=False)
        for c in COLUMNS + ("U1",):
            arrays[f"{c}_{t}"] = res[c][t]
        names += [f"{tp}_{k}" for k in range(res["score"][t].shape[1])]
    arrays["domains"] = np.asarray(names)
    np.savez(out_file("markers.npz"), **arrays)
    print(f"markers: {len(names)} domains x {len(res['genes'])} genes written to {args.output_dir}", file=sys.stderr)
    return res
