"""The trends stage: which genes change along the lineage of a domain, and which genes go with a fate.  Both read the outputs of
`analyze --lineage` (trajectories.npz: per domain a probability vector over the spots of every time point; fates.npz: per spot
the share of its mass that ends in each final domain) against v = float32(log1p(count * 1e4 / row_total)), the values of the
markers stage.  The reference has no such stage; the definitions are this project's (Waddington-OT's trajectory_trends and
CellRank's lineage drivers are the ideas), pinned to numpy.average and scipy.stats.pearsonr (tests/trends_ref.py).

    weighted_moments(dc, values, W)                 the device primitive: S0, S1, S2 [T, G, C] (csrc/trends.hip)
    lognorm_values(dc)                              the fp32 v of a DeviceCounts, in CSC order
    gene_trends(counts, W, names=None, device=)     weighted mean expression of every gene under every column of W
    fate_drivers(counts, F, names=None, device=)    Pearson correlation of every gene with every fate
    trends(args)    args: data, trajectories and / or fates, output_dir, prefix (''), top (100; 0 = all), device

The primitive: over the stored entries (i, g) of the counts whose row i lies in time point t,
    S0[t,g,c] = sum W[i,c],   S1[t,g,c] = sum v_ig W[i,c],   S2[t,g,c] = sum v_ig^2 W[i,c]        (fp64, a fixed order).

gene_trends, per (time point t, gene g, column c) with s = sum of W[i,c] over the spots of t:
    mean = S1 / s,  var = max(S2 / s - mean^2, 0),  pct = S0 / s,  all NaN where s = 0,
    baseline[t,g] = the unweighted mean of v over the time point,  delta = mean - baseline,
    change[g,c] = mean[last t with s > 0] - mean[first t with s > 0]  (NaN where no time point has s > 0).
pct is the weighted share of the spots where the gene has a STORED count: load_counts drops explicit zeros, and no positive count
has a v that rounds to 0, so this is the share with v > 0 unless the caller hands over a sparse matrix with stored zeros.

fate_drivers, per (time point t, gene g, fate k) over the valid spots of t (F's row sum nonzero; n' of them; u their 0/1
indicator, Fbar_k the mean of F_.k over them, Wc = u (F - Fbar)): the device is called with [Wc | u], so
    M1 = S1[u],  M2 = S2[u],  cov_k = S1[k],  SSv = M2 - M1^2 / n',  SSF_k = sum Wc[i,k]^2,
    r = clip(cov_k / sqrt(SSv SSF_k), -1, 1),  t = r sqrt((n' - 2) / ((1 - r)(1 + r))),  p = 2 stdtr(n' - 2, -|t|),
and r = 0, p = 1 where n' < 3, SSF_k <= 0 or SSv <= n' 2^-50 M2 (eight times the first-order rounding bound of the raw-moment
form: the variance is not distinguishable from zero; scipy returns NaN there).  padj: Benjamini-Hochberg within one (time
point, fate) over the genes with a nonzero among the valid spots (the others: r = 0, p = padj = 1).

The device sums; the host does the plumbing (row matching, centring, the t distribution, BH, ordering and the files)."""
import sys
import time

import numpy as np

from ._call import launched, ptr as _p, stream as _stream
from .markers import TARGET_SUM, bh_adjust
from .utils._preprocess_utils import RawCounts, load_counts
from .utils._stage_utils import align_rows, load_marker_counts, open_output, top_setting

MAX_COLUMNS = 1024             # columns of W in one call (the kernel keeps 16 per lane)
MAX_ROWS = 2 ** 31 - 1
TREND_KEYS = ("mean", "var", "pct", "delta", "baseline", "change")
DRIVER_KEYS = ("r", "pval", "padj", "n_valid")
DRIVER_COLUMNS = ("gene", "fate", "r", "pval", "padj")


def _check(rc, name):
    if rc == -7:
        raise ValueError(f"{name}: W must have 1 .. {MAX_COLUMNS} columns and at most {MAX_ROWS} rows")
    launched(rc, name)


def lognorm_values(dc):
    """fp32 v = log1p(count * 1e4 / row_total) of every stored entry of a DeviceCounts, in CSC order (row total over all genes)."""
    import torch
    from ._lib import model_lib
    mask = torch.ones((dc.T, dc.G), dtype=torch.uint8, device=dc.device)
    total = dc.row_total(mask)
    nnz = int(dc.cval.numel())
    values = torch.empty(nnz, dtype=torch.float32, device=dc.device)
    launched(model_lib().spadot_mk_lognorm(_p(dc.ridx), _p(dc.cval), _p(total), nnz, TARGET_SUM, _p(values), _stream()),
             "spadot_mk_lognorm")
    return values


def weighted_moments(dc, values, W):
    """S0, S1, S2 (fp64 device tensors [T, G, C]) of a DeviceCounts, its fp32 values in CSC order and a dense fp64 W[n, C] in
    the permuted row order.  ValueError for a wrong shape or dtype and for C outside 1 .. 1024, RuntimeError for a tensor that
    is not on the device; both before any launch."""
    import torch
    from ._lib import model_lib
    if not isinstance(W, torch.Tensor) or not isinstance(values, torch.Tensor):
        raise RuntimeError("weighted_moments takes device tensors (torch), not host arrays")
    if not W.is_cuda or not values.is_cuda:
        raise RuntimeError(f"weighted_moments runs on the device: W is on {W.device}, values on {values.device}")
    if W.dtype != torch.float64:
        raise ValueError(f"W must be float64, not {W.dtype}")
    if values.dtype != torch.float32 or values.shape != dc.cval.shape:
        raise ValueError(f"values must be float32 of shape {tuple(dc.cval.shape)}, one per stored entry")
    if W.dim() != 2 or W.shape[0] != dc.n:
        raise ValueError(f"W must be [n, C] with one row per spot: {dc.n} spots, W of shape {tuple(W.shape)}")
    C = int(W.shape[1])
    if C < 1 or C > MAX_COLUMNS:
        raise ValueError(f"W has {C} columns: weighted_moments takes 1 .. {MAX_COLUMNS}")
    if dc.n > MAX_ROWS:
        raise ValueError(f"{dc.n} spots: weighted_moments takes at most {MAX_ROWS}")
    W = W.contiguous()
    values = values.contiguous()
    out = [torch.empty((dc.T, dc.G, C), dtype=torch.float64, device=dc.device) for _ in range(3)]
    with torch.cuda.device(dc.device):
        _check(model_lib().spadot_weighted_moments(_p(dc.colptr), _p(dc.ridx), _p(values), _p(dc.tp_off), dc.T, dc.G, _p(W),
                                                   dc.n, C, _p(out[0]), _p(out[1]), _p(out[2]), _stream()),
               "spadot_weighted_moments")
    return tuple(out)


def _dense(M, n, what):
    M = np.asarray(M)
    if M.ndim != 2 or M.shape[0] != n:
        raise ValueError(f"{what} must be [n, columns] with one row per spot: {n} spots, {what} of shape {M.shape}")
    if M.shape[1] < 1 or M.shape[1] + 1 > MAX_COLUMNS:
        raise ValueError(f"{what} has {M.shape[1]} columns: the trends stage takes 1 .. {MAX_COLUMNS - 1}")
    M = np.ascontiguousarray(M, dtype=np.float64)
    if not np.all(np.isfinite(M)):
        raise ValueError(f"{what} has entries that are not finite")
    return M


def _names(names, C, stem):
    names = [f"{stem}{c}" for c in range(C)] if names is None else [str(x) for x in names]
    if len(names) != C:
        raise ValueError(f"{len(names)} names for {C} columns")
    return np.asarray(names)


class _Run:
    """The device side shared by gene_trends and fate_drivers: upload, log-normalise, one kernel call, the timings."""

    def __init__(self, counts, device):
        import torch
        if torch.device(device).type != "cuda":
            raise ValueError(f"the trends stage runs on the MI355X (a cuda device), not on {device!r}")
        self.t0 = time.perf_counter()
        self.raw = counts if isinstance(counts, RawCounts) else load_counts(counts)[0]
        self.device = device

    def upload(self, M):
        import torch
        from .preprocess import DeviceCounts
        self.dc = DeviceCounts(self.raw, self.device)
        Mp = torch.as_tensor(M[self.dc.perm], device=self.dc.device)
        torch.cuda.synchronize(self.dc.device)
        self.t_up = time.perf_counter()
        return self.dc, Mp

    def moments(self, Wd):
        import torch
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        with torch.cuda.device(self.dc.device):
            ev[0].record()
            self.values = lognorm_values(self.dc)
            ev[1].record()
            S = weighted_moments(self.dc, self.values, Wd)
            ev[2].record()
        self.ev = ev
        return S

    def device_done(self):
        import torch
        torch.cuda.synchronize(self.dc.device)
        self.t_dev = time.perf_counter()

    def timings(self):
        t_end = time.perf_counter()
        return dict(upload_s=self.t_up - self.t0, device_s=self.t_dev - self.t_up, host_s=t_end - self.t_dev,
                    total_s=t_end - self.t0, lognorm_ms=self.ev[0].elapsed_time(self.ev[1]),
                    moments_ms=self.ev[1].elapsed_time(self.ev[2]))

    def layout(self):
        dc = self.dc
        return dict(values=self.values.cpu().numpy(), colptr=dc.colptr.cpu().numpy(), ridx=dc.ridx.cpu().numpy(), perm=dc.perm,
                    tp_off=dc.tp_off_host.astype(np.int64), genes=dc.genes, timepoints=list(dc.tps))


def gene_trends(counts, W, names=None, device="cuda:0"):
    """Weighted mean expression of every gene under every column of W, per time point.  counts: anything load_counts accepts
    in memory; W: [n, C] in input row order, non-negative (normally the X of trajectories.npz).

    Returns a dict: mean, var, pct, delta (fp64 [T, G, C]), baseline [T, G], change [G, C], colsum [T, C] (the s of every time
    point and column), S0, S1, S2 (the device's sums, fp64 [T, G, C + 1]: the last column is the column of ones), names, genes,
    timepoints (in order of first appearance), values / colptr / ridx / perm / tp_off (the fp32 v the device read, in the CSC
    order of the permuted rows) and timings (seconds; the kernels in device milliseconds)."""
    import torch
    run = _Run(counts, device)
    W = _dense(W, run.raw.n_obs, "W")
    if W.min() < 0:
        raise ValueError("W must be non-negative (weights over the spots)")
    C = W.shape[1]
    names = _names(names, C, "trajectory_")
    dc, Wp = run.upload(W)
    Wd = torch.cat([Wp, torch.ones((dc.n, 1), dtype=torch.float64, device=dc.device)], dim=1)
    S0, S1, S2 = run.moments(Wd)
    off = dc.tp_off_host
    s = torch.stack([Wp[int(off[t]):int(off[t + 1])].sum(0) for t in range(dc.T)])                 # [T, C]
    n_t = torch.as_tensor(np.diff(off).astype(np.float64), device=dc.device)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dc.device)
    ok = (s > 0)[:, None, :]
    sd = torch.where(ok, s[:, None, :], torch.ones_like(s[:, None, :]))
    mean = torch.where(ok, S1[:, :, :C] / sd, nan)
    var = torch.where(ok, torch.clamp(S2[:, :, :C] / sd - mean * mean, min=0.0), nan)
    pct = torch.where(ok, S0[:, :, :C] / sd, nan)
    baseline = S1[:, :, C] / n_t[:, None]
    delta = mean - baseline[:, :, None]
    run.device_done()
    out = dict(mean=mean.cpu().numpy(), var=var.cpu().numpy(), pct=pct.cpu().numpy(), delta=delta.cpu().numpy(),
               baseline=baseline.cpu().numpy(), colsum=s.cpu().numpy(), S0=S0.cpu().numpy(), S1=S1.cpu().numpy(),
               S2=S2.cpu().numpy())
    live = out["colsum"] > 0
    change = np.full((dc.G, C), np.nan)
    for c in range(C):
        ts = np.flatnonzero(live[:, c])
        if ts.size:
            change[:, c] = out["mean"][ts[-1], :, c] - out["mean"][ts[0], :, c]
    out.update(change=change, names=names, **run.layout())
    out["timings"] = run.timings()
    return out


def fate_drivers(counts, F, names=None, device="cuda:0"):
    """Pearson correlation of every gene with every fate, per time point, over the spots that send mass anywhere.  counts:
    anything load_counts accepts in memory; F: [n, K] in input row order (normally the X of fates.npz).

    Returns a dict: r, pval, padj (fp64 [T, G, K]), n_valid (int64 [T]), ssf ([T, K], the sum of squares of the centred fates),
    S0, S1, S2 (the device's sums, fp64 [T, G, K + 1]: the last column is the validity column u), Wc ([n, K + 1] in the permuted
    row order: what the device was called with), names, genes, timepoints, values / colptr / ridx / perm / tp_off, timings."""
    import torch
    from scipy.special import stdtr
    run = _Run(counts, device)
    F = _dense(F, run.raw.n_obs, "F")
    K = F.shape[1]
    names = _names(names, K, "fate_")
    dc, Fp = run.upload(F)
    off = dc.tp_off_host
    Wd = torch.zeros((dc.n, K + 1), dtype=torch.float64, device=dc.device)
    n_valid = np.zeros(dc.T, dtype=np.int64)
    ssf = torch.zeros((dc.T, K), dtype=torch.float64, device=dc.device)
    for t in range(dc.T):
        lo, hi = int(off[t]), int(off[t + 1])
        Ft = Fp[lo:hi]
        u = (Ft.sum(1) != 0).to(torch.float64)
        nv = int(u.sum().item())
        n_valid[t] = nv
        if nv:
            Wc = u[:, None] * (Ft - (u[:, None] * Ft).sum(0) / nv)
            Wd[lo:hi, :K] = Wc
            ssf[t] = (Wc * Wc).sum(0)
        Wd[lo:hi, K] = u
    S0, S1, S2 = run.moments(Wd)
    run.device_done()
    S0, S1, S2, ssf = S0.cpu().numpy(), S1.cpu().numpy(), S2.cpu().numpy(), ssf.cpu().numpy()
    r = np.zeros((dc.T, dc.G, K))
    pval = np.ones((dc.T, dc.G, K))
    padj = np.ones((dc.T, dc.G, K))
    for t in range(dc.T):
        nv = float(n_valid[t])
        if nv < 3:
            continue
        M1, M2, cov = S1[t, :, K], S2[t, :, K], S1[t, :, :K]
        ssv = M2 - M1 * M1 / nv
        ok = (ssv > nv * 2.0 ** -50 * M2)[:, None] & (ssf[t] > 0)[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            rt = np.clip(cov / np.sqrt(np.where(ok, ssv[:, None] * ssf[t][None, :], 1.0)), -1.0, 1.0)
            rt = np.where(ok, rt, 0.0)
            tt = rt * np.sqrt((nv - 2.0) / ((1.0 - rt) * (1.0 + rt)))
            pt = np.where(np.abs(rt) >= 1.0, 0.0, 2.0 * stdtr(nv - 2.0, -np.abs(tt)))
        pt = np.where(ok, pt, 1.0)
        expressed = M2 > 0
        rt[~expressed] = 0.0
        pt[~expressed] = 1.0
        r[t], pval[t] = rt, pt
        for k in range(K):
            padj[t, expressed, k] = bh_adjust(pt[expressed, k])
    out = dict(r=r, pval=pval, padj=padj, n_valid=n_valid, ssf=ssf, S0=S0, S1=S1, S2=S2, Wc=Wd.cpu().numpy(), names=names,
               **run.layout())
    out["timings"] = run.timings()
    return out


# ---------------------------------------------------------------------------------------------------------------- the stage
def read_lineage(path, timepoint):
    """X of a trajectories.npz / fates.npz of `analyze --lineage` in the row order of the data, and its column names.  The
    file's `rows` are row numbers of the data and `timepoint` their time points: every row of the data must appear exactly
    once, with the data's time point (compared as strings), ValueError otherwise."""
    z = np.load(path, allow_pickle=False)
    for key in ("X", "rows", "timepoint", "names"):
        if key not in z.files:
            raise ValueError(f"{path} has no `{key}` array (expected a trajectories.npz or fates.npz of analyze --lineage)")
    X, row, ztp = np.asarray(z["X"]), np.asarray(z["rows"]), np.asarray(z["timepoint"])
    shapes = X.ndim == 2 and X.shape[0] == row.shape[0] and ztp.shape[0] == row.shape[0] and len(z["names"]) == X.shape[1]
    if row.dtype.kind in "iu" and not shapes:                # rows that are no integers are refused first, by align_rows
        raise ValueError(f"{path}: X of shape {X.shape} against {row.shape[0]} rows, {ztp.shape[0]} time point entries and "
                         f"{len(z['names'])} names")
    row = align_rows(row, ztp, timepoint, f"the `rows` of {path}", path, f"appears more than once in {path}",
                     f"is missing from {path}", show=lambda v: repr(str(v)))
    out = np.empty((row.shape[0], X.shape[1]), dtype=np.float64)
    out[row] = X
    return out, np.asarray(z["names"]).astype(str)


def trends_table(res, top=100):
    """The rows of {prefix}trends_top.csv: per trajectory the `top` genes (0 = all) by |change| descending, then gene column."""
    import pandas as pd
    G, C = res["change"].shape
    genes = np.asarray(res["genes"])
    tcols = [f"mean_{tp}" for tp in res["timepoints"]]
    frames = []
    for c in range(C):
        key = np.abs(res["change"][:, c])
        order = np.lexsort((np.arange(G), -np.where(np.isnan(key), -np.inf, key)))
        if top:
            order = order[:top]
        cols = {"trajectory": np.full(order.size, res["names"][c]), "gene": genes[order], "change": res["change"][order, c]}
        cols.update({name: res["mean"][t, order, c] for t, name in enumerate(tcols)})
        frames.append(pd.DataFrame(cols, columns=["trajectory", "gene", "change"] + tcols))
    return pd.concat(frames, ignore_index=True)


def drivers_table(res, t, top=100):
    """The rows of {prefix}drivers_{tp}.csv: per fate the `top` genes (0 = all) by r descending, then gene column."""
    import pandas as pd
    G, K = res["r"][t].shape
    genes = np.asarray(res["genes"])
    frames = []
    for k in range(K):
        order = np.lexsort((np.arange(G), -res["r"][t][:, k]))
        if top:
            order = order[:top]
        frames.append(pd.DataFrame({"gene": genes[order], "fate": np.full(order.size, res["names"][k]),
                                    "r": res["r"][t][order, k], "pval": res["pval"][t][order, k],
                                    "padj": res["padj"][t][order, k]}, columns=list(DRIVER_COLUMNS)))
    return pd.concat(frames, ignore_index=True)


def trends(args):
    """Reads args.data (counts, as the markers stage) and args.trajectories and / or args.fates (the npz files of
    analyze --lineage).  Writes {prefix}trends.npz (mean, var, pct, delta [T, G, C], baseline [T, G], change [G, C], names,
    genes, timepoints) and {prefix}trends_top.csv for the trajectories, {prefix}drivers.npz (r, pval, padj [T, G, K], n_valid
    [T], names, genes, timepoints) and {prefix}drivers_{tp}.csv for the fates.  Returns the arrays of both plus `timings`."""
    traj, fates = getattr(args, "trajectories", None), getattr(args, "fates", None)
    if not traj and not fates:
        raise ValueError("the trends stage needs trajectories.npz and / or fates.npz of analyze --lineage (--trajectories, "
                         "--fates)")
    top = top_setting(args, 100, least=0)
    raw, path = load_marker_counts(args.data)
    tp = raw.obs["timepoint"]
    W = read_lineage(traj, tp) if traj else None
    F = read_lineage(fates, tp) if fates else None
    out_file = open_output(args, path)
    device = getattr(args, "device", None) or "cuda:0"
    out, timings = {}, {}

    def save(res, keys, archive, names_key):
        """The archive of one result; its arrays and names go to `out`."""
        common = dict(names=np.asarray(res["names"]).astype(str), genes=np.asarray(res["genes"]).astype(str),
                      timepoints=np.asarray([str(t) for t in res["timepoints"]]))
        np.savez(out_file(archive), **{k: res[k] for k in keys}, **common)
        out.update({k: res[k] for k in keys}, **{names_key: common["names"]}, genes=common["genes"], timepoints=common["timepoints"])
        return common["timepoints"]

    if W is not None:
        res = gene_trends(raw, W[0], names=W[1], device=device)
        save(res, TREND_KEYS, "trends.npz", "trajectory_names")
        trends_table(res, top).to_csv(out_file("trends_top.csv"), index=False)
        timings["trends"] = res["timings"]
    if F is not None:
        res = fate_drivers(raw, F[0], names=F[1], device=device)
        for t, name in enumerate(save(res, DRIVER_KEYS, "drivers.npz", "fate_names")):
            drivers_table(res, t, top).to_csv(out_file(f"drivers_{name}.csv"), index=False)
        timings["drivers"] = res["timings"]
    out["timings"] = timings
    print(f"trends: {len(out['genes'])} genes x {len(out['timepoints'])} time points written to {args.output_dir}",
          file=sys.stderr)
    return out
