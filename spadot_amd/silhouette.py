"""Silhouette coefficients on the device: how well separated the domains of `analyze` are in the latent space, which spots sit
between two domains, and a second criterion for the number of domains (csrc/silhouette.hip).  The reference has no
such stage; the definition is sklearn.metrics.silhouette_samples on the fp64 values of the input.

    silhouette_many(Xs, labelings)      every (data set t, labeling l) problem of the call in ONE launch
    silhouette_samples(X, labels)       one problem, shaped like sklearn's; silhouette_score(X, labels): its mean
    score(args)    the stage.  args: data (latent.npz), domains ({prefix}domains.csv of analyze), output_dir, prefix (''), device

For n points x_i (fp64) and labels in 0 .. K-1, with dist(i, j) = sqrt(sum_c (x_ic - x_jc)^2), S_i(k) the sum of dist(i, j) over
cluster k and n_k its size, a point of cluster c has
    a_i = S_i(c) / (n_c - 1) (0 if n_c = 1),  b_i = min over the non-empty k != c of S_i(k) / n_k (nearest_i: that k, first
    minimum),  s_i = (b_i - a_i) / max(a_i, b_i), and s_i = 0 if n_c = 1 or max(a_i, b_i) = 0.
A label value without points is skipped.  The score of a labeling is the fp64 mean of s_i; it is undefined (NaN) unless
2 <= non-empty clusters <= n - 1.

The device computes a, b, nearest and s; torch orders every problem's points by (label, row) and forms the cluster offsets on
the device (a stable sort and a bincount); the host validates, takes the means and writes the files.  Limits: 1 <= d <= 32,
2 <= K <= 32, at most 65535 problems per call, at most 2147483391 points per set (int32 positions)."""
import os
import sys
import time

import numpy as np

from .utils._stage_utils import cuda_device, need_domains, open_output, read_domains, timepoint_masks, timings

MAX_DIM = 32
MAX_CLUSTERS = 32
MAX_PROBLEMS = 65535
MAX_POINTS = 2147483391
SAMPLE_COLUMNS = ("row", "timepoint", "kmeans", "a", "b", "nearest", "silhouette")
SUMMARY_COLUMNS = ("timepoint", "domain", "n", "silhouette")


class SilhouetteResult:
    """One (data set, labeling): a, b (fp64 [n]), nearest (int32 [n]; -1 where no other cluster exists), samples (fp64 [n]) in
    the caller's row order, sizes (int64 [K]: points per label value) and score (the mean of samples, NaN where undefined)."""

    def __init__(self, a, b, nearest, samples, sizes):
        self.a, self.b, self.nearest, self.samples, self.sizes = a, b, nearest, samples, sizes
        self.defined = 2 <= int((sizes > 0).sum()) <= samples.shape[0] - 1
        self.score = float(np.mean(samples)) if self.defined else float("nan")


class SilhouetteBatch:
    """The problems of one silhouette_many call, validated (ValueError / RuntimeError before any launch) and uploaded.
    prepare(): the (label, row) order and the cluster offsets, on the device; launch(): the kernel; results(): the download."""

    def __init__(self, Xs, labelings, n_clusters=None):
        import torch
        Xs = [x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)) for x in Xs]
        if not Xs or len(labelings) != len(Xs):
            raise ValueError(f"silhouette_many takes one list of labelings per data set ({len(Xs)} sets, {len(labelings)} lists)")
        for x in Xs:
            if not x.is_cuda:
                raise RuntimeError("spadot_amd scores silhouettes on the MI355X only (got a CPU tensor); there is no CPU path")
            if x.dim() != 2 or x.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"a data set must be an [n, d] fp32 or fp64 tensor (got {tuple(x.shape)} {x.dtype})")
        dev, d = Xs[0].device, int(Xs[0].shape[1])
        if any(int(x.shape[1]) != d or x.device != dev for x in Xs):
            raise ValueError("the data sets of one call must share their dimension and their device")
        if not 1 <= d <= MAX_DIM:
            raise ValueError(f"the device silhouette supports data of 1 to {MAX_DIM} dimensions (got {d})")
        sizes, sets, labs = [], [], []
        for t, (x, ls) in enumerate(zip(Xs, labelings)):
            n = int(x.shape[0])
            if not 1 <= n <= MAX_POINTS:
                raise ValueError(f"data set {t} has {n} points: the device silhouette takes 1 to {MAX_POINTS}")
            for lab in ls:
                lab = lab if isinstance(lab, torch.Tensor) else torch.as_tensor(np.asarray(lab))
                if lab.dim() != 1 or lab.shape[0] != n:
                    raise ValueError(f"a labeling of data set {t} must hold one label per point ({n}), not {tuple(lab.shape)}")
                if lab.dtype.is_floating_point or lab.dtype == torch.bool or lab.dtype.is_complex:
                    raise ValueError(f"labels must be integers (got {lab.dtype})")
                sizes.append(n); sets.append(t); labs.append(lab.to(device=dev, dtype=torch.int64))
        P = len(labs)
        if not 1 <= P <= MAX_PROBLEMS:
            raise ValueError(f"one call scores 1 to {MAX_PROBLEMS} labelings (got {P})")
        self.device, self.d, self.P, self.sizes, self.sets = dev, d, P, sizes, sets
        self.shape = [len(ls) for ls in labelings]
        self.total = int(sum(sizes))
        self.ooff_host = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        xoff = np.concatenate([[0], np.cumsum([int(x.shape[0]) for x in Xs])[:-1]]).astype(np.int64)
        with torch.cuda.device(dev):
            self.X = torch.cat([x.to(torch.float64) for x in Xs]).contiguous()
            self.labels = torch.cat(labs)
            self.nper = torch.as_tensor(np.asarray(sizes, dtype=np.int64), device=dev)
            self.pid = torch.repeat_interleave(torch.arange(P, device=dev), self.nper, output_size=self.total)
            lo = torch.zeros(P, dtype=torch.int64, device=dev).scatter_reduce(0, self.pid, self.labels, "amin", include_self=False)
            hi = torch.zeros(P, dtype=torch.int64, device=dev).scatter_reduce(0, self.pid, self.labels, "amax", include_self=False)
            lo, hi = torch.stack([lo, hi]).cpu().numpy()           # the one host round trip ahead of the launch
        if n_clusters is None:
            Ks = (hi + 1).tolist()
        else:
            Ks = [int(k) for kt in n_clusters for k in kt]
            if len(Ks) != P:
                raise ValueError(f"n_clusters holds {len(Ks)} cluster counts for {P} labelings")
        for p, K in enumerate(Ks):
            if not 2 <= K <= MAX_CLUSTERS:
                raise ValueError(f"labeling {p} has {K} label values: the device silhouette takes 2 to {MAX_CLUSTERS}")
            if lo[p] < 0 or hi[p] >= K:
                raise ValueError(f"labeling {p} holds labels {int(lo[p])} .. {int(hi[p])}: labels must lie in 0 .. {K - 1}")
        self.Ks = Ks
        prob = np.stack([xoff[np.asarray(sets)], self.ooff_host, np.asarray(sizes, dtype=np.int64),
                         np.asarray(Ks, dtype=np.int64)], axis=1)
        self.prob = torch.as_tensor(np.ascontiguousarray(prob), device=dev)
        self.ooff = torch.as_tensor(self.ooff_host, device=dev)
        self.order = self.coff = self.counts = self.out = None

    def prepare(self):
        import torch
        with torch.cuda.device(self.device):
            key = self.pid * MAX_CLUSTERS + self.labels                       # labels < 32: validated
            idx = torch.sort(key, stable=True).indices                         # by (problem, label, row)
            self.order = (idx - torch.repeat_interleave(self.ooff, self.nper, output_size=self.total)).to(torch.int32)
            self.counts = torch.bincount(key, minlength=self.P * MAX_CLUSTERS).view(self.P, MAX_CLUSTERS)
            coff = torch.zeros((self.P, MAX_CLUSTERS + 1), dtype=torch.int32, device=self.device)
            coff[:, 1:] = torch.cumsum(self.counts, dim=1)
            self.coff = coff

    def launch(self):
        import torch
        from .stage_ops import silhouette_launch
        with torch.cuda.device(self.device):
            self.out = silhouette_launch(self.X, self.prob, self.order, self.coff, max(self.sizes), min(self.Ks),
                                         max(self.Ks), out=self.out)

    def results(self):
        """[t][l] -> SilhouetteResult."""
        a, b, nearest, s = (x.cpu().numpy() for x in self.out)
        counts = self.counts.cpu().numpy()
        flat = []
        for p in range(self.P):
            lo, hi = int(self.ooff_host[p]), int(self.ooff_host[p]) + self.sizes[p]
            flat.append(SilhouetteResult(a[lo:hi].copy(), b[lo:hi].copy(), nearest[lo:hi].copy(), s[lo:hi].copy(),
                                         counts[p, :self.Ks[p]].astype(np.int64)))
        out, p = [], 0
        for m in self.shape:
            out.append(flat[p:p + m])
            p += m
        return out


def silhouette_many(Xs, labelings, n_clusters=None):
    """Xs: [n_t, d] device tensors (fp32 or fp64, converted to fp64: exact); labelings[t]: integer label vectors of set t
    (numpy or torch).  n_clusters[t][l]: the K of each labeling (labels in 0 .. K-1; default: its largest label + 1).  One
    launch; returns [t][l] -> SilhouetteResult.  A problem's result does not depend on what else the call holds."""
    batch = SilhouetteBatch(Xs, labelings, n_clusters)
    batch.prepare()
    batch.launch()
    return batch.results()


def silhouette_samples(X, labels):
    """sklearn.metrics.silhouette_samples(X, labels) for a device tensor X: fp64 [n].  ValueError unless 2 <= the number of
    distinct labels <= n - 1, as sklearn; RuntimeError for a CPU tensor."""
    r = silhouette_many([X], [[labels]])[0][0]
    if not r.defined:
        raise ValueError(f"Number of labels is {int((r.sizes > 0).sum())}. Valid values are 2 to n_samples - 1 (inclusive)")
    return r.samples


def silhouette_score(X, labels):
    """sklearn.metrics.silhouette_score(X, labels) (no sampling): the fp64 mean of silhouette_samples."""
    return float(np.mean(silhouette_samples(X, labels)))


def _positions(df, row_ids, n):
    """The domains table with its `row` column as positions 0 .. n-1 of the latents.  analyze writes the latents' own row ids
    (latent.npz `rows`) there; where the latents carry none, the column already holds positions."""
    if row_ids is None or "row" not in df.columns:
        return df
    ids = np.asarray(row_ids)
    if ids.shape[0] == n and ids.dtype.kind in "iu" and np.array_equal(ids, np.arange(n)):
        return df
    lookup = {v: i for i, v in enumerate(ids.tolist())}
    if len(lookup) != n:
        raise ValueError("the latents' row ids are not unique: the domains table cannot be matched to them")
    pos = [lookup.get(v, -1) for v in np.asarray(df["row"]).tolist()]
    if -1 in pos:
        bad = np.asarray(df["row"])[pos.index(-1)]
        raise ValueError(f"the domains table names row {bad!r}, which the latents do not have")
    return df.assign(row=np.asarray(pos, dtype=np.int64))


def score(args):
    """Reads args.data (the latents, as analyze reads them) and args.domains (the domains.csv of analyze); writes
    {prefix}silhouette.csv (row, timepoint, kmeans, a, b, nearest, silhouette per spot, in input order) and
    {prefix}silhouette_summary.csv (timepoint, domain, n, silhouette: the mean over every domain's spots and a row `all` per
    time point).  Returns {'samples', 'summary' (DataFrames), 'scores' (per time point), 'timepoints', 'timings'}."""
    import pandas as pd
    from .utils import _utils
    t_start = time.perf_counter()
    adata, path = _utils.load_data(args.data)
    domains = need_domains(args, "score")
    X = np.asarray(adata.X.toarray() if hasattr(adata.X, "toarray") else adata.X)
    tp_all = np.asarray(adata.obs["timepoint"])
    n = X.shape[0]
    obs = adata.obs
    row_ids = (np.asarray(obs["row"]) if "row" in obs else None) if isinstance(obs, dict) else np.asarray(obs.index)
    out_ids = row_ids if row_ids is not None else np.arange(n)
    df = pd.read_csv(domains) if isinstance(domains, (str, os.PathLike)) else domains
    if row_ids is not None and "row" in df.columns and np.asarray(df["row"]).dtype.kind != np.asarray(row_ids).dtype.kind:
        row_ids = np.asarray(row_ids).astype(str)
        df = df.assign(row=np.asarray(df["row"]).astype(str))
    labels = read_domains(_positions(df, row_ids, n), tp_all).astype(np.int64)
    if not 1 <= X.shape[1] <= MAX_DIM:
        raise ValueError(f"the latent has {X.shape[1]} dimensions; the device silhouette supports 1 to {MAX_DIM}")
    out_file = open_output(args, path)

    import torch
    dev = cuda_device(args, "scores silhouettes")
    tps, masks = timepoint_masks(tp_all)
    t_read = time.perf_counter()
    Xs = [torch.as_tensor(np.ascontiguousarray(X[m]), device=dev) for m in masks]
    labs = [labels[m] for m in masks]
    Ks = [[max(int(lab.max()) + 1, 2)] for lab in labs]            # a time point with one domain: an undefined labeling, NaN
    res = silhouette_many(Xs, [[lab] for lab in labs], n_clusters=Ks)
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter()

    cols = {c: np.empty(n, dtype=np.float64) for c in ("a", "b", "silhouette")}
    nearest = np.empty(n, dtype=np.int64)
    summary, scores = [], {}
    for tp, m, lab, rt in zip(tps, masks, labs, res):
        r = rt[0]
        cols["a"][m], cols["b"][m], cols["silhouette"][m], nearest[m] = r.a, r.b, r.samples, r.nearest
        for k in np.flatnonzero(r.sizes > 0).tolist():
            summary.append((tp, str(k), int(r.sizes[k]), float(np.mean(r.samples[lab == k]))))
        summary.append((tp, "all", int(lab.shape[0]), float(np.mean(r.samples))))
        scores[tp] = r.score
    samples = pd.DataFrame({"row": out_ids, "timepoint": tp_all, "kmeans": labels,
                            "a": cols["a"], "b": cols["b"], "nearest": nearest, "silhouette": cols["silhouette"]},
                           columns=list(SAMPLE_COLUMNS))
    summary = pd.DataFrame(summary, columns=list(SUMMARY_COLUMNS))
    samples.to_csv(out_file("silhouette.csv"), index=False)
    summary.to_csv(out_file("silhouette_summary.csv"), index=False)
    t_end = time.perf_counter()
    print(f"score: {n} spots of {len(tps)} time points written to {args.output_dir}", file=sys.stderr)
    return {"samples": samples, "summary": summary, "scores": scores, "timepoints": tps,
            "timings": timings(t_start, t_read, t_dev, t_end)}
