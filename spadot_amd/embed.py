"""A two-dimensional map of the latent space on the device: t-SNE with sklearn 1.7's objective and optimiser, Barnes-Hut's sparse
input affinities and EXACT repulsion over all pairs in fp64 (csrc/embed.hip).  The reference has no such stage.

    latent_knn(X, k)                  the k nearest other points of every point: (idx int32 [n, k], d2 fp64 [n, k])
    tsne_affinities(X, perplexity)    idx, d2, the conditional affinities, beta and the joint P as CSR
    pca_start(X)                      sklearn's init="pca": the two leading principal components, scaled (on the host)
    tsne_many(Xs, ...)                one embedding per set; the sets are the problems of ONE launch per kernel
    tsne(X, ...)                      one set
    embed(args)                       the stage.  args: data (latent.npz), domains (optional), output_dir, prefix, perplexity,
                                      n_iter, early, learning_rate, per_timepoint, device

A problem is a set of n points in d dimensions (fp64, 1 <= d <= 32) and a perplexity u with 2 <= u <= 50 and n >= u + 2.
  1. Neighbours: per point the k = min(n - 1, floor(3 u)) nearest other points by (squared distance, index) ascending; the
     squared distance is sum_c (x_ic - x_jc)^2, c ascending, unfused.  Self is left out by index; duplicates are neighbours at 0.
  2. Conditional affinities: per row e_j = d2_j - min d2, p_j = exp(-beta e_j), s = sum p_j, H = log s + beta sum e_j p_j / s;
     beta by bisection from 1 (doubled without an upper bracket, halved without a lower one, up when H > log u), 200 steps with no
     early stop -- sklearn's _binary_search_perplexity without its float32 distances and its 1e-5 entropy tolerance.  A row whose
     e are all 0 is uniform and reports beta = 0.
  3. Joint affinities: P = (C + C^T) / sum(C + C^T) as CSR with ascending columns, built on the host once per problem; an entry
     is stored wherever C or C^T has one.
  4. Start: pca_start, sklearn's init="pca".
  5. Iteration `it`, with eps = exaggeration (12) and mu = 0.5 while it < early (250), then eps = 1 and mu = 0.8:
     q_ij = 1 / (1 + |y_i - y_j|^2) for j != i;  z_i = sum_j q_ij;  r_i = sum_j q_ij^2 (y_i - y_j);  Z = sum_i z_i;
     a_i = sum over the stored entries of row i of eps P_ij q_ij (y_i - y_j);  g_i = 4 (a_i - r_i / Z);  then sklearn's
     _gradient_descent update per component (gain + 0.2 where update g < 0, else x 0.8, at least 0.01; update = mu update - lr
     gain g; y += update; lr = max(n / 12 / 4, 50) unless given);  kl[it] = sum_stored P_ij (log P_ij - log q_ij) + log Z.
Two departures from sklearn: kl[it] is Barnes-Hut's KL over the stored entries with the UNEXAGGERATED P in both phases, and there
is no gradient-norm stop and no no-progress stop: a run is exactly n_iter iterations, queued without a host synchronisation.

The partner range of the repulsion is cut into S slices of whole 256-tiles whose partial sums are added in slice order; S is
embed_slices(n), a function of n alone, unless `slices` overrides it.  Every sum has one fixed order and there are no atomics:
results are bitwise repeatable run to run, and alone or in a batch.  Nothing is random, so there is no seed."""
import os
import sys
import time

import numpy as np

from .utils._stage_utils import cuda_device, open_output, read_domains, savez_pinned, timepoint_masks, timings

MAX_DIM = 32
COLUMNS = ("row", "timepoint", "tsne_1", "tsne_2")


def _device_matrix(X, what):
    import torch
    X = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X))
    if X.dim() != 2 or X.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be an [n, d] fp32 or fp64 tensor (got {tuple(X.shape)} {X.dtype})")
    if not 1 <= int(X.shape[1]) <= MAX_DIM:
        raise ValueError(f"the device t-SNE supports data of 1 to {MAX_DIM} dimensions (got {int(X.shape[1])})")
    return X


def latent_knn(X, k):
    """(idx int32 [n, k], d2 fp64 [n, k]) on the device: the k nearest other points of every point of the device tensor X [n, d]
    by (squared distance, index) ascending, 1 <= k <= min(n - 1, 150).  RuntimeError for a CPU tensor."""
    import torch
    from . import stage_ops as so
    X = _device_matrix(X, "X")
    n, k = int(X.shape[0]), int(k)
    if not 1 <= k <= min(n - 1, so.EMBED_MAX_K) or n > so.EMBED_MAX_N:
        raise ValueError(f"latent_knn takes 1 <= k <= min(n - 1, {so.EMBED_MAX_K}) and n <= {so.EMBED_MAX_N} (got k = {k}, n = {n})")
    so.need_cuda(X)
    desc = np.zeros((1, so.EMBED_DESC), dtype=np.int64)
    desc[0, 1], desc[0, 2] = n, k
    with torch.cuda.device(X.device):
        X = X.to(torch.float64).contiguous()
        so.embed_check(X, desc)
        idx, d2 = so.latent_knn_launch(X, desc)
    return idx.view(n, k), d2.view(n, k)


def joint_csr(idx, cond):
    """P = (C + C^T) / sum(C + C^T) of the conditional affinities cond [n, k] at the columns idx [n, k], on the host: (rowptr
    int64 [n + 1], col int32, val fp64) with ascending columns; an entry is stored wherever C or C^T has one."""
    idx, cond = np.asarray(idx, dtype=np.int64), np.asarray(cond, dtype=np.float64)
    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    key = np.concatenate([rows * n + idx.ravel(), idx.ravel() * n + rows])
    order = np.argsort(key, kind="stable")
    key, v = key[order], np.concatenate([cond.ravel(), cond.ravel()])[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    val = np.add.reduceat(v, first)                               # at most two terms per entry: c_ij + c_ji
    key = key[first]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=rowptr[1:])
    return rowptr, (key % n).astype(np.int32), val / val.sum()


def pca_start(X):
    """sklearn's init="pca" in fp64, on the host: the two leading principal components of the centred data (eigen-decomposition
    of the d x d covariance), each flipped so that its entry of largest magnitude is positive, both scaled by 1e-4 / std(first
    component).  X: [n, d], a tensor or an array; returns fp64 [n, 2] (the second column is 0 for d = 1)."""
    X = np.asarray(X.detach().cpu() if hasattr(X, "detach") else X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    w, V = np.linalg.eigh(Xc.T @ Xc / max(X.shape[0] - 1, 1))
    V = V[:, np.argsort(-w, kind="stable")[:2]]
    if V.shape[1] < 2:
        V = np.concatenate([V, np.zeros((V.shape[0], 2 - V.shape[1]))], axis=1)
    for c in range(2):
        if V[np.argmax(np.abs(V[:, c])), c] < 0:
            V[:, c] = -V[:, c]
    Y = Xc @ V
    sd = np.std(Y[:, 0])
    return Y / sd * 1e-4 if sd > 0 else np.zeros_like(Y)          # all points equal: nothing to spread


class TsneResult:
    """One problem: embedding fp64 [n, 2], kl fp64 [n_iter], beta fp64 [n] and the parameters of the run."""

    def __init__(self, embedding, kl, beta, **par):
        self.embedding, self.kl, self.beta = embedding, kl, beta
        self.__dict__.update(par)


class TsneBatch:
    """The problems of one tsne_many call: validated (ValueError / RuntimeError before any launch), their neighbours, affinities
    and joint CSR computed, the optimiser's state on the device.  steps(m) queues the next m iterations; results() downloads.
    start[p]: None (pca_start), Y [n, 2], or (Y, update, gains) -- the state of the optimiser ahead of iteration it0."""

    def __init__(self, Xs, perplexity=30.0, n_iter=1000, early=250, exaggeration=12.0, learning_rate=None, slices=None, start=None,
                 it0=0, two=False):
        import torch
        from . import stage_ops as so
        Xs = [_device_matrix(x, f"data set {t}") for t, x in enumerate(Xs)]
        if not Xs:
            raise ValueError("tsne_many takes at least one data set")
        d = max(int(x.shape[1]) for x in Xs)              # a narrower set is padded with zero coordinates: exact zeros in d2
        if any(x.device != Xs[0].device for x in Xs):
            raise ValueError("the data sets of one call must share their device")
        sizes = [int(x.shape[0]) for x in Xs]
        n_iter, early, it0 = int(n_iter), int(early), int(it0)
        if n_iter < 0 or early < 0 or not 0 <= it0 <= n_iter:
            raise ValueError(f"n_iter and early must be >= 0 and it0 in 0 .. n_iter (got {n_iter}, {early}, {it0})")
        if not float(exaggeration) >= 1.0 or not np.isfinite(float(exaggeration)):
            raise ValueError(f"the exaggeration must be a finite number >= 1 (got {exaggeration})")
        desc, perp = so.embed_table(sizes, perplexity, slices)
        so.need_cuda(*Xs)
        self.device, self.sizes, self.P, self.d = Xs[0].device, sizes, len(sizes), d
        self.n_iter, self.early, self.exaggeration, self.it, self.two = n_iter, early, float(exaggeration), it0, bool(two)
        P = self.P
        if learning_rate is None:
            lr = [max(n / self.exaggeration / 4.0, 50.0) for n in sizes]
        else:
            lr = np.broadcast_to(np.asarray(learning_rate, dtype=np.float64), (P,)).tolist()
        if not all(np.isfinite(v) and v > 0 for v in lr):
            raise ValueError(f"the learning rate must be a finite positive number (got {learning_rate})")
        self.learning_rate = lr
        start = [None] * P if start is None else list(start)
        if len(start) != P:
            raise ValueError(f"start holds {len(start)} entries for {P} data sets")
        with torch.cuda.device(self.device):
            X = torch.cat([torch.nn.functional.pad(x.to(torch.float64), (0, d - int(x.shape[1]))) for x in Xs]).contiguous()
            so.embed_check(X, desc)
            desc_dev = torch.as_tensor(desc, device=self.device)
            self.idx, self.d2 = so.latent_knn_launch(X, desc, desc_dev)
            self.cond, self.beta = so.tsne_affinities_launch(self.d2, desc, perp, desc_dev)
            idx_h, cond_h = self.idx.cpu().numpy(), self.cond.cpu().numpy()
            csr = []
            for off, n, k, koff, *_rest in desc.tolist():
                csr.append(joint_csr(idx_h[koff:koff + n * k].reshape(n, k), cond_h[koff:koff + n * k].reshape(n, k)))
            self.csr_host = csr
            self.desc, self.perp = so.embed_table(sizes, perplexity, slices, nnz=[c[1].shape[0] for c in csr])
            self.desc_dev = torch.as_tensor(self.desc, device=self.device)
            self.rowptr = torch.as_tensor(np.concatenate([c[0] for c in csr]), device=self.device)
            self.col = torch.as_tensor(np.concatenate([c[1] for c in csr]), device=self.device)
            self.val = torch.as_tensor(np.concatenate([c[2] for c in csr]), device=self.device)
            so.tsne_csr_check(self.desc, self.rowptr, self.col, self.val)
            self.state = so.tsne_state(self.desc, n_iter, self.device)
            self.state["lr"].copy_(torch.as_tensor(np.asarray(lr, dtype=np.float64)))
            Y, upd, gains = [], [], []
            for p, (x, st, n) in enumerate(zip(Xs, start, sizes)):
                y, u, g = (st if isinstance(st, (tuple, list)) else (st, None, None))
                y = pca_start(x) if y is None else np.asarray(y, dtype=np.float64)
                u = np.zeros((n, 2)) if u is None else np.asarray(u, dtype=np.float64)
                g = np.ones((n, 2)) if g is None else np.asarray(g, dtype=np.float64)
                if y.shape != (n, 2) or u.shape != (n, 2) or g.shape != (n, 2) or not np.all(np.isfinite(y)):
                    raise ValueError(f"the start of data set {p} must be finite and of shape [{n}, 2]")
                Y.append(y); upd.append(u); gains.append(g)
            self.state["Y1" if it0 & 1 else "Y0"].copy_(torch.as_tensor(np.concatenate(Y)))
            self.state["upd"].copy_(torch.as_tensor(np.concatenate(upd)))
            self.state["gains"].copy_(torch.as_tensor(np.concatenate(gains)))

    def steps(self, m):
        import torch
        from . import stage_ops as so
        with torch.cuda.device(self.device):
            so.tsne_steps_launch(self.desc, self.desc_dev, self.rowptr, self.col, self.val, self.state, self.it, m, self.early,
                                 self.exaggeration, self.two)
        self.it += int(m)

    def current(self):
        """The device tensor that holds Y ahead of iteration self.it, [sum n, 2]."""
        return self.state["Y1" if self.it & 1 else "Y0"]

    def download(self, *names):
        """Per problem the rows of the named state buffers ('Y' for the current embedding) as numpy arrays: [p][name]."""
        out = []
        host = {k: (self.current() if k == "Y" else self.state[k]).cpu().numpy() for k in names}
        for p, (off, n, *_rest) in enumerate(self.desc.tolist()):
            out.append({k: (v[p].copy() if k in ("Z", "kl", "lr") else v[off:off + n].copy()) for k, v in host.items()})
        return out

    def results(self):
        Y, kl, beta = self.current().cpu().numpy(), self.state["kl"].cpu().numpy(), self.beta.cpu().numpy()
        out = []
        for p, (off, n, k, _koff, S, *_rest) in enumerate(self.desc.tolist()):
            out.append(TsneResult(Y[off:off + n].copy(), kl[p, :self.n_iter].copy(), beta[off:off + n].copy(),
                                  perplexity=float(self.perp[p]), n_neighbors=k, n_iter=self.n_iter, early=self.early,
                                  exaggeration=self.exaggeration, learning_rate=float(self.learning_rate[p]), slices=S))
        return out


def tsne_many(Xs, perplexity=30.0, n_iter=1000, early=250, exaggeration=12.0, learning_rate=None, slices=None, start=None):
    """t-SNE of every set of Xs ([n_t, d] device tensors, fp32 or fp64, converted to fp64: exact) as the problems of one launch per
    kernel.  perplexity, learning_rate (default max(n / exaggeration / 4, 50)) and slices (default embed_slices(n)): one value
    or one per set; start[t]: the starting Y [n_t, 2] (default pca_start).  Returns one TsneResult per set: embedding fp64 [n, 2],
    kl [n_iter], beta [n] and the parameters.  A set's result does not depend on what else the call holds; sets of fewer
    dimensions than the widest are padded with zero coordinates, which add exact zeros to every squared distance.  ValueError outside
    the limits and RuntimeError for a CPU tensor, before any launch."""
    batch = TsneBatch(Xs, perplexity, n_iter, early, exaggeration, learning_rate, slices, start)
    batch.steps(batch.n_iter)
    return batch.results()


def tsne(X, perplexity=30.0, n_iter=1000, early=250, exaggeration=12.0, learning_rate=None, slices=None, start=None):
    """tsne_many for one set: its TsneResult."""
    return tsne_many([X], perplexity, n_iter, early, exaggeration, learning_rate, slices, None if start is None else [start])[0]


def tsne_affinities(X, perplexity=30.0):
    """The input affinities of one set (a device tensor [n, d]): a dict of numpy arrays idx int32 [n, k], d2, cond fp64 [n, k] (the
    conditional p_{j|i}), beta fp64 [n] and rowptr int64 [n + 1], col int32, val fp64: the joint P as CSR."""
    batch = TsneBatch([X], perplexity, n_iter=0)
    n, k = batch.sizes[0], int(batch.desc[0, 2])
    rowptr, col, val = batch.csr_host[0]
    return dict(idx=batch.idx.cpu().numpy().reshape(n, k), d2=batch.d2.cpu().numpy().reshape(n, k),
                cond=batch.cond.cpu().numpy().reshape(n, k), beta=batch.beta.cpu().numpy(), rowptr=rowptr, col=col, val=val)


def embed(args):
    """Reads args.data (the latents, as analyze and score read them) and, where given, args.domains (the domains.csv of analyze);
    embeds all time points jointly, or every time point on its own with args.per_timepoint (the time points are then the problems
    of one launch).  Writes {prefix}embedding.csv (row, timepoint, tsne_1, tsne_2 and, with domains, kmeans, in input order),
    {prefix}embedding.npz (Y, kl [problems, n_iter], beta, perplexity, n_iter, early, learning_rate, slices, offsets: the sizes
    of the problems summed up, timepoints) and, with matplotlib, {prefix}embedding.png.  Returns {'embedding' (DataFrame), 'kl',
    'timepoints', 'timings'}."""
    import pandas as pd
    from . import stage_ops as so
    from .silhouette import _positions
    from .utils import _analyze_utils, _utils
    t_start = time.perf_counter()
    adata, path = _utils.load_data(args.data)
    X = np.asarray(adata.X.toarray() if hasattr(adata.X, "toarray") else adata.X, dtype=np.float64)
    tp_all = np.asarray(adata.obs["timepoint"])
    n = X.shape[0]
    obs = adata.obs
    row_ids = (np.asarray(obs["row"]) if "row" in obs else None) if isinstance(obs, dict) else np.asarray(obs.index)
    out_ids = row_ids if row_ids is not None else np.arange(n)
    perplexity = float(getattr(args, "perplexity", None) or 30.0)
    n_iter = 1000 if getattr(args, "n_iter", None) is None else int(args.n_iter)
    early = 250 if getattr(args, "early", None) is None else int(args.early)
    lr = getattr(args, "learning_rate", None)
    per_tp = bool(getattr(args, "per_timepoint", False))
    if X.ndim != 2 or not 1 <= X.shape[1] <= MAX_DIM:
        raise ValueError(f"the latent has {X.shape[1] if X.ndim == 2 else X.shape} dimensions; the device t-SNE supports 1 to "
                         f"{MAX_DIM}")
    if not np.all(np.isfinite(X)):
        raise ValueError("the latents hold values that are not finite")
    tps, masks = timepoint_masks(tp_all)
    sizes = [int(m.sum()) for m in masks] if per_tp else [n]
    try:
        so.embed_table(sizes, perplexity)                          # the perplexity and the sizes, before anything else is read
    except ValueError as e:
        raise ValueError(f"{e}" + (f" (the problems are the time points {tps})" if per_tp else "")) from None
    labels = None
    domains = getattr(args, "domains", None)
    if domains is not None and not (isinstance(domains, str) and not domains):
        df = pd.read_csv(domains) if isinstance(domains, (str, os.PathLike)) else domains
        ids = row_ids
        if ids is not None and "row" in df.columns and np.asarray(df["row"]).dtype.kind != np.asarray(ids).dtype.kind:
            ids = np.asarray(ids).astype(str)
            df = df.assign(row=np.asarray(df["row"]).astype(str))
        labels = read_domains(_positions(df, ids, n), tp_all).astype(np.int64)
    out_file = open_output(args, path)

    import torch
    dev = cuda_device(args, "embeds the latents")
    t_read = time.perf_counter()
    Xs = [torch.as_tensor(np.ascontiguousarray(X[m]), device=dev) for m in masks] if per_tp else [torch.as_tensor(X, device=dev)]
    res = tsne_many(Xs, perplexity=perplexity, n_iter=n_iter, early=early, learning_rate=lr)
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter()

    Y, beta = np.empty((n, 2)), np.empty(n)
    for m, r in zip(masks if per_tp else [np.ones(n, dtype=bool)], res):
        Y[m], beta[m] = r.embedding, r.beta
    cols = {"row": out_ids, "timepoint": tp_all, "tsne_1": Y[:, 0], "tsne_2": Y[:, 1]}
    if labels is not None:
        cols["kmeans"] = labels
    table = pd.DataFrame(cols, columns=list(COLUMNS) + (["kmeans"] if labels is not None else []))
    table.to_csv(out_file("embedding.csv"), index=False)
    kl = np.stack([r.kl for r in res])
    savez_pinned(out_file("embedding.npz"), dict(
        Y=Y, kl=kl, beta=beta, perplexity=np.float64(perplexity), n_iter=np.int64(n_iter), early=np.int64(early),
        learning_rate=np.asarray([r.learning_rate for r in res]), slices=np.asarray([r.slices for r in res], dtype=np.int64),
        offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), per_timepoint=np.int64(per_tp),
        timepoints=np.asarray([str(t) for t in tps])))
    if _analyze_utils.have_matplotlib():
        _analyze_utils.plot_embedding(out_file("embedding.png"), Y, tp_all, labels)
    else:
        print("matplotlib not installed: no plots")
    t_end = time.perf_counter()
    print(f"embed: {n} spots of {len(tps)} time points as {len(res)} embedding(s) written to {args.output_dir}", file=sys.stderr)
    return {"embedding": table, "kl": kl, "timepoints": tps, "results": res, "timings": timings(t_start, t_read, t_dev, t_end)}
