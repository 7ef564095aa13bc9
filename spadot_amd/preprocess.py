"""The preprocess stage: mirror of SpaDOT.preprocess (SpaDOT/preprocess.py, SpaDOT/utils/_preprocess_utils.py) with SPARK-X
(SpaDOT/utils/_utils.py:121-414) on the MI355X.

    preprocess(args)   args: data, output_dir (default: the data's directory), prefix ('preprocessed_'),
                       feature_selection (True), device ('cuda:0'), gene_clusters ('kmeans' or 'louvain'; default 'kmeans')

Per time point (in order of first appearance) with feature selection on: the SCTransform gene filter (a count >= 0.01 in at
least 5 spots), the spot and gene filters of _sparkx, the 11 SPARK-X statistics and p-values per gene, ACAT, Benjamini-
Yekutieli and the selection of min(G, max(#(adj <= 0.05), 500)) genes, then a clustering of the selected genes and the
balancing rule across time points (select_svgs).  Then, per time point on the selected genes: normalize_total(target_sum=1e-4)
over those genes, log1p, scale (ddof 1, std 0 -> 1, no clip), float32.  The per-gene work runs in HIP kernels
(csrc/preprocess.hip: fp64 sums owned by one wavefront each, no atomics, bitwise repeatable); the host does the plumbing
(row permutation, CSR -> CSC, the N x 22 kernel coordinates, ordering G values).

Deviations from the reference:
  * by default the `cluster` column of {tp}_SVG_sparkx_clustered_louvain.csv comes from K-means, not Louvain: the genes' standardised
    log1p(x * 1e4 / total) over the time point's spots, clipped at +-sqrt(N/30), its 29 leading principal components of genes
    as points (the device K-means admits 29 dimensions at k = 10; the reference's graph uses 30),
    KMeansDevice(10, random_state=1993, n_init=10).  The reference clusters SCTransform Pearson residuals with a 100-NN graph
    and Louvain at rising resolution until >= 10 clusters; gene_clusters='louvain' does that (cluster_genes_louvain on the
    device SCTransform of spadot_amd.sctransform; its own deviations are listed there and in DESIGN 7c).  Only the
    per-cluster quota of the balancing rule reads the clusters, so with K-means the choice of genes beyond the smallest time
    point's list can differ from the reference's;
  * p-values use the exact survival function of ylam (l1 chi^2_1 + l2 chi^2_1) in place of Davies / Liu (Liu is exact too
    when l1 = l2, which is SPARK-X's case up to rounding), and a gene with ylam = 0 gets p = 1 (the reference gets NaN and
    ACAT raises);
  * ties in adjusted p are broken by combined p, then by column order (the reference's sort is unstable).
Quirk kept: target_sum=1e-4 (likely meant as 1e4) is what the reference runs."""
import os
import sys

import numpy as np
import torch

from ._call import launched as _check, ptr as _p, stream as _stream
from ._lib import model_lib
from .sctransform import sctransform
from .utils._preprocess_utils import (N_KERNELS, RawCounts, by_adjust, kernel_coordinates, load_counts, rank_genes,  # noqa: F401
                                      select_svgs, timepoint_order)
from .utils._stage_utils import open_output

DETECT_THRESHOLD = 0.01        # sctransform vst: genes with a count >= 0.01 ...
MIN_CELLS = 5                  # ... in at least 5 spots
TARGET_SUM = 1e-4              # _preprocess_utils.py:33 (sic)
CLUSTER_TARGET = 1e4           # the clustering input's normalisation
N_PCS = 29                     # scanpy's n_pcs=30 less one: (10 + 256) * d <= 7936 doubles of LDS caps the device K-means at d = 29
N_GENE_CLUSTERS = 10
N_PCS_LOUVAIN = 30             # sc.pp.neighbors(n_pcs=30)
N_NEIGHBORS = 100              # sc.pp.neighbors(n_neighbors=100)
GENE_CLUSTERS = ("kmeans", "louvain")
PVAL_NODES = 256               # trapezoid nodes of the two-term survival function
CSV_SUFFIX = "_SVG_sparkx_clustered_louvain.csv"


class DeviceCounts:
    """The counts on the device, rows permuted into output order (time point blocks in `tps` order, input order inside a
    block): CSR (indptr int64, cidx int32, val fp32) and CSC (colptr int64, ridx int32 sorted, val fp32), tp_off int32."""

    def __init__(self, raw, device):
        import scipy.sparse as sp
        if torch.device(device).type != "cuda":
            raise ValueError(f"the preprocess stage runs on the MI355X (a cuda device), not on {device!r}")
        tp = np.asarray(raw.obs["timepoint"])
        if tp.dtype == object:                       # categorical / object columns: stored as strings in the npz
            tp = tp.astype(str)
        self.tps = timepoint_order(tp)
        self.perm = np.concatenate([np.flatnonzero(tp == t) for t in self.tps])
        X = raw.X[self.perm]
        if not sp.isspmatrix_csr(X):
            X = sp.csr_matrix(X)
        X.sort_indices()
        if X.nnz >= 2 ** 31 or X.shape[0] >= 2 ** 31 or X.shape[1] >= 2 ** 31:
            raise ValueError("the count matrix is too large for 32-bit indices")
        C = X.tocsc()
        C.sort_indices()
        self.X = X
        self.n, self.G = X.shape
        sizes = [int((tp == t).sum()) for t in self.tps]
        self.tp_off_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.T = len(self.tps)
        self.spatial = np.asarray(raw.obsm["spatial"], dtype=np.float64)[self.perm]
        self.timepoint = tp[self.perm]
        self.genes = np.asarray(raw.var_names).astype(str)
        self.device = torch.device(device)
        d = self.device
        self.tp_off = torch.as_tensor(self.tp_off_host, device=d)
        self.indptr = torch.as_tensor(X.indptr.astype(np.int64), device=d)
        self.cidx = torch.as_tensor(X.indices.astype(np.int32), device=d)
        self.val = torch.as_tensor(X.data.astype(np.float32), device=d)
        self.colptr = torch.as_tensor(C.indptr.astype(np.int64), device=d)
        self.ridx = torch.as_tensor(C.indices.astype(np.int32), device=d)
        self.cval = torch.as_tensor(C.data.astype(np.float32), device=d)

    def _csc(self):
        return _p(self.colptr), _p(self.ridx), _p(self.cval)

    def _csr(self):
        return _p(self.indptr), _p(self.cidx), _p(self.val)

    def _tp_slice(self, t):
        return self.tp_off if t is None else self.tp_off[t:t + 2]

    def gene_detect(self, thr=DETECT_THRESHOLD):
        """[T, G] int32 spots with x >= thr, [T, G] fp64 column totals, per time point."""
        cnt = torch.empty((self.T, self.G), dtype=torch.int32, device=self.device)
        colsum = torch.empty((self.T, self.G), dtype=torch.float64, device=self.device)
        _check(model_lib().spadot_pre_gene_detect(*self._csc(), _p(self.tp_off), self.T, self.G, float(thr), _p(cnt),
                                                  _p(colsum), _stream()), "spadot_pre_gene_detect")
        return cnt, colsum

    def row_total(self, mask):
        """fp64 [n] row totals over the genes of a per-time-point mask ([T, G] bool)."""
        mask = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        assert mask.shape == (self.T, self.G)
        out = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        _check(model_lib().spadot_pre_row_total(*self._csr(), _p(self.tp_off), self.T, self.G, _p(mask), self.n, _p(out),
                                                _stream()), "spadot_pre_row_total")
        return out

    def lognorm_stats(self, cols, total, target, t=None):
        """mean, std [T', S] of log1p(x * target / total) over the columns `cols` (time point t only when given)."""
        cols = torch.as_tensor(np.asarray(cols, dtype=np.int32), device=self.device)
        assert int(cols.numel()) == 0 or (int(cols.min()) >= 0 and int(cols.max()) < self.G)
        T = self.T if t is None else 1
        S = int(cols.numel())
        mean = torch.empty((T, S), dtype=torch.float64, device=self.device)
        std = torch.empty((T, S), dtype=torch.float64, device=self.device)
        _check(model_lib().spadot_pre_lognorm_stats(*self._csc(), _p(self._tp_slice(t)), T, S, _p(cols), _p(total),
                                                    float(target), _p(mean), _p(std), _stream()), "spadot_pre_lognorm_stats")
        return mean, std

    def scale_write(self, cols, total, target, mean, std, clip=0.0, t=None):
        """Dense float32 [rows of t (or all), S]: clip((log1p(x * target / total) - mean) / std)."""
        S = len(cols)
        colpos = np.full(self.G, -1, dtype=np.int32)
        colpos[np.asarray(cols, dtype=np.int64)] = np.arange(S, dtype=np.int32)
        colpos = torch.as_tensor(colpos, device=self.device)
        T = self.T if t is None else 1
        lo, hi = (0, self.n) if t is None else (int(self.tp_off_host[t]), int(self.tp_off_host[t + 1]))
        assert mean.shape == (T, S) and std.shape == (T, S)
        mean, std = mean.contiguous(), std.contiguous()
        out = torch.empty((hi - lo, S), dtype=torch.float32, device=self.device)
        _check(model_lib().spadot_pre_scale_write(*self._csr(), _p(self._tp_slice(t)), T, S, _p(colpos), _p(total),
                                                  float(target), _p(mean), _p(std), float(clip), hi - lo, _p(out), _stream()),
               "spadot_pre_scale_write")
        return out


def sparkx(dc, timings=None):
    """SPARK-X of every time point.  Returns one dict per time point: vst (bool [G], the SCTransform gene filter), spots (kept
    row indices into the permuted rows), genes (kept column indices, ascending), mom [Gt, 24], stat / pval [Gt, 11],
    combined [Gt], adjusted [Gt].  timings: a dict that receives the device milliseconds of the moments and p-value launches
    (tools/preprocess_time.py)."""
    dev = dc.device
    cnt, colsum = dc.gene_detect()
    vst = cnt >= MIN_CELLS                                        # [T, G]
    total = dc.row_total(vst)                                     # over the kept genes of each time point
    vst_h, colsum_h, total_h = vst.cpu().numpy(), colsum.cpu().numpy(), total.cpu().numpy()
    rowmap = np.full(dc.n, -1, dtype=np.int32)
    xts, invs, lams, nkeep, pair_t, pair_g, per = [], [], [], [], [], [], []
    off = 0
    for t in range(dc.T):
        lo, hi = int(dc.tp_off_host[t]), int(dc.tp_off_host[t + 1])
        spots = lo + np.flatnonzero(total_h[lo:hi] != 0)
        genes = np.flatnonzero(vst_h[t] & (colsum_h[t] != 0))
        xt, inv, lam = kernel_coordinates(dc.spatial[spots])
        rowmap[spots] = off + np.arange(spots.size, dtype=np.int32)
        off += spots.size
        xts.append(xt); invs.append(inv); lams.append(lam); nkeep.append(spots.size)
        pair_t.append(np.full(genes.size, t, dtype=np.int32)); pair_g.append(genes.astype(np.int32))
        per.append(dict(vst=vst_h[t], spots=spots, genes=genes, total=total))
    pt = torch.as_tensor(np.concatenate(pair_t), device=dev)
    pg = torch.as_tensor(np.concatenate(pair_g), device=dev)
    P = int(pt.numel())
    xt = torch.as_tensor(np.concatenate(xts), device=dev).contiguous()
    mom = torch.empty((P, 2 * N_KERNELS + 2), dtype=torch.float64, device=dev)
    # uploads are held by name: a temporary built inside the argument list is freed as soon as its data_ptr() is taken, and
    # the upload of a later argument of the same call can then reuse its block before the launch, so two arguments would
    # point at one buffer.  (Freeing a buffer after the launch is safe: later uploads are ordered behind it on the stream.)
    rowmap_d = torch.as_tensor(rowmap, device=dev)
    nkeep_d = torch.as_tensor(np.asarray(nkeep, dtype=np.int32), device=dev)
    inv_d = torch.as_tensor(np.stack(invs), device=dev).contiguous()
    lam_d = torch.as_tensor(np.stack(lams), device=dev).contiguous()
    lib = model_lib()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timings is not None else None
    if ev:
        ev[0].record()
    _check(lib.spadot_sparkx_moments(*dc._csc(), _p(dc.tp_off), P, _p(pt), _p(pg), _p(rowmap_d), _p(xt), _p(mom), _stream()),
           "spadot_sparkx_moments")
    if ev:
        ev[1].record()
    stat = torch.empty((P, N_KERNELS), dtype=torch.float64, device=dev)
    pval = torch.empty((P, N_KERNELS), dtype=torch.float64, device=dev)
    comb = torch.empty(P, dtype=torch.float64, device=dev)
    _check(lib.spadot_sparkx_pvals(_p(mom), P, _p(pt), _p(nkeep_d), _p(inv_d), _p(lam_d), PVAL_NODES, _p(stat), _p(pval),
                                   _p(comb), _stream()), "spadot_sparkx_pvals")
    if ev:
        ev[2].record()
        ev[2].synchronize()
        timings.update(moments_ms=ev[0].elapsed_time(ev[1]), pvals_ms=ev[1].elapsed_time(ev[2]), pairs=P)
    mom_h, stat_h, pval_h, comb_h = (x.cpu().numpy() for x in (mom, stat, pval, comb))
    a = 0
    for r in per:
        b = a + r["genes"].size
        r.update(mom=mom_h[a:b], stat=stat_h[a:b], pval=pval_h[a:b], combined=comb_h[a:b])
        r["adjusted"] = by_adjust(r["combined"])
        a = b
    return per


def cluster_genes(dc, t, genes, total, k=N_GENE_CLUSTERS, n_pcs=N_PCS):
    """K-means labels of the genes `genes` (column indices) of time point t: standardised log1p(x * 1e4 / total) over the
    time point's spots, clipped at +-sqrt(N/30) (SCTransform's clip range), N_PCS leading principal components of genes as
    points, KMeansDevice(k, random_state=1993, n_init=10).  The components come from an eigendecomposition on the device of
    the smaller Gram matrix, genes x genes or spots x spots (deterministic, no random draws)."""
    from .kmeans import KMeansDevice
    genes = np.asarray(genes)
    if genes.size == 0:
        return np.zeros(0, dtype=np.int64)
    n_t = int(dc.tp_off_host[t + 1] - dc.tp_off_host[t])
    mean, std = dc.lognorm_stats(genes, total, CLUSTER_TARGET, t=t)
    Z = dc.scale_write(genes, total, CLUSTER_TARGET, mean, std, clip=float(np.sqrt(n_t / 30.0)), t=t)   # [N_t, S]
    pcs = _pca_scores(Z.to(torch.float64).T, min(n_pcs, genes.size, n_t))                   # genes x spots -> genes x npc
    kk = min(k, genes.size)
    km = KMeansDevice(kk, random_state=1993, n_init=10).fit(pcs.contiguous())
    return np.asarray(km.labels_, dtype=np.int64)


def _pca_scores(M, npc):
    """The npc leading principal-component scores of the rows of M (fp64, centred per column here) from an eigendecomposition
    of the smaller Gram matrix, rows x rows or columns x columns (deterministic, no random draws)."""
    M = M - M.mean(0, keepdim=True)
    if M.shape[0] <= M.shape[1]:
        w, V = torch.linalg.eigh(M @ M.T)                  # ascending eigenvalues; scores = V sqrt(w)
        w, V = w.flip(0)[:npc], V.flip(1)[:, :npc]
        return V * w.clamp(min=0).sqrt()[None, :]
    w, U = torch.linalg.eigh(M.T @ M)                      # column-side vectors; scores = M U
    return M @ U.flip(1)[:, :npc]


def cluster_genes_louvain(dc, t, genes, sct, k=N_GENE_CLUSTERS, n_pcs=N_PCS_LOUVAIN, n_neighbors=N_NEIGHBORS):
    """_cluster_SVGs (SpaDOT/utils/_utils.py:195-221) on the genes `genes` (column indices) of time point t: their SCTransform
    scale.data rows (sct: the time point's SCTResult), the 30 leading principal components of genes as points, the
    Gaussian 100-NN graph and Louvain at resolution 1.0, + 0.1, ... until >= k communities.  Returns int64 labels (0 = the
    largest community)."""
    from .utils._sctransform_utils import cluster_by_resolution, gauss_knn_graph
    genes = np.asarray(genes)
    if genes.size == 0:
        return np.zeros(0, dtype=np.int64)
    M = sct.scale_data(genes)                                                      # [S, N] fp64 on the device
    pcs = _pca_scores(M, min(n_pcs, genes.size, M.shape[1]))
    W = gauss_knn_graph(pcs, n_neighbors)
    labels, _ = cluster_by_resolution(W, k)
    return labels


def scale_output(dc, cols):
    """Step 4 on the columns `cols`: per time point normalize_total(target_sum=1e-4) over those columns, log1p, scale."""
    mask = np.zeros((dc.T, dc.G), dtype=bool)
    mask[:, np.asarray(cols, dtype=np.int64)] = True
    total = dc.row_total(mask)
    mean, std = dc.lognorm_stats(cols, total, TARGET_SUM)
    return dc.scale_write(cols, total, TARGET_SUM, mean, std)


def preprocess_counts(raw, feature_selection=True, device="cuda:0", output_dir=None, cluster=True, gene_clusters="kmeans"):
    """The whole stage on a RawCounts.  Returns a dict: X (float32 [n, S] numpy), genes, cols (column indices), timepoint,
    spatial, perm (input row of each output row), counts (scipy CSR of the raw counts of `cols`), tps, and with feature
    selection the per-time-point SPARK-X results `sparkx` and SVG tables `tables` (genes, combinedPval, adjustedPval,
    cluster).  gene_clusters: 'kmeans' (cluster_genes, the default) or 'louvain' (SCTransform of each time point, then
    cluster_genes_louvain; the SCTResults are returned as `sct`).  Writes the per-time-point CSVs and SVG_genes.txt into
    output_dir when given."""
    if gene_clusters not in GENE_CLUSTERS:
        raise ValueError(f"gene_clusters must be one of {GENE_CLUSTERS}, not {gene_clusters!r}")
    dc = DeviceCounts(raw, device)
    out = dict(tps=dc.tps, timepoint=dc.timepoint, spatial=dc.spatial, perm=dc.perm)
    if feature_selection:
        per = sparkx(dc)
        tables = []
        for t, r in enumerate(per):
            order, n_keep = rank_genes(r["adjusted"], r["combined"])
            sel = order[:n_keep]
            cols = r["genes"][sel]
            if not cluster:
                clus = np.zeros(cols.size, dtype=np.int64)
            elif gene_clusters == "louvain":
                sct = sctransform(dc, t)
                clus = cluster_genes_louvain(dc, t, cols, sct)
                r["sct"] = sct
            else:
                clus = cluster_genes(dc, t, cols, r["total"])
            r.update(selected=cols, cluster=clus)
            tables.append((dc.genes[cols], r["combined"][sel], r["adjusted"][sel], clus))
            if output_dir:
                import pandas as pd
                pd.DataFrame({"combinedPval": r["combined"][sel], "adjustedPval": r["adjusted"][sel], "cluster": clus},
                             index=dc.genes[cols]).to_csv(os.path.join(output_dir, str(dc.tps[t]) + CSV_SUFFIX))
        svgs = select_svgs([(g, a, c) for g, _, a, c in tables])
        pos = {g: i for i, g in enumerate(dc.genes.tolist())}
        cols = np.asarray([pos[g] for g in svgs], dtype=np.int64)
        if output_dir:
            with open(os.path.join(output_dir, "SVG_genes.txt"), "w") as f:
                for g in svgs:
                    f.write("%s\n" % g)
        out.update(sparkx=per, tables=tables)
    else:
        cols = np.arange(dc.G, dtype=np.int64)
    X = scale_output(dc, cols).cpu().numpy()
    out.update(X=X, cols=cols, genes=dc.genes[cols], counts=dc.X[:, cols].tocsr())
    return out


def _write_h5ad(path, res):
    try:
        import anndata
        import pandas as pd
    except ImportError:
        return False
    ad = anndata.AnnData(X=res["X"], obs=pd.DataFrame({"timepoint": res["timepoint"]}),
                         var=pd.DataFrame(index=res["genes"]))
    ad.obsm["spatial"] = res["spatial"]
    ad.layers["counts"] = res["counts"]
    ad.write_h5ad(path)
    return True


def preprocess(args):
    """SpaDOT.preprocess: reads args.data, writes {prefix}{stem}.npz (X, timepoint, spatial, genes and the selected genes' raw
    counts as counts_data / counts_indices / counts_indptr / counts_shape; readable by load_data, so by train), with anndata
    also {prefix}{stem}.h5ad, and with feature selection SVG_genes.txt and {tp}_SVG_sparkx_clustered_louvain.csv.
    Returns the result dict of preprocess_counts."""
    raw, path = load_counts(args.data)
    open_output(args, path)                               # this stage has a default prefix of its own
    prefix = getattr(args, "prefix", "preprocessed_")
    prefix = "" if prefix is None else prefix
    device = getattr(args, "device", None) or "cuda:0"
    fs = bool(getattr(args, "feature_selection", True))
    gc = getattr(args, "gene_clusters", None) or "kmeans"
    res = preprocess_counts(raw, feature_selection=fs, device=device, output_dir=args.output_dir, gene_clusters=gc)
    stem = os.path.splitext(os.path.basename(path))[0] if path else "data"
    c = res["counts"]
    np.savez(os.path.join(args.output_dir, prefix + stem + ".npz"), X=res["X"], timepoint=res["timepoint"],
             spatial=res["spatial"], genes=np.asarray(res["genes"]).astype(str), counts_data=c.data, counts_indices=c.indices,
             counts_indptr=c.indptr, counts_shape=np.asarray(c.shape, dtype=np.int64))
    _write_h5ad(os.path.join(args.output_dir, prefix + stem + ".h5ad"), res)
    print(f"preprocess: {res['X'].shape[0]} spots x {res['X'].shape[1]} genes written to {args.output_dir}", file=sys.stderr)
    return res
