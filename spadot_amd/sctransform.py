"""SCTransform on the MI355X: mirror of SpaDOT/utils/sctransform (SCTransform -> vst -> ScaleData) as the reference's preprocess
stage calls it (_preprocess_utils.py:81-103: n_cells=None, variable_features_n=None, variable_features_rv_th=1.3,
return_only_var_genes=False), per time point.

    sctransform(dc, t)                    one time point of a DeviceCounts: an SCTResult
    SCTransform(umi, genes, cells, ...)   the reference's signature on a genes x cells matrix: (assay_out, vst_out)

Per time point: umi_j = the spot's total over all genes, log_umi = log10(umi); the genes with a count >= 0.01 in >= 5 spots;
log10 of the geometric mean (eps 1); at most 2000 step-1 genes; per step-1 gene the Poisson fit of y ~ 1 + log_umi and
theta.ml (k_sct_fit: one wavefront per gene, fp64); the od_factor regularisation (outliers, bw.SJ, ksmooth: host helpers of
utils/_sctransform_utils.py); the Pearson residuals of every kept gene clipped at +-sqrt(N) with their mean and variance
(k_sct_resid_stats); and scale.data = clip(r, +-sqrt(N/30)) - float32(row mean), written on the device for the rows asked
for (k_sct_resid_write).  The dense residual matrix of all genes is never formed.

Deviations from the reference:
  * spots whose total over all genes is zero are left out (with log_umi = -inf the reference's fits are NaN for every gene);
  * when more than 2000 genes pass the filter, the step-1 weights come from an exact Gaussian KDE at the points with KDEpy's
    Silverman bandwidth, not KDEpy's FFT grid and linear interpolation, so the step-1 set can differ from the reference's;
  * the gene clusters (preprocess.cluster_genes_louvain): the PCA is an fp64 eigendecomposition (scanpy: float32 arpack;
    only the 30-component subspace matters), and the Louvain node order and tie rule are ours, not louvain-igraph's; the
    resolution loop stops with an error past resolution 100 and targets min(10, S) communities for S genes.
Quirks kept: `fitted` is the Poisson mean before the last coefficient update; theta is not clamped at min_theta (the
reference's chained assignment is a no-op); ScaleData subtracts the float32-rounded row mean in fp64."""
import numpy as np
import torch

from ._call import launched as _check, ptr as _p, stream as _stream
from ._lib import model_lib
from .utils._sctransform_utils import regularize, sample_step1

MIN_CELLS = 5
DETECT_THRESHOLD = 0.01
N_GENES = 2000
SEED = 1448145
POIS_TOL, POIS_MAXIT = 1e-9, 100          # qpois_reg(..., 1e-9, 100, ...)
THETA_LIMIT, THETA_EPS = 10, 0.0001220703  # theta_ml(limit=10, eps=...)
BW_ADJUST = 3
RV_TH = 1.3


class SCTResult:
    """SCTransform of one time point.  spots: kept rows (into the DeviceCounts' permuted rows), genes: kept columns
    (ascending), log_umi [N], log_gmean [G], step1 (positions into genes), model_pars [G1, 3], outliers [G1],
    model_pars_fit [G, 3] (columns PARS = theta, Intercept, log_umi), gene_attr (dict of [G] arrays: detection_rate, gmean,
    amean, variance, residual_mean, residual_variance), fit_info [G1, 5] (fitted b0, b1, Poisson iterations, theta
    iterations, sum y).  scale_data(cols) returns the device fp64 [len(cols), N] scale.data rows of the columns cols."""

    def __init__(self, dc, t, **kw):
        self.dc, self.t = dc, t
        self.__dict__.update(kw)

    @property
    def N(self):
        return int(self.spots.size)

    def top_features(self, rv_th=RV_TH):
        """The genes (column indices) with residual variance >= rv_th, by residual variance descending (stable)."""
        rv = self.gene_attr["residual_variance"]
        o = np.argsort(-rv, kind="stable")
        return self.genes[o[rv[o] >= rv_th]]

    def scale_data(self, cols):
        dc = self.dc
        cols = np.asarray(cols, dtype=np.int64)
        pos = np.searchsorted(self.genes, cols)
        if cols.size and (pos.max() >= self.genes.size or np.any(self.genes[np.minimum(pos, self.genes.size - 1)] != cols)):
            raise ValueError("scale_data: every column must be a kept gene of the time point")
        S, N = int(cols.size), self.N
        out = torch.empty((S, N), dtype=torch.float64, device=dc.device)
        if S == 0:
            return out
        pars = torch.as_tensor(np.ascontiguousarray(self.model_pars_fit[pos]), device=dc.device)
        center = self.gene_attr["scale_mean"][pos].astype(np.float32).astype(np.float64)
        center_d = torch.as_tensor(center, device=dc.device)
        genes_d = torch.as_tensor(cols.astype(np.int32), device=dc.device)
        _check(model_lib().spadot_sct_resid_write(*dc._csc(), _p(dc.tp_off), self.t, S, _p(genes_d), _p(self._lur),
                                                  _p(self._lu), _p(self._krow), _p(self._rowmap), N, _p(pars), _p(center_d),
                                                  float(np.sqrt(N / 30.0)), _p(out), _stream()), "spadot_sct_resid_write")
        return out


def sctransform(dc, t, n_genes=N_GENES, seed=SEED, min_cells=MIN_CELLS, bw_adjust=BW_ADJUST, timings=None):
    """SCTransform of time point t of the DeviceCounts dc (see the module docstring).  timings: a dict that receives the device
    milliseconds of the four launches (tools/sctransform_time.py)."""
    dev = dc.device
    lib = model_lib()
    lo, hi = int(dc.tp_off_host[t]), int(dc.tp_off_host[t + 1])
    umi = dc.row_total(np.ones((dc.T, dc.G), dtype=bool))[lo:hi].cpu().numpy()
    keep = np.flatnonzero(umi > 0)
    spots = lo + keep
    N = int(keep.size)
    if N < 2:
        raise ValueError(f"time point {dc.tps[t]!r}: SCTransform needs at least two spots with counts")
    log_umi = np.log10(umi[keep])
    lur = np.zeros(dc.n)
    lur[spots] = log_umi
    rowmap = np.full(dc.n, -1, dtype=np.int32)
    rowmap[spots] = np.arange(N, dtype=np.int32)
    # uploads are held by name (see preprocess.sparkx)
    lur_d = torch.as_tensor(lur, device=dev)
    lu_d = torch.as_tensor(log_umi, device=dev)
    krow_d = torch.as_tensor(spots.astype(np.int32), device=dev)
    rowmap_d = torch.as_tensor(rowmap, device=dev)
    cnt, _ = dc.gene_detect(DETECT_THRESHOLD)
    cnt_t = cnt[t].cpu().numpy()
    genes = np.flatnonzero(cnt_t >= min_cells)
    G = int(genes.size)
    if G == 0:
        raise ValueError(f"time point {dc.tps[t]!r}: no gene is detected in {min_cells} spots")
    genes_d = torch.as_tensor(genes.astype(np.int32), device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timings is not None else None

    if ev:
        ev[0].record()
    st = torch.empty((G, 3), dtype=torch.float64, device=dev)
    _check(lib.spadot_sct_gene_stats(*dc._csc(), _p(dc.tp_off), t, G, _p(genes_d), N, _p(st), _stream()),
           "spadot_sct_gene_stats")
    if ev:
        ev[1].record()
    st = st.cpu().numpy()
    log_gmean = np.log10(np.exp(st[:, 0] / N) - 1)
    step1 = sample_step1(log_gmean, n_genes, seed)
    G1 = int(step1.size)
    g1_d = torch.as_tensor(genes[step1].astype(np.int32), device=dev)
    fit = torch.empty((G1, 8), dtype=torch.float64, device=dev)
    if ev:
        ev[2].record()
    _check(lib.spadot_sct_fit(*dc._csc(), _p(dc.tp_off), t, G1, _p(g1_d), _p(lur_d), _p(lu_d), N, POIS_TOL, POIS_MAXIT,
                              THETA_LIMIT, THETA_EPS, _p(fit), _stream()), "spadot_sct_fit")
    if ev:
        ev[3].record()
        ev[3].synchronize()
        timings.update(gene_stats_ms=ev[0].elapsed_time(ev[1]), fit_ms=ev[2].elapsed_time(ev[3]), step1_genes=G1, kept_genes=G,
                       spots=N)
    fit = fit.cpu().numpy()
    model_pars = np.ascontiguousarray(fit[:, :3])
    model_pars_fit, outliers = regularize(model_pars, log_gmean[step1], log_gmean, bw_adjust)

    pars_d = torch.as_tensor(np.ascontiguousarray(model_pars_fit), device=dev)
    rs = torch.empty((G, 3), dtype=torch.float64, device=dev)
    ev2 = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timings is not None else None
    if ev2:
        ev2[0].record()
    _check(lib.spadot_sct_resid_stats(*dc._csc(), _p(dc.tp_off), t, G, _p(genes_d), _p(lur_d), _p(lu_d), N, _p(pars_d),
                                      float(np.sqrt(N)), float(np.sqrt(N / 30.0)), _p(rs), _stream()), "spadot_sct_resid_stats")
    if ev2:
        ev2[1].record()
        ev2[1].synchronize()
        timings.update(resid_stats_ms=ev2[0].elapsed_time(ev2[1]))
    rs = rs.cpu().numpy()
    amean = st[:, 1] / N
    gene_attr = dict(detection_rate=cnt_t[genes] / N, gmean=np.power(10, log_gmean), amean=amean,
                     variance=st[:, 2] / (N - 1), residual_mean=rs[:, 0], residual_variance=rs[:, 1], scale_mean=rs[:, 2])
    return SCTResult(dc, t, spots=spots, genes=genes, log_umi=log_umi, log_gmean=log_gmean, step1=step1,
                     model_pars=model_pars, outliers=outliers, model_pars_fit=model_pars_fit, gene_attr=gene_attr,
                     fit_info=fit[:, 3:], _lur=lur_d, _lu=lu_d, _krow=krow_d, _rowmap=rowmap_d)


def SCTransform(umi, genes, cells, reference_sct_model=None, do_correct_umi=False, n_cells=None, residual_features=None,
                variable_features_n=None, variable_features_rv_th=RV_TH, vars_to_regress=None, do_scale=False, do_center=True,
                conserve_memory=False, return_only_var_genes=False, seed_use=SEED, device="cuda:0", **kwargs):
    """SpaDOT/utils/sctransform/sctransform.py's SCTransform on a genes x cells count matrix, for the settings the reference's
    preprocess uses.  Returns (assay_out, vst_out): assay_out['scale.data'] is a DataFrame genes x cells (the kept genes, the
    cells with a non-zero total); vst_out holds model_pars, model_outlier, model_pars_fit, gene_attr (DataFrames indexed by
    gene), top_features and the SCTResult as 'result'.  Other settings raise NotImplementedError."""
    import pandas as pd
    import scipy.sparse as sp
    from .preprocess import DeviceCounts
    from .utils._preprocess_utils import RawCounts
    if reference_sct_model is not None or residual_features is not None or conserve_memory or vars_to_regress:
        raise NotImplementedError("only the default SCTransform method is available")
    if "batch_var" in kwargs or kwargs.get("method", "poisson") != "poisson" or kwargs.get("vst_flavor") is not None:
        raise NotImplementedError("only method='poisson' without batch_var or vst_flavor is available")
    if n_cells is not None or variable_features_n is not None or return_only_var_genes or do_correct_umi or do_scale or \
            not do_center:
        raise NotImplementedError("only n_cells=None, variable_features_n=None, return_only_var_genes=False, "
                                  "do_correct_umi=False, do_scale=False and do_center=True are available")
    genes = np.asarray(genes).astype(str)
    cells = np.asarray(cells).astype(str)
    X = sp.csr_matrix(sp.csr_matrix(umi).T, dtype=np.float32)       # cells x genes
    raw = RawCounts(X, np.zeros(X.shape[0], dtype=np.int64), np.zeros((X.shape[0], 2)), genes)
    dc = DeviceCounts(raw, device)
    r = sctransform(dc, 0, n_genes=kwargs.get("n_genes", N_GENES), seed=seed_use,
                    min_cells=kwargs.get("min_cells", MIN_CELLS), bw_adjust=kwargs.get("bw_adjust", BW_ADJUST))
    gk, ck = genes[r.genes], cells[dc.perm[r.spots]]
    cols = ["theta", "Intercept", "log_umi"]
    model_pars = pd.DataFrame(r.model_pars, index=gk[r.step1], columns=cols)
    model_pars_fit = pd.DataFrame(r.model_pars_fit[:, [1, 2, 0]], index=gk, columns=["Intercept", "log_umi", "theta"])
    gene_attr = pd.DataFrame({k: v for k, v in r.gene_attr.items() if k != "scale_mean"}, index=gk)
    top = genes[r.top_features(variable_features_rv_th)]
    block = r.scale_data(r.genes).cpu().numpy()
    assay_out = {"counts": umi, "data": None, "scale.data": pd.DataFrame(block, index=gk, columns=ck)}
    vst_out = {"model_str": "y ~ log_umi", "model_pars": model_pars, "model_outlier": pd.DataFrame(r.outliers, index=gk[r.step1]),
               "model_pars_fit": model_pars_fit, "gene_attr": gene_attr, "top_features": top,
               "genes_log_gmean_step1": pd.Series(r.log_gmean[r.step1], index=gk[r.step1]), "umi_genes": gk, "umi_cells": ck,
               "result": r}
    return assay_out, vst_out
