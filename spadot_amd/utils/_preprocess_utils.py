"""Host helpers of the preprocess stage: mirror of the pure-host parts of SpaDOT/utils/_preprocess_utils.py and of SPARK-X in
SpaDOT/utils/_utils.py.  Everything here is small (G values per time point, N x 2 coordinates) and runs in numpy, so the CPU
suite tests it directly; the per-gene work runs on the device (spadot_amd/preprocess.py, csrc/preprocess.hip).

    load_counts         the raw-count reader (.npz, .h5ad with anndata, or an in-memory object) with the reference's checks
    timepoint_order     adata.obs['timepoint'].unique(): order of first appearance
    transloc            _transloc_func_vec (_utils.py:394-414)
    kernel_coordinates  the 11 centred coordinate sets of _sparkx / _sparkx_sk, with their 2 x 2 inverses and eigenvalues
    acat                _ACAT (_utils.py:376-392) with equal weights
    by_adjust           multipletests(p, method='fdr_by')[1]
    rank_genes          the order of sort_values('adjustedPval') with a defined tie order, and the SPARK-X selection count
    select_svgs         _get_SVGs (_preprocess_utils.py:52-79): the balancing rule across time points"""
import os

import numpy as np

N_KERNELS = 11


class RawCounts:
    """Raw counts as the preprocess stage reads them: X (scipy CSR float32, spots x genes, non-negative), obs['timepoint'],
    obsm['spatial'] (float64, N x 2), var_names (gene names as strings)."""

    def __init__(self, X, timepoint, spatial, var_names):
        self.X = X
        self.obs = {"timepoint": np.asarray(timepoint)}
        self.obsm = {"spatial": spatial}
        self.var_names = np.asarray(var_names).astype(str)
        self.n_obs, self.n_vars = X.shape


def _check_inputs(obs_has_tp, spatial):
    # preprocess.py:21-28 of the reference, with its messages
    if not obs_has_tp:
        raise ValueError("The `timepoint` column is not found in adata.obs. Please make sure timepoint information is given.")
    if spatial is None:
        raise ValueError("The `spatial` key is not found in adata.obsm. Please make sure spatial coordinates are provided.")
    if not isinstance(spatial, np.ndarray) or spatial.ndim != 2:
        raise ValueError("The `spatial` key in adata.obsm is not a 2D numpy array. Please make sure spatial coordinates are "
                         "correctly provided.")


def _to_csr(X):
    import scipy.sparse as sp
    X = sp.csr_matrix(X, dtype=np.float32) if not sp.issparse(X) else sp.csr_matrix(X).astype(np.float32)
    X.sum_duplicates()
    X.eliminate_zeros()
    X.sort_indices()
    if X.nnz and float(X.data.min()) < 0:
        raise ValueError("the count matrix has negative entries: the preprocess stage reads raw counts")
    return X


def load_counts(data):
    """The input of the preprocess stage: a path to an .npz (timepoint, spatial, optional genes, and the counts as X (dense)
    or X_data / X_indices / X_indptr / X_shape (CSR)), a path to an .h5ad (needs `anndata`), or an in-memory object with .X
    (dense or scipy sparse), .obs['timepoint'], .obsm['spatial'] and optionally .var_names.  Returns (RawCounts, absolute path
    or None)."""
    path = None
    if isinstance(data, (str, os.PathLike)):
        path = os.path.abspath(data)
        if path.endswith(".npz"):
            import scipy.sparse as sp
            z = np.load(path, allow_pickle=False)
            if "X" in z.files:
                X = z["X"]
            else:
                X = sp.csr_matrix((z["X_data"], z["X_indices"], z["X_indptr"]), shape=tuple(int(v) for v in z["X_shape"]))
            _check_inputs("timepoint" in z.files, z["spatial"] if "spatial" in z.files else None)
            genes = z["genes"] if "genes" in z.files else np.arange(X.shape[1]).astype(str)
            return RawCounts(_to_csr(X), z["timepoint"], np.asarray(z["spatial"], dtype=np.float64), genes), path
        try:
            import anndata
        except ImportError as e:
            raise ImportError("reading .h5ad needs the `anndata` package (as the reference does); alternatively pass an .npz "
                              "with the counts, timepoint and spatial") from e
        data = anndata.read_h5ad(path)
    obs = data.obs
    has_tp = ("timepoint" in obs.columns) if hasattr(obs, "columns") else ("timepoint" in obs)
    obsm = data.obsm
    spatial = obsm["spatial"] if "spatial" in obsm.keys() else None
    _check_inputs(has_tp, spatial)
    genes = getattr(data, "var_names", None)
    if genes is None:
        genes = np.arange(data.X.shape[1]).astype(str)
    return RawCounts(_to_csr(data.X), np.asarray(obs["timepoint"]), np.asarray(spatial, dtype=np.float64), genes), path


def timepoint_order(timepoint):
    """The distinct time points in order of first appearance (pandas' unique())."""
    tp = np.asarray(timepoint)
    _, first = np.unique(tp, return_index=True)
    return [tp[i] for i in np.sort(first)]


def transloc(coord, lker, transfunc="gaussian"):
    """_transloc_func_vec: centre, per-column quantiles 0.2 .. 1.0 of |coord|, then a Gaussian or cosine transform."""
    coord = coord - np.mean(coord, axis=0)
    probs = np.arange(0.2, 1.01, 0.2)
    l = np.quantile(np.abs(coord), q=probs, axis=0)
    if transfunc == "gaussian":
        return np.exp(-coord ** 2 / (2 * l[lker, :][np.newaxis, :] ** 2))
    if transfunc == "cosine":
        return np.cos(2 * np.pi * coord / l[lker, :][np.newaxis, :])
    raise ValueError("transfunc must be 'gaussian' or 'cosine'")


def kernel_coordinates(location):
    """The 11 coordinate sets of SPARK-X's mixture option over the kept spots (projection, Gaussian 1-5, cosine 1-5), each
    centred as _sparkx_sk does.  Returns xt [N, 22] (set k in columns 2k, 2k+1), inv [11, 4] ((X^T X)^-1 row-major) and
    lam [11, 2] (eigvalsh of X^T X (X^T X)^-1, the Klam of _sparkx_sk)."""
    location = np.asarray(location, dtype=np.float64)
    sets = [location] + [transloc(location, k, "gaussian") for k in range(5)] + [transloc(location, k, "cosine")
                                                                               for k in range(5)]
    xt = np.empty((location.shape[0], 2 * N_KERNELS), dtype=np.float64)
    inv = np.empty((N_KERNELS, 4), dtype=np.float64)
    lam = np.empty((N_KERNELS, 2), dtype=np.float64)
    for k, s in enumerate(sets):
        xc = s - s.mean(axis=0, keepdims=True)
        a = np.linalg.inv(xc.T @ xc)
        xt[:, 2 * k:2 * k + 2] = xc
        inv[k] = a.ravel()
        lam[k] = np.linalg.eigvalsh(xc.T @ (xc @ a))
    return xt, inv, lam


def acat(pvals):
    """_ACAT with equal weights.  Raises like the reference on NaN, out-of-range or a mix of 0 and 1."""
    p = np.asarray(pvals, dtype=np.float64)
    if np.any(np.isnan(p)):
        raise ValueError("Cannot have NAs in the p-values!")
    if np.any(p < 0) or np.any(p > 1):
        raise ValueError("P-values must be between 0 and 1!")
    is_zero, is_one = bool(np.any(p == 0)), bool(np.any(p == 1))
    if is_zero and is_one:
        raise ValueError("Cannot have both 0 and 1 p-values!")
    if is_zero:
        return 0.0
    if is_one:
        return 1.0
    w = 1.0 / p.size
    small = p < 1e-16
    cct = 0.0
    if not small.any():
        for v in p:
            cct += w * np.tan((0.5 - v) * np.pi)
    else:
        s = 0.0
        for v in p[small]:
            s += w / (np.pi * v)
        r = 0.0
        for v in p[~small]:
            r += w * np.tan((0.5 - v) * np.pi)
        cct = s + r
    if cct > 1e15:
        return 1.0 / (cct * np.pi)
    return 1.0 - (0.5 + np.arctan(cct) / np.pi)


def by_adjust(p):
    """Benjamini-Yekutieli adjusted p-values, as statsmodels' multipletests(p, method='fdr_by')[1]."""
    p = np.asarray(p, dtype=np.float64)
    n = p.size
    if n == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    i = np.arange(1, n + 1, dtype=np.float64)
    cm = np.sum(1.0 / i)
    raw = p[order] / (i / n / cm)
    adj = np.minimum.accumulate(raw[::-1])[::-1]
    adj[adj > 1] = 1
    out = np.empty(n, dtype=np.float64)
    out[order] = adj
    return out


def rank_genes(adjusted, combined):
    """Order of the genes by adjusted p, ties by combined p, then by column order (pandas' default sort, which the reference
    uses, is unstable, so its tie order is undefined), and SPARK-X's selection count min(G, max(#(adj <= 0.05), 500))."""
    adjusted = np.asarray(adjusted, dtype=np.float64)
    order = np.lexsort((np.arange(adjusted.size), np.asarray(combined, dtype=np.float64), adjusted))
    n_keep = min(adjusted.size, max(int((adjusted <= 0.05).sum()), 500))
    return order, n_keep


def select_svgs(tables):
    """_get_SVGs.  tables: one (genes, adjusted, cluster) triple per time point, in time point order, each already in SPARK-X
    order (rank_genes).  The time point with the fewest SVGs is taken whole (the first one on ties); from every other one the
    top max(100, round(min_len / n_clusters)) genes of each cluster by adjusted p (round: half to even, as Python's).
    Returns the sorted union of gene names."""
    lens = [len(t[0]) for t in tables]
    min_idx = min(range(len(tables)), key=lambda i: lens[i])
    min_len = lens[min_idx]
    out = set(np.asarray(tables[min_idx][0]).astype(str).tolist())
    for idx, (genes, adjusted, cluster) in enumerate(tables):
        if idx == min_idx:
            continue
        genes = np.asarray(genes).astype(str)
        cluster = np.asarray(cluster)
        quota = max(100, round(min_len / len(set(cluster.tolist()))))
        order = np.argsort(np.asarray(adjusted, dtype=np.float64), kind="stable")
        taken = {}
        for i in order:
            c = cluster[i]
            if taken.get(c, 0) < quota:
                taken[c] = taken.get(c, 0) + 1
                out.add(genes[i])
    return sorted(out)
