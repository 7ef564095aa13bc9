"""fp64 numpy / scipy restatement of the reference's preprocess stage, the parity oracle of tests/test_preprocess_*.py (the
reference module itself needs scanpy, anndata, chi2comb, statsmodels, ... at import time).  Line numbers refer to
SpaDOT/utils/_utils.py (SPARK-X), SpaDOT/utils/_preprocess_utils.py and SpaDOT/utils/sctransform/vst.py of the reference.
Written without the package's own helpers, so that the tests compare two independent statements."""
import numpy as np
import scipy.sparse as sp
from scipy import integrate
from scipy.stats import cauchy, ncx2


def gene_filter(counts, min_cells=5):
    """vst.py:71-75: genes with a count >= 0.01 in at least min_cells spots (column indices)."""
    return np.flatnonzero(np.asarray((counts >= 0.01).sum(0)).ravel() >= min_cells)


def transloc_func_vec(coord, lker, transfunc="gaussian"):
    """_utils.py:394-414."""
    coord = coord - np.mean(coord, axis=0)
    l = np.quantile(np.abs(coord), q=np.arange(0.2, 1.01, 0.2), axis=0)
    if transfunc == "gaussian":
        return np.exp(-coord ** 2 / (2 * l[lker, :][np.newaxis, :] ** 2))
    return np.cos(2 * np.pi * coord / l[lker, :][np.newaxis, :])


def sparkx_sk(counts, infomat):
    """_utils.py:230-261 without the p-values: stat, ylam, Klam, and the moments EHL, sum y, sum y^2."""
    X = infomat - infomat.mean(axis=0, keepdims=True)
    XtX = X.T @ X
    loc_inv = np.linalg.inv(XtX)
    klam = np.linalg.eigvalsh(X.T @ (X @ loc_inv))
    ehl = np.asarray(counts.T @ X)
    n = X.shape[0]
    syy = np.asarray(counts.power(2).sum(axis=0)).ravel()
    sy = np.asarray(counts.sum(axis=0)).ravel()
    stat = np.einsum("ij,jk,ik->i", ehl, loc_inv, ehl) * n / syy
    ybar = sy / n
    ylam = 1 - n * ybar ** 2 / syy
    return dict(stat=stat, ylam=ylam, klam=klam, ehl=ehl, sy=sy, syy=syy)


def sf_two_term(q, l1, l2):
    """P[l1 X1 + l2 X2 > q] for independent chi^2_1: exp(-q / (2 l)) for equal weights, else the integral
    (1/pi) int_0^pi exp(-q / (2 (l1 cos^2 + l2 sin^2))) by adaptive quadrature."""
    if q <= 0:
        return 1.0
    if l1 == l2 or abs(l1 - l2) <= 1e-13 * max(abs(l1), abs(l2)):
        return float(np.exp(-q / (l1 + l2)))
    f = lambda th: np.exp(-q / (2 * (l1 * np.cos(th) ** 2 + l2 * np.sin(th) ** 2)))
    return integrate.quad(f, 0, np.pi, epsabs=0, epsrel=1e-13, limit=200)[0] / np.pi


def liu(q, lambdas):
    """_utils.py:291-373 (CompQuadForm's liu) for central chi^2_1 terms, via scipy.stats.ncx2."""
    lam = np.asarray(lambdas, dtype=np.float64)
    c1, c2, c3, c4 = (np.sum(lam ** k) for k in (1, 2, 3, 4))
    s1, s2 = c3 / c2 ** 1.5, c4 / c2 ** 2
    tstar = (q - c1) / np.sqrt(2 * c2)
    if s1 ** 2 > s2:
        a = 1 / (s1 - np.sqrt(s1 ** 2 - s2))
        delta = s1 * a ** 3 - a ** 2
        l = a ** 2 - 2 * delta
    else:
        a, delta, l = 1 / s1, 0.0, c2 ** 3 / c3 ** 2
    return float(ncx2.sf(tstar * np.sqrt(2) * a + l + delta, df=l, nc=delta))


def acat(p):
    """_utils.py:376-392 with equal weights; the sums in index order."""
    p = np.asarray(p, dtype=np.float64)
    if np.any(p == 0):
        return 0.0
    if np.any(p == 1):
        return 1.0
    w = 1.0 / p.size
    small = p < 1e-16
    s = 0.0
    for v in p[small]:
        s += w / (np.pi * v)
    r = 0.0
    for v in p[~small]:
        r += w * np.tan((0.5 - v) * np.pi)
    cct = s + r if small.any() else r
    return 1 / (cct * np.pi) if cct > 1e15 else 1 - cauchy.cdf(cct)


def fdr_by(p):
    """statsmodels multipletests(p, method='fdr_by')[1], written out."""
    p = np.asarray(p, dtype=np.float64)
    n = p.size
    o = np.argsort(p, kind="mergesort")
    cm = sum(1.0 / k for k in range(1, n + 1))
    raw = p[o] * n * cm / np.arange(1, n + 1)
    adj = np.minimum(np.minimum.accumulate(raw[::-1])[::-1], 1.0)
    out = np.empty(n)
    out[o] = adj
    return out


def sparkx(counts, location):
    """_utils.py:121-191 on one time point after the SCTransform gene filter: counts (scipy sparse, spots x kept genes, fp64),
    location (spots x 2).  Returns the kept spots / genes (indices into the input), moments, the 11 statistics and p-values,
    ACAT, BY and the selected genes (indices into the input) in order."""
    counts = sp.csr_matrix(counts, dtype=np.float64)
    keep_cell = np.flatnonzero(np.asarray(counts.sum(axis=1)).ravel() != 0)
    counts = counts[keep_cell]
    location = location[keep_cell]
    keep_gene = np.flatnonzero(np.asarray(counts.sum(axis=0)).ravel() != 0)
    counts = sp.csc_matrix(counts[:, keep_gene])
    sets = [location] + [transloc_func_vec(location, k, "gaussian") for k in range(5)] + \
        [transloc_func_vec(location, k, "cosine") for k in range(5)]
    res = [sparkx_sk(counts, s) for s in sets]
    stat = np.column_stack([r["stat"] for r in res])
    pval = np.empty_like(stat)
    for k, r in enumerate(res):
        for i in range(stat.shape[0]):
            lam = r["ylam"][i] * r["klam"]
            pval[i, k] = sf_two_term(stat[i, k], lam[0], lam[1]) if r["ylam"][i] > 0 else 1.0
    comb = np.array([acat(row) for row in pval])
    adj = fdr_by(comb)
    order = np.lexsort((np.arange(adj.size), comb, adj))
    n_keep = min(adj.size, max(int((adj <= 0.05).sum()), 500))
    return dict(spots=keep_cell, genes=keep_gene, sy=res[0]["sy"], syy=res[0]["syy"],
                ehl=np.concatenate([r["ehl"] for r in res], axis=1), stat=stat, pval=pval, combined=comb, adjusted=adj,
                selected=keep_gene[order[:n_keep]])


def log_stats(counts, target=1e-4):
    """normalize_total(target_sum) over the given columns and log1p on one time point, fp64 dense: (v, mean, std with ddof 1
    and std 0 -> 1; a single row has std 0 as well, not numpy's NaN)."""
    x = np.asarray(sp.csr_matrix(counts, dtype=np.float64).todense())
    tot = x.sum(1, keepdims=True)
    v = np.log1p(np.divide(x * target, tot, out=np.zeros_like(x), where=tot > 0))
    mu = v.mean(0)
    sd = v.std(0, ddof=1) if v.shape[0] > 1 else np.zeros(v.shape[1])
    sd[sd == 0] = 1
    return v, mu, sd


def normalize_log_scale(counts, target=1e-4, clip=None):
    """_preprocess_utils.py:31-49 on one time point: normalize_total(target_sum) over the given columns, log1p, scale (ddof
    1, std 0 -> 1), fp64; clip: symmetric clip after scaling (None: none)."""
    v, mu, sd = log_stats(counts, target)
    z = (v - mu) / sd
    return np.clip(z, -clip, clip) if clip else z
