"""An fp64 numpy / scipy / pandas restatement of the reference's SCTransform and gene clusters (steps 1-9 of the SCTransform
issue), written without the package's helpers so that the GPU tests compare two independent statements.  Line numbers are
SpaDOT/utils/sctransform/{vst,sctransform_utils,bw,ksmooth,scale_data,sctransform}.py.  Loops follow the reference's
order where it matters (bw.SJ, ksmooth); the per-gene fits run over all genes at once with a per-gene stop flag.

Input of every function: B, the time point's counts, spots x genes (scipy sparse or dense), rows in the package's order."""
import numpy as np
import pandas as pd
import scipy.sparse as sp
from scipy import optimize
from scipy.special import digamma, polygamma


def cell_attr(B):
    """make_cell_attr (sctransform_utils.py:58-62) on the spots with a non-zero total: (kept spot positions, log10 umi)."""
    umi = np.asarray(sp.csr_matrix(B, dtype=np.float64).sum(1)).ravel()
    keep = np.flatnonzero(umi > 0)
    return keep, np.log10(umi[keep])


def kept_genes(B):
    """vst.py:71-75: a count >= 0.01 in >= 5 spots."""
    return np.flatnonzero(np.asarray((sp.csr_matrix(B) >= 0.01).sum(0)).ravel() >= 5)


def dense_y(B, keep, genes):
    """genes x kept spots, fp64."""
    return np.asarray(sp.csr_matrix(B, dtype=np.float64)[keep][:, genes].toarray().T)


def log_gmean(Y):
    """row_gmean (sctransform_utils.py:50-55) with eps 1, log10."""
    return np.log10(np.exp(np.log(Y + 1).mean(1)) - 1)


# ---------------------------------------------------------------- step-1 draw (vst.py:110-115, dds)
def step1_set(lg, n_genes=2000, seed=1448145):
    G = lg.size
    if G <= n_genes:
        return np.arange(G)
    n = lg.size
    sd = lg.std(ddof=1)
    iqr = (np.percentile(lg, 75) - np.percentile(lg, 25)) / 1.3489795
    h = min(sd, iqr) * (n * 3 / 4.0) ** (-1 / 5)
    dens = np.array([np.exp(-0.5 * ((lg[i] - lg) / h) ** 2).sum() for i in range(n)]) / (n * h * np.sqrt(2 * np.pi))
    w = 1 / (dens + np.finfo(float).eps)
    return np.sort(np.random.RandomState(seed).choice(G, n_genes, replace=False, p=w / w.sum()))


# ---------------------------------------------------------------- qpois_reg + theta_ml (sctransform_utils.py:88-187)
def fit_poisson(Y, x, tol=1e-9, maxiters=100, full=False):
    """All rows of Y at once.  Returns (coefficients [G, 2] = b_new, fitted mu [G, N], iterations [G]); with full also the
    coefficients [G, 2] that the fitted mu was computed from (those before the last update)."""
    G, N = Y.shape
    X = np.stack([np.ones(N), x], axis=1)
    b = np.zeros((G, 2))
    b[:, 0] = np.log(Y.mean(1))                    # the `break` after the intercept column: the slope starts at 0
    active = np.ones(G, dtype=bool)
    dif = np.ones(G)
    ij = np.full(G, 2)
    m_last = np.zeros((G, N))
    b_last = np.zeros((G, 2))
    iters = np.zeros(G, dtype=np.int64)
    while active.any():
        a = np.flatnonzero(active)
        yhat = np.clip(b[a] @ X.T, -708, 709)
        m = np.exp(yhat)
        L1 = (Y[a] - m) @ X                                          # X^T (y - m)
        L2 = np.einsum("gn,ni,nj->gij", m, X, X)                     # X^T M X
        step = np.einsum("gij,gj->gi", np.linalg.inv(L2), L1)
        bn = b[a] + step
        dif[a] = np.abs(bn - b[a]).sum(1)
        b_last[a] = b[a]
        b[a] = bn
        m_last[a] = m
        iters[a] += 1
        ij[a] += 1
        active[a] = (dif[a] > tol) & (ij[a] != maxiters)
    return (b, m_last, iters, b_last) if full else (b, m_last, iters)


def theta_ml(Y, mu, limit=10, eps=0.0001220703, full=False):
    """theta [G]; with full also the iterations taken [G]."""
    G, N = Y.shape
    t0 = N / ((Y / mu - 1) ** 2).sum(1)
    it = np.ones(G, dtype=np.int64)
    de = np.ones(G)
    active = (it < limit) & (np.abs(de) > eps)
    while active.any():
        a = np.flatnonzero(active)
        th = np.abs(t0[a])[:, None]
        y, m = Y[a], mu[a]
        A, Bq = th + y, th + m
        info = (-polygamma(1, A) + polygamma(1, th) - 1 / th + 2 / Bq - A / Bq ** 2).sum(1)
        score = (digamma(A) - digamma(th) + np.log(th) + 1 - np.log(Bq) - A / Bq).sum(1)
        de[a] = score / info
        t0[a] = th[:, 0] + de[a]
        it[a] += 1
        active[a] = (it[a] < limit) & (np.abs(de[a]) > eps)
    theta = np.where(t0 < 0, 0.0, t0)
    return (theta, it - 1) if full else theta


def pearson_residuals(Y, x, pars):
    """pearson_residual (sctransform_utils.py:17-37) without a clip: Y [G, N], x = log10 umi [N], pars [G, 3] rows of
    (theta, b0, b1); mu = exp(b0 + b1 x), r = (y - mu) / sqrt(mu + mu^2 / theta)."""
    mu = np.exp(pars[:, 1:2] + pars[:, 2:3] * x[None, :])
    return (Y - mu) / np.sqrt(mu + mu ** 2 / pars[:, :1])


# ---------------------------------------------------------------- bw.SJ (bw.py), loops as written there
PI = 3.14159265


def _bw_pair_cnts(x, nb):
    n = len(x)
    if n > nb / 2:
        d = (x.max() - x.min()) * 1.01 / nb
        xx = np.trunc(np.abs(x) / d) * np.sign(x)
        xx = (xx - xx.min() + 1).astype(np.int64)
        sx = np.bincount(xx, minlength=nb + 1)[1:].astype(float)
        cnt = np.zeros(sx.size)
        for ii in range(sx.size):
            w = sx[ii]
            cnt[0] += w * (w - 1.0)
            if ii:
                cnt[ii:0:-1] += w * sx[:ii]                          # cnt[ii - jj] += w * sx[jj], jj < ii
        cnt[0] *= 0.5
        return d, cnt
    dd = (x.max() - x.min()) * 1.01 / nb
    cnt = np.zeros(nb)
    for i in range(n):
        ii = int(x[i] / dd)
        for j in range(i):
            cnt[abs(ii - int(x[j] / dd))] += 1
    return dd, cnt


def _bw_phi(n, d, cnt, h, order):
    s = 0.0
    for i in range(len(cnt)):
        delta = (i * d / h) ** 2
        if delta >= 1000:
            break
        if order == 4:
            s += np.exp(-delta / 2) * (delta * delta - 6 * delta + 3) * cnt[i]
        else:
            s += np.exp(-delta / 2) * (delta ** 3 - 15 * delta ** 2 + 45 * delta - 15) * cnt[i]
    if order == 4:
        return (2 * s + n * 3) / (n * (n - 1) * h ** 5.0 * np.sqrt(2 * PI))
    return (2 * s - 15 * n) / (n * (n - 1) * h ** 7.0 * np.sqrt(2 * PI))


def bw_sj(x, nb=1000):
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    d, cnt = _bw_pair_cnts(x, nb)
    q75, q25 = np.percentile(x, [75, 25])
    scale = min(np.std(x, ddof=1), (q75 - q25) / 1.349)
    a = 1.24 * scale * n ** (-1 / 7)
    b = 1.23 * scale * n ** (-1 / 9)
    c1 = 1 / (2 * np.sqrt(PI) * n)
    TD = -_bw_phi(n, d, cnt, b, 6)
    hmax = 1.144 * scale * n ** (-1 / 5)
    lower, upper = 0.1 * hmax, hmax
    alph2 = 1.357 * (_bw_phi(n, d, cnt, a, 4) / TD) ** (1 / 7)

    def f(h):
        return (c1 / _bw_phi(n, d, cnt, alph2 * h ** (5 / 7), 4)) ** (1 / 5) - h

    itry = 1
    while f(lower) * f(upper) > 0:
        if itry % 2:
            upper *= 1.2
        else:
            lower /= 1.2
        itry += 1
    return optimize.brentq(f, lower, upper, xtol=0.1 * lower)


# ---------------------------------------------------------------- ksmooth (ksmooth.py), the R loop
def ksmooth(x, y, xp, bw):
    o = np.argsort(x, kind="stable")
    x, y = np.asarray(x)[o], np.asarray(y)[o]
    xs = np.sort(np.asarray(xp, dtype=np.float64))
    bw = bw * 0.3706506
    cut = 4 * bw
    out = np.zeros(xs.size)
    imin = 0
    while imin < x.size and x[imin] < xs[0] - cut:
        imin += 1
    for j, x0 in enumerate(xs):
        num = den = 0.0
        for i in range(imin, x.size):
            if x[i] < x0 - cut:
                imin = i
            else:
                if x[i] > x0 + cut:
                    break
                w = np.exp(-0.5 * (abs(x[i] - x0) / bw) ** 2)
                num += w * y[i]
                den += w
        out[j] = num / den if den > 0 else 0.0
    return xs, out


# ---------------------------------------------------------------- is_outlier (sctransform_utils.py:190-227), with pandas
def _robust_binned(y, x, breaks):
    bins = pd.cut(x, bins=breaks)
    score = pd.Series(np.zeros(len(x)))
    for _, idx in pd.Series(np.arange(len(x))).groupby(bins, observed=True):
        v = y[idx.values]
        med = np.median(v)
        mad = np.median(np.abs(v - med)) * 1.4826
        score[idx.values] = (v - med) / (mad + 2.220446e-16)
    return score.values


def is_outlier(y, x, th=10):
    eps = 2.220446e-16 * 10
    w = (x.max() - x.min()) * bw_sj(x) / 2
    s1 = _robust_binned(y, x, np.arange(x.min() - eps, x.max() + w, w))
    s2 = _robust_binned(y, x, np.arange(x.min() - eps - w / 2, x.max() + w, w))
    return np.where(np.abs(s1) < np.abs(s2), np.abs(s1), np.abs(s2)) > th


# ---------------------------------------------------------------- the whole vst + scale (steps 1-8)
def sctransform(B, n_genes=2000, seed=1448145):
    keep, x = cell_attr(B)
    genes = kept_genes(B)
    Y = dense_y(B, keep, genes)
    N = keep.size
    lg = log_gmean(Y)
    s1 = step1_set(lg, n_genes, seed)
    coef, mu, iters = fit_poisson(Y[s1], x)
    theta = theta_ml(Y[s1], mu)
    # reg_model_pars (vst.py:245-325), od_factor
    lg1 = lg[s1]
    disp = np.log10(1 + 10 ** lg1 / theta)
    cols = np.stack([coef[:, 0], coef[:, 1], disp], axis=1)
    out = np.zeros(s1.size, dtype=bool)
    for c in range(3):
        out |= is_outlier(cols[:, c], lg1)
    xk, ck = lg1[~out], cols[~out]
    xp = np.minimum(np.maximum(lg, xk.min()), xk.max())
    o = np.argsort(xp, kind="stable")
    bw = bw_sj(xk) * 3
    fit = np.zeros((lg.size, 3))
    for c in range(3):
        fit[o, c] = ksmooth(xk, ck[:, c], xp, bw)[1]
    theta_fit = 10 ** lg / (10 ** fit[:, 2] - 1)
    # Pearson residuals (sctransform_utils.py:17-37), clip +-sqrt(N) (vst.py:207-208), gene_attr (vst.py:212-223)
    m = np.exp(fit[:, :1] + fit[:, 1:2] * x[None, :])
    r = (Y - m) / np.sqrt(m + m ** 2 / theta_fit[:, None])
    r = np.clip(r, -np.sqrt(N), np.sqrt(N))
    # SCTransform's clip at +-sqrt(N / 30), then fast_row_scale's float32 mean subtracted in fp64 (scale_data.py:45-56)
    r30 = np.clip(r, -np.sqrt(N / 30), np.sqrt(N / 30))
    scale = r30 - r30.mean(1).astype(np.float32).astype(np.float64)[:, None]
    return dict(spots=keep, log_umi=x, genes=genes, log_gmean=lg, step1=s1, coef=coef, theta=theta, disp=disp, iters=iters,
                outliers=out, fit_intercept=fit[:, 0], fit_slope=fit[:, 1], fit_theta=theta_fit,
                residual_mean=r.mean(1), residual_variance=r.var(1, ddof=1), scale=scale,
                amean=Y.mean(1), variance=Y.var(1, ddof=1))
