"""The Gaussian-mixture definition of spadot_amd.gmm restated in numpy / scipy fp64: sklearn 1.7's
GaussianMixture(covariance_type='full', reg_covar=1e-6, tol=1e-3, max_iter=100, n_init=1) started from a hard labeling, on data
centred by the set's column mean.  tests/test_gmm_cpu.py pins it to sklearn; tests/test_gmm_gpu.py pins the kernels to it.  Next
to every quantity it returns the absolute-value sums that the GPU test's rounding bounds are made of."""
import numpy as np
from scipy import linalg
from scipy.special import logsumexp

EPS10 = 10.0 * np.finfo(np.float64).eps


def one_hot(labels, K):
    r = np.zeros((len(labels), K), dtype=np.float64)
    r[np.arange(len(labels)), np.asarray(labels, dtype=np.int64)] = 1.0
    return r


def m_step(Xc, resp, reg_covar=1e-6):
    """The M-step from responsibilities resp [n, K] on centred data Xc [n, d].  Returns nk, weights, means, covariances,
    precisions_cholesky (upper), the raw sums s0 = sum r, s1 = sum r x, s2 = sum r x x^T and their absolute-value forms a1, a2."""
    n, d = Xc.shape
    K = resp.shape[1]
    s0 = resp.sum(0)
    nk = s0 + EPS10
    s1 = resp.T @ Xc
    mu = s1 / nk[:, None]
    cov = np.empty((K, d, d))
    s2 = np.empty((K, d, d))
    a2 = np.empty((K, d, d))
    for k in range(K):
        diff = Xc - mu[k]
        cov[k] = (resp[:, k, None] * diff).T @ diff / nk[k]
        cov[k].flat[::d + 1] += reg_covar
        s2[k] = (resp[:, k, None] * Xc).T @ Xc
        a2[k] = (resp[:, k, None] * np.abs(Xc)).T @ np.abs(Xc)
    pchol = np.empty((K, d, d))
    for k in range(K):
        L = linalg.cholesky(cov[k], lower=True)
        pchol[k] = linalg.solve_triangular(L, np.eye(d), lower=True).T
    return dict(nk=nk, weights=nk / n, means=mu, covariances=cov, precisions_cholesky=pchol, s0=s0, s1=s1, s2=s2,
                a1=resp.T @ np.abs(Xc), a2=a2)


def e_step(Xc, weights, means, pchol):
    """lp [n, K], norm [n], log_resp [n, K] and A [n, K], the absolute-value sum of lp's terms."""
    n, d = Xc.shape
    K = means.shape[0]
    lp = np.empty((n, K))
    A = np.empty((n, K))
    for k in range(K):
        y = (Xc - means[k]) @ pchol[k]
        logdet = np.sum(np.log(np.diag(pchol[k])))
        lp[:, k] = -0.5 * (d * np.log(2 * np.pi) + np.sum(y * y, axis=1)) + logdet + np.log(weights[k])
        ya = np.abs(Xc - means[k]) @ np.abs(pchol[k])
        A[:, k] = (0.5 * np.sum(ya * ya, axis=1) + np.sum(np.abs(np.log(np.diag(pchol[k])))) + 0.5 * d * np.log(2 * np.pi)
                   + abs(np.log(weights[k])))
    norm = logsumexp(lp, axis=1)
    with np.errstate(under="ignore"):
        log_resp = lp - norm[:, None]
    return lp, norm, log_resp, A


def n_parameters(K, d):
    return K * d * (d + 1) // 2 + K * d + K - 1


def fit(X, labels, K, reg_covar=1e-6, tol=1e-3, max_iter=100, stop_after=None):
    """The fit of the definition.  stop_after: return the parameters after that many iterations (no stop rule), for the kernel
    tests.  Returns a dict: mean (the set's column mean), Xc, weights, means (mean added back), means_c (centred), covariances,
    precisions_cholesky, lower_bound, n_iter, converged, resp, labels, log_likelihood, bic, aic, lbs (lb of every iteration)."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    m = X.mean(0)
    Xc = X - m
    p = m_step(Xc, one_hot(labels, K), reg_covar)
    lb_prev, lbs, converged, n_iter = -np.inf, [], False, 0
    for it in range(1, (stop_after if stop_after is not None else max_iter) + 1):
        _, norm, log_resp, _ = e_step(Xc, p["weights"], p["means"], p["precisions_cholesky"])
        lb = float(np.mean(norm))
        with np.errstate(under="ignore"):
            p = m_step(Xc, np.exp(log_resp), reg_covar)
        lbs.append(lb)
        n_iter = it
        if stop_after is None and abs(lb - lb_prev) < tol:
            converged = True
            break
        lb_prev = lb
    lp, norm, log_resp, _ = e_step(Xc, p["weights"], p["means"], p["precisions_cholesky"])
    with np.errstate(under="ignore"):
        resp = np.exp(log_resp)
    ll = float(np.sum(norm))
    npar = n_parameters(K, d)
    return dict(mean=m, Xc=Xc, weights=p["weights"], means=p["means"] + m, means_c=p["means"], covariances=p["covariances"],
                precisions_cholesky=p["precisions_cholesky"], lower_bound=lbs[-1] if lbs else -np.inf, n_iter=n_iter,
                converged=converged, resp=resp, labels=np.argmax(resp, axis=1), log_likelihood=ll,
                bic=-2.0 * ll + npar * np.log(n), aic=-2.0 * ll + 2.0 * npar, lbs=np.asarray(lbs))


def factor_bound(cov, pchol):
    """The rounding bound [d, d] of |P^T Sigma P - I| for a factor P = Z^T computed from Sigma in fp64 (u = 2^-53) by a
    Cholesky factorisation Sigma = L L^T and forward substitution for Z = L^-1 (Higham, Accuracy and Stability of Numerical
    Algorithms, 2nd ed., theorems 10.3 and 8.5): the computed L satisfies L L^T = Sigma + D with |D| <= (d + 1) u |L| |L^T|,
    and column c of Z satisfies (L + D_c) z_c = e_c with |D_c| <= d u |L|, so Z = L^-1 + F with |F| <= d u |L^-1| |L| |Z|.
    Then Z Sigma Z^T = (I + F L)(I + F L)^T - Z D Z^T, and to first order, with G = |Z| |L| (which also stands for |L^-1| |L|),
      |Z Sigma Z^T - I| <= (d + 1) u (G G^T + G G + (G G)^T).
    The product P^T Sigma P that a test forms in fp64 adds at most 2 d u |P^T| |Sigma| |P|.  The whole is doubled for the
    second-order terms and for L being refactored here from Sigma, not the computed one.  G grows like the square root of
    Sigma's condition number, so the bound is about u d cond(Sigma): 1e-15 for a round component, 1e-7 to 1e-6 for one of
    fewer than d + 1 points (rank < d plus reg I, condition number about 1e7 to 1e8), whose factor no method in fp64 gives to
    1e-9 (LAPACK's, in the restatement, leaves 2.7e-9 on few_d20 and 1.7e-9 on k32_d20)."""
    d = cov.shape[0]
    u = 2.0 ** -53
    G = np.abs(pchol.T) @ np.abs(linalg.cholesky(cov, lower=True))
    GG = G @ G
    return 2.0 * u * ((d + 1) * (G @ G.T + GG + GG.T) + 2 * d * (np.abs(pchol.T) @ np.abs(cov) @ np.abs(pchol)))


def label_margin(resp):
    """Per spot, the difference between its two largest responsibilities (1 where K = 1)."""
    if resp.shape[1] == 1:
        return np.ones(resp.shape[0])
    s = np.sort(resp, axis=1)
    return s[:, -1] - s[:, -2]
