"""numpy restatement of the trends stage's definitions (spadot_amd/trends.py) in fp64 on dense values: the three
weighted moments with the absolute-value sums that bound their rounding, the weighted mean / variance / share of every gene
under every column, and the Pearson correlation of every gene with every fate over the valid spots."""
import numpy as np
from scipy.special import stdtr

from markers_ref import bh, dense_values, lognorm  # noqa: F401  (the same values and the same BH as the markers stage)


def stored_mask(res, t):
    """Which (spot, gene) of time point t has a stored entry, dense bool [n_t, G], from the CSC arrays of a result."""
    lo, hi = int(res["tp_off"][t]), int(res["tp_off"][t + 1])
    G = len(res["genes"])
    colptr, ridx = np.asarray(res["colptr"]), np.asarray(res["ridx"])
    col = np.repeat(np.arange(G), np.diff(colptr))
    sel = (ridx >= lo) & (ridx < hi)
    M = np.zeros((hi - lo, G), dtype=bool)
    M[ridx[sel] - lo, col[sel]] = True
    return M


def moments(V, W, stored=None):
    """One time point.  V: fp32 [n, G] dense, W: fp64 [n, C], stored: bool [n, G] (default V > 0).  Returns S (3 x [G, C]: S0,
    S1, S2), A (3 x [G, C]: the sums of the absolute values of the same terms) and m ([G], the terms of every sum)."""
    Vd = np.asarray(V, dtype=np.float32).astype(np.float64)
    W = np.asarray(W, dtype=np.float64)
    st = (Vd > 0) if stored is None else np.asarray(stored, dtype=bool)
    assert not np.any((Vd != 0) & ~st)
    P = [st.astype(np.float64), Vd, Vd * Vd]
    S = [p.T @ W for p in P]
    A = [p.T @ np.abs(W) for p in P]
    return S, A, st.sum(0)


def trend_stats(S0, S1, S2, s, n):
    """mean, var, pct, delta [G, C] and baseline [G] of one time point from its sums [G, C + 1] (the last column: the column
    of ones), the column sums s [C] of W and the spots n."""
    C = s.shape[0]
    ok = s > 0
    sd = np.where(ok, s, 1.0)[None, :]
    mean = np.where(ok[None, :], S1[:, :C] / sd, np.nan)
    var = np.where(ok[None, :], np.maximum(S2[:, :C] / sd - mean * mean, 0.0), np.nan)
    pct = np.where(ok[None, :], S0[:, :C] / sd, np.nan)
    baseline = S1[:, C] / float(n)
    return mean, var, pct, mean - baseline[:, None], baseline


def change(mean, s):
    """mean [T, G, C], s [T, C] -> [G, C]: last minus first time point with s > 0, NaN where there is none."""
    T, G, C = mean.shape
    out = np.full((G, C), np.nan)
    for c in range(C):
        ts = np.flatnonzero(s[:, c] > 0)
        if ts.size:
            out[:, c] = mean[ts[-1], :, c] - mean[ts[0], :, c]
    return out


def centred_fates(F):
    """One time point.  F [n, K] -> ([Wc | u] [n, K + 1], n', SSF [K]): u marks the rows of F with a nonzero sum."""
    F = np.asarray(F, dtype=np.float64)
    u = (F.sum(1) != 0).astype(np.float64)
    nv = int(u.sum())
    Wd = np.zeros((F.shape[0], F.shape[1] + 1))
    Wd[:, -1] = u
    ssf = np.zeros(F.shape[1])
    if nv:
        Wd[:, :-1] = u[:, None] * (F - (u[:, None] * F).sum(0) / nv)
        ssf = (Wd[:, :-1] ** 2).sum(0)
    return Wd, nv, ssf


def driver_stats(S1, S2, nv, ssf):
    """r, pval, padj [G, K] of one time point from its sums [G, K + 1] (the last column: u), n' and SSF [K]."""
    K = ssf.shape[0]
    G = S1.shape[0]
    r, p, padj = np.zeros((G, K)), np.ones((G, K)), np.ones((G, K))
    if nv < 3:
        return r, p, padj
    M1, M2 = S1[:, K], S2[:, K]
    ssv = M2 - M1 * M1 / nv
    for g in range(G):
        if not M2[g] > 0:
            continue
        for k in range(K):
            if ssf[k] <= 0 or ssv[g] <= nv * 2.0 ** -50 * M2[g]:
                continue
            x = min(1.0, max(-1.0, S1[g, k] / np.sqrt(ssv[g] * ssf[k])))
            r[g, k] = x
            if abs(x) >= 1.0:
                p[g, k] = 0.0
            else:
                p[g, k] = 2.0 * stdtr(nv - 2.0, -abs(x * np.sqrt((nv - 2.0) / ((1.0 - x) * (1.0 + x)))))
    expressed = M2 > 0
    for k in range(K):
        padj[expressed, k] = bh(p[expressed, k])
    return r, p, padj


def gene_trends(Vs, Ws):
    """All time points.  Vs: fp32 [n_t, G] per time point, Ws: fp64 [n_t, C] per time point.  Returns a dict of mean, var, pct,
    delta [T, G, C], baseline [T, G], change [G, C], colsum [T, C]."""
    cols = {k: [] for k in ("mean", "var", "pct", "delta", "baseline", "colsum")}
    for V, W in zip(Vs, Ws):
        W = np.asarray(W, dtype=np.float64)
        S, _, _ = moments(V, np.concatenate([W, np.ones((W.shape[0], 1))], axis=1))
        s = W.sum(0)
        for k, x in zip(("mean", "var", "pct", "delta", "baseline"), trend_stats(S[0], S[1], S[2], s, W.shape[0])):
            cols[k].append(x)
        cols["colsum"].append(s)
    out = {k: np.stack(x) for k, x in cols.items()}
    out["change"] = change(out["mean"], out["colsum"])
    return out


def fate_drivers(Vs, Fs):
    """All time points.  Returns a dict of r, pval, padj [T, G, K], n_valid [T]."""
    rs, ps, qs, nvs = [], [], [], []
    for V, F in zip(Vs, Fs):
        Wd, nv, ssf = centred_fates(F)
        S, _, _ = moments(V, Wd)
        r, p, q = driver_stats(S[1], S[2], nv, ssf)
        rs.append(r); ps.append(p); qs.append(q); nvs.append(nv)
    return dict(r=np.stack(rs), pval=np.stack(ps), padj=np.stack(qs), n_valid=np.asarray(nvs, dtype=np.int64))


def planted(seed=2024, sizes=(400, 600), G=60, K=3):
    """The planted data of the end-to-end tests: counts [n, G] (fp32), time point per row, F [n, K], W [n, K]."""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    F = rng.dirichlet(0.3 * np.ones(K), size=n)
    F[rng.choice(n, n // 20, replace=False)] = 0.0
    rate = np.full((n, G), 0.8)
    rate[:, 0:10] = (0.3 + 3.0 * F[:, 0])[:, None]
    rate[:, 10:20] = (0.3 + 3.0 * F[:, 1])[:, None]
    X = rng.poisson(rate).astype(np.float32)
    X[:, G - 1] = 0
    X[:, G - 1] = np.maximum(1, 150 - X.sum(1))
    tp = np.repeat(np.array([f"t{i}" for i in range(len(sizes))]), sizes)
    W = np.zeros_like(F)
    for t in np.unique(tp):
        m = tp == t
        W[m] = F[m] / F[m].sum(0)
    return X, tp, F, W
