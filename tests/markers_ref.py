"""numpy restatement of the markers stage's definition (spadot_amd/markers.py): average ranks from a stable argsort
and the tie runs, exact integers (twice the rank sums, Ties, nonzeros per domain), then the asymptotic two-sided Mann-Whitney
test with continuity correction in fp64.  Vectorised over the genes (columns) of one time point."""
import numpy as np
from scipy.special import erfc

MAX_N = 2097151                # n^3 < 2^63: the int64 sums below are exact


def lognorm(counts, total):
    """float32(log1p(c * 1e4 / total)) evaluated in fp64 before the rounding; counts [n, G] dense, total [n]."""
    c = np.asarray(counts, dtype=np.float64)
    tot = np.asarray(total, dtype=np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(tot > 0, np.log1p(c * 1e4 / tot), 0.0)
    return v.astype(np.float32)


def twice_ranks(V):
    """Twice the average ranks of every column of the fp32 matrix V [n, G] (bit patterns define ties; all values >= 0, so
    no -0.0), int64 [n, G], and Ties = sum of t^3 - t over each column's tie runs as Python ints."""
    V = np.asarray(V, dtype=np.float32)
    n, G = V.shape
    assert 0 < n <= MAX_N
    order = np.argsort(V, axis=0, kind="stable")
    S = np.take_along_axis(V, order, axis=0)
    pos = np.arange(n, dtype=np.int64)[:, None]
    head = np.ones((n, G), dtype=bool)
    head[1:] = S[1:] != S[:-1]
    tail = np.ones((n, G), dtype=bool)
    tail[:-1] = head[1:]
    s = np.maximum.accumulate(np.where(head, pos, 0), axis=0)                       # start of the run of each sorted position
    e = np.minimum.accumulate(np.where(tail, pos + 1, n)[::-1], axis=0)[::-1]       # its end
    tw = np.empty((n, G), dtype=np.int64)
    np.put_along_axis(tw, order, s + e + 1, axis=0)                                 # ranks s+1 .. e: twice their mean
    t = np.where(head, e - s, 0)
    ties = [int(x) for x in (t * t * t - t).sum(0)]
    return tw, ties


def statistic(R2, n1, n, ties):
    """U1, score, pval (fp64 arrays) from twice the rank sums R2 (int64) of groups of n1 among n values; ties: int64,
    broadcast against R2."""
    R2, n1, ties = np.asarray(R2, dtype=np.int64), np.asarray(n1, dtype=np.int64), np.asarray(ties, dtype=np.int64)
    n = np.int64(n)
    n2 = n - n1
    d2 = R2 - n1 * (n1 + 1)                                          # 2 U1
    dd = d2 - n1 * n2                                                # 2 (U1 - mu)
    br = (n + 1) * n * (n - 1) - ties
    ok = (n1 > 0) & (n2 > 0) & (br > 0) & (dd != 0)
    d = 0.5 * dd.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = (n1 * n2).astype(np.float64) * br.astype(np.float64) / (12.0 * float(n) * float(n - 1))
        score = np.where(ok, (d - 0.5 * np.sign(d)) / np.sqrt(np.where(ok, var, 1.0)), 0.0)
    pval = np.where(ok, np.minimum(1.0, erfc(np.abs(score) / np.sqrt(2.0))), 1.0)
    return 0.5 * d2.astype(np.float64), score, pval


def ranksum_timepoint(V, labels, K):
    """All genes of one time point.  V: fp32 [n, G] dense, labels: int [n] in 0 .. K-1.  Returns r2 (int64 [G, K], twice the
    rank sums), ties (list of G Python ints), nnz_k (int64 [G, K]), vsum, U1, score, pval (fp64 [G, K]), n_k [K]."""
    V = np.asarray(V, dtype=np.float32)
    labels = np.asarray(labels)
    n = V.shape[0]
    tw, ties = twice_ranks(V)
    onehot = (labels[None, :] == np.arange(K)[:, None])
    r2 = (onehot.astype(np.int64) @ tw).T
    nnz_k = (onehot.astype(np.int64) @ (V > 0).astype(np.int64)).T
    vsum = np.stack([V[onehot[k]].astype(np.float64).sum(0) for k in range(K)], axis=1)
    nk = onehot.sum(1).astype(np.int64)
    u1, score, pval = statistic(r2, nk[None, :], n, np.asarray(ties, dtype=np.int64)[:, None])
    return dict(r2=r2, ties=ties, nnz_k=nnz_k, vsum=vsum, U1=u1, score=score, pval=pval, n_k=nk)


def bh(p):
    """Benjamini-Hochberg, written directly: adj_(i) = min over j >= i of p_(j) m / j, capped at 1."""
    p = np.asarray(p, dtype=np.float64)
    m = p.size
    order = sorted(range(m), key=lambda i: (p[i], i))
    out = np.empty(m)
    low = 1.0
    for j in range(m - 1, -1, -1):                                   # from the largest p down: the running minimum
        low = min(low, p[order[j]] * m / (j + 1))
        out[order[j]] = low
    return out


def dense_values(res, t):
    """The device's own v of time point t as a dense fp32 [n_t, G] (from the CSC arrays find_markers returns)."""
    lo, hi = int(res["tp_off"][t]), int(res["tp_off"][t + 1])
    G = len(res["genes"])
    colptr, ridx, val = np.asarray(res["colptr"]), np.asarray(res["ridx"]), np.asarray(res["values"])
    col = np.repeat(np.arange(G), np.diff(colptr))
    sel = (ridx >= lo) & (ridx < hi)
    V = np.zeros((hi - lo, G), dtype=np.float32)
    V[ridx[sel] - lo, col[sel]] = val[sel]
    return V
