"""Host helpers of SCTransform and of the Louvain gene clusters: the parts of SpaDOT/utils/sctransform (bw.py, ksmooth.py,
sctransform_utils.py, vst.py) and of _cluster_SVGs (SpaDOT/utils/_utils.py:195-221) that act on G values per time point or on
the S x S gene graph.  Pure numpy / scipy (the kNN of gauss_knn_graph runs in torch on the tensor's device), tested on the
CPU; the per-gene fits and residuals run on the device (spadot_amd/sctransform.py, csrc/sctransform.hip).

    bw_sj                  R's bw.SJ(method='ste') as bw.py ports it (pi = 3.14159265, binned pair counts for n > 500)
    ksmooth                R's ksmooth with the normal kernel (ksmooth.py), vectorised
    is_outlier             sctransform_utils.py:190-227: binned robust scores, two shifted break sets
    step1_weights          1 / (density + eps) at the points: an exact Gaussian KDE with KDEpy's Silverman bandwidth
    sample_step1           the step-1 draw of vst.py:110-115
    regularize             reg_model_pars with theta_regularization='od_factor' (vst.py:245-325)
    gauss_knn_graph        sc.pp.neighbors(n_neighbors=100, method='gauss'): kNN and Gaussian connectivities
    louvain                two-phase Louvain of the RB-configuration (modularity) objective at a resolution
    cluster_by_resolution  the resolution loop of _cluster_SVGs: from 1.0 by 0.1 until >= k communities"""
import numpy as np
from scipy import optimize

PI_SJ = 3.14159265             # bw.py:4
DELTA_MAX = 1000.0             # bw.py:5
PARS = ("theta", "Intercept", "log_umi")    # column order of every model_pars array here
OUTLIER_TH = 10.0
OUTLIER_EPS = 2.220446e-16 * 10
ROBUST_EPS = 2.220446e-16
KSMOOTH_SCALE = 0.3706506      # R's ksmooth: the normal kernel's quartiles at +-0.25 bandwidth
GAMMA_STEP = 0.1
GAMMA_MAX = 100.0              # the resolution loop's ceiling (the reference would loop forever)


# ---------------------------------------------------------------- bandwidth (bw.py)
def _pair_counts(x, nb):
    """(d, cnt): bin width and pair counts per bin distance, binned for n > nb / 2 (bw_pair_cnts / bw_den / bw_den_binned)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    if n > nb / 2:
        d = (x.max() - x.min()) * 1.01 / nb
        xx = (np.trunc(np.abs(x) / d) * np.sign(x))
        xx = (xx - xx.min() + 1).astype(np.int64)
        w = np.bincount(xx, minlength=nb + 1)[1:].astype(np.float64)
        full = np.correlate(w, w, mode="full")[w.size - 1:]     # full[k] = sum_j w[j + k] w[j]: integers, exact
        cnt = full.copy()
        cnt[0] = 0.5 * float((w * (w - 1.0)).sum())
        return d, cnt
    dd = (x.max() - x.min()) * 1.01 / nb
    ii = (x / dd).astype(np.int64)                               # int(): truncation toward zero, as bw_den does
    i, j = np.triu_indices(n, k=1)
    cnt = np.bincount(np.abs(ii[i] - ii[j]), minlength=nb).astype(np.float64)
    return dd, cnt


def _phi(n, d, cnt, h, six):
    delta = (np.arange(cnt.size) * d / h) ** 2
    keep = delta < DELTA_MAX
    if not keep.all():                                           # the loops stop at the first delta >= DELTA_MAX
        keep[np.argmin(keep):] = False
    delta, c = delta[keep], cnt[keep]
    if six:
        s = 2.0 * float((np.exp(-delta / 2) * (delta ** 3 - 15 * delta ** 2 + 45 * delta - 15) * c).sum()) - 15 * n
        return s / (n * (n - 1) * h ** 7.0 * np.sqrt(2 * PI_SJ))
    s = 2.0 * float((np.exp(-delta / 2) * (delta ** 2 - 6 * delta + 3) * c).sum()) + n * 3
    return s / (n * (n - 1) * h ** 5.0 * np.sqrt(2 * PI_SJ))


def bw_sj(x, nb=1000):
    """Sheather-Jones 'solve-the-equation' bandwidth as bw.py's bwSJ computes it."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    d, cnt = _pair_counts(x, nb)
    q75, q25 = np.percentile(x, [75, 25])
    scale = min(np.std(x, ddof=1), (q75 - q25) / 1.349)
    a = 1.24 * scale * n ** (-1 / 7)
    b = 1.23 * scale * n ** (-1 / 9)
    c1 = 1 / (2 * np.sqrt(PI_SJ) * n)
    TD = -_phi(n, d, cnt, b, True)
    if not np.isfinite(TD) or TD <= 0:
        raise ValueError("bw_sj: sample is too sparse to find TD")
    hmax = 1.144 * scale * n ** (-1 / 5)
    lower, upper = 0.1 * hmax, hmax
    alph2 = 1.357 * (_phi(n, d, cnt, a, False) / TD) ** (1 / 7)

    def fsd(h):
        return (c1 / _phi(n, d, cnt, alph2 * h ** (5 / 7), False)) ** (1 / 5) - h

    itry = 1
    while fsd(lower) * fsd(upper) > 0:
        if itry >= 99:
            raise ValueError("bw_sj: no solution in the widened interval")
        if itry % 2:
            upper *= 1.2
        else:
            lower /= 1.2
        itry += 1
    return optimize.brentq(fsd, lower, upper, xtol=0.1 * lower)


# ---------------------------------------------------------------- kernel smoother (ksmooth.py)
def ksmooth(x, y, xp, bandwidth, chunk=2048):
    """R's ksmooth(x, y, 'normal', bandwidth, x.points = xp) at the points xp (any order, returned in that order): the
    Nadaraya-Watson mean of y with weights exp(-0.5 (|x - x0| / (0.3706506 bw))^2) over |x - x0| <= 4 * 0.3706506 bw
    (closed window), 0 where the window is empty."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    xp = np.asarray(xp, dtype=np.float64)
    o = np.argsort(x, kind="stable")
    x, y = x[o], y[o]
    bw = bandwidth * KSMOOTH_SCALE
    cut = 4 * bw
    out = np.zeros(xp.size)
    for s in range(0, xp.size, chunk):
        x0 = xp[s:s + chunk, None]
        inwin = (x[None, :] >= x0 - cut) & (x[None, :] <= x0 + cut)
        w = np.where(inwin, np.exp(-0.5 * (np.abs(x[None, :] - x0) / bw) ** 2), 0.0)
        num, den = (w * y[None, :]).sum(1), w.sum(1)
        out[s:s + chunk] = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
    return out


# ---------------------------------------------------------------- outliers (sctransform_utils.py:190-227)
def _robust_scale_binned(y, x, breaks):
    b = np.searchsorted(breaks, x, side="left") - 1             # right-closed bins (b_i, b_i+1], as pd.cut
    b[(x <= breaks[0]) | (x > breaks[-1])] = -1
    score = np.zeros(y.size)
    for k in np.unique(b[b >= 0]):
        m = b == k
        v = y[m]
        med = np.median(v)
        mad = np.median(np.abs(v - med)) * 1.4826
        score[m] = (v - med) / (mad + ROBUST_EPS)
    return score


def is_outlier(y, x, th=OUTLIER_TH, bw=None):
    """True where the smaller of the two binned robust scores of y exceeds th in absolute value.  bw: bw_sj(x), if known."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    lo, hi = x.min(), x.max()
    width = (hi - lo) * (bw_sj(x) if bw is None else bw) / 2
    s1 = _robust_scale_binned(y, x, np.arange(lo - OUTLIER_EPS, hi + width, width))
    s2 = _robust_scale_binned(y, x, np.arange(lo - OUTLIER_EPS - width / 2, hi + width, width))
    return np.minimum(np.abs(s1), np.abs(s2)) > th


# ---------------------------------------------------------------- step-1 genes (vst.py:110-115)
def silverman_bw(x):
    """KDEpy's Silverman bandwidth: min(sd, IQR / 1.3489795) * (3 n / 4)^(-1/5)."""
    x = np.asarray(x, dtype=np.float64)
    q75, q25 = np.percentile(x, [75, 25])
    sigma = min(np.std(x, ddof=1), (q75 - q25) / 1.3489795)
    return sigma * (x.size * 3 / 4.0) ** (-1 / 5)


def step1_weights(log_gmean, chunk=2048):
    """1 / (density(x) + eps) at every point: the Gaussian KDE of the points, evaluated exactly at them."""
    x = np.asarray(log_gmean, dtype=np.float64)
    h = silverman_bw(x)
    dens = np.empty(x.size)
    for s in range(0, x.size, chunk):
        z = (x[s:s + chunk, None] - x[None, :]) / h
        dens[s:s + chunk] = np.exp(-0.5 * z * z).sum(1)
    dens /= x.size * h * np.sqrt(2 * np.pi)
    return 1.0 / (dens + np.finfo(float).eps)


def sample_step1(log_gmean, n_genes=2000, seed=1448145):
    """Positions of the step-1 genes, ascending: all when at most n_genes, else RandomState(seed).choice(G, n_genes,
    replace=False, p=w / w.sum()) with w = step1_weights."""
    G = np.asarray(log_gmean).size
    if not n_genes or n_genes >= G:
        return np.arange(G)
    w = step1_weights(log_gmean)
    pick = np.random.RandomState(seed).choice(G, n_genes, replace=False, p=w / w.sum())
    return np.sort(pick)


# ---------------------------------------------------------------- regularisation (vst.py:245-325)
def regularize(model_pars, log_gmean_step1, log_gmean, bw_adjust=3):
    """model_pars [G1, 3] (PARS order) of the step-1 genes, their log10 geometric means, and those of all kept genes.  Returns
    (model_pars_fit [G, 3] in PARS order, outliers bool [G1]): theta through log10(1 + gmean / theta), each column
    smoothed by ksmooth over the non-outlier step-1 genes with bandwidth bw_sj * bw_adjust, at log_gmean clamped to their
    range."""
    mp = np.asarray(model_pars, dtype=np.float64)
    x1 = np.asarray(log_gmean_step1, dtype=np.float64)
    xg = np.asarray(log_gmean, dtype=np.float64)
    with np.errstate(divide="ignore"):
        disp = np.log10(1 + np.power(10, x1) / mp[:, 0])
    cols = np.stack([mp[:, 1], mp[:, 2], disp], axis=1)          # Intercept, log_umi, dispersion_par
    bw_x = bw_sj(x1)
    outliers = np.zeros(x1.size, dtype=bool)
    for c in range(3):
        outliers |= is_outlier(cols[:, c], x1, bw=bw_x)
    keep = ~outliers
    xs, cs = x1[keep], cols[keep]
    xp = np.clip(xg, xs.min(), xs.max())
    bw = bw_sj(xs) * bw_adjust
    fit = np.stack([ksmooth(xs, cs[:, c], xp, bw) for c in range(3)], axis=1)
    theta = np.power(10, xg) / (np.power(10, fit[:, 2]) - 1)
    return np.stack([theta, fit[:, 0], fit[:, 1]], axis=1), outliers


# ---------------------------------------------------------------- the gene graph (sc.pp.neighbors, method='gauss')
def knn(pcs, k):
    """k nearest rows of pcs (self included, first), by Euclidean distance, ties by index: (indices [S, k], distances)."""
    import torch
    P = torch.as_tensor(pcs).to(torch.float64)
    sq = (P * P).sum(1)
    D2 = (sq[:, None] + sq[None, :] - 2.0 * (P @ P.T)).clamp_(min=0.0)
    D2.fill_diagonal_(0.0)
    order = torch.sort(D2, dim=1, stable=True).indices[:, :k]   # stable: equal distances keep index order
    # the point itself first (its distance is 0; another point at distance 0 sorts after it only if its index is larger)
    idx = order.cpu().numpy()
    S = idx.shape[0]
    for i in np.flatnonzero(idx[:, 0] != np.arange(S)):
        row = [i] + [j for j in idx[i] if j != i]
        idx[i] = row[:k]
    d2 = np.take_along_axis(D2.cpu().numpy(), idx, axis=1)
    return idx, np.sqrt(d2)


def gauss_knn_graph(pcs, k=100):
    """Symmetric Gaussian connectivities of the k-NN graph (k counts the point itself): sigma_i^2 = median of the squared
    distances to the k - 1 nearest other points, W_ij = sqrt(2 s_i s_j / (s_i^2 + s_j^2)) exp(-d_ij^2 / (s_i^2 + s_j^2))
    wherever j is among i's neighbours or i among j's, no self loops.  scipy CSR [S, S]."""
    import scipy.sparse as sp
    S = int(pcs.shape[0])
    k = min(k, S)
    if S < 2:
        return sp.csr_matrix((S, S))
    idx, dist = knn(pcs, k)
    nb, d2 = idx[:, 1:], dist[:, 1:] ** 2
    sig2 = np.median(d2, axis=1)
    sig = np.sqrt(sig2)
    rows = np.repeat(np.arange(S), k - 1)
    cols = nb.ravel()
    den = sig2[rows] + sig2[cols]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.sqrt(2 * sig[rows] * sig[cols] / den) * np.exp(-d2.ravel() / den)
    w = np.nan_to_num(w, nan=0.0)
    A = sp.csr_matrix((w, (rows, cols)), shape=(S, S))
    A = A.maximum(A.T).tocsr()                                   # union of the patterns; W is symmetric where both exist
    A.setdiag(0.0)
    A.eliminate_zeros()
    A.sort_indices()
    return A


# ---------------------------------------------------------------- Louvain
def _local_moves(A, k, m2, gamma, order):
    """One level of local moving on the symmetric weighted graph A (CSR, self loops allowed).  Returns community ids."""
    S = A.shape[0]
    comm = np.arange(S)
    tot = k.astype(np.float64).copy()                            # sum of degrees per community
    indptr, indices, data = A.indptr, A.indices, A.data
    moved_any = False
    while True:
        moved = 0
        for i in order:
            lo, hi = indptr[i], indptr[i + 1]
            nbr, w = indices[lo:hi], data[lo:hi]
            sel = nbr != i
            nbr, w = nbr[sel], w[sel]
            ci = comm[i]
            tot[ci] -= k[i]
            cs = comm[nbr]
            uc, inv = np.unique(cs, return_inverse=True)
            kin = np.bincount(inv, weights=w, minlength=uc.size)
            gain = kin - gamma * tot[uc] * k[i] / m2
            own = np.flatnonzero(uc == ci)
            stay = gain[own[0]] if own.size else -gamma * tot[ci] * k[i] / m2
            best = ci
            if uc.size:
                j = int(np.argmax(gain))                          # first maximum: uc is ascending, so the lowest id
                if gain[j] > stay + 1e-12 * max(1.0, abs(stay)):
                    best = uc[j]
            tot[best] += k[i]
            if best != ci:
                comm[i] = best
                moved += 1
        if moved == 0:
            break
        moved_any = True
    return comm, moved_any


def modularity(A, labels, gamma=1.0):
    """sum over communities of (internal weight / 2m - gamma (degree sum / 2m)^2) of the symmetric matrix A."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    labels = np.asarray(labels)
    k = np.asarray(A.sum(1)).ravel()
    m2 = k.sum()
    coo = A.tocoo()
    same = labels[coo.row] == labels[coo.col]
    inside = coo.data[same].sum()
    tot = np.bincount(labels, weights=k)
    return inside / m2 - gamma * float((tot ** 2).sum()) / m2 ** 2


def louvain(W, resolution=1.0, seed=0):
    """Labels of a two-phase Louvain on the symmetric weighted graph W (scipy sparse, no self loops needed): local moves in a
    RandomState(seed) permutation of the nodes (to the neighbouring community of largest positive gain, ties to the lowest
    id), then aggregation, until a level moves nothing.  Labels are renumbered by community size, descending, ties by the
    smallest member."""
    import scipy.sparse as sp
    W = sp.csr_matrix(W, dtype=np.float64)
    S = W.shape[0]
    if S == 0:
        return np.zeros(0, dtype=np.int64)
    rng = np.random.RandomState(seed)
    node_comm = np.arange(S)
    A = W
    while True:
        k = np.asarray(A.sum(1)).ravel()
        m2 = k.sum()
        if m2 <= 0:
            break
        order = rng.permutation(A.shape[0])
        comm, moved = _local_moves(A, k, m2, resolution, order)
        if not moved:
            break
        _, comm = np.unique(comm, return_inverse=True)
        node_comm = comm[node_comm]
        H = sp.csr_matrix((np.ones(comm.size), (np.arange(comm.size), comm)), shape=(comm.size, comm.max() + 1))
        A = (H.T @ A @ H).tocsr()
        A.sort_indices()
    _, node_comm = np.unique(node_comm, return_inverse=True)
    size = np.bincount(node_comm)
    first = np.full(size.size, S)
    np.minimum.at(first, node_comm, np.arange(S))
    rank = np.lexsort((first, -size))
    new = np.empty_like(rank)
    new[rank] = np.arange(rank.size)
    return new[node_comm].astype(np.int64)


def cluster_by_resolution(W, k=10, seed=0, gamma_max=GAMMA_MAX):
    """_cluster_SVGs' loop: Louvain at resolution 1.0, then + 0.1 (float accumulation) until at least min(k, S) communities.
    Returns (labels, resolution).  Past gamma_max it stops with an error (the reference would loop forever)."""
    S = W.shape[0]
    target = min(k, S)
    gamma = 1.0
    labels = louvain(W, gamma, seed)
    while np.unique(labels).size < target:
        gamma += GAMMA_STEP
        if gamma > gamma_max:
            raise RuntimeError(f"Louvain found fewer than {target} communities up to resolution {gamma_max}")
        labels = louvain(W, gamma, seed)
    return labels, gamma
