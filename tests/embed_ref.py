"""The numpy restatement of the embed stage's definitions (include/spadot_model.h, embed stage): the neighbours, the
200-step search for beta, the joint affinities as CSR, the PCA start, one iteration and a run.  Every sum is taken in the order
the device takes it (np.cumsum adds one element after the other), so the device tests apply the stated rounding bound and not a
guessed tolerance.  Dense n x n arrays throughout: for the sizes of the tests only."""
import numpy as np

SEARCH_STEPS = 200
TILE = 256


def seq_sum(a, axis=-1):
    """The sum along `axis`, one element after the other (np.sum adds pairwise)."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def sq_dists(X):
    """D[i, j] = sum_c (x_ic - x_jc)^2, c ascending, every operation rounded once (numpy has no fused multiply-add)."""
    X = np.asarray(X, dtype=np.float64)
    D = np.zeros((X.shape[0], X.shape[0]))
    for c in range(X.shape[1]):
        diff = X[:, None, c] - X[None, :, c]
        D = D + diff * diff
    return D


def n_neighbors(n, perplexity):
    return min(n - 1, int(np.floor(3.0 * perplexity)))


def knn(X, k):
    """(idx int32 [n, k], d2 [n, k]): the k nearest other points by (squared distance, index) ascending; self left out by index."""
    D = sq_dists(X)
    n = D.shape[0]
    order = np.argsort(D, axis=1, kind="stable")                  # stable: ties keep the ascending index
    order = order[order != np.arange(n)[:, None]].reshape(n, n - 1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(D, order, axis=1)


def _wave_sum(v):
    """The device's sum of a row over a wavefront: entry j sits in lane j % 64; a lane adds its entries in ascending order, then
    the lanes add in a butterfly (xor 32, 16, .., 1).  v: [rows, k] with k <= 192."""
    rows, k = v.shape
    pad = np.zeros((rows, 192))
    pad[:, :k] = v
    lanes = (pad[:, :64] + pad[:, 64:128]) + pad[:, 128:]
    for m in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(64) ^ m]
    return lanes[:, 0]


def entropy(e, beta):
    """(H, p, s) of the rows e [rows, k] at beta [rows]: p = exp(-(beta e)), s = sum p, H = log s + beta (sum e p) / s."""
    p = np.exp(-(beta[:, None] * e))
    s = _wave_sum(p)
    with np.errstate(invalid="ignore"):
        H = np.log(s) + beta * (_wave_sum(e * p) / s)
    return H, p, s


def conditional(d2, perplexity):
    """(cond [n, k], beta [n]): the 200-step search of every row, no early stop; a row whose e are all 0 is uniform with beta 0."""
    d2 = np.asarray(d2, dtype=np.float64)
    e = d2 - d2.min(axis=1, keepdims=True)
    n = e.shape[0]
    target = np.log(perplexity)
    beta, bmin, bmax = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    for _ in range(SEARCH_STEPS):
        H, _p, _s = entropy(e, beta)
        up = H > target
        new_up = np.where(np.isinf(bmax), beta * 2.0, (beta + bmax) * 0.5)
        new_dn = np.where(np.isinf(bmin), beta * 0.5, (beta + bmin) * 0.5)
        bmin = np.where(up, beta, bmin)
        bmax = np.where(up, bmax, beta)
        beta = np.where(up, new_up, new_dn)
    beta = np.where(e.max(axis=1) == 0.0, 0.0, beta)
    _H, p, s = entropy(e, beta)
    return p / s[:, None], beta


def joint_csr(idx, cond):
    """P = (C + C^T) / sum(C + C^T) as CSR with ascending columns: (rowptr int64 [n + 1], col int32, val fp64).  An entry is
    stored where C or C^T has one, whatever its value."""
    n, k = idx.shape
    C = np.zeros((n, n))
    stored = np.zeros((n, n), dtype=bool)
    rows = np.repeat(np.arange(n), k)
    C[rows, idx.ravel()] = np.asarray(cond, dtype=np.float64).ravel()
    stored[rows, idx.ravel()] = True
    stored |= stored.T
    S = C + C.T
    S = S / S.sum()
    r, c = np.nonzero(stored)                                     # row-major: the columns of a row ascend
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return rowptr, c.astype(np.int32), S[r, c]


def dense(rowptr, col, val, n):
    P = np.zeros((n, n))
    P[np.repeat(np.arange(n), np.diff(rowptr)), col] = val
    return P


def pca_start(X):
    """The two leading principal components of the centred data (eigen-decomposition of the d x d covariance), each flipped so
    that its entry of largest magnitude is positive, both scaled by 1e-4 / std(first)."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    w, V = np.linalg.eigh(Xc.T @ Xc / max(X.shape[0] - 1, 1))
    V = V[:, np.argsort(-w, kind="stable")[:2]]
    if V.shape[1] < 2:
        V = np.concatenate([V, np.zeros((V.shape[0], 2 - V.shape[1]))], axis=1)
    for c in range(2):
        big = np.argmax(np.abs(V[:, c]))
        if V[big, c] < 0:
            V[:, c] = -V[:, c]
    Y = Xc @ V
    sd = np.std(Y[:, 0])
    return Y / sd * 1e-4 if sd > 0 else np.zeros_like(Y)          # all points equal: nothing to spread


def default_slices(n):
    """The slices of the partner range of a problem of n points: a function of n alone."""
    T = -(-n // TILE)
    return max(1, min(T, -(-1024 // T)))


def default_learning_rate(n, exaggeration=12.0):
    return max(n / exaggeration / 4.0, 50.0)


def _block_tree(v):
    """The device's sum over the points: per block of 256 the tree sm[t] += sm[t + h], h = 128 .. 1; the blocks ascending."""
    n = v.shape[0]
    nb = -(-n // TILE)
    pad = np.zeros(nb * TILE)
    pad[:n] = v
    pad = pad.reshape(nb, TILE)
    h = TILE // 2
    while h >= 1:
        pad = pad[:, :h] + pad[:, h:2 * h]
        h //= 2
    return float(seq_sum(pad[:, 0]))


def forces(Y, rowptr, col, val, eps, slices):
    """What one iteration sums, in the device's order, each with the sum of the magnitudes of its terms (for the rounding bound):
    z [n], r [n, 2], Z, a [n, 2], g [n, 2], kl, and z_abs (= z), r_abs, a_abs [n, 2]."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    dx = Y[:, None, 0] - Y[None, :, 0]
    dy = Y[:, None, 1] - Y[None, :, 1]
    q = 1.0 / (1.0 + (dx * dx + dy * dy))
    q[np.arange(n), np.arange(n)] = 0.0                           # the self term is left out by a select
    w = q * q
    T = -(-n // TILE)
    z, r, r_abs = np.zeros(n), np.zeros((n, 2)), np.zeros((n, 2))
    for s in range(slices):
        lo, hi = min(s * T // slices * TILE, n), min((s + 1) * T // slices * TILE, n)
        z = z + seq_sum(q[:, lo:hi])
        r[:, 0] = r[:, 0] + seq_sum(w[:, lo:hi] * dx[:, lo:hi])
        r[:, 1] = r[:, 1] + seq_sum(w[:, lo:hi] * dy[:, lo:hi])
        r_abs[:, 0] += np.abs(w[:, lo:hi] * dx[:, lo:hi]).sum(axis=1)
        r_abs[:, 1] += np.abs(w[:, lo:hi] * dy[:, lo:hi]).sum(axis=1)
    Z = _block_tree(z)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    qe = q[rows, col]
    we = (eps * val) * qe
    a, a_abs, klr = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        klt = np.where(val > 0.0, val * (np.log(val) - np.log(qe)), 0.0)
    for i in range(n):                                            # the stored entries of a row in their order
        lo, hi = rowptr[i], rowptr[i + 1]
        a[i, 0] = seq_sum(we[lo:hi] * dx[i, col[lo:hi]])
        a[i, 1] = seq_sum(we[lo:hi] * dy[i, col[lo:hi]])
        a_abs[i, 0] = np.abs(we[lo:hi] * dx[i, col[lo:hi]]).sum()
        a_abs[i, 1] = np.abs(we[lo:hi] * dy[i, col[lo:hi]]).sum()
        klr[i] = seq_sum(klt[lo:hi])
    g = 4.0 * (a - r / Z)
    return dict(z=z, r=r, Z=Z, a=a, g=g, kl=_block_tree(klr) + np.log(Z), z_abs=z.copy(), r_abs=r_abs, a_abs=a_abs,
                kl_abs=float(np.abs(klt).sum()))


def apply_update(Y, update, gains, g, mu, lr):
    """sklearn's _gradient_descent update on the gradient g: (Y, update, gains) after it."""
    inc = update * g < 0.0
    gains = np.where(inc, gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, 0.01)
    update = mu * update - lr * (gains * g)
    return Y + update, update, gains


def phase(it, early, exaggeration=12.0):
    return (exaggeration, 0.5) if it < early else (1.0, 0.8)


def step(Y, update, gains, rowptr, col, val, it, early, lr, slices, exaggeration=12.0):
    """One iteration: (Y, update, gains, the dict of forces())."""
    eps, mu = phase(it, early, exaggeration)
    f = forces(Y, rowptr, col, val, eps, slices)
    Y, update, gains = apply_update(Y, update, gains, f["g"], mu, lr)
    return Y, update, gains, f


def run(Y, rowptr, col, val, n_iter, early=250, lr=None, slices=None, exaggeration=12.0, it0=0, update=None, gains=None):
    """n_iter iterations from iteration number it0 on: (Y, update, gains, kl [n_iter])."""
    n = Y.shape[0]
    lr = default_learning_rate(n, exaggeration) if lr is None else lr
    slices = default_slices(n) if slices is None else slices
    update = np.zeros_like(Y) if update is None else update
    gains = np.ones_like(Y) if gains is None else gains
    kl = np.zeros(n_iter)
    for t in range(n_iter):
        Y, update, gains, f = step(Y, update, gains, rowptr, col, val, it0 + t, early, lr, slices, exaggeration)
        kl[t] = f["kl"]
    return Y, update, gains, kl
