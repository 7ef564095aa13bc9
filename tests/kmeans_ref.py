"""References of the device K-means, written apart from the package so that the tests compare two independent statements
of each rule.  init_centers: the k-means++ selection rounds in torch (sklearn's _kmeans_plusplus: 2 + int(log k) candidates
per centre drawn by potential, the candidate with the smallest new potential wins), all restarts batched, the draws those
of spadot_amd.kmeans.sweep_draws.  seed_rows / lloyd_step / fit / assign: the same rounds, one Lloyd iteration, the whole
fit and the nearest-centre rule in plain numpy on the host, sums accumulated wider than fp64."""
import math

import numpy as np
import torch


def init_centers(X, xsq, seeds, k):
    """Seeded centres [R, k, d] of the centred data X [n, d] (xsq: its squared row norms) for the restart seeds `seeds`."""
    n, d = X.shape
    R = len(seeds)
    trials = 2 + int(np.log(k))
    first = np.empty(R, dtype=np.int64)
    U = np.empty((R, max(k - 1, 1), trials), dtype=np.float64)
    for r, s in enumerate(seeds):
        rs = np.random.RandomState(int(s))
        first[r] = int(rs.choice(n))
        for c in range(1, k):
            U[r, c - 1] = rs.uniform(size=trials)
    first = torch.as_tensor(first, device=X.device)
    U = torch.as_tensor(U, dtype=X.dtype, device=X.device)
    centers = torch.empty((R, k, d), dtype=X.dtype, device=X.device)
    centers[:, 0] = X[first]
    c0 = centers[:, 0]                                                        # [R, d]
    closest = (xsq[None, :] - 2.0 * (c0 @ X.T) + (c0 * c0).sum(1)[:, None]).clamp_(min=0)     # [R, n]
    pot = closest.sum(1)                                                      # [R]
    ar = torch.arange(R, device=X.device)
    for c in range(1, k):
        rv = U[:, c - 1] * pot[:, None]                                       # [R, trials]
        cand = torch.searchsorted(torch.cumsum(closest, 1), rv).clamp_(max=n - 1)
        Xc = X[cand]                                                          # [R, trials, d]
        dist = (xsq[None, None, :] - 2.0 * torch.matmul(Xc, X.T) + (Xc * Xc).sum(2)[:, :, None]).clamp_(min=0)
        dist = torch.minimum(dist, closest[:, None, :])                       # [R, trials, n]
        pots = dist.sum(2)                                                    # [R, trials]
        best = torch.argmin(pots, dim=1)                                      # [R]
        centers[:, c] = Xc[ar, best]
        closest = dist[ar, best]
        pot = pots[ar, best]
    return centers


# ---------------------------------------------------------------------------------------------------------------------
# Host statements of the rules in plain numpy (no torch, no device), written from the rule and not from the kernels' loops.
# ---------------------------------------------------------------------------------------------------------------------
LD = np.longdouble
WIDE = np.finfo(LD).nmant >= 63          # x87 extended or wider: sums accumulate in it; otherwise math.fsum (exact) is used
EPS = 2.0 ** -53


def trials_of(k):
    return 2 + int(np.log(k))


def _sum0(a):
    """Sum over axis 0 of an array, accumulated wider than fp64 (longdouble, or the exact math.fsum where longdouble is no
    wider than fp64)."""
    if WIDE:
        return np.asarray(a, dtype=LD).sum(0)
    a = np.asarray(a, dtype=np.float64)
    flat = a.reshape(a.shape[0], -1)
    return np.array([math.fsum(flat[:, j]) for j in range(flat.shape[1])], dtype=np.float64).reshape(a.shape[1:])


def seed_rows(X, k, first, U):
    """sklearn's k-means++ rounds on X [n, d] with the draws of spadot_amd.kmeans.sweep_draws (U: (k - 1) * trials uniforms,
    round-major).  Distances in the expanded form xsq - 2 x.c + csq clamped at 0; candidate = searchsorted(cumsum(closest),
    u * pot) (side left) clamped to n - 1; 2 + int(log k) candidates per round, the smallest new potential wins, first on
    ties.  Returns (rows int64 [k], draw_dist [k - 1, trials], cand_gap [k - 1]): draw_dist is the distance of u * pot to the
    nearest prefix sum and cand_gap the gap between the two smallest potentials of DISTINCT candidate rows (the same row
    drawn twice is one candidate), both relative to pot; inf where pot = 0 or only one row was drawn."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    trials = trials_of(k)
    U = np.asarray(U, dtype=np.float64).reshape(max(k - 1, 0), trials)
    xsq = (X * X).sum(1)
    d2 = lambda c: np.maximum(xsq - 2.0 * (X @ c) + (c * c).sum(), 0.0)
    rows = np.empty(k, dtype=np.int64)
    rows[0] = first
    closest = d2(X[first])
    pot = closest.sum()
    draw_dist = np.full((max(k - 1, 0), trials), np.inf)
    cand_gap = np.full(max(k - 1, 0), np.inf)
    for c in range(1, k):
        rv = U[c - 1] * pot
        cum = np.cumsum(closest)
        cand = np.minimum(np.searchsorted(cum, rv, side="left"), n - 1)
        dist = np.stack([np.minimum(d2(X[j]), closest) for j in cand])          # [trials, n]
        pots = dist.sum(1)
        best = int(np.argmin(pots))                                             # first minimum
        if pot > 0:
            draw_dist[c - 1] = [np.abs(cum - v).min() / pot for v in rv]
            distinct = sorted(pots[int(np.flatnonzero(cand == j)[0])] for j in np.unique(cand))
            if len(distinct) > 1:
                cand_gap[c - 1] = (distinct[1] - distinct[0]) / pot
        rows[c] = cand[best]
        closest = dist[best]
        pot = pots[best]
    return rows, draw_dist, cand_gap


def sq_dists(X, C):
    """Squared distances [n, K] as sums of squared differences, accumulated wider than fp64."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    if not WIDE:
        return np.array([[math.fsum((x - c) ** 2) for c in C] for x in X], dtype=np.float64)
    out = np.zeros((X.shape[0], C.shape[0]), dtype=LD)
    Xl = X.astype(LD)
    for j in range(C.shape[0]):                         # (one centre at a time keeps the temporaries small)
        df = Xl - C[j].astype(LD)
        out[:, j] = (df * df).sum(1)
    return out


def assign(X, C):
    """(labels int32 [n], first minimum wins; smallest squared distance [n]; gap [n] = (second smallest - smallest) /
    second smallest: inf with one centre, 0 where both are 0)."""
    d = sq_dists(X, C)
    n = d.shape[0]
    labels = np.argmin(d, axis=1)
    dmin = d[np.arange(n), labels]
    if d.shape[1] == 1:
        return labels.astype(np.int32), dmin, np.full(n, np.inf)
    second = np.partition(d, 1, axis=1)[:, 1]
    pos = second > 0
    gap = np.where(pos, (second - dmin) / np.where(pos, second, 1), 0).astype(np.float64)
    return labels.astype(np.int32), dmin, gap


def lloyd_step(X, C, tol):
    """One Lloyd iteration from the centres C [K, d]: labels (first minimum wins), C_new (mean of members; an EMPTY cluster
    KEEPS its centre), the inertia of C (not of C_new), shift = sum (C_new - C)^2, done = shift <= tol, gap [n] (see assign)
    and bound [K, d] = (n_k + 4) 2^-53 (sum over members |x_ic|) / n_k, the forward error bound of a device centre.
    The member sums are rounded to fp64 once and divided in fp64: where they are exact (lattice data) C_new is the correctly
    rounded quotient."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    labels, dmin, gap = assign(X, C)
    inertia = float(_sum0(dmin))
    C_new = C.copy()
    bound = np.zeros_like(C)
    for k in range(C.shape[0]):
        m = X[labels == k]
        if m.shape[0] == 0:
            continue
        C_new[k] = np.asarray(_sum0(m), dtype=np.float64) / float(m.shape[0])
        bound[k] = (m.shape[0] + 4) * EPS * np.asarray(_sum0(np.abs(m)), dtype=np.float64) / m.shape[0]
    df = (C_new - C).reshape(-1)
    shift = float(_sum0(df.astype(LD) * df.astype(LD) if WIDE else df * df))
    return labels, C_new, inertia, shift, bool(shift <= tol), gap, bound


def inertia_bound(n, d, ref):
    return (n + 2 * d + 8) * EPS * ref


def fit(X, C0, tol, max_iter=300):
    """Lloyd iterations from C0 until done or max_iter.  Returns (centres, labels and inertia of those final centres, n_iter,
    min_gap, min_tol_dist, emptied, bound): min_gap over every assignment of the trajectory (the final one included), min_tol_dist
    = the smallest |shift - tol| / tol (inf for tol = 0), emptied = some cluster had no member at some step (there sklearn
    relocates the centre and the two fits part ways), bound = lloyd_step's bound of the step that wrote the final centres."""
    C = np.asarray(C0, dtype=np.float64).copy()
    min_gap, min_tol = np.inf, np.inf
    n_iter, emptied = 0, False
    for _ in range(max_iter):
        lab, C, _, shift, done, gap, bound = lloyd_step(X, C, tol)
        emptied = emptied or np.bincount(lab, minlength=C.shape[0]).min() == 0
        n_iter += 1
        min_gap = min(min_gap, float(gap.min()))
        if tol > 0:
            min_tol = min(min_tol, abs(shift - tol) / tol)
        if done:
            break
    labels, dmin, gap = assign(X, C)
    emptied = bool(emptied or np.bincount(labels, minlength=C.shape[0]).min() == 0)
    return C, labels, float(_sum0(dmin)), n_iter, min(min_gap, float(gap.min())), min_tol, emptied, bound
