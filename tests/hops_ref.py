"""The hop distances of DESIGN 7s restated with numpy and scipy: all-pairs distances through
scipy.sparse.csgraph.shortest_path(unweighted=True) on the symmetrised 0 / 1 graph; the distance to a set as the minimum over
the rows of its members; the three integers per (set, class) and the eccentricities; the per-spot sums; the host statistics
entry by entry; the relabelings of nhood_ref.perm.  Independent of the package."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import shortest_path

import nhood_ref

FAR = np.iinfo(np.int32).max


def dist_matrix(src, dst, n):
    """int32 [n, n]: the number of edges of a shortest path, direction ignored; FAR where there is none; 0 on the diagonal."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    keep = src != dst
    a = sp.coo_matrix((np.ones(2 * int(keep.sum())), (np.r_[src[keep], dst[keep]], np.r_[dst[keep], src[keep]])), shape=(n, n)).tocsr()
    a.data[:] = 1.0                                                    # duplicates summed by tocsr: back to 0 / 1
    d = shortest_path(a, method="D", directed=False, unweighted=True)
    out = np.full((n, n), FAR, dtype=np.int32)
    ok = np.isfinite(d)
    out[ok] = d[ok].astype(np.int32)
    return out


def set_dist(D, lab, K):
    """int32 [K, n]: the distance of every spot to the set of the spots with label a; FAR out of reach or for an empty set."""
    lab = np.asarray(lab, dtype=np.int64)
    out = np.full((K, D.shape[0]), FAR, dtype=np.int32)
    for a in range(K):
        rows = np.flatnonzero(lab == a)
        if rows.size:
            out[a] = D[rows].min(axis=0)
    return out


def tallies(sd, cls, K):
    """From set distances sd [S, n] and the class of every spot: (sums int64 [S, K, 3] = reached, sumdist, adjacent per class;
    ecc int64 [S])."""
    cls = np.asarray(cls, dtype=np.int64)
    S = sd.shape[0]
    sums, ecc = np.zeros((S, K, 3), dtype=np.int64), np.zeros(S, dtype=np.int64)
    for a in range(S):
        hit = (sd[a] >= 1) & (sd[a] < FAR)
        d = sd[a][hit].astype(np.int64)
        sums[a, :, 0] = np.bincount(cls[hit], minlength=K)
        sums[a, :, 1] = np.bincount(cls[hit], weights=d, minlength=K).astype(np.int64)
        sums[a, :, 2] = np.bincount(cls[hit][d == 1], minlength=K)
        ecc[a] = d.max() if d.size else 0
    return sums, ecc


def integers(D, lab, K):
    """The label item of a labeling: (sums int64 [K, K, 3], ecc int64 [K], hops int64 [n, K]: 0 inside, -1 out of reach)."""
    sd = set_dist(D, lab, K)
    sums, ecc = tallies(sd, lab, K)
    return sums, ecc, np.where(sd == FAR, -1, sd).T.astype(np.int64)


def perm_integers(D, lab, K, n_perms, seed, g, first=0):
    """The sums and eccentricities of lab[pi_p] for p = first .. first + n_perms - 1: (int64 [n_perms, K, K, 3], [n_perms, K])."""
    lab = np.asarray(lab, dtype=np.int64)
    got = [integers(D, lab[nhood_ref.perm(lab.shape[0], seed, g, first + p)], K)[:2] for p in range(n_perms)]
    return np.stack([s for s, _ in got]), np.stack([e for _, e in got])


def spot_integers(D, lab, K):
    """The source items of a graph, spot by spot: (reached_by int64 [n, K], sumdist_by int64 [n, K], degree int64 [n], ecc
    int64 [n])."""
    sums, ecc = tallies(D, lab, K)
    return sums[:, :, 0], sums[:, :, 1], sums[:, :, 2].sum(axis=1), ecc


def depth(hops, lab):
    """Per spot the smallest number of hops to a domain other than its own that it reaches; -1 without one."""
    out = []
    for i, row in enumerate(np.asarray(hops).tolist()):
        d = [h for b, h in enumerate(row) if b != lab[i] and h >= 0]
        out.append(min(d) if d else -1)
    return np.asarray(out, dtype=np.int64)


def _closeness(sums_a, size, n):
    if size == 0:
        return np.nan
    total = int(sums_a[:, 1].sum())
    return (n - size) / total if total else 0.0


def _separation(sums, a, b):
    return sums[a, b, 1] / sums[a, b, 0] if a != b and sums[a, b, 0] else np.nan


def stats(obs, ecc, perm, sizes, n):
    """The statistics of the module docstring of spadot_amd/centrality.py, entry by entry."""
    obs = np.asarray(obs, dtype=np.int64)
    K = obs.shape[0]
    perm = np.asarray(perm, dtype=np.int64).reshape(-1, K, K, 3)
    P = perm.shape[0]
    vec = ("closeness", "degree", "reached_share", "closeness_expected", "closeness_sd", "closeness_z", "p_lower", "p_higher", "padj")
    mat = ("separation", "separation_expected", "separation_sd", "separation_z")
    out = {name: np.full(K, np.nan) for name in vec}
    out.update({name: np.full((K, K), np.nan) for name in mat})
    out["eccentricity"] = np.asarray(ecc, dtype=np.int64).copy()
    for a in range(K):
        size = int(sizes[a])
        out["closeness"][a] = _closeness(obs[a], size, n)
        if size and size < n:
            out["degree"][a] = int(obs[a, :, 2].sum()) / (n - size)
            out["reached_share"][a] = int(obs[a, :, 0].sum()) / (n - size)
        for b in range(K):
            out["separation"][a, b] = _separation(obs, a, b)
        if P == 0:
            continue
        cp = np.asarray([_closeness(perm[p, a], size, n) for p in range(P)])
        out["closeness_expected"][a], out["closeness_sd"][a] = cp.mean(), cp.std()
        if out["closeness_sd"][a] > 0:
            out["closeness_z"][a] = (out["closeness"][a] - cp.mean()) / cp.std()
        if size:
            out["p_lower"][a] = (1 + int((cp <= out["closeness"][a]).sum())) / (P + 1)
            out["p_higher"][a] = (1 + int((cp >= out["closeness"][a]).sum())) / (P + 1)
        for b in range(K):
            sp_ = np.asarray([_separation(perm[p], a, b) for p in range(P)])
            out["separation_expected"][a, b], out["separation_sd"][a, b] = sp_.mean(), sp_.std()
            if out["separation_sd"][a, b] > 0:
                out["separation_z"][a, b] = (out["separation"][a, b] - sp_.mean()) / sp_.std()
    if P:
        family = [a for a in range(K) if sizes[a] > 0]
        if family:
            adj = nhood_ref.bh([min(1.0, 2.0 * min(out["p_lower"][a], out["p_higher"][a])) for a in family])
            for a, v in zip(family, adj):
                out["padj"][a] = v
    return out


def spot_stats(reached, sumdist, ecc):
    """Per spot (closeness, closeness_wf) and per graph (diameter, radius, centre spots) over the spots that reach the most
    others."""
    n = len(reached)
    close = np.asarray([r / s if s else 0.0 for r, s in zip(reached.tolist(), sumdist.tolist())])
    wf = np.asarray([c * (r / (n - 1.0)) if n > 1 else 0.0 for c, r in zip(close.tolist(), reached.tolist())])
    main = [i for i in range(n) if reached[i] == max(reached)]
    radius = min(int(ecc[i]) for i in main)
    return close, wf, max(int(ecc[i]) for i in main), radius, [i for i in main if ecc[i] == radius]
