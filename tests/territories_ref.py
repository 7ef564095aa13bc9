"""The territories definition of DESIGN 7r restated with numpy and scipy: the connected pieces of every domain through
scipy.sparse.csgraph.connected_components on the same-label edges, renamed to their smallest spot; the four integers per
domain; the host statistics; the refinement rule; the relabelings of nhood_ref.perm.  Independent of the package."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import nhood_ref

INTEGERS = ("count", "largest", "singletons", "sumsq")


def components(src, dst, lab):
    """(ids int64 [n], sizes int64 [n]): per spot the smallest spot of its territory and the territory's size."""
    lab = np.asarray(lab, dtype=np.int64)
    n = lab.shape[0]
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    same = lab[src] == lab[dst]
    graph = sp.coo_matrix((np.ones(int(same.sum()), dtype=np.int8), (src[same], dst[same])), shape=(n, n)).tocsr()
    _, comp = connected_components(graph, directed=False)
    first = np.full(comp.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp], np.bincount(comp)[comp].astype(np.int64)


def integers(src, dst, lab, K):
    """int64 [K, 4]: count, largest, singletons, sumsq per label value."""
    lab = np.asarray(lab, dtype=np.int64)
    ids, sizes = components(src, dst, lab)
    out = np.zeros((K, 4), dtype=np.int64)
    for r in np.flatnonzero(ids == np.arange(lab.shape[0])).tolist():
        a, s = int(lab[r]), int(sizes[r])
        out[a, 0] += 1
        out[a, 1] = max(out[a, 1], s)
        out[a, 2] += s == 1
        out[a, 3] += s * s
    return out


def perm_integers(src, dst, lab, K, n_perms, seed, g, first=0):
    """The integers of lab[pi_p] for p = first .. first + n_perms - 1: int64 [n_perms, K, 4]."""
    lab = np.asarray(lab, dtype=np.int64)
    return np.stack([integers(src, dst, lab[nhood_ref.perm(lab.shape[0], seed, g, first + p)], K) for p in range(n_perms)])


def boundary(src, dst, lab):
    lab = np.asarray(lab)
    out = np.zeros(lab.shape[0], dtype=bool)
    for s, d in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        if lab[s] != lab[d]:
            out[s] = out[d] = True
    return out


def stats(obs, perm, sizes, alpha=0.05):
    """The statistics of the module docstring of spadot_amd/territories.py, entry by entry."""
    obs = np.asarray(obs, dtype=np.int64)
    K = obs.shape[0]
    perm = np.asarray(perm, dtype=np.int64).reshape(-1, K, 4)
    P = perm.shape[0]
    names = ("largest_share", "contiguity", "count_expected", "count_sd", "count_z", "contiguity_expected", "contiguity_sd",
             "contiguity_z", "p_fewer", "p_more", "padj")
    out = {name: np.full(K, np.nan) for name in names}
    verdict = [""] * K
    for a in range(K):
        size = float(sizes[a])
        if size > 0:
            out["largest_share"][a] = obs[a, 1] / size
            out["contiguity"][a] = obs[a, 3] / (size * size)
        if P == 0:
            continue
        cp = perm[:, a, 0].astype(np.float64)
        gp = perm[:, a, 3] / (size * size) if size > 0 else np.full(P, np.nan)
        for name, o, p in (("count", float(obs[a, 0]), cp), ("contiguity", out["contiguity"][a], gp)):
            out[name + "_expected"][a], out[name + "_sd"][a] = p.mean(), p.std()
            if out[name + "_sd"][a] > 0:
                out[name + "_z"][a] = (o - p.mean()) / p.std()
        out["p_fewer"][a] = (1 + int((perm[:, a, 0] <= obs[a, 0]).sum())) / (P + 1)
        out["p_more"][a] = (1 + int((perm[:, a, 0] >= obs[a, 0]).sum())) / (P + 1)
    if P:
        family = [a for a in range(K) if sizes[a] > 0]
        if family:
            adj = nhood_ref.bh([min(1.0, 2.0 * min(out["p_fewer"][a], out["p_more"][a])) for a in family])
            for a, v in zip(family, adj):
                out["padj"][a] = v
        for a in range(K):
            verdict[a] = "random"
            if out["padj"][a] <= alpha and obs[a, 0] < out["count_expected"][a]:
                verdict[a] = "contiguous"
            elif out["padj"][a] <= alpha and obs[a, 0] > out["count_expected"][a]:
                verdict[a] = "fragmented"
    out["verdict"] = np.array(verdict, dtype=object)
    return out


def refine_round(src, dst, lab, K, s):
    """One round of the refinement rule: (the new labels, the spots in small territories before the round)."""
    lab = np.asarray(lab, dtype=np.int64)
    ids, sizes = components(src, dst, lab)
    small = sizes < s
    votes = {}
    for u, v in list(zip(np.asarray(src).tolist(), np.asarray(dst).tolist())) + list(zip(np.asarray(dst).tolist(),
                                                                                       np.asarray(src).tolist())):
        if small[u] and not small[v]:
            votes.setdefault(int(ids[u]), np.zeros(K, dtype=np.int64))[lab[v]] += 1
    new = lab.copy()
    for t, c in votes.items():
        new[ids == t] = int(np.argmax(c))                              # numpy: the first of equal counts, the smallest label
    return new, int(small.sum())


def refine(src, dst, lab, K, s, max_rounds=64):
    """(labels, the rounds that changed something, the spots moved, the spots in small territories before every round run)."""
    lab0 = np.asarray(lab, dtype=np.int64)
    cur, rounds, smalls = lab0.copy(), 0, []
    while rounds < max_rounds:
        new, n_small = refine_round(src, dst, cur, K, s)
        smalls.append(n_small)
        if np.array_equal(new, cur):
            break
        cur, rounds = new, rounds + 1
    return cur, rounds, int((cur != lab0).sum()), smalls
