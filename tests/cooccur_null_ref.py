"""The random-labelling null of the cooccurrence stage, restated in numpy: what k_cooccur_null of
csrc/cooccur.hip and spadot_amd.cooccurrence's *_null functions are held to.  It forms the n x n matrix of squared distances and
every relabelled labeling, which the device never does.

A problem is one of cooccur_ref plus S >= 1 relabelings, a seed and a problem number g.  The spots are stored by (label, index)
as ripley_ref.by_label stores them; ls are the sorted labels.  Pattern 0 is ls; pattern s >= 1 is ls[nhood_ref.perm(n, seed, g,
s - 1)] on the sorted positions (sorted position j keeps ls[j] and receives the coordinates xs[pi^-1(j)]: the same labelled set).
    N[s, a, b, t] = cooccur_ref.counts of pattern s                                                   int64 [1 + S, K, K, B]
The domain sizes are those of the observed labeling in every pattern, so testing the integer N[a, b, t] is testing the cross-type
K function A N / (n_a n_b) under random labelling."""
import numpy as np

import cooccur_ref
import nhood_ref
import ripley_ref


def labelings(lab, K, S, seed=0, g=0, first=0):
    """(xs order, [1 + S, n] labelings of the sorted positions): row 0 the sorted labels, row s the relabeling first + s - 1."""
    lab = np.asarray(lab, dtype=np.int64)
    order = np.argsort(lab, kind="stable")
    ls = lab[order]
    n = ls.shape[0]
    return order, np.stack([ls] + [ls[nhood_ref.perm(n, seed, g, first + s)] for s in range(S)])


def counts(xy, lab, r2, K, S, seed=0, g=0, first=0):
    """int64 [1 + S, K, K, B] of one problem.  The n x n distances are binned once (pair (i, j) falls into the first t with
    d2 <= r2[t]); every pattern is one histogram of (label pair, bin) and a cumulative sum along t."""
    r2 = np.asarray(r2, dtype=np.float64).reshape(-1)
    B = r2.shape[0]
    order, labs = labelings(lab, K, S, seed, g, first)
    xs = np.asarray(xy, dtype=np.float64)[order]
    n = xs.shape[0]
    bins = np.searchsorted(r2, cooccur_ref.d2_matrix(xs), side="left")          # B: beyond the largest threshold
    bins[np.arange(n), np.arange(n)] = B                                        # a spot is never its own neighbour
    out = np.zeros((1 + S, K, K, B), dtype=np.int64)
    for s, ls in enumerate(labs):
        pair = (ls[:, None] * K + ls[None, :]) * (B + 1) + bins
        hist = np.bincount(pair.reshape(-1), minlength=K * K * (B + 1)).reshape(K, K, B + 1)
        out[s] = np.cumsum(hist[:, :, :B], axis=2)
    return out


def relabelled(xy, lab, K, s, seed=0, g=0):
    """(xs, labels) of pattern s as an explicit labelled set, for cooccur_ref.counts."""
    order, labs = labelings(lab, K, s, seed, g)
    return np.asarray(xy, dtype=np.float64)[order], labs[s]


def stats(N, sizes, ring=False, alpha=0.05):
    """The host statistics of one problem from its integers, cell by cell.  Returns a dict: count int64 [K, K, B] (the tested
    integers: N[0], or its differences along t with ring); sim_mean, sim_min, sim_max, z, p_lo, p_hi fp64 [K, K, B]; ratio,
    ratio_sim_mean, ratio_sim_min, ratio_sim_max fp64 [K, K, B]; p_global, padj fp64 [K, K]; relation [K, K] of str."""
    N = np.asarray(N, dtype=np.int64)
    P, K, _, B = N.shape
    S = P - 1
    T = np.concatenate([N[..., :1], N[..., 1:] - N[..., :-1]], axis=3) if ring else N
    nc = [int(v) for v in sizes]
    out = {k: np.full((K, K, B), np.nan) for k in ("sim_mean", "sim_min", "sim_max", "z", "p_lo", "p_hi")}
    p_global, padj = np.full((K, K), np.nan), np.full((K, K), np.nan)
    excess = np.zeros((K, K))
    for a in range(K):
        for b in range(K):
            if nc[a] == 0 or nc[b] == 0 or (a == b and nc[a] < 2):
                continue
            for t in range(B):
                col = [int(v) for v in T[1:, a, b, t]]
                obs = int(T[0, a, b, t])
                mean = sum(col) / S
                sd = float(np.std(np.array(col, dtype=np.float64)))
                out["sim_mean"][a, b, t], out["sim_min"][a, b, t], out["sim_max"][a, b, t] = mean, min(col), max(col)
                if sd > 0:
                    out["z"][a, b, t] = (obs - mean) / sd
                out["p_hi"][a, b, t] = (1 + sum(v >= obs for v in col)) / (S + 1)
                out["p_lo"][a, b, t] = (1 + sum(v <= obs for v in col)) / (S + 1)
                excess[a, b] += obs - mean
            p_global[a, b] = ripley_ref.mad_p(None, exact=T[:, a, b, :])
    cells = [(a, b) for a in range(K) for b in range(a, K) if not np.isnan(p_global[a, b])]     # N is symmetric: a <= b only
    if cells:
        for (a, b), v in zip(cells, nhood_ref.bh([p_global[a, b] for a, b in cells])):
            padj[a, b] = padj[b, a] = v
    relation = np.full((K, K), "independent", dtype=object)
    for a in range(K):
        for b in range(K):
            if padj[a, b] <= alpha:
                relation[a, b] = "attract" if excess[a, b] > 0 else "avoid"
    ratios = np.stack([cooccur_ref.stats(N[s], ring=ring)["ratio"] for s in range(P)])
    env = {}
    for name, fn in (("ratio_sim_mean", np.mean), ("ratio_sim_min", np.min), ("ratio_sim_max", np.max)):
        env[name] = np.full((K, K, B), np.nan)
        for idx in np.ndindex(K, K, B):
            v = ratios[(slice(1, None),) + idx]
            v = v[~np.isnan(v)]
            if v.size:
                env[name][idx] = fn(v)
    out.update(env, count=T[0].copy(), ratio=ratios[0], p_global=p_global, padj=padj, relation=relation.astype(str))
    return out
