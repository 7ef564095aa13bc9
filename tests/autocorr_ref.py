"""The spatial-autocorrelation definition of DESIGN 7j restated in numpy: the labeled values, the two edge sums, Moran's I and
Geary's C, the analytic (normality) null, the permutation null and the graph moments, once from the edge list and once from the
dense matrix.  Independent of the package; the permutation and Benjamini-Hochberg are those of nhood_ref."""
import math

import numpy as np

from nhood_ref import bh, perm

FIELDS = ("I", "C", "z_norm_I", "p_norm_I", "z_sim_I", "p_sim_I", "padj_I", "z_norm_C", "p_norm_C", "z_sim_C", "p_sim_C",
          "padj_C")


def labeled(v, seed, g, p):
    """Labeling 1 + p of graph g under seed: spot i gets v[pi_p(i)]."""
    v = np.asarray(v)
    return v[perm(v.shape[0], seed, g, p)]


def edge_sums(src, dst, x, c):
    """(N, D, A) of one labeling: N = sum (x_i - c)(x_j - c), D = sum (x_i - x_j)^2 over the edges in fp64, and A = sum |(x_i -
    c)(x_j - c)|, the size of N's terms (for the rounding bound of a comparison)."""
    x = np.asarray(x).astype(np.float64)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    z = x - float(c)
    t = z[src] * z[dst]
    d = x[src] - x[dst]
    return float(t.sum()), float((d * d).sum()), float(np.abs(t).sum())


def all_sums(src, dst, v, c, n_perms, seed, g, first=0, observed=True):
    """N, D, A [L] of the identity labeling (if observed) and the permutations first .. first + n_perms - 1."""
    rows = [edge_sums(src, dst, v, c)] if observed else []
    rows += [edge_sums(src, dst, labeled(v, seed, g, first + p), c) for p in range(n_perms)]
    out = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    return out[:, 0], out[:, 1], out[:, 2]


def all_sums_genes(src, dst, V, c, n_perms, seed, g, first=0, observed=True):
    """N, D, A [G, L] of the columns of V [n, G] with centres c [G]: every permutation is drawn once and applied to all columns."""
    V = np.asarray(V)
    n, G = V.shape
    maps = ([np.arange(n)] if observed else []) + [perm(n, seed, g, first + p) for p in range(n_perms)]
    out = np.empty((3, G, len(maps)), dtype=np.float64)
    for l, m in enumerate(maps):
        for k in range(G):
            out[:, k, l] = edge_sums(src, dst, V[m, k], c[k])
    return out[0], out[1], out[2]


def graph_moments(src, dst, n):
    """S0, S1, S2 from the edge list (a dictionary of multiplicities)."""
    a = {}
    for i, j in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        a[(i, j)] = a.get((i, j), 0) + 1
    pairs = set(a) | {(j, i) for i, j in a}
    S1 = sum((a.get((i, j), 0) + a.get((j, i), 0)) ** 2 for i, j in pairs)
    deg = np.bincount(np.asarray(src, dtype=np.int64), minlength=n) + np.bincount(np.asarray(dst, dtype=np.int64), minlength=n)
    assert S1 % 2 == 0
    return len(np.asarray(src)), S1 // 2, int((deg.astype(np.int64) ** 2).sum())


def graph_moments_dense(src, dst, n):
    """S0, S1, S2 from the dense n x n matrix of multiplicities."""
    A = np.zeros((n, n), dtype=np.int64)
    np.add.at(A, (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)), 1)
    S1 = ((A + A.T) ** 2).sum()
    assert S1 % 2 == 0
    return int(A.sum()), int(S1 // 2), int(((A.sum(0) + A.sum(1)) ** 2).sum())


def analytic_null(n, S0, S1, S2):
    """E[I], Var[I], E[C], Var[C] under normality (Cliff and Ord)."""
    n, S0, S1, S2 = float(n), float(S0), float(S1), float(S2)
    EI = -1.0 / (n - 1.0)
    VI = (n * n * S1 - n * S2 + 3.0 * S0 * S0) / (S0 * S0 * (n * n - 1.0)) - EI * EI
    VC = ((2.0 * S1 + S2) * (n - 1.0) - 4.0 * S0 * S0) / (2.0 * (n + 1.0) * S0 * S0)
    return EI, VI, 1.0, VC


def spread(v, c):
    """m2 = sum (v_i - c)^2 and sum v^2 in fp64."""
    v = np.asarray(v).astype(np.float64)
    return float(((v - float(c)) ** 2).sum()), float((v * v).sum())


def is_degenerate(n, E, m2, sumsq):
    return n < 3 or E == 0 or m2 <= n * 2.0 ** -50 * sumsq


def two_sided(z):
    return math.erfc(abs(z) / math.sqrt(2.0)) if math.isfinite(z) else float("nan")


def stats(N, D, n, E, m2, sumsq, moments):
    """The statistics of one time point, gene by gene: N, D [G, 1 + P] (labeling 0 observed), m2 and sumsq [G], moments = (S0,
    S1, S2).  Returns a dict of fp64 [G] arrays (FIELDS) and `degenerate`."""
    N, D = np.asarray(N, dtype=np.float64), np.asarray(D, dtype=np.float64)
    G, P = N.shape[0], N.shape[1] - 1
    out = {k: np.full(G, np.nan) for k in FIELDS}
    bad = np.array([is_degenerate(n, E, float(m2[g]), float(sumsq[g])) for g in range(G)], dtype=bool)
    out["degenerate"] = bad
    if n >= 3 and E > 0:
        EI, VI, EC, VC = analytic_null(n, *moments)
    for g in np.flatnonzero(~bad):
        I = n * N[g] / (E * m2[g])
        C = (n - 1.0) * D[g] / (2.0 * E * m2[g])
        for name, s, mu, var, sums, cmp in (("I", I, EI, VI, N[g], np.greater_equal), ("C", C, EC, VC, D[g], np.less_equal)):
            out[name][g] = s[0]
            if var > 0:
                out[f"z_norm_{name}"][g] = (s[0] - mu) / math.sqrt(var)
                out[f"p_norm_{name}"][g] = two_sided(out[f"z_norm_{name}"][g])
            if P >= 1:
                sd = s[1:].std()
                if sd > 0:
                    out[f"z_sim_{name}"][g] = (s[0] - s[1:].mean()) / sd
                out[f"p_sim_{name}"][g] = (1 + int(cmp(sums[1:], sums[0]).sum())) / (P + 1)
    for name in ("I", "C"):
        base = out[f"p_sim_{name}"] if P >= 1 else out[f"p_norm_{name}"]
        fam = ~bad & np.isfinite(base)
        if fam.any():
            out[f"padj_{name}"][fam] = bh(base[fam])
    return out
