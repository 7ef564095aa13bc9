"""Inputs of the gene-module tests (CPU and GPU), built on autocorr_cases and nhood_cases: the graphs around the 4-deep contraction
step and the 256-spot row blocks of csrc/crossmoran.hip, the gene counts around its 16-column blocks and its 64 x 64 tile, the
cases behind the p-values with the restatement's sums, and the stage's counts restated on the host (graph, values, selection,
statistics) with the three conditions that the planted data must meet."""
import functools
import os
import tempfile

import numpy as np

import autocorr_cases as ac
import autocorr_ref as aref
import markers_ref
import modules_ref as ref
import nhood_cases as nc

SEED = nc.SEED
TILE, BLOCK, KSTEP, KB = 64, 16, 4, 256        # the kernel's tile of M, its column blocks, spots per step and per row block
TILE_NS = (3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)
GENE_COUNTS = (1, 15, 16, 17, 33, TILE + 1)
STAGE_K = {"E10": 4, "E12": 5, "E14": 6}
STAGE_PERMS, STAGE_SEED, MIN_SIM = 199, 3, 0.15


def continuous_values(rng, n, G):
    """fp32 [n, G], every entry a different positive number: no two sums tie."""
    return (0.05 + rng.gamma(2.0, 0.5, (n, G))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tile_case(n, G=5):
    """(src, dst, V fp32 [n, G]) of a random graph of n >= 2 spots with 6 n edges; about 40 % of the entries are zero."""
    rng = np.random.default_rng(7000 + 131 * n + G)
    src, dst = nc.random_edges(rng, n, 6 * n)
    return src, dst, ac.random_values(rng, n, G, density=0.6)


@functools.lru_cache(maxsize=None)
def wide_case():
    """(src, dst, V fp32 [130, 65]): one gene more than the workgroup's tile; every selection of the gene-count tests reads it."""
    rng = np.random.default_rng(65)
    src, dst = nc.random_edges(rng, 130, 780)
    return src, dst, ac.random_values(rng, 130, TILE + 1, density=0.7)


@functools.lru_cache(maxsize=None)
def want(key, n_perms, seed, first=0, observed=True, sel=None):
    """[t] -> (M, A) of the restatement for the problems named by key (a tuple of ('tile', n, G), ('wide',), ('edge',),
    ('stored',), ('planted',) or ('cont', n, G)), graph index = position; sel: a tuple of gene positions (default: all)."""
    out = []
    for t, (src, dst, V) in enumerate(problems(key)):
        V = V if sel is None else V[:, list(sel)]
        out.append(ref.cross_sums(src, dst, V, ac.centres(V), n_perms, seed, t, first, observed))
    return out


@functools.lru_cache(maxsize=None)
def cont_case(n, G):
    rng = np.random.default_rng(9000 + 17 * n + G)
    src, dst = nc.random_edges(rng, n, 6 * n)
    return src, dst, continuous_values(rng, n, G)


def problems(key):
    out = []
    for k in key:
        if k[0] == "tile":
            out.append(tile_case(*k[1:]))
        elif k[0] == "wide":
            out.append(wide_case())
        elif k[0] == "cont":
            out.append(cont_case(*k[1:]))
        elif k[0] == "planted":
            out.append(ac.planted_genes())
        elif k[0] == "edge":
            out += list(ac.edge_call())
        elif k[0] == "stored":
            out += list(ac.stored_case())
        else:
            raise KeyError(k)
    return out


# the cases behind the p-value tests: (key, permutations, seed).  The planted genes hold a single nonzero (its sums tie with the
# observed ones in most permutations); the continuous cases hold no tie at all, and carry the share below 1 %.
PVALUE_CASES = (((("planted",),), 99, SEED), ((("cont", 300, 33),), 49, 5), ((("cont", 37, 5), ("cont", 65, 5)), 49, 6))


def single_or_degenerate(V, E):
    """[G] bool: the genes with at most one nonzero, or degenerate by autocorr's rule."""
    V = np.asarray(V)
    m2, sumsq = ref.spread(V, ac.centres(V))
    return ((V != 0).sum(axis=0) <= 1) | ref.degenerate(V.shape[0], E, m2, sumsq)


@functools.lru_cache(maxsize=None)
def stage_host():
    """[(tp, src, dst, V fp32 [n, 40])] of autocorr_cases.stage_counts restated on the host: the spots of every time point in
    file order, the graph of nhood_cases.knn_edges(.., 6) and the values float32(log1p(count 1e4 / total))."""
    with tempfile.TemporaryDirectory() as d:
        z = np.load(ac.stage_counts(os.path.join(d, "counts.npz")))
        X, tp, xy = z["X"], z["timepoint"].astype(str), z["spatial"]
    out = []
    for name in sorted(set(tp.tolist())):
        rows = np.flatnonzero(tp == name)
        src, dst = nc.knn_edges(xy[rows], 6)
        out.append((name, src, dst, markers_ref.lognorm(X[rows], X[rows].sum(axis=1))))
    return out


def morans(src, dst, V):
    """Moran's I of every column (NaN where degenerate) from autocorr_ref."""
    n, E, c = V.shape[0], src.shape[0], ac.centres(V)
    out = np.full(V.shape[1], np.nan)
    for g in range(V.shape[1]):
        m2, sumsq = aref.spread(V[:, g], c[g])
        if not aref.is_degenerate(n, E, m2, sumsq):
            out[g] = n * aref.edge_sums(src, dst, V[:, g], c[g])[0] / (E * m2)
    return out


def top_union(Is, top):
    """The stage's selection: the union over the time points of the `top` genes by descending I (NaN last, then gene index)."""
    picked = set()
    for I in Is:
        order = np.lexsort((np.arange(I.size), -np.where(np.isnan(I), -np.inf, I)))
        picked.update(int(g) for g in order[:top] if not np.isnan(I[g]))
    return np.asarray(sorted(picked), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def stage_restatement(top):
    """(sel, [(tp, M, A, stats dict, m2)]) of the stage's counts under --top `top`, STAGE_PERMS permutations and STAGE_SEED."""
    host = stage_host()
    sel = top_union([morans(src, dst, V) for _, src, dst, V in host], top)
    out = []
    for t, (tp, src, dst, V) in enumerate(host):
        W = V[:, sel]
        c = ac.centres(W)
        M, A = ref.cross_sums(src, dst, W, c, STAGE_PERMS, STAGE_SEED, t)
        m2, sumsq = ref.spread(W, c)
        out.append((tp, M, A, ref.stats(M, W.shape[0], src.shape[0], m2, sumsq), m2))
    return sel, out


def broken_conditions(sel, K, R, p_sim, labels, P):
    """The violations of the three conditions of the planted stage data, as strings (none: the conditions hold), and the
    smallest R of a same-domain marker pair and the range of R between markers of different domains."""
    sel = np.asarray(sel)
    bad, same, diff = [], [], []
    for a in range(sel.size):
        for b in range(a + 1, sel.size):
            g, h = int(sel[a]), int(sel[b])
            together = labels[a] >= 0 and labels[a] == labels[b]
            if g < 10 and h < 10 and g % K == h % K:
                same.append(R[a, b])
                if p_sim[a, b] != 1.0 / (P + 1) or not together:
                    bad.append(f"(a) markers {g}, {h} of domain {g % K}: p_sim {p_sim[a, b]}, modules {labels[a]}, {labels[b]}")
            elif g < 10 and h < 10:
                diff.append(R[a, b])
                if together:
                    bad.append(f"(b) markers {g}, {h} of domains {g % K}, {h % K} share module {labels[a]}")
            elif 10 <= g < 20 and 10 <= h < 20 and g % 2 != h % 2 and together:
                bad.append(f"(c) gradient genes {g}, {h} along different axes share module {labels[a]}")
    return bad, (min(same) if same else np.nan), ((min(diff), max(diff)) if diff else (np.nan, np.nan))
