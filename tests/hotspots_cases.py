"""Inputs of the local Moran's I tests (CPU and GPU), built on autocorr_cases and nhood_cases: the edge call with spots that lose
their out-edges, graphs that straddle the wavefront and the workgroup, the restatement of a set of time points and the domains
table that goes with autocorr_cases.stage_counts."""
import functools

import numpy as np

import autocorr_cases as ac
import hotspots_ref as ref
import nhood_cases as nc

SEED = nc.SEED
THREADS, GS, CHUNK = 1024, 4, 128              # the library's defaults (spadot_amd.stage_ops.LOCAL_*)
LDS_BYTES, LDS_FIXED = 163840, 256
PLANTED_PERMS = 199
TILE_NS = (63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1)
GROUP_SIZES = (1, GS - 1, GS, GS + 1, 2 * GS + 1)
LONE = {2: (3, 17, 36), 3: (0, 150, 299)}      # the sources whose rows are removed from the edge call, per time point


@functools.lru_cache(maxsize=None)
def edge_call():
    """autocorr_cases.edge_call() (n = 1 without edges, n = 2, n = 37 with a duplicate and a reciprocal edge, n = 300) with the
    out-edges of three spots of the last two time points removed: [(src, dst, V fp32 [n, 4])]."""
    out = []
    for t, (src, dst, V) in enumerate(ac.edge_call()):
        keep = ~np.isin(src, LONE.get(t, ()))
        out.append((src[keep], dst[keep], V))
    assert all(np.isin(LONE[t], out[t][1]).any() for t in LONE)              # they are still somebody's neighbours
    return out


def tile_case(n, E=None, G=3):
    """(src, dst, V fp32 [n, G]) of a random graph of n spots and E (default 6 n) edges, in random edge order."""
    E = 6 * n if E is None else E
    rng = np.random.default_rng(n * 100003 + E + G)
    src, dst = nc.random_edges(rng, n, E) if E else (np.zeros(0, np.int32), np.zeros(0, np.int32))
    return src, dst, ac.random_values(rng, n, G)


def want(problems, n_perms, seed=SEED, first=0, centre=None, genes=None):
    """The restatement of a call: [t] -> (lag, ge, le) [genes, n_t], time point t as graph t, on the centres given (default
    the fp64 means)."""
    out = []
    for t, (src, dst, V) in enumerate(problems):
        c = ac.centres(V) if centre is None else np.asarray(centre[t])
        sel = np.arange(V.shape[1]) if genes is None else np.asarray(genes)
        out.append(ref.local_counts_genes(src, dst, V.shape[0], V[:, sel], c[sel], n_perms, seed, t, first))
    return out


@functools.lru_cache(maxsize=None)
def planted_counts():
    """The restatement's (lag, ge, le) [6, 400] of autocorr_cases.planted_genes under 199 permutations, (SEED, graph 0)."""
    src, dst, V = ac.planted_genes()
    return ref.local_counts_genes(src, dst, V.shape[0], V, ac.centres(V), PLANTED_PERMS, SEED, 0)


def stage_domains(counts_path, csv_path):
    """Writes the domains.csv that goes with autocorr_cases.stage_counts(counts_path): its generator replayed for the labels
    (asserted: the replay reproduces the file's coordinates).  Returns the path."""
    import pandas as pd
    rng = np.random.default_rng(6)
    labs, tps, xys = [], [], []
    for tp, n, K in (("E10", 400, 4), ("E12", 500, 5), ("E14", 600, 6)):
        xy, lab = nc.planted_points(rng, n, K)
        rate = np.full((n, 40), 0.5)
        for g in range(10):
            rate[:, g] += 4.0 * (lab == g % K)
            rate[:, 10 + g] += 4.0 * xy[:, g % 2] / np.sqrt(n)
        rate[:, 39] = 0.0
        rng.poisson(rate)
        labs.append(lab)
        tps += [tp] * n
        xys.append(xy)
    order = rng.permutation(len(tps))
    z = np.load(counts_path)
    np.testing.assert_array_equal(z["spatial"], np.concatenate(xys)[order])
    pd.DataFrame({"row": np.arange(len(tps)), "timepoint": np.asarray(tps)[order], "kmeans": np.concatenate(labs)[order]}).to_csv(
        csv_path, index=False)
    return csv_path
