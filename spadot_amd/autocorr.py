"""The autocorr stage: which genes are spatially structured inside a time point, and how strongly.  On the spatial k-nearest-
neighbour graph of every time point, Moran's I and Geary's C of every gene with an analytic and a permutation null (squidpy's
gr.spatial_autocorr; csrc/autocorr.hip).  The reference has no such stage; the definition is restated in numpy in
tests/autocorr_ref.py.

    autocorr_sums(edges, dc, values, centre, n_perms)   the device primitive: N and D of every (time point, gene, labeling)
    graph_moments(src, dst, n)                          S0, S1, S2 of a directed graph from integer torch ops on the device
    autocorr_stats(N, D, n, E, m2, moments)             the host part: I, C, both nulls, BH
    spatial_autocorr(edges, dc | dense, n_perms=100)    the test of every gene (or dense column) of every time point
    autocorr(args)    the stage.  args: data, output_dir, prefix (''), k (6), n_perms (100), seed (0), top (100; 0 = all), device

One time point: n spots, directed edges i -> j (no self loops; duplicates count; E of them), per gene the fp32 values v of
trends.lognorm_values (0 where nothing is stored) promoted to fp64, and the centre c = the mean of v over the n spots.  Labeling 0
is the identity; labeling 1 + p gives spot i the value x_i = v[pi_p(i)], pi_p the permutation of neighbors.py's docstring under
(seed, index of the time point, p, n).  The device computes, in fp64 and a fixed order,
    N[g, l] = sum over edges (x_i - c)(x_j - c),     D[g, l] = sum over edges (x_i - x_j)^2,
and the host, with m2 = sum_i (v_i - c)^2 (from the fixed-order sums of trends.weighted_moments: S2 - S1^2 / n) and S0 = E,
    I = n N / (S0 m2),     C = (n - 1) D / (2 S0 m2).
A gene is degenerate in a time point if n < 3, E = 0 or m2 <= n 2^-50 sum v^2 (the rule of trends for a variance that cannot be
told from zero): NaN in every statistic, left out of the BH family.
Analytic null (normality; Cliff and Ord), a_ij the edge multiplicities: S1 = 1/2 sum_ij (a_ij + a_ji)^2, S2 = sum_i (outdeg_i +
indeg_i)^2,
    E[I] = -1 / (n - 1),  Var[I] = (n^2 S1 - n S2 + 3 S0^2) / (S0^2 (n^2 - 1)) - E[I]^2,
    E[C] = 1,             Var[C] = ((2 S1 + S2)(n - 1) - 4 S0^2) / (2 (n + 1) S0^2),
z_norm = (statistic - expectation) / sd, p_norm = 2 sf(|z_norm|) (NaN where the variance is not positive).
Permutation null (P >= 1): mean and sd (ddof 0) of I_p and C_p give z_sim (NaN where sd = 0); on the device's own sums
    p_sim_I = (1 + #{p : N_p >= N_0}) / (P + 1),     p_sim_C = (1 + #{p : D_p <= D_0}) / (P + 1)
(one-sided towards positive autocorrelation); padj: Benjamini-Hochberg of p_sim over the non-degenerate genes of one time point
(of p_norm with P = 0).

The device sums; the host validates, takes the statistics and writes the files.  Limits: at most 2147483647 spots and edges per
time point; permutation indices below 2^32."""
import sys
import time

import numpy as np

from .moran import centre_spread, columns, degenerate, moran_order, refuse_edge_ends
from .utils._stage_utils import edge_pair, labeling_runs, open_stage, savez_pinned, timings, top_setting, write_timepoints

FIELDS = ("I", "C", "z_norm_I", "p_norm_I", "z_sim_I", "p_sim_I", "padj_I", "z_norm_C", "p_norm_C", "z_sim_C", "p_sim_C",
          "padj_C", "mean", "pct")
TABLE_COLUMNS = ("gene",) + FIELDS
ARRAYS = FIELDS + ("N", "D", "m2")
SCRATCH_FLOATS = 2 ** 28           # the images of one launch outside LDS: at most 1 GiB, the labelings are split beyond that


class AutocorrResult:
    """One time point: the fp64 statistics of the module docstring per gene (FIELDS, m2 [G]), the device's sums N, D [G, 1 + P]
    (labeling 0 the observed one), n, E, the graph moments S0, S1, S2 and `degenerate` [G] bool."""

    def __init__(self, N, D, n, E, mean, m2, sumsq, pct, moments):
        self.N, self.D, self.n, self.E, self.mean, self.m2, self.pct = N, D, int(n), int(E), mean, m2, pct
        self.S0, self.S1, self.S2 = (int(v) for v in moments)
        for name, v in autocorr_stats(N, D, n, E, m2, moments, sumsq=sumsq).items():
            setattr(self, name, v)


def graph_moments(src, dst, n):
    """S0 = E, S1 = 1/2 sum_ij (a_ij + a_ji)^2 and S2 = sum_i (outdeg_i + indeg_i)^2 of the directed graph src -> dst over n
    nodes (a_ij the multiplicity of the edge i -> j), as Python integers: integer torch ops on the edges' device (unique on the
    key i n + j of both orientations), no n x n array."""
    import torch
    if not isinstance(src, torch.Tensor) or not isinstance(dst, torch.Tensor) or not src.is_cuda or not dst.is_cuda:
        raise RuntimeError("graph_moments takes the edges as device tensors; there is no CPU path")
    n = int(n)
    s, d = src.long(), dst.long()
    E = int(s.numel())
    if E == 0:
        return 0, 0, 0
    key = torch.cat([s * n + d, d * n + s])                  # a_ij + a_ji is the multiplicity of (i, j) in both orientations
    _, w = torch.unique(key, return_counts=True)             # every unordered pair appears as (i, j) and as (j, i)
    deg = torch.bincount(torch.cat([s, d]), minlength=n)
    return E, int((w * w).sum().item()) // 2, int((deg * deg).sum().item())


def autocorr_stats(N, D, n, E, m2, moments, sumsq=None):
    """The host part of one time point (module docstring).  N, D: fp64 [G, 1 + P], labeling 0 the observed one; m2 [G];
    moments = (S0, S1, S2); sumsq [G]: sum v^2 of the degeneracy rule (None: degenerate where m2 <= 0).  Returns a dict of fp64
    [G] arrays (I, C and per statistic z_norm, p_norm, z_sim, p_sim, padj) and `degenerate` [G] bool."""
    from scipy.special import ndtr
    from .markers import bh_adjust
    N, D, m2 = np.asarray(N, dtype=np.float64), np.asarray(D, dtype=np.float64), np.asarray(m2, dtype=np.float64)
    G, P = N.shape[0], N.shape[1] - 1
    n, E = int(n), int(E)
    S0, S1, S2 = (float(v) for v in moments)
    bad = degenerate(n, E, m2, sumsq)
    out = {"degenerate": bad}
    safe = np.where(bad, 1.0, m2)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        stat = {"I": n * N / (max(S0, 1.0) * safe), "C": (n - 1.0) * D / (2.0 * max(S0, 1.0) * safe)}
        if n >= 3 and E > 0:
            EI = -1.0 / (n - 1.0)
            null = {"I": (EI, (n * n * S1 - n * S2 + 3.0 * S0 * S0) / (S0 * S0 * (n * n - 1.0)) - EI * EI),
                    "C": (1.0, ((2.0 * S1 + S2) * (n - 1.0) - 4.0 * S0 * S0) / (2.0 * (n + 1.0) * S0 * S0))}
        else:
            null = {"I": (np.nan, np.nan), "C": (np.nan, np.nan)}
        for name, sums, tail in (("I", N, np.greater_equal), ("C", D, np.less_equal)):
            obs, (mu, var) = stat[name][:, 0], null[name]
            z = (obs - mu) / np.sqrt(var) if var > 0 else np.full(G, np.nan)
            p_norm = 2.0 * ndtr(-np.abs(z))
            if P >= 1:
                sims = stat[name][:, 1:]
                sd = sims.std(axis=1)
                z_sim = np.where(sd > 0, (obs - sims.mean(axis=1)) / np.where(sd > 0, sd, 1.0), np.nan)
                p_sim = (1.0 + tail(sums[:, 1:], sums[:, :1]).sum(axis=1)) / (P + 1.0)
            else:
                z_sim, p_sim = np.full(G, np.nan), np.full(G, np.nan)
            base = p_sim if P >= 1 else p_norm
            family = ~bad & np.isfinite(base)
            padj = np.full(G, np.nan)
            padj[family] = bh_adjust(base[family])
            for key, v in ((name, obs), (f"z_norm_{name}", z), (f"p_norm_{name}", p_norm), (f"z_sim_{name}", z_sim),
                           (f"p_sim_{name}", p_sim), (f"padj_{name}", padj)):
                out[key] = np.where(bad, np.nan, v)
    return out


def _gene_range(genes, G):
    if genes is None:
        return 0, G
    g0, g1 = (genes.start, genes.stop) if isinstance(genes, range) and genes.step == 1 else genes
    g0, g1 = int(g0), int(g1)
    if not 0 <= g0 < g1 <= G:
        raise ValueError(f"genes must be a contiguous range inside the {G} genes (got {g0} .. {g1 - 1})")
    return g0, g1 - g0


def autocorr_sums(edges, dc, values, centre, n_perms, seed=0, first=0, observed=True, genes=None, lds_limit=None, out=None,
                  threads=None, gs=None):
    """N and D of every (time point, gene, labeling) (module docstring).  edges[t]: (src, dst) integer device tensors of time
    point t, in the order of dc's time points; dc: a DeviceCounts (its colptr, ridx, tp_off); values: fp32 device tensor, one per
    stored entry in CSC order; centre: fp64 [T, G] (device tensor or array).  Labelings: the identity first (observed), then the
    permutations first .. first + n_perms - 1 under seed, time point t as graph index t.  genes: a contiguous range (range or
    (start, stop)) of genes (default: all).  lds_limit: the LDS bytes a workgroup may use (default 163840): a time point whose
    image does not fit (2048 + 8 n > lds_limit) keeps it in global memory, with the same bits.  One launch (several only where
    the global-memory images of all labelings would pass 1 GiB).  Returns (N, D): [t] -> fp64 numpy [genes, labelings].
    ValueError / RuntimeError before any launch; out: a pair of fp64 device tensors [T, genes, labelings] to write into."""
    import torch
    from . import stage_ops as ops
    T, G = int(dc.T), int(dc.G)
    if not edges or len(edges) != T:
        raise ValueError(f"autocorr_sums takes one edge list per time point ({len(edges) if edges else 0} lists, {T} time points)")
    pairs = [edge_pair(e, dc.device, t) for t, e in enumerate(edges)]
    if not isinstance(values, torch.Tensor):
        raise RuntimeError("autocorr_sums takes the values as a device tensor (torch), not a host array")
    centre = centre if isinstance(centre, torch.Tensor) else torch.as_tensor(np.asarray(centre, dtype=np.float64), device=dc.device)
    g0, ng = _gene_range(genes, G)
    n_perms, first, observed = int(n_perms), int(first), bool(observed)
    if n_perms < 0:
        raise ValueError(f"the number of permutations must not be negative (got n_perms = {n_perms})")
    off = np.asarray(dc.tp_off_host, dtype=np.int64)
    with torch.cuda.device(dc.device):
        refuse_edge_ends(pairs, np.diff(off), wide_only=True)
        eoff = np.concatenate([[0], np.cumsum([int(s.shape[0]) for s, _ in pairs])]).astype(np.int64)
        src = torch.cat([s.to(torch.int32) for s, _ in pairs]) if T > 1 else pairs[0][0].to(torch.int32).contiguous()
        dst = torch.cat([d.to(torch.int32) for _, d in pairs]) if T > 1 else pairs[0][1].to(torch.int32).contiguous()
        desc = np.zeros((T, ops.AUTOCORR_DESC), dtype=np.int64)
        for t in range(T):
            desc[t, :5] = (eoff[t], off[t + 1] - off[t], eoff[t + 1] - eoff[t], off[t], t)
        args = (src, dst, dc.colptr, dc.ridx, values, centre.contiguous())
        checked = ops.autocorr_check(*args, desc, g0, ng, observed, first, n_perms)
        L = int(observed) + n_perms
        per = ops.autocorr_scratch_floats(desc, ng, 1, lds_limit, gs)
        runs = labeling_runs(n_perms, observed, first, per, SCRATCH_FLOATS)
        if len(runs) == 1:
            N, D = ops.autocorr_launch(*args, checked, g0, ng, observed, first, n_perms, seed, lds_limit, out, None, threads, gs)
        else:                                                # the labelings in runs that share one scratch buffer
            if out is not None:
                raise ValueError("out is taken only by a call that is one launch")
            scratch = torch.empty(per * (runs[0][0] + runs[0][2]), dtype=torch.float32, device=dc.device)
            parts = [ops.autocorr_launch(*args, checked, g0, ng, obs, p0, n, seed, lds_limit, None, scratch, threads, gs)
                     for obs, p0, n in runs]
            N, D = (torch.cat([p[i] for p in parts], dim=2) for i in range(2))
        N, D = N.reshape(T, ng, L).cpu().numpy(), D.reshape(T, ng, L).cpu().numpy()
    return [N[t] for t in range(T)], [D[t] for t in range(T)]


def spatial_autocorr(edges, data, values=None, n_perms=100, seed=0, lds_limit=None):
    """Moran's I and Geary's C of every gene of every time point with both nulls (module docstring).  edges[t]: (src, dst) device
    tensors of time point t (spatial_edges); data: a DeviceCounts (values: its fp32 values in CSC order, default
    trends.lognorm_values) or, per time point, a dense float32 / float64 device tensor [n, C] of columns such as fates or
    memberships, taken as fp32 and stored completely as a CSC for the same kernel.  The observed labeling and all n_perms
    permutations of all time points are one call to the library; time point t permutes under (seed, t).  Returns [t] ->
    AutocorrResult."""
    import torch
    n_perms = int(n_perms)
    if n_perms < 0:
        raise ValueError(f"the number of permutations must not be negative (got n_perms = {n_perms})")
    dc = columns(data, values)
    off = np.asarray(dc.tp_off_host, dtype=np.int64)
    with torch.cuda.device(dc.device):
        S0, centre, m2, S2 = centre_spread(dc)
        N, D = autocorr_sums(edges, dc, dc.values, centre, n_perms, seed=seed, lds_limit=lds_limit)
        moments = [graph_moments(s, d, int(off[t + 1] - off[t])) for t, (s, d) in enumerate(edges)]
        n_t = torch.as_tensor(np.diff(off).astype(np.float64), device=dc.device)[:, None]
        centre, m2, S2, pct = centre.cpu().numpy(), m2.cpu().numpy(), S2.cpu().numpy(), (S0 / n_t).cpu().numpy()
    return [AutocorrResult(N[t], D[t], int(off[t + 1] - off[t]), moments[t][0], centre[t], m2[t], S2[t], pct[t], moments[t])
            for t in range(dc.T)]


def autocorr_table(r, genes, top=100):
    """The rows of {prefix}autocorr_{tp}.csv: the `top` genes (0 = all) by I descending (NaN last), then gene column."""
    import pandas as pd
    order = moran_order(r.I)
    if top:
        order = order[:top]
    cols = {"gene": np.asarray(genes)[order]}
    cols.update({name: getattr(r, name)[order] for name in FIELDS})
    return pd.DataFrame(cols, columns=list(TABLE_COLUMNS))


def autocorr(args):
    """Reads args.data (counts, as the markers and trends stages: coordinates from obsm['spatial']), builds spatial_edges(.., k) of
    every time point and runs one spatial_autocorr call.  Writes {prefix}autocorr_{tp}.csv (TABLE_COLUMNS; args.top rows by
    descending I, 0 = all) and {prefix}autocorr.npz ('{tp}_{field}' for ARRAYS over all genes and '{tp}_S0/S1/S2', plus timepoints,
    genes, k, n_perms, seed; pinned time stamps: two runs with one seed write the same bytes).  Returns {'tables', 'results' (per
    time point), 'timepoints', 'timings'}."""
    import torch
    from .trends import lognorm_values
    t_start = time.perf_counter()
    top = top_setting(args, 100)
    k, n_perms, seed = int(getattr(args, "k", 6)), int(getattr(args, "n_perms", 100)), int(getattr(args, "seed", 0))
    if top < 0 or k < 1 or n_perms < 0:
        raise ValueError(f"the autocorr stage takes top >= 0, k >= 1 and n_perms >= 0 (got top = {top}, k = {k}, n_perms = "
                         f"{n_perms})")
    st = open_stage(args, k, "the autocorrelation", t_start)
    dc, tps = st.dc, st.tps
    with torch.cuda.device(st.dev):
        res = spatial_autocorr(st.edges, dc, lognorm_values(dc), n_perms=n_perms, seed=seed)
    torch.cuda.synchronize(st.dev)
    t_dev = time.perf_counter()
    arrays = dict(timepoints=np.asarray(tps), genes=np.asarray(dc.genes).astype(str), k=np.int64(k), n_perms=np.int64(n_perms),
                  seed=np.int64(seed))
    tables, arrays = write_timepoints(st.path, "autocorr", tps, res, lambda t, r: autocorr_table(r, dc.genes, top), ARRAYS, arrays,
                                      lambda t, r: {name: np.int64(getattr(r, name)) for name in ("S0", "S1", "S2")})
    savez_pinned(st.path("autocorr.npz"), arrays)
    t_end = time.perf_counter()
    print(f"autocorr: {dc.G} genes x {dc.n} spots of {dc.T} time points, k = {k}, {n_perms} permutations, written to "
          f"{args.output_dir}", file=sys.stderr)
    return {"tables": tables, "results": dict(zip(tps, res)), "timepoints": tps,
            "timings": timings(st.t_start, st.t_read, t_dev, t_end, st.t_graph)}
