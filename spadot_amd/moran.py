"""What the three Moran stages share on the host: autocorr (Moran's I and Geary's C per gene), hotspots (local Moran's I) and modules
(bivariate Moran's I) work on the same graph, the same values with the same centre and spread, one degeneracy rule, one selection
of genes.  Every rule is written here once.  The frame of their drivers is the one every stage has
(utils/_stage_utils.py: Stage, open_stage and timings are handed on from here).

    columns(data, values)                the data of a call as one object: a DeviceCounts with its values, or dense columns as a CSC
    column_moments(cols)                 per (time point, gene) the stored count, sum v and sum v^2
    centre_spread(cols)                  S0, the centre c = sum v / n, m2 = sum (v - c)^2 and sum v^2
    degenerate(n, E, m2, sumsq)          the genes of a time point whose statistics are NaN
    gene_selection(genes, G)             the selected genes as int32 indices
    refuse_edge_ends(pairs, sizes)       edge ends outside 0 .. n-1, before they are narrowed to int32 or sorted
    edge_csr(pairs, sizes, device)       the CSR of every time point: the edges sorted stably by source
    read_genes(spec, names)              the gene indices of --genes
    moran_order(I), top_genes(res, top)  the genes by descending Moran's I, and the union of the first `top` over the time points"""
import os

import numpy as np

from .utils._stage_utils import Stage, open_stage, timings  # noqa: F401  (handed on: the stages and their tests took them from here)


class Columns:
    """What the launches read of the data of a call: the CSC arrays colptr int64 [G + 1] and ridx int32, the fp32 `values` of
    the stored entries in CSC order, tp_off_host [T + 1], G, T, n and the device; `counts`: the DeviceCounts behind them, or
    `dense`: the caller's dense columns, of which every entry is stored."""

    def __init__(self, colptr, ridx, values, tp_off_host, G, device, counts=None, dense=None):
        self.colptr, self.ridx, self.values, self.tp_off_host, self.G, self.device = colptr, ridx, values, tp_off_host, int(G), device
        self.T, self.n, self.counts, self.dense = len(tp_off_host) - 1, int(tp_off_host[-1]), counts, dense


def columns(data, values=None):
    """The data of a call as Columns.  data: a DeviceCounts (values: its fp32 values in CSC order, default
    trends.lognorm_values) or, per time point, a dense float32 / float64 device tensor [n, C] of columns such as fates or
    memberships, taken as fp32 and stored completely as a CSC for the same kernels."""
    import torch
    if hasattr(data, "colptr"):
        if values is None:
            from .trends import lognorm_values
            values = lognorm_values(data)
        return Columns(data.colptr, data.ridx, values, data.tp_off_host, data.G, data.device, counts=data)
    if values is not None:
        raise ValueError("values go with a DeviceCounts; dense columns are their own values")
    if not data or any(not isinstance(x, torch.Tensor) for x in data):
        raise RuntimeError("spatial_autocorr takes a DeviceCounts or one dense device tensor [n, C] per time point")
    device, C = data[0].device, None
    for t, x in enumerate(data):
        if not x.is_cuda:
            raise RuntimeError("spadot_amd takes the autocorrelation on the MI355X only (got a CPU tensor); there is no CPU path")
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"the columns of time point {t} must be a float32 or float64 tensor [n, C] (got {tuple(x.shape)} "
                             f"{x.dtype})")
        if C is not None and int(x.shape[1]) != C:
            raise ValueError(f"every time point must hold the same {C} columns (time point {t}: {int(x.shape[1])})")
        C = int(x.shape[1])
    off = np.concatenate([[0], np.cumsum([int(x.shape[0]) for x in data])]).astype(np.int64)
    n = int(off[-1])
    if n * C > 2 ** 31 - 1:
        raise ValueError(f"{n} spots x {C} columns: the dense path stores every entry and takes at most {2 ** 31 - 1}")
    X = torch.cat([x.to(device=device, dtype=torch.float32) for x in data])                    # [n, C]
    if not bool(torch.isfinite(X).all()):
        raise ValueError("the dense columns hold entries that are not finite")
    colptr = torch.arange(C + 1, dtype=torch.int64, device=device) * n
    ridx = torch.arange(n, dtype=torch.int32, device=device).repeat(C)
    return Columns(colptr, ridx, X.t().contiguous().reshape(-1), off, C, device, dense=list(data))


def column_moments(cols):
    """Per (time point, gene): the stored count, sum v and sum v^2 in fp64, a fixed order (trends.weighted_moments with a
    column of ones for a DeviceCounts)."""
    import torch
    if cols.dense is not None:                               # every entry stored: the columns are rows of a [C, n] matrix
        V = cols.values.reshape(cols.G, cols.n).to(torch.float64)
        off = cols.tp_off_host
        S1 = torch.stack([V[:, int(off[t]):int(off[t + 1])].sum(1) for t in range(cols.T)])
        S2 = torch.stack([(V[:, int(off[t]):int(off[t + 1])] ** 2).sum(1) for t in range(cols.T)])
        S0 = torch.as_tensor(np.diff(off).astype(np.float64), device=cols.device)[:, None].expand(cols.T, cols.G)
        return S0, S1, S2
    from .trends import weighted_moments
    S0, S1, S2 = weighted_moments(cols.counts, cols.values, torch.ones((cols.n, 1), dtype=torch.float64, device=cols.device))
    return S0[:, :, 0], S1[:, :, 0], S2[:, :, 0]


def centre_spread(cols):
    """(S0, centre, m2, sumsq), fp64 device tensors [T, G]: the stored count, the mean of v over the n spots of the time point,
    sum (v - centre)^2 as S2 - S1^2 / n (not below 0) and sum v^2."""
    import torch
    with torch.cuda.device(cols.device):
        S0, S1, S2 = column_moments(cols)
        n_t = torch.as_tensor(np.diff(np.asarray(cols.tp_off_host)).astype(np.float64), device=cols.device)[:, None]
        return S0, (S1 / n_t).contiguous(), torch.clamp(S2 - S1 * S1 / n_t, min=0.0), S2


def degenerate(n, E, m2, sumsq=None):
    """bool [G]: the genes of a time point of n spots and E edges whose statistics are NaN: all of them with n < 3 or E = 0,
    otherwise those with m2 <= n 2^-50 sum v^2, the rule of trends for a variance that cannot be told from zero (sumsq None:
    m2 <= 0)."""
    m2 = np.asarray(m2, dtype=np.float64)
    if int(n) < 3 or int(E) == 0:
        return np.full(m2.shape, True)
    return ~(m2 > (0.0 if sumsq is None else int(n) * 2.0 ** -50 * np.asarray(sumsq, dtype=np.float64)))


def gene_selection(genes, G):
    sel = np.asarray(genes).reshape(-1)
    if sel.size < 1 or sel.dtype.kind not in "iu":
        raise ValueError("genes must be a selection of at least one integer gene index (repeats and any order are taken)")
    if sel.min() < 0 or sel.max() >= G:
        raise ValueError(f"the selected genes {int(sel.min())} .. {int(sel.max())} must lie in 0 .. {G - 1}")
    return sel.astype(np.int32)


def refuse_edge_ends(pairs, sizes, wide_only=False):
    """ValueError for a time point with edge ends outside 0 .. n-1, taken before the ends are narrowed to int32 or sorted (one
    host round trip).  wide_only: only the ends that are not int32 yet (stage_ops.autocorr_check sees the others)."""
    import torch
    some = [(t, torch.stack(torch.aminmax(torch.cat([s.reshape(-1), d.reshape(-1)]))).long()) for t, (s, d) in enumerate(pairs)
            if s.numel() and not (wide_only and s.dtype == torch.int32)]
    if some:
        for (t, _), (lo, hi) in zip(some, torch.stack([w for _, w in some]).cpu().tolist()):
            if lo < 0 or hi >= sizes[t]:
                raise ValueError(f"time point {t} has edge ends {lo} .. {hi}: they must lie in 0 .. {int(sizes[t]) - 1}")


def edge_csr(pairs, sizes, device):
    """The CSR of every time point on the device: the edges sorted stably by source.  Refuses edge ends outside 0 .. n-1 first.
    Returns (rowptr int32 [sum (n + 1)], col int32 [sum E], the descriptor [T, 8] of stage_ops.local_check)."""
    import torch
    from . import stage_ops as ops
    refuse_edge_ends(pairs, sizes)
    rowptrs, cols = [], []
    desc = np.zeros((len(pairs), ops.LOCAL_DESC), dtype=np.int64)
    eoff = roff = row0 = 0
    for t, (s, d) in enumerate(pairs):
        n, E = int(sizes[t]), int(s.numel())
        s = s.reshape(-1).long()
        order = torch.sort(s, stable=True).indices
        cols.append(d.reshape(-1)[order].to(torch.int32))
        rp = torch.zeros(n + 1, dtype=torch.int64, device=device)
        rp[1:] = torch.cumsum(torch.bincount(s, minlength=n), 0)
        rowptrs.append(rp.to(torch.int32))
        desc[t, :6] = (eoff, n, E, row0, t, roff)
        eoff, roff, row0 = eoff + E, roff + n + 1, row0 + n
    return torch.cat(rowptrs).contiguous(), torch.cat(cols).contiguous(), desc


def read_genes(spec, names):
    """The gene indices of --genes: a comma list of names, or a file with one name per line.  Unknown names: ValueError."""
    names = np.asarray(names).astype(str)
    if os.path.exists(spec):
        with open(spec) as f:
            want = [line.strip() for line in f if line.strip()]
    else:
        want = [w.strip() for w in str(spec).split(",") if w.strip()]
    if not want:
        raise ValueError(f"--genes names no gene ({spec!r})")
    where = {g: i for i, g in reversed(list(enumerate(names.tolist())))}
    unknown = [w for w in want if w not in where]
    if unknown:
        raise ValueError(f"--genes names {len(unknown)} genes that the data does not hold: {', '.join(unknown[:10])}")
    return np.asarray([where[w] for w in want], dtype=np.int32)


def moran_order(I):
    """The genes by descending Moran's I, NaN last, ties by gene index."""
    I = np.asarray(I)
    return np.lexsort((np.arange(I.shape[0]), -np.where(np.isnan(I), -np.inf, I)))


def top_genes(results, top):
    """The sorted union over the time points (results: one object with I [G] each) of the first `top` genes of moran_order that
    have a Moran's I, int32; empty where no gene has one."""
    picked = set()
    for r in results:
        picked.update(int(g) for g in moran_order(r.I)[:top] if not np.isnan(r.I[g]))
    return np.asarray(sorted(picked), dtype=np.int32)
