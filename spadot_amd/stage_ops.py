"""The launches of the analysis stages (silhouette, gmm, neighbors, territories, centrality, cooccurrence, autocorr, ligrec, hotspots, modules, ripley,
correlogram, embed, sepal) in
libspadot_model.so (include/spadot_model.h).  A *_check refuses, before any launch, what the library would refuse or cannot see (ranges that only a
reduction on the device knows: one host round trip); a *_launch hands over what the check returned.  CPU tensors raise."""
import ctypes

import numpy as np
import torch

from ._call import launched, need_cuda, ptr as _p, stream as _stream
from ._lib import model_lib


def _host(a):
    return ctypes.c_void_p(a.ctypes.data)


def _host_desc(desc, width, unit):
    """The caller's descriptor as a fresh int64 [rows >= 1, width] host array in C order."""
    desc = np.array(desc, dtype=np.int64, order="C", copy=True)
    if desc.ndim != 2 or desc.shape[1] != width or desc.shape[0] < 1:
        raise ValueError(f"a descriptor holds {width} numbers per {unit} (got an array of shape {desc.shape})")
    return desc


def _typed(*specs, any_dim=()):
    for t, dt, what in specs:
        if t.dtype != dt or not t.is_contiguous() or (t.dim() != 1 and what not in any_dim):
            raise ValueError(f"{what} must be a contiguous 1-d {dt} tensor (got {tuple(t.shape)} {t.dtype})")


def _edge_ends(src, dst, eoff, E, zero):
    """[smallest, largest] edge end of the E edges from eoff on, as 0-d int64 device tensors (zeros without edges)."""
    if E <= 0:
        return [zero, zero]
    lo_s, hi_s = torch.aminmax(src[eoff:eoff + E])
    lo_d, hi_d = torch.aminmax(dst[eoff:eoff + E])
    return [torch.minimum(lo_s, lo_d).long(), torch.maximum(hi_s, hi_d).long()]


def _refuse_edge_ends(unit, i, lo, hi, n, E):
    if E > 0 and (lo < 0 or hi >= n):
        raise ValueError(f"{unit} {i} has edge ends {int(lo)} .. {int(hi)}: they must lie in 0 .. {n - 1}")


def _csc_stats(colptr, ridx, zero):
    """[smallest row index, largest, colptr[0], colptr[-1], colptr descends somewhere] as 0-d int64 device tensors."""
    lo, hi = torch.aminmax(ridx) if ridx.numel() > 0 else (zero, zero)
    return [lo.long(), hi.long(), colptr[0], colptr[-1], (colptr[1:] < colptr[:-1]).any().long()]


def _refuse_rows(ridx_lo, ridx_hi, nnz, rows):
    if nnz > 0 and (ridx_lo < 0 or ridx_hi >= rows):
        raise ValueError(f"ridx holds the row indices {ridx_lo} .. {ridx_hi}: they must lie in 0 .. {rows - 1}")


def _refuse_colptr(c0, c1, unordered, nnz):
    if c0 != 0 or c1 != nnz or unordered:
        raise ValueError(f"colptr must ascend from 0 to the {nnz} stored entries (it runs from {c0} to {c1})")


def _csc_sizes(colptr, ridx, values, limit):
    G, nnz = int(colptr.numel()) - 1, int(ridx.numel())
    if G < 1 or values.numel() != nnz or nnz > limit:
        raise ValueError(f"colptr holds {G} genes, ridx {nnz} and values {int(values.numel())} stored entries: at least one gene, "
                         f"one value per entry and at most {limit} entries")
    return G, nnz


def _csr_stats(rowptr, col, desc, zero):
    """Per time point of a descriptor whose columns 0, 1, 2 and 5 are eoff, n, E and roff: [smallest neighbour in col, largest,
    rowptr[0], rowptr[-1], rowptr descends somewhere] as 0-d int64 device tensors."""
    stats = []
    for eoff, n, E, _row0, _gid, roff, *_rest in desc.tolist():
        rp = rowptr[roff:roff + n + 1]
        lo, hi = torch.aminmax(col[eoff:eoff + E]) if E > 0 else (zero, zero)
        stats += [lo.long(), hi.long(), rp[0].long(), rp[-1].long(), (rp[1:] < rp[:-1]).any().long()]
    return stats


def _refuse_csr(desc, per):
    """per: the numbers of _csr_stats on the host, [T, 5]; columns 6 and 7 of the descriptor, the range of col, are filled in."""
    desc[:, 6], desc[:, 7] = per[:, 0], per[:, 1]
    for t in range(desc.shape[0]):
        n, E = int(desc[t, 1]), int(desc[t, 2])
        if E > 0 and (per[t, 0] < 0 or per[t, 1] >= n):
            raise ValueError(f"time point {t} has neighbours {int(per[t, 0])} .. {int(per[t, 1])} in col: they must lie in 0 .. "
                             f"{n - 1}")
        if per[t, 2] != 0 or per[t, 3] != E or per[t, 4]:
            raise ValueError(f"the rowptr of time point {t} must ascend from 0 to its {E} edges (it runs from {int(per[t, 2])} to "
                             f"{int(per[t, 3])})")


def _refuse_genes(gene_lo, gene_hi, G):
    if gene_lo < 0 or gene_hi >= G:
        raise ValueError(f"the selected genes {gene_lo} .. {gene_hi} must lie in 0 .. {G - 1}")


def _refuse_time_point(t, name, row, n, E, most, consistent):
    """The limits of one row of a descriptor of time points: 1 .. most spots, 0 .. most edges, and what the caller found of
    its other columns."""
    if not 1 <= n <= most:
        raise ValueError(f"time point {t} has {n} spots: {name} takes 1 to {most} (int32 spot numbers)")
    if not 0 <= E <= most:
        raise ValueError(f"time point {t} has {E} edges: {name} takes at most {most} per time point")
    if not consistent:
        raise ValueError(f"time point {t}: inconsistent descriptor {row}")


def labelings(name, observed, first, P):
    """(observed as 0 / 1, first, P) of a call over the observed labeling and / or the permutations first .. first + P - 1."""
    observed, first, P = int(bool(observed)), int(first), int(P)
    if P < 0 or first < 0 or observed + P < 1:
        raise ValueError(f"{name} takes P >= 0 permutations from first >= 0 on, and at least one labeling (got P = {P}, "
                         f"first = {first}, observed = {bool(observed)})")
    if first + P > 2 ** 32:
        raise ValueError(f"permutation indices {first} .. {first + P - 1}: the indices must stay below 2^32")
    return observed, first, P


def _lds_limit(lds_limit, most):
    lds_limit = most if lds_limit is None else min(int(lds_limit), most)
    if lds_limit < 0:
        raise ValueError(f"lds_limit is a number of bytes, 0 to {most} (got {lds_limit})")
    return lds_limit


def _signed64(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed


def silhouette_launch(X, prob, order, coff, n_max, k_min, k_max, out=None):
    """Silhouette coefficients of P (data set, labeling) problems in ONE launch (include/spadot_model.h: spadot_silhouette).
    X [rows, d] fp64, the sets one after the other; prob [P, 4] int64 (first row of the set, offset of the problem, n, K);
    order int32 [sum n]: per problem its rows sorted by (label, row); coff int32 [P, 33] cluster offsets.  Returns (a, b,
    nearest, s) of length sum n in the caller's row order (out: tensors to write into).  ValueError outside 1 <= d <= 32,
    2 <= K <= 32, P <= 65535, n <= 2147483391, before any launch."""
    need_cuda(X, prob, order, coff)
    if X.dtype != torch.float64 or not X.is_contiguous():
        raise RuntimeError("silhouette_launch takes a contiguous fp64 matrix")
    total, P = int(order.shape[0]), int(prob.shape[0])
    a, b, nearest, s = out if out is not None else (
        torch.empty(total, dtype=torch.float64, device=X.device), torch.empty(total, dtype=torch.float64, device=X.device),
        torch.empty(total, dtype=torch.int32, device=X.device), torch.empty(total, dtype=torch.float64, device=X.device))
    rc = model_lib().spadot_silhouette(_p(X), int(X.shape[1]), P, _p(prob), _p(order), _p(coff), int(n_max), int(k_min),
                                       int(k_max), _p(a), _p(b), _p(nearest), _p(s), _stream())
    launched(rc, "spadot_silhouette", "1 <= d <= 32, 2 <= K <= 32, at most 65535 problems of at most 2147483391 points",
             f": d = {int(X.shape[1])}, K = {int(k_min)} .. {int(k_max)}, {P} problems, n <= {int(n_max)}")
    return a, b, nearest, s


GMM_LIMITS = ("1 <= d <= 32, 1 <= K <= 32, at most 65535 problems of at most 2147483391 points, and 8 (max(K S, (K + 256) DP) + "
              "256 (K | 1)) + 2048 <= 163840 bytes of LDS with DP = 4 ceil(d / 4), S = DP + DP (DP + 1) / 2 + 2 (K = 32 up to "
              "d = 24, K <= 29 up to d = 28, K <= 24 up to d = 32)")


def gmm_em_steps(X, prob, n_max, par, w, cov, part, done, n_iter, lb, reg_covar, tol, steps, resp_init=None, mom=None):
    """Gaussian-mixture EM for P problems (include/spadot_model.h: spadot_gmm_em_step): if resp_init is given, first the M-step
    from those responsibilities; then `steps` iterations (E-step, M-step, stop rule), frozen problems left alone.  X [rows, d]
    centred fp64; prob [P, 4] int64; par [P, K_max, S], w [P, K_max], cov [P, K_max, d, d], mom [P, K_max, M] or None, part (work
    space), done / n_iter int32 [P], lb fp64 [P]: updated in place.  ValueError outside the limits, before any launch."""
    need_cuda(X, prob, par, w, cov, part, done, n_iter, lb, resp_init, mom)
    if X.dtype != torch.float64 or not X.is_contiguous():
        raise RuntimeError("gmm_em_steps takes a contiguous fp64 matrix")
    P, K_max, d = int(prob.shape[0]), int(par.shape[1]), int(X.shape[1])
    rc = model_lib().spadot_gmm_em_step(_p(X), d, P, _p(prob), K_max, int(n_max), _p(par), _p(w), _p(cov), _p(mom),
                                        _p(resp_init), float(reg_covar), float(tol), int(steps), _p(part), _p(done), _p(n_iter),
                                        _p(lb), _stream())
    launched(rc, "spadot_gmm_em_step", GMM_LIMITS, f": d = {d}, K = {K_max}, {P} problems, n <= {int(n_max)}")


def gmm_estep(X, prob, n_max, par, norm, labels=None, resp=None, lp=None):
    """One E-step of P problems with the parameters in par (spadot_gmm_estep): norm [sum n] fp64 and, where given, labels [sum n]
    int32, resp and lp [sum n, K_max] fp64 are written.  ValueError outside the limits, before any launch."""
    need_cuda(X, prob, par, norm, labels, resp, lp)
    if X.dtype != torch.float64 or not X.is_contiguous():
        raise RuntimeError("gmm_estep takes a contiguous fp64 matrix")
    P, K_max, d = int(prob.shape[0]), int(par.shape[1]), int(X.shape[1])
    rc = model_lib().spadot_gmm_estep(_p(X), d, P, _p(prob), K_max, int(n_max), _p(par), _p(norm), _p(labels), _p(resp), _p(lp),
                                      _stream())
    launched(rc, "spadot_gmm_estep", GMM_LIMITS, f": d = {d}, K = {K_max}, {P} problems, n <= {int(n_max)}")


NHOOD_MAX_K = 32
NHOOD_MAX = 2147483647             # nodes and edges of a graph (int32), and (graph, labeling) pairs of a call (gridDim.x)
NHOOD_LDS_BYTES = 163840
NHOOD_DESC = 12
NHOOD_LIMITS = ("1 <= K <= 32, 1 <= n <= 2147483647 nodes and at most 2147483647 edges per graph, every edge end in 0 .. n-1, every "
                "label below K, at most 2147483647 labelings per call, permutation indices below 2^32")


def nhood_check(src, dst, labels, desc, K_max):
    """The refusals of nhood_counts, before any launch: the limits from the descriptor, then the range of the edge ends and the
    largest label of every graph by reductions on the device (one host round trip).  Returns the descriptor with columns 10 and
    11 filled in; ValueError otherwise."""
    need_cuda(src, dst, labels)
    desc = _host_desc(desc, NHOOD_DESC, "graph")
    K_max = int(K_max)
    if not 1 <= K_max <= NHOOD_MAX_K:
        raise ValueError(f"spadot_nhood_counts takes 1 to {NHOOD_MAX_K} label values (got K_max = {K_max})")
    items = 0
    for g, (eoff, n, E, K, loff, L, p0, gid, item0, _seed, _lo, _hi) in enumerate(desc.tolist()):
        if not 1 <= K <= K_max:
            raise ValueError(f"graph {g} has {K} label values: spadot_nhood_counts takes 1 to {K_max} here, at most {NHOOD_MAX_K}")
        if not 1 <= n <= NHOOD_MAX:
            raise ValueError(f"graph {g} has {n} nodes: spadot_nhood_counts takes 1 to {NHOOD_MAX} (int32 node numbers)")
        if not 0 <= E <= NHOOD_MAX:
            raise ValueError(f"graph {g} has {E} edges: spadot_nhood_counts takes at most {NHOOD_MAX} per graph")
        if L < 1 or item0 != items or eoff < 0 or loff < 0 or p0 < -1 or gid < 0:
            raise ValueError(f"graph {g}: inconsistent descriptor {desc[g].tolist()}")
        if p0 >= 0 and (p0 + L > 2 ** 32 or gid > NHOOD_MAX):
            raise ValueError(f"graph {g}: permutation indices {p0} .. {p0 + L - 1} of graph id {gid}: the indices must stay below "
                             f"2^32 and the graph id below 2^31")
        items += L
        if items > NHOOD_MAX:
            raise ValueError(f"the call holds more than {NHOOD_MAX} labelings (the grid of one launch)")
    _typed((src, torch.int32, "src"), (dst, torch.int32, "dst"), (labels, torch.uint8, "labels"))
    zero = torch.zeros((), dtype=torch.int64, device=labels.device)
    stats = []
    for g, (eoff, n, E, K, loff, L, p0, *_rest) in enumerate(desc.tolist()):
        nlab = n if p0 >= 0 else L * n
        if eoff + E > src.numel() or eoff + E > dst.numel() or loff + nlab > labels.numel():
            raise ValueError(f"graph {g}: its edges or labels reach past the end of the tensors")
        stats += _edge_ends(src, dst, eoff, E, zero) + [labels[loff:loff + nlab].max().long()]
    stats = torch.stack(stats).cpu().numpy().reshape(-1, 3)            # the one host round trip ahead of the launch
    desc[:, 10], desc[:, 11] = stats[:, 0], stats[:, 1]
    for g in range(desc.shape[0]):
        n, E, K = (int(v) for v in desc[g, 1:4])
        _refuse_edge_ends("graph", g, stats[g, 0], stats[g, 1], n, E)
        if stats[g, 2] >= K:
            raise ValueError(f"graph {g} holds the label {int(stats[g, 2])}: labels must lie in 0 .. {K - 1}")
    return desc


def nhood_launch(src, dst, labels, desc, K_max, lds_limit=None, out=None, desc_dev=None):
    """The launch of nhood_counts for a descriptor that nhood_check has returned (the library checks it again, on the host)."""
    need_cuda(src, dst, labels, out, desc_dev)
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    K_max, items = int(K_max), int(desc[:, 5].sum())
    lds_limit = _lds_limit(lds_limit, NHOOD_LDS_BYTES)
    if out is None:
        out = torch.empty((items, K_max, K_max), dtype=torch.int32, device=labels.device)
    elif out.dtype != torch.int32 or not out.is_contiguous() or out.numel() != items * K_max * K_max:
        raise ValueError(f"out must be a contiguous int32 tensor of {items} x {K_max} x {K_max} values")
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=labels.device)
    launched(model_lib().spadot_nhood_counts(_p(src), _p(dst), _p(labels), _host(desc), _p(desc_dev), int(desc.shape[0]), K_max,
                                             lds_limit, _p(out), _stream()), "spadot_nhood_counts", NHOOD_LIMITS)
    return out


def nhood_counts(src, dst, labels, desc, K_max, lds_limit=None, out=None):
    """Label-pair edge counts of many (graph, labeling) problems in ONE launch (include/spadot_model.h: spadot_nhood_counts).
    src, dst int32 and labels uint8 device tensors, the graphs back to back; desc: int64 [G, 12] on the host as the header lays
    it out (columns 10 and 11, the range of the edge ends, are filled in here).  lds_limit: the LDS bytes a workgroup may use
    (default and at most 163840); a graph whose labels do not fit reads them from global memory.  Returns int32
    [sum L, K_max, K_max] (out: the tensor to write into).  ValueError, before any launch, outside the limits."""
    return nhood_launch(src, dst, labels, nhood_check(src, dst, labels, desc, K_max), K_max, lds_limit, out)


TERRITORY_DESC = 14
TERRITORY_LDS_BYTES = 163840
TERRITORY_FIXED = 1024            # the per-label tables and flags of a workgroup, ahead of its per-node arrays
TERRITORY_LIMITS = (NHOOD_LIMITS + "; a problem stays in LDS where 1024 + 8 n + (n rounded up to 16) <= lds_limit <= 163840 bytes (9 "
                    "bytes a node: n <= 18090) and works in its scratch slab of 2 n + ceil(n / 4) ints per labeling otherwise")


def territory_lds_bytes(n):
    """The LDS bytes a problem of n nodes needs to stay on chip: the fixed tables, then parent, size (int32) and label byte."""
    return TERRITORY_FIXED + 8 * n + ((n + 15) & ~15)


def territory_slab_ints(n):
    return 2 * n + (n + 3) // 4


def territory_check(src, dst, labels, desc, K_max):
    """The refusals of territory_counts, before any launch: those of nhood_check on the columns 0 .. 11 (limits, then the range
    of the edge ends and the largest label by reductions on the device, one host round trip) and column 12 >= -1.  Returns the
    descriptor with columns 10 and 11 filled in; ValueError otherwise."""
    desc = _host_desc(desc, TERRITORY_DESC, "problem")
    if (desc[:, 12] < -1).any():
        raise ValueError(f"problem {int(np.flatnonzero(desc[:, 12] < -1)[0])}: inconsistent descriptor (column 12 is -1 or the first "
                         f"node in ids)")
    try:
        desc[:, :NHOOD_DESC] = nhood_check(src, dst, labels, desc[:, :NHOOD_DESC], K_max)
    except ValueError as e:
        raise ValueError(str(e).replace("spadot_nhood_counts", "spadot_territory_counts")) from None
    return desc


def territory_launch(src, dst, labels, desc, K_max, lds_limit=None):
    """The launch of territory_counts for a descriptor that territory_check has returned (the library checks it again, on the
    host).  Column 13, the slab offsets, is filled in here, the scratch tensor made and the descriptor uploaded.  Returns (out int64 [items, K_max, 4], ids
    int32, sizes int32 -- both of the length the descriptor's column 12 asks for --, status int32 [items, 2])."""
    need_cuda(src, dst, labels)
    desc = np.array(desc, dtype=np.int64, order="C", copy=True)
    K_max, items = int(K_max), int(desc[:, 5].sum())
    lds_limit = _lds_limit(lds_limit, TERRITORY_LDS_BYTES)
    slabs = n_ids = 0
    for g in range(desc.shape[0]):
        n, L = int(desc[g, 1]), int(desc[g, 5])
        if desc[g, 12] >= 0:
            n_ids = max(n_ids, int(desc[g, 12]) + n)
        if territory_lds_bytes(n) > lds_limit:
            desc[g, 13] = slabs
            slabs += L * territory_slab_ints(n)
    dev = labels.device
    out = torch.empty((items, K_max, 4), dtype=torch.int64, device=dev)
    status = torch.empty((items, 2), dtype=torch.int32, device=dev)
    ids = torch.empty(n_ids, dtype=torch.int32, device=dev)
    sizes = torch.empty(n_ids, dtype=torch.int32, device=dev)
    scratch = torch.empty(slabs, dtype=torch.int32, device=dev)
    desc_dev = torch.as_tensor(desc, device=dev)
    launched(model_lib().spadot_territory_counts(_p(src), _p(dst), _p(labels), _host(desc), _p(desc_dev), int(desc.shape[0]), K_max,
                                                 lds_limit, _p(out), _p(ids) if n_ids else None, _p(sizes) if n_ids else None,
                                                 n_ids, _p(status), _p(scratch) if slabs else None, slabs, _stream()),
             "spadot_territory_counts", TERRITORY_LIMITS)
    return out, ids, sizes, status


def territory_counts(src, dst, labels, desc, K_max, lds_limit=None):
    """The territories of many (graph, labeling) problems in ONE launch (include/spadot_model.h: spadot_territory_counts).  src,
    dst int32 and labels uint8 device tensors, the graphs back to back; desc: int64 [G, 14] on the host as the header lays it
    out (columns 10, 11 and 13 are filled in here).  lds_limit: the LDS bytes a workgroup may use (default and at most 163840); a
    problem that needs more works in a slab of global scratch.  Returns (out, ids, sizes, status) as territory_launch does.
    ValueError, before any launch, outside the limits."""
    return territory_launch(src, dst, labels, territory_check(src, dst, labels, desc, K_max), K_max, lds_limit)


HOP_DESC = 15
HOP_LDS_BYTES = 163840
HOP_FIXED = 16640                 # the per-(set, class) tables, eccentricities and flags of a workgroup, ahead of its per-node arrays
HOP_SETS = 32                     # the source sets of one item: the bits of a mask
HOP_LIMITS = (NHOOD_LIMITS + "; a source problem has one explicit labeling, ceil(n / 32) items and K_max = 32; a problem stays in "
              "LDS where 16640 + 8 n + (n rounded up to 16) <= lds_limit <= 163840 bytes (9 bytes a node: n <= 16354) and works "
              "in its scratch slab of 2 n + ceil(n / 4) ints per item otherwise")


def hop_lds_bytes(n):
    """The LDS bytes a problem of n nodes needs to stay on chip: the fixed tables, then the two masks (uint32) and the class byte."""
    return HOP_FIXED + 8 * n + ((n + 15) & ~15)


def hop_slab_ints(n):
    return 2 * n + (n + 3) // 4


def hop_check(src, dst, labels, desc, K_max):
    """The refusals of hop_sums, before any launch: those of nhood_check on the columns 0 .. 11 (limits, then the range of the
    edge ends and the largest label by reductions on the device, one host round trip), column 12 >= -1, column 14 in (0, 1) and,
    for a source problem (column 14 = 1), one explicit labeling, ceil(n / 32) items, no hops and K_max = 32.  Returns the
    descriptor with columns 10 and 11 filled in; ValueError otherwise."""
    desc = _host_desc(desc, HOP_DESC, "problem")
    if (desc[:, 12] < -1).any():
        raise ValueError(f"problem {int(np.flatnonzero(desc[:, 12] < -1)[0])}: inconsistent descriptor (column 12 is -1 or the first "
                         f"int in hops)")
    for g, row in enumerate(desc.tolist()):
        if row[14] not in (0, 1):
            raise ValueError(f"problem {g}: inconsistent descriptor (column 14 is 0 for label items, 1 for source items)")
        if row[14] == 1 and (row[6] != -1 or row[5] != (row[1] + HOP_SETS - 1) // HOP_SETS or row[12] != -1):
            raise ValueError(f"problem {g}: a source problem has one explicit labeling, ceil(n / {HOP_SETS}) items and no hops "
                             f"(got {row})")
        if row[14] == 1 and int(K_max) != HOP_SETS:
            raise ValueError(f"problem {g}: spadot_hop_sums takes source problems with K_max = {HOP_SETS} only (got {int(K_max)})")
    seen = desc[:, :NHOOD_DESC].copy()
    seen[desc[:, 14] == 1, 6] = 0                       # a source problem reads one labeling of n labels, as a permuted one does
    try:
        seen = nhood_check(src, dst, labels, seen, K_max)
    except ValueError as e:
        raise ValueError(str(e).replace("spadot_nhood_counts", "spadot_hop_sums")) from None
    desc[:, 10], desc[:, 11] = seen[:, 10], seen[:, 11]
    return desc


def hop_launch(src, dst, labels, desc, K_max, lds_limit=None):
    """The launch of hop_sums for a descriptor that hop_check has returned (the library checks it again, on the host).  Column
    13, the slab offsets, is filled in here, the scratch tensor made and the descriptor uploaded.  Returns (out int64
    [items, K_max, K_max, 3], ecc int32 [items, K_max], hops int32 of the length the descriptor's column 12 asks for, status
    int32 [items, 2])."""
    need_cuda(src, dst, labels)
    desc = np.array(desc, dtype=np.int64, order="C", copy=True)
    K_max, items = int(K_max), int(desc[:, 5].sum())
    lds_limit = _lds_limit(lds_limit, HOP_LDS_BYTES)
    slabs = n_hops = 0
    for g in range(desc.shape[0]):
        n, K, L = int(desc[g, 1]), int(desc[g, 3]), int(desc[g, 5])
        if desc[g, 12] >= 0:
            n_hops = max(n_hops, int(desc[g, 12]) + n * K)
        if hop_lds_bytes(n) > lds_limit:
            desc[g, 13] = slabs
            slabs += L * hop_slab_ints(n)
    dev = labels.device
    out = torch.empty((items, K_max, K_max, 3), dtype=torch.int64, device=dev)
    ecc = torch.empty((items, K_max), dtype=torch.int32, device=dev)
    status = torch.empty((items, 2), dtype=torch.int32, device=dev)
    hops = torch.empty(n_hops, dtype=torch.int32, device=dev)
    scratch = torch.empty(slabs, dtype=torch.int32, device=dev)
    desc_dev = torch.as_tensor(desc, device=dev)
    launched(model_lib().spadot_hop_sums(_p(src), _p(dst), _p(labels), _host(desc), _p(desc_dev), int(desc.shape[0]), K_max,
                                         lds_limit, _p(out), _p(ecc), _p(hops) if n_hops else None, n_hops, _p(status),
                                         _p(scratch) if slabs else None, slabs, _stream()),
             "spadot_hop_sums", HOP_LIMITS)
    return out, ecc, hops, status


def hop_sums(src, dst, labels, desc, K_max, lds_limit=None):
    """The hop distances from every source set of many (graph, labeling) problems in ONE launch (include/spadot_model.h:
    spadot_hop_sums).  src, dst int32 and labels uint8 device tensors, the graphs back to back; desc: int64 [G, 15] on the host
    as the header lays it out (columns 10, 11 and 13 are filled in here).  lds_limit: the LDS bytes a workgroup may use (default
    and at most 163840); a problem that needs more works in a slab of global scratch.  Returns (out, ecc, hops, status) as
    hop_launch does.  ValueError, before any launch, outside the limits."""
    return hop_launch(src, dst, labels, hop_check(src, dst, labels, desc, K_max), K_max, lds_limit)


COOCCUR_MAX_K = 32
COOCCUR_MAX_B = 64
COOCCUR_GRANULE = 16               # the thresholds of a problem are padded to a multiple of this with -1.0
COOCCUR_MAX_N = 2147483391         # spots of a problem: int32 positions of a 256-wide tile (as spadot_silhouette)
COOCCUR_MAX_P = 65535              # problems of a call (gridDim.y)
COOCCUR_DESC = 40
COOCCUR_LIMITS = ("1 <= K <= 32 label values, 1 <= B <= 64 thresholds that are finite, >= 0 and strictly increasing, "
                  "1 <= n <= 2147483391 spots per problem, at most 65535 problems per call")
COOCCUR_DESC_G = 37                # the problem number g of the null: K <= 32 leaves the columns 37 .. 39 of a descriptor free
COOCCUR_MAX_Y = 65535              # patterns of a call of the null (gridDim.y; its problems are gridDim.z)
COOCCUR_MAX_G = 2147483647         # problem numbers, as the graph ids of spadot_nhood_counts
COOCCUR_NULL_LIMITS = (COOCCUR_LIMITS + ", 1 to 65535 patterns per call, relabelings first >= 0 with first + n_perms <= 2^31, "
                       "problem numbers in 0 .. 2147483647")


def cooccur_padded(B_max):
    """The threshold columns of a call whose largest problem has B_max thresholds."""
    return (int(B_max) + COOCCUR_GRANULE - 1) // COOCCUR_GRANULE * COOCCUR_GRANULE


def _cluster_offsets_ok(coff, n):
    """The cluster-offset rule of the stages that count pairs by distance: a problem's K + 1 offsets ascend from 0 to n."""
    return coff[0] == 0 and coff[-1] == n and all(hi >= lo for lo, hi in zip(coff, coff[1:]))


def _padded_thresholds(pad, p, t, B):
    """Writes the B squared thresholds t of problem p, given as they are or already padded to pad's width with -1.0, into row p
    of pad (fp64 [P, BP], filled with -1.0); ValueError unless they are B finite values >= 0 in strictly increasing order."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    if t.shape[0] == pad.shape[1] and np.all(t[B:] == -1.0):
        t = t[:B]
    if t.shape[0] != B:
        raise ValueError(f"problem {p} has {t.shape[0]} thresholds and its descriptor says {B}")
    if not np.all(np.isfinite(t)) or np.any(t < 0) or np.any(np.diff(t) <= 0):
        raise ValueError(f"the squared thresholds of problem {p} must be finite, >= 0 and strictly increasing")
    pad[p, :B] = t


def _out_int64(out, shape, device):
    """The int64 output of a counting launch: a fresh tensor of `shape`, or the caller's if it is contiguous and of that size."""
    if out is None:
        return torch.empty(shape, dtype=torch.int64, device=device)
    if out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != int(np.prod(shape, dtype=object)):
        raise ValueError(f"out must be a contiguous int64 tensor of {' x '.join(str(v) for v in shape)} values")
    return out


def cooccur_check(xy, desc, r2, K_max, B_max):
    """The refusals of cooccur_counts that the descriptor and the thresholds decide, before any launch.  Returns (desc int64
    [P, 40], r2 fp64 [P, BP] padded with -1.0); ValueError otherwise.  r2: [P] sequences of squared thresholds, or the padded
    array itself."""
    need_cuda(xy)
    desc = _host_desc(desc, COOCCUR_DESC, "problem")
    K_max, B_max, P = int(K_max), int(B_max), desc.shape[0]
    if not 1 <= K_max <= COOCCUR_MAX_K:
        raise ValueError(f"spadot_cooccur_counts takes 1 to {COOCCUR_MAX_K} label values (got K_max = {K_max})")
    if not 1 <= B_max <= COOCCUR_MAX_B:
        raise ValueError(f"spadot_cooccur_counts takes 1 to {COOCCUR_MAX_B} thresholds (got B_max = {B_max})")
    if P > COOCCUR_MAX_P:
        raise ValueError(f"the call holds {P} problems: spadot_cooccur_counts takes at most {COOCCUR_MAX_P} (the grid of one "
                         f"launch)")
    if len(r2) != P:
        raise ValueError(f"the call holds {P} problems and {len(r2)} sets of thresholds")
    pad = np.full((P, cooccur_padded(B_max)), -1.0, dtype=np.float64)
    first = 0
    for p, row in enumerate(desc.tolist()):
        off, n, K, B = row[:4]
        if not 1 <= K <= K_max:
            raise ValueError(f"problem {p} has {K} label values: spadot_cooccur_counts takes 1 to {K_max} here, at most "
                             f"{COOCCUR_MAX_K}")
        if not 1 <= B <= B_max:
            raise ValueError(f"problem {p} has {B} thresholds: spadot_cooccur_counts takes 1 to {B_max} here, at most "
                             f"{COOCCUR_MAX_B}")
        if not 1 <= n <= COOCCUR_MAX_N:
            raise ValueError(f"problem {p} has {n} spots: spadot_cooccur_counts takes 1 to {COOCCUR_MAX_N} (int32 positions)")
        if off != first or not _cluster_offsets_ok(row[4:5 + K], n):
            raise ValueError(f"problem {p}: inconsistent descriptor {row[:5 + K]}")
        first += n
        _padded_thresholds(pad, p, r2[p], B)
    if xy.dtype != torch.float64 or xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_contiguous() or xy.shape[0] != first:
        raise ValueError(f"xy must be a contiguous fp64 [{first}, 2] tensor (got {tuple(xy.shape)} {xy.dtype})")
    return desc, pad


def _cooccur_launch(xy, desc, r2, K_max, B_max, null, out, desc_dev, r2_dev):
    """The launch of both entries.  null: None for spadot_cooccur_counts, (observed, first, n_perms, seed) for spadot_cooccur_null."""
    need_cuda(xy, out, desc_dev, r2_dev)
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    r2 = np.ascontiguousarray(r2, dtype=np.float64)
    K_max, B_max, P = int(K_max), int(B_max), int(desc.shape[0])
    out = _out_int64(out, (P,) + (() if null is None else (int(null[0]) + int(null[2]),)) + (K_max, K_max, B_max), xy.device)
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=xy.device)
    if r2_dev is None:
        r2_dev = torch.as_tensor(r2, device=xy.device)
    args = (_p(xy), _host(desc), _p(desc_dev), _host(r2), _p(r2_dev), P, K_max, B_max)
    if null is None:
        launched(model_lib().spadot_cooccur_counts(*args, _p(out), _stream()), "spadot_cooccur_counts", COOCCUR_LIMITS)
    else:
        observed, first, n_perms, seed = null
        launched(model_lib().spadot_cooccur_null(*args, int(observed), int(first), int(n_perms), _signed64(seed), _p(out),
                                                 _stream()), "spadot_cooccur_null", COOCCUR_NULL_LIMITS)
    return out


def cooccur_launch(xy, desc, r2, K_max, B_max, out=None, desc_dev=None, r2_dev=None):
    """The launch of cooccur_counts for what cooccur_check has returned (the library checks both again, on the host)."""
    return _cooccur_launch(xy, desc, r2, K_max, B_max, None, out, desc_dev, r2_dev)


def cooccur_counts(xy, desc, r2, K_max, B_max, out=None):
    """Label-pair counts by distance of many problems in ONE counting launch (include/spadot_model.h: spadot_cooccur_counts).
    xy: fp64 [sum n, 2] device tensor, per problem its spots ordered by (label, index), the problems back to back; desc: int64
    [P, 40] on the host as the header lays it out; r2[p]: the squared thresholds of problem p.  Returns int64
    [P, K_max, K_max, B_max] (out: the tensor to write into).  ValueError, before any launch, outside the limits."""
    desc, pad = cooccur_check(xy, desc, r2, K_max, B_max)
    return cooccur_launch(xy, desc, pad, K_max, B_max, out)


def cooccur_null_check(xy, desc, r2, K_max, B_max, observed, first, n_perms):
    """The refusals of cooccur_null_counts, before any launch: those of cooccur_check, the problem numbers in column 37 of the
    descriptor and the patterns of the call.  Returns (desc, r2 padded, observed as 0 / 1, first, n_perms); ValueError
    otherwise."""
    desc, pad = cooccur_check(xy, desc, r2, K_max, B_max)
    observed, first, n_perms = labelings("cooccur_null_counts", observed, first, n_perms)
    if not 1 <= observed + n_perms <= COOCCUR_MAX_Y:
        raise ValueError(f"the call holds {observed + n_perms} patterns: spadot_cooccur_null takes 1 to {COOCCUR_MAX_Y} (the grid "
                         f"of one launch)")
    if first + n_perms > 2 ** 31:
        raise ValueError(f"relabelings {first} .. {first + n_perms - 1}: spadot_cooccur_null takes indices below 2^31")
    for p, g in enumerate(desc[:, COOCCUR_DESC_G].tolist()):
        if not 0 <= g <= COOCCUR_MAX_G:
            raise ValueError(f"problem {p} has the problem number {g}: spadot_cooccur_null takes 0 to {COOCCUR_MAX_G}")
    return desc, pad, observed, first, n_perms


def cooccur_null_launch(xy, checked, K_max, B_max, seed=0, out=None, desc_dev=None, r2_dev=None):
    """The launch of cooccur_null_counts for what cooccur_null_check has returned (the library checks it again, on the host)."""
    desc, r2, observed, first, n_perms = checked
    return _cooccur_launch(xy, desc, r2, K_max, B_max, (observed, first, n_perms, seed), out, desc_dev, r2_dev)


def cooccur_null_counts(xy, desc, r2, K_max, B_max, observed, first, n_perms, seed=0, out=None):
    """The label-pair counts by distance of the observed labeling (observed) and of the relabelings first .. first + n_perms - 1
    of many problems in ONE counting launch (include/spadot_model.h: spadot_cooccur_null).  xy, desc, r2 as for cooccur_counts,
    with the problem number g of a problem in column 37 of its descriptor.  Returns int64 [P, observed + n_perms, K_max, K_max,
    B_max] (out: the tensor to write into).  ValueError, before any launch, outside the limits."""
    checked = cooccur_null_check(xy, desc, r2, K_max, B_max, observed, first, n_perms)
    return cooccur_null_launch(xy, checked, K_max, B_max, seed, out)


AUTOCORR_DESC = 7
AUTOCORR_MAX = 2147483647          # spots, edges and stored entries (int32), graph ids, and workgroups of a call (gridDim.x)
AUTOCORR_LDS_BYTES = 163840
AUTOCORR_LDS_FIXED = 2048          # LDS beside the image: the reduction and the segment bounds
AUTOCORR_THREADS = 1024            # the library's defaults (Time)
AUTOCORR_GS = 2
AUTOCORR_LIMITS = ("1 <= n <= 2147483647 spots and at most 2147483647 edges per time point, at most 2147483647 stored entries, every "
                   "edge end in 0 .. n-1, every row index inside the time points, permutation indices below 2^32, at most "
                   "2147483647 workgroups per call, threads in (256, 512, 1024), gs in (2, 4)")


def autocorr_check(src, dst, colptr, ridx, values, centre, desc, g0, ng, observed, first, P):
    """The refusals of autocorr_sums, before any launch: the limits from the descriptor and the ranges, then the range of the
    edge ends of every time point, the range of the row indices and the order of colptr by reductions on the device (one host
    round trip).  Returns (the descriptor with columns 5 and 6 filled in, the smallest row index, the largest); ValueError
    otherwise."""
    need_cuda(src, dst, colptr, ridx, values, centre)
    desc = _host_desc(desc, AUTOCORR_DESC, "time point")
    T, g0, ng = int(desc.shape[0]), int(g0), int(ng)
    _typed((src, torch.int32, "src"), (dst, torch.int32, "dst"), (ridx, torch.int32, "ridx"), (colptr, torch.int64, "colptr"),
           (values, torch.float32, "values"), (centre, torch.float64, "centre"), any_dim=("centre",))
    G, nnz = _csc_sizes(colptr, ridx, values, AUTOCORR_MAX)
    if tuple(centre.shape) != (T, G):
        raise ValueError(f"centre must be [T, G] = [{T}, {G}] (got {tuple(centre.shape)})")
    if g0 < 0 or ng < 1 or g0 + ng > G:
        raise ValueError(f"the genes {g0} .. {g0 + ng - 1} are not a range of the {G} genes")
    observed, first, P = labelings("autocorr_sums", observed, first, P)
    rows = 0
    for t, (eoff, n, E, row0, gid, _lo, _hi) in enumerate(desc.tolist()):
        _refuse_time_point(t, "spadot_autocorr_sums", desc[t].tolist(), n, E, AUTOCORR_MAX,
                           eoff >= 0 and 0 <= row0 <= AUTOCORR_MAX and 0 <= gid <= AUTOCORR_MAX)
        if eoff + E > src.numel() or eoff + E > dst.numel():
            raise ValueError(f"time point {t}: its edges reach past the end of the tensors")
        rows = max(rows, row0 + n)
    if T * (observed + P) * -(-ng // 2) > AUTOCORR_MAX:
        raise ValueError(f"the call holds more than {AUTOCORR_MAX} workgroups (the grid of one launch)")
    zero = torch.zeros((), dtype=torch.int64, device=colptr.device)
    stats = [s for eoff, _n, E, *_rest in desc.tolist() for s in _edge_ends(src, dst, eoff, E, zero)]
    stats = torch.stack(stats + _csc_stats(colptr, ridx, zero)).cpu().numpy()   # the one host round trip ahead of the launch
    ends = stats[:2 * T].reshape(T, 2)
    desc[:, 5], desc[:, 6] = ends[:, 0], ends[:, 1]
    for t in range(T):
        _refuse_edge_ends("time point", t, ends[t, 0], ends[t, 1], int(desc[t, 1]), int(desc[t, 2]))
    ridx_lo, ridx_hi, c0, c1, unordered = (int(v) for v in stats[2 * T:])
    _refuse_rows(ridx_lo, ridx_hi, nnz, rows)
    _refuse_colptr(c0, c1, unordered, nnz)
    return desc, ridx_lo, ridx_hi


def autocorr_scratch_floats(desc, ng, L, lds_limit=None, gs=None):
    """The floats of the scratch buffer of a call (0: every image fits in LDS), as the library computes it."""
    gs = AUTOCORR_GS if not gs else int(gs)
    lds_limit = AUTOCORR_LDS_BYTES if lds_limit is None else min(int(lds_limit), AUTOCORR_LDS_BYTES)
    slab = max([(gs * int(n) + 3) & ~3 for n in desc[:, 1] if AUTOCORR_LDS_FIXED + 4 * gs * int(n) > lds_limit] or [0])
    return slab * int(desc.shape[0]) * int(L) * -(-int(ng) // gs)


def autocorr_launch(src, dst, colptr, ridx, values, centre, checked, g0, ng, observed, first, P, seed=0, lds_limit=None, out=None,
                    scratch=None, threads=None, gs=None, desc_dev=None):
    """The launch of autocorr_sums for what autocorr_check has returned (the library checks the descriptor again, on the host)."""
    desc, ridx_lo, ridx_hi = checked
    need_cuda(src, dst, colptr, ridx, values, centre, scratch, desc_dev, *(out or ()))
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    T, G, L = int(desc.shape[0]), int(colptr.numel()) - 1, int(bool(observed)) + int(P)
    lds_limit = _lds_limit(lds_limit, AUTOCORR_LDS_BYTES)
    threads, gs = int(threads or 0), int(gs or 0)
    if threads not in (0, 256, 512, 1024) or gs not in (0, 2, 4):         # the library's refusal, ahead of the call
        launched(-7, "spadot_autocorr_sums", AUTOCORR_LIMITS)
    dev = colptr.device
    if out is None:
        out = tuple(torch.empty((T, int(ng), L), dtype=torch.float64, device=dev) for _ in range(2))
    elif len(out) != 2 or any(o.dtype != torch.float64 or not o.is_contiguous() or o.numel() != T * int(ng) * L for o in out):
        raise ValueError(f"out must be two contiguous float64 tensors of {T} x {int(ng)} x {L} values")
    need = autocorr_scratch_floats(desc, ng, L, lds_limit, gs)
    if need and scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    elif need and (scratch.dtype != torch.float32 or not scratch.is_contiguous() or scratch.numel() < need):
        raise ValueError(f"scratch must be a contiguous float32 tensor of at least {need} values")
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=dev)
    rc = model_lib().spadot_autocorr_sums(_p(src), _p(dst), _p(colptr), _p(ridx), _p(values), int(ridx.numel()), ridx_lo, ridx_hi,
                                          _p(centre), _host(desc), _p(desc_dev), T, G, int(g0), int(ng), int(bool(observed)),
                                          int(first), int(P), _signed64(seed), lds_limit, _p(scratch) if need else None,
                                          int(scratch.numel()) if need else 0, threads, gs, _p(out[0]), _p(out[1]), _stream())
    launched(rc, "spadot_autocorr_sums", AUTOCORR_LIMITS)
    return out


def autocorr_sums(src, dst, colptr, ridx, values, centre, desc, g0, ng, observed, first, P, seed=0, lds_limit=None, out=None,
                  scratch=None, threads=None, gs=None):
    """The edge sums N and D behind Moran's I and Geary's C of every (time point, gene, labeling) in ONE launch
    (include/spadot_model.h: spadot_autocorr_sums).  src, dst int32 edge ends of the time points back to back; colptr int64,
    ridx int32 and values fp32: the CSC arrays of a DeviceCounts; centre fp64 [T, G]; desc: int64 [T, 7] on the host as the
    header lays it out (columns 5 and 6, the range of the edge ends, are filled in here).  Labelings: the identity (observed)
    and the permutations first .. first + P - 1 under seed.  lds_limit: the LDS bytes a workgroup may use (default and at most
    163840); a time point whose image does not fit keeps it in `scratch` (allocated here when not given).  Returns (N, D), fp64
    device tensors [T, ng, observed + P] (out: the pair to write into).  ValueError, before any launch, outside the limits;
    RuntimeError for a CPU tensor."""
    checked = autocorr_check(src, dst, colptr, ridx, values, centre, desc, g0, ng, observed, first, P)
    return autocorr_launch(src, dst, colptr, ridx, values, centre, checked, g0, ng, observed, first, P, seed, lds_limit, out,
                           scratch, threads, gs)


LIGREC_DESC = 3
LIGREC_MAX_K = 32
LIGREC_MAX = 2147483647            # spots and stored entries (int32), graph ids, and workgroups of a call (gridDim.x)
LIGREC_LDS_BYTES = 163840
LIGREC_THREADS = 512               # the library's defaults (Time)
LIGREC_GC = 128
LIGREC_LIMITS = ("1 <= K <= 32 label values, every label below K, 1 <= n <= 2147483647 spots per time point, at most 2147483647 "
                 "stored entries, every row index inside the time points, every selected gene inside the genes, permutation "
                 "indices below 2^32, at most 2147483647 workgroups per call, threads in (256, 512), gene_chunk >= 1")


def ligrec_lds_bytes(n, K, threads=None):
    """The LDS bytes a workgroup needs to keep the labels of a time point of n spots beside its accumulators."""
    return int(threads or LIGREC_THREADS) // 64 * int(K) * 512 + ((int(n) + 15) & ~15)


def ligrec_check(colptr, ridx, values, labels, genes, desc, K, observed, first, P, gene_chunk=None):
    """The refusals of ligrec_sums, before any launch: the limits from the descriptor and the ranges, then the range of the row
    indices, of the labels and of the selected genes and the order of colptr by reductions on the device (one host round trip).
    Returns (the descriptor, the smallest row index, the largest, the largest label, the smallest selected gene, the largest);
    ValueError otherwise."""
    need_cuda(colptr, ridx, values, labels, genes)
    desc = _host_desc(desc, LIGREC_DESC, "time point")
    T, K = int(desc.shape[0]), int(K)
    gc = LIGREC_GC if not gene_chunk else int(gene_chunk)
    _typed((ridx, torch.int32, "ridx"), (colptr, torch.int64, "colptr"), (values, torch.float32, "values"),
           (labels, torch.uint8, "labels"), (genes, torch.int32, "genes"))
    if not 1 <= K <= LIGREC_MAX_K:
        raise ValueError(f"spadot_ligrec_sums takes 1 to {LIGREC_MAX_K} label values (got K = {K})")
    (G, nnz), ng = _csc_sizes(colptr, ridx, values, LIGREC_MAX), int(genes.numel())
    if ng < 1 or gc < 1:
        raise ValueError(f"spadot_ligrec_sums takes at least one selected gene and gene_chunk >= 1 (got {ng} genes, gene_chunk = "
                         f"{gc})")
    observed, first, P = labelings("ligrec_sums", observed, first, P)
    rows = 0
    for t, (n, row0, gid) in enumerate(desc.tolist()):
        if not 1 <= n <= LIGREC_MAX:
            raise ValueError(f"time point {t} has {n} spots: spadot_ligrec_sums takes 1 to {LIGREC_MAX} (int32 spot numbers)")
        if not 0 <= row0 <= LIGREC_MAX or not 0 <= gid <= LIGREC_MAX:
            raise ValueError(f"time point {t}: inconsistent descriptor {desc[t].tolist()}")
        rows = max(rows, row0 + n)
    if labels.numel() < rows:
        raise ValueError(f"labels holds {int(labels.numel())} bytes: one per row of the time points, {rows}")
    if T * (observed + P) * -(-ng // gc) > LIGREC_MAX:
        raise ValueError(f"the call holds more than {LIGREC_MAX} workgroups (the grid of one launch)")
    zero = torch.zeros((), dtype=torch.int64, device=colptr.device)
    stats = _csc_stats(colptr, ridx, zero) + [s.long() for s in (labels[:rows].max(), *torch.aminmax(genes))]
    ridx_lo, ridx_hi, c0, c1, unordered, label_hi, gene_lo, gene_hi = (
        int(v) for v in torch.stack(stats).cpu().numpy())                                        # the one host round trip
    _refuse_rows(ridx_lo, ridx_hi, nnz, rows)
    if label_hi >= K:
        raise ValueError(f"labels holds the label {label_hi}: labels must lie in 0 .. {K - 1}")
    _refuse_genes(gene_lo, gene_hi, G)
    _refuse_colptr(c0, c1, unordered, nnz)
    return desc, ridx_lo, ridx_hi, label_hi, gene_lo, gene_hi


def ligrec_launch(colptr, ridx, values, labels, genes, checked, K, observed, first, P, seed=0, lds_limit=None, out=None,
                  threads=None, gene_chunk=None, desc_dev=None):
    """The launch of ligrec_sums for what ligrec_check has returned (the library checks the descriptor again, on the host)."""
    desc, ridx_lo, ridx_hi, label_hi, gene_lo, gene_hi = checked
    need_cuda(colptr, ridx, values, labels, genes, desc_dev, *(out or ()))
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    T, G, K, ng = int(desc.shape[0]), int(colptr.numel()) - 1, int(K), int(genes.numel())
    observed, L = int(bool(observed)), int(bool(observed)) + int(P)
    lds_limit = _lds_limit(lds_limit, LIGREC_LDS_BYTES)
    threads, gc = int(threads or 0), int(gene_chunk or 0)
    if threads not in (0, 256, 512) or gc < 0:                            # the library's refusal, ahead of the call
        launched(-7, "spadot_ligrec_sums", LIGREC_LIMITS)
    dev = colptr.device
    if out is None:
        out = (torch.empty((T, L, ng, K), dtype=torch.float64, device=dev),
               torch.empty((T, ng, K), dtype=torch.int32, device=dev) if observed else None)
    elif (len(out) != 2 or out[0].dtype != torch.float64 or not out[0].is_contiguous() or out[0].numel() != T * L * ng * K
          or (observed and (out[1] is None or out[1].dtype != torch.int32 or not out[1].is_contiguous()
                            or out[1].numel() != T * ng * K))):
        raise ValueError(f"out must be a contiguous float64 tensor of {T} x {L} x {ng} x {K} values and, with the observed "
                         f"labeling, a contiguous int32 tensor of {T} x {ng} x {K}")
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=dev)
    rc = model_lib().spadot_ligrec_sums(_p(colptr), _p(ridx), _p(values), int(ridx.numel()), ridx_lo, ridx_hi, _p(labels), label_hi,
                                        _host(desc), _p(desc_dev), T, G, K, _p(genes), ng, gene_lo, gene_hi, observed, int(first),
                                        int(P), _signed64(seed), lds_limit, threads, gc, _p(out[0]),
                                        _p(out[1]) if observed else None, _stream())
    launched(rc, "spadot_ligrec_sums", LIGREC_LIMITS)
    return out


def ligrec_sums(colptr, ridx, values, labels, genes, desc, K, observed, first, P, seed=0, lds_limit=None, out=None, threads=None,
                gene_chunk=None):
    """The per-domain expression sums of the selected genes of every (time point, labeling) in ONE launch
    (include/spadot_model.h: spadot_ligrec_sums).  colptr int64, ridx int32 and values fp32: the CSC arrays of a DeviceCounts;
    labels uint8, one per row; genes int32: the selected genes; desc: int64 [T, 3] on the host as the header lays it out.
    Labelings: the labels themselves (observed) and the permutations first .. first + P - 1 under seed.  lds_limit: the LDS
    bytes a workgroup may use (default and at most 163840); a time point whose labels do not fit beside the accumulators
    permutes per stored entry.  Returns (S fp64 [T, observed + P, genes, K], c int32 [T, genes, K] or None without the observed
    labeling) on the device (out: the pair to write into).  ValueError, before any launch, outside the limits; RuntimeError for a
    CPU tensor."""
    checked = ligrec_check(colptr, ridx, values, labels, genes, desc, K, observed, first, P, gene_chunk)
    return ligrec_launch(colptr, ridx, values, labels, genes, checked, K, observed, first, P, seed, lds_limit, out, threads,
                         gene_chunk)


def ligrec_count(S0, S, wk, pairs, pair_range, mask, skip, ge):
    """Adds, for every masked cell, the labelings l >= skip of the run S [T, L, ns, K] whose statistic is at least that of S0
    [T, ns, K] into ge int32 [T, M, K, K] (include/spadot_model.h: spadot_ligrec_count).  wk fp64 [T, K]; pairs int32 [M, 2]
    positions in the selected genes, pair_range their (smallest, largest); mask uint8 [T, M, K, K]."""
    need_cuda(S0, S, wk, pairs, mask, ge)
    T, L, ns, K = (int(v) for v in S.shape)
    M = int(pairs.shape[0])
    for t, dt, shape, what in ((S0, torch.float64, (T, ns, K), "S0"), (S, torch.float64, (T, L, ns, K), "S"),
                               (wk, torch.float64, (T, K), "wk"), (pairs, torch.int32, (M, 2), "pairs"),
                               (mask, torch.uint8, (T, M, K, K), "mask"), (ge, torch.int32, (T, M, K, K), "ge")):
        if t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"{what} must be a contiguous {dt} tensor {shape} (got {tuple(t.shape)} {t.dtype})")
    launched(model_lib().spadot_ligrec_count(_p(S0), _p(S), _p(wk), _p(pairs), int(pair_range[0]), int(pair_range[1]), _p(mask), T,
                                             M, ns, K, L, int(skip), _p(ge), _stream()),
             "spadot_ligrec_count", f"K <= {LIGREC_MAX_K}, pairs inside the {ns} selected genes")
    return ge


LOCAL_DESC = 8
LOCAL_MAX = 2147483647             # spots, edges and stored entries (int32), graph ids, and workgroups of a call (gridDim.x)
LOCAL_LDS_BYTES = 163840
LOCAL_LDS_FIXED = 256              # LDS beside the image: the segment bounds
LOCAL_THREADS = 1024               # the library's defaults (Time)
LOCAL_GS = 4
LOCAL_CHUNK = 128
LOCAL_LIMITS = ("P >= 1 permutations, 1 <= n <= 2147483647 spots and at most 2147483647 edges per time point, at most 2147483647 "
                "stored entries, every entry of col in 0 .. n-1, every row index inside the time points, every selected gene inside "
                "the genes, permutation indices below 2^32, at most 2147483647 workgroups per call, threads in (256, 512, 1024), "
                "gs in (2, 4), perm_chunk >= 1")


def local_lds_bytes(n, gs=None):
    """The LDS bytes a workgroup needs to keep the image of a time point of n spots (the per-spot state lives in global memory:
    DESIGN 7l)."""
    return LOCAL_LDS_FIXED + 4 * int(gs or LOCAL_GS) * int(n)


def local_scratch_bytes(desc, ng, P, lds_limit=None, gs=None, perm_chunk=None):
    """The bytes of the scratch buffer of a call (the per-spot state of every workgroup and the images that do not fit in LDS),
    as the library computes it."""
    gs, chunk = int(gs or LOCAL_GS), int(perm_chunk or LOCAL_CHUNK)
    lds_limit = LOCAL_LDS_BYTES if lds_limit is None else min(int(lds_limit), LOCAL_LDS_BYTES)
    spots = max(int(n) for n in desc[:, 1])
    slab = max([(gs * int(n) + 3) & ~3 for n in desc[:, 1] if local_lds_bytes(n, gs) > lds_limit] or [0])
    return int(desc.shape[0]) * -(-int(P) // chunk) * -(-int(ng) // gs) * (16 * gs * spots + 4 * slab)


def local_check(rowptr, col, colptr, ridx, values, centre, genes, desc, first, P, threads=None, gs=None, perm_chunk=None):
    """The refusals of local_lag, before any launch: the limits from the descriptor and the ranges, then per time point the range
    of col and the order of rowptr, the range of the row indices and of the selected genes and the order of colptr by reductions
    on the device (one host round trip).  Returns (the descriptor with columns 6 and 7 filled in, the smallest row index, the
    largest, the smallest selected gene, the largest); ValueError otherwise."""
    need_cuda(rowptr, col, colptr, ridx, values, centre, genes)
    desc = _host_desc(desc, LOCAL_DESC, "time point")
    T = int(desc.shape[0])
    _typed((rowptr, torch.int32, "rowptr"), (col, torch.int32, "col"), (ridx, torch.int32, "ridx"), (colptr, torch.int64, "colptr"),
           (values, torch.float32, "values"), (centre, torch.float64, "centre"), (genes, torch.int32, "genes"), any_dim=("centre",))
    (G, nnz), ng = _csc_sizes(colptr, ridx, values, LOCAL_MAX), int(genes.numel())
    if tuple(centre.shape) != (T, G):
        raise ValueError(f"centre must be [T, G] = [{T}, {G}] (got {tuple(centre.shape)})")
    threads, gs, chunk = int(threads or 0), int(gs or 0), int(perm_chunk or 0)
    if ng < 1 or threads not in (0, 256, 512, 1024) or gs not in (0, 2, 4) or chunk < 0:
        raise ValueError(f"spadot_local_lag takes at least one selected gene, threads in (256, 512, 1024), gs in (2, 4) and "
                         f"perm_chunk >= 1 (got {ng} genes, threads = {threads}, gs = {gs}, perm_chunk = {chunk})")
    if int(P) < 1:
        raise ValueError(f"local_lag takes P >= 1 permutations (got P = {int(P)})")
    _, first, P = labelings("local_lag", False, first, P)
    rows = 0
    for t, (eoff, n, E, row0, gid, roff, _lo, _hi) in enumerate(desc.tolist()):
        _refuse_time_point(t, "spadot_local_lag", desc[t].tolist(), n, E, LOCAL_MAX,
                           eoff >= 0 and roff >= 0 and 0 <= row0 <= LOCAL_MAX and 0 <= gid <= LOCAL_MAX)
        if eoff + E > col.numel() or roff + n + 1 > rowptr.numel():
            raise ValueError(f"time point {t}: its rows or edges reach past the end of the tensors")
        rows = max(rows, row0 + n)
    if T * -(-P // (chunk or LOCAL_CHUNK)) * -(-ng // (gs or LOCAL_GS)) > LOCAL_MAX:
        raise ValueError(f"the call holds more than {LOCAL_MAX} workgroups (the grid of one launch)")
    zero = torch.zeros((), dtype=torch.int64, device=colptr.device)
    stats = _csr_stats(rowptr, col, desc, zero) + _csc_stats(colptr, ridx, zero) + [s.long() for s in torch.aminmax(genes)]
    stats = torch.stack(stats).cpu().numpy()                                # the one host round trip ahead of the launch
    _refuse_csr(desc, stats[:5 * T].reshape(T, 5))
    ridx_lo, ridx_hi, c0, c1, unordered, gene_lo, gene_hi = (int(v) for v in stats[5 * T:])
    _refuse_rows(ridx_lo, ridx_hi, nnz, rows)
    _refuse_genes(gene_lo, gene_hi, G)
    _refuse_colptr(c0, c1, unordered, nnz)
    return desc, ridx_lo, ridx_hi, gene_lo, gene_hi


def local_launch(rowptr, col, colptr, ridx, values, centre, genes, checked, first, P, seed=0, lds_limit=None, out=None,
                 scratch=None, threads=None, gs=None, perm_chunk=None, desc_dev=None):
    """The launch of local_lag for what local_check has returned (the library checks the descriptor again, on the host).  out:
    (lag, ge, le) of an earlier launch over the same rows: ge and le are added to (the integers of disjoint runs accumulate
    exactly), lag is written again with the same bits."""
    desc, ridx_lo, ridx_hi, gene_lo, gene_hi = checked
    need_cuda(rowptr, col, colptr, ridx, values, centre, genes, scratch, desc_dev, *(out or ()))
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    T, G, ng = int(desc.shape[0]), int(colptr.numel()) - 1, int(genes.numel())
    rows = int((desc[:, 3] + desc[:, 1]).max())
    lds_limit = _lds_limit(lds_limit, LOCAL_LDS_BYTES)
    threads, gs, chunk = int(threads or 0), int(gs or 0), int(perm_chunk or 0)
    if threads not in (0, 256, 512, 1024) or gs not in (0, 2, 4) or chunk < 0:    # the library's refusal, ahead of the call
        launched(-7, "spadot_local_lag", LOCAL_LIMITS)
    dev = colptr.device
    if out is None:
        out = (torch.zeros((ng, rows), dtype=torch.float64, device=dev), torch.zeros((ng, rows), dtype=torch.int32, device=dev),
               torch.zeros((ng, rows), dtype=torch.int32, device=dev))
    elif (len(out) != 3 or any(not o.is_contiguous() or tuple(o.shape) != (ng, rows) for o in out)
          or out[0].dtype != torch.float64 or out[1].dtype != torch.int32 or out[2].dtype != torch.int32):
        raise ValueError(f"out must be a contiguous float64 and two contiguous int32 tensors [{ng}, {rows}]")
    need = local_scratch_bytes(desc, ng, P, lds_limit, gs, chunk)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < need:
        raise ValueError(f"scratch must be a contiguous uint8 tensor of at least {need} bytes")
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=dev)
    rc = model_lib().spadot_local_lag(_p(rowptr), _p(col), _p(colptr), _p(ridx), _p(values), int(ridx.numel()), ridx_lo, ridx_hi,
                                      _p(centre), _host(desc), _p(desc_dev), T, G, _p(genes), ng, gene_lo, gene_hi, int(first),
                                      int(P), _signed64(seed), lds_limit, _p(scratch), int(scratch.numel()), threads, gs, chunk,
                                      rows, _p(out[0]), _p(out[1]), _p(out[2]), _stream())
    launched(rc, "spadot_local_lag", LOCAL_LIMITS)
    return out


def local_lag(rowptr, col, colptr, ridx, values, centre, genes, desc, first, P, seed=0, lds_limit=None, out=None, scratch=None,
              threads=None, gs=None, perm_chunk=None):
    """The observed neighbour sums of local Moran's I and the counts of the conditional permutations whose sum is at least / at
    most the observed one, for every (selected gene, spot) of every time point in ONE launch (include/spadot_model.h:
    spadot_local_lag).  rowptr, col int32: the CSR of the time points back to back; colptr int64, ridx int32 and values fp32: the
    CSC arrays of a DeviceCounts; centre fp64 [T, G]; genes int32: the selected genes; desc: int64 [T, 8] on the host as the
    header lays it out (columns 6 and 7, the range of col, are filled in here).  Permutations first .. first + P - 1 under seed.
    lds_limit: the LDS bytes a workgroup may use (default and at most 163840); a time point whose image does not fit keeps it in
    `scratch` (allocated here when not given).  Returns (lag fp64, ge int32, le int32), device tensors [genes, rows].
    ValueError, before any launch, outside the limits; RuntimeError for a CPU tensor."""
    checked = local_check(rowptr, col, colptr, ridx, values, centre, genes, desc, first, P, threads, gs, perm_chunk)
    return local_launch(rowptr, col, colptr, ridx, values, centre, genes, checked, first, P, seed, lds_limit, out, scratch, threads,
                        gs, perm_chunk)


CROSS_DESC = 9
CROSS_MAX = 2147483647             # spots, edges and stored entries (int32), graph ids, and workgroups of a call (gridDim.x)
CROSS_MAX_G = 4096                 # selected genes of a call
CROSS_MAX_T = 65535                # time points of the images (gridDim.y)
CROSS_TILE = 64                    # rows and columns of M per workgroup
CROSS_LIMITS = ("1 <= G <= 4096 selected genes, 1 <= n <= 2147483647 spots and at most 2147483647 edges per time point, at most "
                "2147483647 stored entries, every entry of col in 0 .. n-1, every row index inside the time points, every selected "
                "gene inside the genes, permutation indices below 2^32, at most 65535 time points and 2147483647 workgroups per "
                "call")


def cross_padded(ng):
    """The columns of the images of a call over ng selected genes."""
    return (int(ng) + 15) // 16 * 16


def cross_layout(sizes):
    """(zoff int64 [T], zrows): the first row of every time point in the images, n rounded up to a multiple of 4 each."""
    pad = (np.asarray(sizes, dtype=np.int64) + 3) // 4 * 4
    zoff = np.concatenate([[0], np.cumsum(pad)]).astype(np.int64)
    return zoff[:-1], int(zoff[-1])


def _cross_desc(desc, ng, name):
    """The limits that the descriptor and the number of selected genes decide.  Returns (desc, zrows needed)."""
    desc = _host_desc(desc, CROSS_DESC, "time point")
    ng = int(ng)
    if not 1 <= ng <= CROSS_MAX_G:
        raise ValueError(f"{name} takes 1 to {CROSS_MAX_G} selected genes (got {ng})")
    need = 0
    for t, (eoff, n, E, row0, gid, roff, _lo, _hi, zoff) in enumerate(desc.tolist()):
        _refuse_time_point(t, name, desc[t].tolist(), n, E, CROSS_MAX,
                           eoff >= 0 and roff >= 0 and zoff >= 0 and 0 <= row0 <= CROSS_MAX and 0 <= gid <= CROSS_MAX)
        need = max(need, zoff + (n + 3) // 4 * 4)
    return desc, need


def _cross_image(t, what, zrows, GP):
    if t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != (zrows, GP):
        raise ValueError(f"{what} must be a contiguous float64 tensor [{zrows}, {GP}] (got {tuple(t.shape)} {t.dtype})")


def cross_dense_check(rowptr, col, colptr, ridx, values, centre, genes, desc, Z=None):
    """The refusals of cross_dense, before any launch: the limits from the descriptor, then per time point the range of col and
    the order of rowptr and, with a CSC, the range of the row indices and of the selected genes and the order of colptr by
    reductions on the device (one host round trip).  colptr None: the dense columns, Z [zrows, GP] is the caller's and genes the
    number of its columns.  Returns (the descriptor with columns 6 and 7 filled in, the smallest row index, the largest, the
    smallest selected gene, the largest, ng); ValueError otherwise."""
    csc = colptr is not None
    need_cuda(rowptr, col, Z, *((colptr, ridx, values, centre, genes) if csc else ()))
    ng = int(genes.numel()) if csc else int(genes)
    desc, need = _cross_desc(desc, ng, "spadot_cross_dense")
    T = int(desc.shape[0])
    if T > CROSS_MAX_T:
        raise ValueError(f"the call holds {T} time points: spadot_cross_dense takes at most {CROSS_MAX_T} (the grid of one launch)")
    _typed((rowptr, torch.int32, "rowptr"), (col, torch.int32, "col"))
    G = nnz = 0
    if csc:
        _typed((ridx, torch.int32, "ridx"), (colptr, torch.int64, "colptr"), (values, torch.float32, "values"),
               (centre, torch.float64, "centre"), (genes, torch.int32, "genes"), any_dim=("centre",))
        G, nnz = _csc_sizes(colptr, ridx, values, CROSS_MAX)
        if tuple(centre.shape) != (T, G):
            raise ValueError(f"centre must be [T, G] = [{T}, {G}] (got {tuple(centre.shape)})")
    elif Z is None:
        raise ValueError("without a CSC, cross_dense takes the image Z of the dense columns")
    if Z is not None:
        _cross_image(Z, "Z", int(Z.shape[0]) if Z.dim() == 2 else -1, cross_padded(ng))
        if Z.shape[0] < need:
            raise ValueError(f"Z holds {int(Z.shape[0])} rows: the time points need {need}")
    rows = 0
    for t, (eoff, n, E, row0, _gid, roff, _lo, _hi, _zoff) in enumerate(desc.tolist()):
        if eoff + E > col.numel() or roff + n + 1 > rowptr.numel():
            raise ValueError(f"time point {t}: its rows or edges reach past the end of the tensors")
        rows = max(rows, row0 + n)
    if -(-need * cross_padded(ng) // 256) > CROSS_MAX:
        raise ValueError(f"the images hold more than {CROSS_MAX} workgroups of 256 cells (the grid of one launch)")
    zero = torch.zeros((), dtype=torch.int64, device=rowptr.device)
    stats = _csr_stats(rowptr, col, desc, zero)
    if csc:
        stats += _csc_stats(colptr, ridx, zero) + [s.long() for s in torch.aminmax(genes)]
    stats = torch.stack(stats).cpu().numpy()                                # the one host round trip ahead of the launch
    _refuse_csr(desc, stats[:5 * T].reshape(T, 5))
    ridx_lo = ridx_hi = gene_lo = gene_hi = 0
    if csc:
        ridx_lo, ridx_hi, c0, c1, unordered, gene_lo, gene_hi = (int(v) for v in stats[5 * T:])
        _refuse_rows(ridx_lo, ridx_hi, nnz, rows)
        if gene_lo < 0 or gene_hi >= G:
            raise ValueError(f"the selected genes {gene_lo} .. {gene_hi} must lie in 0 .. {G - 1}")
        _refuse_colptr(c0, c1, unordered, nnz)
    return desc, ridx_lo, ridx_hi, gene_lo, gene_hi, ng


def cross_dense_launch(rowptr, col, colptr, ridx, values, centre, genes, checked, Z=None, out=None, desc_dev=None):
    """The launch of cross_dense for what cross_dense_check has returned (the library checks the descriptor again, on the
    host).  Returns (Z, Y)."""
    desc, ridx_lo, ridx_hi, gene_lo, gene_hi, ng = checked
    csc = colptr is not None
    need_cuda(rowptr, col, Z, desc_dev, *((colptr, ridx, values, centre, genes) if csc else ()), *(out or ()))
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    T, GP = int(desc.shape[0]), cross_padded(ng)
    need = int((desc[:, 8] + (desc[:, 1] + 3) // 4 * 4).max())
    dev = rowptr.device
    if out is not None:
        if len(out) != 2 or (not csc and out[0] is not Z):
            raise ValueError("out is the pair (Z, Y); with dense columns its Z is the image that was given")
        Z, Y = out
    else:
        Z = torch.empty((need, GP), dtype=torch.float64, device=dev) if csc else Z
        Y = torch.empty((int(Z.shape[0]), GP), dtype=torch.float64, device=dev)
    zrows = int(Z.shape[0]) if Z.dim() == 2 else -1
    _cross_image(Z, "Z", zrows, GP)
    _cross_image(Y, "Y", zrows, GP)
    if zrows < need:
        raise ValueError(f"the images hold {zrows} rows: the time points need {need}")
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=dev)
    G = int(colptr.numel()) - 1 if csc else 0
    rc = model_lib().spadot_cross_dense(_p(rowptr), _p(col), _p(colptr) if csc else None, _p(ridx) if csc else None,
                                        _p(values) if csc else None, int(ridx.numel()) if csc else 0, ridx_lo, ridx_hi,
                                        _p(centre) if csc else None, _host(desc), _p(desc_dev), T, G, _p(genes) if csc else None,
                                        ng, gene_lo, gene_hi, GP, zrows, _p(Z), _p(Y), _stream())
    launched(rc, "spadot_cross_dense", CROSS_LIMITS)
    return Z, Y


def cross_dense(rowptr, col, colptr, ridx, values, centre, genes, desc, Z=None, out=None):
    """The centred dense image Z of the selected genes and its neighbour sums Y (include/spadot_model.h: spadot_cross_dense), fp64
    device tensors [zrows, GP].  rowptr, col int32: the CSR of the time points back to back; colptr int64, ridx int32 and values
    fp32: the CSC arrays of a DeviceCounts; centre fp64 [T, G]; genes int32: the selected genes (any order, repeats allowed);
    desc: int64 [T, 9] on the host as the header lays it out (columns 6 and 7, the range of col, are filled in here; column 8
    from cross_layout).  Dense columns: colptr, ridx, values, centre None, genes the number of columns and Z their image.
    ValueError, before any launch, outside the limits; RuntimeError for a CPU tensor."""
    checked = cross_dense_check(rowptr, col, colptr, ridx, values, centre, genes, desc, Z)
    return cross_dense_launch(rowptr, col, colptr, ridx, values, centre, genes, checked, Z, out)


def cross_check(Z, Y, desc, ng, observed, first, P):
    """The refusals of cross_sums, before any launch: all of them follow from the descriptor and the shapes.  Returns the
    descriptor; ValueError otherwise."""
    need_cuda(Z, Y)
    desc, need = _cross_desc(desc, ng, "spadot_cross_sums")
    observed, first, P = labelings("cross_sums", observed, first, P)
    zrows = int(Z.shape[0]) if Z.dim() == 2 else -1
    _cross_image(Z, "Z", zrows, cross_padded(ng))
    _cross_image(Y, "Y", zrows, cross_padded(ng))
    if zrows < need:
        raise ValueError(f"the images hold {zrows} rows: the time points need {need}")
    if int(desc.shape[0]) * (observed + P) * (-(-int(ng) // CROSS_TILE)) ** 2 > CROSS_MAX:
        raise ValueError(f"the call holds more than {CROSS_MAX} workgroups (the grid of one launch)")
    return desc


def cross_launch(Z, Y, checked, ng, observed, first, P, seed=0, out=None, desc_dev=None):
    """The launch of cross_sums for what cross_check has returned (the library checks the descriptor again, on the host)."""
    need_cuda(Z, Y, out, desc_dev)
    desc = np.ascontiguousarray(checked, dtype=np.int64)
    T, ng, L = int(desc.shape[0]), int(ng), int(bool(observed)) + int(P)
    if out is None:
        out = torch.empty((T, L, ng, ng), dtype=torch.float64, device=Z.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != T * L * ng * ng:
        raise ValueError(f"out must be a contiguous float64 tensor of {T} x {L} x {ng} x {ng} values")
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=Z.device)
    rc = model_lib().spadot_cross_sums(_p(Z), _p(Y), int(Z.shape[0]), cross_padded(ng), _host(desc), _p(desc_dev), T, ng,
                                       int(bool(observed)), int(first), int(P), _signed64(seed), _p(out), _stream())
    launched(rc, "spadot_cross_sums", CROSS_LIMITS)
    return out


def cross_sums(Z, Y, desc, ng, observed, first, P, seed=0, out=None):
    """The cross sums M[t, l, g, h] = sum_i Z[pi_l(i), g] Y[i, h] of every pair of the ng selected genes of every (time point,
    labeling) in ONE launch on the fp64 matrix cores (include/spadot_model.h: spadot_cross_sums).  Z, Y: the images of
    cross_dense; desc: the same descriptor.  Labelings: the identity (observed) and the permutations first .. first + P - 1 under
    seed.  Returns M, an fp64 device tensor [T, observed + P, ng, ng] (out: the tensor to write into).  ValueError, before any
    launch, outside the limits; RuntimeError for a CPU tensor."""
    return cross_launch(Z, Y, cross_check(Z, Y, desc, ng, observed, first, P), ng, observed, first, P, seed, out)


CORR_DESC = 6
CORR_MAX_B = 16                    # bands of a time point: the thresholds are padded to this with +inf
CORR_MAX_G = CROSS_MAX_G           # selected genes of a call, as the images of cross_dense
CORR_MAX_N = COOCCUR_MAX_N
CORR_MAX_T = 65535                 # time points of a call (gridDim.z)
CORR_MAX_Y = 65535                 # labelings x chunks of genes of a call (gridDim.y)
CORR_MAX_GID = COOCCUR_MAX_G
CORR_CS = 2                        # the library's default
CORR_LIMITS = ("1 <= B <= 16 thresholds that are finite, >= 0 and strictly increasing, 1 <= G <= 4096 selected genes, 1 <= n <= "
               "2147483391 spots per time point, at most 65535 time points and (observed + P) ceil(G / cs) <= 65535 labelings x "
               "chunks of genes per call, permutation indices below 2^32, graph ids in 0 .. 2147483647, cs in (2, 4)")


def corr_layout(sizes):
    """(boff int64 [T], blocks): the blocks of 256 spots ahead of every time point, and of the call."""
    b = np.concatenate([[0], np.cumsum((np.asarray(sizes, dtype=np.int64) + 255) // 256)]).astype(np.int64)
    return b[:-1], int(b[-1])


def corr_scratch_doubles(blocks, ng, L, B_max):
    """The doubles of the scratch buffer of a call, as the library computes it: the boxes, then the partials."""
    return int(blocks) * 4 + 2 * int(blocks) * int(L) * int(ng) * int(B_max)


def corr_check(xy, order, Z, desc, r2, ng, observed, first, P, cs=None):
    """The refusals of corr_sums, before any launch: the limits from the descriptor, the thresholds and the shapes, then, by
    reductions on the device (one host round trip), that `order` holds a permutation of 0 .. n-1 per time point and that the
    coordinates are finite.  r2: [T] sequences of squared thresholds, or the array [T, 16] padded with +inf.  Returns (desc
    int64 [T, 6], r2 fp64 [T, 16] padded with +inf, B_max, observed as 0 / 1, first, P); ValueError otherwise."""
    need_cuda(xy, order, Z)
    desc = _host_desc(desc, CORR_DESC, "time point")
    T, ng, cs = int(desc.shape[0]), int(ng), int(cs or 0)
    if not 1 <= ng <= CORR_MAX_G:
        raise ValueError(f"spadot_corr_sums takes 1 to {CORR_MAX_G} selected genes (got {ng})")
    if cs not in (0, 2, 4):
        raise ValueError(f"spadot_corr_sums takes cs in (2, 4) (got {cs})")
    if T > CORR_MAX_T:
        raise ValueError(f"the call holds {T} time points: spadot_corr_sums takes at most {CORR_MAX_T} (the grid of one launch)")
    if len(r2) != T:
        raise ValueError(f"the call holds {T} time points and {len(r2)} sets of thresholds")
    observed, first, P = labelings("corr_sums", observed, first, P)
    if (observed + P) * -(-ng // (cs or CORR_CS)) > CORR_MAX_Y:
        raise ValueError(f"the call holds {observed + P} labelings x {-(-ng // (cs or CORR_CS))} chunks of genes: spadot_corr_sums "
                         f"takes at most {CORR_MAX_Y} (the grid of one launch; split the labelings or the genes)")
    pad = np.full((T, CORR_MAX_B), np.inf, dtype=np.float64)
    off = blocks = need = B_max = 0
    for t, (o, n, B, gid, zoff, boff) in enumerate(desc.tolist()):
        if not 1 <= B <= CORR_MAX_B:
            raise ValueError(f"time point {t} has {B} thresholds: spadot_corr_sums takes 1 to {CORR_MAX_B}")
        if not 1 <= n <= CORR_MAX_N:
            raise ValueError(f"time point {t} has {n} spots: spadot_corr_sums takes 1 to {CORR_MAX_N} (int32 positions)")
        if not 0 <= gid <= CORR_MAX_GID:
            raise ValueError(f"time point {t} has the graph id {gid}: spadot_corr_sums takes 0 to {CORR_MAX_GID}")
        if o != off or boff != blocks or zoff < 0:
            raise ValueError(f"time point {t}: inconsistent descriptor {desc[t].tolist()}")
        th = np.asarray(r2[t], dtype=np.float64).reshape(-1)
        if th.shape[0] == CORR_MAX_B and np.all(th[B:] == np.inf):
            th = th[:B]
        if th.shape[0] != B:
            raise ValueError(f"time point {t} has {th.shape[0]} thresholds and its descriptor says {B}")
        if not np.all(np.isfinite(th)) or np.any(th < 0) or np.any(np.diff(th) <= 0):
            raise ValueError(f"the squared thresholds of time point {t} must be finite, >= 0 and strictly increasing")
        pad[t, :B] = th
        off, blocks, need, B_max = off + n, blocks + (n + 255) // 256, max(need, zoff + (n + 3) // 4 * 4), max(B_max, B)
    if xy.dtype != torch.float64 or xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_contiguous() or xy.shape[0] != off:
        raise ValueError(f"xy must be a contiguous fp64 [{off}, 2] tensor (got {tuple(xy.shape)} {xy.dtype})")
    if order.dtype != torch.int32 or order.dim() != 1 or not order.is_contiguous() or order.shape[0] != off:
        raise ValueError(f"order must be a contiguous int32 tensor of {off} positions (got {tuple(order.shape)} {order.dtype})")
    _cross_image(Z, "Z", int(Z.shape[0]) if Z.dim() == 2 else -1, cross_padded(ng))
    if Z.shape[0] < need:
        raise ValueError(f"Z holds {int(Z.shape[0])} rows: the time points need {need}")
    stats = []
    for o, n, *_rest in desc.tolist():
        seen = torch.sort(order[o:o + n].long()).values
        stats += [(seen != torch.arange(n, dtype=torch.int64, device=order.device)).any().long(),
                  torch.isfinite(xy[o:o + n]).all().long()]
    stats = torch.stack(stats).cpu().numpy().reshape(T, 2)                  # the one host round trip ahead of the launch
    for t in range(T):
        if stats[t, 0]:
            raise ValueError(f"the order of time point {t} is not a permutation of 0 .. {int(desc[t, 1]) - 1}")
        if not stats[t, 1]:
            raise ValueError(f"time point {t} holds coordinates that are not finite")
    return desc, pad, B_max, observed, first, P


def corr_launch(xy, order, Z, checked, ng, seed=0, cull=True, cs=None, out=None, scratch=None, skipped=None, desc_dev=None,
                r2_dev=None):
    """The launch of corr_sums for what corr_check has returned (the library checks the descriptor and the thresholds again, on
    the host).  Returns (W, S2c, N, Q)."""
    desc, r2, B_max, observed, first, P = checked
    need_cuda(xy, order, Z, scratch, skipped, desc_dev, r2_dev, *(out or ()))
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    r2 = np.ascontiguousarray(r2, dtype=np.float64)
    T, ng, L, cs, dev = int(desc.shape[0]), int(ng), int(observed) + int(P), int(cs or 0), xy.device
    if cs not in (0, 2, 4):                                               # the library's refusal, ahead of the call
        launched(-7, "spadot_corr_sums", CORR_LIMITS)
    if out is None:
        out = (torch.empty((T, B_max), dtype=torch.int64, device=dev), torch.empty((T, B_max), dtype=torch.int64, device=dev),
               torch.empty((T, ng, L, B_max), dtype=torch.float64, device=dev),
               torch.empty((T, ng, L, B_max), dtype=torch.float64, device=dev))
    elif (len(out) != 4 or any(not o.is_contiguous() for o in out)
          or any(o.dtype != torch.int64 or o.numel() != T * B_max for o in out[:2])
          or any(o.dtype != torch.float64 or o.numel() != T * ng * L * B_max for o in out[2:])):
        raise ValueError(f"out must be two contiguous int64 tensors of {T} x {B_max} values and two contiguous float64 tensors of "
                         f"{T} x {ng} x {L} x {B_max}")
    need = corr_scratch_doubles(int(((desc[:, 1] + 255) // 256).sum()), ng, L, B_max)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float64, device=dev)
    elif scratch.dtype != torch.float64 or not scratch.is_contiguous() or scratch.numel() < need:
        raise ValueError(f"scratch must be a contiguous float64 tensor of at least {need} values")
    if skipped is not None and (skipped.dtype != torch.int64 or skipped.numel() != 1):
        raise ValueError("skipped must be an int64 tensor of one value")
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=dev)
    if r2_dev is None:
        r2_dev = torch.as_tensor(r2, device=dev)
    rc = model_lib().spadot_corr_sums(_p(xy), _p(order), _p(Z), int(Z.shape[0]), cross_padded(ng), _host(desc), _p(desc_dev),
                                      _host(r2), _p(r2_dev), T, ng, B_max, int(observed), int(first), int(P), _signed64(seed),
                                      int(bool(cull)), cs, _p(scratch), int(scratch.numel()), _p(out[0]), _p(out[1]), _p(out[2]),
                                      _p(out[3]), _p(skipped), _stream())
    launched(rc, "spadot_corr_sums", CORR_LIMITS)
    return out


def corr_sums(xy, order, Z, desc, r2, ng, observed, first, P, seed=0, cull=True, cs=None, out=None, scratch=None, skipped=None):
    """The band sums behind the spatial correlogram of every (time point, selected gene, labeling) (include/spadot_model.h:
    spadot_corr_sums).  xy: fp64 [sum n, 2] device tensor, per time point its spots in Morton order, the time points back to back;
    order int32 [sum n]: the original index of every position; Z: the image of cross_dense; desc: int64 [T, 6] on the host as
    the header lays it out; r2[t]: the squared thresholds of time point t.  Labelings: the identity (observed) and the
    permutations first .. first + P - 1 under seed.  cull: skip the tiles out of reach (the same bits either way); skipped: an
    int64 device tensor of one value that receives the number of skipped tiles.  Returns (W int64 [T, B_max], S2c int64
    [T, B_max], N fp64 [T, ng, observed + P, B_max], Q the same) (out: the four to write into).  ValueError, before any launch,
    outside the limits; RuntimeError for a CPU tensor."""
    checked = corr_check(xy, order, Z, desc, r2, ng, observed, first, P, cs)
    return corr_launch(xy, order, Z, checked, ng, seed, cull, cs, out, scratch, skipped)


RIPLEY_MAX_K = COOCCUR_MAX_K
RIPLEY_MAX_B = COOCCUR_MAX_B
RIPLEY_MAX_S = 9999                # simulations of a problem
RIPLEY_MAX_M = 1048576             # probe points of a problem
RIPLEY_MAX_V = 256                 # vertices of a window (LDS)
RIPLEY_MAX_N = COOCCUR_MAX_N
RIPLEY_MAX_P = COOCCUR_MAX_P       # problems of a call (gridDim.z)
RIPLEY_MAX_Y = COOCCUR_MAX_Y       # patterns of a problem, K (1 + S) (gridDim.y)
RIPLEY_MAX_G = COOCCUR_MAX_G       # problem numbers, as the graph ids of spadot_nhood_counts
RIPLEY_MAX_STREAM = 1 + RIPLEY_MAX_K * RIPLEY_MAX_S
RIPLEY_DESC = 48
RIPLEY_MODES = {"L": 1, "G": 2, "F": 4}
RIPLEY_LIMITS = ("1 <= K <= 32 label values, 1 <= B <= 64 thresholds that are finite, >= 0 and strictly increasing, 1 <= S <= 9999 "
                 "simulations, 1 <= M <= 1048576 probe points, a window of at most 256 vertices, 1 <= n <= 2147483391 spots per "
                 "problem, at most 65535 problems per call and K (1 + S) <= 65535 patterns per problem")


def ripley_window(vertices, cum, what="the window"):
    """(vertices fp64 [V, 2], cum fp64 [V - 2]) as the library accepts them: 3 to 256 finite vertices that never turn right and go
    round once, ascending areas >= 0.  ValueError otherwise."""
    v = np.ascontiguousarray(vertices, dtype=np.float64)
    c = np.ascontiguousarray(cum, dtype=np.float64).reshape(-1)
    if v.ndim != 2 or v.shape[1] != 2 or v.shape[0] < 3 or c.shape[0] != v.shape[0] - 2:
        raise ValueError(f"{what} must hold V >= 3 vertices [V, 2] and V - 2 cumulative areas (got {v.shape} and {c.shape})")
    if v.shape[0] > RIPLEY_MAX_V:
        raise ValueError(f"{what} has {v.shape[0]} vertices: the device takes at most {RIPLEY_MAX_V} (window=\"box\" has four)")
    if not np.all(np.isfinite(v)) or not np.all(np.isfinite(c)):
        raise ValueError(f"{what} holds vertices or areas that are not finite")
    e = np.roll(v, -1, axis=0) - v
    f = np.roll(e, -1, axis=0)
    if np.any(e[:, 0] * f[:, 1] < e[:, 1] * f[:, 0]):
        raise ValueError(f"{what} must be convex with its vertices counter-clockwise (it turns right somewhere)")
    for s in (np.sign(e[:, 0]), np.sign(e[:, 1])):
        s = s[s != 0]
        if s.size and np.count_nonzero(s != np.roll(s, 1)) > 2:
            raise ValueError(f"{what} must be convex with its vertices counter-clockwise (it goes round more than once)")
    if np.any(c < 0) or np.any(np.diff(c) < 0):
        raise ValueError(f"the cumulative areas of {what} must be >= 0 and ascend")
    return v, c


def ripley_check(xy, desc, r2, windows, K_max, S_max, B_max):
    """The refusals of ripley_counts that the descriptor, the thresholds and the windows decide, before any launch.  windows[p]:
    (vertices [V, 2], cum [V - 2]) of problem p on the host.  Returns (desc int64 [P, 48] with columns 9 and 10 filled in, r2 fp64
    [P, BP] padded with -1.0, hull fp64 [rows, 2], cum fp64 [rows]); ValueError otherwise."""
    need_cuda(xy)
    desc = _host_desc(desc, RIPLEY_DESC, "problem")
    K_max, S_max, B_max, P = int(K_max), int(S_max), int(B_max), desc.shape[0]
    if not 1 <= K_max <= RIPLEY_MAX_K:
        raise ValueError(f"spadot_ripley_counts takes 1 to {RIPLEY_MAX_K} label values (got K_max = {K_max})")
    if not 1 <= B_max <= RIPLEY_MAX_B:
        raise ValueError(f"spadot_ripley_counts takes 1 to {RIPLEY_MAX_B} thresholds (got B_max = {B_max})")
    if not 1 <= S_max <= RIPLEY_MAX_S:
        raise ValueError(f"spadot_ripley_counts takes 1 to {RIPLEY_MAX_S} simulations (got S_max = {S_max})")
    if P > RIPLEY_MAX_P:
        raise ValueError(f"the call holds {P} problems: spadot_ripley_counts takes at most {RIPLEY_MAX_P} (the grid of one launch)")
    if len(r2) != P or len(windows) != P:
        raise ValueError(f"the call holds {P} problems, {len(r2)} sets of thresholds and {len(windows)} windows")
    pad = np.full((P, cooccur_padded(B_max)), -1.0, dtype=np.float64)
    first, rows, hulls, cums = 0, 0, [], []
    for p, row in enumerate(desc.tolist()):
        off, n, K, B, S, M, null, modes, g = row[:9]
        if not 1 <= K <= K_max:
            raise ValueError(f"problem {p} has {K} label values: spadot_ripley_counts takes 1 to {K_max} here, at most {RIPLEY_MAX_K}")
        if not 1 <= B <= B_max:
            raise ValueError(f"problem {p} has {B} thresholds: spadot_ripley_counts takes 1 to {B_max} here, at most {RIPLEY_MAX_B}")
        if not 1 <= S <= S_max:
            raise ValueError(f"problem {p} has {S} simulations: spadot_ripley_counts takes 1 to {S_max} here, at most {RIPLEY_MAX_S}")
        if not 1 <= M <= RIPLEY_MAX_M:
            raise ValueError(f"problem {p} has {M} probe points: spadot_ripley_counts takes 1 to {RIPLEY_MAX_M}")
        if not 1 <= n <= RIPLEY_MAX_N:
            raise ValueError(f"problem {p} has {n} spots: spadot_ripley_counts takes 1 to {RIPLEY_MAX_N} (int32 positions)")
        if K * (1 + S) > RIPLEY_MAX_Y:
            raise ValueError(f"problem {p} has {K} x {1 + S} patterns: spadot_ripley_counts takes at most {RIPLEY_MAX_Y} per problem "
                             f"(the grid of one launch)")
        if (off != first or not _cluster_offsets_ok(row[12:13 + K], n) or null not in (0, 1) or not 1 <= modes <= 7
                or not 0 <= g <= RIPLEY_MAX_G):
            raise ValueError(f"problem {p}: inconsistent descriptor {row[:13 + K]}")
        first += n
        _padded_thresholds(pad, p, r2[p], B)
        v, c = ripley_window(*windows[p], what=f"the window of problem {p}")
        desc[p, 9], desc[p, 10], desc[p, 11] = rows, v.shape[0], 0
        hulls.append(v)
        cums.append(np.concatenate([c, [0.0, 0.0]]))
        rows += v.shape[0]
    if xy.dtype != torch.float64 or xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_contiguous() or xy.shape[0] != first:
        raise ValueError(f"xy must be a contiguous fp64 [{first}, 2] tensor (got {tuple(xy.shape)} {xy.dtype})")
    return desc, pad, np.ascontiguousarray(np.concatenate(hulls)), np.ascontiguousarray(np.concatenate(cums))


def ripley_launch(xy, checked, K_max, S_max, B_max, seed=0, out=None):
    """The launch of ripley_counts for what ripley_check has returned (the library checks all of it again, on the host)."""
    desc, r2, hull, cum = checked
    need_cuda(xy, out)
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    r2, hull, cum = (np.ascontiguousarray(a, dtype=np.float64) for a in (r2, hull, cum))
    K_max, S_max, B_max, P = int(K_max), int(S_max), int(B_max), int(desc.shape[0])
    out = _out_int64(out, (P, K_max, 1 + S_max, 3, B_max), xy.device)
    dev = [torch.as_tensor(a, device=xy.device) for a in (desc, r2, hull, cum)]
    launched(model_lib().spadot_ripley_counts(_p(xy), _host(desc), _p(dev[0]), _host(r2), _p(dev[1]), _host(hull), _p(dev[2]),
                                              _host(cum), _p(dev[3]), int(hull.shape[0]), P, K_max, S_max, B_max, _signed64(seed),
                                              _p(out), _stream()), "spadot_ripley_counts", RIPLEY_LIMITS)
    return out


def ripley_counts(xy, desc, r2, windows, K_max, S_max, B_max, seed=0, out=None):
    """The integers behind Ripley's L, G and F of every (problem, domain, pattern) in ONE counting launch (include/spadot_model.h:
    spadot_ripley_counts).  xy: fp64 [sum n, 2] device tensor, per problem its spots ordered by (label, index), the problems back
    to back; desc: int64 [P, 48] on the host as the header lays it out (columns 9 to 11, the place of the window, are filled in
    here); r2[p]: the squared thresholds of problem p; windows[p]: its (vertices, cum) on the host.  Returns int64
    [P, K_max, 1 + S_max, 3, B_max] (out: the tensor to write into).  ValueError, before any launch, outside the limits;
    RuntimeError for a CPU tensor."""
    return ripley_launch(xy, ripley_check(xy, desc, r2, windows, K_max, S_max, B_max), K_max, S_max, B_max, seed, out)


def ripley_points(vertices, cum, seed, g, stream, count, device=None, out=None):
    """The generated points 0 .. count - 1 of (seed, problem g, stream) in a window, by the device function that ripley_counts
    uses (include/spadot_model.h: spadot_ripley_points).  vertices, cum: on the host.  Returns an fp64 device tensor [count, 2]
    (out: the tensor to write into).  ValueError, before any launch, outside the limits; RuntimeError for a CPU tensor."""
    need_cuda(out)
    v, c = ripley_window(vertices, cum)
    count, g, stream = int(count), int(g), int(stream)
    if not 1 <= count <= RIPLEY_MAX_N:
        raise ValueError(f"spadot_ripley_points writes 1 to {RIPLEY_MAX_N} points (got {count})")
    if not 0 <= stream <= RIPLEY_MAX_STREAM or not 0 <= g <= RIPLEY_MAX_G:
        raise ValueError(f"spadot_ripley_points takes a stream in 0 .. {RIPLEY_MAX_STREAM} and a problem number in 0 .. "
                         f"{RIPLEY_MAX_G} (got stream {stream}, problem {g})")
    if out is None:
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            need_cuda(torch.empty(0))
        out = torch.empty((count, 2), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != 2 * count:
        raise ValueError(f"out must be a contiguous float64 tensor of {count} x 2 values")
    with torch.cuda.device(out.device):
        vd, cd = torch.as_tensor(v, device=out.device), torch.as_tensor(c, device=out.device)
        launched(model_lib().spadot_ripley_points(_host(v), _p(vd), _host(c), _p(cd), int(v.shape[0]), _signed64(seed), g, stream,
                                                  count, _p(out), _stream()), "spadot_ripley_points", RIPLEY_LIMITS)
    return out


EMBED_DESC = 10
EMBED_MAX_D = 32
EMBED_MAX_K = 150                  # floor(3 * 50)
EMBED_MAX_P = 65535                # problems of a call (gridDim.y / gridDim.z)
EMBED_MAX_S = 65535                # slices of a problem (gridDim.y)
EMBED_MAX_N = 2147483135           # points of a problem: int32 positions of a 512-wide block
EMBED_TILE = 256
EMBED_WORKGROUPS = 1024            # the slice rule aims at this many repulsion workgroups: four per CU of an MI355X
EMBED_SCRATCH_BYTES = 1 << 30
EMBED_LIMITS = ("1 <= d <= 32, at most 65535 problems, 2 <= perplexity <= 50, perplexity + 2 <= n <= 2147483135 points per problem, "
                "k = min(n - 1, floor(3 perplexity)) neighbours, 1 <= slices <= 65535, exaggeration >= 1")


def embed_neighbors(n, perplexity):
    """k = min(n - 1, floor(3 perplexity)): the neighbours behind the affinities of a problem of n points."""
    return min(int(n) - 1, int(np.floor(3.0 * float(perplexity))))


def embed_slices(n):
    """The slices of the partner range of a problem of n points: a function of n alone, so that the bits of a problem do not depend
    on what else a launch holds.  ceil(1024 / tiles) slices of whole tiles, at most one per tile: 6 at 50 000 points (1176
    workgroups on the 256 CUs of an MI355X), 26 at 10 000."""
    tiles = -(-int(n) // EMBED_TILE)
    return max(1, min(tiles, -(-EMBED_WORKGROUPS // tiles)))


def embed_table(sizes, perplexity, slices=None, nnz=None):
    """The problem table of the embed entries, int64 [P, 10] on the host as the header lays it out, and the perplexities fp64 [P].
    perplexity: one number or one per problem; slices: None (embed_slices), one number or one per problem; nnz: the stored
    entries of every problem's CSR (None before it exists).  ValueError outside the limits."""
    sizes = [int(n) for n in sizes]
    P = len(sizes)
    if not 1 <= P <= EMBED_MAX_P:
        raise ValueError(f"one call embeds 1 to {EMBED_MAX_P} problems (got {P})")
    perp = np.broadcast_to(np.asarray(perplexity, dtype=np.float64), (P,)).copy()
    per = [None] * P if slices is None else np.broadcast_to(np.asarray(slices, dtype=np.int64), (P,)).tolist()
    nnz = [0] * P if nnz is None else [int(v) for v in nnz]
    desc = np.zeros((P, EMBED_DESC), dtype=np.int64)
    off = koff = soff = eoff = boff = 0
    for p, (n, u) in enumerate(zip(sizes, perp.tolist())):
        if not 2.0 <= u <= 50.0:
            raise ValueError(f"problem {p} has the perplexity {u}: the device t-SNE takes 2 to 50")
        if not u + 2.0 <= n <= EMBED_MAX_N:
            raise ValueError(f"problem {p} has {n} points: a perplexity of {u} needs at least {int(np.ceil(u + 2.0))}, and the "
                             f"device t-SNE takes at most {EMBED_MAX_N}")
        tiles = -(-n // EMBED_TILE)
        S = embed_slices(n) if per[p] is None else int(per[p])
        if not 1 <= S <= EMBED_MAX_S:                   # more slices than tiles: the surplus ones hold no tile and add exact zeros
            raise ValueError(f"problem {p} takes 1 to {EMBED_MAX_S} slices of the partner range (got {S})")
        k = embed_neighbors(n, u)
        desc[p] = (off, n, k, koff, S, soff, off + p, eoff, boff, nnz[p])
        off, koff, soff, eoff, boff = off + n, koff + n * k, soff + n * S, eoff + nnz[p], boff + tiles
    if 24 * soff > EMBED_SCRATCH_BYTES:
        raise ValueError(f"the partial sums of the slices would take {24 * soff} bytes of scratch: more than 1 GiB "
                         f"({EMBED_SCRATCH_BYTES}); give fewer slices or fewer problems per call")
    return desc, perp


def embed_check(X, desc):
    """The refusals that the points decide, before any launch: X a contiguous fp64 [sum n, d] device tensor with 1 <= d <= 32 and
    finite values (one reduction on the device, one host round trip)."""
    need_cuda(X)
    total = int(desc[-1, 0] + desc[-1, 1])
    if X.dtype != torch.float64 or X.dim() != 2 or not X.is_contiguous() or X.shape[0] != total:
        raise ValueError(f"X must be a contiguous fp64 [{total}, d] tensor (got {tuple(X.shape)} {X.dtype})")
    d = int(X.shape[1])
    if not 1 <= d <= EMBED_MAX_D:
        raise ValueError(f"the device t-SNE supports data of 1 to {EMBED_MAX_D} dimensions (got {d})")
    if not bool(torch.isfinite(X).all().cpu()):                              # the one host round trip ahead of the launch
        raise ValueError("the points hold values that are not finite")
    return d


def latent_knn_launch(X, desc, desc_dev=None, out=None):
    """The k nearest other points of every point of P problems in ONE launch (include/spadot_model.h: spadot_latent_knn), for what
    embed_table and embed_check have passed.  Returns (idx int32, d2 fp64), both [sum n k]: row i of problem p at desc[p, 3] + i k."""
    need_cuda(X, desc_dev, *(out or ()))
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    P, total = int(desc.shape[0]), int(desc[-1, 3] + desc[-1, 1] * desc[-1, 2])
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=X.device)
    idx, d2 = out if out is not None else (torch.empty(total, dtype=torch.int32, device=X.device),
                                           torch.empty(total, dtype=torch.float64, device=X.device))
    _typed((idx, torch.int32, "idx"), (d2, torch.float64, "d2"))
    if idx.numel() != total or d2.numel() != total:
        raise ValueError(f"idx and d2 must hold {total} values")
    launched(model_lib().spadot_latent_knn(_p(X), int(X.shape[1]), P, _host(desc), _p(desc_dev), _p(idx), _p(d2), _stream()),
             "spadot_latent_knn", EMBED_LIMITS, f": d = {int(X.shape[1])}, {P} problems")
    return idx, d2


def tsne_affinities_launch(d2, desc, perp, desc_dev=None):
    """The conditional affinities of every row of P problems in ONE launch (spadot_tsne_affinities).  d2: what latent_knn_launch
    returned; perp: fp64 [P] on the host.  Returns (cond fp64 [sum n k], beta fp64 [sum n])."""
    need_cuda(d2, desc_dev)
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    perp = np.ascontiguousarray(perp, dtype=np.float64)
    P, rows = int(desc.shape[0]), int(desc[-1, 0] + desc[-1, 1])
    _typed((d2, torch.float64, "d2"))
    if d2.numel() != int(desc[-1, 3] + desc[-1, 1] * desc[-1, 2]) or perp.shape != (P,):
        raise ValueError(f"d2 must hold the neighbour lists of the {P} problems and perp one perplexity per problem")
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=d2.device)
    perp_dev = torch.as_tensor(perp, device=d2.device)
    cond, beta = torch.empty_like(d2), torch.empty(rows, dtype=torch.float64, device=d2.device)
    launched(model_lib().spadot_tsne_affinities(_p(d2), P, _host(desc), _p(desc_dev), _host(perp), _p(perp_dev), _p(cond), _p(beta),
                                                _stream()), "spadot_tsne_affinities", EMBED_LIMITS)
    return cond, beta


def tsne_csr_check(desc, rowptr, col, val):
    """The refusals of tsne_steps_launch that the joint affinities decide, before any launch: per problem a rowptr that ascends
    from 0 to its stored entries and columns in 0 .. n-1 (reductions on the device, one host round trip)."""
    need_cuda(rowptr, col, val)
    _typed((rowptr, torch.int64, "rowptr"), (col, torch.int32, "col"), (val, torch.float64, "val"))
    P, nnz = int(desc.shape[0]), int(desc[:, 9].sum())
    if rowptr.numel() != int(desc[-1, 6] + desc[-1, 1] + 1) or col.numel() != nnz or val.numel() != nnz:
        raise ValueError(f"rowptr must hold n + 1 entries per problem, col and val the {nnz} stored entries of the table")
    zero = torch.zeros((), dtype=torch.int64, device=col.device)
    stats = []
    for _off, n, _k, _koff, _S, _soff, roff, eoff, _boff, E in desc.tolist():
        rp = rowptr[roff:roff + n + 1]
        lo, hi = torch.aminmax(col[eoff:eoff + E]) if E > 0 else (zero, zero)
        stats += [lo.long(), hi.long(), rp[0], rp[-1], (rp[1:] < rp[:-1]).any().long()]
    stats = torch.stack(stats).cpu().numpy().reshape(P, 5)                   # the one host round trip ahead of the launch
    for p in range(P):
        n, E = int(desc[p, 1]), int(desc[p, 9])
        if E > 0 and (stats[p, 0] < 0 or stats[p, 1] >= n):
            raise ValueError(f"problem {p} has the columns {int(stats[p, 0])} .. {int(stats[p, 1])} in col: they must lie in 0 .. "
                             f"{n - 1}")
        if stats[p, 2] != 0 or stats[p, 3] != E or stats[p, 4]:
            raise ValueError(f"the rowptr of problem {p} must ascend from 0 to its {E} stored entries (it runs from "
                             f"{int(stats[p, 2])} to {int(stats[p, 3])})")


def tsne_state(desc, n_iter, device):
    """The buffers of tsne_steps_launch for a table: Y0, Y1, upd, gains, grad, att fp64 [sum n, 2] (gains ones, the rest zeros), zr
    [sum n, 3], part [sum n S, 3], blk [sum ceil(n / 256), 2], Z [P], kl [P, n_iter] (NaN), lr [P] (zeros: the caller's to set)."""
    N, P = int(desc[-1, 0] + desc[-1, 1]), int(desc.shape[0])
    rows = int(desc[-1, 5] + desc[-1, 1] * desc[-1, 4])
    blocks = int(desc[-1, 8]) + -(-int(desc[-1, 1]) // EMBED_TILE)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=device)  # noqa: E731
    return dict(Y0=z(N, 2), Y1=z(N, 2), upd=z(N, 2), gains=torch.ones((N, 2), dtype=torch.float64, device=device), grad=z(N, 2),
                att=z(N, 2), zr=z(N, 3), part=z(rows, 3), blk=z(blocks, 2), Z=z(P), lr=z(P),
                kl=torch.full((P, max(int(n_iter), 1)), float("nan"), dtype=torch.float64, device=device))


def tsne_steps_launch(desc, desc_dev, rowptr, col, val, state, it0, steps, early, exaggeration=12.0, two=False):
    """Queues the iterations it0 .. it0 + steps - 1 of P problems (spadot_tsne_steps) on the buffers of tsne_state, for a table
    and a CSR that embed_table and tsne_csr_check have passed.  Iteration `it` reads Y0 where it is even and Y1 where it is odd,
    and writes the other.  No host synchronisation."""
    need_cuda(desc_dev, rowptr, col, val, *state.values())
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    it0, steps, early = int(it0), int(steps), int(early)
    if steps < 0 or it0 < 0 or early < 0 or it0 + steps > int(state["kl"].shape[1]):
        raise ValueError(f"the iterations {it0} .. {it0 + steps - 1} do not fit the {int(state['kl'].shape[1])} of the run")
    s = state
    rc = model_lib().spadot_tsne_steps(_host(desc), _p(desc_dev), int(desc.shape[0]), _p(rowptr), _p(col), _p(val), _p(s["Y0"]),
                                       _p(s["Y1"]), _p(s["upd"]), _p(s["gains"]), _p(s["lr"]), _p(s["part"]), _p(s["zr"]),
                                       _p(s["att"]), _p(s["blk"]), _p(s["grad"]), _p(s["Z"]), _p(s["kl"]), int(s["kl"].shape[1]), it0,
                                       steps, early, float(exaggeration), int(bool(two)), _stream())
    launched(rc, "spadot_tsne_steps", EMBED_LIMITS)


SEPAL_DESC = LOCAL_DESC            # the descriptor of moran.edge_csr; column 2 holds the entries of the symmetric CSR
SEPAL_MAX = 2147483647             # spots, CSR entries and stored entries (int32), steps, and workgroups of a call (gridDim.x)
SEPAL_THREADS = 1024               # the workgroup: the summation order of the entropy depends on it and on n alone
SEPAL_SPT = 12                     # spots a thread holds in registers between the two barriers of a step
SEPAL_LDS_FIXED = 512              # LDS beside the image: the reduction slots, the broadcast words, the segment bounds
SEPAL_LDS_BYTES = SEPAL_LDS_FIXED + 8 * SEPAL_SPT * SEPAL_THREADS          # 98816: 12288 spots
SEPAL_STEPS = 2048                 # steps per launch of sepal_steps
SEPAL_LIMITS = ("1 <= steps and n_iter <= 2147483647, thresh >= 0 and finite, a rate > 0 and finite for every time point with edges, "
                "1 <= n <= 2147483647 spots and at most 2147483647 CSR entries per time point, at most 2147483647 stored entries, "
                "every entry of col in 0 .. n-1, every row index inside the time points, every selected gene inside the genes, at "
                "most 2147483647 workgroups per call")


def sepal_rate(dt, n, M):
    """a = dt n / M in fp64, M = 2 E the entries of the symmetric CSR: the product rounded, then the quotient (0.0 where M = 0)."""
    return float(dt) * int(n) / int(M) if int(M) > 0 else 0.0


def sepal_max_dt(n, M, deg):
    """The largest fp64 dt with sepal_rate(dt, n, M) * deg < 1 for a largest degree deg >= 1 (inf without edges)."""
    n, M, deg = int(n), int(M), int(deg)
    if M < 1 or deg < 1:
        return float("inf")
    y = M / (n * deg)
    while sepal_rate(y, n, M) * deg >= 1.0:
        y = float(np.nextafter(y, 0.0))
    while sepal_rate(float(np.nextafter(y, np.inf)), n, M) * deg < 1.0:
        y = float(np.nextafter(y, np.inf))
    return y


def sepal_lds_bytes(n):
    """The LDS bytes a workgroup needs to keep the image of a time point of n spots."""
    return SEPAL_LDS_FIXED + 8 * int(n)


def sepal_stride(desc, lds_limit=None):
    """The doubles of one item's row of the state's image, as the library computes it: the largest n, plus the largest n of
    the time points whose image does not fit in LDS (the second slab of that path; 0 if all fit)."""
    lds_limit = _lds_limit(lds_limit, SEPAL_LDS_BYTES)
    return max(int(n) for n in desc[:, 1]) + max([int(n) for n in desc[:, 1] if sepal_lds_bytes(n) > lds_limit] or [0])


def sepal_check(rowptr, col, colptr, ridx, values, genes, desc, dt, thresh, n_iter, steps):
    """The refusals of sepal_steps, before any launch: dt, thresh, n_iter and steps, the limits from the descriptor, then per
    time point the range of col, the order of rowptr and the largest degree, the range of the row indices and of the selected
    genes, the order of colptr and the smallest value and whether all are finite by reductions on the device (one host round
    trip); last dt against the largest degree: a max deg >= 1 is refused with the largest admissible dt.  Returns (the
    descriptor with columns 6 and 7 filled in, the smallest row index, the largest, the smallest selected gene, the largest, the
    rates fp64 [T]); ValueError otherwise."""
    need_cuda(rowptr, col, colptr, ridx, values, genes)
    desc = _host_desc(desc, SEPAL_DESC, "time point")
    T = int(desc.shape[0])
    dt, thresh, n_iter, steps = float(dt), float(thresh), int(n_iter), int(steps)
    if not (dt > 0.0 and np.isfinite(dt)) or not (thresh >= 0.0 and np.isfinite(thresh)):
        raise ValueError(f"sepal takes a finite dt > 0 and a finite thresh >= 0 (got dt = {dt}, thresh = {thresh})")
    if not 1 <= n_iter <= SEPAL_MAX or not 1 <= steps <= SEPAL_MAX:
        raise ValueError(f"sepal takes 1 to {SEPAL_MAX} steps in all and per launch (got n_iter = {n_iter}, steps = {steps})")
    _typed((rowptr, torch.int32, "rowptr"), (col, torch.int32, "col"), (ridx, torch.int32, "ridx"), (colptr, torch.int64, "colptr"),
           (values, torch.float32, "values"), (genes, torch.int32, "genes"))
    (G, nnz), ng = _csc_sizes(colptr, ridx, values, SEPAL_MAX), int(genes.numel())
    if ng < 1:
        raise ValueError("spadot_sepal_steps takes at least one selected gene")
    rows = 0
    for t, (eoff, n, M, row0, _gid, roff, _lo, _hi) in enumerate(desc.tolist()):
        _refuse_time_point(t, "spadot_sepal_steps", desc[t].tolist(), n, M, SEPAL_MAX,
                           eoff >= 0 and roff >= 0 and 0 <= row0 <= SEPAL_MAX)
        if eoff + M > col.numel() or roff + n + 1 > rowptr.numel():
            raise ValueError(f"time point {t}: its rows or edges reach past the end of the tensors")
        rows = max(rows, row0 + n)
    if T * ng > SEPAL_MAX:
        raise ValueError(f"the call holds more than {SEPAL_MAX} workgroups (the grid of one launch)")
    zero = torch.zeros((), dtype=torch.int64, device=colptr.device)
    degs = [torch.diff(rowptr[roff:roff + n + 1]).max().long() for _e, n, _M, _r, _g, roff, *_rest in desc.tolist()]
    vals = [values.min() < 0, ~torch.isfinite(values).all()] if nnz > 0 else [zero, zero]
    stats = (_csr_stats(rowptr, col, desc, zero) + _csc_stats(colptr, ridx, zero) + [s.long() for s in torch.aminmax(genes)]
             + degs + [v.long() for v in vals])
    stats = torch.stack(stats).cpu().numpy()                                # the one host round trip ahead of the launch
    _refuse_csr(desc, stats[:5 * T].reshape(T, 5))
    ridx_lo, ridx_hi, c0, c1, unordered, gene_lo, gene_hi = (int(v) for v in stats[5 * T:5 * T + 7])
    _refuse_rows(ridx_lo, ridx_hi, nnz, rows)
    _refuse_genes(gene_lo, gene_hi, G)
    _refuse_colptr(c0, c1, unordered, nnz)
    if stats[-1]:
        raise ValueError("the values hold entries that are not finite: sepal diffuses finite values >= 0")
    if stats[-2]:
        raise ValueError("the values hold negative entries: sepal diffuses finite values >= 0")
    rate = np.zeros(T, dtype=np.float64)
    for t, deg in enumerate(stats[5 * T + 7:6 * T + 7].tolist()):
        n, M = int(desc[t, 1]), int(desc[t, 2])
        rate[t] = sepal_rate(dt, n, M)
        if M > 0 and not rate[t] * deg < 1.0:
            raise ValueError(f"dt = {dt} is too large for time point {t}: with {n} spots, {M // 2} edges and a largest degree of "
                             f"{deg} the rate a = dt n / (2 E) = {rate[t]} gives a max deg >= 1 and the explicit step is "
                             f"unstable; the largest admissible dt is {sepal_max_dt(n, M, deg)!r}")
        if M > 0 and not rate[t] > 0.0:
            raise ValueError(f"dt = {dt} gives time point {t} the rate {rate[t]}: it must be above 0")
    return desc, ridx_lo, ridx_hi, gene_lo, gene_hi, rate


def sepal_state(desc, ng, device, lds_limit=None, trace_len=0):
    """The per-item state of sepal_launch for a descriptor, items = T ng: image fp64 [items, sepal_stride] (zeros), H_prev and H0
    fp64 [items] (NaN), iterations and done int32 [items] (zeros) and, with trace_len, trace fp64 [items, trace_len] (NaN)."""
    items = int(desc.shape[0]) * int(ng)
    state = dict(image=torch.zeros((items, sepal_stride(desc, lds_limit)), dtype=torch.float64, device=device),
                 H_prev=torch.full((items,), float("nan"), dtype=torch.float64, device=device),
                 H0=torch.full((items,), float("nan"), dtype=torch.float64, device=device),
                 iterations=torch.zeros(items, dtype=torch.int32, device=device),
                 done=torch.zeros(items, dtype=torch.int32, device=device))
    if trace_len:
        state["trace"] = torch.full((items, int(trace_len)), float("nan"), dtype=torch.float64, device=device)
    return state


def _sepal_state_ok(state, items, stride):
    for name, dt in (("image", torch.float64), ("H_prev", torch.float64), ("H0", torch.float64), ("iterations", torch.int32),
                     ("done", torch.int32)):
        t = state[name]
        if t.dtype != dt or not t.is_contiguous() or int(t.shape[0]) != items or (name != "image" and t.numel() != items):
            raise ValueError(f"the state's {name} must be a contiguous {dt} tensor of {items} items (got {tuple(t.shape)} {t.dtype})")
    if state["image"].dim() != 2 or int(state["image"].shape[1]) < stride:
        raise ValueError(f"the state's image must hold {stride} doubles per item (got {tuple(state['image'].shape)})")
    trace = state.get("trace")
    if trace is not None and (trace.dtype != torch.float64 or not trace.is_contiguous() or trace.dim() != 2
                              or int(trace.shape[0]) != items or int(trace.shape[1]) < 1):
        raise ValueError(f"the state's trace must be a contiguous float64 tensor [{items}, columns >= 1] (got {tuple(trace.shape)})")


def sepal_launch(rowptr, col, colptr, ridx, values, genes, checked, state, init, steps, n_iter, thresh, stop=True, lds_limit=None,
                 desc_dev=None, rate_dev=None):
    """One launch of at most `steps` further steps of every item that is not done, on the state of sepal_state, for what
    sepal_check has returned (the library checks the descriptor again, on the host).  init: the first launch, which builds the
    images and H0; stop: apply the stop rule.  lds_limit must be the one the state was made for.  No host synchronisation."""
    desc, ridx_lo, ridx_hi, gene_lo, gene_hi, rate = checked
    need_cuda(rowptr, col, colptr, ridx, values, genes, desc_dev, rate_dev, *state.values())
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    rate = np.ascontiguousarray(rate, dtype=np.float64)
    T, G, ng = int(desc.shape[0]), int(colptr.numel()) - 1, int(genes.numel())
    lds_limit = _lds_limit(lds_limit, SEPAL_LDS_BYTES)
    _sepal_state_ok(state, T * ng, sepal_stride(desc, lds_limit))
    dev = colptr.device
    if desc_dev is None:
        desc_dev = torch.as_tensor(desc, device=dev)
    if rate_dev is None:
        rate_dev = torch.as_tensor(rate, device=dev)
    image, trace = state["image"], state.get("trace")
    rc = model_lib().spadot_sepal_steps(_p(rowptr), _p(col), _p(colptr), _p(ridx), _p(values), int(ridx.numel()), ridx_lo, ridx_hi,
                                        _host(desc), _p(desc_dev), _host(rate), _p(rate_dev), T, G, _p(genes), ng, gene_lo, gene_hi,
                                        int(bool(init)), int(bool(stop)), int(steps), int(n_iter), float(thresh), lds_limit,
                                        _p(image), int(image.numel()), int(image.shape[1]), _p(state["H_prev"]), _p(state["H0"]),
                                        _p(state["iterations"]), _p(state["done"]), _p(trace),
                                        int(trace.shape[1]) if trace is not None else 0, _stream())
    launched(rc, "spadot_sepal_steps", SEPAL_LIMITS)
    return state


def sepal_steps(rowptr, col, colptr, ridx, values, genes, desc, dt, thresh=1e-8, n_iter=30000, steps_per_launch=None, stop=True,
                lds_limit=None, state=None, trace_len=0):
    """The diffusion of every (time point, selected gene) until it stops or has taken n_iter steps (include/spadot_model.h:
    spadot_sepal_steps).  rowptr, col int32: the symmetric CSR of the time points back to back; colptr int64, ridx int32 and
    values fp32: the CSC arrays of a DeviceCounts; genes int32: the selected genes; desc: int64 [T, 8] on the host as
    moran.edge_csr lays it out (columns 6 and 7, the range of col, are filled in here); dt: the time step, from which the rate
    of a time point is sepal_rate(dt, n, M).  Launches of steps_per_launch (default 2048) steps follow one another until every item is
    done or has reached n_iter; between two launches the host reads the flags and the counts, one small copy.  stop=False: no
    stop rule, exactly n_iter steps.  lds_limit: the LDS bytes a workgroup may use (default and at most 98816); a time point
    whose image does not fit keeps it in the state, with the same bits.  state: a sepal_state to run in (default: a fresh one;
    trace_len: with a trace of that many columns).  Returns the state.  ValueError, before any launch, outside the limits;
    RuntimeError for a CPU tensor."""
    steps = SEPAL_STEPS if steps_per_launch is None else int(steps_per_launch)
    checked = sepal_check(rowptr, col, colptr, ridx, values, genes, desc, dt, thresh, n_iter, steps)
    dev, ng = colptr.device, int(genes.numel())
    if state is None:
        state = sepal_state(checked[0], ng, dev, lds_limit, trace_len)
    else:
        need_cuda(*state.values())
        _sepal_state_ok(state, int(checked[0].shape[0]) * ng, sepal_stride(checked[0], _lds_limit(lds_limit, SEPAL_LDS_BYTES)))
    desc_dev, rate_dev = torch.as_tensor(checked[0], device=dev), torch.as_tensor(checked[5], device=dev)
    init = True
    while True:
        sepal_launch(rowptr, col, colptr, ridx, values, genes, checked, state, init, steps, n_iter, thresh, stop, lds_limit, desc_dev,
                     rate_dev)
        init = False
        flags = torch.stack([state["done"], state["iterations"]]).cpu().numpy()      # the one small copy between two launches
        if np.all((flags[0] != 0) | (flags[1] >= int(n_iter))):
            return state
