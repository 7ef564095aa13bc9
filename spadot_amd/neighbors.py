"""The neighbors stage: where the domains lie in the tissue.  On the spatial k-nearest-neighbour graph of every time point, the
neighbourhood-enrichment permutation test (squidpy's gr.nhood_enrichment): which domains border which, which avoid each other,
how compact each domain is (csrc/nhood.hip).  The reference has no such stage; the definition is restated in numpy in
tests/nhood_ref.py.

    nhood_counts(edges, labelings)        the count matrices of many (graph, labeling) problems in ONE launch
    nhood_enrichment(edges, labels)       the test: observed counts and all permutations of all graphs in one call
    spatial_edges(coords, k=6)            the directed k-nearest-neighbour graph of one time point, on the device
    neighbors(args)    the stage.  args: domains ({prefix}domains.csv of analyze), output_dir, prefix (''), k (6), n_perms (1000),
                       seed (0), device

A problem is a directed edge list i -> j over n nodes (no self loops; duplicates are counted) and a labeling in 0 .. K-1; its
count matrix is C[a, b] = #{edges i -> j : lab[i] = a, lab[j] = b}.  With C_p the count matrix of the labeling lab[pi_p(i)],
p = 0 .. P-1, in fp64 on the host from the integers:
    expected = mean_p C_p,  sd = std_p C_p (ddof 0),  zscore = (C - expected) / sd (NaN where sd = 0),
    p_enriched = (1 + #{p : C_p >= C}) / (P + 1),  p_depleted = (1 + #{p : C_p <= C}) / (P + 1),
    padj = Benjamini-Hochberg of min(1, 2 min(p_enriched, p_depleted)) over the cells whose two domains both hold spots (NaN in
    the others),  share[a, b] = C[a, b] / sum_b C[a, b],  coherence[a] = share[a, a].
pi_p is a pure function of (seed, graph index g, p, n): a balanced Feistel network on b bits, b = ceil(log2 n) rounded up to an
even number and at least 2, six rounds L, R = R, L ^ (mix32(R ^ key_r) & mask) with mix32 the xorshift-multiply mixer (shifts 16 /
15 / 15, multipliers 0x21F0AAAD / 0x735A2D97), round keys the low 32 bits of six splitmix64 draws from the state
splitmix64(seed ^ (g << 32) ^ p), applied again while the value is >= n (cycle walking).

The device counts; the host validates, takes the statistics and writes the files.  Limits: 1 <= K <= 32, at most 2147483647
nodes and edges per graph and labelings per call."""
import sys
import time

import numpy as np

from .utils._stage_utils import (cuda_device, edge_pair, open_output, plot_timepoints, read_domains_table, timings,
                                 write_timepoints)

MAX_CLUSTERS = 32
MAX_NODES = 2147483647
TABLE_COLUMNS = ("domain", "neighbor", "count", "expected", "sd", "zscore", "share", "p_enriched", "p_depleted", "padj")
SPOT_COLUMNS = ("row", "timepoint", "kmeans", "same")
MATRICES = ("counts", "expected", "sd", "zscore", "p_enriched", "p_depleted", "padj", "share", "coherence", "sizes")


class Permuted:
    """The labelings base[pi_p(i)] for p = first .. first + n_perms - 1 of graph index `graph` under `seed`: what nhood_counts
    takes in place of explicit labelings."""

    def __init__(self, base, n_perms, seed=0, graph=0, first=0):
        self.base, self.n_perms, self.seed, self.graph, self.first = base, int(n_perms), int(seed), int(graph), int(first)
        if self.n_perms < 1 or self.first < 0 or self.graph < 0:
            raise ValueError(f"Permuted takes n_perms >= 1, first >= 0 and graph >= 0 (got {n_perms}, {first}, {graph})")


class NhoodResult:
    """One graph: counts int64 [K, K], perm_counts int32 [P, K, K], sizes int64 [K] and the fp64 statistics of the module
    docstring (expected, sd, zscore, p_enriched, p_depleted, padj, share [K, K]; coherence [K])."""

    def __init__(self, counts, perm_counts, sizes):
        self.counts, self.perm_counts, self.sizes = counts, perm_counts, sizes
        for name, v in enrichment_stats(counts, perm_counts, sizes).items():
            setattr(self, name, v)


def enrichment_stats(counts, perm_counts, sizes):
    """The host statistics of one graph from its integers (module docstring): a dict of fp64 arrays."""
    from .markers import bh_adjust
    C = np.asarray(counts, dtype=np.float64)
    Cp = np.asarray(perm_counts)
    P = Cp.shape[0]
    expected = Cp.mean(axis=0, dtype=np.float64)
    sd = Cp.std(axis=0, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd > 0, (C - expected) / sd, np.nan)
        rows = C.sum(axis=1, keepdims=True)
        share = np.where(rows > 0, C / rows, np.nan)
    obs = np.asarray(counts)[None]
    p_enriched = (1.0 + (Cp >= obs).sum(axis=0)) / (P + 1.0)
    p_depleted = (1.0 + (Cp <= obs).sum(axis=0)) / (P + 1.0)
    has = np.asarray(sizes) > 0
    family = has[:, None] & has[None, :]                        # a domain without spots is left out of the BH family
    padj = np.full(C.shape, np.nan)
    padj[family] = bh_adjust(np.minimum(1.0, 2.0 * np.minimum(p_enriched, p_depleted))[family])
    return dict(expected=expected, sd=sd, zscore=z, p_enriched=p_enriched, p_depleted=p_depleted, padj=padj, share=share,
                coherence=np.diagonal(share).copy())


def _label_block(lab, dev, g):
    """An integer labeling block as a device tensor, with its smallest and largest label as 0-d device tensors."""
    import torch
    lab = lab if isinstance(lab, torch.Tensor) else torch.as_tensor(np.asarray(lab))
    if lab.dtype.is_floating_point or lab.dtype == torch.bool or lab.dtype.is_complex:
        raise ValueError(f"labels must be integers (graph {g}: {lab.dtype})")
    if lab.numel() == 0:
        raise ValueError(f"graph {g} has no nodes: a graph takes at least one")
    lab = lab.to(dev)
    lo, hi = torch.aminmax(lab)
    return lab, lo.long(), hi.long()


def _run(edges, problems, lds_limit=None, out=None):
    """edges: [(src, dst)] device tensors per edge set; problems: dicts with `e` (edge set), `lab` (index into the label blocks),
    `blocks` shared through problems[0]['blocks'], n, K, L, p0 (-1: explicit labelings), gid, seed.  One launch; returns the
    int32 [sum L, K_max, K_max] device tensor."""
    import torch
    from .stage_ops import NHOOD_DESC, nhood_counts as launch
    blocks = problems[0]["blocks"]
    dev = blocks[0].device
    with torch.cuda.device(dev):
        eoff = np.concatenate([[0], np.cumsum([int(s.shape[0]) for s, _ in edges])]).astype(np.int64)
        loff = np.concatenate([[0], np.cumsum([int(b.numel()) for b in blocks])]).astype(np.int64)
        src = torch.cat([s.to(torch.int32) for s, _ in edges]) if len(edges) > 1 else edges[0][0].to(torch.int32).contiguous()
        dst = torch.cat([d.to(torch.int32) for _, d in edges]) if len(edges) > 1 else edges[0][1].to(torch.int32).contiguous()
        labels = torch.cat([b.reshape(-1) for b in blocks]) if len(blocks) > 1 else blocks[0].reshape(-1).contiguous()
        desc = np.zeros((len(problems), NHOOD_DESC), dtype=np.int64)
        item = 0
        for i, q in enumerate(problems):
            desc[i, :10] = (eoff[q["e"]], q["n"], eoff[q["e"] + 1] - eoff[q["e"]], q["K"], loff[q["lab"]], q["L"], q["p0"],
                            q["gid"], item, np.array(q["seed"] & (2 ** 64 - 1), dtype=np.uint64).astype(np.int64))
            item += q["L"]
        return launch(src, dst, labels, desc, max(q["K"] for q in problems), lds_limit=lds_limit, out=out)


def _check_range(lo, hi, K, g):
    if not 1 <= K <= MAX_CLUSTERS:
        raise ValueError(f"graph {g} has {K} label values: the device counts 1 to {MAX_CLUSTERS} domains")
    if lo < 0 or hi >= K:
        raise ValueError(f"graph {g} holds labels {lo} .. {hi}: labels must lie in 0 .. {K - 1}")


def nhood_counts(edges, labelings, n_clusters=None, lds_limit=None, out=None):
    """edges[g]: (src, dst) integer device tensors of graph g; labelings[g]: an integer array or tensor [L, n] (or [n]: one
    labeling) of explicit labelings, or a Permuted.  n_clusters[g]: the K of graph g (default: its largest label + 1).
    lds_limit: the LDS bytes a workgroup may use (default 163840): a graph whose n label bytes do not fit beside its four
    histograms (16 K^2 + n rounded up to 16 > lds_limit) reads its labels from global memory.  One launch for the whole call;
    returns [g] -> int32 numpy [L, K, K].  ValueError / RuntimeError before any launch; out: an int32 device tensor
    [sum L, K_max, K_max] to write into."""
    import torch
    if not edges or len(edges) != len(labelings):
        raise ValueError(f"nhood_counts takes one labeling block per graph ({len(edges)} graphs, {len(labelings)} blocks)")
    if n_clusters is not None and len(n_clusters) != len(edges):
        raise ValueError(f"n_clusters holds {len(n_clusters)} cluster counts for {len(edges)} graphs")
    pairs, dev = [], None
    for g, e in enumerate(edges):
        pairs.append(edge_pair(e, dev, g))
        dev = pairs[-1][0].device
    blocks, problems, ranges = [], [], []
    for g, lab in enumerate(labelings):
        spec = lab if isinstance(lab, Permuted) else None
        block, lo, hi = _label_block(spec.base if spec else lab, dev, g)
        if spec:
            if block.dim() != 1:
                raise ValueError(f"the base labeling of graph {g} must be 1-d (got {tuple(block.shape)})")
        elif block.dim() == 1:
            block = block[None]
        elif block.dim() != 2:
            raise ValueError(f"the labelings of graph {g} must form an [L, n] block (got {tuple(block.shape)})")
        blocks.append(block)
        ranges += [lo, hi]
        problems.append(dict(e=g, lab=g, n=int(block.shape[-1]), L=spec.n_perms if spec else int(block.shape[0]),
                             p0=spec.first if spec else -1, gid=spec.graph if spec else g, seed=spec.seed if spec else 0))
    ranges = torch.stack(ranges).cpu().numpy().reshape(-1, 2)
    for g, q in enumerate(problems):
        q["K"] = int(ranges[g, 1]) + 1 if n_clusters is None else int(n_clusters[g])
        _check_range(int(ranges[g, 0]), int(ranges[g, 1]), q["K"], g)
    problems[0]["blocks"] = [b.to(torch.uint8) for b in blocks]
    res = _run(pairs, problems, lds_limit, out).cpu().numpy()
    outs, item = [], 0
    for q in problems:
        outs.append(np.ascontiguousarray(res[item:item + q["L"], :q["K"], :q["K"]]))
        item += q["L"]
    return outs


def nhood_enrichment(edges, labels, n_perms=1000, seed=0, n_clusters=None):
    """The permutation test of every graph (module docstring): edges[g] = (src, dst) device tensors, labels[g] the observed
    labeling (integers, numpy or torch), n_clusters[g] its K (default: largest label + 1).  The observed labelings and all
    n_perms permutations of all graphs are counted by one call to the library; graph g permutes under (seed, g).  Returns
    [g] -> NhoodResult."""
    import torch
    n_perms = int(n_perms)
    if n_perms < 1:
        raise ValueError(f"the permutation test takes at least one permutation (got n_perms = {n_perms})")
    if not edges or len(edges) != len(labels):
        raise ValueError(f"nhood_enrichment takes one labeling per graph ({len(edges)} graphs, {len(labels)} labelings)")
    if n_clusters is not None and len(n_clusters) != len(edges):
        raise ValueError(f"n_clusters holds {len(n_clusters)} cluster counts for {len(edges)} graphs")
    pairs, dev = [], None
    for g, e in enumerate(edges):
        pairs.append(edge_pair(e, dev, g))
        dev = pairs[-1][0].device
    blocks, ranges = [], []
    for g, lab in enumerate(labels):
        block, lo, hi = _label_block(lab, dev, g)
        if block.dim() != 1:
            raise ValueError(f"the labeling of graph {g} must be 1-d (got {tuple(block.shape)})")
        blocks.append(block)
        ranges += [lo, hi]
    ranges = torch.stack(ranges).cpu().numpy().reshape(-1, 2)
    problems = []
    for g, block in enumerate(blocks):
        K = int(ranges[g, 1]) + 1 if n_clusters is None else int(n_clusters[g])
        _check_range(int(ranges[g, 0]), int(ranges[g, 1]), K, g)
        common = dict(e=g, lab=g, n=int(block.shape[0]), K=K, gid=g, seed=int(seed))
        problems.append(dict(common, L=1, p0=-1))                   # the observed labeling: the base of the permutations
        problems.append(dict(common, L=n_perms, p0=0))
    problems[0]["blocks"] = [b.to(torch.uint8) for b in blocks]
    sizes = [torch.bincount(b, minlength=problems[2 * g]["K"]) for g, b in enumerate(blocks)]
    res = _run(pairs, problems).cpu().numpy()
    out, item = [], 0
    for g in range(len(blocks)):
        K = problems[2 * g]["K"]
        counts = res[item, :K, :K].astype(np.int64)
        perm = np.ascontiguousarray(res[item + 1:item + 1 + n_perms, :K, :K])
        item += 1 + n_perms
        out.append(NhoodResult(counts, perm, sizes[g].cpu().numpy().astype(np.int64)))
    return out


def knn_rows_to_edges(idx, k):
    """The rows of a k-nearest-neighbour table (idx [n, kk], every row ordered by distance, the spot itself somewhere in it or,
    among duplicates, not at all) as directed edges: the spot itself is dropped wherever it appears in its row and the first k
    others are kept.  Returns (src, dst), row by row, int32, on idx's device."""
    import torch
    n, kk = idx.shape
    rows = torch.arange(n, device=idx.device, dtype=idx.dtype)[:, None]
    keep = idx != rows
    keep &= torch.cumsum(keep, dim=1) <= k
    return rows.expand(n, kk)[keep].to(torch.int32), idx[keep].to(torch.int32)


def spatial_edges(coords, k=6, device="cuda:0"):
    """The directed spatial graph of one time point: every spot -> its k nearest other spots (ops.knn: fp64, ordered by
    (distance, index)).  coords [n, 2] numpy or tensor.  Fewer than k + 1 spots: n - 1 neighbours per spot; one spot: no edges.
    Returns (src, dst) int32 device tensors, src ascending."""
    import torch
    from .ops import knn
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("spadot_amd builds the spatial graph on the MI355X only (device 'cuda:N'); there is no CPU path")
    k = int(k)
    if not 1 <= k <= 127:
        raise ValueError(f"a spatial graph takes k = 1 .. 127 neighbours (got {k})")
    x = coords if isinstance(coords, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(coords, dtype=np.float64))
    if x.dim() != 2 or x.shape[0] < 1 or not 1 <= x.shape[1] <= 4:
        raise ValueError(f"coords must be an [n, d] array of at least one spot in 1 to 4 dimensions (got {tuple(x.shape)})")
    x = x.to(dev)
    n = int(x.shape[0])
    if n == 1:
        empty = torch.empty(0, dtype=torch.int32, device=dev)
        return empty, empty.clone()
    with torch.cuda.device(dev):
        return knn_rows_to_edges(knn(x, min(k + 1, n)), k)


def same_domain_share(src, dst, labels):
    """Per spot the share of its neighbours (edges src -> dst) in its own domain, fp64 on the labels' device; NaN for a spot
    without neighbours."""
    import torch
    n = labels.shape[0]
    s, d = src.long(), dst.long()
    deg = torch.bincount(s, minlength=n).to(torch.float64)
    own = torch.bincount(s, weights=(labels[s] == labels[d]).to(torch.float64), minlength=n)
    return own / deg


def nhood_table(r):
    """The rows of {prefix}nhood_{tp}.csv: one per ordered pair (domain, neighbor), domain-major."""
    import pandas as pd
    K = r.counts.shape[0]
    a, b = np.divmod(np.arange(K * K), K)
    return pd.DataFrame({"domain": a, "neighbor": b, "count": r.counts.reshape(-1), "expected": r.expected.reshape(-1),
                         "sd": r.sd.reshape(-1), "zscore": r.zscore.reshape(-1), "share": r.share.reshape(-1),
                         "p_enriched": r.p_enriched.reshape(-1), "p_depleted": r.p_depleted.reshape(-1),
                         "padj": r.padj.reshape(-1)}, columns=list(TABLE_COLUMNS))


def neighbors(args):
    """Reads args.domains (the domains.csv of analyze: row, timepoint, kmeans, pixel_x, pixel_y); builds the k-nearest-neighbour
    graph of every time point and runs one nhood_enrichment call.  Writes {prefix}nhood_{tp}.csv (TABLE_COLUMNS, one row per
    ordered pair of domains), {prefix}nhood.npz ('{tp}_{matrix}' for MATRICES, plus timepoints, seed, k, n_perms),
    {prefix}nhood_spots.csv (row, timepoint, kmeans, same: the share of the spot's neighbours in its own domain, input order)
    and, with matplotlib, {prefix}{tp}_nhood.png.  Returns {'tables', 'results' (per time point), 'spots', 'timepoints',
    'timings'}."""
    import pandas as pd
    from .utils import _analyze_utils
    t_start = time.perf_counter()
    tab = read_domains_table(args, "neighbors")
    k, n_perms, seed = int(getattr(args, "k", 6)), int(getattr(args, "n_perms", 1000)), int(getattr(args, "seed", 0))
    if k < 1 or n_perms < 1:
        raise ValueError(f"the neighbors stage takes k >= 1 and n_perms >= 1 (got k = {k}, n_perms = {n_perms})")
    out_file = open_output(args, tab.beside)

    import torch
    dev = cuda_device(args, "counts neighbourhoods")
    tps, masks = tab.tps, tab.masks
    t_read = time.perf_counter()
    edges = [spatial_edges(tab.coords[m], k, dev) for m in masks]
    labs = [torch.as_tensor(tab.labels[m], device=dev) for m in masks]
    torch.cuda.synchronize(dev)
    t_graph = time.perf_counter()
    res = nhood_enrichment(edges, labs, n_perms=n_perms, seed=seed, n_clusters=tab.Ks)
    same = np.empty(tab.n, dtype=np.float64)
    for m, (src, dst), lab in zip(masks, edges, labs):
        same[m] = same_domain_share(src, dst, lab).cpu().numpy()
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter()

    tables, arrays = write_timepoints(out_file, "nhood", tps, res, lambda t, r: nhood_table(r), MATRICES)
    np.savez(out_file("nhood.npz"), timepoints=np.asarray(tps), seed=np.int64(seed), k=np.int64(k), n_perms=np.int64(n_perms),
             **arrays)
    spots = pd.DataFrame({"row": tab.row_ids, "timepoint": tab.tp_all, "kmeans": tab.labels, "same": same},
                         columns=list(SPOT_COLUMNS))
    spots.to_csv(out_file("nhood_spots.csv"), index=False)
    plot_timepoints(tps, res, lambda tp, r: _analyze_utils.plot_nhood(out_file(f"{tp}_nhood.png"), r.zscore, tp))
    t_end = time.perf_counter()
    print(f"neighbors: {tab.n} spots of {len(tps)} time points, k = {k}, {n_perms} permutations, written to {args.output_dir}",
          file=sys.stderr)
    return {"tables": tables, "results": dict(zip(tps, res)), "spots": spots, "timepoints": tps,
            "timings": timings(t_start, t_read, t_dev, t_end, t_graph)}
