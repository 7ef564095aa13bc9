"""The territories stage: the connected pieces of every domain.  Is domain 3 one piece of tissue or forty, which spots are the
stray ones, and can the map be cleaned of them?  (csrc/territories.hip)  The reference has no such stage; the
definition is restated with numpy and scipy in tests/territories_ref.py.

    territory_counts(edges, labelings)    the integers of many (graph, labeling) problems in ONE launch
    territories(edges, labels)            the observed labeling and all relabelings of all graphs in one call, with statistics
    territory_stats(obs, perm, sizes)     the host statistics from the integers
    refine_labels(edges, labels, s)       small territories handed to the domain they touch most
    territories_stage(args)   the stage.  args: domains ({prefix}domains.csv of analyze), output_dir, prefix (''), k (6), n_perms
                              (1000), seed (0), min_size (0: off), alpha (0.05), device

A problem is the directed edge list i -> j over n spots, as spatial_edges(coords, k) returns it, with a labeling in 0 .. K-1,
1 <= K <= 32.  Direction is ignored: an edge in either direction connects its ends.  Duplicates and edges present in both
directions change nothing.

A territory is a connected component of the subgraph that keeps only the edges whose two ends carry the same label.  Its id is
the smallest spot index it contains.  This makes the answer a pure function of the problem: it does not depend on thread order,
batching or path.

Per (labeling, domain a) four integers, int64: `count`, the number of territories; `largest`, the size of the largest;
`singletons`, the number of territories of one spot; `sumsq`, the sum of size^2.  A label value without spots gives 0, 0, 0, 0.

Permuted labelings are lab[pi_p(i)] with the Feistel relabelings, the (seed, graph id, p, n) convention and the Permuted spec
of neighbors (csrc/feistel_perm.h).

Host statistics, fp64 from the integers, with `sizes` from a bincount:
    largest_share = largest / size,  contiguity = sumsq / size^2: the chance that two spots of the domain, drawn with
    replacement, lie in one territory; 1 means one piece.
With P >= 1 relabelings: expected, sd (ddof 0) and z of count and of contiguity (z is NaN where sd = 0);
    p_fewer = (1 + #{p : count_p <= count}) / (P + 1),  p_more = (1 + #{p : count_p >= count}) / (P + 1),
    padj = Benjamini-Hochberg (markers.bh_adjust) of min(1, 2 min(p_fewer, p_more)) over the domains that hold spots, NaN in the
    others; the verdict is `contiguous` if padj <= alpha and count < expected, `fragmented` if padj <= alpha and count >
    expected, otherwise `random`.  With P = 0 the null columns are NaN and the verdict is empty.
What the null is worth: a label dealt at random over the spots lies far below the percolation threshold of a k-nearest-
neighbour graph (7 labels on a jittered 100 x 100 grid, k = 6: 5 904 territories, the largest of 14 spots), so almost any real
domain reads `contiguous`, as almost any real pair reads attract or avoid under the null of cooccurrence.  The useful number is
z: a standardised contiguity that compares across domains, time points and k.

Per spot of the observed labeling: `territory` (the id), `territory_size`, and `boundary`: True if some edge at the spot, in
either direction, leads to another label.

Refinement (min_size s >= 2) runs in rounds on the current labels.  A territory is small if its size is below s.  For every
small territory the edges, symmetrised with multiplicity, from its spots to spots of territories that are not small are counted
by the label of the far end; a small territory with at least one such edge takes the label with the largest count, ties to
the smallest label.  All territories of a round decide on the labels from before the round.  Refinement stops when a round
changes nothing, or after max_rounds.  A small territory that touches only small ones waits for a later round; the number of
spots in small territories falls strictly in every round that changes anything (a territory that moves joins one that is not
small, and no territory shrinks), so the loop ends; small territories of different labels that touch only each other never swap.

The device finds the territories; the host validates, takes the statistics, votes and writes the files.  Limits: those of
neighbors (1 <= K <= 32, at most 2147483647 spots and edges per graph and labelings per call)."""
import sys
import time

import numpy as np

from .neighbors import Permuted, _check_range, _label_block
from .utils._stage_utils import (cuda_device, edge_pair, open_output, plot_timepoints, read_domains_table, timings,
                                 write_timepoints)

INTEGERS = ("count", "largest", "singletons", "sumsq")
NULL_COLUMNS = ("count_expected", "count_sd", "count_z", "contiguity_expected", "contiguity_sd", "contiguity_z", "p_fewer",
                "p_more", "padj")
TABLE_COLUMNS = ("domain", "size", "count", "largest", "largest_share", "singletons", "contiguity") + NULL_COLUMNS + ("verdict",)
SPOT_COLUMNS = ("row", "timepoint", "kmeans", "territory", "territory_size", "boundary")
DOMAIN_COLUMNS = ("row", "timepoint", "kmeans", "pixel_x", "pixel_y")
MATRICES = ("sizes", "counts", "perm_counts", "largest_share", "contiguity") + NULL_COLUMNS + ("territory", "territory_size",
                                                                                              "boundary")
MAX_PERMS = 9999
MAX_ROUNDS = 64


class TerritoryCounts:
    """One problem of territory_counts: counts int64 [L, K, 4] (INTEGERS per labeling and label value), rounds int32 [L] (the
    rounds the workgroup ran: they may differ from run to run, the counts may not) and, where asked for, ids and sizes int32 [n]
    of the first labeling: per spot the id and the size of its territory."""

    def __init__(self, counts, rounds, ids=None, sizes=None):
        self.counts, self.rounds, self.ids, self.sizes = counts, rounds, ids, sizes


class TerritoryResult:
    """One graph: counts int64 [K, 4], perm_counts int64 [P, K, 4], sizes int64 [K], territory and territory_size int32 [n],
    boundary bool [n], rounds (of the observed labeling), verdict [K] and the fp64 statistics of the module docstring [K]."""

    def __init__(self, counts, perm_counts, sizes, territory, territory_size, boundary, rounds, alpha):
        self.counts, self.perm_counts, self.sizes = counts, perm_counts, sizes
        self.territory, self.territory_size, self.boundary, self.rounds = territory, territory_size, boundary, rounds
        for name, v in territory_stats(counts, perm_counts, sizes, alpha).items():
            setattr(self, name, v)


def territory_stats(obs, perm, sizes, alpha=0.05):
    """The host statistics of one graph from its integers (module docstring): obs int [K, 4], perm int [P, K, 4] (P may be 0),
    sizes [K].  A dict of fp64 arrays [K] and `verdict`, an array of str."""
    from .markers import bh_adjust
    obs = np.asarray(obs, dtype=np.int64)
    K = obs.shape[0]
    perm = np.asarray(perm, dtype=np.int64).reshape(-1, K, 4)
    size = np.asarray(sizes, dtype=np.float64)
    P = perm.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(largest_share=obs[:, 1] / size, contiguity=obs[:, 3] / (size * size))
        if P == 0:
            out.update({name: np.full(K, np.nan) for name in NULL_COLUMNS})
            out["verdict"] = np.array([""] * K, dtype=object)
            return out
        cont_p = perm[:, :, 3] / (size * size)[None]
        for name, o, p in (("count", obs[:, 0].astype(np.float64), perm[:, :, 0]), ("contiguity", out["contiguity"], cont_p)):
            expected, sd = p.mean(axis=0, dtype=np.float64), p.std(axis=0, dtype=np.float64)
            out[name + "_expected"], out[name + "_sd"] = expected, sd
            out[name + "_z"] = np.where(sd > 0, (o - expected) / sd, np.nan)
    out["p_fewer"] = (1.0 + (perm[:, :, 0] <= obs[None, :, 0]).sum(axis=0)) / (P + 1.0)
    out["p_more"] = (1.0 + (perm[:, :, 0] >= obs[None, :, 0]).sum(axis=0)) / (P + 1.0)
    has = size > 0                                               # a domain without spots is left out of the BH family
    padj = np.full(K, np.nan)
    padj[has] = bh_adjust(np.minimum(1.0, 2.0 * np.minimum(out["p_fewer"], out["p_more"]))[has])
    out["padj"] = padj
    with np.errstate(invalid="ignore"):
        sig = padj <= alpha
    verdict = np.array(["random"] * K, dtype=object)
    verdict[sig & (obs[:, 0] < out["count_expected"])] = "contiguous"
    verdict[sig & (obs[:, 0] > out["count_expected"])] = "fragmented"
    out["verdict"] = verdict
    return out


def _run(edges, problems, lds_limit=None):
    """edges: [(src, dst)] device tensors per edge set; problems: dicts with `e` (edge set), `lab` (index into the label blocks),
    `blocks` shared through problems[0]['blocks'], n, K, L, p0 (-1: explicit labelings), gid, seed, ids (whether the ids and
    sizes of the first labeling are asked for).  One launch; returns (out int64 [sum L, K_max, 4], ids, sizes, status
    [sum L, 2]) on the host and per problem its first node in ids (-1: not asked for).  RuntimeError where a workgroup reached
    its round cap."""
    import torch
    from .stage_ops import TERRITORY_DESC, territory_counts as launch
    blocks = problems[0]["blocks"]
    dev = blocks[0].device
    with torch.cuda.device(dev):
        eoff = np.concatenate([[0], np.cumsum([int(s.shape[0]) for s, _ in edges])]).astype(np.int64)
        loff = np.concatenate([[0], np.cumsum([int(b.numel()) for b in blocks])]).astype(np.int64)
        src = torch.cat([s.to(torch.int32) for s, _ in edges]) if len(edges) > 1 else edges[0][0].to(torch.int32).contiguous()
        dst = torch.cat([d.to(torch.int32) for _, d in edges]) if len(edges) > 1 else edges[0][1].to(torch.int32).contiguous()
        labels = torch.cat([b.reshape(-1) for b in blocks]) if len(blocks) > 1 else blocks[0].reshape(-1).contiguous()
        desc = np.zeros((len(problems), TERRITORY_DESC), dtype=np.int64)
        item = node = 0
        for i, q in enumerate(problems):
            desc[i, :10] = (eoff[q["e"]], q["n"], eoff[q["e"] + 1] - eoff[q["e"]], q["K"], loff[q["lab"]], q["L"], q["p0"],
                            q["gid"], item, np.array(q["seed"] & (2 ** 64 - 1), dtype=np.uint64).astype(np.int64))
            desc[i, 12] = node if q.get("ids") else -1
            item += q["L"]
            node += q["n"] if q.get("ids") else 0
        out, ids, sizes, status = launch(src, dst, labels, desc, max(q["K"] for q in problems), lds_limit=lds_limit)
        out, ids, sizes, status = out.cpu().numpy(), ids.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy()
    if status[:, 0].any():
        bad = int(np.flatnonzero(status[:, 0])[0])
        raise RuntimeError(f"spadot_territory_counts: labeling {bad} of the call reached its round cap after {int(status[bad, 1])} "
                           f"rounds without a fixed point")
    return out, ids, sizes, status, desc[:, 12]


def _edge_pairs(edges):
    pairs, dev = [], None
    for g, e in enumerate(edges):
        pairs.append(edge_pair(e, dev, g))
        dev = pairs[-1][0].device
    return pairs, dev


def territory_counts(edges, labelings, n_clusters=None, lds_limit=None, ids=False):
    """edges[g]: (src, dst) integer device tensors of graph g; labelings[g]: an integer array or tensor [L, n] (or [n]: one
    labeling) of explicit labelings, or a Permuted.  n_clusters[g]: the K of graph g (default: its largest label + 1).
    lds_limit: the LDS bytes a workgroup may use (default 163840): a graph that needs more than that (1024 + 8 n + n rounded up
    to 16 bytes) works in a slab of global scratch, with the same integers.  ids: also the territory id and size of every spot
    under the first labeling of every graph.  One launch for the whole call; returns [g] -> TerritoryCounts.  ValueError before
    any launch; RuntimeError where a workgroup reached its round cap."""
    import torch
    if not edges or len(edges) != len(labelings):
        raise ValueError(f"territory_counts takes one labeling block per graph ({len(edges)} graphs, {len(labelings)} blocks)")
    if n_clusters is not None and len(n_clusters) != len(edges):
        raise ValueError(f"n_clusters holds {len(n_clusters)} cluster counts for {len(edges)} graphs")
    pairs, dev = _edge_pairs(edges)
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
                             p0=spec.first if spec else -1, gid=spec.graph if spec else g, seed=spec.seed if spec else 0,
                             ids=bool(ids)))
    ranges = torch.stack(ranges).cpu().numpy().reshape(-1, 2)
    for g, q in enumerate(problems):
        q["K"] = int(ranges[g, 1]) + 1 if n_clusters is None else int(n_clusters[g])
        _check_range(int(ranges[g, 0]), int(ranges[g, 1]), q["K"], g)
    problems[0]["blocks"] = [b.to(torch.uint8) for b in blocks]
    out, tid, tsz, status, node = _run(pairs, problems, lds_limit)
    outs, item = [], 0
    for g, q in enumerate(problems):
        sl = slice(int(node[g]), int(node[g]) + q["n"])
        outs.append(TerritoryCounts(np.ascontiguousarray(out[item:item + q["L"], :q["K"]]), status[item:item + q["L"], 1].copy(),
                                    tid[sl].copy() if ids else None, tsz[sl].copy() if ids else None))
        item += q["L"]
    return outs


def boundary_spots(src, dst, labels):
    """Per spot whether some edge at it, in either direction, leads to another label: bool on the labels' device."""
    import torch
    s, d = src.long(), dst.long()
    cut = labels[s] != labels[d]
    out = torch.zeros(labels.shape[0], dtype=torch.bool, device=labels.device)
    out[s[cut]] = True
    out[d[cut]] = True
    return out


def territories(edges, labels, n_perms=1000, seed=0, n_clusters=None, alpha=0.05):
    """The territories of every graph with their test (module docstring): edges[g] = (src, dst) device tensors, labels[g] the
    observed labeling (integers, numpy or torch), n_clusters[g] its K (default: largest label + 1).  The observed labelings and
    all n_perms relabelings (0: none) of all graphs go through one call to the library; graph g permutes under (seed, g).
    Returns [g] -> TerritoryResult."""
    import torch
    n_perms = int(n_perms)
    if n_perms < 0:
        raise ValueError(f"n_perms is a number of relabelings, 0 or more (got {n_perms})")
    if not 0 < float(alpha) <= 1:
        raise ValueError(f"alpha is a level in (0, 1] (got {alpha})")
    if not edges or len(edges) != len(labels):
        raise ValueError(f"territories takes one labeling per graph ({len(edges)} graphs, {len(labels)} labelings)")
    if n_clusters is not None and len(n_clusters) != len(edges):
        raise ValueError(f"n_clusters holds {len(n_clusters)} cluster counts for {len(edges)} graphs")
    pairs, dev = _edge_pairs(edges)
    blocks, ranges = [], []
    for g, lab in enumerate(labels):
        block, lo, hi = _label_block(lab, dev, g)
        if block.dim() != 1:
            raise ValueError(f"the labeling of graph {g} must be 1-d (got {tuple(block.shape)})")
        blocks.append(block)
        ranges += [lo, hi]
    ranges = torch.stack(ranges).cpu().numpy().reshape(-1, 2)
    problems, Ks = [], []
    for g, block in enumerate(blocks):
        K = int(ranges[g, 1]) + 1 if n_clusters is None else int(n_clusters[g])
        _check_range(int(ranges[g, 0]), int(ranges[g, 1]), K, g)
        Ks.append(K)
        common = dict(e=g, lab=g, n=int(block.shape[0]), K=K, gid=g, seed=int(seed))
        problems.append(dict(common, L=1, p0=-1, ids=True))          # the observed labeling: the base of the relabelings
        if n_perms:
            problems.append(dict(common, L=n_perms, p0=0))
    problems[0]["blocks"] = [b.to(torch.uint8) for b in blocks]
    sizes = [torch.bincount(b, minlength=K) for b, K in zip(blocks, Ks)]
    border = [boundary_spots(s, d, b) for (s, d), b in zip(pairs, blocks)]
    out, tid, tsz, status, node = _run(pairs, problems)
    res, item, per = [], 0, 2 if n_perms else 1
    for g, K in enumerate(Ks):
        n = problems[per * g]["n"]
        sl = slice(int(node[per * g]), int(node[per * g]) + n)
        perm = np.ascontiguousarray(out[item + 1:item + 1 + n_perms, :K])
        res.append(TerritoryResult(out[item, :K].copy(), perm, sizes[g].cpu().numpy().astype(np.int64), tid[sl].copy(),
                                   tsz[sl].copy(), border[g].cpu().numpy(), int(status[item, 1]), float(alpha)))
        item += 1 + n_perms
    return res


def refine_labels(edges, labels, min_size, n_clusters=None, max_rounds=MAX_ROUNDS):
    """The refinement of the module docstring on one graph: edges = (src, dst) device tensors, labels [n] integers.  One device
    call per round returns the ids and sizes; the vote is torch on the device.  Returns (labels int64 numpy [n], the rounds that
    changed something, the spots whose label differs from the input)."""
    import torch
    s_min, max_rounds = int(min_size), int(max_rounds)
    if s_min < 2:
        raise ValueError(f"refinement takes min_size >= 2 (got {min_size}): every territory holds at least one spot")
    if max_rounds < 0:
        raise ValueError(f"max_rounds is a number of rounds, 0 or more (got {max_rounds})")
    src, dst = edge_pair(edges, None, 0)
    lab0, lo, hi = _label_block(labels, src.device, 0)
    if lab0.dim() != 1:
        raise ValueError(f"the labeling must be 1-d (got {tuple(lab0.shape)})")
    lo, hi = int(lo), int(hi)
    K = hi + 1 if n_clusters is None else int(n_clusters)
    _check_range(lo, hi, K, 0)
    dev, n = src.device, int(lab0.shape[0])
    lab = lab0.long().clone()
    u = torch.cat([src.long(), dst.long()])                          # the edges symmetrised, with multiplicity
    v = torch.cat([dst.long(), src.long()])
    rounds = 0
    while rounds < max_rounds:
        got = territory_counts([(src, dst)], [lab], n_clusters=[K], ids=True)[0]
        tid = torch.as_tensor(got.ids, device=dev).long()
        small = torch.as_tensor(got.sizes, device=dev) < s_min
        keep = small[u] & ~small[v]
        if not bool(keep.any()):
            break
        votes = torch.bincount(tid[u[keep]] * K + lab[v[keep]], minlength=n * K).reshape(n, K)
        # the largest count, ties to the smallest label: count * K + (K - 1 - label) has one largest entry per row
        best = (votes * K + torch.arange(K - 1, -1, -1, device=dev)[None]).argmax(dim=1)
        moves = small & (votes.sum(dim=1) > 0)[tid]
        lab = torch.where(moves, best[tid], lab)                    # all territories decide on the labels from before the round
        rounds += 1
    return lab.cpu().numpy(), rounds, int((lab != lab0.long()).sum())


def territory_table(r):
    """The rows of {prefix}territories_{tp}.csv: one per domain."""
    import pandas as pd
    K = r.counts.shape[0]
    cols = {"domain": np.arange(K), "size": r.sizes, "count": r.counts[:, 0], "largest": r.counts[:, 1],
            "largest_share": r.largest_share, "singletons": r.counts[:, 2], "contiguity": r.contiguity}
    cols.update({name: getattr(r, name) for name in NULL_COLUMNS})
    cols["verdict"] = r.verdict
    return pd.DataFrame(cols, columns=list(TABLE_COLUMNS))


def territories_stage(args):
    """Reads args.domains (the domains.csv of analyze: row, timepoint, kmeans, pixel_x, pixel_y); builds the k-nearest-neighbour
    graph of every time point and runs one territories call.  Writes {prefix}territories_{tp}.csv (TABLE_COLUMNS, one row per
    domain), {prefix}territories_spots.csv (SPOT_COLUMNS, and `refined` when refining; input order), {prefix}territories.npz
    ('{tp}_{matrix}' for MATRICES, plus timepoints, seed, k, n_perms, min_size, alpha and, when refining, '{tp}_refined',
    refine_rounds and refine_moved), with min_size {prefix}refined_domains.csv in the columns of analyze's domains.csv, and, with
    matplotlib, {prefix}{tp}_territories.png.  Returns {'tables', 'results' (per time point), 'spots', 'refined' (labels per row,
    or None), 'timepoints', 'timings'}."""
    import pandas as pd
    from .neighbors import spatial_edges
    from .utils import _analyze_utils
    t_start = time.perf_counter()
    tab = read_domains_table(args, "territories")
    k, n_perms, seed = int(getattr(args, "k", 6)), int(getattr(args, "n_perms", 1000)), int(getattr(args, "seed", 0))
    min_size, alpha = int(getattr(args, "min_size", 0) or 0), float(getattr(args, "alpha", 0.05))
    if k < 1 or not 0 <= n_perms <= MAX_PERMS:
        raise ValueError(f"the territories stage takes k >= 1 and n_perms = 0 .. {MAX_PERMS} (got k = {k}, n_perms = {n_perms})")
    if min_size != 0 and min_size < 2:
        raise ValueError(f"min_size is 0 (no refinement) or at least 2 (got {min_size})")
    if not 0 < alpha <= 1:
        raise ValueError(f"alpha is a level in (0, 1] (got {alpha})")
    out_file = open_output(args, tab.beside)

    import torch
    dev = cuda_device(args, "finds territories")
    tps, masks = tab.tps, tab.masks
    t_read = time.perf_counter()
    edges = [spatial_edges(tab.coords[m], k, dev) for m in masks]
    labs = [torch.as_tensor(tab.labels[m], device=dev) for m in masks]
    torch.cuda.synchronize(dev)
    t_graph = time.perf_counter()
    res = territories(edges, labs, n_perms=n_perms, seed=seed, n_clusters=tab.Ks, alpha=alpha)
    refined, rounds, moved = None, [], []
    if min_size:
        refined = np.empty(tab.n, dtype=np.int64)
        for m, e, lab, K in zip(masks, edges, labs, tab.Ks):
            refined[m], r, c = refine_labels(e, lab, min_size, n_clusters=K)
            rounds.append(r)
            moved.append(c)
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter()

    more = (lambda t, r: {"refined": refined[masks[t]]}) if min_size else None
    tables, arrays = write_timepoints(out_file, "territories", tps, res, lambda t, r: territory_table(r), MATRICES, more=more)
    extra = dict(refine_rounds=np.asarray(rounds, dtype=np.int64), refine_moved=np.asarray(moved, dtype=np.int64)) if min_size else {}
    np.savez(out_file("territories.npz"), timepoints=np.asarray(tps), seed=np.int64(seed), k=np.int64(k), n_perms=np.int64(n_perms),
             min_size=np.int64(min_size), alpha=np.float64(alpha), **extra, **arrays)
    per_spot = {name: np.empty(tab.n, dtype=dt) for name, dt in (("territory", np.int64), ("territory_size", np.int64),
                                                                  ("boundary", bool))}
    for m, r in zip(masks, res):
        for name in per_spot:
            per_spot[name][m] = getattr(r, name)
    cols = {"row": tab.row_ids, "timepoint": tab.tp_all, "kmeans": tab.labels, **per_spot}
    if min_size:
        cols["refined"] = refined
        pd.DataFrame({"row": tab.row_ids, "timepoint": tab.tp_all, "kmeans": refined, "pixel_x": tab.coords[:, 0],
                      "pixel_y": tab.coords[:, 1]}, columns=list(DOMAIN_COLUMNS)).to_csv(out_file("refined_domains.csv"), index=False)
    spots = pd.DataFrame(cols, columns=list(SPOT_COLUMNS) + (["refined"] if min_size else []))
    spots.to_csv(out_file("territories_spots.csv"), index=False)
    mark = max(min_size, 2)                                          # the spots marked in the plot: those of small territories
    plot_timepoints(tps, list(zip(masks, res)), lambda tp, mr: _analyze_utils.plot_territories(
        out_file(f"{tp}_territories.png"), tab.coords[mr[0], 0], tab.coords[mr[0], 1], tab.labels[mr[0]],
        mr[1].territory_size < mark, tp, mark))
    t_end = time.perf_counter()
    pieces = sum(int(r.counts[:, 0].sum()) for r in res)
    tail = f", {int(sum(moved))} spots moved by min_size = {min_size}" if min_size else ""
    print(f"territories: {tab.n} spots of {len(tps)} time points, k = {k}, {pieces} territories, {n_perms} permutations{tail}, "
          f"written to {args.output_dir}", file=sys.stderr)
    return {"tables": tables, "results": dict(zip(tps, res)), "spots": spots, "refined": refined, "timepoints": tps,
            "timings": timings(t_start, t_read, t_dev, t_end, t_graph)}
