"""The centrality stage: how far apart things are, measured along the tissue.  How many spots lie between domain 2 and domain
5, which domain is the middle of the section and which is its rim, how deep inside its domain a spot sits, and which spots are
the centre of the tissue?  (csrc/hops.hip)  This is squidpy's `gr.centrality_scores` (group closeness and group
degree centrality through networkx) on the spatial k-nearest-neighbour graph; the reference has no such stage.  The definition
is restated with numpy and scipy in tests/hops_ref.py.  The average clustering coefficient, squidpy's third score, needs
triangle counting and is NOT computed here.

    hop_sums(edges, labelings)            the integers of many (graph, labeling block or Permuted) problems in ONE launch
    spot_hop_sums(edges, labels)          all-pairs breadth-first search: the source items of many graphs in ONE launch
    centrality(edges, labels)             the observed labeling, the relabelings and (optionally) the source items of all graphs
    centrality_stats(obs, ecc, perm, sizes, n)   the host statistics from the integers
    centrality_stage(args)    the stage.  args: domains ({prefix}domains.csv of analyze), output_dir, prefix (''), k (6), n_perms
                              (200), seed (0), spots (False), device

A problem is the directed edge list i -> j over n spots, as spatial_edges(coords, k) returns it, with a labeling in 0 .. K-1,
1 <= K <= 32.  Direction is ignored; duplicates, edges present in both directions and self loops change nothing.  The distance
d(u, v) is the number of edges of a shortest path; the distance of a spot to a set of spots is the smallest distance to a
member.  Every number below comes from one device primitive: level-synchronous breadth-first search from up to 32 source sets
at once, one bit of a 32-bit mask per set.

Per (labeling, set a, class c) three integers, int64: `reached`, the spots of class c at a distance 1 .. n-1 of set a;
`sumdist`, the sum of those distances; `adjacent`, those at distance 1; per set `ecc`, the largest of its distances (0: it
reaches nothing).  With bit = domain (label items) set a is domain a and the class of a spot is its domain; a domain without
spots gives zeros.  With bit = one spot of a block of 32 (source items) the sets are the single spots and the sums over the
classes are the spot's own closeness and eccentricity.  Permuted labelings are lab[pi_p(i)] with the Feistel relabelings, the
(seed, graph id, p, n) convention and the Permuted spec of neighbors (csrc/feistel_perm.h).

Host statistics, fp64 from the integers, with `sizes` from a bincount.  Per domain a that holds spots (NaN in the others):
    closeness    = (n - size_a) / sum_c sumdist[a][c], 0 where the sum is 0: networkx's group_closeness_centrality (spots the
                   domain does not reach count in the numerator only);
    degree       = sum_c adjacent[a][c] / (n - size_a): networkx's group_degree_centrality; NaN where size_a = n;
    reached_share = sum_c reached[a][c] / (n - size_a): the share of the other spots the domain reaches at all;
    eccentricity = ecc[a] (an integer; 0 for a domain without spots).
Per ordered pair of domains: separation[a][b] = sumdist[a][b] / reached[a][b], the mean number of hops from a spot of b to the
nearest spot of a; NaN on the diagonal and where nothing is reached.  It is not symmetric: a thin domain inside a broad one is
near for the thin one's spots and far for most of the broad one's.
With P >= 1 relabelings: expected, sd (ddof 0) and z of closeness and of separation (z is NaN where sd = 0; the separation of
a pair is NaN under a relabeling that reaches nothing, and so are then its expected, sd and z);
    p_lower = (1 + #{p : closeness_p <= closeness}) / (P + 1),  p_higher = (1 + #{p : closeness_p >= closeness}) / (P + 1),
    padj = Benjamini-Hochberg (markers.bh_adjust) of min(1, 2 min(p_lower, p_higher)) over the domains that hold spots.
With P = 0 the null columns are NaN.  There is no verdict column.
What the null is worth: a label dealt at random over the spots is one or two hops from everything, so under the null every
domain has a closeness near 1 and every pair a separation near 1, and a real, compact domain reads FAR LESS close than chance:
p_lower sits at its floor for almost any real map.  z is the number that compares across domains, time points and k; the
separation matrix itself, in hops, is the finding.

Per spot of the observed labeling: `hops_to_{a}`, the distance to domain a (0 inside it, -1 where it is out of reach), and
`depth`: the smallest hops_to_{b} over the domains b other than its own that it reaches, -1 if there is none.  Depth 1 is
exactly the `boundary` of territories; a larger depth says how far inside its domain the spot sits.
With spots=True, from the source items: reached and sumdist of every spot (also by class), its `eccentricity` (within its
connected piece), `closeness` = reached / sumdist (0 for an isolated spot), `closeness_wf` = closeness * reached / (n - 1),
networkx's closeness_centrality with and without wf_improved; per graph over the spots that reach the most others (the largest
connected piece): the diameter and the radius (the largest and the smallest eccentricity) and the centre (the spots of the
smallest eccentricity); per domain the mean closeness_wf of its spots.

The device searches; the host validates, takes the statistics and writes the files.  Limits: those of neighbors (1 <= K <= 32,
at most 2147483647 spots and edges per graph and items per call)."""
import sys
import time

import numpy as np

from .neighbors import Permuted, _check_range, _label_block
from .territories import _edge_pairs
from .utils._stage_utils import cuda_device, open_output, plot_timepoints, read_domains_table, timings, write_timepoints

INTEGERS = ("reached", "sumdist", "adjacent")
NULL_COLUMNS = ("closeness_expected", "closeness_sd", "closeness_z", "p_lower", "p_higher", "padj")
PAIR_NULL = ("separation_expected", "separation_sd", "separation_z")
TABLE_COLUMNS = ("domain", "size", "closeness", "degree", "eccentricity", "reached_share") + NULL_COLUMNS
SPOT_TABLE_COLUMN = "spot_closeness"                # with --spots, after TABLE_COLUMNS
PAIR_COLUMNS = ("domain", "other", "reached", "sumdist", "adjacent", "separation") + PAIR_NULL
SPOT_COLUMNS = ("row", "timepoint", "kmeans", "depth")          # then hops_to_0 .. hops_to_{K-1}; with --spots SPOT_EXTRA
SPOT_EXTRA = ("reached", "closeness", "closeness_wf", "eccentricity", "centre")
MATRICES = ("sizes", "sums", "ecc", "perm_sums", "closeness", "degree", "eccentricity", "reached_share",
            "separation") + NULL_COLUMNS + PAIR_NULL + ("hops", "depth")
SPOT_MATRICES = ("spot_reached", "spot_sumdist", "spot_reached_by", "spot_sumdist_by", "spot_eccentricity", "spot_closeness",
                 "spot_closeness_wf", "diameter", "radius", "centre", "domain_spot_closeness")
MAX_PERMS = 9999
SETS = 32


class HopSums:
    """One problem of hop_sums: sums int64 [L, K, K, 3] (INTEGERS per labeling, set and class), ecc int32 [L, K], rounds int32
    [L] (the rounds the workgroup ran: the largest distance + 1) and, where asked for, hops int32 [n, K] of the first
    labeling: per spot and domain the distance (0 inside, -1 out of reach)."""

    def __init__(self, sums, ecc, rounds, hops=None):
        self.sums, self.ecc, self.rounds, self.hops = sums, ecc, rounds, hops


class SpotHops:
    """One graph of spot_hop_sums: per spot reached and sumdist int64 [n], reached_by and sumdist_by int64 [n, K] (by the class
    of the spot reached), degree int64 [n] (the spots at distance 1), ecc int32 [n]; rounds int32 [ceil(n / 32)]."""

    def __init__(self, reached_by, sumdist_by, degree, ecc, rounds):
        self.reached_by, self.sumdist_by, self.degree, self.ecc, self.rounds = reached_by, sumdist_by, degree, ecc, rounds
        self.reached, self.sumdist = reached_by.sum(axis=1), sumdist_by.sum(axis=1)


class CentralityResult:
    """One graph: n, sizes int64 [K], sums int64 [K, K, 3], ecc int32 [K], perm_sums int64 [P, K, K, 3], hops int32 [n, K],
    depth int32 [n], rounds (of the observed labeling), the fp64 statistics of the module docstring ([K] and [K, K]) and, with
    spots=True, `spots` (a SpotHops) and SPOT_MATRICES."""

    def __init__(self, n, sums, ecc, perm_sums, sizes, hops, rounds, labels, spots=None):
        self.n, self.sums, self.ecc, self.perm_sums, self.sizes, self.hops, self.rounds = n, sums, ecc, perm_sums, sizes, hops, rounds
        self.spots, self.depth = spots, spot_depth(hops, labels)
        for name, v in centrality_stats(sums, ecc, perm_sums, sizes, n).items():
            setattr(self, name, v)
        if spots is not None:
            for name, v in spot_stats(spots, labels, sizes.shape[0]).items():
                setattr(self, name, v)


def _ratio(num, den):
    """num / den in fp64 where den != 0, NaN elsewhere."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def _closeness(sums, sizes, n):
    """[.., K]: (n - size_a) / sum_c sumdist[a][c], 0 where the sum is 0, NaN for a domain without spots."""
    total = sums[..., 1].sum(axis=-1)
    out = _ratio(n - sizes, total)
    out[total == 0] = 0.0
    out[np.broadcast_to(sizes == 0, out.shape)] = np.nan
    return out


def _separation(sums):
    """[.., K, K]: sumdist / reached, NaN on the diagonal and where nothing is reached."""
    out = _ratio(sums[..., 1], sums[..., 0])
    K = out.shape[-1]
    out[..., np.arange(K), np.arange(K)] = np.nan
    return out


def centrality_stats(obs, ecc, perm, sizes, n):
    """The host statistics of one graph from its integers (module docstring): obs int [K, K, 3], ecc int [K], perm int
    [P, K, K, 3] (P may be 0), sizes [K], n spots.  A dict of fp64 arrays [K] or [K, K] and `eccentricity`, int64 [K]."""
    from .markers import bh_adjust
    obs = np.asarray(obs, dtype=np.int64)
    K = obs.shape[0]
    perm = np.asarray(perm, dtype=np.int64).reshape(-1, K, K, 3)
    sizes = np.asarray(sizes, dtype=np.int64)
    n, P = int(n), perm.shape[0]
    has = sizes > 0
    rest = np.where(has, n - sizes, 0)                                  # 0 where size_a = n: NaN degree and reached_share
    out = dict(closeness=_closeness(obs, sizes, n), degree=np.where(has, _ratio(obs[:, :, 2].sum(axis=1), rest), np.nan),
               eccentricity=np.asarray(ecc, dtype=np.int64).copy(),
               reached_share=np.where(has, _ratio(obs[:, :, 0].sum(axis=1), rest), np.nan), separation=_separation(obs))
    if P == 0:
        out.update({name: np.full(K, np.nan) for name in NULL_COLUMNS})
        out.update({name: np.full((K, K), np.nan) for name in PAIR_NULL})
        return out
    for name, o, p in (("closeness", out["closeness"], _closeness(perm, sizes, n)),
                       ("separation", out["separation"], _separation(perm))):
        expected, sd = p.mean(axis=0, dtype=np.float64), p.std(axis=0, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            z = np.where(sd > 0, (o - expected) / sd, np.nan)
        out[name + "_expected"], out[name + "_sd"], out[name + "_z"] = expected, sd, z
        if name == "closeness":
            with np.errstate(invalid="ignore"):
                lower, higher = (p <= o[None]).sum(axis=0), (p >= o[None]).sum(axis=0)
            out["p_lower"] = np.where(has, (1.0 + lower) / (P + 1.0), np.nan)
            out["p_higher"] = np.where(has, (1.0 + higher) / (P + 1.0), np.nan)
    padj = np.full(K, np.nan)                                           # a domain without spots is left out of the BH family
    if has.any():
        padj[has] = bh_adjust(np.minimum(1.0, 2.0 * np.minimum(out["p_lower"], out["p_higher"]))[has])
    out["padj"] = padj
    return out


def spot_depth(hops, labels):
    """int32 [n]: the smallest hops[i][b] >= 0 over the domains b other than the spot's own, -1 if there is none."""
    hops, labels = np.asarray(hops), np.asarray(labels, dtype=np.int64)
    n, K = hops.shape
    far = np.iinfo(np.int32).max
    h = np.where(hops < 0, far, hops).astype(np.int64)
    h[np.arange(n), labels] = far
    depth = h.min(axis=1) if K else np.full(n, far)
    return np.where(depth == far, -1, depth).astype(np.int32)


def spot_stats(spots, labels, K):
    """The per-spot numbers of the module docstring from a SpotHops: a dict of SPOT_MATRICES."""
    n = spots.reached.shape[0]
    closeness = _ratio(spots.reached, spots.sumdist)
    closeness[spots.sumdist == 0] = 0.0
    wf = closeness * (spots.reached / (n - 1.0)) if n > 1 else np.zeros(n)
    ecc = spots.ecc.astype(np.int64)
    main = spots.reached == spots.reached.max()                         # the largest connected piece (all of equal size)
    radius = int(ecc[main].min())
    labels = np.asarray(labels, dtype=np.int64)
    by = _ratio(np.bincount(labels, weights=wf, minlength=K), np.bincount(labels, minlength=K))
    return dict(spot_reached=spots.reached, spot_sumdist=spots.sumdist, spot_reached_by=spots.reached_by,
                spot_sumdist_by=spots.sumdist_by, spot_eccentricity=ecc, spot_closeness=closeness, spot_closeness_wf=wf,
                diameter=np.int64(ecc[main].max()), radius=np.int64(radius), centre=np.flatnonzero(main & (ecc == radius)),
                domain_spot_closeness=by)


def _run(edges, problems, lds_limit=None, status=None):
    """edges: [(src, dst)] device tensors per edge set; problems: dicts with `e` (edge set), `lab` (index into the label blocks),
    `blocks` shared through problems[0]['blocks'], n, K, L, p0 (-1: explicit labelings), gid, seed, hops (whether the distances
    of the first labeling are asked for) and kind (1: source items).  One launch; returns (out int64 [sum L, K_max, K_max, 3],
    ecc, hops, status [sum L, 2]) on the host and per problem its first int in hops (-1: not asked for).  RuntimeError where a
    workgroup reached its round cap.  status: a status array to judge in place of a launch (the cap's host path alone)."""
    if status is None:
        import torch
        from .stage_ops import HOP_DESC, HOP_SETS, hop_sums as launch
        blocks = problems[0]["blocks"]
        dev = blocks[0].device
        with torch.cuda.device(dev):
            eoff = np.concatenate([[0], np.cumsum([int(s.shape[0]) for s, _ in edges])]).astype(np.int64)
            loff = np.concatenate([[0], np.cumsum([int(b.numel()) for b in blocks])]).astype(np.int64)
            src = torch.cat([s.to(torch.int32) for s, _ in edges]) if len(edges) > 1 else edges[0][0].to(torch.int32).contiguous()
            dst = torch.cat([d.to(torch.int32) for _, d in edges]) if len(edges) > 1 else edges[0][1].to(torch.int32).contiguous()
            labels = torch.cat([b.reshape(-1) for b in blocks]) if len(blocks) > 1 else blocks[0].reshape(-1).contiguous()
            desc = np.zeros((len(problems), HOP_DESC), dtype=np.int64)
            item = node = 0
            for i, q in enumerate(problems):
                desc[i, :10] = (eoff[q["e"]], q["n"], eoff[q["e"] + 1] - eoff[q["e"]], q["K"], loff[q["lab"]], q["L"], q["p0"],
                                q["gid"], item, np.array(q["seed"] & (2 ** 64 - 1), dtype=np.uint64).astype(np.int64))
                desc[i, 12] = node if q.get("hops") else -1
                desc[i, 14] = int(q.get("kind", 0))
                item += q["L"]
                node += q["n"] * q["K"] if q.get("hops") else 0
            K_max = HOP_SETS if any(q.get("kind") for q in problems) else max(q["K"] for q in problems)
            out, ecc, hops, status = launch(src, dst, labels, desc, K_max, lds_limit=lds_limit)
            out, ecc, hops, status = out.cpu().numpy(), ecc.cpu().numpy(), hops.cpu().numpy(), status.cpu().numpy()
        first = desc[:, 12]
    else:
        out = ecc = hops = first = None
        status = np.asarray(status)
    if status[:, 0].any():
        bad = int(np.flatnonzero(status[:, 0])[0])
        raise RuntimeError(f"spadot_hop_sums: item {bad} of the call reached its round cap after {int(status[bad, 1])} rounds with "
                           f"spots still being reached")
    return out, ecc, hops, status, first


def _observed(labels, dev, n_clusters):
    """The 1-d labelings of the graphs on the device with their K: (blocks, Ks); one host round trip."""
    import torch
    blocks, ranges = [], []
    for g, lab in enumerate(labels):
        block, lo, hi = _label_block(lab, dev, g)
        if block.dim() != 1:
            raise ValueError(f"the labeling of graph {g} must be 1-d (got {tuple(block.shape)})")
        blocks.append(block)
        ranges += [lo, hi]
    ranges = torch.stack(ranges).cpu().numpy().reshape(-1, 2)
    Ks = []
    for g in range(len(blocks)):
        K = int(ranges[g, 1]) + 1 if n_clusters is None else int(n_clusters[g])
        _check_range(int(ranges[g, 0]), int(ranges[g, 1]), K, g)
        Ks.append(K)
    return blocks, Ks


def _graphs_and_labelings(name, edges, labels, n_clusters, what="labeling"):
    if not edges or len(edges) != len(labels):
        raise ValueError(f"{name} takes one {what} per graph ({len(edges)} graphs, {len(labels)} {what}s)")
    if n_clusters is not None and len(n_clusters) != len(edges):
        raise ValueError(f"n_clusters holds {len(n_clusters)} cluster counts for {len(edges)} graphs")


def hop_sums(edges, labelings, n_clusters=None, lds_limit=None, hops=False):
    """edges[g]: (src, dst) integer device tensors of graph g; labelings[g]: an integer array or tensor [L, n] (or [n]: one
    labeling) of explicit labelings, or a Permuted.  n_clusters[g]: the K of graph g (default: its largest label + 1).
    lds_limit: the LDS bytes a workgroup may use (default 163840): a graph that needs more than that (stage_ops.hop_lds_bytes:
    16640 + 8 n + n rounded up to 16 bytes) works in a slab of global scratch, with the same integers.  hops: also the distance
    of every spot to every domain under the first labeling of every graph.  One launch for the whole call; returns [g] ->
    HopSums.  ValueError before any launch; RuntimeError where a workgroup reached its round cap."""
    import torch
    _graphs_and_labelings("hop_sums", edges, labelings, n_clusters, "labeling block")
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
                             hops=bool(hops)))
    ranges = torch.stack(ranges).cpu().numpy().reshape(-1, 2)
    for g, q in enumerate(problems):
        q["K"] = int(ranges[g, 1]) + 1 if n_clusters is None else int(n_clusters[g])
        _check_range(int(ranges[g, 0]), int(ranges[g, 1]), q["K"], g)
    problems[0]["blocks"] = [b.to(torch.uint8) for b in blocks]
    out, ecc, dist, status, first = _run(pairs, problems, lds_limit)
    outs, item = [], 0
    for g, q in enumerate(problems):
        K, sl = q["K"], slice(item, item + q["L"])
        h = dist[int(first[g]):int(first[g]) + q["n"] * K].reshape(q["n"], K).copy() if hops else None
        outs.append(HopSums(np.ascontiguousarray(out[sl, :K, :K]), np.ascontiguousarray(ecc[sl, :K]), status[sl, 1].copy(), h))
        item += q["L"]
    return outs


def _spot_hops(out, ecc, status, item, n, K):
    """The SpotHops of a graph whose ceil(n / 32) source items start at `item`."""
    I = (n + SETS - 1) // SETS
    per = out[item:item + I].reshape(I * SETS, SETS, 3)[:n, :K]
    return SpotHops(np.ascontiguousarray(per[:, :, 0]), np.ascontiguousarray(per[:, :, 1]), per[:, :, 2].sum(axis=1),
                    ecc[item:item + I].reshape(-1)[:n].copy(), status[item:item + I, 1].copy())


def spot_hop_sums(edges, labels, n_clusters=None, lds_limit=None):
    """All-pairs breadth-first search: edges[g] as for hop_sums, labels[g] the one labeling [n] of graph g (the classes by which
    the sums are split).  Every graph has ceil(n / 32) source items of 32 spots each; all of them go through one launch.
    Returns [g] -> SpotHops.  ValueError before any launch; RuntimeError where a workgroup reached its round cap."""
    import torch
    _graphs_and_labelings("spot_hop_sums", edges, labels, n_clusters)
    pairs, dev = _edge_pairs(edges)
    blocks, Ks = _observed(labels, dev, n_clusters)
    problems = [dict(e=g, lab=g, n=int(b.shape[0]), K=K, L=(int(b.shape[0]) + SETS - 1) // SETS, p0=-1, gid=g, seed=0, kind=1)
                for g, (b, K) in enumerate(zip(blocks, Ks))]
    problems[0]["blocks"] = [b.to(torch.uint8) for b in blocks]
    out, ecc, _, status, _ = _run(pairs, problems, lds_limit)
    res, item = [], 0
    for q in problems:
        res.append(_spot_hops(out, ecc, status, item, q["n"], q["K"]))
        item += q["L"]
    return res


def centrality(edges, labels, n_perms=200, seed=0, n_clusters=None, spots=False):
    """The centrality of every graph with its null (module docstring): edges[g] = (src, dst) device tensors, labels[g] the
    observed labeling (integers, numpy or torch), n_clusters[g] its K (default: largest label + 1).  The observed labelings and
    all n_perms relabelings (0: none) of all graphs go through one launch; graph g permutes under (seed, g).  spots: also the
    source items of all graphs, in a second launch (its sets are the 32 spots of a block, so its tables are 32 wide).
    Returns [g] -> CentralityResult."""
    import torch
    n_perms = int(n_perms)
    if n_perms < 0:
        raise ValueError(f"n_perms is a number of relabelings, 0 or more (got {n_perms})")
    _graphs_and_labelings("centrality", edges, labels, n_clusters)
    pairs, dev = _edge_pairs(edges)
    blocks, Ks = _observed(labels, dev, n_clusters)
    problems = []
    for g, (block, K) in enumerate(zip(blocks, Ks)):
        common = dict(e=g, lab=g, n=int(block.shape[0]), K=K, gid=g, seed=int(seed))
        problems.append(dict(common, L=1, p0=-1, hops=True))          # the observed labeling: the base of the relabelings
        if n_perms:
            problems.append(dict(common, L=n_perms, p0=0))
    problems[0]["blocks"] = [b.to(torch.uint8) for b in blocks]
    sizes = [torch.bincount(b, minlength=K) for b, K in zip(blocks, Ks)]
    out, ecc, dist, status, first = _run(pairs, problems)
    per_spot = spot_hop_sums(pairs, blocks, n_clusters=Ks) if spots else [None] * len(Ks)
    res, item, per = [], 0, 2 if n_perms else 1
    for g, K in enumerate(Ks):
        n, f = problems[per * g]["n"], int(first[per * g])
        lab = blocks[g].cpu().numpy()
        perm = np.ascontiguousarray(out[item + 1:item + 1 + n_perms, :K, :K])
        res.append(CentralityResult(n, out[item, :K, :K].copy(), ecc[item, :K].copy(), perm, sizes[g].cpu().numpy().astype(np.int64),
                                    dist[f:f + n * K].reshape(n, K).copy(), int(status[item, 1]), lab, per_spot[g]))
        item += 1 + n_perms
    return res


def centrality_table(r):
    """The rows of {prefix}centrality_{tp}.csv: one per domain."""
    import pandas as pd
    K = r.sizes.shape[0]
    cols = {"domain": np.arange(K), "size": r.sizes}
    cols.update({name: getattr(r, name) for name in TABLE_COLUMNS[2:]})
    names = list(TABLE_COLUMNS)
    if r.spots is not None:
        cols[SPOT_TABLE_COLUMN] = r.domain_spot_closeness
        names.append(SPOT_TABLE_COLUMN)
    return pd.DataFrame(cols, columns=names)


def pair_table(r):
    """The rows of {prefix}centrality_pairs_{tp}.csv: one per ordered pair (domain = the set a, other = the class b)."""
    import pandas as pd
    K = r.sizes.shape[0]
    a, b = (v.reshape(-1) for v in np.meshgrid(np.arange(K), np.arange(K), indexing="ij"))
    cols = {"domain": a, "other": b, "reached": r.sums[:, :, 0].reshape(-1), "sumdist": r.sums[:, :, 1].reshape(-1),
            "adjacent": r.sums[:, :, 2].reshape(-1), "separation": r.separation.reshape(-1)}
    cols.update({name: getattr(r, name).reshape(-1) for name in PAIR_NULL})
    return pd.DataFrame(cols, columns=list(PAIR_COLUMNS))


def centrality_stage(args):
    """Reads args.domains (the domains.csv of analyze, or the refined_domains.csv of territories: row, timepoint, kmeans,
    pixel_x, pixel_y); builds the k-nearest-neighbour graph of every time point and runs one centrality call.  Writes
    {prefix}centrality_{tp}.csv (TABLE_COLUMNS, with --spots also spot_closeness; one row per domain),
    {prefix}centrality_pairs_{tp}.csv (PAIR_COLUMNS, one row per ordered pair), {prefix}centrality_spots.csv (SPOT_COLUMNS,
    hops_to_0 .. hops_to_{K-1} with K the largest of the time points, -1 where a time point has no such domain, and with
    --spots SPOT_EXTRA; input order), {prefix}centrality.npz ('{tp}_{matrix}' for MATRICES, with --spots SPOT_MATRICES, plus
    timepoints, seed, k, n_perms, spots) and, with matplotlib, {prefix}{tp}_centrality.png: the spots coloured by depth.
    Returns {'tables', 'pairs', 'results' (per time point), 'spots', 'timepoints', 'timings'}."""
    import pandas as pd
    from .neighbors import spatial_edges
    from .utils import _analyze_utils
    t_start = time.perf_counter()
    tab = read_domains_table(args, "centrality")
    k, n_perms, seed = int(getattr(args, "k", 6)), int(getattr(args, "n_perms", 200)), int(getattr(args, "seed", 0))
    with_spots = bool(getattr(args, "spots", False))
    if k < 1 or not 0 <= n_perms <= MAX_PERMS:
        raise ValueError(f"the centrality stage takes k >= 1 and n_perms = 0 .. {MAX_PERMS} (got k = {k}, n_perms = {n_perms})")
    out_file = open_output(args, tab.beside)

    import torch
    dev = cuda_device(args, "measures hop distances")
    tps, masks = tab.tps, tab.masks
    t_read = time.perf_counter()
    edges = [spatial_edges(tab.coords[m], k, dev) for m in masks]
    labs = [torch.as_tensor(tab.labels[m], device=dev) for m in masks]
    torch.cuda.synchronize(dev)
    t_graph = time.perf_counter()
    res = centrality(edges, labs, n_perms=n_perms, seed=seed, n_clusters=tab.Ks, spots=with_spots)
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter()

    fields = MATRICES + (SPOT_MATRICES if with_spots else ())
    tables, arrays = write_timepoints(out_file, "centrality", tps, res, lambda t, r: centrality_table(r), fields)
    pairs = {}
    for tp, r in zip(tps, res):
        pairs[tp] = pair_table(r)
        pairs[tp].to_csv(out_file(f"centrality_pairs_{tp}.csv"), index=False)
    np.savez(out_file("centrality.npz"), timepoints=np.asarray(tps), seed=np.int64(seed), k=np.int64(k), n_perms=np.int64(n_perms),
             spots=np.bool_(with_spots), **arrays)
    K_all = max(tab.Ks)
    cols = {"row": tab.row_ids, "timepoint": tab.tp_all, "kmeans": tab.labels, "depth": np.empty(tab.n, dtype=np.int64)}
    hops = np.full((tab.n, K_all), -1, dtype=np.int64)
    extra = {"reached": np.empty(tab.n, dtype=np.int64), "closeness": np.empty(tab.n), "closeness_wf": np.empty(tab.n),
             "eccentricity": np.empty(tab.n, dtype=np.int64), "centre": np.zeros(tab.n, dtype=bool)} if with_spots else {}
    for m, r in zip(masks, res):
        rows = np.flatnonzero(m)
        cols["depth"][rows] = r.depth
        hops[rows[:, None], np.arange(r.hops.shape[1])[None]] = r.hops
        if with_spots:
            for name, v in (("reached", r.spot_reached), ("closeness", r.spot_closeness), ("closeness_wf", r.spot_closeness_wf),
                            ("eccentricity", r.spot_eccentricity)):
                extra[name][rows] = v
            extra["centre"][rows[r.centre]] = True
    cols.update({f"hops_to_{a}": hops[:, a] for a in range(K_all)})
    cols.update(extra)
    spots = pd.DataFrame(cols)
    spots.to_csv(out_file("centrality_spots.csv"), index=False)
    plot_timepoints(tps, list(zip(masks, res)), lambda tp, mr: _analyze_utils.plot_depth(
        out_file(f"{tp}_centrality.png"), tab.coords[mr[0], 0], tab.coords[mr[0], 1], mr[1].depth, tp))
    t_end = time.perf_counter()
    tail = ", per-spot closeness and eccentricity" if with_spots else ""
    print(f"centrality: {tab.n} spots of {len(tps)} time points, k = {k}, {n_perms} permutations{tail}, written to "
          f"{args.output_dir}", file=sys.stderr)
    return {"tables": tables, "pairs": pairs, "results": dict(zip(tps, res)), "spots": spots, "timepoints": tps,
            "timings": timings(t_start, t_read, t_dev, t_end, t_graph)}
