"""What the stages that count pairs of spots by distance share on the host: cooccurrence (pairs between two domains, with its
random-labelling null) and ripley (pairs, nearest neighbours and empty space inside one domain) take the same spots ordered by
(label, index), the same ladder of radii compared as squares formed in fp64, the same limits and the same global envelope test
(DESIGN 7i-0).  Every rule is written here once; csrc/pair_count.h is the device side of the same family.

    sorted_problems(coords, labels, n_clusters)    the refusals about spots and labelings, and the layout the device reads
    default_radii(coords, bins), ladder(r_max, bins)      the stage's radii of one time point
    thresholds(name, P, radii, radii_sq)           the squared thresholds of every problem of a call, refused or returned
    counted(coords, labels, radii, bins, count)    what a stage's call does around its counting: radii, counts, domain sizes
    mad_p(T, axis)                                 p_global of the maximum-absolute-deviation envelope test over 1 + S curves

The squared distance that the thresholds are compared with is d2 = fl(fl(dx dx) + fl(dy dy)): five rounded fp64 operations and no
fused multiply-add (pc_d2 of csrc/pair_count.h; restated in tests/cooccur_ref.py)."""
import numpy as np

MAX_CLUSTERS = 32
MAX_BINS = 64
MAX_SPOTS = 2147483391
MAX_PROBLEMS = 65535
NO_CPU = "spadot_amd counts co-occurrences on the MI355X only ({}); there is no CPU path"


def _bounding_box(xy):
    """(min x, max x, min y, max y) of an [n, 2] array or tensor as Python floats."""
    if hasattr(xy, "is_cuda"):
        import torch
        if xy.dim() != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
            raise ValueError(f"coords must be an [n, 2] array of at least one spot (got {tuple(xy.shape)})")
        lo, hi = torch.aminmax(xy.to(torch.float64), dim=0)
        lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    else:
        xy = np.asarray(xy, dtype=np.float64)
        if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
            raise ValueError(f"coords must be an [n, 2] array of at least one spot (got {xy.shape})")
        lo, hi = xy.min(axis=0), xy.max(axis=0)
    return float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1])


def ladder(r_max, bins):
    """The radii r_max * (1 .. bins) / bins."""
    bins, r_max = int(bins), float(r_max)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"the co-occurrence takes 1 to {MAX_BINS} radii (got bins = {bins})")
    if not np.isfinite(r_max) or r_max <= 0:
        raise ValueError(f"the largest radius must be finite and above 0 (got {r_max})")
    return r_max * np.arange(1, bins + 1) / bins


def default_radii(coords, bins=50):
    """The stage's radii of one time point: r_max = 0.25 * hypot(max x - min x, max y - min y), radii = r_max * (1 .. bins) /
    bins.  ValueError where the spots all coincide (or are not finite)."""
    x0, x1, y0, y1 = _bounding_box(coords)
    r_max = 0.25 * np.hypot(x1 - x0, y1 - y0)
    if not np.isfinite(r_max):
        raise ValueError("the coordinates must be finite")
    if r_max <= 0:
        raise ValueError("the spots all coincide: there is no distance to bin (give radii)")
    return ladder(r_max, bins)


def _squares(radii, g):
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if not 1 <= r.shape[0] <= MAX_BINS:
        raise ValueError(f"problem {g} has {r.shape[0]} radii: the device takes 1 to {MAX_BINS}")
    if not np.all(np.isfinite(r)) or np.any(r < 0) or np.any(np.diff(r) <= 0):
        raise ValueError(f"the radii of problem {g} must be finite, >= 0 and strictly increasing")
    return r * r


def thresholds(name, P, radii, radii_sq, labelings=None):
    """[g] -> the fp64 squared thresholds of the P problems of a call of `name`, from exactly one of radii (squared here: r * r)
    and radii_sq; labelings: the number of labelings the call was given (default P).  ValueError for both or neither, for
    anything but one labeling and one set per problem, for more than 65535 problems, and for a set that does not hold 1 to 64
    finite values >= 0 in strictly increasing order."""
    if (radii is None) == (radii_sq is None):
        raise ValueError(f"{name} takes exactly one of radii and radii_sq")
    given = radii if radii is not None else radii_sq
    labelings = P if labelings is None else labelings
    if P < 1 or labelings != P or len(given) != P:
        raise ValueError(f"{name} takes one labeling and one set of radii per problem ({P} problems, {labelings} "
                         f"labelings, {len(given)} sets of radii)")
    if P > MAX_PROBLEMS:
        raise ValueError(f"the call holds {P} problems: the device takes at most {MAX_PROBLEMS} per call")
    r2 = []
    for g, r in enumerate(given):
        t = _squares(r, g) if radii is not None else np.asarray(r, dtype=np.float64).reshape(-1)
        r2.append(t)                                     # two radii that differ may still have one square: checked as squares too
        if not 1 <= t.shape[0] <= MAX_BINS:
            raise ValueError(f"problem {g} has {t.shape[0]} thresholds: the device takes 1 to {MAX_BINS}")
        if not np.all(np.isfinite(t)) or np.any(t < 0) or np.any(np.diff(t) <= 0):
            raise ValueError(f"the squared thresholds of problem {g} must be finite, >= 0 and strictly increasing")
    return r2


def sorted_problems(coords, labels, n_clusters=None, no_cpu=NO_CPU):
    """What the stages that count by distance refuse about the spots and the labelings of a call, before any launch, and the
    layout they hand to the device.  Returns (the device, xy fp64 [sum n, 2] with every problem's spots ordered by (label,
    index), [g] -> K, int64 [P, 32] domain sizes); one host round trip."""
    import torch
    P = len(coords)
    if n_clusters is not None and len(n_clusters) != P:
        raise ValueError(f"n_clusters holds {len(n_clusters)} cluster counts for {P} problems")
    dev, xs, labs = None, [], []
    for g, (xy, lab) in enumerate(zip(coords, labels)):
        if not isinstance(xy, torch.Tensor) or not xy.is_cuda:
            raise RuntimeError(no_cpu.format("the coordinates of problem %d are not a device tensor" % g))
        if xy.dim() != 2 or xy.shape[1] != 2 or xy.shape[0] < 1 or not xy.dtype.is_floating_point:
            raise ValueError(f"the coordinates of problem {g} must form a floating-point [n, 2] block of at least one spot "
                             f"(got {tuple(xy.shape)} {xy.dtype})")
        if dev is not None and xy.device != dev:
            raise ValueError("all problems of a call lie on one device")
        dev = xy.device
        if xy.shape[0] > MAX_SPOTS:
            raise ValueError(f"problem {g} has {xy.shape[0]} spots: the device takes at most {MAX_SPOTS} per problem")
        lab = lab if isinstance(lab, torch.Tensor) else torch.as_tensor(np.asarray(lab))
        if lab.dtype.is_floating_point or lab.dtype == torch.bool or lab.dtype.is_complex:
            raise ValueError(f"labels must be integers (problem {g}: {lab.dtype})")
        if lab.dim() != 1 or lab.shape[0] != xy.shape[0]:
            raise ValueError(f"problem {g} has {xy.shape[0]} spots and a labeling of shape {tuple(lab.shape)}")
        xs.append(xy.to(torch.float64))
        labs.append(lab.to(dev).long())
    with torch.cuda.device(dev):
        stats = []
        for xy, lab in zip(xs, labs):
            lo, hi = torch.aminmax(lab)
            hist = torch.bincount(lab.clamp(0, MAX_CLUSTERS), minlength=MAX_CLUSTERS + 1)[:MAX_CLUSTERS]
            stats.append(torch.cat([torch.stack([lo, hi, torch.isfinite(xy).all().long()]), hist]))
        stats = torch.stack(stats).cpu().numpy()                       # the one host round trip ahead of the launch
        Ks = []
        for g in range(P):
            lo, hi, finite = (int(v) for v in stats[g, :3])
            K = hi + 1 if n_clusters is None else int(n_clusters[g])
            if not 1 <= K <= MAX_CLUSTERS:
                raise ValueError(f"problem {g} has {K} label values: the device counts 1 to {MAX_CLUSTERS} domains")
            if lo < 0 or hi >= K:
                raise ValueError(f"problem {g} holds labels {lo} .. {hi}: labels must lie in 0 .. {K - 1}")
            if not finite:
                raise ValueError(f"problem {g} holds coordinates that are not finite")
            Ks.append(K)
        # the spots of every problem by (label, index): a stable sort of the labels
        xy = torch.cat([x[torch.sort(lab, stable=True)[1]] for x, lab in zip(xs, labs)]).contiguous()
    return dev, xy, Ks, stats[:, 3:]


def counted(coords, labels, radii, bins, count, k_axis=0, no_cpu=NO_CPU):
    """What the call of a stage does around its counting: refuses coordinates that are not device tensors, takes
    default_radii(coords[g], bins) where radii is None, counts (count(radii) -> [g] -> the integers of problem g, K along
    k_axis) and takes the domain sizes by bincount.  Returns [g] -> (integers, radii fp64 [B], sizes int64 [K])."""
    import torch
    for g, xy in enumerate(coords):
        if not isinstance(xy, torch.Tensor) or not xy.is_cuda:
            raise RuntimeError(no_cpu.format("the coordinates of problem %d are not a device tensor" % g))
    if radii is None:
        radii = [default_radii(xy, bins) for xy in coords]
    radii = [np.asarray(r, dtype=np.float64).reshape(-1) for r in radii]
    out = []
    for g, N in enumerate(count(radii)):
        lab = labels[g].cpu().numpy() if isinstance(labels[g], torch.Tensor) else np.asarray(labels[g])
        out.append((N, radii[g], np.bincount(lab, minlength=N.shape[k_axis]).astype(np.int64)))
    return out


def mad_p(T, axis=0):
    """p_global of the global envelope (maximum absolute deviation) test over the 1 + S curves of T, which lie along `axis` with
    the radii along the last: u_i = max_t |(S + 1) x_i(t) - sum_k x_k(t)|, p = #{i : u_i >= u_0} / (S + 1).  Integers are compared
    exactly: in int64 where (S + 1) max |T| cannot wrap, with Python integers otherwise; anything else in fp64."""
    T = np.asarray(T)
    axis, n = axis % T.ndim, T.shape[axis]
    if T.dtype.kind in "iub":
        T = T.astype(np.int64)
        if T.size and int(np.abs(T).max()) * n >= 2 ** 62:
            T = T.astype(object)
    dev = np.abs(n * T - T.sum(axis=axis, keepdims=True)).max(axis=-1)
    return np.asarray((dev >= np.take(dev, [0], axis=axis)).sum(axis=axis), dtype=np.float64) / n
