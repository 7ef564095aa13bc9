"""Synthetic spatio-temporal transcriptomics of the shape SURVEY.md 8(d) prescribes (the reference's
.h5ad inputs are not redistributable and there is no network): per time point a jittered sqrt(N) x
sqrt(N) grid of spots, 10 spatial domains (k-means of the coordinates), expression = domain one-hot @
W + 0.5 * noise, z-scored per gene (what sc.pp.scale leaves, _preprocess_utils.py:49)."""
import numpy as np


class SpatialData:
    """Minimal stand-in for the AnnData fields SpaDOT.train reads (train.py:18-24,
    _train_utils.py:118-140): X (dense, N x G), obs['timepoint'], obsm['spatial']."""

    def __init__(self, X, timepoint, spatial):
        self.X = X
        self.obs = {"timepoint": np.asarray(timepoint)}
        self.obsm = {"spatial": np.asarray(spatial, dtype=np.float64)}
        self.n_obs, self.n_vars = X.shape


def make_timepoint(n_spots, n_genes, seed, n_domains=10, shuffle=True, dtype=np.float32):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_spots)))
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    xy = np.stack([gx.ravel(), gy.ravel()], 1)[:n_spots].astype(np.float64)
    xy += rng.uniform(-0.3, 0.3, size=xy.shape)
    # spatial domains: a few Lloyd iterations on the coordinates
    cen = xy[rng.choice(n_spots, n_domains, replace=False)]
    for _ in range(5):
        lab = ((xy[:, None, :] - cen[None]) ** 2).sum(-1).argmin(1)
        for c in range(n_domains):
            if np.any(lab == c):
                cen[c] = xy[lab == c].mean(0)
    W = rng.normal(size=(n_domains, n_genes)).astype(dtype)
    Y = W[lab] + 0.5 * rng.standard_normal(size=(n_spots, n_genes), dtype=dtype)
    Y -= Y.mean(0, keepdims=True)
    Y /= Y.std(0, keepdims=True) + 1e-12
    if shuffle:   # spot order of real data sets is not spatial; see DESIGN.md "batches"
        perm = rng.permutation(n_spots)
        xy, Y, lab = xy[perm], Y[perm], lab[perm]
    return xy, np.ascontiguousarray(Y, dtype=dtype), lab


def make_dataset(n_timepoints, spots_per_tp, n_genes, seed=1993, shuffle=True):
    """spots_per_tp: one count for every time point, or a list of n_timepoints counts (ragged time points, like the
    747 / 1966 / 1916 / 1967 spots of the reference's ChickenHeart tutorial, examples/ChickenHeart.ipynb:221-230)."""
    counts = [int(spots_per_tp)] * n_timepoints if np.isscalar(spots_per_tp) else [int(c) for c in spots_per_tp]
    if len(counts) != n_timepoints:
        raise ValueError("spots_per_tp must be a count or one count per time point")
    Xs, tps, locs, doms = [], [], [], []
    for t in range(n_timepoints):
        xy, Y, lab = make_timepoint(counts[t], n_genes, seed + 17 * t, shuffle=shuffle)
        Xs.append(Y); locs.append(xy); doms.append(lab)
        tps.append(np.full(counts[t], t))
    data = SpatialData(np.concatenate(Xs), np.concatenate(tps), np.concatenate(locs))
    data.obs["domain"] = np.concatenate(doms)
    return data


def make_raw_counts(spots_per_tp=(400, 1200, 2000), n_genes=1500, n_modules=4, genes_per_module=30, n_rare=5, seed=1993,
                    shuffle=True):
    """Raw counts for the preprocess stage: per time point negative-binomial counts (dispersion 5) on the jittered grid of
    make_timepoint.  Genes 0 .. n_modules * genes_per_module - 1 are spatially patterned, module m sharing one smooth
    pattern of the time point's normalised coordinates (a Gaussian bump for even m, a stripe for odd m); the rest are null
    genes with a constant mean.  The last n_rare genes are detected in fewer than 5 spots of every time point, the last null
    gene before them is zero in the first time point (a zero-variance gene there), and one spot per time point has a zero
    total.  Returns a SpatialData whose X is dense float32 counts, with var_names and uns['module'] (module per gene, -1 for
    null genes)."""
    rng = np.random.default_rng(seed)
    n_tp = len(spots_per_tp)
    n_sp = n_modules * genes_per_module
    module = np.full(n_genes, -1)
    module[:n_sp] = np.repeat(np.arange(n_modules), genes_per_module)
    base = np.exp(rng.uniform(np.log(0.3), np.log(3.0), size=n_genes))
    Xs, tps, locs = [], [], []
    for t, n in enumerate(spots_per_tp):
        xy, _, _ = make_timepoint(int(n), 1, seed + 17 * t, shuffle=shuffle)
        u = (xy - xy.min(0)) / np.maximum(np.ptp(xy, 0), 1e-12)
        pats = []
        for m in range(n_modules):
            c = np.array([0.25 + 0.5 * ((m // 2) % 2), 0.25 + 0.5 * (m % 2)])
            if m % 2 == 0:
                pats.append(np.exp(-((u - c) ** 2).sum(1) / (2 * 0.15 ** 2)))
            else:
                pats.append(0.5 * (1 + np.sin(2 * np.pi * (u[:, 0] * 1.5 + 0.3 * m))))
        mu = np.tile(base, (int(n), 1))
        for m in range(n_modules):
            sel = module == m
            mu[:, sel] = base[sel][None, :] * np.exp(2.0 * pats[m])[:, None]
        r = 5.0
        Y = rng.negative_binomial(r, r / (r + mu)).astype(np.float32)
        Y[:, n_genes - n_rare:] = 0
        for g in range(n_genes - n_rare, n_genes):
            Y[rng.choice(int(n), 3, replace=False), g] = 1
        if t == 0:
            Y[:, n_genes - n_rare - 1] = 0
        Y[rng.integers(int(n))] = 0
        Xs.append(Y); locs.append(xy); tps.append(np.full(int(n), t))
    data = SpatialData(np.concatenate(Xs), np.concatenate(tps), np.concatenate(locs))
    data.var_names = np.array([f"g{g:04d}" for g in range(n_genes)])
    data.uns = {"module": module}
    return data
