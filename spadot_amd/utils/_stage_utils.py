"""What the analysis stages (neighbors, cooccurrence, autocorr, ligrec, hotspots, modules, ripley) share on the host.  What only
the three Moran stages share is in spadot_amd/moran.py."""
import zipfile

import numpy as np

MAX_EDGES = 2147483647


def labeling_runs(n_perms, observed, first, per, budget):
    """The labelings of a call -- the observed one, if any, then the permutations first .. first + n_perms - 1 -- in runs that
    share one buffer of `budget` units at `per` units a labeling: [(observed in the run, its first permutation, its
    permutations)].  One run where everything fits; otherwise max(1, budget // per) labelings a run, the observed one in the
    first."""
    observed, n_perms, first = int(bool(observed)), int(n_perms), int(first)
    L = observed + n_perms
    step = L if per * L <= budget else max(1, budget // per)
    runs = []
    for l in range(0, L, step):                                  # l: the labelings ahead of the run, the observed one included
        obs = observed if l == 0 else 0
        runs.append((bool(obs), first + l - (observed - obs), min(step, L - l) - obs))
    return runs


def edge_pair(e, dev, g):
    """The (src, dst) of graph g as 1-d integer device tensors on `dev` (None: wherever they are)."""
    import torch
    src, dst = e
    src = src if isinstance(src, torch.Tensor) else torch.as_tensor(np.asarray(src))
    dst = dst if isinstance(dst, torch.Tensor) else torch.as_tensor(np.asarray(dst))
    for t in (src, dst):
        if not t.is_cuda:
            raise RuntimeError("spadot_amd counts neighbourhoods on the MI355X only (got a CPU tensor); there is no CPU path")
        if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
            raise ValueError(f"the edges of graph {g} must be two 1-d integer tensors (got {tuple(t.shape)} {t.dtype})")
    if src.shape != dst.shape or src.device != dst.device or (dev is not None and src.device != dev):
        raise ValueError(f"the sources and targets of graph {g} must have one length and all graphs one device")
    if src.shape[0] > MAX_EDGES:
        raise ValueError(f"graph {g} has {src.shape[0]} edges: the device takes at most {MAX_EDGES} per graph")
    return src, dst


def savez_pinned(path, arrays):
    """np.savez with the archive's time stamps pinned, so that two runs write the same bytes (np.load reads it as any npz)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED, allowZip64=True) as z:
        for name, v in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
