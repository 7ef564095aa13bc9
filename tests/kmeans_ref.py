"""The k-means++ selection rounds in torch (sklearn's _kmeans_plusplus: 2 + int(log k) candidates per centre drawn by
potential, the candidate with the smallest new potential wins), written apart from the package's seeding kernel so that
the GPU tests compare two independent statements of the rule.  All restarts run batched; the draws are those of
spadot_amd.kmeans.sweep_draws."""
import numpy as np
import torch


def init_centers(X, xsq, seeds, k):
    """Seeded centres [R, k, d] of the centred data X [n, d] (xsq: its squared row norms) for the restart seeds `seeds`."""
    n, d = X.shape
    R = len(seeds)
    trials = 2 + int(np.log(k))
    first = np.empty(R, dtype=np.int64)
    U = np.empty((R, max(k - 1, 1), trials), dtype=np.float64)
    for r, s in enumerate(seeds):
        rs = np.random.RandomState(int(s))
        first[r] = int(rs.choice(n))
        for c in range(1, k):
            U[r, c - 1] = rs.uniform(size=trials)
    first = torch.as_tensor(first, device=X.device)
    U = torch.as_tensor(U, dtype=X.dtype, device=X.device)
    centers = torch.empty((R, k, d), dtype=X.dtype, device=X.device)
    centers[:, 0] = X[first]
    c0 = centers[:, 0]                                                        # [R, d]
    closest = (xsq[None, :] - 2.0 * (c0 @ X.T) + (c0 * c0).sum(1)[:, None]).clamp_(min=0)     # [R, n]
    pot = closest.sum(1)                                                      # [R]
    ar = torch.arange(R, device=X.device)
    for c in range(1, k):
        rv = U[:, c - 1] * pot[:, None]                                       # [R, trials]
        cand = torch.searchsorted(torch.cumsum(closest, 1), rv).clamp_(max=n - 1)
        Xc = X[cand]                                                          # [R, trials, d]
        dist = (xsq[None, None, :] - 2.0 * torch.matmul(Xc, X.T) + (Xc * Xc).sum(2)[:, :, None]).clamp_(min=0)
        dist = torch.minimum(dist, closest[:, None, :])                       # [R, trials, n]
        pots = dist.sum(2)                                                    # [R, trials]
        best = torch.argmin(pots, dim=1)                                      # [R]
        centers[:, c] = Xc[ar, best]
        closest = dist[ar, best]
        pot = pots[ar, best]
    return centers
