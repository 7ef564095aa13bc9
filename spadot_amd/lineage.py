"""Domain lineages of the analyze stage: what the spot-level transport plans say ACROSS more than one step.

The analyze stage solves one unbalanced plan Pi_t per pair of consecutive time points (analyze_ot.spot_transport) and, until
now, reduced each to one domain x domain table.  A table forgets which spots inside a domain received the mass, so tables
cannot be chained.  This module keeps the T - 1 solvers alive (TransportChain) and chains the plans themselves through
OTSolver.apply, the device product of the implicit plan (or its transpose) with a skinny matrix: no plan is ever formed.

The three analyses are defined HERE, by this project.  The idea of trajectories, fates and long-range transitions read off a
chain of transport maps comes from Waddington-OT; wot is not installed and cannot be pinned (the position analyze_ot.py takes
for the solver), so nothing below claims to reproduce its numbers.  Write r_t for the row sums of Pi_t and 1_c for the
indicator column of domain c:

  push(P, t, u)      P <- Pi_s^T P for s = t .. u - 1 (mass carried forward);  pull(P, u, t): P <- Pi_s P for s = u - 1 .. t.
                     With normalize=True every column is divided by its sum after every step (a zero column stays zero).
  trajectories       for every domain c of time point t start from 1_c / |c|; descendants at u > t by push, ancestors at
                     u < t by pull, both normalised per step: one probability vector over the spots of u per domain.
  fates              F = pull(indicators of the domains at u, u, t) without normalisation, then every ROW divided by its sum:
                     per spot at t, the share of its transported mass that arrives in each domain of u (a zero row stays zero).
  transition_table   indicators_t^T Pi_t M_{t+1} ... M_{u-1} indicators_u with M_s = diag(1 / r_s) Pi_s: every intermediate
                     spot hands on the mass it received in the proportions of its own plan row.  The transport is
                     unbalanced, so the column sums of Pi_s and the row sums of Pi_{s+1} differ and the plain product would
                     rescale the mass at every step.  For u = t + 1 it is the stage's existing table (OTSolver.transition_table,
                     the same reduction).  r_s comes from apply(ones) on the device (one more product per solver, cached), not
                     from plan_rowsums(), which copies to the host and synchronises.
"""
import numpy as np
import torch

from . import analyze_ot


def indicators(labels, k=None, device="cuda:0"):
    """One-hot columns [N, k] (fp64, on the device) of integer labels; k defaults to max + 1."""
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.int64, device=device)
    k = int(lab.max()) + 1 if k is None else int(k)
    out = torch.zeros((lab.numel(), k), dtype=torch.float64, device=device)
    out[torch.arange(lab.numel(), device=device), lab] = 1.0
    return out


def _safe_div(x, s):
    """x / s where s != 0, else 0 (x is 0 there whenever s is a sum of the non-negative x)."""
    return torch.where(s != 0, x / torch.where(s != 0, s, torch.ones_like(s)), torch.zeros_like(x))


class TransportChain:
    """The plans between all consecutive time points, solved exactly as the transition tables solve them
    (analyze_ot.spot_transport: cost from the latents, `growth_iters` solves for which='last') and kept on the device.

    Memory: every pair keeps its solver, that is the cost and the kernel matrix, 2 * I * ld * 4 B in f32 storage (8 B in f64;
    ld = J rounded up to 64) -- 0.8 GB per 10 000 x 10 000 pair -- plus, from the first product on, one work space of at most
    about 70 MB per solver.  Nothing of size I * J is allocated by the analyses.  Use it as a context manager, or close() it:
    that closes every solver, also when a solve raised half way through the chain."""

    def __init__(self, latents, config=None, which="last", storage="f32", device="cuda:0"):
        self.device = torch.device(device)
        self.which = which
        self.sizes = [int(np.shape(x)[0]) for x in latents]
        self.solvers, self.infos, self._rowsums = [], [], {}
        try:
            for t in range(len(latents) - 1):
                solver, infos = analyze_ot.spot_transport(latents[t], latents[t + 1], config, which=which, storage=storage,
                                                          device=device)
                self.solvers.append(solver)
                self.infos.append(infos)
        except BaseException:
            self.close()
            raise

    def __len__(self):
        return len(self.sizes)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        solvers, self.solvers = self.solvers, []
        self._rowsums = {}
        err = None
        for s in solvers:
            try:
                s.close()
            except Exception as e:          # close the rest all the same
                err = err or e
        if err is not None:
            raise err

    # ---- products ----
    def _matrix(self, P, n):
        P = torch.as_tensor(P).to(self.device, torch.float64)
        if P.dim() == 1:
            P = P[:, None]
        if P.dim() != 2 or P.shape[0] != n:
            raise ValueError(f"expected {n} rows, got an array of shape {tuple(P.shape)}")
        return P

    def _check(self, t, u):
        if not (0 <= t < u < len(self.sizes)):
            raise ValueError(f"need 0 <= t < u < {len(self.sizes)} time points, got t = {t}, u = {u}")
        if len(self.solvers) != len(self.sizes) - 1:
            raise RuntimeError("the chain is closed")

    def rowsums(self, s):
        """r_s = Pi_s 1 as a device column [N_s, 1]."""
        if s not in self._rowsums:
            ones = torch.ones((self.sizes[s + 1], 1), dtype=torch.float64, device=self.device)
            self._rowsums[s] = self.solvers[s].apply(ones)
        return self._rowsums[s]

    def push(self, P, t, u, normalize=False):
        """P [N_t, k] at time point t carried forward to u > t.  Returns a device tensor [N_u, k]."""
        self._check(t, u)
        P = self._matrix(P, self.sizes[t])
        for s in range(t, u):
            P = self.solvers[s].apply(P, transpose=True)
            if normalize:
                P = _safe_div(P, P.sum(0, keepdim=True))
        return P

    def pull(self, P, u, t, normalize=False):
        """P [N_u, k] at time point u pulled back to t < u.  Returns a device tensor [N_t, k]."""
        self._check(t, u)
        P = self._matrix(P, self.sizes[u])
        for s in range(u - 1, t - 1, -1):
            P = self.solvers[s].apply(P)
            if normalize:
                P = _safe_div(P, P.sum(0, keepdim=True))
        return P

    # ---- analyses ----
    def trajectories(self, labels, t):
        """labels: the domains of the spots of time point t.  Returns a list over ALL time points u of numpy fp64 arrays
        [N_u, K_t]: column c is where domain c of t comes from (u < t) or goes to (u > t), every column summing to 1 (a column
        whose mass is lost on the way is 0); at u = t it is the start 1_c / |c| itself."""
        T = len(self.sizes)
        if not 0 <= t < T:
            raise ValueError(f"time point {t} outside 0 .. {T - 1}")
        start = indicators(labels, device=self.device)
        if start.shape[0] != self.sizes[t]:
            raise ValueError(f"{start.shape[0]} labels for the {self.sizes[t]} spots of time point {t}")
        start = _safe_div(start, start.sum(0, keepdim=True))
        out = [None] * T
        out[t] = start
        for u in range(t + 1, T):
            out[u] = self.push(out[u - 1], u - 1, u, normalize=True)
        for u in range(t - 1, -1, -1):
            out[u] = self.pull(out[u + 1], u + 1, u, normalize=True)
        return [x.cpu().numpy() for x in out]

    def fates(self, labels_u, u, t):
        """Per spot of time point t < u, the share of its transported mass that arrives in each domain of u:
        numpy fp64 [N_t, K_u], every row summing to 1 (0 for a spot that sends nothing)."""
        F = self.pull(indicators(labels_u, device=self.device), u, t)
        return _safe_div(F, F.sum(1, keepdim=True)).cpu().numpy()

    def transition_table(self, labels_t, labels_u, t, u, n_row_groups=None, n_col_groups=None):
        """Domain x domain table between time points t and u >= t + 1 (numpy fp64 [K_t, K_u]); for u = t + 1 the existing
        table of the stage, from the same device reduction."""
        self._check(t, u)
        if u == t + 1:
            return self.solvers[t].transition_table(labels_t, labels_u, n_row_groups, n_col_groups).cpu().numpy()
        M = indicators(labels_u, n_col_groups, device=self.device)
        for s in range(u - 1, t, -1):
            M = _safe_div(self.solvers[s].apply(M), self.rowsums(s))
        M = self.solvers[t].apply(M)
        return (indicators(labels_t, n_row_groups, device=self.device).T @ M).cpu().numpy()


def lineage_arrays(chain, labels, timepoints, masks):
    """The arrays of the stage's lineage outputs, in input row order (masks: one boolean row mask per sorted time point).
    Returns {"trajectories": X [N, sum_t K_t], "trajectory_names", "fates": X [N, K_last], "fate_names", "long_tables":
    {(d, e): table for e > d + 1}}."""
    T = len(timepoints)
    N = int(masks[0].shape[0])
    ks = [int(np.max(l)) + 1 for l in labels]
    traj = np.zeros((N, sum(ks)), dtype=np.float64)
    names, c0 = [], 0
    for t in range(T):
        cols = chain.trajectories(labels[t], t)
        for u in range(T):
            traj[np.flatnonzero(masks[u])[:, None], np.arange(c0, c0 + ks[t])[None, :]] = cols[u]
        names += [f"{timepoints[t]}_{c}" for c in range(ks[t])]
        c0 += ks[t]
    fates = np.zeros((N, ks[-1]), dtype=np.float64)
    for t in range(T - 1):
        fates[masks[t]] = chain.fates(labels[-1], T - 1, t)
    fates[masks[-1]] = np.eye(ks[-1], dtype=np.float64)[np.asarray(labels[-1])]
    long_tables = {(d, e): chain.transition_table(labels[d], labels[e], d, e, ks[d], ks[e])
                   for d in range(T) for e in range(d + 2, T)}
    return {"trajectories": traj, "trajectory_names": np.array(names), "fates": fates,
            "fate_names": np.array([f"{timepoints[-1]}_{c}" for c in range(ks[-1])]), "long_tables": long_tables}


def write_lineage(output_dir, chain, labels, timepoints, masks, rows, tp_all, prefix=""):
    """Writes {prefix}transition_table_{d}_{e}.csv / .npz for every e > d + 1 (the layout of the consecutive ones),
    {prefix}trajectories.npz and {prefix}fates.npz (X, rows, timepoint, names).  Returns lineage_arrays()'s dict."""
    import os
    res = lineage_arrays(chain, labels, timepoints, masks)
    for (d, e), tab in res["long_tables"].items():
        obs = np.array([f"{timepoints[d]}_{c}" for c in range(tab.shape[0])])
        var = np.array([f"{timepoints[e]}_{c}" for c in range(tab.shape[1])])
        analyze_ot.write_table(os.path.join(output_dir, f"{prefix}transition_table_{d}_{e}"), tab, obs, var)
    np.savez_compressed(os.path.join(output_dir, prefix + "trajectories.npz"), X=res["trajectories"], rows=np.asarray(rows),
                        timepoint=np.asarray(tp_all), names=res["trajectory_names"])
    np.savez_compressed(os.path.join(output_dir, prefix + "fates.npz"), X=res["fates"], rows=np.asarray(rows),
                        timepoint=np.asarray(tp_all), names=res["fate_names"])
    return res
