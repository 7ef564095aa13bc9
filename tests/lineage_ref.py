"""Host statement of the lineage analyses (spadot_amd/lineage.py's module docstring) in plain numpy on DENSE plans: no torch, no
device.  Written from the definitions, not from lineage.py.  Every sum is accumulated wider than fp64: in longdouble where that
is wider (x87 extended), else with the exact math.fsum; results are returned in that wide type (or fp64) for the caller to compare.

plans: list of dense arrays, plans[t] of shape [N_t, N_{t+1}], non-negative.
"""
import math

import numpy as np

LD = np.longdouble
WIDE = np.finfo(LD).nmant >= 63
EPS = 2.0 ** -53


def matmul(A, B):
    """A @ B with wide accumulation."""
    A, B = np.asarray(A), np.asarray(B)
    if WIDE:
        return A.astype(LD) @ B.astype(LD)
    A, B = A.astype(np.float64), B.astype(np.float64)
    return np.array([[math.fsum(A[i] * B[:, j]) for j in range(B.shape[1])] for i in range(A.shape[0])], dtype=np.float64)


def _sum(a, axis):
    a = np.asarray(a)
    if WIDE:
        return a.astype(LD).sum(axis)
    a = a.astype(np.float64)
    a = a if axis == 0 else a.T
    return np.array([math.fsum(a[:, j]) for j in range(a.shape[1])], dtype=np.float64)


def _div_cols(P):
    """Every column divided by its sum; a column whose sum is 0 stays 0."""
    s = _sum(P, 0)
    out = np.zeros_like(P)
    nz = s != 0
    out[:, nz] = P[:, nz] / s[nz]
    return out


def _div_rows(P, s=None):
    """Every row divided by its sum (or by s); a row whose divisor is 0 becomes / stays 0."""
    s = _sum(P, 1) if s is None else s
    out = np.zeros_like(P)
    nz = s != 0
    out[nz] = P[nz] / s[nz][:, None]
    return out


def onehot(labels, k=None):
    labels = np.asarray(labels)
    k = int(labels.max()) + 1 if k is None else k
    out = np.zeros((labels.size, k), dtype=LD if WIDE else np.float64)
    out[np.arange(labels.size), labels] = 1
    return out


def push(plans, P, t, u, normalize=False):
    for s in range(t, u):
        P = matmul(np.asarray(plans[s]).T, P)
        if normalize:
            P = _div_cols(P)
    return P


def pull(plans, P, u, t, normalize=False):
    for s in range(u - 1, t - 1, -1):
        P = matmul(plans[s], P)
        if normalize:
            P = _div_cols(P)
    return P


def trajectories(plans, labels, t):
    """List over all time points u of [N_u, K_t]."""
    T = len(plans) + 1
    start = _div_cols(onehot(labels))
    out = [None] * T
    out[t] = start
    for u in range(t + 1, T):
        out[u] = push(plans, start, t, u, normalize=True)
    for u in range(t):
        out[u] = pull(plans, start, t, u, normalize=True)
    return out


def fates(plans, labels_u, u, t):
    return _div_rows(pull(plans, onehot(labels_u), u, t))


def transition_table(plans, labels_t, labels_u, t, u):
    M = onehot(labels_u)
    for s in range(u - 1, t, -1):
        r = _sum(plans[s], 1)
        M = _div_rows(matmul(plans[s], M), r)
    M = matmul(plans[t], M)
    return matmul(onehot(labels_t).T, M)


def block_sums(plan, labels_a, labels_b):
    """The consecutive table: sum of the plan over (domain of the row, domain of the column)."""
    return matmul(onehot(labels_a).T, matmul(plan, onehot(labels_b)))
