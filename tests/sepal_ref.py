"""The numpy restatement of the sepal stage (spadot_amd/sepal.py's docstring is the definition): diffusion of a gene's expression on
the symmetric spatial graph, step by step, with the entropy of every image and the stop rule.  Every product and every sum of the
step is a numpy operation of its own (numpy does not fuse), and the row sums are taken neighbour by neighbour in CSR order, so the
images carry the bits the device must produce.  Both sums of the entropy are math.fsum: the correctly rounded sums, against which
the device's fixed summation tree is bounded (entropy_bound), not compared bit for bit."""
import math

import numpy as np

U = 2.0 ** -53


def sym_csr(src, dst, n):
    """The CSR of W = A + A^T with multiplicity: row i lists first the targets of i's own edges in the order given, then the
    sources of the edges that end in i in the order given.  Returns (rowptr int64 [n + 1], col int64 [2 E])."""
    src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
    rows, cols = np.concatenate([src, dst]), np.concatenate([dst, src])
    order = np.argsort(rows, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return rowptr, cols[order]


def rate(dt, n, E):
    """a = dt n / (2 E) in fp64: the product rounded, then the quotient."""
    return float(dt) * int(n) / (2 * int(E))


def stable(dt, n, E, max_deg):
    """Whether the step is admitted: a max deg < 1."""
    return E == 0 or rate(dt, n, E) * int(max_deg) < 1.0


def max_dt(n, E, max_deg):
    """The largest fp64 dt that stable() admits, found by stepping through the neighbouring doubles of 2 E / (n max deg)."""
    y = 2 * E / (n * max_deg)
    while not stable(y, n, E, max_deg):
        y = float(np.nextafter(y, 0.0))
    while stable(float(np.nextafter(y, np.inf)), n, E, max_deg):
        y = float(np.nextafter(y, np.inf))
    return y


def row_sums_loop(C, rowptr, col):
    """s_i = ((0 + c_j1) + c_j2) + .. by the explicit double loop over the CSR (C: fp64 [n] or [n, genes])."""
    s = np.zeros_like(C)
    for i in range(C.shape[0]):
        acc = np.zeros_like(C[0])
        for e in range(rowptr[i], rowptr[i + 1]):
            acc = acc + C[col[e]]
        s[i] = acc
    return s


def row_sums(C, rowptr, col):
    """The same sums, the same order: the loop runs over the position k in the row, every row adding its k-th neighbour in
    one numpy addition (a row's additions are still sequential and in CSR order; test_sepal_cpu holds it to row_sums_loop)."""
    deg = np.diff(rowptr)
    s = np.zeros_like(C)
    for k in range(int(deg.max()) if deg.size else 0):
        rows = np.flatnonzero(deg > k)
        s[rows] = s[rows] + C[col[rowptr[rows] + k]]
    return s


def step(C, rowptr, col, a):
    """One Jacobi step of the images C (fp64 [n] or [n, genes]): every operation a numpy operation of its own."""
    deg = np.diff(rowptr).astype(np.float64)
    deg = deg if C.ndim == 1 else deg[:, None]
    s = row_sums(C, rowptr, col)
    p = deg * C
    l = s - p
    q = a * l
    new = C + q
    new[new < 0.0] = 0.0
    return new


def entropy_parts(c):
    """(H, S, A) of one image: S = fsum c_i and Q = fsum c_i log c_i over the c_i > 0, H = (log S - Q / S) / n, and A = sum
    |c_i log c_i| (what entropy_bound reads).  (NaN, 0, 0) without a positive value."""
    pos = c[c > 0.0]
    if not pos.size:
        return float("nan"), 0.0, 0.0
    terms = pos * np.log(pos)
    S, Q = math.fsum(pos.tolist()), math.fsum(terms.tolist())
    return (math.log(S) - Q / S) / c.shape[0], S, float(np.abs(terms).sum())      # A feeds a bound: numpy's sum will do


def entropy(c):
    return entropy_parts(c)[0]


def entropy_bound(n, S, A):
    """|H_a - H_b| of two evaluations of H on the SAME image of n spots, each with logarithms within 1 ulp and its own order of
    the two sums.  With u = 2^-53 and g = gamma_(n+2) = (n + 2) u / (1 - (n + 2) u), one evaluation against the exact value:
      * S: at most n positive terms in any order: |S^ - S| <= gamma_(n-1) S <= g S.
      * q_i = c_i log c_i: the logarithm within 1 ulp (2 u relative), the product rounded: |q^_i - q_i| <= gamma_3 |q_i|; their
        sum in any order adds gamma_(n-1) sum |q^_i|: |Q^ - Q| <= g A, A = sum |c_i log c_i|.
      * log S^: |log S^ - log S| <= 2 g (log(1 + e) <= 2 |e| for |e| <= 1/2), and the computed logarithm is within 2 u |log S|.
      * Q^ / S^ against Q / S: g A / S (from Q^) + 2 g |Q| / S (from S^, |Q| <= A) + u A / S (the quotient's rounding), second
        order terms covered by rounding 3 g + u up to 5 g.
      * the subtraction and the division by n are rounded: 2 u (|log S| + A / S) in all, u <= g / 2.
    In all |H^ - H| <= B = (2 g + 4 u |log S| + 5 g A / S) / n, and two evaluations differ by at most 2 B."""
    if not S > 0.0:
        return 0.0
    g = (n + 2) * U / (1.0 - (n + 2) * U)
    return 2.0 * (2.0 * g + 4.0 * U * abs(math.log(S)) + 5.0 * g * A / S) / n


def diffuse(c0, rowptr, col, a, steps):
    """(the image after `steps` steps, [(H, S, A)] of the images 0 .. steps) of one gene; no stop rule.  A degenerate gene
    (no positive value, n < 2 or no edge) takes no step: its parts are NaN throughout."""
    c = np.asarray(c0, dtype=np.float64).copy()
    if is_degenerate(c, col):
        return c, [(float("nan"), 0.0, 0.0)] * (steps + 1)
    parts = [entropy_parts(c)]
    for _ in range(steps):
        c = step(c, rowptr, col, a)
        parts.append(entropy_parts(c))
    return c, parts


def is_degenerate(c0, col):
    return c0.shape[0] < 2 or len(col) == 0 or not np.any(np.asarray(c0) > 0.0)


class Run:
    """One gene under the stop rule: iterations, converged, score, degenerate, image (the last one) and parts, [(H, S, A)] of
    the images 0 .. iterations."""


def run(c0, rowptr, col, a, dt, thresh, n_iter):
    r = Run()
    c = np.asarray(c0, dtype=np.float64).copy()
    r.degenerate = is_degenerate(c, col)
    r.iterations, r.converged, r.image = 0, False, c
    if r.degenerate:
        r.score, r.parts = float("nan"), [(float("nan"), 0.0, 0.0)]
        return r
    r.parts = [entropy_parts(c)]
    for t in range(1, n_iter + 1):
        c = step(c, rowptr, col, a)
        r.parts.append(entropy_parts(c))
        r.iterations = t
        if abs(r.parts[-1][0] - r.parts[-2][0]) <= thresh:
            r.converged = True
            break
    r.image, r.score = c, float(dt) * r.iterations
    return r


def run_genes(C0, rowptr, col, a, dt, thresh, n_iter):
    """run() of every column of C0 [n, genes], the running genes stepped together (the same bits: a step works column by
    column)."""
    C = np.asarray(C0, dtype=np.float64).copy()
    runs = []
    for g in range(C.shape[1]):
        r = Run()
        r.degenerate = is_degenerate(C[:, g], col)
        r.iterations, r.converged, r.score = 0, False, float("nan")
        r.parts = [(float("nan"), 0.0, 0.0)] if r.degenerate else [entropy_parts(C[:, g])]
        runs.append(r)
    active = np.array([g for g, r in enumerate(runs) if not r.degenerate], dtype=np.int64)
    for t in range(1, n_iter + 1):
        if not active.size:
            break
        C[:, active] = step(C[:, active], rowptr, col, a)
        keep = []
        for g in active:
            r = runs[g]
            r.parts.append(entropy_parts(C[:, g]))
            r.iterations = t
            if abs(r.parts[-1][0] - r.parts[-2][0]) <= thresh:
                r.converged = True
            else:
                keep.append(g)
        active = np.array(keep, dtype=np.int64)
    for g, r in enumerate(runs):
        r.image = C[:, g].copy()
        if not r.degenerate:
            r.score = float(dt) * r.iterations
    return runs


def order(score):
    """The genes by descending score, NaN last, ties by gene index."""
    score = np.asarray(score, dtype=np.float64)
    return np.lexsort((np.arange(score.shape[0]), -np.where(np.isnan(score), -np.inf, score)))
