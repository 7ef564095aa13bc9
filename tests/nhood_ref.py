"""The neighbourhood-enrichment definition of DESIGN 7h restated in numpy: the permutation pi of (seed, g, p, n), the count matrix
of a labeling, the permuted count stacks and the host statistics.  Independent of the package (its own Benjamini-Hochberg)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
ROUNDS = 6


def _u64(v):
    return np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


def splitmix64(state):
    """One splitmix64 draw: (new state, output), uint64 wrap-around arithmetic."""
    with np.errstate(over="ignore"):
        state = state + np.uint64(0x9E3779B97F4A7C15)
        z = state
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return state, z ^ (z >> np.uint64(31))


def mix32(x):
    """The xorshift-multiply mixer on 32-bit values held in uint64 arrays."""
    x = x & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x21F0AAAD)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x735A2D97)) & M32
    return x ^ (x >> np.uint64(15))


def round_keys(seed, g, p):
    _, s = splitmix64(_u64(seed) ^ (_u64(g) << np.uint64(32)) ^ _u64(p))
    keys = []
    for _ in range(ROUNDS):
        s, z = splitmix64(s)
        keys.append(z & M32)
    return keys


def domain_bits(n):
    """ceil(log2 n) rounded up to an even number, at least 2."""
    b = max(1, (max(int(n), 2) - 1).bit_length())
    return b + (b & 1)


def perm(n, seed, g, p):
    """pi_p of graph g under seed: int64 [n], a bijection of 0 .. n-1."""
    half = np.uint64(domain_bits(n) // 2)
    mask = np.uint64((1 << int(half)) - 1)
    keys = round_keys(seed, g, p)

    def feistel(x):
        L, R = x >> half, x & mask
        for k in keys:
            L, R = R, L ^ (mix32(R ^ k) & mask)
        return (L << half) | R

    x = feistel(np.arange(n, dtype=np.uint64))
    while True:
        bad = x >= np.uint64(n)
        if not bad.any():
            return x.astype(np.int64)
        x[bad] = feistel(x[bad])


def count_matrix(src, dst, lab, K):
    """C[a, b] = #{edges i -> j : lab[i] = a, lab[j] = b}, int64 [K, K]."""
    lab = np.asarray(lab, dtype=np.int64)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    return np.bincount(lab[src] * K + lab[dst], minlength=K * K).reshape(K, K)


def perm_counts(src, dst, lab, K, n_perms, seed, g, first=0):
    """The count matrices of lab[pi_p] for p = first .. first + n_perms - 1: int64 [n_perms, K, K]."""
    lab = np.asarray(lab, dtype=np.int64)
    return np.stack([count_matrix(src, dst, lab[perm(lab.shape[0], seed, g, first + p)], K) for p in range(n_perms)])


def bh(p):
    p = np.asarray(p, dtype=np.float64)
    m = p.size
    order = np.argsort(p, kind="stable")
    adj = np.empty(m)
    running = 1.0
    for rank in range(m, 0, -1):
        running = min(running, p[order[rank - 1]] * m / rank)
        adj[order[rank - 1]] = running
    return adj


def stats(counts, perms, sizes):
    """expected, sd, zscore, p_enriched, p_depleted, padj, share, coherence from the integers (fp64)."""
    C = np.asarray(counts, dtype=np.float64)
    Cp = np.asarray(perms)
    P, K = Cp.shape[0], C.shape[0]
    expected = Cp.mean(axis=0, dtype=np.float64)
    sd = Cp.std(axis=0, dtype=np.float64)
    z = np.full((K, K), np.nan)
    share = np.full((K, K), np.nan)
    pe, pd = np.empty((K, K)), np.empty((K, K))
    for a in range(K):
        for b in range(K):
            if sd[a, b] > 0:
                z[a, b] = (C[a, b] - expected[a, b]) / sd[a, b]
            if C[a].sum() > 0:
                share[a, b] = C[a, b] / C[a].sum()
            pe[a, b] = (1 + int((Cp[:, a, b] >= counts[a][b]).sum())) / (P + 1)
            pd[a, b] = (1 + int((Cp[:, a, b] <= counts[a][b]).sum())) / (P + 1)
    cells = [(a, b) for a in range(K) for b in range(K) if sizes[a] > 0 and sizes[b] > 0]
    padj = np.full((K, K), np.nan)
    if cells:
        adj = bh([min(1.0, 2.0 * min(pe[a, b], pd[a, b])) for a, b in cells])
        for (a, b), v in zip(cells, adj):
            padj[a, b] = v
    return dict(expected=expected, sd=sd, zscore=z, p_enriched=pe, p_depleted=pd, padj=padj, share=share,
                coherence=np.diagonal(share).copy())


def analytic_expectation(E, sizes):
    """E n_a n_b / (n (n - 1)) off the diagonal, E n_a (n_a - 1) / (n (n - 1)) on it: the mean of C_p over all permutations."""
    nk = np.asarray(sizes, dtype=np.float64)
    n = nk.sum()
    ana = E * np.outer(nk, nk) / (n * (n - 1.0))
    ana[np.diag_indices(nk.size)] = E * nk * (nk - 1.0) / (n * (n - 1.0))
    return ana


def same_share(src, dst, lab, n):
    """Per node the share of its out-neighbours with its own label; NaN without neighbours."""
    lab = np.asarray(lab)
    deg = np.bincount(src, minlength=n).astype(np.float64)
    own = np.bincount(src, weights=(lab[src] == lab[dst]).astype(np.float64), minlength=n)
    with np.errstate(invalid="ignore", divide="ignore"):
        return own / deg
