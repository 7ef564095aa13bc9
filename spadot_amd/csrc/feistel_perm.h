// feistel_perm.h -- the permutation pi_p of (seed, graph id, p, n) that the neighbors, autocorr, ligrec, hotspots, modules and
// ripley stages share (restated in numpy in tests/nhood_ref.py): a six-round balanced Feistel network with cycle
// walking, evaluated per element; no permutation is stored or sorted anywhere.
#ifndef SPADOT_FEISTEL_PERM_H
#define SPADOT_FEISTEL_PERM_H
#include <hip/hip_runtime.h>

#define NH_ROUNDS 6

struct NhPerm {
    unsigned key[NH_ROUNDS];
    unsigned half, mask, n;
};

__host__ __device__ static inline unsigned nh_mix32(unsigned x) {
    x ^= x >> 16; x *= 0x21F0AAADu;
    x ^= x >> 15; x *= 0x735A2D97u;
    x ^= x >> 15;
    return x;
}

__host__ __device__ static inline unsigned long long nh_splitmix(unsigned long long &s) {
    s += 0x9E3779B97F4A7C15ull;
    unsigned long long z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// bits of the Feistel domain: ceil(log2 n) rounded up to an even number, at least 2 (n < 2^31: at most 32)
__host__ __device__ static inline unsigned nh_bits(unsigned n) {
    unsigned b = 1;
    while (b < 32 && (1ull << b) < (unsigned long long)n) ++b;
    b += b & 1;
    return b;
}

__host__ __device__ static inline NhPerm nh_perm_setup(unsigned long long seed, unsigned long long g, unsigned long long p, unsigned n) {
    NhPerm q;
    unsigned long long s = seed ^ (g << 32) ^ p;
    s = nh_splitmix(s);
#pragma unroll
    for (int r = 0; r < NH_ROUNDS; ++r) q.key[r] = (unsigned)nh_splitmix(s);
    q.half = nh_bits(n) / 2;
    q.mask = (1u << q.half) - 1u;
    q.n = n;
    return q;
}

__host__ __device__ static inline unsigned nh_perm_at(const NhPerm &q, unsigned i) {
    unsigned x = i;
    do {                                                 // cycle walking: the domain is below 4 n, so fewer than 4 turns on average
        unsigned L = x >> q.half, R = x & q.mask;
#pragma unroll
        for (int r = 0; r < NH_ROUNDS; ++r) {
            const unsigned t = L ^ (nh_mix32(R ^ q.key[r]) & q.mask);
            L = R;
            R = t;
        }
        x = (L << q.half) | R;
    } while (x >= q.n);
    return x;
}

// pi^-1 of nh_perm_at: the rounds backwards, walking the same cycle the other way
__host__ __device__ static inline unsigned ac_perm_inv(const NhPerm &q, unsigned y) {
    unsigned x = y;
    do {
        unsigned L = x >> q.half, R = x & q.mask;
#pragma unroll
        for (int r = NH_ROUNDS - 1; r >= 0; --r) {
            const unsigned t = R ^ (nh_mix32(L ^ q.key[r]) & q.mask);
            R = L;
            L = t;
        }
        x = (L << q.half) | R;
    } while (x >= q.n);
    return x;
}

#endif
