// markers.hip -- the markers stage's device work (gfx950, wave64): per (time point, gene, domain) Wilcoxon rank-sum tests of
// log-normalised counts, scipy.stats.mannwhitneyu(x_in, x_out, 'two-sided', method='asymptotic', use_continuity=True).
//
// Data layout as preprocess.hip: CSC (genes x spots), rows in output order, a time point t owns the rows
// [tp_off[t], tp_off[t+1]), so a gene's column splits into one contiguous segment per time point (binary search).
//
// k_mk_lognorm   v = float(log1p(x * target / total[row])) per stored entry.
// k_mk_ranksum   one 256-thread workgroup per (time point, gene).  The zeros are never materialised: with Z implicit zeros every
//                zero has twice-rank Z + 1 and a nonzero in the tie run [s, e) of the sorted nonzeros has twice-rank
//                2 Z + s + e + 1.  The nonzeros are sorted as u64 = fp32 bits << 32 | domain (non-negative floats order as
//                unsigned integers; the domain rides in the low word), a bitonic network in LDS for segments of up to MK_CAP
//                entries.  Longer segments are queued and sorted by k_mk_ranksum_long through a global slab: MK_CAP-sized
//                chunks in LDS, the strides >= MK_CAP of the same network in global memory.
//                Integer outputs (twice the rank sums, sum of t^3 - t, nonzeros per domain) are exact and order-free: LDS
//                integer atomics.  The fp64 sums of v per domain have a fixed order: lane l of one wavefront owns the sorted
//                positions l, l + 64, ... and a private row of accumulators, then one thread per domain adds the 64 rows in
//                order.  No floating-point atomics: two runs are bitwise identical.
// k_mk_finish    U1, score, p per (time point, gene, domain) from the integers.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/spadot_model.h"
#include "csc_walk.h"

typedef unsigned long long mk_u64;

#define MK_THREADS 256
#define MK_WAVE 64
#define MK_CAP 4096                // u64 entries sorted in LDS: 32 KiB, four workgroups per CU beside the accumulators
#define MK_MAX_K 32                // domains per time point (the cap of analyze)
#define MK_MAX_N 2097151           // spots per time point: n^3 < 2^63
#define MK_MAX_LONG 1024           // workgroups (and slabs) of the long path: 4 per CU
#define MK_SLAB_BYTES (1ll << 30)  // most scratch the slabs of the long path take together
#define MK_HEAD 256                // bytes ahead of the queue: the counter

static inline long long mk_pow2(long long n) {
    long long p = 4;
    while (p < n) p <<= 1;
    return p;
}

// ---------------------------------------------------------------- log-normalise
__global__ void __launch_bounds__(MK_THREADS) k_mk_lognorm(const int *ridx, const float *val, const double *total, long long nnz,
                                                           double target, float *v) {
    const long long p = (long long)blockIdx.x * MK_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const double tot = total[ridx[p]];
    v[p] = tot > 0.0 ? (float)log1p((double)val[p] * target / tot) : 0.0f;
}

// ---------------------------------------------------------------- bitonic network
__device__ __forceinline__ void mk_cx(mk_u64 &x, mk_u64 &y, bool up) {
    if ((x > y) == up) { const mk_u64 t = x; x = y; y = t; }
}

// steps j = j0, j0 / 2, ..., 1 of stage k on the P entries of a (LDS; P a power of two >= 4, a[0] has index gbase in the whole
// sequence).  The strides 2 and 1 run in registers on four consecutive entries per thread (two 16-byte LDS accesses).
__device__ __forceinline__ void mk_stage(mk_u64 *a, int P, long long k, int j0, long long gbase) {
    for (int j = j0; j >= 4; j >>= 1) {
        for (int p = threadIdx.x; p < P / 2; p += MK_THREADS) {
            const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
            mk_u64 x = a[i], y = a[i | j];
            const bool up = ((gbase + i) & k) == 0;
            if ((x > y) == up) { a[i] = y; a[i | j] = x; }
        }
        __syncthreads();
    }
    for (int q = threadIdx.x; q < P / 4; q += MK_THREADS) {
        mk_u64 *e = a + 4 * q;
        mk_u64 x0 = e[0], x1 = e[1], x2 = e[2], x3 = e[3];
        const long long g = gbase + 4 * q;
        if (j0 >= 2) {
            const bool up = (g & k) == 0;
            mk_cx(x0, x2, up); mk_cx(x1, x3, up);
            mk_cx(x0, x1, up); mk_cx(x2, x3, up);
        } else {
            mk_cx(x0, x1, (g & k) == 0);
            mk_cx(x2, x3, ((g + 2) & k) == 0);
        }
        e[0] = x0; e[1] = x1; e[2] = x2; e[3] = x3;
    }
    __syncthreads();
}

__device__ __forceinline__ mk_u64 mk_key(const float *v, const int *ridx, const int *labels, long long p) {
    return ((mk_u64)__float_as_uint(v[p]) << 32) | (mk_u64)(unsigned)labels[ridx[p]];
}

// ---------------------------------------------------------------- ranks, ties and sums of a sorted segment
// a: the m sorted keys (LDS or global).  acc: 64 * Kp doubles of LDS.  n: spots of the time point, nk: its domain sizes.
// All 256 threads call; ends with the outputs written.
__device__ __forceinline__ void mk_reduce_sorted(const mk_u64 *a, int m, int n, int K, const int *nk, double *acc,
                                                 mk_u64 *s_r2, int *s_nnz, mk_u64 *s_ties, long long *r2, long long *ties,
                                                 int *nnz_k, double *vsum) {
    const int tid = threadIdx.x, lane = tid & (MK_WAVE - 1), wave = tid >> 6;
    const int Kp = K | 1;
    if (tid < MK_MAX_K) { s_r2[tid] = 0; s_nnz[tid] = 0; }
    if (tid == 0) *s_ties = 0;
    for (int i = tid; i < MK_WAVE * Kp; i += MK_THREADS) acc[i] = 0.0;
    // stored entries whose v rounded to 0 sort first and join the run of zeros
    int z0 = 0;
    {
        int hi = m;
        while (z0 < hi) {
            const int mid = z0 + ((hi - z0) >> 1);
            if ((a[mid] >> 32) == 0) z0 = mid + 1; else hi = mid;
        }
    }
    __syncthreads();
    const long long Z = (long long)n - m;                // implicit zeros
    if (wave == 0) {
        // fp64 sums: lane l adds the sorted positions l, l + 64, ... into its own row
        for (int i = z0 + lane; i < m; i += MK_WAVE) {
            const mk_u64 key = a[i];
            const unsigned lab = (unsigned)key;
            if (lab < (unsigned)K) acc[lane * Kp + lab] += (double)__uint_as_float((unsigned)(key >> 32));
        }
    } else {
        // wavefronts 1 .. 3 take 64 consecutive sorted positions at a time
        for (int c0 = z0 + (wave - 1) * MK_WAVE; c0 < m; c0 += 3 * MK_WAVE) {
            const int i = c0 + lane;
            const bool on = i < m;
            mk_u64 key = 0;
            unsigned bits = 0;
            bool head = false, tail = false;
            if (on) {
                key = a[i];
                bits = (unsigned)(key >> 32);
                head = i == z0 || (unsigned)(a[i - 1] >> 32) != bits;
                tail = i == m - 1 || (unsigned)(a[i + 1] >> 32) != bits;
            }
            int s = head ? i : -1;                       // start of the run: the last head at or before i ...
            int e = tail ? i + 1 : 0x7fffffff;           // ... its end: the first tail at or after i
#pragma unroll
            for (int off = 1; off < MK_WAVE; off <<= 1) {
                const int ts = __shfl_up(s, off, MK_WAVE);
                const int te = __shfl_down(e, off, MK_WAVE);
                if (lane >= off) s = max(s, ts);
                if (lane + off < MK_WAVE) e = min(e, te);
            }
            if (on) {
                if (s < 0) {                             // the run began before this block of 64
                    int lo = z0, hi = c0;
                    while (lo < hi) {
                        const int mid = lo + ((hi - lo) >> 1);
                        if ((unsigned)(a[mid] >> 32) < bits) lo = mid + 1; else hi = mid;
                    }
                    s = lo;
                }
                if (e == 0x7fffffff) {                   // the run ends after this block of 64
                    int lo = min(c0 + MK_WAVE, m), hi = m;
                    while (lo < hi) {
                        const int mid = lo + ((hi - lo) >> 1);
                        if ((unsigned)(a[mid] >> 32) <= bits) lo = mid + 1; else hi = mid;
                    }
                    e = lo;
                }
                const unsigned lab = (unsigned)key;
                if (lab < (unsigned)K) {
                    atomicAdd(&s_r2[lab], (mk_u64)(2 * Z + s + e + 1));
                    atomicAdd(&s_nnz[lab], 1);
                }
                if (head && e - s > 1) {
                    const mk_u64 t = (mk_u64)(e - s);
                    atomicAdd(s_ties, t * t * t - t);
                }
            }
        }
    }
    __syncthreads();
    if (tid < K) {
        const long long Zr = Z + z0;                     // the run of zeros
        r2[tid] = (long long)s_r2[tid] + (long long)(nk[tid] - s_nnz[tid]) * (Zr + 1);
        nnz_k[tid] = s_nnz[tid];
        double sum = 0.0;
        for (int l = 0; l < MK_WAVE; ++l) sum += acc[l * Kp + tid];
        vsum[tid] = sum;
        if (tid == 0) *ties = (long long)*s_ties + Zr * Zr * Zr - Zr;
    }
    __syncthreads();
}

// dynamic LDS: MK_CAP keys, then 64 * (K | 1) doubles
#define MK_LDS_BYTES(K) (sizeof(mk_u64) * MK_CAP + sizeof(double) * MK_WAVE * ((K) | 1))

__global__ void __launch_bounds__(MK_THREADS) k_mk_ranksum(const long long *colptr, const int *ridx, const float *v,
                                                           const int *tp_off, const int *labels, const int *nk, int T, int G,
                                                           int K, int *queue_n, int *queue, long long *r2, long long *ties,
                                                           int *nnz_k, double *vsum) {
    extern __shared__ mk_u64 mk_lds[];
    __shared__ mk_u64 s_r2[MK_MAX_K];
    __shared__ int s_nnz[MK_MAX_K];
    __shared__ mk_u64 s_ties;
    const int item = blockIdx.x;
    const int t = item / G, g = item % G;
    const long long lo = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
    const long long hi = csc_walk_lower_bound(ridx, lo, colptr[g + 1], tp_off[t + 1]);
    const long long len = hi - lo;
    if (len > MK_CAP) {                                  // uniform over the workgroup
        if (threadIdx.x == 0) queue[atomicAdd(queue_n, 1)] = item;
        return;
    }
    const int m = (int)len;
    int P = 4;
    while (P < m) P <<= 1;
    if (m > 1) {
        for (int i = threadIdx.x; i < P; i += MK_THREADS) mk_lds[i] = i < m ? mk_key(v, ridx, labels, lo + i) : ~0ull;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) mk_stage(mk_lds, P, k, k >> 1, 0);
    } else {
        if (threadIdx.x == 0 && m == 1) mk_lds[0] = mk_key(v, ridx, labels, lo);
        __syncthreads();
    }
    mk_reduce_sorted(mk_lds, m, tp_off[t + 1] - tp_off[t], K, nk + (long long)t * K, (double *)(mk_lds + MK_CAP), s_r2, s_nnz,
                     &s_ties, r2 + (long long)item * K, ties + item, nnz_k + (long long)item * K, vsum + (long long)item * K);
}

// The queued segments, `gridDim.x` workgroups with one slab of `slab` keys each.
__global__ void __launch_bounds__(MK_THREADS) k_mk_ranksum_long(const long long *colptr, const int *ridx, const float *v,
                                                                const int *tp_off, const int *labels, const int *nk, int T,
                                                                int G, int K, const int *queue_n, const int *queue,
                                                                mk_u64 *slabs, long long slab, long long *r2, long long *ties,
                                                                int *nnz_k, double *vsum) {
    extern __shared__ mk_u64 mk_lds[];
    __shared__ mk_u64 s_r2[MK_MAX_K];
    __shared__ int s_nnz[MK_MAX_K];
    __shared__ mk_u64 s_ties;
    mk_u64 *gbuf = slabs + (long long)blockIdx.x * slab;
    const int count = *queue_n;
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const int item = queue[q];
        const int t = item / G, g = item % G;
        const long long lo = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
        const long long hi = csc_walk_lower_bound(ridx, lo, colptr[g + 1], tp_off[t + 1]);
        const long long m = hi - lo;
        long long P = 2 * MK_CAP;
        while (P < m) P <<= 1;
        if (P > slab) continue;                          // a time point longer than the caller sized the slabs for
        // chunks of MK_CAP: stages 2 .. MK_CAP in LDS
        for (long long c = 0; c < P; c += MK_CAP) {
            for (int i = threadIdx.x; i < MK_CAP; i += MK_THREADS)
                mk_lds[i] = c + i < m ? mk_key(v, ridx, labels, lo + c + i) : ~0ull;
            __syncthreads();
            for (int k = 2; k <= MK_CAP; k <<= 1) mk_stage(mk_lds, MK_CAP, k, k >> 1, c);
            for (int i = threadIdx.x; i < MK_CAP; i += MK_THREADS) gbuf[c + i] = mk_lds[i];
            __syncthreads();
        }
        // stages 2 MK_CAP .. P: the strides >= MK_CAP in global memory, the rest per chunk in LDS
        for (long long k = 2 * MK_CAP; k <= P; k <<= 1) {
            for (long long j = k >> 1; j >= MK_CAP; j >>= 1) {
                for (long long p = threadIdx.x; p < P / 2; p += MK_THREADS) {
                    const long long i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                    const mk_u64 x = gbuf[i], y = gbuf[i | j];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) { gbuf[i] = y; gbuf[i | j] = x; }
                }
                __syncthreads();
            }
            for (long long c = 0; c < P; c += MK_CAP) {
                for (int i = threadIdx.x; i < MK_CAP; i += MK_THREADS) mk_lds[i] = gbuf[c + i];
                __syncthreads();
                mk_stage(mk_lds, MK_CAP, k, MK_CAP >> 1, c);
                for (int i = threadIdx.x; i < MK_CAP; i += MK_THREADS) gbuf[c + i] = mk_lds[i];
                __syncthreads();
            }
        }
        mk_reduce_sorted(gbuf, (int)m, tp_off[t + 1] - tp_off[t], K, nk + (long long)t * K, (double *)(mk_lds + MK_CAP), s_r2,
                         s_nnz, &s_ties, r2 + (long long)item * K, ties + item, nnz_k + (long long)item * K,
                         vsum + (long long)item * K);
    }
}

// ---------------------------------------------------------------- U1, score, p
__global__ void __launch_bounds__(MK_THREADS) k_mk_finish(const long long *r2, const long long *ties, const int *tp_off,
                                                          const int *nk, int T, int G, int K, double *u1, double *score,
                                                          double *pval) {
    const long long i = (long long)blockIdx.x * MK_THREADS + threadIdx.x;
    if (i >= (long long)T * G * K) return;
    const int k = (int)(i % K);
    const long long tg = i / K;
    const int t = (int)(tg / G);
    const long long n = tp_off[t + 1] - tp_off[t], n1 = nk[t * K + k], n2 = n - n1;
    const long long d2 = r2[i] - n1 * (n1 + 1);          // 2 U1
    const long long dd = d2 - n1 * n2;                   // 2 (U1 - mu)
    const long long br = (n + 1) * n * (n - 1) - ties[tg];
    double sc = 0.0, p = 1.0;
    if (n1 > 0 && n2 > 0 && br > 0 && dd != 0) {
        const double var = (double)(n1 * n2) * (double)br / (12.0 * (double)n * (double)(n - 1));
        const double d = 0.5 * (double)dd;
        sc = (d - (d > 0.0 ? 0.5 : -0.5)) / sqrt(var);
        p = fmin(1.0, erfc(fabs(sc) * M_SQRT1_2));
    }
    u1[i] = 0.5 * (double)d2;
    score[i] = sc;
    pval[i] = p;
}

// ---------------------------------------------------------------- C ABI (include/spadot_model.h)
static int mk_long_groups(int T, int G, long long slab) {
    long long w = MK_SLAB_BYTES / (slab * (long long)sizeof(mk_u64));
    if (w > MK_MAX_LONG) w = MK_MAX_LONG;
    if (w > (long long)T * G) w = (long long)T * G;
    return w < 1 ? 1 : (int)w;
}

static long long mk_queue_bytes(int T, int G) {
    const long long b = MK_HEAD + (long long)sizeof(int) * T * G;
    return (b + 255) / 256 * 256;
}

extern "C" {

int spadot_mk_lds_capacity(void) { return MK_CAP; }

long long spadot_mk_ranksum_scratch_bytes(int T, int G, int nmax) {
    if (T <= 0 || G <= 0 || nmax < 0 || (long long)T * G > 0x7fffffffll) return -22;
    if (nmax > MK_MAX_N) return -7;
    long long bytes = mk_queue_bytes(T, G);
    if (nmax > MK_CAP) {
        const long long slab = mk_pow2(nmax);
        bytes += (long long)mk_long_groups(T, G, slab) * slab * (long long)sizeof(mk_u64);
    }
    return bytes;
}

int spadot_mk_lognorm(const int *ridx, const float *val, const double *total, long long nnz, double target, float *v,
                      void *stream) {
    if (!ridx || !val || !total || !v || nnz < 0) return -22;
    if (nnz == 0) return 0;
    const long long blocks = (nnz + MK_THREADS - 1) / MK_THREADS;
    if (blocks > 0x7fffffffll) return -22;
    hipLaunchKernelGGL(k_mk_lognorm, dim3((unsigned)blocks), dim3(MK_THREADS), 0, (hipStream_t)stream, ridx, val, total, nnz,
                       target, v);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_mk_ranksum(const long long *colptr, const int *ridx, const float *v, const int *tp_off, const int *labels,
                      const int *nk, int T, int G, int K, int nmax, void *scratch, long long scratch_bytes, long long *r2,
                      long long *ties, int *nnz_k, double *vsum, void *stream) {
    if (!colptr || !ridx || !v || !tp_off || !labels || !nk || !scratch || !r2 || !ties || !nnz_k || !vsum || T <= 0 ||
        G <= 0 || K <= 0 || nmax < 0)
        return -22;
    if (K > MK_MAX_K || nmax > MK_MAX_N) return -7;
    const long long need = spadot_mk_ranksum_scratch_bytes(T, G, nmax);
    if (need < 0 || scratch_bytes < need) return -22;
    hipStream_t st = (hipStream_t)stream;
    int *queue_n = (int *)scratch;
    int *queue = (int *)((char *)scratch + MK_HEAD);
    if (hipMemsetAsync(queue_n, 0, MK_HEAD, st) != hipSuccess) return -5;
    hipLaunchKernelGGL(k_mk_ranksum, dim3((unsigned)((long long)T * G)), dim3(MK_THREADS), MK_LDS_BYTES(K), st, colptr, ridx, v,
                       tp_off, labels, nk, T, G, K, queue_n, queue, r2, ties, nnz_k, vsum);
    if (hipGetLastError() != hipSuccess) return -5;
    if (nmax > MK_CAP) {
        const long long slab = mk_pow2(nmax);
        mk_u64 *slabs = (mk_u64 *)((char *)scratch + mk_queue_bytes(T, G));
        hipLaunchKernelGGL(k_mk_ranksum_long, dim3((unsigned)mk_long_groups(T, G, slab)), dim3(MK_THREADS), MK_LDS_BYTES(K), st,
                           colptr, ridx, v, tp_off, labels, nk, T, G, K, queue_n, queue, slabs, slab, r2, ties, nnz_k, vsum);
        if (hipGetLastError() != hipSuccess) return -5;
    }
    return 0;
}

int spadot_mk_finish(const long long *r2, const long long *ties, const int *tp_off, const int *nk, int T, int G, int K,
                     double *u1, double *score, double *pval, void *stream) {
    if (!r2 || !ties || !tp_off || !nk || !u1 || !score || !pval || T <= 0 || G <= 0 || K <= 0) return -22;
    if (K > MK_MAX_K) return -7;
    const long long blocks = ((long long)T * G * K + MK_THREADS - 1) / MK_THREADS;
    if (blocks > 0x7fffffffll) return -22;
    hipLaunchKernelGGL(k_mk_finish, dim3((unsigned)blocks), dim3(MK_THREADS), 0, (hipStream_t)stream, r2, ties, tp_off, nk, T, G,
                       K, u1, score, pval);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
