// cooccur.hip -- co-occurrence counts of many (spot set, labeling, thresholds) problems in one launch (gfx950, wave64;
// DESIGN 7i).  The definition is restated in numpy in tests/cooccur_ref.py.
//
// A problem is n spots with fp64 coordinates (x, y), a labeling in 0 .. K-1 and B squared thresholds r2[0] < .. < r2[B-1]; its
// counts are N[a, b, t] = #{ordered pairs (i, j), i != j : lab[i] = a, lab[j] = b, d2(i, j) <= r2[t]} with
// d2 = fl(fl(dx dx) + fl(dy dy)): five correctly rounded fp64 operations, NO fused multiply-add (co_d2 below is the only
// place where a distance is formed).  The host has ordered the problem's spots by (label, index): xy holds the gathered
// coordinates and the descriptor the cluster offsets.  No n x n array exists anywhere.
//
// k_cooccur<BP>   one 256-thread workgroup per (problem, block of 256 sorted positions); a thread owns one spot.  For every
//                 neighbour label b the spots of b stream through LDS, 256 (x, y) pairs at a time, every lane reading the
//                 same address (a broadcast); a thread keeps BP int32 counters in registers (BP: the call's B_max rounded up
//                 to 16; every index is a compile-time constant, nothing goes to scratch), cnt[t] += (d2 <= r2[t]).  The
//                 thresholds of a problem are padded with -1: no d2 is <= -1, so a padded threshold never counts.  When
//                 label b ends, the threads add their counters by their own label a into an LDS table [K][BP] of 64-bit
//                 integers and the workgroup adds the rows it holds onto the int64 output [a][b][t], which the call has
//                 zeroed.  Only integers are added, and integer addition commutes: the result does not depend on the order
//                 the atomics retire in -- exact, the same alone, in any batch, run after run.  No floating-point sum.
// k_cooccur_null<BP>  the same workgroup, tile, counters, table and adds for the random-labelling null (restated
//                 in tests/cooccur_null_ref.py): one workgroup per (block of 256 sorted positions, pattern, problem).  Pattern 0
//                 is the observed labeling; pattern s >= 1 keeps the labels on the sorted positions and hands position j the
//                 coordinates of position pi^-1(j), pi the Feistel permutation (seed, g, first + s - 1, n) of the neighbors and
//                 ripley stages, evaluated per element as the spot and the tile are read: no permuted copy of xy, no table of pi.
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/spadot_model.h"
#include "feistel_perm.h"

#define CO_THREADS 256
#define CO_MAX_K 32
#define CO_MAX_B 64
#define CO_GRANULE 16              // thresholds per problem are padded to a multiple of this
#define CO_DESC 40                 // int64 columns of a problem's descriptor (include/spadot_model.h)
#define CO_MAX_P 65535             // problems per launch: gridDim.y
#define CO_MAX_N 2147483391        // spots per problem: int32 positions, and j0 + 256 must not overflow (2^31 - 1 - 256)
#define CO_DESC_G 37               // the null's problem number g: K <= 32 leaves the columns 37 .. 39 free
#define CO_MAX_Y 65535             // patterns per launch of the null: gridDim.y (its problems are gridDim.z)
#define CO_MAX_G 2147483647ll      // problem numbers, as the graph ids of spadot_nhood_counts

// the squared distance of the definition: two multiplications and three additions, each rounded once
__device__ __forceinline__ double co_d2(double xi, double yi, double xj, double yj) {
#pragma clang fp contract(off)
    const double dx = xi - xj, dy = yi - yj;
    const double sx = dx * dx, sy = dy * dy;
    return sx + sy;
}

template <int BP>
__global__ void __launch_bounds__(CO_THREADS) k_cooccur(const double2 *__restrict__ xy, const long long *__restrict__ desc,
                                                         const double *__restrict__ r2, int K_max, int B_max,
                                                         unsigned long long *__restrict__ out) {
    __shared__ double2 tile[CO_THREADS];
    __shared__ unsigned long long tab[CO_MAX_K * BP];
    const int p = blockIdx.y, tid = threadIdx.x;
    const long long *d = desc + (long long)p * CO_DESC;
    const long long nl = d[1];
    const int q0 = blockIdx.x * CO_THREADS;
    if (q0 >= nl) return;                                // uniform: the grid is sized for the largest problem
    // the descriptor is refused on the host before the launch; the clamps keep every access inside its array
    const int n = (int)nl;
    const int K = min(max((int)d[2], 1), min(K_max, CO_MAX_K));
    const int B = min((int)d[3], min(B_max, BP));
    const double2 *pts = xy + d[0];
    const double *th = r2 + (long long)p * BP;
    const int q = q0 + tid;
    const bool on = q < n;
    const double2 me = pts[on ? q : n - 1];              // idle lanes follow a valid spot and add nothing
    int a = -1;
    for (int k = 0; k < K; ++k)
        if (on && q >= d[4 + k] && q < d[5 + k]) a = k;
    for (int i = tid; i < CO_MAX_K * BP; i += CO_THREADS) tab[i] = 0ull;
    int cnt[BP];
#pragma unroll
    for (int t = 0; t < BP; ++t) cnt[t] = 0;

    for (int b = 0; b < K; ++b) {
        const int lo = (int)min(max(d[4 + b], 0ll), nl), hi = (int)min(max(d[5 + b], (long long)lo), nl);
        if (lo == hi) continue;                          // uniform: a label value without spots
        for (int j0 = lo; j0 < hi; j0 += CO_THREADS) {
            const int m = min(CO_THREADS, hi - j0);
            __syncthreads();                             // the previous tile is read
            if (tid < m) tile[tid] = pts[j0 + tid];
            __syncthreads();
            int jj = 0;
            for (; jj + 4 <= m; jj += 4) {               // four spots per pass over the thresholds
                double e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double2 v = tile[jj + u];
                    const double s = co_d2(me.x, me.y, v.x, v.y);
                    e[u] = j0 + jj + u == q ? INFINITY : s;                  // a spot is never its own neighbour
                }
#pragma unroll
                for (int t = 0; t < BP; ++t) {
                    const double r = th[t];
                    cnt[t] += (int)(e[0] <= r) + (int)(e[1] <= r) + (int)(e[2] <= r) + (int)(e[3] <= r);
                }
            }
            for (; jj < m; ++jj) {
                const double2 v = tile[jj];
                const double s = co_d2(me.x, me.y, v.x, v.y);
                const double e = j0 + jj == q ? INFINITY : s;
#pragma unroll
                for (int t = 0; t < BP; ++t) cnt[t] += (int)(e <= th[t]);
            }
        }
        // label b is complete: the threads' counters into the table by their own label, the table onto the output
#pragma unroll
        for (int t = 0; t < BP; ++t) {
            if (a >= 0 && cnt[t] != 0) atomicAdd(&tab[a * BP + t], (unsigned long long)cnt[t]);
            cnt[t] = 0;
        }
        __syncthreads();
        for (int i = tid; i < K * BP; i += CO_THREADS) {
            const unsigned long long v = tab[i];
            if (v != 0ull) {
                const int aa = i / BP, t = i - aa * BP;
                tab[i] = 0ull;                           // read again only after the next tile's two barriers
                if (t < B) atomicAdd(out + ((((long long)p * K_max + aa) * K_max + b) * B_max + t), v);
            }
        }
    }
}

template <int BP>
static int co_launch(dim3 grid, hipStream_t st, const double *xy, const long long *desc, const double *r2, int K_max,
                     int B_max, long long *out) {
    hipLaunchKernelGGL(k_cooccur<BP>, grid, dim3(CO_THREADS), 0, st, reinterpret_cast<const double2 *>(xy), desc, r2, K_max,
                       B_max, reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int spadot_cooccur_counts(const double *xy, const long long *desc_host, const long long *desc_dev,
                                     const double *r2_host, const double *r2_dev, int P, int K_max, int B_max,
                                     long long *out, void *stream) {
    if (!xy || !desc_host || !desc_dev || !r2_host || !r2_dev || !out || P <= 0) return -22;
    if (K_max < 1 || K_max > CO_MAX_K || B_max < 1 || B_max > CO_MAX_B || P > CO_MAX_P) return -7;
    const int BP = (B_max + CO_GRANULE - 1) / CO_GRANULE * CO_GRANULE;
    long long first = 0, n_max = 0;
    for (int p = 0; p < P; ++p) {
        const long long *d = desc_host + (long long)p * CO_DESC;
        const long long n = d[1], K = d[2], B = d[3];
        if (n < 1 || d[0] != first) return -22;          // the problems lie back to back in xy
        if (n > CO_MAX_N || K < 1 || K > K_max || B < 1 || B > B_max) return -7;
        if (d[4] != 0 || d[4 + K] != n) return -22;
        for (int k = 0; k < K; ++k)
            if (d[5 + k] < d[4 + k]) return -22;
        const double *r = r2_host + (long long)p * BP;
        for (int t = 0; t < BP; ++t) {
            if (t >= B) {
                if (r[t] != -1.0) return -22;            // the padding
            } else if (!std::isfinite(r[t]) || r[t] < 0.0 || (t > 0 && !(r[t] > r[t - 1]))) {
                return -7;
            }
        }
        first += n;
        if (n > n_max) n_max = n;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, sizeof(long long) * (size_t)P * K_max * K_max * B_max, st) != hipSuccess) return -5;
    const dim3 grid((unsigned)((n_max + CO_THREADS - 1) / CO_THREADS), (unsigned)P);
    switch (BP) {
        case 16: return co_launch<16>(grid, st, xy, desc_dev, r2_dev, K_max, B_max, out);
        case 32: return co_launch<32>(grid, st, xy, desc_dev, r2_dev, K_max, B_max, out);
        case 48: return co_launch<48>(grid, st, xy, desc_dev, r2_dev, K_max, B_max, out);
        default: return co_launch<64>(grid, st, xy, desc_dev, r2_dev, K_max, B_max, out);
    }
}

template <int BP>
__global__ void __launch_bounds__(CO_THREADS) k_cooccur_null(const double2 *__restrict__ xy, const long long *__restrict__ desc,
                                                              const double *__restrict__ r2, int K_max, int B_max, int observed,
                                                              unsigned long long first, unsigned long long seed,
                                                              unsigned long long *__restrict__ out) {
    __shared__ double2 tile[CO_THREADS];
    __shared__ unsigned long long tab[CO_MAX_K * BP];
    const int p = blockIdx.z, y = blockIdx.y, tid = threadIdx.x;
    const long long *d = desc + (long long)p * CO_DESC;
    const long long nl = d[1];
    const int q0 = blockIdx.x * CO_THREADS;
    if (q0 >= nl) return;                                // uniform: the grid is sized for the largest problem
    // the descriptor is refused on the host before the launch; the clamps keep every access inside its array
    const int n = (int)nl;
    const int K = min(max((int)d[2], 1), min(K_max, CO_MAX_K));
    const int B = min((int)d[3], min(B_max, BP));
    const double2 *pts = xy + d[0];
    const double *th = r2 + (long long)p * BP;
    const int s = observed ? y : y + 1;                  // the global pattern: 0 observed, s >= 1 relabeling first + s - 1
    const bool relabeled = s >= 1;                       // uniform
    NhPerm pi = {};
    if (relabeled) pi = nh_perm_setup(seed, (unsigned long long)d[CO_DESC_G], first + (unsigned long long)(s - 1), (unsigned)n);
    auto at = [&](int j) -> double2 {                    // the coordinates that sorted position j holds in this pattern, 0 <= j < n
        return pts[relabeled ? (int)ac_perm_inv(pi, (unsigned)j) : j];
    };
    const int q = q0 + tid;
    const bool on = q < n;
    const double2 me = at(on ? q : n - 1);               // idle lanes follow a valid spot and add nothing
    int a = -1;                                          // the label stays with the position
    for (int k = 0; k < K; ++k)
        if (on && q >= d[4 + k] && q < d[5 + k]) a = k;
    for (int i = tid; i < CO_MAX_K * BP; i += CO_THREADS) tab[i] = 0ull;
    int cnt[BP];
#pragma unroll
    for (int t = 0; t < BP; ++t) cnt[t] = 0;
    unsigned long long *res = out + ((long long)p * gridDim.y + y) * K_max * K_max * B_max;

    for (int b = 0; b < K; ++b) {
        const int lo = (int)min(max(d[4 + b], 0ll), nl), hi = (int)min(max(d[5 + b], (long long)lo), nl);
        if (lo == hi) continue;                          // uniform: a label value without spots
        for (int j0 = lo; j0 < hi; j0 += CO_THREADS) {
            const int m = min(CO_THREADS, hi - j0);
            __syncthreads();                             // the previous tile is read
            if (tid < m) tile[tid] = at(j0 + tid);
            __syncthreads();
            int jj = 0;
            for (; jj + 4 <= m; jj += 4) {               // four spots per pass over the thresholds
                double e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double2 v = tile[jj + u];
                    const double sq = co_d2(me.x, me.y, v.x, v.y);
                    e[u] = j0 + jj + u == q ? INFINITY : sq;                 // by position: pi is a bijection
                }
#pragma unroll
                for (int t = 0; t < BP; ++t) {
                    const double r = th[t];
                    cnt[t] += (int)(e[0] <= r) + (int)(e[1] <= r) + (int)(e[2] <= r) + (int)(e[3] <= r);
                }
            }
            for (; jj < m; ++jj) {
                const double2 v = tile[jj];
                const double sq = co_d2(me.x, me.y, v.x, v.y);
                const double e = j0 + jj == q ? INFINITY : sq;
#pragma unroll
                for (int t = 0; t < BP; ++t) cnt[t] += (int)(e <= th[t]);
            }
        }
        // label b is complete: the threads' counters into the table by their own label, the table onto the output
#pragma unroll
        for (int t = 0; t < BP; ++t) {
            if (a >= 0 && cnt[t] != 0) atomicAdd(&tab[a * BP + t], (unsigned long long)cnt[t]);
            cnt[t] = 0;
        }
        __syncthreads();
        for (int i = tid; i < K * BP; i += CO_THREADS) {
            const unsigned long long v = tab[i];
            if (v != 0ull) {
                const int aa = i / BP, t = i - aa * BP;
                tab[i] = 0ull;                           // read again only after the next tile's two barriers
                if (t < B) atomicAdd(res + (((long long)aa * K_max + b) * B_max + t), v);
            }
        }
    }
}

template <int BP>
static int co_null_launch(dim3 grid, hipStream_t st, const double *xy, const long long *desc, const double *r2, int K_max,
                          int B_max, int observed, long long first, long long seed, long long *out) {
    hipLaunchKernelGGL(k_cooccur_null<BP>, grid, dim3(CO_THREADS), 0, st, reinterpret_cast<const double2 *>(xy), desc, r2, K_max,
                       B_max, observed, (unsigned long long)first, (unsigned long long)seed,
                       reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int spadot_cooccur_null(const double *xy, const long long *desc_host, const long long *desc_dev,
                                   const double *r2_host, const double *r2_dev, int P, int K_max, int B_max, int observed,
                                   long long first, int n_perms, long long seed, long long *out, void *stream) {
    if (!xy || !desc_host || !desc_dev || !r2_host || !r2_dev || !out || P <= 0) return -22;
    if (observed != 0 && observed != 1) return -22;
    if (K_max < 1 || K_max > CO_MAX_K || B_max < 1 || B_max > CO_MAX_B || P > CO_MAX_P) return -7;
    if (n_perms < 0 || observed + n_perms < 1 || observed + n_perms > CO_MAX_Y) return -7;
    if (first < 0 || first + n_perms > (1ll << 31)) return -7;
    const int BP = (B_max + CO_GRANULE - 1) / CO_GRANULE * CO_GRANULE;
    long long spot0 = 0, n_max = 0;
    for (int p = 0; p < P; ++p) {                        // what spadot_cooccur_counts checks, and the problem number
        const long long *d = desc_host + (long long)p * CO_DESC;
        const long long n = d[1], K = d[2], B = d[3];
        if (n < 1 || d[0] != spot0) return -22;          // the problems lie back to back in xy
        if (n > CO_MAX_N || K < 1 || K > K_max || B < 1 || B > B_max) return -7;
        if (d[CO_DESC_G] < 0 || d[CO_DESC_G] > CO_MAX_G) return -7;
        if (d[4] != 0 || d[4 + K] != n) return -22;
        for (int k = 0; k < K; ++k)
            if (d[5 + k] < d[4 + k]) return -22;
        const double *r = r2_host + (long long)p * BP;
        for (int t = 0; t < BP; ++t) {
            if (t >= B) {
                if (r[t] != -1.0) return -22;            // the padding
            } else if (!std::isfinite(r[t]) || r[t] < 0.0 || (t > 0 && !(r[t] > r[t - 1]))) {
                return -7;
            }
        }
        spot0 += n;
        if (n > n_max) n_max = n;
    }
    hipStream_t st = (hipStream_t)stream;
    const int Y = observed + n_perms;
    if (hipMemsetAsync(out, 0, sizeof(long long) * (size_t)P * Y * K_max * K_max * B_max, st) != hipSuccess) return -5;
    const dim3 grid((unsigned)((n_max + CO_THREADS - 1) / CO_THREADS), (unsigned)Y, (unsigned)P);
    switch (BP) {
        case 16: return co_null_launch<16>(grid, st, xy, desc_dev, r2_dev, K_max, B_max, observed, first, seed, out);
        case 32: return co_null_launch<32>(grid, st, xy, desc_dev, r2_dev, K_max, B_max, observed, first, seed, out);
        case 48: return co_null_launch<48>(grid, st, xy, desc_dev, r2_dev, K_max, B_max, observed, first, seed, out);
        default: return co_null_launch<64>(grid, st, xy, desc_dev, r2_dev, K_max, B_max, observed, first, seed, out);
    }
}
