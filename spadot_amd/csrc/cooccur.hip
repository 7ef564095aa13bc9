// cooccur.hip -- co-occurrence counts of many (spot set, labeling, thresholds) problems in one launch (gfx950, wave64;
// DESIGN 7i).  The definition is restated in numpy in tests/cooccur_ref.py.
//
// A problem is n spots with fp64 coordinates (x, y), a labeling in 0 .. K-1 and B squared thresholds r2[0] < .. < r2[B-1]; its
// counts are N[a, b, t] = #{ordered pairs (i, j), i != j : lab[i] = a, lab[j] = b, d2(i, j) <= r2[t]} with
// d2 = fl(fl(dx dx) + fl(dy dy)): five correctly rounded fp64 operations, NO fused multiply-add (pc_d2 of pair_count.h, which
// this file shares with ripley.hip, is the only place where a distance is formed).  The host has ordered the problem's spots by
// (label, index): xy holds the gathered coordinates and the descriptor the cluster offsets.  No n x n array exists anywhere.
//
// k_cooccur<BP, NULLED>  one 256-thread workgroup per (block of 256 sorted positions, pattern, problem); a thread owns one spot.
//                 For every neighbour label b the spots of b stream through LDS, 256 (x, y) pairs at a time, every lane reading
//                 the same address (a broadcast); a thread keeps BP int32 counters in registers (BP: the call's B_max rounded up
//                 to 16; every index is a compile-time constant, nothing goes to scratch), cnt[t] += (d2 <= r2[t]).  The
//                 thresholds of a problem are padded with -1: no d2 is <= -1, so a padded threshold never counts.  When
//                 label b ends, the threads add their counters by their own label a into an LDS table [K][BP] of 64-bit
//                 integers and the workgroup adds the rows it holds onto the int64 output [a][b][t], which the call has
//                 zeroed.  Only integers are added, and integer addition commutes: the result does not depend on the order
//                 the atomics retire in -- exact, the same alone, in any batch, run after run.  No floating-point sum.
//   NULLED = false  spadot_cooccur_counts: the grid is (blocks, problems), there is one pattern, and position j holds pts[j].
//   NULLED = true   spadot_cooccur_null, the random-labelling null (restated in tests/cooccur_null_ref.py): the
//                 grid is (blocks, patterns, problems).  Pattern 0 is the observed labeling; pattern s >= 1 keeps the labels on
//                 the sorted positions and hands position j the coordinates of position pi^-1(j), pi the Feistel permutation
//                 (seed, g, first + s - 1, n) of the neighbors and ripley stages, evaluated per element as the spot and the tile
//                 are read: no permuted copy of xy, no table of pi.
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/spadot_model.h"
#include "feistel_perm.h"
#include "pair_count.h"

#define CO_DESC 40                 // int64 columns of a problem's descriptor (include/spadot_model.h)
#define CO_DESC_G 37               // the null's problem number g: K <= 32 leaves the columns 37 .. 39 free

template <int BP, bool NULLED>
__global__ void __launch_bounds__(PC_THREADS) k_cooccur(const double2 *__restrict__ xy, const long long *__restrict__ desc,
                                                         const double *__restrict__ r2, int K_max, int B_max, int observed,
                                                         unsigned long long first, unsigned long long seed,
                                                         unsigned long long *__restrict__ out) {
    __shared__ double2 tile[PC_THREADS];
    __shared__ unsigned long long tab[PC_MAX_K * BP];
    const int p = NULLED ? blockIdx.z : blockIdx.y, y = NULLED ? blockIdx.y : 0, Y = NULLED ? gridDim.y : 1, tid = threadIdx.x;
    const long long *d = desc + (long long)p * CO_DESC;
    const long long nl = d[1];
    const int q0 = blockIdx.x * PC_THREADS;
    if (q0 >= nl) return;                                // uniform: the grid is sized for the largest problem
    // the descriptor is refused on the host before the launch; the clamps keep every access inside its array
    const int n = (int)nl;
    const int K = min(max((int)d[2], 1), min(K_max, PC_MAX_K));
    const int B = min((int)d[3], min(B_max, BP));
    const double2 *pts = xy + d[0];
    const double *th = r2 + (long long)p * BP;
    const int s = observed ? y : y + 1;                  // the global pattern: 0 observed, s >= 1 relabeling first + s - 1
    const bool relabeled = NULLED && s >= 1;             // uniform
    NhPerm pi = {};
    if (relabeled) pi = nh_perm_setup(seed, (unsigned long long)d[CO_DESC_G], first + (unsigned long long)(s - 1), (unsigned)n);
    auto at = [&](int j) -> double2 {                    // the coordinates that sorted position j holds in this pattern, 0 <= j < n
        if (!NULLED) return pts[j];
        return pts[relabeled ? (int)ac_perm_inv(pi, (unsigned)j) : j];
    };
    const int q = q0 + tid;
    const bool on = q < n;
    const double2 me = at(on ? q : n - 1);               // idle lanes follow a valid spot and add nothing
    int a = -1;                                          // the label stays with the position
    for (int k = 0; k < K; ++k)
        if (on && q >= d[4 + k] && q < d[5 + k]) a = k;
    for (int i = tid; i < PC_MAX_K * BP; i += PC_THREADS) tab[i] = 0ull;
    int cnt[BP];
#pragma unroll
    for (int t = 0; t < BP; ++t) cnt[t] = 0;
    unsigned long long *res = out + ((long long)p * Y + y) * K_max * K_max * B_max;

    for (int b = 0; b < K; ++b) {
        const int lo = (int)min(max(d[4 + b], 0ll), nl), hi = (int)min(max(d[5 + b], (long long)lo), nl);
        if (lo == hi) continue;                          // uniform: a label value without spots
        for (int j0 = lo; j0 < hi; j0 += PC_THREADS) {
            const int m = min(PC_THREADS, hi - j0);
            __syncthreads();                             // the previous tile is read
            if (tid < m) tile[tid] = at(j0 + tid);
            __syncthreads();
            int jj = 0;
            for (; jj + 4 <= m; jj += 4) {               // four spots per pass over the thresholds
                pc_pass4<BP>(cnt, th, me, tile + jj, j0 + jj, q);                               // by position: pi is a bijection
            }
            for (; jj < m; ++jj) pc_count1<BP>(cnt, th, pc_dist(me, tile[jj], j0 + jj, q));
        }
        // label b is complete: the threads' counters into the table by their own label, the table onto the output
        pc_flush_counters<BP>(cnt, tab, a);
        __syncthreads();
        pc_flush_table<BP>(tab, K, B, res + (long long)b * B_max, (long long)K_max * B_max);
    }
}

// what both entries refuse about the problems of a call, and its largest problem; with_g: the null's problem numbers as well
static int co_check(const long long *desc_host, const double *r2_host, int P, int K_max, int B_max, bool with_g, long long *n_max) {
    const int BP = pc_padded(B_max);
    long long first = 0;
    *n_max = 0;
    for (int p = 0; p < P; ++p) {
        const long long *d = desc_host + (long long)p * CO_DESC;
        const long long n = d[1], K = d[2], B = d[3];
        if (n < 1 || d[0] != first) return -22;          // the problems lie back to back in xy
        if (n > PC_MAX_N || K < 1 || K > K_max || B < 1 || B > B_max) return -7;
        if (with_g && (d[CO_DESC_G] < 0 || d[CO_DESC_G] > PC_MAX_G)) return -7;
        int rc = pc_offsets(d + 4, K, n);
        if (!rc) rc = pc_thresholds(r2_host + (long long)p * BP, B, BP);
        if (rc) return rc;
        first += n;
        if (n > *n_max) *n_max = n;
    }
    return 0;
}

// the checks of the problems, the zeroed output [P, Y, K_max, K_max, B_max] and the launch of both entries
template <bool NULLED>
static int co_run(const double *xy, const long long *desc_host, const long long *desc_dev, const double *r2_host,
                  const double *r2_dev, int P, int K_max, int B_max, int observed, long long first, int Y, long long seed,
                  long long *out, hipStream_t st) {
    long long n_max;
    const int rc = co_check(desc_host, r2_host, P, K_max, B_max, NULLED, &n_max);
    if (rc) return rc;
    if (hipMemsetAsync(out, 0, sizeof(long long) * (size_t)P * Y * K_max * K_max * B_max, st) != hipSuccess) return -5;
    const unsigned blocks = (unsigned)((n_max + PC_THREADS - 1) / PC_THREADS);
    const dim3 grid = NULLED ? dim3(blocks, (unsigned)Y, (unsigned)P) : dim3(blocks, (unsigned)P);
    return pc_dispatch(pc_padded(B_max), [&](auto bp) {
        hipLaunchKernelGGL((k_cooccur<decltype(bp)::value, NULLED>), grid, dim3(PC_THREADS), 0, st,
                           reinterpret_cast<const double2 *>(xy), desc_dev, r2_dev, K_max, B_max, observed,
                           (unsigned long long)first, (unsigned long long)seed, reinterpret_cast<unsigned long long *>(out));
        return hipGetLastError() == hipSuccess ? 0 : -5;
    });
}

extern "C" int spadot_cooccur_counts(const double *xy, const long long *desc_host, const long long *desc_dev,
                                     const double *r2_host, const double *r2_dev, int P, int K_max, int B_max,
                                     long long *out, void *stream) {
    if (!xy || !desc_host || !desc_dev || !r2_host || !r2_dev || !out || P <= 0) return -22;
    if (K_max < 1 || K_max > PC_MAX_K || B_max < 1 || B_max > PC_MAX_B || P > PC_MAX_GRID) return -7;
    return co_run<false>(xy, desc_host, desc_dev, r2_host, r2_dev, P, K_max, B_max, 1, 0, 1, 0, out, (hipStream_t)stream);
}

extern "C" int spadot_cooccur_null(const double *xy, const long long *desc_host, const long long *desc_dev,
                                   const double *r2_host, const double *r2_dev, int P, int K_max, int B_max, int observed,
                                   long long first, int n_perms, long long seed, long long *out, void *stream) {
    if (!xy || !desc_host || !desc_dev || !r2_host || !r2_dev || !out || P <= 0) return -22;
    if (observed != 0 && observed != 1) return -22;
    if (K_max < 1 || K_max > PC_MAX_K || B_max < 1 || B_max > PC_MAX_B || P > PC_MAX_GRID) return -7;
    if (n_perms < 0 || observed + n_perms < 1 || observed + n_perms > PC_MAX_GRID) return -7;
    if (first < 0 || first + n_perms > (1ll << 31)) return -7;
    return co_run<true>(xy, desc_host, desc_dev, r2_host, r2_dev, P, K_max, B_max, observed, first, observed + n_perms, seed, out,
                        (hipStream_t)stream);
}
