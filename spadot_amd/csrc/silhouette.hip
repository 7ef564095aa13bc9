// silhouette.hip -- silhouette coefficients of many (data set, labeling) problems in one launch (gfx950, wave64), pinned to
// sklearn.metrics.silhouette_samples.
//
// A problem is a set of n points in d dimensions (fp64) and a labeling with K label values.  The host has ordered the
// problem's points by (label, index): order[j] is the set's row at sorted position j and coff[k] .. coff[k + 1] are the sorted
// positions of cluster k.  No n x n matrix exists anywhere.
//
// k_silhouette<DP>   one 256-thread workgroup per (problem, block of 256 sorted positions); a thread owns one point and keeps
//                    its coordinates in DP registers (d padded with zeros to a multiple of 4: every index is a compile-time
//                    constant, nothing goes to scratch, and a padded coordinate adds an exact 0 to the square sum).  The
//                    problem's points stream through LDS in sorted order, 256 at a time; every lane reads the same address
//                    (a broadcast, conflict-free).  Cluster boundaries are uniform over the workgroup, so the running sum
//                    S_i(k) of distances to cluster k is ONE register: when the cluster ends it is folded into a_i (own
//                    cluster) or into the running minimum b_i / nearest_i (first minimum wins: strict <, k ascending), and
//                    reset.  Every sum has one fixed order (sorted position ascending), there are no atomics: a problem's
//                    result has the same bits whatever else the launch holds, run after run.
//                    dist = sqrt(sum_c (x_ic - x_jc)^2) in the direct form, c ascending, fp64, IEEE sqrt and division.
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/spadot_model.h"

#define SIL_THREADS 256
#define SIL_MAX_K 32
#define SIL_MAX_D 32
#define SIL_MAX_P 65535            // problems per launch: gridDim.y
#define SIL_MAX_N 2147483391       // points per set: int32 positions, and q0 + 255 must not overflow (2^31 - 1 - 256)

template <int DP>
__global__ void __launch_bounds__(SIL_THREADS) k_silhouette(const double *__restrict__ x, int d,
                                                             const long long *__restrict__ prob,
                                                             const int *__restrict__ order, const int *__restrict__ coff,
                                                             double *__restrict__ a_out, double *__restrict__ b_out,
                                                             int *__restrict__ near_out, double *__restrict__ s_out) {
    __shared__ double tile[SIL_THREADS * DP];
    const int p = blockIdx.y, tid = threadIdx.x;
    const long long xoff = prob[4 * p], ooff = prob[4 * p + 1];
    const int n = (int)prob[4 * p + 2], K = min((int)prob[4 * p + 3], SIL_MAX_K);
    const int q0 = blockIdx.x * SIL_THREADS;
    if (q0 >= n) return;                                 // uniform: the grid is sized for the largest set
    const int *cf = coff + p * (SIL_MAX_K + 1);          // uniform reads; the tile alone is in LDS (40 KiB at d = 20)
    const int *ord = order + ooff;
    const double *xs = x + xoff * d;
    const int q = q0 + tid;
    const bool on = q < n;
    const int row = ord[on ? q : n - 1];                 // idle lanes follow a valid point and write nothing
    double xr[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) xr[c] = c < d ? xs[(long long)row * d + c] : 0.0;

    double S = 0.0, a = 0.0, b = INFINITY;
    int nearest = -1, own_n = 0, k = 0;
    // cluster k is complete: into a (own cluster) or the running minimum of the other clusters' means
    auto fold = [&](int kk, int lo, int hi) {
        const int nk = hi - lo;
        if (nk > 0) {
            if (q >= lo && q < hi) {
                own_n = nk;
                a = nk > 1 ? S / (double)(nk - 1) : 0.0;
            } else {
                const double m = S / (double)nk;
                if (m < b) { b = m; nearest = kk; }
            }
        }
        S = 0.0;
    };
    for (int j0 = 0; j0 < n; j0 += SIL_THREADS) {
        const int cnt = min(SIL_THREADS, n - j0);
        __syncthreads();                                 // the previous tile is read
        for (int e = tid; e < cnt * DP; e += SIL_THREADS) {
            const int j = e / DP, c = e % DP;
            tile[e] = c < d ? xs[(long long)ord[j0 + j] * d + c] : 0.0;
        }
        __syncthreads();
        int j = j0;
        const int jend = j0 + cnt;
        while (j < jend) {
            while (k < K - 1 && cf[k + 1] <= j) { fold(k, cf[k], cf[k + 1]); ++k; }
            const int send = k < K - 1 ? min(cf[k + 1], jend) : jend;        // coff[K] = n: the last cluster takes the rest
#pragma unroll 1                                         // one point in flight: d = 20 stays within 128 VGPRs
            for (; j < send; ++j) {
                const double *pt = tile + (j - j0) * DP;
                double sq = 0.0;
#pragma unroll
                for (int c = 0; c < DP; c += 2) {
                    const double2 v = *reinterpret_cast<const double2 *>(pt + c);
                    const double d0 = xr[c] - v.x, d1 = xr[c + 1] - v.y;
                    sq = fma(d0, d0, sq);
                    sq = fma(d1, d1, sq);
                }
                S += sqrt(sq);
            }
        }
    }
    for (; k < K; ++k) fold(k, cf[k], cf[k + 1]);
    if (!on) return;
    double s = 0.0;
    if (own_n > 1) {
        const double m = fmax(a, b);
        s = m > 0.0 ? (b - a) / m : 0.0;                 // b = inf (no other cluster): NaN, an undefined labeling
    }
    const long long o = ooff + row;
    a_out[o] = a;
    b_out[o] = b;
    near_out[o] = nearest;
    s_out[o] = s;
}

template <int DP>
static int sil_launch(dim3 grid, hipStream_t st, const double *x, int d, const long long *prob, const int *order,
                      const int *coff, double *a, double *b, int *nearest, double *s) {
    hipLaunchKernelGGL(k_silhouette<DP>, grid, dim3(SIL_THREADS), 0, st, x, d, prob, order, coff, a, b, nearest, s);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int spadot_silhouette(const double *x, int d, int P, const long long *prob, const int *order, const int *coff,
                                 int n_max, int k_min, int k_max, double *a, double *b, int *nearest, double *s,
                                 void *stream) {
    if (!x || !prob || !order || !coff || !a || !b || !nearest || !s || P <= 0 || n_max <= 0) return -22;
    if (d < 1 || d > SIL_MAX_D || k_min < 2 || k_max > SIL_MAX_K || k_min > k_max || P > SIL_MAX_P || n_max > SIL_MAX_N)
        return -7;
    const dim3 grid((unsigned)((n_max + SIL_THREADS - 1) / SIL_THREADS), (unsigned)P);
    hipStream_t st = (hipStream_t)stream;
    switch ((d + 3) / 4) {
        case 1: return sil_launch<4>(grid, st, x, d, prob, order, coff, a, b, nearest, s);
        case 2: return sil_launch<8>(grid, st, x, d, prob, order, coff, a, b, nearest, s);
        case 3: return sil_launch<12>(grid, st, x, d, prob, order, coff, a, b, nearest, s);
        case 4: return sil_launch<16>(grid, st, x, d, prob, order, coff, a, b, nearest, s);
        case 5: return sil_launch<20>(grid, st, x, d, prob, order, coff, a, b, nearest, s);
        case 6: return sil_launch<24>(grid, st, x, d, prob, order, coff, a, b, nearest, s);
        case 7: return sil_launch<28>(grid, st, x, d, prob, order, coff, a, b, nearest, s);
        default: return sil_launch<32>(grid, st, x, d, prob, order, coff, a, b, nearest, s);
    }
}
