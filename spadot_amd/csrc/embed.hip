// embed.hip -- t-SNE of the latents with exact repulsion (gfx950, wave64): the k nearest neighbours of every point in
// up to 32 dimensions, the conditional affinities of sklearn's perplexity search, and the iterations of sklearn's optimiser with
// the repulsive force summed over ALL pairs in fp64.  Every entry takes a table of problems, so that the time points of a run are
// one launch; a problem's bits do not depend on what else the launch holds, run after run.
//
// k_latent_knn<DP>     one 64-thread workgroup per (problem, 64 queries); a thread owns one query and keeps its coordinates in DP
//                      registers (d padded with zeros to a multiple of 4, as k_silhouette).  The candidates stream through LDS in
//                      tiles of 64 (every lane reads the same address: a broadcast).  A thread's list of the k best so far is a
//                      column [slot][lane] of an LDS table, ordered by (squared distance, index): a candidate that beats the
//                      worst entry is put in its place by shifting (candidates come in ascending index, so a tie goes behind the
//                      entries it ties with).  12 k_max 64 bytes: 115 200 at k = 150, beside a tile of 16 KiB at d = 32.
//                      The squared distance is UNFUSED: sum_c (x_ic - x_jc)^2 with c ascending, every subtraction, product and
//                      addition rounded once (no fused multiply-add), so that numpy restates it bit for bit.
// k_tsne_aff           one wavefront per row: lane l holds the entries l, l + 64, l + 128 of the row; 200 steps of the search for
//                      beta, every sum a lane-local sum in ascending entry order and then a butterfly over the lanes (one fixed
//                      order; every lane ends with the same bits).
// k_tsne_repulse<QP>   one 256-thread workgroup per (problem, block of 256 QP query points, slice of the partner range); Y streams
//                      through LDS in tiles of 256 double2 (broadcast reads); a thread keeps z, r_x, r_y of its QP points in
//                      registers and adds its partners in ascending order.  The partials of a slice go to scratch.
// k_tsne_rows          one thread per point: the partials of its slices in slice order, the attraction over its CSR row in stored
//                      order and the row's part of the KL sum; the workgroup adds z and the KL parts in a fixed tree per block.
// k_tsne_apply         one thread per point: Z (the blocks in ascending order), the gradient, sklearn's gains / update rule and
//                      the next Y; thread 0 of block 0 completes kl[it].
// No atomics and no floating-point sum whose order depends on scheduling.  Everything that the numpy restatement repeats bit for
// bit (the distances of the neighbour search, the update rule) is written under `#pragma clang fp contract(off)`.
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/spadot_model.h"
#include "pair_count.h"
#include "per_device.h"

#define EMB_DESC 10                // columns of a row of the problem table (include/spadot_model.h)
#define EMB_MAX_D 32
#define EMB_MAX_K 150              // floor(3 * 50)
#define EMB_MAX_P 65535            // problems per launch: gridDim.y / gridDim.z
#define EMB_MAX_S 65535            // slices of a problem: gridDim.y
#define EMB_MAX_N 2147483135       // points per problem: int32 positions, and q0 + 511 must not overflow (2^31 - 1 - 512)
#define EMB_KNN_THREADS 64
#define EMB_LDS_BYTES 163840
#define EMB_SEARCH_STEPS 200
#define EMB_THREADS 256

// ------------------------------------------------------------------------------------------------------------------ neighbours
template <int DP>
__device__ __forceinline__ double emb_sq(const double (&xr)[DP], const double *pt) {
#pragma clang fp contract(off)
    double sq = 0.0;
#pragma unroll
    for (int c = 0; c < DP; c += 2) {
        const double2 v = *reinterpret_cast<const double2 *>(pt + c);
        const double d0 = xr[c] - v.x, d1 = xr[c + 1] - v.y;
        const double s0 = d0 * d0, s1 = d1 * d1;
        sq = sq + s0;
        sq = sq + s1;
    }
    return sq;
}

template <int DP>
__global__ void __launch_bounds__(EMB_KNN_THREADS) k_latent_knn(const double *__restrict__ x, int d,
                                                                 const long long *__restrict__ prob, int k_max,
                                                                 int *__restrict__ idx, double *__restrict__ d2out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char emb_lds[];
    double *ld2 = reinterpret_cast<double *>(emb_lds);                   // [k_max][64]
    double *tile = ld2 + (size_t)k_max * EMB_KNN_THREADS;                // [64][DP]
    int *lidx = reinterpret_cast<int *>(tile + EMB_KNN_THREADS * DP);    // [k_max][64]
    const long long *pd = prob + (long long)blockIdx.y * EMB_DESC;
    const int n = (int)pd[1], k = min((int)pd[2], k_max), lane = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * EMB_KNN_THREADS;
    if (q0 >= n) return;                                 // uniform: the grid is sized for the largest problem
    const double *xs = x + pd[0] * d;
    const int q = (int)q0 + lane;
    const bool on = q < n;
    const int row = on ? q : n - 1;                      // idle lanes follow a valid point and write nothing
    double xr[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) xr[c] = c < d ? xs[(long long)row * d + c] : 0.0;
    double *md2 = ld2 + lane;
    int *mid = lidx + lane;
    int cnt = 0;
    double worst = INFINITY;
    for (int j0 = 0; j0 < n; j0 += EMB_KNN_THREADS) {
        const int m = min(EMB_KNN_THREADS, n - j0);
        __syncthreads();                                 // the previous tile is read
        for (int e = lane; e < m * DP; e += EMB_KNN_THREADS) {
            const int j = e / DP, c = e % DP;
            tile[e] = c < d ? xs[(long long)(j0 + j) * d + c] : 0.0;
        }
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < m; ++jj) {
            const double s = emb_sq<DP>(xr, tile + jj * DP);
            const int j = j0 + jj;
            if (j != q && (cnt < k || s < worst)) {      // self is left out by index; a tie with the worst entry stays out
                int pos = cnt < k ? cnt : k - 1;         // the free slot, or the worst entry's
                while (pos > 0 && md2[(pos - 1) * EMB_KNN_THREADS] > s) {
                    md2[pos * EMB_KNN_THREADS] = md2[(pos - 1) * EMB_KNN_THREADS];
                    mid[pos * EMB_KNN_THREADS] = mid[(pos - 1) * EMB_KNN_THREADS];
                    --pos;
                }
                md2[pos * EMB_KNN_THREADS] = s;
                mid[pos * EMB_KNN_THREADS] = j;
                if (cnt < k) ++cnt;
                if (cnt == k) worst = md2[(k - 1) * EMB_KNN_THREADS];
            }
        }
    }
    if (!on) return;
    const long long o = pd[3] + (long long)q * k;
    for (int t = 0; t < cnt; ++t) {
        idx[o + t] = mid[t * EMB_KNN_THREADS];
        d2out[o + t] = md2[t * EMB_KNN_THREADS];
    }
}

template <int DP>
static int emb_knn_launch(dim3 grid, size_t dyn, hipStream_t st, const double *x, int d, const long long *prob, int k_max, int *idx,
                          double *d2) {
    static PerDeviceFlag attr_set;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_latent_knn<DP>, hipFuncAttributeMaxDynamicSharedMemorySize, EMB_LDS_BYTES) !=
            hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL(k_latent_knn<DP>, grid, dim3(EMB_KNN_THREADS), dyn, st, x, d, prob, k_max, idx, d2);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// what every entry checks of the table on the host: the problems lie back to back in the points (column 0) and in the neighbour
// lists (column 3); 1 <= k <= min(n - 1, 150).  Returns 0, -22 or -7 and the largest n and k.
static int emb_table(const long long *prob, int P, long long *n_max, long long *k_max) {
    long long off = 0, koff = 0;
    *n_max = *k_max = 0;
    for (int p = 0; p < P; ++p) {
        const long long *d = prob + (long long)p * EMB_DESC;
        const long long n = d[1], k = d[2];
        if (d[0] != off || d[3] != koff || n < 2 || k < 1) return -22;
        if (n > EMB_MAX_N || k > EMB_MAX_K || k > n - 1) return -7;
        off += n;
        koff += n * k;
        if (n > *n_max) *n_max = n;
        if (k > *k_max) *k_max = k;
    }
    return 0;
}

extern "C" int spadot_latent_knn(const double *x, int d, int P, const long long *prob_host, const long long *prob_dev, int *idx,
                                 double *d2, void *stream) {
    if (!x || !prob_host || !prob_dev || !idx || !d2 || P <= 0) return -22;
    if (d < 1 || d > EMB_MAX_D || P > EMB_MAX_P) return -7;
    long long n_max, k_max;
    const int rc = emb_table(prob_host, P, &n_max, &k_max);
    if (rc) return rc;
    const int DP = (d + 3) / 4 * 4;
    const size_t dyn = (size_t)k_max * EMB_KNN_THREADS * 12 + (size_t)EMB_KNN_THREADS * DP * 8;
    if (dyn > EMB_LDS_BYTES) return -7;                  // 131 584 bytes at k = 150, d = 32: never
    const dim3 grid((unsigned)((n_max + EMB_KNN_THREADS - 1) / EMB_KNN_THREADS), (unsigned)P);
    hipStream_t st = (hipStream_t)stream;
    switch (DP / 4) {
        case 1: return emb_knn_launch<4>(grid, dyn, st, x, d, prob_dev, (int)k_max, idx, d2);
        case 2: return emb_knn_launch<8>(grid, dyn, st, x, d, prob_dev, (int)k_max, idx, d2);
        case 3: return emb_knn_launch<12>(grid, dyn, st, x, d, prob_dev, (int)k_max, idx, d2);
        case 4: return emb_knn_launch<16>(grid, dyn, st, x, d, prob_dev, (int)k_max, idx, d2);
        case 5: return emb_knn_launch<20>(grid, dyn, st, x, d, prob_dev, (int)k_max, idx, d2);
        case 6: return emb_knn_launch<24>(grid, dyn, st, x, d, prob_dev, (int)k_max, idx, d2);
        case 7: return emb_knn_launch<28>(grid, dyn, st, x, d, prob_dev, (int)k_max, idx, d2);
        default: return emb_knn_launch<32>(grid, dyn, st, x, d, prob_dev, (int)k_max, idx, d2);
    }
}

// ------------------------------------------------------------------------------------------------------------------ affinities
__device__ __forceinline__ double emb_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ void __launch_bounds__(EMB_THREADS) k_tsne_aff(const double *__restrict__ d2, const long long *__restrict__ prob,
                                                          const double *__restrict__ perp, double *__restrict__ cond,
                                                          double *__restrict__ beta_out) {
    const long long *pd = prob + (long long)blockIdx.y * EMB_DESC;
    const int n = (int)pd[1], k = min((int)pd[2], EMB_MAX_K), lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * (EMB_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;                                  // uniform over the wavefront; the kernel has no barrier
    const long long o = pd[3] + i * k;
    double e[3];
    bool has[3];
    double lo = INFINITY;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int j = lane + 64 * t;
        has[t] = j < k;
        e[t] = has[t] ? d2[o + j] : 0.0;
        if (has[t]) lo = fmin(lo, e[t]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) lo = fmin(lo, __shfl_xor(lo, m, 64));
    double hi = 0.0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        e[t] = has[t] ? e[t] - lo : 0.0;
        hi = fmax(hi, e[t]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) hi = fmax(hi, __shfl_xor(hi, m, 64));
    double beta = 1.0;
    if (hi == 0.0) {                                     // every neighbour at one distance: uniform, beta reported as 0
        beta = 0.0;
    } else {
        const double target = log(perp[blockIdx.y]);
        double bmin = -INFINITY, bmax = INFINITY;
#pragma unroll 1
        for (int step = 0; step < EMB_SEARCH_STEPS; ++step) {
            double ps = 0.0, ws = 0.0;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const double pj = has[t] ? exp(-(beta * e[t])) : 0.0;
                ps += pj;
                ws += e[t] * pj;
            }
            ps = emb_wave_sum(ps);
            ws = emb_wave_sum(ws);
            const double H = log(ps) + beta * (ws / ps);
            if (H > target) {
                bmin = beta;
                beta = bmax == INFINITY ? beta * 2.0 : (beta + bmax) * 0.5;
            } else {
                bmax = beta;
                beta = bmin == -INFINITY ? beta * 0.5 : (beta + bmin) * 0.5;
            }
        }
    }
    double pj[3], ps = 0.0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        pj[t] = has[t] ? exp(-(beta * e[t])) : 0.0;
        ps += pj[t];
    }
    ps = emb_wave_sum(ps);
#pragma unroll
    for (int t = 0; t < 3; ++t)
        if (has[t]) cond[o + lane + 64 * t] = pj[t] / ps;
    if (lane == 0) beta_out[pd[0] + i] = beta;
}

extern "C" int spadot_tsne_affinities(const double *d2, int P, const long long *prob_host, const long long *prob_dev,
                                      const double *perp_host, const double *perp_dev, double *cond, double *beta, void *stream) {
    if (!d2 || !prob_host || !prob_dev || !perp_host || !perp_dev || !cond || !beta || P <= 0) return -22;
    if (P > EMB_MAX_P) return -7;
    long long n_max, k_max;
    const int rc = emb_table(prob_host, P, &n_max, &k_max);
    if (rc) return rc;
    for (int p = 0; p < P; ++p) {
        const double u = perp_host[p];
        const long long n = prob_host[(long long)p * EMB_DESC + 1], k = prob_host[(long long)p * EMB_DESC + 2];
        if (!(u >= 2.0 && u <= 50.0) || (double)n < u + 2.0) return -7;
        if (k != (n - 1 < (long long)floor(3.0 * u) ? n - 1 : (long long)floor(3.0 * u))) return -22;
    }
    const int rows = EMB_THREADS / 64;
    const dim3 grid((unsigned)((n_max + rows - 1) / rows), (unsigned)P);
    hipLaunchKernelGGL(k_tsne_aff, grid, dim3(EMB_THREADS), 0, (hipStream_t)stream, d2, prob_dev, perp_dev, cond, beta);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// ------------------------------------------------------------------------------------------------------------------ iterations
// one partner of one query point: q = 1 / (1 + |y_i - y_j|^2), left out by a select where the partner is the point itself
__device__ __forceinline__ void emb_pair(double2 me, double2 v, bool self, double &z, double &rx, double &ry) {
#pragma clang fp contract(off)
    const double dx = me.x - v.x, dy = me.y - v.y;
    double q = 1.0 / (1.0 + pc_d2(me.x, me.y, v.x, v.y));
    q = self ? 0.0 : q;
    const double w = q * q;
    z = z + q;
    rx = rx + w * dx;
    ry = ry + w * dy;
}

template <int QP>
__global__ void __launch_bounds__(EMB_THREADS) k_tsne_repulse(const double2 *__restrict__ Y, const long long *__restrict__ prob,
                                                              double *__restrict__ part) {
    __shared__ double2 tile[EMB_THREADS];
    const long long *pd = prob + (long long)blockIdx.z * EMB_DESC;
    const int n = (int)pd[1], S = (int)pd[4], s = blockIdx.y, tid = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * (EMB_THREADS * QP);
    if (q0 >= n || s >= S) return;                       // uniform: the grid is sized for the largest problem
    const double2 *y = Y + pd[0];
    const long long T = (n + EMB_THREADS - 1) / EMB_THREADS;
    const int t0 = (int)(s * T / S), t1 = (int)((s + 1) * T / S);           // whole tiles; a slice may hold none
    int qi[QP];
    double2 me[QP];
    double z[QP], rx[QP], ry[QP];
#pragma unroll
    for (int u = 0; u < QP; ++u) {
        qi[u] = (int)q0 + u * EMB_THREADS + tid;
        me[u] = y[min(qi[u], n - 1)];                    // idle lanes follow a valid point and write nothing
        z[u] = rx[u] = ry[u] = 0.0;
    }
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * EMB_THREADS, cnt = min(EMB_THREADS, n - j0);
        __syncthreads();                                 // the previous tile is read
        if (tid < cnt) tile[tid] = y[j0 + tid];
        __syncthreads();
#pragma unroll 4
        for (int jj = 0; jj < cnt; ++jj) {
            const double2 v = tile[jj];
#pragma unroll
            for (int u = 0; u < QP; ++u) emb_pair(me[u], v, j0 + jj == qi[u], z[u], rx[u], ry[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < QP; ++u)
        if (qi[u] < n) {
            double *pp = part + (pd[5] + (long long)s * n + qi[u]) * 3;
            pp[0] = z[u], pp[1] = rx[u], pp[2] = ry[u];
        }
}

// the 256 values of a workgroup in one fixed tree; every thread calls it
__device__ __forceinline__ double emb_block_sum(double *sm, double v) {
    const int tid = threadIdx.x;
    __syncthreads();
    sm[tid] = v;
    __syncthreads();
    for (int h = EMB_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) sm[tid] += sm[tid + h];
        __syncthreads();
    }
    return sm[0];
}

__global__ void __launch_bounds__(EMB_THREADS) k_tsne_rows(const double2 *__restrict__ Y, const long long *__restrict__ prob,
                                                           const long long *__restrict__ rowptr, const int *__restrict__ col,
                                                           const double *__restrict__ val, const double *__restrict__ part,
                                                           double eps, double *__restrict__ zr, double *__restrict__ att,
                                                           double *__restrict__ blk) {
    __shared__ double sm[EMB_THREADS];
    const long long *pd = prob + (long long)blockIdx.y * EMB_DESC;
    const int n = (int)pd[1], S = (int)pd[4];
    const long long i = (long long)blockIdx.x * EMB_THREADS + threadIdx.x;
    if ((long long)blockIdx.x * EMB_THREADS >= n) return;                    // uniform
    double z = 0.0, klr = 0.0;
    if (i < n) {
#pragma clang fp contract(off)
        const double2 *y = Y + pd[0];
        double rx = 0.0, ry = 0.0;
        for (int s = 0; s < S; ++s) {                    // the slices in their order
            const double *pp = part + (pd[5] + (long long)s * n + i) * 3;
            z = z + pp[0];
            rx = rx + pp[1];
            ry = ry + pp[2];
        }
        const double2 me = y[i];
        const long long *rp = rowptr + pd[6] + i;
        const int *cj = col + pd[7];
        const double *pv = val + pd[7];
        double ax = 0.0, ay = 0.0;
        for (long long e = rp[0]; e < rp[1]; ++e) {      // the stored entries in their order
            const int j = min(max(cj[e], 0), n - 1);     // the caller's to refuse; the kernel clamps
            const double2 v = y[j];
            const double dx = me.x - v.x, dy = me.y - v.y;
            const double q = 1.0 / (1.0 + pc_d2(me.x, me.y, v.x, v.y));
            const double pe = pv[e];
            const double w = (eps * pe) * q;
            ax = ax + w * dx;
            ay = ay + w * dy;
            if (pe > 0.0) klr = klr + pe * (log(pe) - log(q));
        }
        double *o = zr + (pd[0] + i) * 3;
        o[0] = z, o[1] = rx, o[2] = ry;
        att[(pd[0] + i) * 2] = ax;
        att[(pd[0] + i) * 2 + 1] = ay;
    }
    const double zb = emb_block_sum(sm, z);
    const double kb = emb_block_sum(sm, klr);
    if (threadIdx.x == 0) {
        blk[(pd[8] + blockIdx.x) * 2] = zb;
        blk[(pd[8] + blockIdx.x) * 2 + 1] = kb;
    }
}

__global__ void __launch_bounds__(EMB_THREADS) k_tsne_apply(const double *__restrict__ Yin, double *__restrict__ Yout,
                                                            const long long *__restrict__ prob, const double *__restrict__ zr,
                                                            const double *__restrict__ att, const double *__restrict__ blk,
                                                            const double *__restrict__ lr, double mu, double *__restrict__ upd,
                                                            double *__restrict__ gains, double *__restrict__ grad,
                                                            double *__restrict__ Zout, double *__restrict__ kl, long long kl_stride,
                                                            long long it) {
#pragma clang fp contract(off)
    const long long *pd = prob + (long long)blockIdx.y * EMB_DESC;
    const int n = (int)pd[1];
    const long long i = (long long)blockIdx.x * EMB_THREADS + threadIdx.x;
    if ((long long)blockIdx.x * EMB_THREADS >= n) return;
    const long long nb = (n + EMB_THREADS - 1) / EMB_THREADS;
    const double *bp = blk + pd[8] * 2;
    double Z = 0.0;
    for (long long b = 0; b < nb; ++b) Z = Z + bp[b * 2];                    // the blocks in ascending order
    if (i < n) {
        const double rate = lr[blockIdx.y];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const long long o = (pd[0] + i) * 2 + c;
            const double g = 4.0 * (att[o] - zr[(pd[0] + i) * 3 + 1 + c] / Z);
            double u = upd[o], gn = gains[o];
            gn = u * g < 0.0 ? gn + 0.2 : gn * 0.8;
            gn = gn < 0.01 ? 0.01 : gn;
            u = mu * u - rate * (gn * g);
            grad[o] = g;
            gains[o] = gn;
            upd[o] = u;
            Yout[o] = Yin[o] + u;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double ks = 0.0;
        for (long long b = 0; b < nb; ++b) ks = ks + bp[b * 2 + 1];
        kl[blockIdx.y * kl_stride + it] = ks + log(Z);
        Zout[blockIdx.y] = Z;
    }
}

extern "C" int spadot_tsne_steps(const long long *prob_host, const long long *prob_dev, int P, const long long *rowptr,
                                 const int *col, const double *val, double *Y0, double *Y1, double *upd, double *gains,
                                 const double *lr, double *part, double *zr, double *att, double *blk, double *grad, double *Z,
                                 double *kl, long long kl_stride, long long it0, int steps, long long early, double exaggeration,
                                 int two, void *stream) {
    if (!prob_host || !prob_dev || !rowptr || !col || !val || !Y0 || !Y1 || !upd || !gains || !lr || !part || !zr || !att || !blk ||
        !grad || !Z || !kl || P <= 0)
        return -22;
    if (steps < 0 || it0 < 0 || early < 0 || kl_stride < it0 + steps || (two != 0 && two != 1)) return -22;
    if (P > EMB_MAX_P || !(exaggeration >= 1.0) || !std::isfinite(exaggeration)) return -7;
    long long n_max, k_max, S_max = 0, soff = 0, roff = 0, eoff = 0, boff = 0;
    const int rc = emb_table(prob_host, P, &n_max, &k_max);
    if (rc) return rc;
    for (int p = 0; p < P; ++p) {
        const long long *d = prob_host + (long long)p * EMB_DESC;
        const long long n = d[1], S = d[4], T = (n + EMB_THREADS - 1) / EMB_THREADS;
        if (d[5] != soff || d[6] != roff || d[7] != eoff || d[8] != boff || d[9] < 0) return -22;
        if (S < 1 || S > EMB_MAX_S) return -7;                 // S > T: slices without tiles, exact zeros
        soff += n * S;
        roff += n + 1;
        eoff += d[9];
        boff += T;
        if (S > S_max) S_max = S;
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)((n_max + EMB_THREADS - 1) / EMB_THREADS);
    const dim3 rgrid(two ? (nb + 1) / 2 : nb, (unsigned)S_max, (unsigned)P), grid(nb, (unsigned)P);
    for (long long it = it0; it < it0 + steps; ++it) {
        const double *yin = (it & 1) ? Y1 : Y0;
        double *yout = (it & 1) ? Y0 : Y1;
        const double eps = it < early ? exaggeration : 1.0, mu = it < early ? 0.5 : 0.8;
        if (two)
            hipLaunchKernelGGL(k_tsne_repulse<2>, rgrid, dim3(EMB_THREADS), 0, st, reinterpret_cast<const double2 *>(yin), prob_dev,
                               part);
        else
            hipLaunchKernelGGL(k_tsne_repulse<1>, rgrid, dim3(EMB_THREADS), 0, st, reinterpret_cast<const double2 *>(yin), prob_dev,
                               part);
        hipLaunchKernelGGL(k_tsne_rows, grid, dim3(EMB_THREADS), 0, st, reinterpret_cast<const double2 *>(yin), prob_dev, rowptr, col,
                           val, (const double *)part, eps, zr, att, blk);
        hipLaunchKernelGGL(k_tsne_apply, grid, dim3(EMB_THREADS), 0, st, yin, yout, prob_dev, (const double *)zr,
                           (const double *)att, (const double *)blk, lr, mu, upd, gains, grad, Z, kl, kl_stride, it);
        if (hipGetLastError() != hipSuccess) return -5;
    }
    return 0;
}
