// gmm.hip -- EM for full-covariance Gaussian mixtures of many (data set, component count) problems at once (gfx950, wave64),
// pinned to sklearn.mixture.GaussianMixture(covariance_type="full").  fp64 throughout, no atomics, every sum in one
// fixed order that depends on the problem alone: a problem gives the same bits alone, inside any batch, run after run and for
// any grouping of the iterations into calls.
//
// A problem p is a set of n points in d dimensions (centred, fp64) and K components.  Its parameters are the K_max S doubles of
// par[p] (S = DP + T + 2, DP = 4 ceil(d / 4), T = DP (DP + 1) / 2): first the means, [K_max, DP] (zero padding), then per
// component T + 2 doubles:
//   [0, T)             P_k = L_k^-T (Sigma_k = L_k L_k^T), upper triangular, packed by columns: P[a, j] (a <= j) at j (j + 1) / 2 + a;
//                      the padding is the identity
//   [T]                sum_j log P_k[j, j]
//   [T + 1]            log w_k
//
// One EM iteration is three launches:
// k_gmm_points<DP, MODE>  one 256-thread workgroup per (problem, block of 256 points).  The problem's parameters sit in LDS
//                    (K S doubles: 58 KiB at d = 20, K = 32); a thread owns one point and keeps its coordinates in DP registers
//                    (every index a compile-time constant, nothing goes to scratch; a padded coordinate adds an exact 0).  Per
//                    component: y = (x - mu) P column by column (a ascending), lp = (-(d log 2pi + |y|^2) / 2 + log det) + log w;
//                    the lp of a point go to its row of an LDS tile (odd row stride: conflict-free), then norm = max + log(sum_k
//                    exp(lp - max)) (k ascending) and r = exp(lp - norm).  The block's sum of norm is a fixed tree.  Then the
//                    points' coordinates replace the precision factors in LDS (the means stay) and a thread per (component k,
//                    coordinate a) runs over the block's points in ascending order, with u = x - mu_k, the CURRENT mean:
//                    s0 += r, s1 += r u_a, s2[b] = fma(r u_a, u_b, s2[b]) for every b (the row of x is a broadcast read;
//                    b >= a is stored, packed).  Points with r = 0 are skipped (they add exact zeros).  The partial moments
//                    go to part[p, block, k, M], M = 1 + DP + T.
//                    MODE GIVEN takes r from global memory instead (the first M-step, from the one-hot labels).  It runs twice:
//                    with u = x (the raw moments of the centred data, which give the means) and with u = x - those means.
//                    MODE FINAL writes norm, argmax (first maximum of lp - norm), r and lp per point and forms no moments.
// k_gmm_mstep        one workgroup per (problem, component): adds the partials in ascending block order and forms
//                    delta = s1 / nk, mu = mu_old + delta and Sigma = s2 / nk - delta delta^T + reg I.  (The 10 eps in nk make
//                    these forms inexact by a factor 10 eps / nk; the kernel carries that term exactly, see its comment.)
//                    The moments are taken about the mean the iteration started from, so the cancellation in Sigma shrinks
//                    with the step: a component that has collapsed onto a few points keeps reg I to full precision.  Then
//                    the d x d Cholesky factor (right-looking, column by column) and its inverse by forward substitution
//                    (a thread per column); it writes par, w and Sigma.
// k_gmm_stop         a thread per problem: lb = (sum of the blocks' norm sums, ascending) / n, n_iter += 1, done = |lb - lb_prev|
//                    < tol.  It runs AFTER the M-step, so the M-step of the stopping iteration has been applied.
// A problem whose done flag is set is frozen: none of the three kernels touches its parameters, lb or n_iter again.
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/spadot_model.h"
#include "per_device.h"

#define GMM_THREADS 256
#define GMM_MAX_K 32
#define GMM_MAX_D 32
#define GMM_MAX_P 65535            // problems per launch: gridDim.y
#define GMM_MAX_N 2147483391       // points per set: int32 positions, q0 + 255 must not overflow
#define GMM_LDS_BYTES 163840       // one workgroup may take the whole LDS of a compute unit
#define GMM_STATIC_BYTES 2048      // the tree of the norm sum

enum { GMM_EM = 0, GMM_GIVEN = 1, GMM_FINAL = 2 };

static inline int gmm_dp(int d) { return (d + 3) / 4 * 4; }
static inline int gmm_S(int DP) { return DP + DP * (DP + 1) / 2 + 2; }
static inline int gmm_M(int DP) { return 1 + DP + DP * (DP + 1) / 2; }
static inline long long gmm_region_a(int DP, int K_max) {
    const long long a = (long long)K_max * gmm_S(DP), b = (long long)(K_max + GMM_THREADS) * DP;
    return a > b ? a : b;
}
static inline long long gmm_dyn_bytes(int DP, int K_max) {
    return 8 * (gmm_region_a(DP, K_max) + (long long)GMM_THREADS * (K_max | 1));
}

template <int DP, int MODE>
__global__ void __launch_bounds__(GMM_THREADS) k_gmm_points(const double *__restrict__ x, int d, const long long *__restrict__ prob,
                                                             const double *__restrict__ par, const double *__restrict__ resp_in,
                                                             int K_max, int region_a, int nblk_max, int shifted,
                                                             const int *__restrict__ done,
                                                             double *__restrict__ part, double *__restrict__ norm_out,
                                                             int *__restrict__ lab_out, double *__restrict__ resp_out,
                                                             double *__restrict__ lp_out) {
    constexpr int T = DP * (DP + 1) / 2, S = DP + T + 2, S2 = T + 2, M = 1 + DP + T;
    extern __shared__ __attribute__((aligned(16))) double gm_lds[];
    __shared__ double red[GMM_THREADS];
    const int p = blockIdx.y, tid = threadIdx.x;
    const long long xoff = prob[4 * p], roff = prob[4 * p + 1];
    const int n = (int)prob[4 * p + 2], K = min((int)prob[4 * p + 3], K_max);
    const int q0 = blockIdx.x * GMM_THREADS;
    if (q0 >= n) return;                                 // uniform: the grid is sized for the largest set
    if (MODE == GMM_EM && done[p]) return;               // frozen
    double *A = gm_lds, *R = gm_lds + region_a;          // means, then factors (later the points); the tile of lp / r
    double *F = A + K_max * DP;
    const int Kp = K_max | 1;                            // odd row stride
    const double *xs = x + xoff * d;
    const int q = q0 + tid;
    const bool on = q < n;
    const int row = on ? q : n - 1;                      // idle lanes follow a valid point and weigh nothing
    const int cnt = min(GMM_THREADS, n - q0);
    double xr[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) xr[c] = c < d ? xs[(long long)row * d + c] : 0.0;
    double *Rt = R + tid * Kp;

    if (MODE == GMM_GIVEN) {
        for (int k = 0; k < K; ++k) Rt[k] = on ? resp_in[(roff + row) * K_max + k] : 0.0;
        const double *pp = par + (long long)p * K_max * S;            // the means alone: the moments are taken about them
        for (int e = tid; e < K_max * DP; e += GMM_THREADS) A[e] = shifted ? pp[e] : 0.0;
    } else {
        const double *pp = par + (long long)p * K_max * S;
        for (int e = tid; e < K_max * DP + K * S2; e += GMM_THREADS) A[e] = pp[e];
        __syncthreads();
        const double c0 = (double)d * 1.8378770664093453;            // d log(2 pi)
        double mx = -INFINITY;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const double *pk = F + k * S2, *mk = A + k * DP;
            double diff[DP];
#pragma unroll
            for (int c = 0; c < DP; ++c) diff[c] = xr[c] - mk[c];
            double qq = 0.0;
#pragma unroll
            for (int j = 0; j < DP; ++j) {
                double y = 0.0;
#pragma unroll
                for (int a = 0; a <= j; ++a) y = fma(diff[a], pk[j * (j + 1) / 2 + a], y);
                qq = fma(y, y, qq);
            }
            const double lp = (-0.5 * (c0 + qq) + pk[T]) + pk[T + 1];
            Rt[k] = lp;
            mx = fmax(mx, lp);
        }
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += exp(Rt[k] - mx);
        const double norm = mx + log(s);
        double best = -INFINITY;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            const double lp = Rt[k], lr = lp - norm;
            if (lr > best) { best = lr; arg = k; }                    // first maximum
            const double r = exp(lr);
            if (MODE == GMM_FINAL) {
                if (on) {
                    if (resp_out) resp_out[(roff + row) * K_max + k] = r;
                    if (lp_out) lp_out[(roff + row) * K_max + k] = lp;
                }
            } else {
                Rt[k] = on ? r : 0.0;
            }
        }
        if (MODE == GMM_FINAL) {
            if (on) {
                norm_out[roff + row] = norm;
                if (lab_out) lab_out[roff + row] = arg;
            }
            return;
        }
        red[tid] = on ? norm : 0.0;
        __syncthreads();
        for (int h = GMM_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
    }
    if (MODE == GMM_FINAL) return;
    const long long PS = (long long)K_max * M + 1;
    double *pb = part + ((long long)p * nblk_max + blockIdx.x) * PS;
    if (tid == 0) pb[(long long)K_max * M] = MODE == GMM_EM ? red[0] : 0.0;
    __syncthreads();                                     // the factors are read: the points' coordinates take their place
#pragma unroll
    for (int c = 0; c < DP; ++c) F[tid * DP + c] = xr[c];
    __syncthreads();
    for (int e = tid; e < K * DP; e += GMM_THREADS) {
        const int k = e / DP, a = e % DP;
        double acc[DP], mk[DP];
#pragma unroll
        for (int b = 0; b < DP; ++b) {
            acc[b] = 0.0;
            mk[b] = A[k * DP + b];
        }
        const double ma = A[k * DP + a];
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 1
        for (int i = 0; i < cnt; ++i) {
            const double r = R[i * Kp + k];
            if (r != 0.0) {
                const double *pt = F + i * DP;
                const double t = r * (pt[a] - ma);
                s0 += r;
                s1 += t;
#pragma unroll
                for (int b = 0; b < DP; b += 2) {
                    const double2 v = *reinterpret_cast<const double2 *>(pt + b);
                    acc[b] = fma(t, v.x - mk[b], acc[b]);
                    acc[b + 1] = fma(t, v.y - mk[b + 1], acc[b + 1]);
                }
            }
        }
        double *pm = pb + (long long)k * M;
        if (a == 0) pm[0] = s0;
        pm[1 + a] = s1;
#pragma unroll
        for (int b = 0; b < DP; ++b)
            if (b >= a) pm[1 + DP + b * (b + 1) / 2 + a] = acc[b];
    }
}

__global__ void __launch_bounds__(GMM_THREADS) k_gmm_mstep(int d, int DP, const long long *__restrict__ prob, int K_max,
                                                            int nblk_max, const double *__restrict__ part,
                                                            const int *__restrict__ done, double reg, int shifted,
                                                            double *__restrict__ par,
                                                            double *__restrict__ w_out, double *__restrict__ cov_out,
                                                            double *__restrict__ mom_out) {
    __shared__ double mom[1 + GMM_MAX_D + GMM_MAX_D * (GMM_MAX_D + 1) / 2];
    __shared__ double C[GMM_MAX_D * GMM_MAX_D];          // Sigma, then its Cholesky factor in the lower triangle
    __shared__ double Z[GMM_MAX_D * GMM_MAX_D];          // L^-1, lower triangle
    __shared__ double mu[GMM_MAX_D], dlt[GMM_MAX_D], eps_[GMM_MAX_D];
    const int p = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const int n = (int)prob[4 * p + 2], K = min((int)prob[4 * p + 3], K_max);
    if (k >= K || done[p]) return;
    const int T = DP * (DP + 1) / 2, S = DP + T + 2, M = 1 + DP + T;
    const int nblk = (n + GMM_THREADS - 1) / GMM_THREADS;
    const long long PS = (long long)K_max * M + 1;
    const double *pp = part + (long long)p * nblk_max * PS + (long long)k * M;
    for (int e = tid; e < M; e += GMM_THREADS) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += pp[b * PS + e];          // ascending block order
        mom[e] = s;
        if (mom_out) mom_out[((long long)p * K_max + k) * M + e] = s;
    }
    const double nk_e = 10.0 * 2.220446049250313e-16;
    double *pm = par + (long long)p * K_max * S + (long long)k * DP, *out = par + (long long)p * K_max * S + (long long)K_max * DP + (long long)k * (T + 2);
    __syncthreads();
    // sklearn's nk = s0 + 10 eps is not translation invariant; with u = x - mu_old, f = s0 / nk and g = 10 eps / nk the exact
    // forms are mu = mu_old + e, e = delta - g mu_old, and Sigma = s2 / nk - (e delta^T + delta e^T) + f e e^T (e = delta up to g)
    const double nk = mom[0] + nk_e, f = mom[0] / nk, g = nk_e / nk;
    if (tid < DP) {
        const double m0 = tid < d && shifted ? pm[tid] : 0.0, dl = tid < d ? mom[1 + tid] / nk : 0.0, e = dl - m0 * g;
        dlt[tid] = dl;
        eps_[tid] = e;
        mu[tid] = m0 + e;
    }
    __syncthreads();
    for (int e = tid; e < DP * DP; e += GMM_THREADS) {
        const int a = e / DP, b = e % DP, lo = min(a, b), hi = max(a, b);
        double c;
        if (hi < d) {
            c = mom[1 + DP + hi * (hi + 1) / 2 + lo] / nk - (eps_[a] * dlt[b] + dlt[a] * eps_[b]) + f * (eps_[a] * eps_[b]);
            if (a == b) c += reg;
            cov_out[(((long long)p * K_max + k) * d + a) * d + b] = c;
        } else {
            c = a == b ? 1.0 : 0.0;
        }
        C[e] = c;
    }
    __syncthreads();
    for (int j = 0; j < d; ++j) {                        // a Sigma that is not positive definite gives NaN, which stays NaN
        if (tid == 0) C[j * DP + j] = sqrt(C[j * DP + j]);
        __syncthreads();
        for (int i = j + 1 + tid; i < d; i += GMM_THREADS) C[i * DP + j] /= C[j * DP + j];
        __syncthreads();
        for (int e = tid; e < d * d; e += GMM_THREADS) {
            const int i = e / d, c = e % d;
            if (c > j && i >= c) C[i * DP + c] = fma(-C[i * DP + j], C[c * DP + j], C[i * DP + c]);
        }
        __syncthreads();
    }
    if (tid < d) {                                       // column tid of L^-1: L z = e_tid, forward
        const int c = tid;
        Z[c * DP + c] = 1.0 / C[c * DP + c];
        for (int i = c + 1; i < d; ++i) {
            double s = 0.0;
            for (int m = c; m < i; ++m) s = fma(C[i * DP + m], Z[m * DP + c], s);
            Z[i * DP + c] = -s / C[i * DP + i];
        }
    }
    __syncthreads();
    if (tid < DP) pm[tid] = mu[tid];
    for (int e = tid; e < DP * DP; e += GMM_THREADS) {
        const int j = e / DP, a = e % DP;
        if (a <= j) out[j * (j + 1) / 2 + a] = j < d ? Z[j * DP + a] : (a == j ? 1.0 : 0.0);    // P[a, j] = L^-1[j, a]
    }
    if (tid == 0) {
        double ld = 0.0;
        for (int j = 0; j < d; ++j) ld += log(Z[j * DP + j]);
        const double w = nk / (double)n;
        out[T] = ld;
        out[T + 1] = log(w);
        w_out[(long long)p * K_max + k] = w;
    }
}

__global__ void k_gmm_stop(int P, int DP, const long long *__restrict__ prob, int K_max, int nblk_max,
                           const double *__restrict__ part, double tol, int *__restrict__ done, int *__restrict__ n_iter,
                           double *__restrict__ lb) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || done[p]) return;
    const int n = (int)prob[4 * p + 2], M = 1 + DP + DP * (DP + 1) / 2;
    const int nblk = (n + GMM_THREADS - 1) / GMM_THREADS;
    const long long PS = (long long)K_max * M + 1;
    const double *pp = part + (long long)p * nblk_max * PS + (long long)K_max * M;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += pp[b * PS];
    const double now = s / (double)n, prev = lb[p];
    lb[p] = now;
    n_iter[p] += 1;
    if (fabs(now - prev) < tol) done[p] = 1;
}

static int gmm_check(int d, int P, int K_max, int n_max) {
    if (d < 1 || d > GMM_MAX_D || K_max < 1 || K_max > GMM_MAX_K || P > GMM_MAX_P || n_max > GMM_MAX_N) return -7;
    if (gmm_dyn_bytes(gmm_dp(d), K_max) + GMM_STATIC_BYTES > GMM_LDS_BYTES) return -7;
    return 0;
}

template <int DP, int MODE>
static int gmm_points(dim3 grid, hipStream_t st, const double *x, int d, const long long *prob, const double *par,
                      const double *resp_in, int K_max, int shifted, const int *done, double *part, double *norm, int *lab, double *resp,
                      double *lp) {
    static PerDeviceFlag attr_set;
    const long long dyn = gmm_dyn_bytes(DP, K_max);
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_gmm_points<DP, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                GMM_LDS_BYTES - GMM_STATIC_BYTES) != hipSuccess) return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL((k_gmm_points<DP, MODE>), grid, dim3(GMM_THREADS), (size_t)dyn, st, x, d, prob, par, resp_in, K_max,
                       (int)gmm_region_a(DP, K_max), (int)grid.x, shifted, done, part, norm, lab, resp, lp);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

template <int MODE>
static int gmm_points_d(dim3 grid, hipStream_t st, const double *x, int d, const long long *prob, const double *par,
                        const double *resp_in, int K_max, int shifted, const int *done, double *part, double *norm, int *lab, double *resp,
                        double *lp) {
#define GMM_CASE(DPV) case DPV: return gmm_points<DPV, MODE>(grid, st, x, d, prob, par, resp_in, K_max, shifted, done, part, norm, lab, resp, lp);
    switch (gmm_dp(d)) {
        GMM_CASE(4) GMM_CASE(8) GMM_CASE(12) GMM_CASE(16) GMM_CASE(20) GMM_CASE(24) GMM_CASE(28) GMM_CASE(32)
        default: return -7;
    }
#undef GMM_CASE
}

extern "C" int spadot_gmm_em_step(const double *x, int d, int P, const long long *prob, int K_max, int n_max, double *par,
                                  double *w, double *cov, double *mom, const double *resp_init, double reg_covar, double tol,
                                  int steps, double *part, int *done, int *n_iter, double *lb, void *stream) {
    if (!x || !prob || !par || !w || !cov || !part || !done || !n_iter || !lb || P <= 0 || n_max <= 0 || steps < 0) return -22;
    const int rc = gmm_check(d, P, K_max, n_max);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int DP = gmm_dp(d);
    const dim3 grid((unsigned)((n_max + GMM_THREADS - 1) / GMM_THREADS), (unsigned)P), mgrid((unsigned)K_max, (unsigned)P);
    auto mstep = [&](int shifted, double *mom_out) {
        hipLaunchKernelGGL(k_gmm_mstep, mgrid, dim3(GMM_THREADS), 0, st, d, DP, prob, K_max, (int)grid.x, part, done, reg_covar,
                           shifted, par, w, cov, mom_out);
        return hipGetLastError() == hipSuccess ? 0 : -5;
    };
    if (resp_init) {                                     // the M-step from given responsibilities: no lb, no count.  Two passes:
        for (int pass = 0; pass < 2; ++pass) {           // raw moments give the means, moments about those means the rest
            int e = gmm_points_d<GMM_GIVEN>(grid, st, x, d, prob, par, resp_init, K_max, pass, done, part, nullptr, nullptr,
                                            nullptr, nullptr);
            if (e || (e = mstep(pass, pass == 0 ? mom : nullptr))) return e;
        }
    }
    for (int it = 0; it < steps; ++it) {
        int e = gmm_points_d<GMM_EM>(grid, st, x, d, prob, par, nullptr, K_max, 1, done, part, nullptr, nullptr, nullptr, nullptr);
        if (e || (e = mstep(1, mom))) return e;
        hipLaunchKernelGGL(k_gmm_stop, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, DP, prob, K_max, (int)grid.x, part,
                           tol, done, n_iter, lb);
        if (hipGetLastError() != hipSuccess) return -5;
    }
    return 0;
}

extern "C" int spadot_gmm_estep(const double *x, int d, int P, const long long *prob, int K_max, int n_max, const double *par,
                                double *norm, int *labels, double *resp, double *lp, void *stream) {
    if (!x || !prob || !par || !norm || P <= 0 || n_max <= 0) return -22;
    const int rc = gmm_check(d, P, K_max, n_max);
    if (rc) return rc;
    const dim3 grid((unsigned)((n_max + GMM_THREADS - 1) / GMM_THREADS), (unsigned)P);
    return gmm_points_d<GMM_FINAL>(grid, (hipStream_t)stream, x, d, prob, par, nullptr, K_max, 0, nullptr, nullptr, norm, labels,
                                   resp, lp);
}
