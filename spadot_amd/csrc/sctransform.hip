// sctransform.hip -- SCTransform's per-gene device work (gfx950, wave64): gene statistics, the Poisson fit with theta.ml of
// every step-1 gene, the Pearson residual statistics of every kept gene, and the dense centred residual block of the SVGs.
//
// Reference arithmetic (under SpaDOT/utils/sctransform): row_gmean (sctransform_utils.py:50-55), qpois_reg
// (sctransform_utils.py:88-148, method='poisson'), theta_ml / score / info (sctransform_utils.py:151-187), pearson_residual
// (sctransform_utils.py:17-37), the clips of vst.py:207-208 and sctransform.py:167-168 + 245-246, and fast_row_scale
// (scale_data.py:45-56).
//
// Conventions of preprocess.hip: counts in CSC (colptr, ridx sorted within a column, fp32 val), rows already in output order
// so that time point t owns the rows [tp_off[t], tp_off[t+1]) and a column's segment of t is found by binary search.  Every
// sum is fp64 and owned by ONE wavefront: lanes take a fixed stride, a fixed xor-butterfly reduces them, no atomics, so two
// runs are bitwise identical.  The spots a time point keeps (those with a non-zero total over all genes) are given twice:
// lu[k], k = 0 .. N-1, their log10 totals in row order (the dense side), and lur[row] / rowmap[row], the same value and the
// position k per row (the sparse side; a spot with a zero total has no nonzeros, so the sparse side never meets one).
//
// Every sum over spots splits into a dense part, the y = 0 value summed over all N spots, and a sparse part over the gene's
// nonzeros that adds (value at y) - (value at y = 0).  Digamma and trigamma are therefore only evaluated at the nonzeros:
// psi(t + 0) - psi(t) is exactly 0.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/spadot_model.h"
#include "csc_walk.h"

#define SCT_WAVE 64
#define SCT_WAVES 4                 // wavefronts per 256-thread workgroup, one gene each
#define SCT_TILE 4096               // most spots per workgroup of k_sct_resid_write (32 KB of LDS)
#define SCT_FIT_OUT 8               // outputs per step-1 gene of k_sct_fit

__device__ __forceinline__ double sct_wave_sum(double x) {
#pragma unroll
    for (int off = SCT_WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, SCT_WAVE);
    return x;
}

__device__ __forceinline__ double sct_clamp(double v, double c) { return v < -c ? -c : (v > c ? c : v); }

// digamma: psi(x) = psi(x + n) - sum_{k<n} 1/(x + k) up to x + n >= 12, then the asymptotic series
// ln x - 1/(2x) - sum_k B_2k / (2k x^2k) through k = 7 (the next term is below 3e-18 at x = 12).
__device__ double sct_digamma(double x) {
    double s = 0.0;
    while (x < 12.0) { s += 1.0 / x; x += 1.0; }
    const double r = 1.0 / x, r2 = r * r;
    const double p = r2 * (1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240 - r2 * (1.0 / 132 -
                     r2 * (691.0 / 32760 - r2 * (1.0 / 12)))))));
    return (log(x) - 0.5 * r - p) - s;
}

// trigamma: psi1(x) = psi1(x + n) + sum_{k<n} 1/(x + k)^2, then 1/x + 1/(2x^2) + sum_k B_2k / x^(2k+1) through k = 7
__device__ double sct_trigamma(double x) {
    double s = 0.0;
    while (x < 12.0) { s += 1.0 / (x * x); x += 1.0; }
    const double r = 1.0 / x, r2 = r * r;
    const double p = r * r2 * (1.0 / 6 - r2 * (1.0 / 30 - r2 * (1.0 / 42 - r2 * (1.0 / 30 - r2 * (5.0 / 66 -
                     r2 * (691.0 / 2730 - r2 * (7.0 / 6)))))));
    return (r + 0.5 * r2 + p) + s;
}

// the Poisson mean of qpois_reg: exp(clip(b0 + b1 x, -708, 709))
__device__ __forceinline__ double sct_qpois_mu(double b0, double b1, double x) {
    double eta = b0 + b1 * x;
    eta = eta < -708.0 ? -708.0 : (eta > 709.0 ? 709.0 : eta);
    return exp(eta);
}

// ---------------------------------------------------------------- gene statistics (row_gmean, gene_attr)
// One wavefront per kept gene of time point t: out[i, 0] = sum log1p(y), out[i, 1] = sum y, out[i, 2] = sum (y - mean)^2
// over the N kept spots (second pass around the mean; the N - nnz zeros add (N - nnz) mean^2).
__global__ void __launch_bounds__(256) k_sct_gene_stats(const long long *colptr, const int *ridx, const float *val,
                                                        const int *tp_off, int t, int Gk, const int *genes, int N, double *out) {
    const int lane = threadIdx.x & (SCT_WAVE - 1);
    const int item = blockIdx.x * SCT_WAVES + (threadIdx.x >> 6);
    if (item >= Gk) return;
    const int g = genes[item];
    const long long a = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
    const long long b = csc_walk_lower_bound(ridx, a, colptr[g + 1], tp_off[t + 1]);
    double sl = 0.0, sy = 0.0;
    for (long long p = a + lane; p < b; p += SCT_WAVE) {
        const double y = (double)val[p];
        sl += log1p(y);
        sy += y;
    }
    sl = sct_wave_sum(sl);
    sy = sct_wave_sum(sy);
    const double n = (double)N, mean = sy / n;
    double ss = 0.0;
    for (long long p = a + lane; p < b; p += SCT_WAVE) {
        const double d = (double)val[p] - mean;
        ss += d * d;
    }
    ss = sct_wave_sum(ss) + (n - (double)(b - a)) * mean * mean;
    if (lane == 0) {
        out[(long long)item * 3 + 0] = sl;
        out[(long long)item * 3 + 1] = sy;
        out[(long long)item * 3 + 2] = ss;
    }
}

// ---------------------------------------------------------------- Poisson fit + theta.ml of one step-1 gene
// One wavefront per gene; every loop bound and branch below is wave-uniform (the sums are butterflies, so every lane holds
// them).  qpois_reg: b = [log(mean y), 0]; each iteration m = exp(clip(X b)), b_new = b + (X^T M X)^-1 X^T (y - m), dif =
// sum |b_new - b|, counter from 2, stop at dif <= tol or counter == maxit; `fitted` is the m of the last iteration (from the
// coefficients BEFORE its update).  theta_ml: t0 = N / sum (y/mu - 1)^2, then while it < limit and |del| > eps: t0 = |t0|,
// del = score / info, t0 += del; a negative t0 ends as 0.
// out[i, 0 .. 7] = theta, b0, b1 (after the last update), b0, b1 of `fitted`, Poisson iterations, theta iterations, sum y.
__global__ void __launch_bounds__(256) k_sct_fit(const long long *colptr, const int *ridx, const float *val, const int *tp_off,
                                                 int t, int G1, const int *genes, const double *lur, const double *lu, int N,
                                                 double tol, int maxit, int limit, double eps, double *out) {
    const int lane = threadIdx.x & (SCT_WAVE - 1);
    const int item = blockIdx.x * SCT_WAVES + (threadIdx.x >> 6);
    if (item >= G1) return;
    const int g = genes[item];
    const long long a = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
    const long long b = csc_walk_lower_bound(ridx, a, colptr[g + 1], tp_off[t + 1]);
    const double n = (double)N;
    double sy = 0.0, sxy = 0.0;                       // X^T y: constant over the iterations, sparse
    for (long long p = a + lane; p < b; p += SCT_WAVE) {
        const double y = (double)val[p];
        sy += y;
        sxy += lur[ridx[p]] * y;
    }
    sy = sct_wave_sum(sy);
    sxy = sct_wave_sum(sxy);

    double b0 = log(sy / n), b1 = 0.0, f0 = b0, f1 = b1, dif = 1.0;
    int ij = 2, iters = 0;
    while (dif > tol) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;          // X^T M X: dense over the N spots
        for (int j = lane; j < N; j += SCT_WAVE) {
            const double x = lu[j];
            const double m = sct_qpois_mu(b0, b1, x);
            s0 += m;
            s1 += x * m;
            s2 += x * (x * m);
        }
        s0 = sct_wave_sum(s0);
        s1 = sct_wave_sum(s1);
        s2 = sct_wave_sum(s2);
        const double l0 = sy - s0, l1 = sxy - s1;     // X^T (y - m)
        const double det = s0 * s2 - s1 * s1;
        const double n0 = b0 + (s2 * l0 - s1 * l1) / det;
        const double n1 = b1 + (s0 * l1 - s1 * l0) / det;
        dif = fabs(n0 - b0) + fabs(n1 - b1);
        f0 = b0; f1 = b1;
        b0 = n0; b1 = n1;
        ++iters;
        if (++ij == maxit) break;
    }

    // theta.ml on mu = the fitted m
    double sq = 0.0;
    for (long long p = a + lane; p < b; p += SCT_WAVE) {
        const double d = (double)val[p] / sct_qpois_mu(f0, f1, lur[ridx[p]]) - 1.0;
        sq += d * d;
    }
    sq = sct_wave_sum(sq) + (n - (double)(b - a));    // every zero adds (0/mu - 1)^2 = 1
    double t0 = n / sq, del = 1.0;
    int it = 1;
    while (it < limit && fabs(del) > eps) {
        t0 = fabs(t0);
        const double lt = log(t0), pt = sct_digamma(t0), p1t = sct_trigamma(t0), it0 = 1.0 / t0;
        double sc = 0.0, in = 0.0;
        for (int j = lane; j < N; j += SCT_WAVE) {     // the y = 0 terms in the reference's order of operations
            const double q = t0 + sct_qpois_mu(f0, f1, lu[j]);
            sc += ((lt + 1.0) - log(q)) - t0 / q;
            in += (2.0 / q - it0) - t0 / (q * q);
        }
        for (long long p = a + lane; p < b; p += SCT_WAVE) {   // (term at y) - (term at 0) at the nonzeros
            const double y = (double)val[p];
            const double q = t0 + sct_qpois_mu(f0, f1, lur[ridx[p]]);
            sc += (sct_digamma(t0 + y) - pt) - y / q;
            in += (p1t - sct_trigamma(t0 + y)) - y / (q * q);
        }
        sc = sct_wave_sum(sc);
        in = sct_wave_sum(in);
        del = sc / in;
        t0 = t0 + del;
        ++it;
    }
    if (t0 < 0.0) t0 = 0.0;
    if (lane == 0) {
        double *o = out + (long long)item * SCT_FIT_OUT;
        o[0] = t0; o[1] = b0; o[2] = b1; o[3] = f0; o[4] = f1;
        o[5] = (double)iters; o[6] = (double)(it - 1); o[7] = sy;
    }
}

// ---------------------------------------------------------------- Pearson residual statistics of every kept gene
// mu = exp(b0 + b1 x) (no clip), r = (y - mu) / sqrt(mu + mu^2 / theta).  out[i, 0] = mean and out[i, 1] = variance (ddof 1)
// of clip(r, +-clip_hi), out[i, 2] = mean of clip(r, +-clip_lo).  Two passes (sum, then squares around the mean), each the
// dense y = 0 value over the N spots plus the nonzeros' corrections.  pars[i] = (theta, b0, b1).
__global__ void __launch_bounds__(256) k_sct_resid_stats(const long long *colptr, const int *ridx, const float *val,
                                                         const int *tp_off, int t, int Gk, const int *genes, const double *lur,
                                                         const double *lu, int N, const double *pars, double clip_hi,
                                                         double clip_lo, double *out) {
    const int lane = threadIdx.x & (SCT_WAVE - 1);
    const int item = blockIdx.x * SCT_WAVES + (threadIdx.x >> 6);
    if (item >= Gk) return;
    const int g = genes[item];
    const long long a = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
    const long long b = csc_walk_lower_bound(ridx, a, colptr[g + 1], tp_off[t + 1]);
    const double th = pars[(long long)item * 3 + 0], b0 = pars[(long long)item * 3 + 1], b1 = pars[(long long)item * 3 + 2];
    const double n = (double)N;
    double s = 0.0, s30 = 0.0;
    for (int j = lane; j < N; j += SCT_WAVE) {
        const double mu = exp(b0 + b1 * lu[j]);
        const double r0 = -mu / sqrt(mu + mu * mu / th);
        s += sct_clamp(r0, clip_hi);
        s30 += sct_clamp(r0, clip_lo);
    }
    for (long long p = a + lane; p < b; p += SCT_WAVE) {
        const double mu = exp(b0 + b1 * lur[ridx[p]]);
        const double sd = sqrt(mu + mu * mu / th);
        const double r = ((double)val[p] - mu) / sd, r0 = -mu / sd;
        s += sct_clamp(r, clip_hi) - sct_clamp(r0, clip_hi);
        s30 += sct_clamp(r, clip_lo) - sct_clamp(r0, clip_lo);
    }
    const double mean = sct_wave_sum(s) / n;
    s30 = sct_wave_sum(s30);
    double ss = 0.0;
    for (int j = lane; j < N; j += SCT_WAVE) {
        const double mu = exp(b0 + b1 * lu[j]);
        const double d = sct_clamp(-mu / sqrt(mu + mu * mu / th), clip_hi) - mean;
        ss += d * d;
    }
    for (long long p = a + lane; p < b; p += SCT_WAVE) {
        const double mu = exp(b0 + b1 * lur[ridx[p]]);
        const double sd = sqrt(mu + mu * mu / th);
        const double d = sct_clamp(((double)val[p] - mu) / sd, clip_hi) - mean, d0 = sct_clamp(-mu / sd, clip_hi) - mean;
        ss += d * d - d0 * d0;
    }
    ss = sct_wave_sum(ss);
    if (lane == 0) {
        out[(long long)item * 3 + 0] = mean;
        out[(long long)item * 3 + 1] = N > 1 ? ss / (n - 1.0) : 0.0;
        out[(long long)item * 3 + 2] = s30 / n;
    }
}

// ---------------------------------------------------------------- the dense scale.data block of S genes
// out[i * N + k] = clip(r, +-clip_lo) - center[i] (fp64) for spot k of the time point.  One workgroup per (gene, tile of up to
// SCT_TILE spots): the tile starts as the y = 0 values in LDS, the gene's nonzeros inside the tile overwrite their slots
// (found by binary search on the rows krow[k0] .. krow[k0 + width]), then the tile is stored coalesced.
__global__ void __launch_bounds__(256) k_sct_resid_write(const long long *colptr, const int *ridx, const float *val,
                                                         const int *tp_off, int t, int S, const int *genes, const double *lur,
                                                         const double *lu, const int *krow, const int *rowmap, int N,
                                                         const double *pars, const double *center, double clip_lo, int width,
                                                         double *out) {
    __shared__ double tile[SCT_TILE];
    const int i = blockIdx.x;
    const int k0 = blockIdx.y * width;
    const int nk = min(width, N - k0);
    if (i >= S || nk <= 0) return;                                   // uniform over the workgroup
    const double th = pars[(long long)i * 3 + 0], b0 = pars[(long long)i * 3 + 1], b1 = pars[(long long)i * 3 + 2];
    const double c = center[i];
    for (int k = threadIdx.x; k < nk; k += blockDim.x) {
        const double mu = exp(b0 + b1 * lu[k0 + k]);
        tile[k] = sct_clamp(-mu / sqrt(mu + mu * mu / th), clip_lo) - c;
    }
    __syncthreads();
    const int g = genes[i];
    const long long a = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
    const long long b = csc_walk_lower_bound(ridx, a, colptr[g + 1], tp_off[t + 1]);
    const long long pa = csc_walk_lower_bound(ridx, a, b, krow[k0]);
    const long long pb = k0 + nk < N ? csc_walk_lower_bound(ridx, pa, b, krow[k0 + nk]) : b;
    for (long long p = pa + threadIdx.x; p < pb; p += blockDim.x) {
        const int r = ridx[p];
        const int k = rowmap[r] - k0;
        if (k >= 0 && k < nk) {
            const double mu = exp(b0 + b1 * lur[r]);
            tile[k] = sct_clamp(((double)val[p] - mu) / sqrt(mu + mu * mu / th), clip_lo) - c;
        }
    }
    __syncthreads();
    double *o = out + (long long)i * N + k0;
    for (int k = threadIdx.x; k < nk; k += blockDim.x) o[k] = tile[k];
}

// ---------------------------------------------------------------- digamma / trigamma at given points (tests)
__global__ void __launch_bounds__(256) k_sct_polygamma(const double *x, int n, double *psi, double *psi1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    psi[i] = sct_digamma(x[i]);
    psi1[i] = sct_trigamma(x[i]);
}

// ---------------------------------------------------------------- C ABI (include/spadot_model.h)
static inline unsigned sct_blocks(long long items) { return (unsigned)((items + SCT_WAVES - 1) / SCT_WAVES); }

extern "C" {

int spadot_sct_gene_stats(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int t, int Gk,
                          const int *genes, int N, double *out, void *stream) {
    if (!colptr || !ridx || !val || !tp_off || !genes || !out || t < 0 || Gk < 0 || N <= 0) return -22;
    if (Gk == 0) return 0;
    hipLaunchKernelGGL(k_sct_gene_stats, dim3(sct_blocks(Gk)), dim3(256), 0, (hipStream_t)stream, colptr, ridx, val, tp_off, t,
                       Gk, genes, N, out);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_sct_fit(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int t, int G1,
                   const int *genes, const double *lur, const double *lu, int N, double tol, int maxit, int limit, double eps,
                   double *out, void *stream) {
    if (!colptr || !ridx || !val || !tp_off || !genes || !lur || !lu || !out || t < 0 || G1 < 0 || N <= 0 || maxit < 3 ||
        limit < 1)
        return -22;
    if (G1 == 0) return 0;
    hipLaunchKernelGGL(k_sct_fit, dim3(sct_blocks(G1)), dim3(256), 0, (hipStream_t)stream, colptr, ridx, val, tp_off, t, G1,
                       genes, lur, lu, N, tol, maxit, limit, eps, out);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_sct_resid_stats(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int t, int Gk,
                           const int *genes, const double *lur, const double *lu, int N, const double *pars, double clip_hi,
                           double clip_lo, double *out, void *stream) {
    if (!colptr || !ridx || !val || !tp_off || !genes || !lur || !lu || !pars || !out || t < 0 || Gk < 0 || N <= 0) return -22;
    if (Gk == 0) return 0;
    hipLaunchKernelGGL(k_sct_resid_stats, dim3(sct_blocks(Gk)), dim3(256), 0, (hipStream_t)stream, colptr, ridx, val, tp_off,
                       t, Gk, genes, lur, lu, N, pars, clip_hi, clip_lo, out);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_sct_resid_write(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int t, int S,
                           const int *genes, const double *lur, const double *lu, const int *krow, const int *rowmap, int N,
                           const double *pars, const double *center, double clip_lo, double *out, void *stream) {
    if (!colptr || !ridx || !val || !tp_off || !genes || !lur || !lu || !krow || !rowmap || !pars || !center || !out || t < 0 ||
        S < 0 || N <= 0)
        return -22;
    if (S == 0) return 0;
    const int ntile = (N + SCT_TILE - 1) / SCT_TILE;
    const int width = (N + ntile - 1) / ntile;                   // equal tiles, each <= SCT_TILE spots
    hipLaunchKernelGGL(k_sct_resid_write, dim3((unsigned)S, (unsigned)ntile), dim3(256), 0, (hipStream_t)stream, colptr, ridx,
                       val, tp_off, t, S, genes, lur, lu, krow, rowmap, N, pars, center, clip_lo, width, out);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_sct_polygamma(const double *x, int n, double *psi, double *psi1, void *stream) {
    if (!x || !psi || !psi1 || n < 0) return -22;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_sct_polygamma, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, psi, psi1);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
