// preprocess.hip -- the preprocess stage's device work (gfx950, wave64): SPARK-X gene statistics and the log-normalise +
// scale of the output matrix.
//
// Reference arithmetic (all under SpaDOT/utils): the SCTransform gene filter (sctransform/vst.py:71-75), the spot / gene
// filters of _sparkx (_utils.py:139-146), _sparkx_sk (_utils.py:230-261), the two-term p-value that _sparkx_pval computes
// with Davies / Liu (_utils.py:263-374), _ACAT (_utils.py:376-414) and normalize_total + log1p + scale of
// _preprocess_utils.py:31-49.
//
// Counts are fp32 values in CSR (spots x genes) and CSC (genes x spots), rows already in output order: a time point t owns
// the rows [tp_off[t], tp_off[t+1]), so each CSC column splits into one contiguous segment per time point (row indices are
// sorted within a column; the segment bounds are found by binary search).  Every sum is fp64 and is owned by ONE wavefront:
// lanes take a fixed stride of the segment, then a fixed xor-butterfly reduces the lanes.  No floating-point atomics, so two
// runs give bitwise-identical results.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/spadot_model.h"
#include "csc_walk.h"

#define PRE_WAVE 64
#define PRE_WAVES 4                // wavefronts per 256-thread workgroup, one item each
#define PRE_NK 11                  // SPARK-X kernels: projection, 5 Gaussian, 5 cosine
#define PRE_NX (2 * PRE_NK)        // columns of the centred kernel coordinates
#define PRE_NM (PRE_NX + 2)        // moments per (time point, gene): sum y, sum y^2, sum y * xt[:, 0 .. 21]
#define PRE_TILE 15360             // most output columns per workgroup of k_pre_scale_write (60 KB of LDS)

__device__ __forceinline__ double pre_wave_sum(double x) {
#pragma unroll
    for (int off = PRE_WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, PRE_WAVE);
    return x;
}

__device__ __forceinline__ int pre_wave_sum_i(int x) {
#pragma unroll
    for (int off = PRE_WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, PRE_WAVE);
    return x;
}

// time point of a row: tp_off is short (one entry per time point), a linear scan is enough
__device__ __forceinline__ int pre_row_tp(const int *tp_off, int T, int row) {
    int t = 0;
    while (t + 1 < T && row >= tp_off[t + 1]) ++t;
    return t;
}

// ---------------------------------------------------------------- gene detection (vst.py:71-75)
__global__ void __launch_bounds__(256) k_pre_gene_detect(const long long *colptr, const int *ridx, const float *val,
                                                         const int *tp_off, int T, int G, double thr, int *cnt, double *colsum) {
    const int lane = threadIdx.x & (PRE_WAVE - 1);
    const long long item = (long long)blockIdx.x * PRE_WAVES + (threadIdx.x >> 6);
    if (item >= (long long)T * G) return;
    const int t = (int)(item / G), g = (int)(item % G);
    const long long a = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
    const long long b = csc_walk_lower_bound(ridx, a, colptr[g + 1], tp_off[t + 1]);
    int c = 0;
    double s = 0.0;
    for (long long p = a + lane; p < b; p += PRE_WAVE) {
        const double v = (double)val[p];
        c += v >= thr ? 1 : 0;
        s += v;
    }
    c = pre_wave_sum_i(c);
    s = pre_wave_sum(s);
    if (lane == 0) { cnt[item] = c; colsum[item] = s; }
}

// ---------------------------------------------------------------- row totals over a per-time-point gene mask
__global__ void __launch_bounds__(256) k_pre_row_total(const long long *indptr, const int *cidx, const float *val,
                                                       const int *tp_off, int T, int G, const unsigned char *mask, double *total) {
    const int lane = threadIdx.x & (PRE_WAVE - 1);
    const int row = tp_off[0] + blockIdx.x * PRE_WAVES + (threadIdx.x >> 6);
    if (row >= tp_off[T]) return;
    const unsigned char *m = mask + (long long)pre_row_tp(tp_off, T, row) * G;
    double s = 0.0;
    for (long long p = indptr[row] + lane; p < indptr[row + 1]; p += PRE_WAVE) {
        const int c = cidx[p];
        if (m[c]) s += (double)val[p];
    }
    s = pre_wave_sum(s);
    if (lane == 0) total[row] = s;
}

// ---------------------------------------------------------------- SPARK-X moments (_sparkx_sk: EHL = y^T X, sum y^2, mean y)
// One wavefront per (time point, gene) pair; one pass over the column segment.  xt holds the 22 centred kernel coordinates of
// every kept spot (fp64, row rowmap[r] for spot r; a time point's block fits in L2), so the traffic is the nonzeros plus one
// gathered 176-byte xt row per nonzero.
__global__ void __launch_bounds__(256) k_sparkx_moments(const long long *colptr, const int *ridx, const float *val,
                                                        const int *tp_off, int P, const int *pair_t, const int *pair_g,
                                                        const int *rowmap, const double *xt, double *mom) {
    const int lane = threadIdx.x & (PRE_WAVE - 1);
    const int item = blockIdx.x * PRE_WAVES + (threadIdx.x >> 6);
    if (item >= P) return;
    const int t = pair_t[item], g = pair_g[item];
    const long long a = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
    const long long b = csc_walk_lower_bound(ridx, a, colptr[g + 1], tp_off[t + 1]);
    double acc[PRE_NM];
#pragma unroll
    for (int k = 0; k < PRE_NM; ++k) acc[k] = 0.0;
    for (long long p = a + lane; p < b; p += PRE_WAVE) {
        const double y = (double)val[p];
        acc[0] += y;
        acc[1] += y * y;
        const int xr = rowmap[ridx[p]];
        if (xr >= 0) {
            const double2 *x2 = reinterpret_cast<const double2 *>(xt + (long long)xr * PRE_NX);
#pragma unroll
            for (int k = 0; k < PRE_NX / 2; ++k) {
                const double2 v = x2[k];
                acc[2 + 2 * k] += y * v.x;
                acc[3 + 2 * k] += y * v.y;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PRE_NM; ++k) acc[k] = pre_wave_sum(acc[k]);
    if (lane == 0) {
        double *o = mom + (long long)item * PRE_NM;
#pragma unroll
        for (int k = 0; k < PRE_NM; ++k) o[k] = acc[k];
    }
}

// P[l1 X1 + l2 X2 > q], X1, X2 independent chi^2_1:  (1/pi) int_0^pi exp(-q / (2 (l1 cos^2 + l2 sin^2))) dtheta.
// The integrand is smooth and pi-periodic, so the trapezoid rule on `nodes` equispaced points converges geometrically.
__device__ double pre_sf_two_chi2(double q, double l1, double l2, int nodes) {
    if (!(q > 0.0)) return 1.0;
    if (l1 == l2) return exp(-q / (2.0 * l1));
    double s = 0.0;
    for (int j = 0; j < nodes; ++j) {
        double sn, cs;
        sincos(M_PI * (double)j / (double)nodes, &sn, &cs);
        s += exp(-q / (2.0 * (l1 * cs * cs + l2 * sn * sn)));
    }
    return s / (double)nodes;
}

// ---------------------------------------------------------------- SPARK-X statistics, p-values and ACAT
// One thread per pair.  inv: [T, 11, 4] row-major (X^T X)^-1 per time point and kernel, lam: [T, 11, 2] the eigenvalues of
// X^T X (X^T X)^-1, nkeep[t]: the kept spots of time point t.
__global__ void __launch_bounds__(256) k_sparkx_pvals(const double *mom, int P, const int *pair_t, const int *nkeep,
                                                      const double *inv, const double *lam, int nodes, double *stat,
                                                      double *pval, double *comb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int t = pair_t[i];
    const double *m = mom + (long long)i * PRE_NM;
    const double n = (double)nkeep[t];
    const double sy = m[0], syy = m[1];
    const double ybar = sy / n;
    const double ylam = 1.0 - n * ybar * ybar / syy;
    bool any_zero = false, any_one = false, any_small = false;
    double p[PRE_NK];
    for (int k = 0; k < PRE_NK; ++k) {
        const double *a = inv + ((long long)t * PRE_NK + k) * 4;
        const double e1 = m[2 + 2 * k], e2 = m[3 + 2 * k];
        const double s = (e1 * (a[0] * e1 + a[1] * e2) + e2 * (a[2] * e1 + a[3] * e2)) * n / syy;
        const double *l = lam + ((long long)t * PRE_NK + k) * 2;
        // ylam = 0 (a gene constant over the kept spots) has no null distribution: p = 1 (the reference yields NaN there)
        const double pk = ylam > 0.0 ? pre_sf_two_chi2(s, ylam * l[0], ylam * l[1], nodes) : 1.0;
        stat[(long long)i * PRE_NK + k] = s;
        pval[(long long)i * PRE_NK + k] = pk;
        p[k] = pk;
        any_zero |= pk == 0.0;
        any_one |= pk == 1.0;
        any_small |= pk < 1e-16;
    }
    // _ACAT with equal weights 1/11 (a zero p-value wins over a p-value of one; the reference raises on that mix)
    double out;
    if (any_zero) {
        out = 0.0;
    } else if (any_one) {
        out = 1.0;
    } else {
        const double w = 1.0 / (double)PRE_NK;
        double cct = 0.0;
        if (!any_small) {
            for (int k = 0; k < PRE_NK; ++k) cct += w * tan((0.5 - p[k]) * M_PI);
        } else {
            double small = 0.0, rest = 0.0;
            for (int k = 0; k < PRE_NK; ++k)
                if (p[k] < 1e-16) small += w / (M_PI * p[k]);
            for (int k = 0; k < PRE_NK; ++k)
                if (!(p[k] < 1e-16)) rest += w * tan((0.5 - p[k]) * M_PI);
            cct = small + rest;
        }
        out = cct > 1e15 ? 1.0 / (cct * M_PI) : 1.0 - (0.5 + atan(cct) / M_PI);
    }
    comb[i] = out;
}

// ---------------------------------------------------------------- log-normalise: per (time point, column) mean and std
// v = log1p(x * target / total[row]) (0 where total is 0); mean over the N_t rows of the time point, variance with ddof 1
// from a second pass around the mean, the N_t - nnz zeros counted as (N_t - nnz) mean^2; std 0 -> 1 (sc.pp.scale).
__device__ __forceinline__ double pre_lognorm(float x, double tot, double target) {
    return tot > 0.0 ? log1p((double)x * target / tot) : 0.0;
}

__global__ void __launch_bounds__(256) k_pre_lognorm_stats(const long long *colptr, const int *ridx, const float *val,
                                                           const int *tp_off, int T, int S, const int *cols,
                                                           const double *total, double target, double *mean, double *stdv) {
    const int lane = threadIdx.x & (PRE_WAVE - 1);
    const long long item = (long long)blockIdx.x * PRE_WAVES + (threadIdx.x >> 6);
    if (item >= (long long)T * S) return;
    const int t = (int)(item / S), g = cols[item % S];
    const long long a = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
    const long long b = csc_walk_lower_bound(ridx, a, colptr[g + 1], tp_off[t + 1]);
    const double n = (double)(tp_off[t + 1] - tp_off[t]);
    double s = 0.0;
    for (long long p = a + lane; p < b; p += PRE_WAVE) s += pre_lognorm(val[p], total[ridx[p]], target);
    const double mu = pre_wave_sum(s) / n;
    double ss = 0.0;
    for (long long p = a + lane; p < b; p += PRE_WAVE) {
        const double d = pre_lognorm(val[p], total[ridx[p]], target) - mu;
        ss += d * d;
    }
    ss = pre_wave_sum(ss) + (n - (double)(b - a)) * mu * mu;
    double sd = n > 1.0 ? sqrt(ss / (n - 1.0)) : 0.0;
    if (sd == 0.0) sd = 1.0;
    if (lane == 0) { mean[item] = mu; stdv[item] = sd; }
}

// ---------------------------------------------------------------- dense standardised block
// out[(row - tp_off[0]) * S + j] = clip((v - mean[t, j]) / std[t, j]) as float32, for the S columns colpos maps to 0 .. S-1
// (colpos[g] = -1: not written).  One workgroup per (row, tile of up to PRE_TILE columns): the tile starts as the zero entries'
// value in LDS, the row's nonzeros overwrite their slots, then the tile is stored coalesced.
__device__ __forceinline__ float pre_clip(double z, double clip) {
    if (clip > 0.0) z = z < -clip ? -clip : (z > clip ? clip : z);
    return (float)z;
}

__global__ void __launch_bounds__(256) k_pre_scale_write(const long long *indptr, const int *cidx, const float *val,
                                                         const int *tp_off, int T, int S, const int *colpos,
                                                         const double *total, double target, const double *mean,
                                                         const double *stdv, double clip, int width, float *out) {
    extern __shared__ float tile[];               // `width` floats: the whole row in one tile up to PRE_TILE columns, so
    const int row = tp_off[0] + blockIdx.x;       // the row's nonzeros are read once per tile, at most ceil(S / PRE_TILE) times
    const int j0 = blockIdx.y * width;
    const int nj = min(width, S - j0);
    const int t = pre_row_tp(tp_off, T, row);
    const double *mu = mean + (long long)t * S, *sd = stdv + (long long)t * S;
    for (int j = threadIdx.x; j < nj; j += blockDim.x) tile[j] = pre_clip(-mu[j0 + j] / sd[j0 + j], clip);
    __syncthreads();
    const double tot = total[row];
    for (long long p = indptr[row] + threadIdx.x; p < indptr[row + 1]; p += blockDim.x) {
        const int j = colpos[cidx[p]] - j0;
        if (j >= 0 && j < nj) tile[j] = pre_clip((pre_lognorm(val[p], tot, target) - mu[j0 + j]) / sd[j0 + j], clip);
    }
    __syncthreads();
    float *o = out + (long long)(row - tp_off[0]) * S + j0;
    for (int j = threadIdx.x; j < nj; j += blockDim.x) o[j] = tile[j];
}

// ---------------------------------------------------------------- C ABI (include/spadot_model.h)
static inline unsigned pre_blocks(long long items) { return (unsigned)((items + PRE_WAVES - 1) / PRE_WAVES); }

extern "C" {

int spadot_pre_gene_detect(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int T, int G,
                           double thr, int *cnt, double *colsum, void *stream) {
    if (!colptr || !ridx || !val || !tp_off || !cnt || !colsum || T <= 0 || G <= 0) return -22;
    if (pre_blocks((long long)T * G) > 0x7fffffffu) return -22;
    hipLaunchKernelGGL(k_pre_gene_detect, dim3(pre_blocks((long long)T * G)), dim3(256), 0, (hipStream_t)stream, colptr, ridx,
                       val, tp_off, T, G, thr, cnt, colsum);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_pre_row_total(const long long *indptr, const int *cidx, const float *val, const int *tp_off, int T, int G,
                         const unsigned char *mask, int nrows, double *total, void *stream) {
    if (!indptr || !cidx || !val || !tp_off || !mask || !total || T <= 0 || G <= 0 || nrows < 0) return -22;
    if (nrows == 0) return 0;
    hipLaunchKernelGGL(k_pre_row_total, dim3(pre_blocks(nrows)), dim3(256), 0, (hipStream_t)stream, indptr, cidx, val, tp_off, T,
                       G, mask, total);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_sparkx_moments(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int P,
                          const int *pair_t, const int *pair_g, const int *rowmap, const double *xt, double *mom, void *stream) {
    if (!colptr || !ridx || !val || !tp_off || !pair_t || !pair_g || !rowmap || !xt || !mom || P < 0) return -22;
    if (P == 0) return 0;
    hipLaunchKernelGGL(k_sparkx_moments, dim3(pre_blocks(P)), dim3(256), 0, (hipStream_t)stream, colptr, ridx, val, tp_off, P,
                       pair_t, pair_g, rowmap, xt, mom);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_sparkx_pvals(const double *mom, int P, const int *pair_t, const int *nkeep, const double *inv, const double *lam,
                        int nodes, double *stat, double *pval, double *comb, void *stream) {
    if (!mom || !pair_t || !nkeep || !inv || !lam || !stat || !pval || !comb || P < 0 || nodes < 1) return -22;
    if (P == 0) return 0;
    hipLaunchKernelGGL(k_sparkx_pvals, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, mom, P, pair_t, nkeep, inv, lam,
                       nodes, stat, pval, comb);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_pre_lognorm_stats(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int T, int S,
                             const int *cols, const double *total, double target, double *mean, double *stdv, void *stream) {
    if (!colptr || !ridx || !val || !tp_off || !cols || !total || !mean || !stdv || T <= 0 || S < 0) return -22;
    if (S == 0) return 0;
    hipLaunchKernelGGL(k_pre_lognorm_stats, dim3(pre_blocks((long long)T * S)), dim3(256), 0, (hipStream_t)stream, colptr, ridx,
                       val, tp_off, T, S, cols, total, target, mean, stdv);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_pre_scale_write(const long long *indptr, const int *cidx, const float *val, const int *tp_off, int T, int S,
                           const int *colpos, const double *total, double target, const double *mean, const double *stdv,
                           double clip, int nrows, float *out, void *stream) {
    if (!indptr || !cidx || !val || !tp_off || !colpos || !total || !mean || !stdv || !out || T <= 0 || S < 0 || nrows < 0)
        return -22;
    if (S == 0 || nrows == 0) return 0;
    const int ntile = (S + PRE_TILE - 1) / PRE_TILE;
    const int width = (S + ntile - 1) / ntile;                   // equal tiles, each <= PRE_TILE columns (<= 60 KB of LDS)
    const dim3 grid((unsigned)nrows, (unsigned)ntile);
    hipLaunchKernelGGL(k_pre_scale_write, grid, dim3(256), sizeof(float) * (size_t)width, (hipStream_t)stream, indptr, cidx, val,
                       tp_off, T, S, colpos, total, target, mean, stdv, clip, width, out);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
