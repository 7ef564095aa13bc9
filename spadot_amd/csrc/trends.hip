// trends.hip -- the trends stage's device work (gfx950, wave64): the sparse log-normalised counts of every time point, transposed,
// times a skinny dense fp64 matrix W[n, C], as three weighted moments per (time point, gene, column) in one pass over the
// stored entries:
//     S0[t,g,c] = sum W[i,c],   S1[t,g,c] = sum v_ig W[i,c],   S2[t,g,c] = sum v_ig^2 W[i,c]
// over the stored entries (i, g) whose row i lies in time point t (v converted to fp64, v^2 formed once in fp64).
//
// Data layout as preprocess.hip and markers.hip: CSC (genes x spots), rows in output order, a time point t owns the rows
// [tp_off[t], tp_off[t+1]), so a gene's column splits into one contiguous segment per time point (binary search).
//
// k_tr_moments<NJ, VW>   one 256-thread workgroup per (time point, gene); consecutive workgroups share a time point, so its rows
//                    of W (a few MB) stay in L2 / Infinity Cache.  The segment's (row, v) pairs are staged once, TR_CHUNK at a
//                    time, into LDS with coalesced loads.  Lanes map to columns, waves to stored entries: with VW = 1 lane l of
//                    every wavefront owns the columns l, l + 64, ..., l + 64 (NJ - 1), so a stored entry costs one wave NJ
//                    loads of 512 contiguous bytes of its row of W (the row index is wave-uniform: a scalar base, no per-lane
//                    address arithmetic) and 3 NJ fp64 instructions per lane into accumulators that are indexed by unrolled
//                    constants only.  VW = 2 (-DTR_VW=2, the mapping it was measured against: DESIGN 7f) gives a lane two
//                    adjacent columns per 16-byte load.  Wavefront w takes the entries w, w + 4, w + 8, ... of the segment in
//                    that order, whatever C is; the four partial sums are then added as ((p0 + p1) + p2) + p3 through LDS.
//                    So every output element is summed in an order that depends only on the position of each entry inside
//                    its segment: no floating-point atomics, two runs give the same bits, and a column alone, or a problem
//                    inside another batch, gives the bits it gives here.
//                    Loads are unconditional: a lane whose column is past C reads inside the row's end and does not store;
//                    the trip counts are wave-uniform.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/spadot_model.h"
#include "csc_walk.h"

#define TR_THREADS 256
#define TR_WAVE 64
#define TR_WAVES (TR_THREADS / TR_WAVE)
#define TR_CHUNK 1024              // stored entries staged in LDS at a time: 8 KiB; a multiple of TR_WAVES
#define TR_MAX_C 1024              // columns of W: 16 per lane
#ifndef TR_VW
#define TR_VW 1                    // columns per load and lane: 1 (8-byte loads) or 2 (16-byte loads)
#endif

// one stored entry (row i, value x) into the lane's accumulators; w: the lane's NJ columns of row i
template <int NJ>
__device__ __forceinline__ void tr_add(const double (&w)[NJ], float x, double (&a0)[NJ], double (&a1)[NJ], double (&a2)[NJ]) {
    const double xd = (double)x, xx = xd * xd;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        a0[j] += w[j];
        a1[j] = fma(xd, w[j], a1[j]);
        a2[j] = fma(xx, w[j], a2[j]);
    }
}

// columns c, c + 1 of a row (8-byte aligned: C may be odd) as one 16-byte load
__device__ __forceinline__ void tr_load2(const double *p, double &x, double &y) {
    double t[2];
    __builtin_memcpy(t, p, 16);
    x = t[0]; y = t[1];
}

template <int NJ, int VW>
__global__ void __launch_bounds__(TR_THREADS) k_tr_moments(const long long *__restrict__ colptr, const int *__restrict__ ridx,
                                                           const float *__restrict__ v, const int *__restrict__ tp_off, int G,
                                                           const double *__restrict__ W, int C, double *__restrict__ S0,
                                                           double *__restrict__ S1, double *__restrict__ S2) {
    constexpr int NS = NJ / VW;                          // loads per entry and lane, VW columns each
    constexpr int U = NJ <= 4 ? 4 : (NJ <= 8 ? 2 : 1);   // entries in flight per wave: U * NS loads of VW * 512 B
    __shared__ int s_row[TR_CHUNK];
    __shared__ float s_val[TR_CHUNK];
    __shared__ double s_part[2][TR_WAVES - 1][3][TR_WAVE * VW];
    const int tid = threadIdx.x, lane = tid & (TR_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long item = blockIdx.x;
    const int t = (int)(item / G), g = (int)(item % G);
    const long long lo = csc_walk_lower_bound(ridx, colptr[g], colptr[g + 1], tp_off[t]);
    const long long hi = csc_walk_lower_bound(ridx, lo, colptr[g + 1], tp_off[t + 1]);
    const int m = (int)(hi - lo);                        // <= the spots of the time point < 2^31

    // slot s of the lane: the columns VW * (lane + 64 s) .. + VW - 1, as accumulators s * VW .. ; a load past the row's end is
    // moved back inside it (VW = 2, C >= 2: to C - 2, and the lane whose first column is C - 1 takes the second value)
    int col[NS];
    bool second[NS];
    double a0[NJ], a1[NJ], a2[NJ];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = VW * (lane + TR_WAVE * s);
        col[s] = min(c, C - VW);
        second[s] = VW == 2 && c == C - 1;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) { a0[j] = 0.0; a1[j] = 0.0; a2[j] = 0.0; }

    for (int c0 = 0; c0 < m; c0 += TR_CHUNK) {
        const int len = min(TR_CHUNK, m - c0);
        if (c0) __syncthreads();                         // every wave is through with the chunk before
        for (int i = tid; i < len; i += TR_THREADS) {
            s_row[i] = ridx[lo + c0 + i];
            s_val[i] = v[lo + c0 + i];
        }
        __syncthreads();
        int p = wave;                                    // TR_CHUNK is a multiple of TR_WAVES: position c0 + p belongs to wave
        for (; p + (U - 1) * TR_WAVES < len; p += U * TR_WAVES) {
            double w[U][NJ];
            float x[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const long long row = __builtin_amdgcn_readfirstlane(s_row[p + k * TR_WAVES]);
                x[k] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s_val[p + k * TR_WAVES])));
                const double *wr = W + row * C;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (VW == 1) {
                        w[k][s] = wr[col[s]];
                    } else {
                        tr_load2(wr + col[s], w[k][2 * s], w[k][2 * s + 1]);
                        if (second[s]) w[k][2 * s] = w[k][2 * s + 1];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < U; ++k) tr_add<NJ>(w[k], x[k], a0, a1, a2);
        }
        for (; p < len; p += TR_WAVES) {
            double w[NJ];
            const long long row = __builtin_amdgcn_readfirstlane(s_row[p]);
            const float x = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s_val[p])));
            const double *wr = W + row * C;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (VW == 1) {
                    w[s] = wr[col[s]];
                } else {
                    tr_load2(wr + col[s], w[2 * s], w[2 * s + 1]);
                    if (second[s]) w[2 * s] = w[2 * s + 1];
                }
            }
            tr_add<NJ>(w, x, a0, a1, a2);
        }
    }

    // ((p0 + p1) + p2) + p3 per column, one slot at a time; the LDS rows alternate, so one barrier per step is enough
    const long long out = item * C;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (TR_WAVE * VW * s < C) {                      // uniform over the workgroup
            double(*part)[3][TR_WAVE * VW] = s_part[s & 1];
            if (wave > 0) {
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    part[wave - 1][0][lane * VW + e] = a0[s * VW + e];
                    part[wave - 1][1][lane * VW + e] = a1[s * VW + e];
                    part[wave - 1][2][lane * VW + e] = a2[s * VW + e];
                }
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    double r0 = a0[s * VW + e], r1 = a1[s * VW + e], r2 = a2[s * VW + e];
#pragma unroll
                    for (int q = 0; q < TR_WAVES - 1; ++q) {
                        r0 += part[q][0][lane * VW + e];
                        r1 += part[q][1][lane * VW + e];
                        r2 += part[q][2][lane * VW + e];
                    }
                    const int c = VW * (lane + TR_WAVE * s) + e;
                    if (c < C) {
                        S0[out + c] = r0;
                        S1[out + c] = r1;
                        S2[out + c] = r2;
                    }
                }
            }
        }
    }
}

template <int NJ, int VW>
static int tr_launch(const long long *colptr, const int *ridx, const float *v, const int *tp_off, int T, int G, const double *W,
                     int C, double *S0, double *S1, double *S2, hipStream_t st) {
    hipLaunchKernelGGL((k_tr_moments<NJ, VW>), dim3((unsigned)((long long)T * G)), dim3(TR_THREADS), 0, st, colptr, ridx, v, tp_off, G,
                       W, C, S0, S1, S2);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// the smallest instance whose lanes hold every column: NJ accumulator sets per lane, loaded VW columns at a time
template <int VW>
static int tr_dispatch(const long long *colptr, const int *ridx, const float *v, const int *tp_off, int T, int G, const double *W,
                       int C, double *S0, double *S1, double *S2, hipStream_t st) {
    const int nj = VW * ((C + VW * TR_WAVE - 1) / (VW * TR_WAVE));
    if constexpr (VW == 1) {
        if (nj <= 1) return tr_launch<1, 1>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
        if (nj == 3) return tr_launch<3, 1>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
    }
    if (nj <= 2) return tr_launch<2, VW>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
    if (nj <= 4) return tr_launch<4, VW>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
    if (nj <= 6) return tr_launch<6, VW>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
    if (nj <= 8) return tr_launch<8, VW>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
    if (nj <= 12) return tr_launch<12, VW>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
    return tr_launch<16, VW>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
}

extern "C" {

int spadot_weighted_moments_chunk(void) { return TR_CHUNK; }

int spadot_weighted_moments(const long long *colptr, const int *ridx, const float *v, const int *tp_off, int T, int G,
                            const double *W, long long n, int C, double *S0, double *S1, double *S2, void *stream) {
    if (!colptr || !ridx || !v || !tp_off || !W || !S0 || !S1 || !S2 || T <= 0 || G <= 0 || n <= 0) return -22;
    if (C < 1 || C > TR_MAX_C || n > 0x7fffffffll || (long long)T * G > 0x7fffffffll) return -7;
    hipStream_t st = (hipStream_t)stream;
    if constexpr (TR_VW == 2) {
        if (C >= 2) return tr_dispatch<2>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
    }
    return tr_dispatch<1>(colptr, ridx, v, tp_off, T, G, W, C, S0, S1, S2, st);
}

}  // extern "C"
