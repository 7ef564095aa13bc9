// crossmoran.hip -- the cross sums behind the bivariate Moran's I of every pair of selected genes of every time point, observed and
// under relabelings of the spots (gfx950, wave64).  The definition is restated in numpy in tests/modules_ref.py.
//
// A time point is a CSR over its n spots (rowptr [n + 1] from 0 to E, col [E]: the out-neighbours of a spot in edge-list order)
// and the rows row0 .. row0 + n - 1 of a CSC matrix; selected gene j (genes[j]) has the fp32 values v of its stored entries (0
// elsewhere) and the centre c.  Both entries work on two dense fp64 images [zrows, GP], GP = the selected genes rounded up to a
// multiple of 16, in which time point t owns the rows zoff .. zoff + npad - 1, npad = n rounded up to a multiple of 4:
//     Z[zoff + i, j] = (double)v_i - c                                   (0.0 in the rows i >= n and in the columns j >= ng)
//     Y[zoff + i, j] = ((0 + Z[zoff + j1, j]) + Z[zoff + j2, j]) + ...   over the row of i in row order (0.0 in the padding)
// -- subtractions and additions only: the bits are those of numpy and of the lag of localmoran.hip.
//
// spadot_cross_dense   k_cross_fill writes 0 - c (0.0 in the padding), k_cross_scatter overwrites the stored entries with v - c
//                      (one workgroup per (selected gene, time point): no two threads write one element) and k_cross_lag walks
//                      the CSR row of every (spot, column) sequentially.  No atomics.  Without a CSC (colptr null) Z is the
//                      caller's and only the lag is taken: the dense columns.
// spadot_cross_sums    M[t, l, g, h] = sum_i Z[zoff + pi_l(i), g] Y[zoff + i, h] on the fp64 matrix cores.  One workgroup of four
//                      wavefronts per (time point, labeling, 64 x 64 tile of M); wavefront w owns the 32 x 32 quarter (w & 1, w >>
//                      1) as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64 and runs over ALL the spots of the time point, four a
//                      step, in ascending order: the order of the additions depends on n alone, not on G, the tile, the batch,
//                      the labelings of the call or the wavefront.  The A operand is the gathered row pi(i) of Z, read from
//                      global memory (no permuted copy of Z exists): every 256 spots the workgroup evaluates pi once per spot
//                      into 1 KiB of LDS, the only LDS of the kernel.  The rows n .. npad - 1 are zero in both images and map to
//                      themselves, so the last step needs no conditional load; a 16-column block past GP is clamped to the
//                      last block of the image (computed twice, stored once).
//                      Operand layout (v_mfma_f64_16x16x4_f64): lane L gives A[row L & 15][k L >> 4] and B[k L >> 4][col L & 15]
//                      and holds D[row (L >> 4) + 4 r][col L & 15] in register r.
#include <hip/hip_runtime.h>

#include "../../include/spadot_model.h"
#include "csc_image.h"

#define CM_DESC 9                  // int64 columns of a time point's descriptor (include/spadot_model.h)
#define CM_THREADS 256             // four wavefronts: 2 x 2 quarters of a tile
#define CM_TILE 64                 // rows and columns of M per workgroup
#define CM_KB 256                  // spots per evaluation of the permutation (one per thread)
#define CM_MAX_G 4096
#define CM_MAX 2147483647LL

typedef double cm_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ long long cm_pad4(long long n) { return (n + 3) & ~3LL; }

// what the kernels take from a row of the device descriptor: nothing outside the images whatever it holds
struct CmTp {
    long long eoff, n, E, row0, gid, roff, zoff, npad;
    bool ok;
};

__device__ __forceinline__ CmTp cm_tp(const long long *__restrict__ desc, int t, long long zrows) {
    const long long *d = desc + (long long)t * CM_DESC;
    CmTp a;
    a.eoff = d[0], a.n = d[1], a.E = d[2], a.row0 = d[3], a.gid = d[4], a.roff = d[5], a.zoff = d[8];
    a.ok = a.n >= 1 && a.n <= CM_MAX && a.zoff >= 0 && a.zoff <= zrows;
    a.npad = a.ok ? cm_pad4(a.n) : 0;
    a.ok = a.ok && a.npad <= zrows - a.zoff;
    return a;
}

__global__ void __launch_bounds__(256) k_cross_fill(const double *__restrict__ centre, const long long *__restrict__ desc, int G,
                                                     const int *__restrict__ genes, int ng, int GP, long long zrows,
                                                     double *__restrict__ Z) {
    const int t = blockIdx.y;
    const CmTp a = cm_tp(desc, t, zrows);
    if (!a.ok) return;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.npad * GP) return;
    const long long i = idx / GP;
    const int j = (int)(idx - i * GP);
    const int g = csc_gene(genes[j < ng ? j : 0], G);
    const double c = centre[(long long)t * G + g];
    Z[(a.zoff + i) * GP + j] = (i < a.n && j < ng) ? 0.0 - c : 0.0;
}

__global__ void __launch_bounds__(256) k_cross_scatter(const long long *__restrict__ colptr, const int *__restrict__ ridx,
                                                        const float *__restrict__ vals, long long nnz,
                                                        const double *__restrict__ centre, const long long *__restrict__ desc,
                                                        int G, const int *__restrict__ genes, int GP, long long zrows,
                                                        double *__restrict__ Z) {
    __shared__ long long seg[2];
    const int j = blockIdx.x, t = blockIdx.y;
    const CmTp a = cm_tp(desc, t, zrows);
    if (!a.ok) return;
    const int g = csc_gene(genes[j], G);
    if (threadIdx.x < 2)                                 // the rows of this time point in the gene's column: two lower bounds
        seg[threadIdx.x] = csc_lower_bound(ridx, colptr[g], colptr[g + 1], nnz, a.row0 + (threadIdx.x ? a.n : 0LL));
    __syncthreads();
    const double c = centre[(long long)t * G + g];
    const long long hi = seg[1];
    for (long long idx = seg[0] + threadIdx.x; idx < hi; idx += 256) {
        const long long r = (long long)ridx[idx] - a.row0;
        if (r >= 0 && r < a.n) Z[(a.zoff + r) * GP + j] = (double)vals[idx] - c;   // true between the bounds of a sorted column
    }
}

__global__ void __launch_bounds__(256) k_cross_lag(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                    const long long *__restrict__ desc, int GP, long long zrows,
                                                    const double *__restrict__ Z, double *__restrict__ Y) {
    const int t = blockIdx.y;
    const CmTp a = cm_tp(desc, t, zrows);
    if (!a.ok) return;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.npad * GP) return;
    const long long i = idx / GP;
    const int j = (int)(idx - i * GP);
    double acc = 0.0;
    if (i < a.n) {
        // a neighbour out of range (refused on the host as the rowptr is) reads spot 0 and is not added
        const int *cl = col + a.eoff;
        long long r0, r1;
        csr_row(rowptr + a.roff, i, a.E, r0, r1);
        for (long long e = r0; e < r1; ++e) {
            const long long nb = cl[e];
            const bool ok = nb >= 0 && nb < a.n;
            const double s = acc + Z[(a.zoff + (ok ? nb : 0)) * GP + j];
            acc = ok ? s : acc;
        }
    }
    Y[(a.zoff + i) * GP + j] = acc;
}

__global__ void __launch_bounds__(CM_THREADS) k_cross_sums(const double *__restrict__ Z, const double *__restrict__ Y,
                                                            long long zrows, int GP, const long long *__restrict__ desc, int T,
                                                            int ng, int tiles, int observed, long long L, long long first,
                                                            unsigned long long seed, double *__restrict__ M) {
    __shared__ unsigned at[CM_KB];
    const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long per = (long long)tiles * tiles, item = blockIdx.x;
    const long long tl = item / per, tile = item - tl * per;
    const int t = (int)(tl / L);
    const long long l = tl - (long long)t * L;
    if (t >= T) return;
    const CmTp a = cm_tp(desc, t, zrows);
    if (!a.ok) return;
    const int tg = (int)(tile / tiles), th = (int)(tile - (long long)tg * tiles);
    const bool perm = !(observed && l == 0);
    NhPerm q = {};
    if (perm) q = nh_perm_setup(seed, (unsigned long long)a.gid, (unsigned long long)(first + l - observed), (unsigned)a.n);

    // the four 16-column blocks of the wavefront: two of Z (rows of M) and two of Y (columns of M); a block past the image is
    // clamped to the last one and not stored
    const int last = GP - 16, sub = lane & 15, kq = lane >> 4;
    int gb[2], hb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        gb[s] = tg * CM_TILE + (int)(w & 1) * 32 + s * 16;
        hb[s] = th * CM_TILE + (int)(w >> 1) * 32 + s * 16;
    }
    const double *za0 = Z + a.zoff * GP + (gb[0] < last ? gb[0] : last) + sub;
    const double *za1 = Z + a.zoff * GP + (gb[1] < last ? gb[1] : last) + sub;
    const double *yb0 = Y + a.zoff * GP + (hb[0] < last ? hb[0] : last) + sub;
    const double *yb1 = Y + a.zoff * GP + (hb[1] < last ? hb[1] : last) + sub;

    cm_d4 acc00 = {0, 0, 0, 0}, acc01 = {0, 0, 0, 0}, acc10 = {0, 0, 0, 0}, acc11 = {0, 0, 0, 0};
    for (long long c0 = 0; c0 < a.npad; c0 += CM_KB) {
        __syncthreads();                                 // the steps of the chunk before have read `at`
        {
            const long long i = c0 + tid;                // rows n .. npad - 1 are zero and map to themselves; beyond: unused
            const unsigned ii = (unsigned)(i < a.npad ? i : a.npad - 1);
            at[tid] = (perm && i < a.n) ? nh_perm_at(q, ii) : ii;
        }
        __syncthreads();
        const long long left = a.npad - c0;
        const int steps = (int)((left < CM_KB ? left : CM_KB) >> 2);
        const double *y0 = yb0 + c0 * GP, *y1 = yb1 + c0 * GP;
#pragma unroll 4
        for (int ks = 0; ks < steps; ++ks) {
            const int k = ks * 4 + kq;
            const long long ar = (long long)at[k] * GP, br = (long long)k * GP;
            const double a0 = za0[ar], a1 = za1[ar], b0 = y0[br], b1 = y1[br];
            acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc11, 0, 0, 0);
        }
    }
    double *out = M + tl * ng * ng;
#define CM_STORE(ACC, S, U)                                                                          \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                 \
        const int g = gb[S] + kq + 4 * r, h = hb[U] + sub;                                           \
        if (g < ng && h < ng) out[(long long)g * ng + h] = ACC[r];                                   \
    }
    CM_STORE(acc00, 0, 0)
    CM_STORE(acc01, 0, 1)
    CM_STORE(acc10, 1, 0)
    CM_STORE(acc11, 1, 1)
#undef CM_STORE
}

// the checks that both entries share; the rows of the images the time points need, or < 0: the return code
static long long cm_desc_check(const long long *desc_host, int T, long long zrows, bool graph, long long *most_rows,
                               long long *most_cells) {
    long long most = 0, cells = 0;
    for (int t = 0; t < T; ++t) {
        const long long *d = desc_host + (long long)t * CM_DESC;
        const long long eoff = d[0], n = d[1], E = d[2], row0 = d[3], gid = d[4], roff = d[5], zoff = d[8];
        if (eoff < 0 || n < 1 || E < 0 || row0 < 0 || gid < 0 || roff < 0 || zoff < 0) return -22;
        if (n > CM_MAX || E > CM_MAX || gid > CM_MAX || row0 > CM_MAX) return -7;
        if (graph && E > 0 && (d[6] < 0 || d[7] >= n)) return -7;                // the smallest and the largest neighbour
        const long long npad = (n + 3) & ~3LL;
        if (zoff > zrows || npad > zrows - zoff) return -22;
        if (row0 + n > most) most = row0 + n;
        if (npad > cells) cells = npad;
    }
    *most_rows = most;
    *most_cells = cells;
    return 0;
}

extern "C" int spadot_cross_dense(const int *rowptr, const int *col, const long long *colptr, const int *ridx, const float *vals,
                                  long long nnz, long long ridx_lo, long long ridx_hi, const double *centre,
                                  const long long *desc_host, const long long *desc_dev, int T, int G, const int *genes, int ng,
                                  int gene_lo, int gene_hi, int GP, long long zrows, double *Z, double *Y, void *stream) {
    const bool csc = colptr != nullptr;
    if (!rowptr || !desc_host || !desc_dev || !Z || !Y) return -22;
    if (T <= 0 || ng < 1 || zrows < 1 || nnz < 0) return -22;
    if (csc && (!centre || !genes || G <= 0 || (nnz > 0 && (!ridx || !vals)))) return -22;
    if (ng > CM_MAX_G || T > 65535 || nnz > CM_MAX) return -7;
    if (GP != ((ng + 15) & ~15)) return -22;
    if (csc && (gene_lo < 0 || gene_hi >= G)) return -7;
    long long most = 0, cells = 0;
    const long long rc = cm_desc_check(desc_host, T, zrows, true, &most, &cells);
    if (rc) return (int)rc;
    for (int t = 0; t < T; ++t)
        if (desc_host[(long long)t * CM_DESC + 2] > 0 && !col) return -22;
    if (csc && nnz > 0 && (ridx_lo < 0 || ridx_hi >= most)) return -7;           // the smallest and the largest row index
    const long long blocks = (cells * GP + 255) / 256;
    if (blocks > CM_MAX) return -7;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks, (unsigned)T);
    if (csc) {
        hipLaunchKernelGGL(k_cross_fill, grid, dim3(256), 0, s, centre, desc_dev, G, genes, ng, GP, zrows, Z);
        hipLaunchKernelGGL(k_cross_scatter, dim3((unsigned)ng, (unsigned)T), dim3(256), 0, s, colptr, ridx, vals, nnz, centre,
                           desc_dev, G, genes, GP, zrows, Z);
    }
    hipLaunchKernelGGL(k_cross_lag, grid, dim3(256), 0, s, rowptr, col, desc_dev, GP, zrows, (const double *)Z, Y);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int spadot_cross_sums(const double *Z, const double *Y, long long zrows, int GP, const long long *desc_host,
                                 const long long *desc_dev, int T, int ng, int observed, long long first, long long P,
                                 long long seed, double *M, void *stream) {
    if (!Z || !Y || !desc_host || !desc_dev || !M) return -22;
    if (T <= 0 || ng < 1 || zrows < 1 || P < 0 || first < 0 || (observed != 0 && observed != 1) || observed + P < 1) return -22;
    if (ng > CM_MAX_G || first + P > 4294967296LL) return -7;
    if (GP != ((ng + 15) & ~15)) return -22;
    long long most = 0, cells = 0;
    const long long rc = cm_desc_check(desc_host, T, zrows, false, &most, &cells);
    if (rc) return (int)rc;
    const long long L = observed + P, tiles = (ng + CM_TILE - 1) / CM_TILE;
    if (L > CM_MAX / (tiles * tiles) || T > CM_MAX / (L * tiles * tiles)) return -7;
    const long long items = T * L * tiles * tiles;
    hipLaunchKernelGGL(k_cross_sums, dim3((unsigned)items), dim3(CM_THREADS), 0, (hipStream_t)stream, Z, Y, zrows, GP, desc_dev, T,
                       ng, (int)tiles, observed, L, first, (unsigned long long)seed, M);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
