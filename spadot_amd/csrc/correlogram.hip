// correlogram.hip -- the sums behind the spatial correlogram of many (time point, gene, labeling) problems (gfx950, wave64;
// DESIGN 7o).  The definition is restated in numpy in tests/correlogram_ref.py.
//
// A time point is n spots with fp64 coordinates and B squared thresholds r2[0] < .. < r2[B-1].  Band b holds the ordered pairs
// (i, j), i != j, with r2[b-1] < d2(i, j) <= r2[b] (r2[-1] below 0: coincident spots fall into band 0), d2 the unfused squared
// distance pc_d2 of pair_count.h.  cnt_b(i): the partners of spot i in band b.  With x the centred values of a column (a selected
// gene under a labeling), read from the fp64 image Z of spadot_cross_dense at row pi_l(original index):
//     W[b] = sum_i cnt_b(i),   S2c[b] = sum_i cnt_b(i)^2                                         (int64, exact)
//     N[b] = sum over the pairs of band b of x_i x_j,   Q[b] = sum_i cnt_b(i) x_i^2             (fp64, a fixed order)
// The host hands the spots of a time point over in Morton order with `order`, position -> original index: positions give the
// tiles, original indices go into the Feistel network.
//
// k_corr_boxes   the bounding box of every block of 256 positions (min / max: no order to fix).
// k_corr<CS>     one 256-thread workgroup per (256 query positions, labeling and chunk of CS genes, time point); a thread owns one
//                query spot.  The spots of the time point stream through LDS in tiles of 256: double2 coordinates and the CS
//                centred values of every tile spot, whose row of Z is evaluated while the tile is loaded (no permuted copy, no
//                stored permutation).  The band of a pair is a branch-free count of the thresholds below d2 (padded to 16 with
//                +inf) and serves all CS columns.  lag[b][c] and cnt[b] of a thread are indexed by a runtime band: they live in
//                LDS as [b][c][thread], so the 32 lanes of a half wave touch 32 consecutive doubles whatever their bands are (no
//                bank conflict), and a thread only ever touches its own column (no barrier, no atomic).  A tile whose box lies
//                further than r2[B-1] from the box of the query block is skipped: the boxes are made of the coordinates
//                themselves and the gap by the same rounded subtraction, fl is monotone, so every d2 of a skipped tile is above
//                r2[B-1] and the tile holds no pair of any band -- culling changes no bit.  A thread adds its partners in
//                ascending position; the workgroup adds x_i lag_i and cnt_b(i) x_i^2 over its threads by a fixed shuffle tree
//                and in wave order into one partial per (block, column, band).  W and S2c: 64-bit integer atomics, from the
//                workgroups of column chunk 0 only.
// k_corr_reduce  adds the partials of a (time point, column, band) in ascending block order.  No floating-point atomics anywhere.
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/spadot_model.h"
#include "feistel_perm.h"
#include "pair_count.h"
#include "per_device.h"

#define CG_DESC 6                  // int64 columns of a time point's descriptor (include/spadot_model.h)
#define CG_MAX_B 16
#define CG_MAX_G 4096              // selected genes, as spadot_cross_dense
#define CG_LDS_BYTES 163840

// what the kernels take from a row of the device descriptor: nothing outside the arrays whatever it holds (the host refuses it)
struct CgTp {
    long long off, n, gid, zoff, blk0;
    int B;
    bool ok;
};

__device__ __forceinline__ CgTp cg_tp(const long long *__restrict__ desc, int t, int B_max, long long zrows) {
    const long long *d = desc + (long long)t * CG_DESC;
    CgTp a;
    a.off = d[0], a.n = d[1], a.gid = d[3], a.zoff = d[4], a.blk0 = d[5];
    a.B = (int)min(max(d[2], 1ll), (long long)min(B_max, CG_MAX_B));
    a.ok = a.off >= 0 && a.n >= 1 && a.n <= PC_MAX_N && a.blk0 >= 0 && a.zoff >= 0 && a.zoff <= zrows &&
           ((a.n + 3) & ~3ll) <= zrows - a.zoff;
    return a;
}

__global__ void __launch_bounds__(PC_THREADS) k_corr_boxes(const double2 *__restrict__ xy, const long long *__restrict__ desc,
                                                            int B_max, double *__restrict__ boxes) {
    __shared__ double s[4][PC_THREADS];
    const int t = blockIdx.y, tid = threadIdx.x;
    const CgTp a = cg_tp(desc, t, B_max, 0x7fffffffffffffffll);
    const long long q0 = (long long)blockIdx.x * PC_THREADS;
    if (!a.ok || q0 >= a.n) return;
    const double2 p = xy[a.off + min(q0 + tid, a.n - 1)];
    s[0][tid] = p.x, s[1][tid] = p.x, s[2][tid] = p.y, s[3][tid] = p.y;
    for (int w = PC_THREADS / 2; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) {
            s[0][tid] = fmin(s[0][tid], s[0][tid + w]);
            s[1][tid] = fmax(s[1][tid], s[1][tid + w]);
            s[2][tid] = fmin(s[2][tid], s[2][tid + w]);
            s[3][tid] = fmax(s[3][tid], s[3][tid + w]);
        }
    }
    if (tid == 0) {
        double *b = boxes + (a.blk0 + blockIdx.x) * 4;
        b[0] = s[0][0], b[1] = s[1][0], b[2] = s[2][0], b[3] = s[3][0];
    }
}

// the gap between two intervals by the subtraction of the definition: no |x_i - x_j| of their points is below it
__device__ __forceinline__ double cg_gap(double lo_a, double hi_a, double lo_b, double hi_b) {
    return fmax(0.0, fmax(lo_a - hi_b, lo_b - hi_a));
}

template <int CS>
__global__ void __launch_bounds__(PC_THREADS) k_corr(const double2 *__restrict__ xy, const int *__restrict__ order,
                                                      const double *__restrict__ Z, long long zrows, int GP,
                                                      const long long *__restrict__ desc, const double *__restrict__ r2, int ng,
                                                      int B_max, int observed, unsigned long long first, int L,
                                                      unsigned long long seed, int cull, const double *__restrict__ boxes,
                                                      double *__restrict__ part, unsigned long long *__restrict__ W,
                                                      unsigned long long *__restrict__ S2c, unsigned long long *__restrict__ skipped) {
    extern __shared__ double smem[];
    double *lag = smem;                                                      // [B_max][CS][256]
    double *tv = lag + (size_t)B_max * CS * PC_THREADS;                      // [CS][256]: the values of the tile
    double2 *txy = reinterpret_cast<double2 *>(tv + CS * PC_THREADS);        // [256]: its coordinates; at the end the wave sums
    int *cnt = reinterpret_cast<int *>(txy + PC_THREADS);                    // [B_max][256]

    const int t = blockIdx.z, tid = threadIdx.x;
    const CgTp a = cg_tp(desc, t, B_max, zrows);
    const long long q0l = (long long)blockIdx.x * PC_THREADS;
    if (!a.ok || q0l >= a.n) return;                     // uniform: the grid is sized for the largest time point
    const int chunks = (ng + CS - 1) / CS;
    const int l = blockIdx.y / chunks, j0 = (blockIdx.y - l * chunks) * CS;  // j0 + CS <= GP: GP is a multiple of 16
    if (l >= L) return;
    const int n = (int)a.n, B = a.B, q0 = (int)q0l;
    const double2 *pts = xy + a.off;
    const int *ord = order + a.off;
    double th[CG_MAX_B];
#pragma unroll
    for (int k = 0; k < CG_MAX_B; ++k) th[k] = r2[(long long)t * CG_MAX_B + k];
    const double r_max = r2[(long long)t * CG_MAX_B + B - 1];
    const int s = observed ? l : l + 1;                  // the global labeling: 0 the identity, s >= 1 permutation first + s - 1
    const bool relabeled = s >= 1;                       // uniform
    NhPerm pi = {};
    if (relabeled) pi = nh_perm_setup(seed, (unsigned long long)a.gid, first + (unsigned long long)(s - 1), (unsigned)n);
    auto row = [&](int pos) -> const double * {          // the CS values that position pos shows in this labeling, 0 <= pos < n
        const unsigned o = (unsigned)min(max(ord[pos], 0), n - 1);
        return Z + (a.zoff + (long long)(relabeled ? nh_perm_at(pi, o) : o)) * GP + j0;
    };
    const int q = q0 + tid;
    const bool on = q < n;
    const double2 me = pts[on ? q : n - 1];              // idle lanes follow a valid spot and add nothing
    double xi[CS];
    {
        const double *z = row(on ? q : n - 1);
#pragma unroll
        for (int c = 0; c < CS; ++c) xi[c] = on ? z[c] : 0.0;
    }
    for (int b = 0; b < B; ++b) {                        // a thread's own column of LDS: no barrier before it is used
        cnt[b * PC_THREADS + tid] = 0;
#pragma unroll
        for (int c = 0; c < CS; ++c) lag[(b * CS + c) * PC_THREADS + tid] = 0.0;
    }
    const double *qb = boxes + (a.blk0 + blockIdx.x) * 4;
    const double qx0 = qb[0], qx1 = qb[1], qy0 = qb[2], qy1 = qb[3];

    for (int t0 = 0; t0 < n; t0 += PC_THREADS) {
        if (cull) {                                      // uniform
            const double *tb = boxes + (a.blk0 + t0 / PC_THREADS) * 4;
            if (pc_d2(cg_gap(qx0, qx1, tb[0], tb[1]), cg_gap(qy0, qy1, tb[2], tb[3]), 0.0, 0.0) > r_max) {
                if (skipped && blockIdx.y == 0 && tid == 0) atomicAdd(skipped, 1ull);
                continue;
            }
        }
        const int m = min(PC_THREADS, n - t0);
        __syncthreads();                                 // the previous tile is read
        if (tid < m) {
            txy[tid] = pts[t0 + tid];
            const double *z = row(t0 + tid);
#pragma unroll
            for (int c = 0; c < CS; ++c) tv[c * PC_THREADS + tid] = z[c];
        }
        __syncthreads();
        for (int jj = 0; jj < m; ++jj) {                 // ascending position
            const double e = pc_dist(me, txy[jj], t0 + jj, q);
            int band = 0;
#pragma unroll
            for (int k = 0; k < CG_MAX_B; ++k) band += (int)(th[k] < e);
            if (on && band < B) {
                cnt[band * PC_THREADS + tid] += 1;
#pragma unroll
                for (int c = 0; c < CS; ++c) lag[(band * CS + c) * PC_THREADS + tid] += tv[c * PC_THREADS + jj];
            }
        }
    }

    __syncthreads();                                     // the last tile is read: its place takes the sums of the waves
    double *red = reinterpret_cast<double *>(txy);       // [B][CS][2][4]: at most 512 doubles, the 4 KiB of txy
    const int lane = tid & 63, wave = tid >> 6;
    for (int b = 0; b < B; ++b) {
        const double cb = (double)cnt[b * PC_THREADS + tid];
#pragma unroll
        for (int c = 0; c < CS; ++c) {
            double vn = xi[c] * lag[(b * CS + c) * PC_THREADS + tid];
            double vq = cb * (xi[c] * xi[c]);
#pragma unroll
            for (int w = 32; w > 0; w >>= 1) {
                vn += __shfl_down(vn, w);
                vq += __shfl_down(vq, w);
            }
            if (lane == 0) {
                red[((b * CS + c) * 2 + 0) * 4 + wave] = vn;
                red[((b * CS + c) * 2 + 1) * 4 + wave] = vq;
            }
        }
    }
    if (blockIdx.y == 0) {                               // the integers do not depend on the column: written by chunk 0 alone
        for (int b = 0; b < B; ++b) {
            unsigned long long c1 = (unsigned long long)cnt[b * PC_THREADS + tid], c2 = c1 * c1;
#pragma unroll
            for (int w = 32; w > 0; w >>= 1) {
                c1 += __shfl_down(c1, w);
                c2 += __shfl_down(c2, w);
            }
            if (lane == 0 && c1 != 0ull) {
                atomicAdd(W + (long long)t * B_max + b, c1);
                atomicAdd(S2c + (long long)t * B_max + b, c2);
            }
        }
    }
    __syncthreads();
    const long long ncol = (long long)L * ng;
    for (int i = tid; i < B * CS * 2; i += PC_THREADS) {
        const double sum = ((red[i * 4] + red[i * 4 + 1]) + red[i * 4 + 2]) + red[i * 4 + 3];
        const int b = i / (CS * 2), c = (i >> 1) % CS, j = j0 + c;
        if (j < ng) part[((((a.blk0 + blockIdx.x) * ncol + (long long)l * ng + j) * B_max) + b) * 2 + (i & 1)] = sum;
    }
}

__global__ void __launch_bounds__(256) k_corr_reduce(const long long *__restrict__ desc, const double *__restrict__ part, int T,
                                                     int ng, int L, int B_max, double *__restrict__ N, double *__restrict__ Q) {
    const long long ncol = (long long)L * ng, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)T * ncol * B_max) return;
    const int b = (int)(idx % B_max);
    const long long col = (idx / B_max) % ncol;
    const int t = (int)(idx / (B_max * ncol));
    const CgTp a = cg_tp(desc, t, B_max, 0x7fffffffffffffffll);
    const int l = (int)(col / ng), j = (int)(col - (long long)l * ng);
    double sn = 0.0, sq = 0.0;
    if (a.ok && b < a.B) {
        const long long blocks = (a.n + PC_THREADS - 1) / PC_THREADS;
        for (long long k = 0; k < blocks; ++k) {         // ascending block order
            const double *p = part + (((a.blk0 + k) * ncol + col) * B_max + b) * 2;
            sn = k ? sn + p[0] : p[0];
            sq = k ? sq + p[1] : p[1];
        }
    }
    const long long o = (((long long)t * ng + j) * L + l) * B_max + b;
    N[o] = sn, Q[o] = sq;
}

// the doubles of the scratch buffer: the boxes of every block, then one (N, Q) partial per (block, column, band)
static long long cg_scratch(long long blocks, long long L, long long ng, long long B_max) {
    return blocks * 4 + blocks * L * ng * B_max * 2;
}

template <int CS>
static int cg_launch(dim3 grid, size_t dyn, hipStream_t st, const double *xy, const int *order, const double *Z, long long zrows,
                     int GP, const long long *desc_dev, const double *r2_dev, int ng, int B_max, int observed, long long first, int L,
                     long long seed, int cull, double *scratch, long long blocks, long long *W, long long *S2c, long long *skipped) {
    static PerDeviceFlag attr_set;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_corr<CS>, hipFuncAttributeMaxDynamicSharedMemorySize, CG_LDS_BYTES) != hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL((k_corr<CS>), grid, dim3(PC_THREADS), dyn, st, reinterpret_cast<const double2 *>(xy), order, Z, zrows, GP,
                       desc_dev, r2_dev, ng, B_max, observed, (unsigned long long)first, L, (unsigned long long)seed, cull,
                       (const double *)scratch, scratch + blocks * 4, reinterpret_cast<unsigned long long *>(W),
                       reinterpret_cast<unsigned long long *>(S2c), reinterpret_cast<unsigned long long *>(skipped));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int spadot_corr_sums(const double *xy, const int *order, const double *Z, long long zrows, int GP,
                                const long long *desc_host, const long long *desc_dev, const double *r2_host, const double *r2_dev,
                                int T, int ng, int B_max, int observed, long long first, long long P, long long seed, int cull,
                                int cs, double *scratch, long long scratch_doubles, long long *W, long long *S2c, double *N,
                                double *Q, long long *skipped, void *stream) {
    if (!xy || !order || !Z || !desc_host || !desc_dev || !r2_host || !r2_dev || !scratch || !W || !S2c || !N || !Q) return -22;
    if (T <= 0 || ng < 1 || zrows < 1 || P < 0 || first < 0 || (observed != 0 && observed != 1) || observed + P < 1) return -22;
    if (GP != ((ng + 15) & ~15) || (cull != 0 && cull != 1)) return -22;
    if (cs != 0 && cs != 2 && cs != 4) return -7;
    if (B_max < 1 || B_max > CG_MAX_B || ng > CG_MAX_G || T > PC_MAX_GRID || first + P > 4294967296ll) return -7;
    const int CS = cs ? cs : 2;
    const long long L = observed + P, chunks = (ng + CS - 1) / CS;
    if (L > PC_MAX_GRID / chunks) return -7;             // gridDim.y
    long long off = 0, blocks = 0, n_max = 0;
    for (int t = 0; t < T; ++t) {
        const long long *d = desc_host + (long long)t * CG_DESC;
        const long long n = d[1], B = d[2], gid = d[3], zoff = d[4];
        if (n < 1 || d[0] != off || d[5] != blocks || zoff < 0) return -22;     // the time points lie back to back
        if (n > PC_MAX_N || B < 1 || B > B_max || gid < 0 || gid > PC_MAX_G) return -7;
        if (zoff > zrows || ((n + 3) & ~3ll) > zrows - zoff) return -22;
        const double *r = r2_host + (long long)t * CG_MAX_B;
        for (int k = 0; k < CG_MAX_B; ++k) {
            if (k >= B) {
                if (!(r[k] == INFINITY)) return -22;
            } else if (!std::isfinite(r[k]) || r[k] < 0.0 || (k > 0 && !(r[k] > r[k - 1]))) {
                return -7;
            }
        }
        off += n;
        blocks += (n + PC_THREADS - 1) / PC_THREADS;
        if (n > n_max) n_max = n;
    }
    if (L * ng > 0x7fffffffll * 256 / ((long long)T * B_max)) return -7;        // the grid of the second launch
    if (blocks > (1ll << 40) / (L * ng * B_max)) return -7;
    if (scratch_doubles < cg_scratch(blocks, L, ng, B_max)) return -22;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(W, 0, sizeof(long long) * (size_t)T * B_max, st) != hipSuccess) return -5;
    if (hipMemsetAsync(S2c, 0, sizeof(long long) * (size_t)T * B_max, st) != hipSuccess) return -5;
    if (skipped && hipMemsetAsync(skipped, 0, sizeof(long long), st) != hipSuccess) return -5;
    const unsigned bx = (unsigned)((n_max + PC_THREADS - 1) / PC_THREADS);
    hipLaunchKernelGGL(k_corr_boxes, dim3(bx, (unsigned)T), dim3(PC_THREADS), 0, st, reinterpret_cast<const double2 *>(xy), desc_dev,
                       B_max, scratch);
    if (hipGetLastError() != hipSuccess) return -5;
    const size_t dyn = ((size_t)B_max * CS * PC_THREADS + (size_t)CS * PC_THREADS) * sizeof(double) + PC_THREADS * sizeof(double2) +
                       (size_t)B_max * PC_THREADS * sizeof(int);
    const dim3 grid(bx, (unsigned)(L * chunks), (unsigned)T);
    const int rc = CS == 2 ? cg_launch<2>(grid, dyn, st, xy, order, Z, zrows, GP, desc_dev, r2_dev, ng, B_max, observed, first, (int)L,
                                          seed, cull, scratch, blocks, W, S2c, skipped)
                           : cg_launch<4>(grid, dyn, st, xy, order, Z, zrows, GP, desc_dev, r2_dev, ng, B_max, observed, first, (int)L,
                                          seed, cull, scratch, blocks, W, S2c, skipped);
    if (rc) return rc;
    const long long cells = (long long)T * L * ng * B_max;
    hipLaunchKernelGGL(k_corr_reduce, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, desc_dev, (const double *)(scratch + blocks * 4),
                       T, ng, (int)L, B_max, N, Q);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
