// sepal.hip -- the diffusion time of every (time point, selected gene) on the spatial graph (sepal, Andersson & Lundeberg 2021;
// squidpy's gr.sepal), as a persistent on-chip iteration (gfx950, wave64).  The definition is restated in numpy in
// tests/sepal_ref.py.
//
// A time point is a symmetric CSR over its n spots (rowptr [n + 1] from 0 to M, col [M]: for row i first the targets of i's own
// edges, then the sources of the edges that end in i; M = 2 E entries, deg_i the length of row i) and a rate a = dt n / M, formed
// in fp64 on the host.  Gene g has the image c, fp64 [n]: at first the fp32 values of the stored entries of its CSC column
// widened, 0 elsewhere.  One step, Jacobi (every spot reads the image of the step before), every operation rounded once:
//     s_i = ((0 + c_j1) + c_j2) + ...  over row i in row order      l_i = s_i - deg_i * c_i      c'_i = c_i + a * l_i, 0 where < 0
// -- the whole file is compiled under `fp contract(off)`, so no product is fused into the addition behind it and the image after
// any number of steps has the bits of numpy.  The entropy of an image, over the spots with c_i > 0:
//     S = sum c_i,   Q = sum c_i log c_i,   H = (log S - Q / S) / n
// SUMMATION ORDER of S and of Q, fixed by n and the width W = 1024 of the workgroup alone: thread t adds its spots t, t + W,
// t + 2 W, .. in ascending order from 0.0; the 64 lanes of a wavefront are folded by shuffles, lane l taking lane l + 32, then
// l + 16, 8, 4, 2, 1; lane 0 of wavefront w writes slot w, and one thread adds the slots 0 .. 15 in ascending order.  No atomics.
// After step t the item stops if |H^t - H^(t-1)| <= thresh (only where `stop` is set); `iterations` counts its steps.
//
// k_sepal_steps  one workgroup per item = (time point, selected gene); all items of a call are one launch.  The workgroup owns the
//                image for the whole launch: in LDS where 512 + 8 n <= lds_limit (at most 98816: n <= 12288), otherwise in the
//                item's slab in global memory.
//                LDS path: a thread holds the new values of its (at most SP_SPT) spots in registers until a barrier has seen every
//                read of the old image, then stores them.  Global path: two slabs, read one, write the other, swap behind a
//                barrier.  Both paths perform the same operations in the same order: the bits do not depend on the path.
//                State between launches lives in global memory per item: the image (first half of the slab; written at the end
//                of a launch, read at the start of the next), H_prev, iterations, done (0 running, 1 stopped by the rule, 2
//                degenerate: no positive value, n < 2 or no edge -- no step is run).  With init = 1 the launch builds the image
//                from the CSC column and computes H0 first.  A launch runs at most `steps` further steps of every item that is
//                not done, and never past n_iter.
// BARRIERS       The loop over steps runs `left` times unless `stop` ends it.  Both are words in LDS that thread 0 alone writes
//                and every thread reads behind a __syncthreads() that all threads of the workgroup reach: `left` once ahead of
//                the loop, `stop` behind the last barrier of every step.  So every thread takes the same number of trips and
//                leaves the loop at the same barrier; no barrier stands inside a divergent branch (the loops over a thread's
//                own spots contain none).  Nothing spins on memory and no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/spadot_model.h"
#include "per_device.h"
#include "csc_image.h"

#pragma clang fp contract(off)

#define SP_DESC 8                  // int64 columns of a time point's descriptor (include/spadot_model.h)
#define SP_LDS_FIXED 512           // what the reduction slots, the broadcast words and the segment bounds take (static, at most)
#define SP_THREADS 1024
#define SP_WAVES (SP_THREADS / 64)
#define SP_SPT 12                  // spots per thread on the LDS path: 96 VGPRs, no spill (14: 104; 16 spills SGPRs, 20 both)
#define SP_LDS_BYTES (SP_LDS_FIXED + 8 * SP_SPT * SP_THREADS)      // 98816: the cap is what the registers of a workgroup hold, not
                                                                   // the 160 KiB of the compute unit (12288 spots)
#define SP_MAX 2147483647LL

// the new value of spot i from the image `cur` (rounded once per operation: contraction is off)
__device__ __forceinline__ double sp_update(const double *cur, const int *rowptr, const int *col, unsigned i, long long M, unsigned n,
                                            double a) {
    long long r0, r1;
    csr_row(rowptr, i, M, r0, r1);
    const double ci = cur[i];
    double s = 0.0;
    for (unsigned e = (unsigned)r0, e1 = (unsigned)r1; e < e1; ++e) {        // 0 <= r0 <= r1 <= M <= 2^31 - 1
        // a neighbour out of range is refused on the host; the load stays unconditional from a clamped spot
        const unsigned j = (unsigned)col[e];
        const bool ok = j < n;
        const double x = cur[ok ? j : 0u];
        s = ok ? s + x : s;
    }
    const double dc = (double)(r1 - r0) * ci;
    const double l = s - dc;
    const double al = a * l;
    const double c = ci + al;
    return c < 0.0 ? 0.0 : c;
}

// the thread's part of S and Q over its own spots of `img` in ascending order, folded over the wavefront into the slots
__device__ __forceinline__ void sp_partial(const double *img, unsigned n, double *red) {
    const unsigned tid = threadIdx.x;
    double S = 0.0, Q = 0.0;
    for (unsigned i = tid; i < n; i += SP_THREADS) {
        const double c = img[i];
        if (c > 0.0) {
            const double term = c * log(c);
            S = S + c;
            Q = Q + term;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        S = S + __shfl_down(S, off, 64);
        Q = Q + __shfl_down(Q, off, 64);
    }
    if ((tid & 63u) == 0) red[tid >> 6] = S, red[SP_WAVES + (tid >> 6)] = Q;
}

// one thread, behind the barrier that follows sp_partial: the slots in ascending order; NaN without a positive value
__device__ __forceinline__ double sp_entropy(const double *red, unsigned n, bool &any) {
    double S = red[0], Q = red[SP_WAVES];
    for (int w = 1; w < SP_WAVES; ++w) S = S + red[w], Q = Q + red[SP_WAVES + w];
    any = S > 0.0;
    if (!any) return __builtin_nan("");
    const double q = Q / S;
    return (log(S) - q) / (double)n;
}

__global__ void __launch_bounds__(SP_THREADS) k_sepal_steps(const int *__restrict__ rowptr_all, const int *__restrict__ col_all,
                                                            const long long *__restrict__ colptr, const int *__restrict__ ridx,
                                                            const float *__restrict__ vals, long long nnz,
                                                            const long long *__restrict__ desc, const double *__restrict__ rate,
                                                            int T, int G, const int *__restrict__ genes, int ng, int init, int stop,
                                                            int steps, int n_iter, double thresh, long long lds_limit,
                                                            double *image, long long stride, long long second,
                                                            double *__restrict__ H_prev, double *__restrict__ H0,
                                                            int *__restrict__ iterations, int *__restrict__ done,
                                                            double *__restrict__ trace, long long trace_len) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sp_lds[];
    __shared__ double red[2 * SP_WAVES];
    __shared__ long long seg[2];
    __shared__ int bc_left, bc_stop;
    static_assert(sizeof(double) * 2 * SP_WAVES + sizeof(long long) * 2 + sizeof(int) * 2 <= SP_LDS_FIXED, "fixed LDS");
    const unsigned tid = threadIdx.x;
    const long long item = blockIdx.x;
    const int t = (int)(item / ng), j = (int)(item - (long long)t * ng);
    if (t >= T) return;                                  // the whole workgroup: blockIdx is uniform
    const long long *dg = desc + (long long)t * SP_DESC;
    const int *col = col_all + dg[0], *rowptr = rowptr_all + dg[5];
    const unsigned n = (unsigned)dg[1];
    const long long M = dg[2], row0 = dg[3];
    const double a = rate[t];
    const bool in_lds = SP_LDS_FIXED + 8LL * (long long)n <= lds_limit;
    double *slab = image + item * stride;                // the state's image; on the global path also the first of the two slabs
    double *other = slab + second;                       // the second slab (read only on the global path)
    double *lds = reinterpret_cast<double *>(sp_lds);

    if (init) {                                          // c0 from the CSC column, into the slab
        if (tid < 2) {
            const int g = csc_gene(genes[j], G);
            seg[tid] = csc_lower_bound(ridx, colptr[g], colptr[g + 1], nnz, row0 + (tid ? (long long)n : 0LL));
        }
        for (unsigned i = tid; i < n; i += SP_THREADS) slab[i] = 0.0;
        __syncthreads();
        const long long hi = seg[1];
        for (long long idx = seg[0] + tid; idx < hi; idx += SP_THREADS) {
            const long long r = (long long)ridx[idx] - row0;
            if (r >= 0 && r < (long long)n) slab[r] = (double)vals[idx];      // true between the two bounds; kept as the guard
        }
        __syncthreads();
    }
    if (in_lds) {
        for (unsigned i = tid; i < n; i += SP_THREADS) lds[i] = slab[i];     // a thread reads the spots it will own
    }
    double *cur = in_lds ? lds : slab, *nxt = other;
    double Hp = 0.0;
    int it = 0, flag = 0;
    if (init) {
        sp_partial(cur, n, red);                         // own spots only: no barrier between the copy above and this
        __syncthreads();
    }
    if (tid == 0) {
        if (init) {
            bool any;
            const double h = sp_entropy(red, n, any);
            flag = (!any || n < 2 || M < 1) ? 2 : 0;
            Hp = flag ? __builtin_nan("") : h;
            H0[item] = Hp;
            if (trace && trace_len > 0) trace[item * trace_len] = Hp;
        } else {
            Hp = H_prev[item], it = iterations[item], flag = done[item];
        }
        int left = (flag || it >= n_iter) ? 0 : n_iter - it;
        bc_left = left < steps ? left : steps;
        bc_stop = 0;
    }
    __syncthreads();                                     // the copy into LDS, bc_left and bc_stop are written
    const int left = bc_left;                            // the same word for every thread (header: BARRIERS)

    for (int s = 0; s < left; ++s) {
        if (in_lds) {
            double nv[SP_SPT];
#pragma unroll
            for (int k = 0; k < SP_SPT; ++k) {
                const unsigned i = tid + (unsigned)k * SP_THREADS;
                nv[k] = i < n ? sp_update(lds, rowptr, col, i, M, n, a) : 0.0;
                __builtin_amdgcn_sched_barrier(0);       // one spot after the other: loads hoisted across spots cost registers
            }
            __syncthreads();                             // every read of the old image is done
#pragma unroll
            for (int k = 0; k < SP_SPT; ++k) {
                const unsigned i = tid + (unsigned)k * SP_THREADS;
                if (i < n) lds[i] = nv[k];
            }
            sp_partial(lds, n, red);                     // reads what this thread has just stored
        } else {
            for (unsigned i = tid; i < n; i += SP_THREADS) nxt[i] = sp_update(cur, rowptr, col, i, M, n, a);
            sp_partial(nxt, n, red);
            double *swap = cur;
            cur = nxt, nxt = swap;
        }
        __syncthreads();                                 // the new image and the slots are written
        if (tid == 0) {
            bool any;
            const double h = sp_entropy(red, n, any);
            it += 1;
            if (trace && it < trace_len) trace[item * trace_len + it] = h;
            if (stop && fabs(h - Hp) <= thresh) flag = 1, bc_stop = 1;
            Hp = h;
        }
        __syncthreads();                                 // bc_stop is written; the slots are free again
        if (bc_stop) break;                              // the same word for every thread: all leave here together
    }

    if (in_lds) {
        for (unsigned i = tid; i < n; i += SP_THREADS) slab[i] = lds[i];
    } else if (cur != slab) {                            // an odd number of steps: the image lies in the second slab
        for (unsigned i = tid; i < n; i += SP_THREADS) slab[i] = cur[i];
    }
    if (tid == 0) H_prev[item] = Hp, iterations[item] = it, done[item] = flag;
}

extern "C" int spadot_sepal_steps(const int *rowptr, const int *col, const long long *colptr, const int *ridx, const float *vals,
                                  long long nnz, long long ridx_lo, long long ridx_hi, const long long *desc_host,
                                  const long long *desc_dev, const double *rate_host, const double *rate_dev, int T, int G,
                                  const int *genes, int ng, int gene_lo, int gene_hi, int init, int stop, long long steps,
                                  long long n_iter, double thresh, long long lds_limit, double *image, long long image_doubles,
                                  long long stride, double *H_prev, double *H0, int *iterations, int *done, double *trace,
                                  long long trace_len, void *stream) {
    if (!rowptr || !desc_host || !desc_dev || !rate_host || !rate_dev || !colptr || !genes || !image || !H_prev || !H0 ||
        !iterations || !done)
        return -22;
    if (T <= 0 || G <= 0 || nnz < 0 || ng < 1 || lds_limit < 0 || stride < 1 || image_doubles < 1 || trace_len < 0 ||
        (trace_len > 0 && !trace))
        return -22;
    if (nnz > 0 && (!ridx || !vals)) return -22;
    if (steps < 1 || steps > SP_MAX || n_iter < 1 || n_iter > SP_MAX || !(thresh >= 0.0) || !isfinite(thresh)) return -7;
    if (nnz > SP_MAX || gene_lo < 0 || gene_hi >= G) return -7;
    if (lds_limit > SP_LDS_BYTES) lds_limit = SP_LDS_BYTES;
    long long most = 0, dyn = 0, slab = 0, spots = 0;
    for (int t = 0; t < T; ++t) {
        const long long *d = desc_host + (long long)t * SP_DESC;
        const long long eoff = d[0], n = d[1], M = d[2], row0 = d[3], roff = d[5];
        if (eoff < 0 || n < 1 || M < 0 || row0 < 0 || roff < 0) return -22;
        if (n > SP_MAX || M > SP_MAX || row0 > SP_MAX) return -7;
        if (M > 0 && (d[6] < 0 || d[7] >= n)) return -7;                     // the smallest and the largest neighbour
        if (M > 0 && !col) return -22;
        if (M > 0 && (!(rate_host[t] > 0.0) || !isfinite(rate_host[t]))) return -7;
        if (row0 + n > most) most = row0 + n;
        if (n > spots) spots = n;
        if (SP_LDS_FIXED + 8 * n <= lds_limit) {
            if (8 * n > dyn) dyn = 8 * n;
        } else if (n > slab) {
            slab = n;
        }
    }
    if (nnz > 0 && (ridx_lo < 0 || ridx_hi >= most)) return -7;              // the smallest and the largest row index
    if ((long long)T > SP_MAX / ng) return -7;
    const long long items = (long long)T * ng;
    if (stride < spots + slab || stride > image_doubles / items) return -22;
    dyn = (dyn + 15) & ~15LL;
    static PerDeviceFlag attr_set;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_sepal_steps, hipFuncAttributeMaxDynamicSharedMemorySize,
                                SP_LDS_BYTES - SP_LDS_FIXED) != hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL(k_sepal_steps, dim3((unsigned)items), dim3(SP_THREADS), (size_t)dyn, (hipStream_t)stream, rowptr, col, colptr,
                       ridx, vals, nnz, desc_dev, rate_dev, T, G, genes, ng, init ? 1 : 0, stop ? 1 : 0, (int)steps, (int)n_iter,
                       thresh, lds_limit, image, stride, spots, H_prev, H0, iterations, done, trace, trace_len);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
