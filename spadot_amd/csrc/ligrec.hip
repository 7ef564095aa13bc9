// ligrec.hip -- the per-domain expression sums behind the ligand-receptor permutation test, for many (time point, labeling, gene)
// problems in one launch, and the comparison counts of its cells (gfx950, wave64).  The definition is restated in
// numpy in tests/ligrec_ref.py.
//
// A time point is the rows row0 .. row0 + n - 1 of a CSC matrix and one label byte per row; labeling 0 is the label itself,
// labeling 1 + p gives spot i the label lab[pi_p(i)] with pi_p the permutation of feistel_perm.h.  With v the fp32 values of the
// stored entries promoted to fp64,
//     S[t, l, j, k] = sum over the stored entries r of gene genes[j] in time point t with label k under labeling l, of v_r.
//
// k_lr_sums    one workgroup per (time point, labeling, chunk of GC selected genes).  It writes the permuted label bytes of its
//              time point into LDS, four to a dword, with one nh_perm_at per spot (k_nhood's loop): the n Feistel evaluations
//              are paid once per chunk.  Each wavefront then takes genes of the chunk in turn: two binary searches bound the
//              gene's rows inside the time point; lane u adds the entries u, u + 64, ... of that segment in ascending order into
//              its own K fp64 accumulators, a table [wavefront][k][lane] in LDS (lane u of a wavefront touches only its own
//              column: conflict-free 8-byte accesses, no atomics); per k the 64 lane sums are added by shuffles at offsets 32,
//              16, .. 1 and one value is stored, zeros included.  The bits of a sum depend on (the segment, the labels of its
//              rows) alone: not on GC, the gene's place in its chunk, the batch, the thread count, the path or the run.
//              For labeling 0 a second pass over the segment counts the entries with v > 0 per label the same way.
//              A time point whose labels do not fit beside the accumulators (512 K THREADS / 64 + n rounded up to 16 >
//              lds_limit) evaluates nh_perm_at per stored entry and reads the base labeling through L2: the same additions in
//              the same order.
// k_lr_count   one workgroup per (time point, interaction), one thread per cell (a, b): stat_0 from labeling 0's sums, then a
//              loop over the labelings of the run adding the comparisons stat >= stat_0 into an int32.
#include <hip/hip_runtime.h>

#include "../../include/spadot_model.h"
#include "per_device.h"
#include "feistel_perm.h"

#define LR_DESC 3                  // int64 columns of a time point's descriptor (include/spadot_model.h)
#define LR_MAX_K 32
#define LR_LDS_BYTES 163840        // one workgroup may take the whole LDS of a compute unit
#define LR_THREADS 512             // the default workgroup and
#define LR_GC 128                  // selected genes per chunk (Time)
#define LR_MAX 2147483647LL        // spots, stored entries, graph ids and the workgroups of one call (gridDim.x)

static inline long long lr_acc_bytes(long long threads, long long K) { return threads / 64 * K * 512; }
static inline long long lr_need_bytes(long long threads, long long K, long long n) {
    return lr_acc_bytes(threads, K) + ((n + 15) & ~15LL);
}

enum { LR_LDS = 0, LR_BASE = 1, LR_PERM = 2 };       // where the label of a row comes from

template <int MODE>
__device__ __forceinline__ unsigned lr_label(const unsigned char *lab, const unsigned char *glab, const NhPerm &q, unsigned r) {
    if (MODE == LR_LDS) return lab[r];
    if (MODE == LR_BASE) return glab[r];
    return glab[nh_perm_at(q, r)];
}

// lane u adds the entries lo + u, lo + u + 64, ... in that order into mine[k * 64] (its column of the wavefront's table)
template <int MODE, bool COUNT>
__device__ __forceinline__ void lr_pass(double *mine, const unsigned char *lab, const unsigned char *glab, const NhPerm &q,
                                        const int *__restrict__ ridx, const float *__restrict__ vals, long long lo, long long hi,
                                        long long row0, unsigned n, int K, unsigned lane) {
#pragma unroll 4
    for (long long idx = lo + lane; idx < hi; idx += 64) {
        const long long r = (long long)ridx[idx] - row0;
        const float v = vals[idx];
        if (r >= 0 && r < (long long)n) {                // true between the two bounds of a sorted column; kept as the guard
            const unsigned k = lr_label<MODE>(lab, glab, q, (unsigned)r);
            if (k < (unsigned)K) mine[k * 64] += COUNT ? (v > 0.f ? 1.0 : 0.0) : (double)v;
        }
    }
}

// the 64 lane sums of every k, added by shuffles; lane 0 holds the total.  The column is left zero for the next gene.
__device__ __forceinline__ double lr_reduce(double *mine, int k) {
    double x = mine[k * 64];
    mine[k * 64] = 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}

template <int MODE>
__device__ __forceinline__ void lr_genes(double *mine, const unsigned char *lab, const unsigned char *glab, const NhPerm &q,
                                         const long long *__restrict__ colptr, const int *__restrict__ ridx,
                                         const float *__restrict__ vals, long long nnz, const int *__restrict__ genes, int G,
                                         int j0, int j1, int step, long long row0, unsigned n, int K, unsigned lane,
                                         double *__restrict__ So, int *__restrict__ co) {
    for (int j = j0; j < j1; j += step) {
        const int g = genes[j];
        long long lo = 0, hi = 0;
        if (g >= 0 && g < G) {                           // the rows of this time point in the gene's column: two lower bounds
            lo = colptr[g];
            hi = colptr[g + 1];
            lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
            hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
            long long a = lo, b = hi;
            while (a < b) {
                const long long mid = a + ((b - a) >> 1);
                if ((long long)ridx[mid] < row0) a = mid + 1; else b = mid;
            }
            lo = a, b = hi;
            while (a < b) {
                const long long mid = a + ((b - a) >> 1);
                if ((long long)ridx[mid] < row0 + (long long)n) a = mid + 1; else b = mid;
            }
            hi = a;
        }
        lr_pass<MODE, false>(mine, lab, glab, q, ridx, vals, lo, hi, row0, n, K, lane);
        for (int k = 0; k < K; ++k) {
            const double x = lr_reduce(mine, k);
            if (lane == 0) So[(long long)j * K + k] = x;
        }
        if (co) {                                        // labeling 0 only: the stored entries with v > 0 per label
            lr_pass<MODE, true>(mine, lab, glab, q, ridx, vals, lo, hi, row0, n, K, lane);
            for (int k = 0; k < K; ++k) {
                const double x = lr_reduce(mine, k);
                if (lane == 0) co[(long long)j * K + k] = (int)x;
            }
        }
    }
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_lr_sums(const long long *__restrict__ colptr, const int *__restrict__ ridx,
                                                     const float *__restrict__ vals, long long nnz,
                                                     const unsigned char *__restrict__ labels, const long long *__restrict__ desc,
                                                     int T, int G, int K, const int *__restrict__ genes, int ng, int gc,
                                                     int observed, long long first, int L, unsigned long long seed,
                                                     long long lds_limit, double *__restrict__ S, int *__restrict__ cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lr_lds[];
    constexpr int W = THREADS / 64;
    const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nchunks = (ng + gc - 1) / gc;
    const long long item = blockIdx.x, tl = item / nchunks;
    const int chunk = (int)(item - tl * nchunks), t = (int)(tl / L), l = (int)(tl - (long long)t * L);
    if (t >= T) return;
    const long long *dg = desc + (long long)t * LR_DESC;
    const unsigned n = (unsigned)dg[0];
    const long long row0 = dg[1];
    const bool perm = !(observed && l == 0);
    NhPerm q = {};
    if (perm) q = nh_perm_setup(seed, (unsigned long long)dg[2], (unsigned long long)(first + l - (observed ? 1 : 0)), n);
    const unsigned char *glab = labels + row0;           // the base labeling of this time point
    double *mine = reinterpret_cast<double *>(lr_lds) + (size_t)w * K * 64 + lane;
    unsigned char *lab = lr_lds + (size_t)W * K * 512;
    const bool in_lds = (long long)W * K * 512 + (((long long)n + 15) & ~15LL) <= lds_limit;
    for (int k = 0; k < K; ++k) mine[k * 64] = 0.0;
    if (in_lds) {
        for (unsigned i0 = tid * 4; i0 < n; i0 += THREADS * 4) {
            unsigned word = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned i = i0 + j;
                const unsigned v = i < n ? glab[perm ? nh_perm_at(q, i) : i] : 0u;
                word |= v << (8 * j);
            }
            *reinterpret_cast<unsigned *>(lab + i0) = word;
        }
    }
    __syncthreads();
    const int j0 = chunk * gc, j1 = ng - j0 < gc ? ng : j0 + gc;
    double *So = S + ((long long)t * L + l) * ng * K;
    int *co = (observed && l == 0 && cnt) ? cnt + (long long)t * ng * K : nullptr;
    // a label or a row out of range is refused on the host before the launch; the guards keep every access inside its array
    if (in_lds)
        lr_genes<LR_LDS>(mine, lab, glab, q, colptr, ridx, vals, nnz, genes, G, j0 + (int)w, j1, W, row0, n, K, lane, So, co);
    else if (!perm)
        lr_genes<LR_BASE>(mine, lab, glab, q, colptr, ridx, vals, nnz, genes, G, j0 + (int)w, j1, W, row0, n, K, lane, So, co);
    else
        lr_genes<LR_PERM>(mine, lab, glab, q, colptr, ridx, vals, nnz, genes, G, j0 + (int)w, j1, W, row0, n, K, lane, So, co);
}

template <int THREADS>
static int lr_launch(long long items, size_t dyn, hipStream_t stream, const long long *colptr, const int *ridx, const float *vals,
                     long long nnz, const unsigned char *labels, const long long *desc, int T, int G, int K, const int *genes,
                     int ng, int gc, int observed, long long first, int L, unsigned long long seed, long long lds_limit, double *S,
                     int *cnt) {
    static PerDeviceFlag attr_set;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_lr_sums<THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, LR_LDS_BYTES) !=
            hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL((k_lr_sums<THREADS>), dim3((unsigned)items), dim3(THREADS), dyn, stream, colptr, ridx, vals, nnz, labels,
                       desc, T, G, K, genes, ng, gc, observed, first, L, seed, lds_limit, S, cnt);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int spadot_ligrec_sums(const long long *colptr, const int *ridx, const float *vals, long long nnz, long long ridx_lo,
                                  long long ridx_hi, const unsigned char *labels, int label_hi, const long long *desc_host,
                                  const long long *desc_dev, int T, int G, int K, const int *genes, int ng, int gene_lo,
                                  int gene_hi, int observed, long long first, long long P, long long seed, long long lds_limit,
                                  int threads, int gc, double *S, int *cnt, void *stream) {
    if (!desc_host || !desc_dev || !colptr || !labels || !genes || !S || T <= 0 || G <= 0) return -22;
    if (nnz < 0 || ng < 1 || first < 0 || P < 0 || lds_limit < 0 || K < 1 || gc < 0) return -22;
    if ((observed != 0 && observed != 1) || observed + P < 1 || (observed && !cnt)) return -22;
    if (nnz > 0 && (!ridx || !vals)) return -22;
    if (K > LR_MAX_K || nnz > LR_MAX || P > LR_MAX - observed || first > 4294967296LL - P) return -7;
    if (label_hi < 0 || label_hi >= K || gene_lo < 0 || gene_hi >= G) return -7;
    if (threads == 0) threads = LR_THREADS;
    if (gc == 0) gc = LR_GC;
    if (threads != 256 && threads != 512) return -7;
    if (lds_limit > LR_LDS_BYTES) lds_limit = LR_LDS_BYTES;
    const long long L = observed + P, nchunks = ((long long)ng + gc - 1) / gc;
    long long rows = 0, dyn = lr_acc_bytes(threads, K);
    for (int t = 0; t < T; ++t) {
        const long long *d = desc_host + (long long)t * LR_DESC;
        const long long n = d[0], row0 = d[1], gid = d[2];
        if (n < 1 || row0 < 0 || gid < 0) return -22;
        if (n > LR_MAX || row0 > LR_MAX || gid > LR_MAX) return -7;
        if (row0 + n > rows) rows = row0 + n;
        const long long need = lr_need_bytes(threads, K, n);
        if (need <= lds_limit && need > dyn) dyn = need;
    }
    if (nnz > 0 && (ridx_lo < 0 || ridx_hi >= rows)) return -7;              // the smallest and the largest row index
    if (T * L > LR_MAX / nchunks) return -7;
    const long long items = T * L * nchunks;
    if (threads == 512)
        return lr_launch<512>(items, (size_t)dyn, (hipStream_t)stream, colptr, ridx, vals, nnz, labels, desc_dev, T, G, K, genes,
                              ng, gc, observed, first, (int)L, (unsigned long long)seed, lds_limit, S, cnt);
    return lr_launch<256>(items, (size_t)dyn, (hipStream_t)stream, colptr, ridx, vals, nnz, labels, desc_dev, T, G, K, genes, ng,
                          gc, observed, first, (int)L, (unsigned long long)seed, lds_limit, S, cnt);
}

// the statistic of the definition: two products and one sum, each rounded once, then the exact halving
__device__ __forceinline__ double lr_stat(double sa, double wa, double sb, double wb) {
#pragma clang fp contract(off)
    const double x = sa * wa, y = sb * wb;
    const double s = x + y;
    return 0.5 * s;
}

__global__ void __launch_bounds__(1024) k_lr_count(const double *__restrict__ S0, const double *__restrict__ S,
                                                   const double *__restrict__ wk, const int *__restrict__ pairs,
                                                   const unsigned char *__restrict__ mask, int M, int ns, int K, int L, int skip,
                                                   int *__restrict__ ge) {
    const int cell = threadIdx.x;
    if (cell >= K * K) return;
    const long long tm = blockIdx.x, t = tm / M;
    const int m = (int)(tm - t * M), a = cell / K, b = cell - a * K;
    const long long at = tm * K * K + cell;
    if (!mask[at]) return;
    const int src = pairs[2 * m], tgt = pairs[2 * m + 1];
    if (src < 0 || src >= ns || tgt < 0 || tgt >= ns) return;                // refused on the host; kept as the guard
    const double wa = wk[t * K + a], wb = wk[t * K + b];
    const long long ia = (long long)src * K + a, ib = (long long)tgt * K + b, stride = (long long)ns * K;
    const double s0 = lr_stat(S0[t * stride + ia], wa, S0[t * stride + ib], wb);
    const double *base = S + t * L * stride;
    int count = 0;
    for (int l = skip; l < L; ++l) count += lr_stat(base[l * stride + ia], wa, base[l * stride + ib], wb) >= s0 ? 1 : 0;
    ge[at] += count;
}

extern "C" int spadot_ligrec_count(const double *S0, const double *S, const double *wk, const int *pairs, int pair_lo, int pair_hi,
                                   const unsigned char *mask, int T, int M, int ns, int K, long long L, int skip, int *ge,
                                   void *stream) {
    if (!S0 || !S || !wk || !pairs || !mask || !ge || T <= 0 || M <= 0 || ns <= 0 || K < 1 || L < 1) return -22;
    if (skip < 0 || skip > 1 || skip > L) return -22;
    if (K > LR_MAX_K || L > LR_MAX || (long long)T * M > LR_MAX || pair_lo < 0 || pair_hi >= ns) return -7;
    hipLaunchKernelGGL(k_lr_count, dim3((unsigned)((long long)T * M)), dim3((unsigned)((K * K + 63) & ~63)), 0,
                       (hipStream_t)stream, S0, S, wk, pairs, mask, M, ns, K, (int)L, skip, ge);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
