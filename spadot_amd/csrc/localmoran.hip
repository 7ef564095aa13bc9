// localmoran.hip -- the neighbour sums behind local Moran's I (Anselin's LISA) of every (time point, selected gene, spot) and
// their comparison with the sums under conditional permutations, in one launch (gfx950, wave64).  The definition is
// restated in numpy in tests/hotspots_ref.py.
//
// A time point is a CSR over its n spots (rowptr [n + 1] from 0 to E, col [E]: the out-neighbours of a spot in edge-list order);
// gene g has the fp32 values v of the stored entries of its CSC column (0 elsewhere) and a centre c.  The neighbour sum of spot i
// under the shown values x is, in fp64 and in row order,
//     lag_i = ((0 + (x_j1 - c)) + (x_j2 - c)) + ...
// -- subtractions and additions only: there is no product that could be contracted into an fma.  The observed sum shows x = v.
// Permutation p shows x_j = v[pi_p(j)], pi_p the permutation of feistel_perm.h, except that, while spot i is evaluated, the
// neighbour j* = pi_p^-1(i) (which would show spot i's own value) shows v[pi_p(i)] instead: pi_p composed with the transposition
// (i, j*), a uniform draw from the permutations that fix i.  Per (gene, spot): lag (observed), ge = #{p : lag^p >= lag^0} and
// le = #{p : lag^p <= lag^0}.
//
// k_local_lag  one workgroup per (time point, chunk of permutations, group of GS selected genes).  For the identity and then for
//              every permutation of its chunk it zeroes a dense fp32 image x[spot][gene in group] in LDS, scatters the stored
//              entries of its genes into it (an entry of row r goes to spot pi^-1(r)) and, behind a barrier, thread t walks the
//              rows of the spots t, t + THREADS, ...: one contiguous LDS read of GS floats per neighbour, where the neighbour j*
//              reads the image at i itself (x_i = v[pi(i)] is exactly the replacement), so the conditional draw costs one inverse
//              Feistel evaluation per spot and permutation and no second image.  The observed sums and the two counters of the
//              workgroup's spots live in a slab of the caller's scratch buffer that only the owning thread touches (DESIGN 7l:
//              the image takes the LDS); at the end every workgroup adds its counters into the zeroed outputs with integer
//              atomics -- exact in any order -- and the workgroups of chunk 0 write lag.
//              A time point whose image does not fit (256 + 4 GS n > lds_limit) keeps it in the same slab instead and performs
//              the same operations in the same order.
#include <hip/hip_runtime.h>

#include "../../include/spadot_model.h"
#include "per_device.h"
#include "csc_image.h"

#define LM_DESC 8                  // int64 columns of a time point's descriptor (include/spadot_model.h)
#define LM_LDS_BYTES 163840        // one workgroup may take the whole LDS of a compute unit
#define LM_LDS_FIXED 256           // what the segment bounds take beside the image (static, at most)
#define LM_THREADS 1024            // the default workgroup,
#define LM_GS 4                    // genes per group and
#define LM_CHUNK 128               // permutations per workgroup (Time)
#define LM_MAX 2147483647LL

template <int GS> struct alignas(4 * GS) LmVec { float v[GS]; };
template <int GS> struct alignas(8 * GS) LmLag { double v[GS]; };
template <int GS> struct alignas(8 * GS) LmCnt { int ge[GS], le[GS]; };

struct LmItem {
    const int *rowptr, *col, *ridx;
    const float *vals;
    long long row0;
    unsigned n, E;
    int genes;                                           // how many of the group's GS genes exist
};

// every labeling of the workgroup over an image at `img` (LDS or a global slab: the caller's branch fixes the address space)
template <int THREADS, int GS>
__device__ __forceinline__ void lm_pass(float *__restrict__ img, const LmItem &a, const double *cg, const long long *seg,
                                        LmLag<GS> *__restrict__ lag0, LmCnt<GS> *__restrict__ cnt, unsigned long long seed,
                                        unsigned long long gid, unsigned long long p0, int np) {
    const unsigned tid = threadIdx.x;
    for (int l = 0; l <= np; ++l) {                      // labeling 0 is the identity, 1 + u permutation p0 + u
        const bool perm = l > 0;
        NhPerm q = {};
        if (perm) q = nh_perm_setup(seed, gid, p0 + (unsigned long long)(l - 1), a.n);
        __syncthreads();                                 // the bounds are written; the image of the labeling before is read
        csc_image_zero<THREADS, GS>(img, a.n);
        __syncthreads();
        csc_image_scatter<THREADS, GS>(img, seg, a.ridx, a.vals, a.row0, a.n, perm, q);
        __syncthreads();
        for (unsigned i = tid; i < a.n; i += THREADS) {
            long long r0, r1;
            csr_row(a.rowptr, i, a.E, r0, r1);
            const unsigned jstar = perm ? ac_perm_inv(q, i) : i;
            double acc[GS];
#pragma unroll
            for (int k = 0; k < GS; ++k) acc[k] = 0.0;
            for (long long e = r0; e < r1; ++e) {
                // a neighbour out of range is refused on the host; the load stays unconditional from a clamped spot
                const unsigned j = (unsigned)a.col[e];
                const bool ok = j < a.n;
                const unsigned at = !ok ? 0u : (j == jstar ? i : j);
                const LmVec<GS> x = *reinterpret_cast<const LmVec<GS> *>(img + (unsigned long long)at * GS);
#pragma unroll
                for (int k = 0; k < GS; ++k) {
                    const double s = acc[k] + ((double)x.v[k] - cg[k]);
                    acc[k] = ok ? s : acc[k];
                }
            }
            if (!perm) {
                LmLag<GS> z;
                LmCnt<GS> c;
#pragma unroll
                for (int k = 0; k < GS; ++k) z.v[k] = acc[k], c.ge[k] = 0, c.le[k] = 0;
                lag0[i] = z;
                cnt[i] = c;
            } else {
                const LmLag<GS> z = lag0[i];
                LmCnt<GS> c = cnt[i];
#pragma unroll
                for (int k = 0; k < GS; ++k) {
                    c.ge[k] += acc[k] >= z.v[k] ? 1 : 0;
                    c.le[k] += acc[k] <= z.v[k] ? 1 : 0;
                }
                cnt[i] = c;
            }
        }
    }
}

template <int THREADS, int GS>
__global__ void __launch_bounds__(THREADS) k_local_lag(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                       const long long *__restrict__ colptr, const int *__restrict__ ridx,
                                                       const float *__restrict__ vals, long long nnz,
                                                       const double *__restrict__ centre, const long long *__restrict__ desc,
                                                       int T, int G, const int *__restrict__ genes, int ng, long long first,
                                                       long long P, long long chunk, long long chunks, unsigned long long seed,
                                                       long long lds_limit, unsigned char *__restrict__ scratch, long long stride,
                                                       long long state_spots, long long rows, double *__restrict__ lag,
                                                       int *__restrict__ ge, int *__restrict__ le) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lm_lds[];
    __shared__ long long seg[2 * GS];
    static_assert(sizeof(long long) * 2 * GS <= LM_LDS_FIXED && GS <= 4, "fixed LDS");
    const unsigned tid = threadIdx.x;
    const long long ngroups = ((long long)ng + GS - 1) / GS;
    const long long item = blockIdx.x, tc = item / ngroups;
    const int grp = (int)(item - tc * ngroups), t = (int)(tc / chunks);
    const long long ch = tc - (long long)t * chunks;
    if (t >= T) return;
    const long long *dg = desc + (long long)t * LM_DESC;
    LmItem a;
    a.col = col + dg[0];
    a.rowptr = rowptr + dg[5];
    a.ridx = ridx, a.vals = vals;
    a.n = (unsigned)dg[1], a.E = (unsigned)dg[2], a.row0 = dg[3];
    a.genes = ng - grp * GS < GS ? ng - grp * GS : GS;
    double cg[GS];
#pragma unroll
    for (int k = 0; k < GS; ++k) {
        const int g = csc_gene(genes[k < a.genes ? grp * GS + k : grp * GS], G);
        cg[k] = k < a.genes ? centre[(long long)t * G + g] : 0.0;
    }
    if (tid < 2 * GS) {                                  // the rows of this time point in the gene's column: two lower bounds
        const int k = tid >> 1;
        long long lo = 0;
        if (k < a.genes) {
            const int g = csc_gene(genes[grp * GS + k], G);
            lo = csc_lower_bound(ridx, colptr[g], colptr[g + 1], nnz, a.row0 + ((tid & 1) ? (long long)a.n : 0LL));
        }
        seg[tid] = lo;
    }
    const long long p0 = ch * chunk, left = P - p0;
    const int np = (int)(left < chunk ? left : chunk);
    unsigned char *mine = scratch + item * stride;
    LmLag<GS> *lag0 = reinterpret_cast<LmLag<GS> *>(mine);
    LmCnt<GS> *cnt = reinterpret_cast<LmCnt<GS> *>(mine + 8LL * GS * state_spots);
    if (LM_LDS_FIXED + 4LL * GS * (long long)a.n <= lds_limit)
        lm_pass<THREADS, GS>(reinterpret_cast<float *>(lm_lds), a, cg, seg, lag0, cnt, seed, (unsigned long long)dg[4],
                             (unsigned long long)(first + p0), np);
    else
        lm_pass<THREADS, GS>(reinterpret_cast<float *>(mine + 16LL * GS * state_spots), a, cg, seg, lag0, cnt, seed,
                             (unsigned long long)dg[4], (unsigned long long)(first + p0), np);
    for (unsigned i = tid; i < a.n; i += THREADS) {      // the owning thread's own entries: no barrier needed
        const LmLag<GS> z = lag0[i];
        const LmCnt<GS> c = cnt[i];
#pragma unroll
        for (int k = 0; k < GS; ++k) {
            if (k < a.genes) {
                const long long o = ((long long)grp * GS + k) * rows + a.row0 + i;
                if (c.ge[k]) atomicAdd(ge + o, c.ge[k]);
                if (c.le[k]) atomicAdd(le + o, c.le[k]);
                if (ch == 0) lag[o] = z.v[k];
            }
        }
    }
}

template <int THREADS, int GS>
static int lm_launch(long long items, size_t dyn, hipStream_t stream, const int *rowptr, const int *col, const long long *colptr,
                     const int *ridx, const float *vals, long long nnz, const double *centre, const long long *desc, int T, int G,
                     const int *genes, int ng, long long first, long long P, long long chunk, long long chunks,
                     unsigned long long seed, long long lds_limit, unsigned char *scratch, long long stride, long long state_spots,
                     long long rows, double *lag, int *ge, int *le) {
    static PerDeviceFlag attr_set;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_local_lag<THREADS, GS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                LM_LDS_BYTES - LM_LDS_FIXED) != hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL((k_local_lag<THREADS, GS>), dim3((unsigned)items), dim3(THREADS), dyn, stream, rowptr, col, colptr, ridx,
                       vals, nnz, centre, desc, T, G, genes, ng, first, P, chunk, chunks, seed, lds_limit, scratch, stride,
                       state_spots, rows, lag, ge, le);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int spadot_local_lag(const int *rowptr, const int *col, const long long *colptr, const int *ridx, const float *vals,
                                long long nnz, long long ridx_lo, long long ridx_hi, const double *centre,
                                const long long *desc_host, const long long *desc_dev, int T, int G, const int *genes, int ng,
                                int gene_lo, int gene_hi, long long first, long long P, long long seed, long long lds_limit,
                                void *scratch, long long scratch_bytes, int threads, int gs, long long perm_chunk, long long rows,
                                double *lag, int *ge, int *le, void *stream) {
    if (!rowptr || !desc_host || !desc_dev || !colptr || !centre || !genes || !lag || !ge || !le || !scratch) return -22;
    if (T <= 0 || G <= 0 || nnz < 0 || ng < 1 || first < 0 || lds_limit < 0 || scratch_bytes < 0 || rows < 1) return -22;
    if (nnz > 0 && (!ridx || !vals)) return -22;
    if (P < 1 || perm_chunk < 0 || first + P > 4294967296LL || nnz > LM_MAX || gene_lo < 0 || gene_hi >= G) return -7;
    if (threads == 0) threads = LM_THREADS;
    if (gs == 0) gs = LM_GS;
    if (perm_chunk == 0) perm_chunk = LM_CHUNK;
    if ((threads != 256 && threads != 512 && threads != 1024) || (gs != 2 && gs != 4)) return -7;
    if (lds_limit > LM_LDS_BYTES) lds_limit = LM_LDS_BYTES;
    const long long chunks = (P + perm_chunk - 1) / perm_chunk, ngroups = ((long long)ng + gs - 1) / gs;
    long long most = 0, dyn = 0, slab = 0, spots = 0;
    for (int t = 0; t < T; ++t) {
        const long long *d = desc_host + (long long)t * LM_DESC;
        const long long eoff = d[0], n = d[1], E = d[2], row0 = d[3], gid = d[4], roff = d[5];
        if (eoff < 0 || n < 1 || E < 0 || row0 < 0 || gid < 0 || roff < 0) return -22;
        if (n > LM_MAX || E > LM_MAX || gid > LM_MAX || row0 > LM_MAX) return -7;
        if (E > 0 && (d[6] < 0 || d[7] >= n)) return -7;                     // the smallest and the largest neighbour
        if (E > 0 && !col) return -22;
        if (row0 + n > most) most = row0 + n;
        if (n > spots) spots = n;
        const long long image = 4LL * gs * n;
        if (LM_LDS_FIXED + image <= lds_limit) {
            if (image > dyn) dyn = image;
        } else if (((image / 4 + 3) & ~3LL) > slab) {
            slab = (image / 4 + 3) & ~3LL;
        }
    }
    if (most > rows) return -22;
    if (nnz > 0 && (ridx_lo < 0 || ridx_hi >= most)) return -7;              // the smallest and the largest row index
    if (T * chunks > LM_MAX / ngroups) return -7;
    const long long items = T * chunks * ngroups, stride = 16LL * gs * spots + 4LL * slab;
    if (stride > scratch_bytes / items) return -22;
    dyn = (dyn + 15) & ~15LL;
#define LM_GO(TH, GSZ)                                                                                                          \
    return lm_launch<TH, GSZ>(items, (size_t)dyn, (hipStream_t)stream, rowptr, col, colptr, ridx, vals, nnz, centre, desc_dev, \
                              T, G, genes, ng, first, P, perm_chunk, chunks, (unsigned long long)seed, lds_limit,              \
                              (unsigned char *)scratch, stride, spots, rows, lag, ge, le)
    if (gs == 4) {
        if (threads == 256) LM_GO(256, 4);
        if (threads == 512) LM_GO(512, 4);
        LM_GO(1024, 4);
    }
    if (threads == 256) LM_GO(256, 2);
    if (threads == 512) LM_GO(512, 2);
    LM_GO(1024, 2);
#undef LM_GO
}
