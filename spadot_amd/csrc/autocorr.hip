// autocorr.hip -- the two edge sums behind Moran's I and Geary's C of every gene, for many (time point, labeling, gene) problems
// in one launch (gfx950, wave64).  The definition is restated in numpy in tests/autocorr_ref.py.
//
// A time point is a directed edge list i -> j over its n spots; gene g has the fp32 values v of the stored entries of its CSC
// column (0 elsewhere) and a centre c.  Labeling 0 is the identity, labeling 1 + p gives spot i the value v[pi_p(i)] with pi_p
// the permutation of feistel_perm.h.  With x the fp64 promotion of the labeled values,
//     N = sum over edges (x_i - c)(x_j - c),     D = sum over edges (x_i - x_j)^2.
//
// k_autocorr   one workgroup per (time point, labeling, group of GS consecutive genes).  It zeroes a dense fp32 image
//              x[spot][gene in group] in LDS, scatters the stored entries of its genes into it -- an entry of row r goes to spot
//              pi^-1(r), the Feistel network run backwards, so no table of the permutation exists anywhere -- and streams the
//              edges once in coalesced reads of src and dst: an edge costs one contiguous LDS read of GS floats per end, no
//              Feistel work and no atomics.  Thread t adds the edges t, t + THREADS, ... in that order into fp64 registers (one
//              subtraction per centring, one fma per term); the partial sums are added by shuffles inside the wavefront (offsets
//              32, 16, .. 1) and then across the wavefronts through LDS in wavefront order.  The order of the additions of a sum
//              depends on (E, THREADS) alone: not on GS, the batch, the path or the run.
//              A time point whose image does not fit (2048 + 4 GS n > lds_limit) keeps it in a slab of the caller's scratch
//              buffer instead, one slab per workgroup, and performs the same additions in the same order.
#include <hip/hip_runtime.h>

#include "../../include/spadot_model.h"
#include "per_device.h"
#include "csc_image.h"

#define AC_DESC 7                  // int64 columns of a time point's descriptor (include/spadot_model.h)
#define AC_LDS_BYTES 163840        // one workgroup may take the whole LDS of a compute unit
#define AC_LDS_FIXED 2048          // what the reduction and the segment bounds take beside the image (static, at most)
#define AC_THREADS 1024            // the default workgroup and
#define AC_GS 2                    // genes per group (Time)
#define AC_MAX_ITEMS 2147483647LL  // (time point, labeling, group) triples of one call: gridDim.x
#define AC_MAX 2147483647LL

template <int GS> struct alignas(4 * GS) AcVec { float v[GS]; };

struct AcItem {
    const int *es, *ed;
    const long long *colptr;
    const int *ridx;
    const float *vals;
    long long nnz, row0;
    unsigned n, E;
    int gene0, genes;                                    // the group's first gene (absolute) and how many of its GS exist
    bool perm;
};

// the whole pass over an image at `img` (LDS or a global slab: the caller's branch fixes the address space)
template <int THREADS, int GS>
__device__ __forceinline__ void ac_pass(float *__restrict__ img, const AcItem &a, const NhPerm &q, const double *cg,
                                        long long *seg, double *red, double *acc) {
    const unsigned tid = threadIdx.x;
    if (tid < 2 * GS) {                                  // the rows of this time point in the gene's column: two lower bounds
        const int k = tid >> 1;
        seg[tid] = k < a.genes ? csc_lower_bound(a.ridx, a.colptr[a.gene0 + k], a.colptr[a.gene0 + k + 1], a.nnz,
                                                 a.row0 + ((tid & 1) ? (long long)a.n : 0LL)) : 0LL;
    }
    csc_image_zero<THREADS, GS>(img, a.n);
    __syncthreads();
    csc_image_scatter<THREADS, GS>(img, seg, a.ridx, a.vals, a.row0, a.n, a.perm, q);
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 2 * GS; ++v) acc[v] = 0.0;
    // an edge end out of range is refused on the host before the launch; the guard keeps every access inside the image
    for (unsigned e = tid; e < a.E; e += THREADS) {
        const unsigned s = (unsigned)a.es[e], d = (unsigned)a.ed[e];
        if (s < a.n && d < a.n) {
            const AcVec<GS> xs = *reinterpret_cast<const AcVec<GS> *>(img + (unsigned long long)s * GS);
            const AcVec<GS> xd = *reinterpret_cast<const AcVec<GS> *>(img + (unsigned long long)d * GS);
#pragma unroll
            for (int k = 0; k < GS; ++k) {
                const double xi = (double)xs.v[k], xj = (double)xd.v[k];
                const double dd = xi - xj;
                acc[k] = fma(xi - cg[k], xj - cg[k], acc[k]);
                acc[GS + k] = fma(dd, dd, acc[GS + k]);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 2 * GS; ++v) {
        double x = acc[v];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((tid & 63) == 0) red[(tid >> 6) * 2 * GS + v] = x;
    }
    __syncthreads();
}

template <int THREADS, int GS>
__global__ void __launch_bounds__(THREADS) k_autocorr(const int *__restrict__ src, const int *__restrict__ dst,
                                                      const long long *__restrict__ colptr, const int *__restrict__ ridx,
                                                      const float *__restrict__ vals, long long nnz,
                                                      const double *__restrict__ centre, const long long *__restrict__ desc,
                                                      int T, int G, int g0, int ng, int observed, long long first, int L,
                                                      unsigned long long seed, long long lds_limit, float *__restrict__ scratch,
                                                      long long slab, double *__restrict__ outN, double *__restrict__ outD) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ac_lds[];
    __shared__ double red[(THREADS / 64) * 2 * GS];
    __shared__ long long seg[2 * GS];
    static_assert(sizeof(double) * (THREADS / 64) * 2 * GS + sizeof(long long) * 2 * GS <= AC_LDS_FIXED, "fixed LDS");
    const unsigned tid = threadIdx.x;
    const int ngroups = (ng + GS - 1) / GS;
    const long long item = blockIdx.x, tl = item / ngroups;
    const int grp = (int)(item - tl * ngroups), t = (int)(tl / L), l = (int)(tl - (long long)t * L);
    if (t >= T) return;
    const long long *dg = desc + (long long)t * AC_DESC;
    AcItem a;
    a.es = src + dg[0];
    a.ed = dst + dg[0];
    a.colptr = colptr, a.ridx = ridx, a.vals = vals, a.nnz = nnz;
    a.n = (unsigned)dg[1], a.E = (unsigned)dg[2], a.row0 = dg[3];
    a.gene0 = g0 + grp * GS;
    a.genes = ng - grp * GS < GS ? ng - grp * GS : GS;
    a.perm = !(observed && l == 0);
    NhPerm q = {};
    if (a.perm) q = nh_perm_setup(seed, (unsigned long long)dg[4], (unsigned long long)(first + l - (observed ? 1 : 0)), a.n);
    double cg[GS], acc[2 * GS];
#pragma unroll
    for (int k = 0; k < GS; ++k) cg[k] = k < a.genes ? centre[(long long)t * G + a.gene0 + k] : 0.0;
    if (AC_LDS_FIXED + 4LL * GS * (long long)a.n <= lds_limit)
        ac_pass<THREADS, GS>(reinterpret_cast<float *>(ac_lds), a, q, cg, seg, red, acc);
    else
        ac_pass<THREADS, GS>(scratch + item * slab, a, q, cg, seg, red, acc);
    if (tid < 2 * GS) {                                  // across the wavefronts, in wavefront order
        double s = red[tid];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) s += red[w * 2 * GS + tid];
        const int k = tid < GS ? tid : tid - GS;
        if (k < a.genes) (tid < GS ? outN : outD)[((long long)t * ng + grp * GS + k) * L + l] = s;
    }
}

template <int THREADS, int GS>
static int ac_launch(long long items, size_t dyn, hipStream_t stream, const int *src, const int *dst, const long long *colptr,
                     const int *ridx, const float *vals, long long nnz, const double *centre, const long long *desc, int T, int G,
                     int g0, int ng, int observed, long long first, int L, unsigned long long seed, long long lds_limit,
                     float *scratch, long long slab, double *outN, double *outD) {
    static PerDeviceFlag attr_set;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_autocorr<THREADS, GS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                AC_LDS_BYTES - AC_LDS_FIXED) != hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL((k_autocorr<THREADS, GS>), dim3((unsigned)items), dim3(THREADS), dyn, stream, src, dst, colptr, ridx,
                       vals, nnz, centre, desc, T, G, g0, ng, observed, first, L, seed, lds_limit, scratch, slab, outN, outD);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int spadot_autocorr_sums(const int *src, const int *dst, const long long *colptr, const int *ridx, const float *vals,
                                    long long nnz, long long ridx_lo, long long ridx_hi, const double *centre,
                                    const long long *desc_host, const long long *desc_dev, int T, int G, int g0, int ng,
                                    int observed, long long first, long long P, long long seed, long long lds_limit,
                                    float *scratch, long long scratch_floats, int threads, int gs, double *outN, double *outD,
                                    void *stream) {
    if (!desc_host || !desc_dev || !colptr || !centre || !outN || !outD || T <= 0 || G <= 0) return -22;
    if (nnz < 0 || g0 < 0 || ng < 1 || first < 0 || P < 0 || lds_limit < 0 || scratch_floats < 0) return -22;
    if ((observed != 0 && observed != 1) || observed + P < 1) return -22;
    if (nnz > 0 && (!ridx || !vals)) return -22;
    if ((long long)g0 + ng > G || nnz > AC_MAX || first + P > 4294967296LL || observed + P > AC_MAX) return -7;
    if (threads == 0) threads = AC_THREADS;
    if (gs == 0) gs = AC_GS;
    if ((threads != 256 && threads != 512 && threads != 1024) || (gs != 2 && gs != 4)) return -7;
    if (lds_limit > AC_LDS_BYTES) lds_limit = AC_LDS_BYTES;
    const long long L = observed + P, ngroups = ((long long)ng + gs - 1) / gs;
    long long rows = 0, dyn = 0, slab = 0;
    for (int t = 0; t < T; ++t) {
        const long long *d = desc_host + (long long)t * AC_DESC;
        const long long eoff = d[0], n = d[1], E = d[2], row0 = d[3], gid = d[4];
        if (eoff < 0 || n < 1 || E < 0 || row0 < 0 || gid < 0) return -22;
        if (n > AC_MAX || E > AC_MAX || gid > AC_MAX || row0 > AC_MAX) return -7;
        if (E > 0 && (d[5] < 0 || d[6] >= n)) return -7;                     // the smallest and the largest edge end
        if (E > 0 && (!src || !dst)) return -22;
        if (row0 + n > rows) rows = row0 + n;
        const long long image = 4LL * gs * n;
        if (AC_LDS_FIXED + image <= lds_limit) {
            if (image > dyn) dyn = image;
        } else if (((image / 4 + 3) & ~3LL) > slab) {
            slab = (image / 4 + 3) & ~3LL;
        }
    }
    if (nnz > 0 && (ridx_lo < 0 || ridx_hi >= rows)) return -7;              // the smallest and the largest row index
    if (T * L > AC_MAX_ITEMS / ngroups) return -7;
    const long long items = T * L * ngroups;
    if (slab > 0 && (!scratch || slab > scratch_floats / items)) return -22;
    dyn = (dyn + 15) & ~15LL;
#define AC_GO(TH, GSZ)                                                                                                          \
    return ac_launch<TH, GSZ>(items, (size_t)dyn, (hipStream_t)stream, src, dst, colptr, ridx, vals, nnz, centre, desc_dev, T, \
                              G, g0, ng, observed, first, (int)L, (unsigned long long)seed, lds_limit, scratch, slab, outN, outD)
    if (gs == 4) {
        if (threads == 256) AC_GO(256, 4);
        if (threads == 512) AC_GO(512, 4);
        AC_GO(1024, 4);
    }
    if (threads == 256) AC_GO(256, 2);
    if (threads == 512) AC_GO(512, 2);
    AC_GO(1024, 2);
#undef AC_GO
}
