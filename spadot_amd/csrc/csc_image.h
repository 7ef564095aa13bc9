// csc_image.h -- what the kernels of the Moran stages share (autocorr.hip, localmoran.hip, crossmoran.hip): the rows of
// a time point inside a CSC column, the dense fp32 image x[spot][gene in group] of a group of GS genes under a labeling, and the
// clamps that keep a selected gene inside the genes and a CSR row inside col whatever the caller's arrays hold.  The host
// refuses what the clamps and guards catch before any launch; they stay so that no access leaves its array.
#ifndef SPADOT_CSC_IMAGE_H
#define SPADOT_CSC_IMAGE_H
#include <hip/hip_runtime.h>

#include "feistel_perm.h"

// the first entry of the column lo .. hi (clamped into 0 .. nnz) whose row index is not below `want`: with want = row0 and
// want = row0 + n, the two lower bounds around the rows of a time point in a sorted column
__device__ __forceinline__ long long csc_lower_bound(const int *ridx, long long lo, long long hi, long long nnz, long long want) {
    lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
    hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if ((long long)ridx[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a selected gene out of range is refused on the host
__device__ __forceinline__ int csc_gene(int g, int G) { return g < 0 ? 0 : (g >= G ? G - 1 : g); }

// the row of spot i in a CSR of E edges: a rowptr that does not ascend from 0 to E is refused on the host before the launch; the
// clamps keep every access inside col
__device__ __forceinline__ void csr_row(const int *rowptr, long long i, long long E, long long &r0, long long &r1) {
    r0 = rowptr[i], r1 = rowptr[i + 1];
    r0 = r0 < 0 ? 0 : (r0 > E ? E : r0);
    r1 = r1 < r0 ? r0 : (r1 > E ? E : r1);
}

// zeroes the image of n spots; the caller's barrier follows
template <int THREADS, int GS>
__device__ __forceinline__ void csc_image_zero(float *__restrict__ img, unsigned n) {
    const unsigned tid = threadIdx.x;
    const unsigned long long total = (unsigned long long)n * GS, quads = total >> 2;
    for (unsigned long long i = tid; i < quads; i += THREADS) reinterpret_cast<float4 *>(img)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned long long i = (quads << 2) + tid; i < total; i += THREADS) img[i] = 0.f;
}

// scatters the stored entries seg[2 k] .. seg[2 k + 1] - 1 of gene k of the group into the zeroed image: under a permutation an
// entry of row r goes to spot pi^-1(r); the caller's barrier follows
template <int THREADS, int GS>
__device__ __forceinline__ void csc_image_scatter(float *__restrict__ img, const long long *seg, const int *ridx, const float *vals,
                                                  long long row0, unsigned n, bool perm, const NhPerm &q) {
    const unsigned tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < GS; ++k) {
        const long long hi = seg[2 * k + 1];
        for (long long idx = seg[2 * k] + tid; idx < hi; idx += THREADS) {
            const long long r = (long long)ridx[idx] - row0;
            if (r >= 0 && r < (long long)n) {            // true between the two bounds of a sorted column; kept as the guard
                const unsigned i = perm ? ac_perm_inv(q, (unsigned)r) : (unsigned)r;
                img[(unsigned long long)i * GS + k] = vals[idx];
            }
        }
    }
}

#endif
