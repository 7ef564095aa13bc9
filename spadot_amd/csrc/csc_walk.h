// csc_walk.h -- the binary search by which preprocess.hip, sctransform.hip, markers.hip and trends.hip find the rows of a time
// point inside a CSC column: the row indices of a column ascend, so a time point t owns the entries between the lower bounds of
// tp_off[t] and tp_off[t + 1].  The caller's range lies inside the array (the host builds colptr); the Moran stages, whose
// callers hand over their own arrays, use the clamped variant of csc_image.h.
#ifndef SPADOT_CSC_WALK_H
#define SPADOT_CSC_WALK_H
#include <hip/hip_runtime.h>

// first position p in [lo, hi) with idx[p] >= key (hi if none)
__device__ __forceinline__ long long csc_walk_lower_bound(const int *idx, long long lo, long long hi, int key) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

#endif
