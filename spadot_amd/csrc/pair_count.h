// pair_count.h -- what the stages that count pairs of spots by distance share (cooccur.hip, ripley.hip): the family's
// limits, the squared distance of the definition, the bodies of a pass over a tile (one distance with the self position excluded;
// four points of the tile against BP register counters; one point against them), the flush of the counters through an LDS table
// of 64-bit integers onto the int64 output, and on the host the walks over a problem's padded thresholds and cluster offsets and
// the dispatch over BP.  The two short loops over a tile (four-wide and tail) stay written in each kernel: in one shared function
// they cost up to 61 VGPRs and a wave of occupancy at BP = 64.
#ifndef SPADOT_PAIR_COUNT_H
#define SPADOT_PAIR_COUNT_H
#include <hip/hip_runtime.h>
#include <cmath>
#include <type_traits>

#define PC_THREADS 256             // a workgroup, and the points of a tile
#define PC_MAX_K 32
#define PC_MAX_B 64
#define PC_GRANULE 16              // thresholds per problem are padded to a multiple of this
#define PC_MAX_N 2147483391        // spots per problem: int32 positions, and j0 + 256 must not overflow (2^31 - 1 - 256)
#define PC_MAX_GRID 65535          // problems per launch and patterns per launch or problem: gridDim.y and gridDim.z
#define PC_MAX_G 2147483647ll      // problem numbers, as the graph ids of spadot_nhood_counts
#define PC_PAD (-1.0)              // no d2 is <= -1: a padded threshold never counts

// the squared distance of the definition: two multiplications and three additions, each rounded once.  The only place where a
// distance is formed.
__device__ __forceinline__ double pc_d2(double xi, double yi, double xj, double yj) {
#pragma clang fp contract(off)
    const double dx = xi - xj, dy = yi - yj;
    const double sx = dx * dx, sy = dy * dy;
    return sx + sy;
}

// the distance from `me` to the tile's point at position pos; a point is never its own neighbour (self: -1 where there is none)
__device__ __forceinline__ double pc_dist(double2 me, double2 v, int pos, int self) {
    const double s = pc_d2(me.x, me.y, v.x, v.y);
    return pos == self ? INFINITY : s;
}

// four points of the tile from position pos on in one pass over the thresholds; returns the smallest of the four distances
template <int BP>
__device__ __forceinline__ double pc_pass4(int (&cnt)[BP], const double *th, double2 me, const double2 *four, int pos, int self) {
    double e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = pc_dist(me, four[u], pos + u, self);
    const double near = fmin(fmin(e[0], e[1]), fmin(e[2], e[3]));
#pragma unroll
    for (int t = 0; t < BP; ++t) {
        const double r = th[t];
        cnt[t] += (int)(e[0] <= r) + (int)(e[1] <= r) + (int)(e[2] <= r) + (int)(e[3] <= r);
    }
    return near;
}

template <int BP>
__device__ __forceinline__ void pc_count1(int (&cnt)[BP], const double *th, double e) {
#pragma unroll
    for (int t = 0; t < BP; ++t) cnt[t] += (int)(e <= th[t]);
}

// a thread's counters into row `row` of the LDS table (row < 0: none), then zeroed for the next round; the caller's barrier
// follows.  Two loops: with the zeroing inside the first, this compiler allots k_cooccur<32> 135 VGPRs instead of 117
template <int BP>
__device__ __forceinline__ void pc_flush_counters(int (&cnt)[BP], unsigned long long *tab, int row) {
#pragma unroll
    for (int t = 0; t < BP; ++t)
        if (row >= 0 && cnt[t] != 0) atomicAdd(&tab[row * BP + t], (unsigned long long)cnt[t]);
#pragma unroll
    for (int t = 0; t < BP; ++t) cnt[t] = 0;
}

// the rows x BP table onto the output: entry (row, t < B) is added to dst[row * stride + t] and zeroed (the table is read again
// only after the next tile's two barriers).  Only integers are added: the result does not depend on the order the atomics retire in.
template <int BP>
__device__ __forceinline__ void pc_flush_table(unsigned long long *tab, int rows, int B, unsigned long long *dst, long long stride) {
    for (int i = threadIdx.x; i < rows * BP; i += PC_THREADS) {
        const unsigned long long v = tab[i];
        if (v != 0ull) {
            const int row = i / BP, t = i - row * BP;
            tab[i] = 0ull;
            if (t < B) atomicAdd(dst + (row * stride + t), v);
        }
    }
}

// the threshold columns of a call whose largest problem has B_max thresholds
static inline int pc_padded(int B_max) { return (B_max + PC_GRANULE - 1) / PC_GRANULE * PC_GRANULE; }

// a problem's BP padded thresholds, B of them its own: -22 for bad padding, -7 for one that is not finite, is negative or does
// not increase
static inline int pc_thresholds(const double *r, long long B, int BP) {
    for (int t = 0; t < BP; ++t) {
        if (t >= B) {
            if (r[t] != PC_PAD) return -22;
        } else if (!std::isfinite(r[t]) || r[t] < 0.0 || (t > 0 && !(r[t] > r[t - 1]))) {
            return -7;
        }
    }
    return 0;
}

// a problem's K + 1 cluster offsets: -22 unless they ascend from 0 to n
static inline int pc_offsets(const long long *off, long long K, long long n) {
    if (off[0] != 0 || off[K] != n) return -22;
    for (long long k = 0; k < K; ++k)
        if (off[k + 1] < off[k]) return -22;
    return 0;
}

// f(std::integral_constant<int, BP>) for the padded threshold count of a call
template <class F>
static inline int pc_dispatch(int BP, F f) {
    switch (BP) {
        case 16: return f(std::integral_constant<int, 16>());
        case 32: return f(std::integral_constant<int, 32>());
        case 48: return f(std::integral_constant<int, 48>());
        default: return f(std::integral_constant<int, 64>());
    }
}

#endif
