// territories.hip -- the connected pieces of every domain of many (graph, labeling) problems in one launch (gfx950, wave64;
// DESIGN 7r).  The definition is restated with scipy in tests/territories_ref.py.
//
// A problem is the directed edge list i -> j over n nodes and a labeling in 0 .. K-1, given or permuted as in nhood.hip.  A
// territory is a connected component of the subgraph that keeps the edges whose two ends carry the same label, direction
// ignored; its id is its smallest node.  Per label value four integers leave: territories, the largest, those of one node,
// the sum of size^2.
//
// k_territories   one 1024-thread workgroup per (problem, labeling).  LDS: 1024 bytes of fixed tables (per label value three
//           int32 and one 64-bit sum; the two stop flags), then per node its parent (int32), the size of the tree it roots
//           (int32) and its label byte: 9 bytes per node, n <= 18 090 in 163 840 bytes.  A larger problem, or any under a lower
//           lds_limit, keeps the same three arrays in its own slab of a global scratch tensor and does the same operations
//           there with L1-bypassing (agent-scope) loads, stores and atomics: it touches no other workgroup's memory.
//           A permuted labeling is gathered through nh_perm_at while the labels are loaded; no permutation is stored.
//
//   The forest.  parent[x] <= x always: it starts as x and is only ever lowered, by atomicMin (hook) or by a store of an
//           ancestor (compress).  So parent has no cycle, every walk x -> parent[x] -> .. strictly descends and ends at a node
//           with parent[r] = r, the root, in at most n steps, and a root is the smallest node of its tree.  Only the two ends of
//           a same-label edge, that is two nodes of one territory, are ever joined, so a tree never leaves its territory.
//   A round.  (1) every same-label edge walks to the roots of its two ends and, if they differ, lowers the parent of the larger
//           to the smaller with an integer atomicMin and raises the flag `changed`; barrier; (2) every node walks to its root
//           and stores it as its parent; thread 0 clears the flag of the next round; barrier; all read `changed`.  A hook may
//           overwrite the link another hook of the same round made (the larger root had just been hung elsewhere); that
//           edge then sees two roots again in the next round.  The loop ends after a round without a hook: every same-label
//           edge then has both ends under one root, so every territory is one tree and its root is its smallest node.
//   Termination.  A node that stops being a root never becomes one again (its parent only falls).  Every root found in step
//           (1) was a root at the start of the round, so the first hook that retires in a round removes a root: at most n - 1
//           rounds hook, n rounds suffice, and the loop is capped at n + 1.  At the cap the item's status becomes 1 and the
//           workgroup leaves; the host raises.  Nothing spins on memory and nothing waits for another workgroup.
//   Barriers.  Every __syncthreads() is reached by all 1024 threads: the branch between the LDS and the scratch path, the trip
//           count of the round loop and its stop test depend only on the descriptor, the kernel arguments and the LDS flags
//           that are read behind a barrier, the same for every thread.  No barrier stands inside a loop over edges or nodes.
//   Order.  Integer min, add and max commute and associate, so the values that parent, the sizes and the per-label tables hold
//           at the fixed point do not depend on the order in which the atomics retire; only the NUMBER of rounds may.  The
//           fixed point itself is a function of the problem alone (every node under the smallest node of its territory), so
//           the outputs are the same alone, in any batch, on either path, run after run.  No floating point, and no atomics
//           across workgroups.
//   Parents that other lanes may be lowering are read through relaxed atomic loads, so no stale value is reused in a walk.
#include <hip/hip_runtime.h>

#include "../../include/spadot_model.h"
#include "per_device.h"
#include "feistel_perm.h"

#define TR_THREADS 1024
#define TR_MAX_K 32
#define TR_DESC 14                 // int64 columns of a problem's descriptor (include/spadot_model.h)
#define TR_LDS_BYTES 163840        // one workgroup may take the whole LDS of a compute unit
#define TR_FIXED 1024              // the per-label tables and the flags, ahead of the per-node arrays
#define TR_MAX_ITEMS 2147483647LL  // (problem, labeling) pairs of one call: gridDim.x

static inline long long tr_lds_bytes(long long n) { return TR_FIXED + 8 * n + ((n + 15) & ~15LL); }
static inline long long tr_slab_ints(long long n) { return 2 * n + (n + 3) / 4; }

// the relaxed loads and stores and the hooks of the two paths: workgroup scope on LDS, agent scope (past L1) on the slab
template <bool LDS> __device__ __forceinline__ int tr_ld(const int *p) {
    return LDS ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
               : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ void tr_st(int *p, int v) {
    if (LDS) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ void tr_min(int *p, int v) {
    if (LDS) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ void tr_add(int *p, int v) {
    if (LDS) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root of x: at most n steps, since every step strictly descends (the bound only guards against a corrupted slab)
template <bool LDS> __device__ __forceinline__ unsigned tr_root(const int *parent, unsigned x, unsigned n) {
    for (unsigned step = 0; step < n; ++step) {
        const unsigned p = (unsigned)tr_ld<LDS>(parent + x);
        if (p >= x) break;
        x = p;
    }
    return x;
}

struct TrTables {                  // the fixed LDS tables: 3 * 128 + 256 + 16 = 656 of TR_FIXED bytes
    int count[TR_MAX_K], largest[TR_MAX_K], single[TR_MAX_K];
    unsigned long long sumsq[TR_MAX_K];
    int changed[2], rounds, status;
};

template <bool LDS>
__device__ __forceinline__ void tr_solve(TrTables *tb, int *parent, int *size, unsigned char *lab, const int *es, const int *ed,
                                         const unsigned char *glab, bool perm, const NhPerm &q, unsigned n, unsigned E, int K,
                                         int *oi, int *os) {
    const unsigned tid = threadIdx.x;
    for (unsigned i0 = tid * 4; i0 < n; i0 += TR_THREADS * 4) {              // the labels, four to a dword, and the forest
        unsigned w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned i = i0 + j;
            const unsigned v = i < n ? glab[perm ? nh_perm_at(q, i) : i] : 0u;
            w |= v << (8 * j);
            if (i < n) {
                tr_st<LDS>(parent + i, (int)i);
                tr_st<LDS>(size + i, 0);
            }
        }
        tr_st<LDS>(reinterpret_cast<int *>(lab + i0), (int)w);
    }
    if (tid < TR_MAX_K) {
        tb->count[tid] = 0;
        tb->largest[tid] = 0;
        tb->single[tid] = 0;
        tb->sumsq[tid] = 0ull;
    }
    if (tid == 0) {
        tb->changed[0] = 0;
        tb->changed[1] = 0;
        tb->rounds = 0;
        tb->status = 0;
    }
    __syncthreads();

    const unsigned cap = n + 1u;                                            // n < 2^31
    unsigned round = 0;
    bool open = true;                                                       // the same for every thread (see Barriers above)
    while (open && round < cap) {
        int *flag = &tb->changed[round & 1];
        // an edge end or a label out of range is refused on the host before the launch; the guards keep every access inside
        for (unsigned e = tid; e < E; e += TR_THREADS) {
            const unsigned s = (unsigned)es[e], d = (unsigned)ed[e];
            if (s < n && d < n && s != d) {
                const unsigned w = (unsigned)tr_ld<LDS>(reinterpret_cast<const int *>(lab + (s & ~3u))) >> (8 * (s & 3u));
                const unsigned v = (unsigned)tr_ld<LDS>(reinterpret_cast<const int *>(lab + (d & ~3u))) >> (8 * (d & 3u));
                if ((w & 255u) == (v & 255u)) {
                    const unsigned rs = tr_root<LDS>(parent, s, n), rd = tr_root<LDS>(parent, d, n);
                    if (rs != rd) {
                        tr_min<LDS>(parent + (rs > rd ? rs : rd), (int)(rs > rd ? rd : rs));
                        *flag = 1;
                    }
                }
            }
        }
        __syncthreads();
        for (unsigned i = tid; i < n; i += TR_THREADS) {
            const unsigned r = tr_root<LDS>(parent, i, n);
            if (r != i) tr_st<LDS>(parent + i, (int)r);                      // an ancestor of i, and no root falls in this step
        }
        if (tid == 0) tb->changed[(round + 1) & 1] = 0;                      // last read behind the barrier that ended round - 1
        __syncthreads();
        open = __builtin_amdgcn_readfirstlane(*flag) != 0;
        ++round;
    }
    if (tid == 0) {
        tb->rounds = (int)round;
        tb->status = open ? 1 : 0;                                           // the cap was reached with a hook in the last round
    }
    for (unsigned i = tid; i < n; i += TR_THREADS) {
        const unsigned r = (unsigned)tr_ld<LDS>(parent + i);
        if (r < n) tr_add<LDS>(size + r, 1);                                 // r <= i always; the guard keeps the add inside
    }
    __syncthreads();
    for (unsigned i = tid; i < n; i += TR_THREADS) {
        if ((unsigned)tr_ld<LDS>(parent + i) == i) {
            const unsigned a = ((unsigned)tr_ld<LDS>(reinterpret_cast<const int *>(lab + (i & ~3u))) >> (8 * (i & 3u))) & 255u;
            const int sz = tr_ld<LDS>(size + i);
            if (a < (unsigned)K) {
                atomicAdd(&tb->count[a], 1);
                atomicMax(&tb->largest[a], sz);
                if (sz == 1) atomicAdd(&tb->single[a], 1);
                atomicAdd(&tb->sumsq[a], (unsigned long long)sz * (unsigned long long)sz);
            }
        }
    }
    if (oi) {                                                                // the ids and sizes of the problem's first labeling
        for (unsigned i = tid; i < n; i += TR_THREADS) {
            const unsigned r = (unsigned)tr_ld<LDS>(parent + i);
            oi[i] = (int)r;
            os[i] = r < n ? tr_ld<LDS>(size + r) : 0;
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(TR_THREADS) k_territories(const int *__restrict__ src, const int *__restrict__ dst,
                                                            const unsigned char *__restrict__ labels,
                                                            const long long *__restrict__ desc, int G, int K_max,
                                                            long long lds_limit, long long *__restrict__ out,
                                                            int *__restrict__ ids, int *__restrict__ sizes,
                                                            int *__restrict__ status, int *scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_lds[];
    const unsigned tid = threadIdx.x;
    const long long item = blockIdx.x;
    int lo = 0, hi = G - 1;                              // the problem of this item: item0 ascends, every problem has L >= 1
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(long long)mid * TR_DESC + 8] <= item) lo = mid; else hi = mid - 1;
    }
    const long long *dg = desc + (long long)lo * TR_DESC;
    const unsigned n = (unsigned)dg[1], E = (unsigned)dg[2];
    const int K = (int)dg[3];
    const long long p0 = dg[6];
    const unsigned long long l = (unsigned long long)(item - dg[8]);
    const bool perm = p0 >= 0;
    const int *es = src + dg[0], *ed = dst + dg[0];
    const unsigned char *glab = labels + dg[4] + (perm ? 0ull : l * n);       // PERM: the base labeling
    const bool in_lds = TR_FIXED + 8 * (long long)n + (((long long)n + 15) & ~15LL) <= lds_limit;
    NhPerm q;
    if (perm) q = nh_perm_setup((unsigned long long)dg[9], (unsigned long long)dg[7], (unsigned long long)p0 + l, n);
    else q = NhPerm{{0u, 0u, 0u, 0u, 0u, 0u}, 1u, 1u, n};

    TrTables *tb = reinterpret_cast<TrTables *>(tr_lds);
    const bool want = l == 0 && dg[12] >= 0;
    int *oi = want ? ids + dg[12] : nullptr, *os = want ? sizes + dg[12] : nullptr;
    int *parent, *size;
    if (in_lds) {                                        // the same branch for the whole workgroup
        parent = reinterpret_cast<int *>(tr_lds + TR_FIXED);
        size = parent + n;
        tr_solve<true>(tb, parent, size, reinterpret_cast<unsigned char *>(size + n), es, ed, glab, perm, q, n, E, K, oi, os);
    } else {
        parent = scratch + dg[13] + (long long)l * (2 * (long long)n + ((long long)n + 3) / 4);
        size = parent + n;
        tr_solve<false>(tb, parent, size, reinterpret_cast<unsigned char *>(size + n), es, ed, glab, perm, q, n, E, K, oi, os);
    }

    long long *o = out + item * (long long)(K_max * 4);
    for (int idx = tid; idx < K_max * 4; idx += TR_THREADS) {
        const int a = idx >> 2, c = idx & 3;
        long long v = 0;
        if (a < K) v = c == 0 ? tb->count[a] : c == 1 ? tb->largest[a] : c == 2 ? tb->single[a] : (long long)tb->sumsq[a];
        o[idx] = v;
    }
    if (tid == 0) {
        status[item * 2] = tb->status;
        status[item * 2 + 1] = tb->rounds;
    }
}

extern "C" int spadot_territory_counts(const int *src, const int *dst, const unsigned char *labels, const long long *desc_host,
                                       const long long *desc_dev, int G, int K_max, long long lds_limit, long long *out, int *ids,
                                       int *sizes, long long n_ids, int *status, int *scratch, long long n_scratch,
                                       void *stream) {
    if (!desc_host || !desc_dev || !out || !status || G <= 0 || n_ids < 0 || n_scratch < 0) return -22;
    if (K_max < 1 || K_max > TR_MAX_K) return -7;
    if (lds_limit < 0) return -22;
    if (lds_limit > TR_LDS_BYTES) lds_limit = TR_LDS_BYTES;
    long long items = 0, dyn = TR_FIXED, slabs = 0;
    for (int g = 0; g < G; ++g) {
        const long long *d = desc_host + (long long)g * TR_DESC;
        const long long eoff = d[0], n = d[1], E = d[2], K = d[3], loff = d[4], L = d[5], p0 = d[6], gid = d[7];
        if (eoff < 0 || loff < 0 || n < 1 || E < 0 || L < 1 || p0 < -1 || gid < 0 || d[8] != items || d[12] < -1) return -22;
        if (n > 2147483647LL || E > 2147483647LL || K < 1 || K > K_max) return -7;
        if (p0 >= 0 && (p0 + L > 4294967296LL || gid > 2147483647LL)) return -7;
        if (E > 0 && (d[10] < 0 || d[11] >= n)) return -7;                   // the smallest and the largest edge end
        if (E > 0 && (!src || !dst)) return -22;
        if (!labels) return -22;
        if (d[12] >= 0 && (!ids || !sizes || d[12] + n > n_ids)) return -22;
        items += L;
        if (items > TR_MAX_ITEMS) return -7;
        const long long need = tr_lds_bytes(n);
        if (need <= lds_limit) {
            if (need > dyn) dyn = need;
        } else {
            if (!scratch || d[13] != slabs || L > (n_scratch - slabs) / tr_slab_ints(n)) return -22;
            slabs += L * tr_slab_ints(n);
        }
    }
    static PerDeviceFlag attr_set;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_territories, hipFuncAttributeMaxDynamicSharedMemorySize, TR_LDS_BYTES) !=
            hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL(k_territories, dim3((unsigned)items), dim3(TR_THREADS), (size_t)dyn, (hipStream_t)stream, src, dst, labels,
                       desc_dev, G, K_max, lds_limit, out, ids, sizes, status, scratch);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
