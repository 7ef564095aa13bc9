// hops.hip -- hop distances from up to 32 source sets at once, for many (graph, labeling) problems in one launch (gfx950,
// wave64).  The definition is restated with scipy in tests/hops_ref.py.
//
// A problem is the directed edge list i -> j over n nodes, as territories.hip takes it (direction ignored; duplicates, two-way
// edges and self loops change nothing), and a labeling in 0 .. K-1, given or permuted as in nhood.hip.  An item is one
// breadth-first search from up to 32 source sets at once, one bit of a 32-bit mask per set:
//   label items   (kind 0; L per problem) set a = the nodes that carry label a under the item's labeling; the class of a
//                 node is that label;
//   source items  (kind 1; ceil(n / 32) per problem) item l has the sets {32 l + j}, j = 0 .. 31, those past n empty; the
//                 class of a node is its label under the problem's one explicit labeling.
// Per (set b, class c) three integers leave: reached (the nodes of class c at a distance 1 .. n-1 of set b), sumdist (the sum
// of those distances) and adjacent (those at distance 1); per set its eccentricity (the largest distance); on request the
// distance of every node to every set of the problem's first labeling.
//
// k_hops    one 1024-thread workgroup per item.  LDS: 16 640 bytes of fixed tables (per (set, class) a 64-bit sum and two
//           int32; per set the eccentricity; the two round flags), then per node its mask of the sets that have reached it
//           (cur), the mask it will have after the round (next) and its class byte: 9 bytes per node, n <= 16 354 in 163 840
//           bytes.  A larger problem, or any under a lower lds_limit, keeps the same three arrays in its own slab of a global
//           scratch tensor and does the same operations there with L1-bypassing (agent-scope) loads, stores and atomics: it
//           touches no other workgroup's memory.  A permuted labeling is gathered through nh_perm_at while the classes are
//           loaded; no permutation is stored.
//
//   A round r = 1, 2, ..  (1) every edge reads the cur masks of its two ends and ORs what the other end lacks into the other
//           end's next mask (an integer atomic OR); barrier; (2) every node takes fresh = next & ~cur, adds for every bit b of
//           fresh and its class c to reached[b][c] (1), sumdist[b][c] (r) and, in round 1, adjacent[b][c] (1), stores
//           hops[node][b] = r where asked, and sets cur = next; the thread ORs its fresh bits into the flag word of the round;
//           barrier; all read the flag word, the threads b < 32 whose bit is set raise ecc[b] to r.  The loop ends after a
//           round whose flag word is 0.
//   Synchronous rounds: TWO MASK ARRAYS.  Step (1) reads only cur and writes only next; step (2) is the only writer of cur
//           and reads no other node's mask; a barrier stands between them and after (2).  So the cur that every edge of round r
//           reads is what round r-1 left, whatever the order of the edges and of the threads: a bit that enters next[v] in
//           round r is invisible to every edge until the barrier, and cannot travel a second hop in that round.  By induction
//           bit b enters cur[v] in step (2) of round r exactly if the distance of v to set b is r.  An update in place (one
//           array) would let a bit ride along a chain of edges that happen to be processed in order and report distances
//           that are too small, without any crash: the shuffled path of the tests is the case.
//   Termination.  A distance is at most n - 1, so round n at the latest has no fresh bit, and the loop is capped at n + 1.
//           At the cap the item's status becomes 1 and the workgroup leaves; the host raises.  Nothing spins on memory and
//           nothing waits for another workgroup.
//   Barriers.  Every __syncthreads() is reached by all 1024 threads: the branch between the LDS and the scratch path, the trip
//           count of the round loop and its stop test depend only on the descriptor, the kernel arguments and the LDS flag
//           words that are read behind a barrier, the same for every thread.  No barrier stands inside a loop over edges or
//           nodes.
//   Order.  Integers only.  OR, add and max commute and associate, so no output depends on the order in which the atomics
//           retire: every output, the number of rounds included, is a function of the problem alone, the same alone, in any
//           batch, on either path, run after run.  No floating point, and no atomics across workgroups.  An edge whose two
//           ends hold the same mask is skipped (that covers the ends that every non-empty set has reached); it changes no
//           integer.
#include <hip/hip_runtime.h>

#include "../../include/spadot_model.h"
#include "per_device.h"
#include "feistel_perm.h"

#define HP_THREADS 1024
#define HP_MAX_K 32
#define HP_DESC 15                 // int64 columns of a problem's descriptor (include/spadot_model.h)
#define HP_LDS_BYTES 163840        // one workgroup may take the whole LDS of a compute unit
#define HP_FIXED 16640             // the per-(set, class) tables, the eccentricities and the flags, ahead of the per-node arrays
#define HP_MAX_ITEMS 2147483647LL  // items of one call: gridDim.x

static inline long long hp_lds_bytes(long long n) { return HP_FIXED + 8 * n + ((n + 15) & ~15LL); }
static inline long long hp_slab_ints(long long n) { return 2 * n + (n + 3) / 4; }

// the relaxed loads, stores and ORs of the two paths: workgroup scope on LDS, agent scope (past L1) on the slab
template <bool LDS> __device__ __forceinline__ unsigned hp_ld(const unsigned *p) {
    return LDS ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
               : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ void hp_st(unsigned *p, unsigned v) {
    if (LDS) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ void hp_or(unsigned *p, unsigned v) {
    if (LDS) __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct HpTables {                  // the fixed LDS tables: 8192 + 4096 + 4096 + 128 + 16 = 16 528 of HP_FIXED bytes
    unsigned long long sumdist[HP_MAX_K * HP_MAX_K];
    int reached[HP_MAX_K * HP_MAX_K], adjacent[HP_MAX_K * HP_MAX_K];
    int ecc[HP_MAX_K];
    unsigned fresh[2];
    int rounds, status;
};

template <bool LDS>
__device__ __forceinline__ void hp_solve(HpTables *tb, unsigned *cur, unsigned *next, unsigned *cls, const int *es, const int *ed,
                                         const unsigned char *glab, bool perm, const NhPerm &q, bool sources, unsigned block,
                                         unsigned n, unsigned E, int K, int *hops) {
    const unsigned tid = threadIdx.x;
    for (unsigned i0 = tid * 4; i0 < n; i0 += HP_THREADS * 4) {              // the classes, four to a dword, and the masks
        unsigned w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned i = i0 + j;
            if (i < n) {
                const unsigned v = glab[perm ? nh_perm_at(q, i) : i] & 31u;  // labels are below K <= 32 (refused on the host)
                w |= v << (8 * j);
                const unsigned m = sources ? ((i >> 5) == block ? 1u << (i & 31u) : 0u) : 1u << v;
                hp_st<LDS>(cur + i, m);
                hp_st<LDS>(next + i, m);
            }
        }
        hp_st<LDS>(cls + (i0 >> 2), w);
    }
    for (unsigned c = tid; c < HP_MAX_K * HP_MAX_K; c += HP_THREADS) {
        tb->sumdist[c] = 0ull;
        tb->reached[c] = 0;
        tb->adjacent[c] = 0;
    }
    if (tid < HP_MAX_K) tb->ecc[tid] = 0;
    if (tid == 0) {
        tb->fresh[0] = 0u;
        tb->fresh[1] = 0u;
        tb->rounds = 0;
        tb->status = 0;
    }
    if (hops) {                                                              // 0 for the members of a set, -1 for the others
        for (unsigned i = tid; i < n; i += HP_THREADS) {                     // node i is written by this thread alone, here and below
            const unsigned v = glab[perm ? nh_perm_at(q, i) : i] & 31u;
            for (int b = 0; b < K; ++b) hops[(long long)i * K + b] = (unsigned)b == v ? 0 : -1;
        }
    }
    __syncthreads();

    const unsigned cap = n + 1u;                                            // n < 2^31
    unsigned round = 0;
    bool open = true;                                                       // the same for every thread (see Barriers above)
    while (open && round < cap) {
        ++round;
        unsigned *flag = &tb->fresh[round & 1];
        // an edge end out of range is refused on the host before the launch; the guard keeps every access inside
        for (unsigned e = tid; e < E; e += HP_THREADS) {
            const unsigned s = (unsigned)es[e], d = (unsigned)ed[e];
            if (s < n && d < n) {
                const unsigned ms = hp_ld<LDS>(cur + s), md = hp_ld<LDS>(cur + d);   // what round - 1 left: cur is not written here
                if (ms != md) {
                    if (ms & ~md) hp_or<LDS>(next + d, ms);
                    if (md & ~ms) hp_or<LDS>(next + s, md);
                }
            }
        }
        __syncthreads();
        unsigned seen = 0;
        for (unsigned i = tid; i < n; i += HP_THREADS) {
            const unsigned nx = hp_ld<LDS>(next + i), old = hp_ld<LDS>(cur + i);
            unsigned f = nx & ~old;
            if (f) {
                const unsigned c = (hp_ld<LDS>(cls + (i >> 2)) >> (8 * (i & 3u))) & 31u;
                hp_st<LDS>(cur + i, nx);
                seen |= f;
                while (f) {
                    const unsigned b = (unsigned)__builtin_ctz(f);
                    f &= f - 1u;
                    const unsigned cell = b * HP_MAX_K + c;
                    atomicAdd(&tb->reached[cell], 1);
                    atomicAdd(&tb->sumdist[cell], (unsigned long long)round);
                    if (round == 1u) atomicAdd(&tb->adjacent[cell], 1);
                    if (hops && b < (unsigned)K) hops[(long long)i * K + b] = (int)round;
                }
            }
        }
        if (seen) atomicOr(flag, seen);
        if (tid == 0) tb->fresh[(round + 1) & 1] = 0u;                       // last read behind the barrier that ended round - 1
        __syncthreads();
        const unsigned got = *flag;
        if (tid < HP_MAX_K && ((got >> tid) & 1u)) tb->ecc[tid] = (int)round;   // rounds ascend: a store raises it
        open = __builtin_amdgcn_readfirstlane(got) != 0u;
    }
    if (tid == 0) {
        tb->rounds = (int)round;
        tb->status = open ? 1 : 0;                                           // the cap was reached with a fresh bit in the last round
    }
    __syncthreads();
}

__global__ void __launch_bounds__(HP_THREADS) k_hops(const int *__restrict__ src, const int *__restrict__ dst,
                                                     const unsigned char *__restrict__ labels,
                                                     const long long *__restrict__ desc, int G, int K_max, long long lds_limit,
                                                     long long *__restrict__ out, int *__restrict__ ecc, int *__restrict__ hops,
                                                     int *__restrict__ status, unsigned *scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hp_lds[];
    const unsigned tid = threadIdx.x;
    const long long item = blockIdx.x;
    int lo = 0, hi = G - 1;                              // the problem of this item: item0 ascends, every problem has L >= 1
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(long long)mid * HP_DESC + 8] <= item) lo = mid; else hi = mid - 1;
    }
    const long long *dg = desc + (long long)lo * HP_DESC;
    const unsigned n = (unsigned)dg[1], E = (unsigned)dg[2];
    const int K = (int)dg[3];
    const long long p0 = dg[6];
    const unsigned long long l = (unsigned long long)(item - dg[8]);
    const bool perm = p0 >= 0, sources = dg[14] == 1;
    const int *es = src + dg[0], *ed = dst + dg[0];
    const unsigned char *glab = labels + dg[4] + (perm || sources ? 0ull : l * n);   // PERM: the base labeling; sources: the one
    const bool in_lds = HP_FIXED + 8 * (long long)n + (((long long)n + 15) & ~15LL) <= lds_limit;
    NhPerm q;
    if (perm) q = nh_perm_setup((unsigned long long)dg[9], (unsigned long long)dg[7], (unsigned long long)p0 + l, n);
    else q = NhPerm{{0u, 0u, 0u, 0u, 0u, 0u}, 1u, 1u, n};

    HpTables *tb = reinterpret_cast<HpTables *>(hp_lds);
    int *oh = (!sources && l == 0 && dg[12] >= 0) ? hops + dg[12] : nullptr;
    unsigned *cur;
    if (in_lds) {                                        // the same branch for the whole workgroup
        cur = reinterpret_cast<unsigned *>(hp_lds + HP_FIXED);
        hp_solve<true>(tb, cur, cur + n, cur + 2ull * n, es, ed, glab, perm, q, sources, (unsigned)l, n, E, K, oh);
    } else {
        cur = scratch + dg[13] + (long long)l * (2 * (long long)n + ((long long)n + 3) / 4);
        hp_solve<false>(tb, cur, cur + n, cur + 2ull * n, es, ed, glab, perm, q, sources, (unsigned)l, n, E, K, oh);
    }

    const int S = sources ? HP_MAX_K : K;                // the sets of the item (a source problem has K_max = 32)
    long long *o = out + item * (long long)(K_max * K_max * 3);
    for (int idx = tid; idx < K_max * K_max; idx += HP_THREADS) {
        const int a = idx / K_max, c = idx - a * K_max;
        const bool in = a < S && c < K;
        const int cell = a * HP_MAX_K + c;
        o[idx * 3] = in ? tb->reached[cell] : 0;
        o[idx * 3 + 1] = in ? (long long)tb->sumdist[cell] : 0;
        o[idx * 3 + 2] = in ? tb->adjacent[cell] : 0;
    }
    if (tid < (unsigned)K_max) ecc[item * K_max + tid] = (int)tid < S ? tb->ecc[tid] : 0;
    if (tid == 0) {
        status[item * 2] = tb->status;
        status[item * 2 + 1] = tb->rounds;
    }
}

extern "C" int spadot_hop_sums(const int *src, const int *dst, const unsigned char *labels, const long long *desc_host,
                               const long long *desc_dev, int G, int K_max, long long lds_limit, long long *out, int *ecc,
                               int *hops, long long n_hops, int *status, unsigned *scratch, long long n_scratch, void *stream) {
    if (!desc_host || !desc_dev || !out || !ecc || !status || G <= 0 || n_hops < 0 || n_scratch < 0) return -22;
    if (K_max < 1 || K_max > HP_MAX_K) return -7;
    if (lds_limit < 0) return -22;
    if (lds_limit > HP_LDS_BYTES) lds_limit = HP_LDS_BYTES;
    long long items = 0, dyn = HP_FIXED, slabs = 0;
    for (int g = 0; g < G; ++g) {
        const long long *d = desc_host + (long long)g * HP_DESC;
        const long long eoff = d[0], n = d[1], E = d[2], K = d[3], loff = d[4], L = d[5], p0 = d[6], gid = d[7], kind = d[14];
        if (eoff < 0 || loff < 0 || n < 1 || E < 0 || L < 1 || p0 < -1 || gid < 0 || d[8] != items || d[12] < -1) return -22;
        if (kind != 0 && kind != 1) return -22;
        if (n > 2147483647LL || E > 2147483647LL || K < 1 || K > K_max) return -7;
        if (p0 >= 0 && (p0 + L > 4294967296LL || gid > 2147483647LL)) return -7;
        if (kind == 1 && (p0 != -1 || L != (n + 31) / 32 || d[12] != -1)) return -22;   // one explicit labeling, 32 sources an item
        if (kind == 1 && K_max != HP_MAX_K) return -7;                                  // 32 sets an item: out is [.., 32, 32, 3]
        if (E > 0 && (d[10] < 0 || d[11] >= n)) return -7;                   // the smallest and the largest edge end
        if (E > 0 && (!src || !dst)) return -22;
        if (!labels) return -22;
        if (d[12] >= 0 && (!hops || d[12] + n * K > n_hops)) return -22;
        items += L;
        if (items > HP_MAX_ITEMS) return -7;
        const long long need = hp_lds_bytes(n);
        if (need <= lds_limit) {
            if (need > dyn) dyn = need;
        } else {
            if (!scratch || d[13] != slabs || L > (n_scratch - slabs) / hp_slab_ints(n)) return -22;
            slabs += L * hp_slab_ints(n);
        }
    }
    static PerDeviceFlag attr_set;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_hops, hipFuncAttributeMaxDynamicSharedMemorySize, HP_LDS_BYTES) != hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL(k_hops, dim3((unsigned)items), dim3(HP_THREADS), (size_t)dyn, (hipStream_t)stream, src, dst, labels,
                       desc_dev, G, K_max, lds_limit, out, ecc, hops, status, scratch);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
