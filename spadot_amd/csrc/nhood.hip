// nhood.hip -- neighbourhood-enrichment count matrices of many (graph, labeling) problems in one launch (gfx950, wave64;
// DESIGN 7h).  The definition is restated in numpy in tests/nhood_ref.py.
//
// A graph is a directed edge list i -> j over n nodes; a labeling gives every node a label in 0 .. K-1; the count matrix is
// C[a, b] = #{edges i -> j : lab[i] = a, lab[j] = b}.  Per graph the call holds either L explicit labelings (GIVEN) or one base
// labeling and L consecutive permutation indices (PERM): labeling l is then base[pi_p(i)] with p = p0 + l and pi_p a pure
// function of (seed, graph id, p, n) -- a six-round balanced Feistel network with cycle walking, evaluated per element; no
// permutation is stored or sorted anywhere.
//
// k_nhood   one 256-thread workgroup per (graph, labeling).  LDS: four K x K int32 histograms (one per wavefront), then the
//           n label bytes of this labeling, written four to a dword.  The edges stream through in coalesced reads of src and
//           dst; an edge costs two LDS byte reads and one integer LDS atomic add on its wavefront's histogram.  Integer
//           addition commutes, so the counts do not depend on the order the atomics retire in: the result is exact, the same
//           alone, in any batch, run after run.  The four histograms are added and K_max x K_max values stored (zeros
//           included).  A graph whose labels do not fit beside the histograms (16 K^2 + n rounded up to 16 > lds_limit) takes
//           its labels from global memory instead: GIVEN reads the labeling, PERM evaluates pi at both ends of every edge
//           and reads the n-byte base labeling through L2.  No global atomics, no floating point.
#include <hip/hip_runtime.h>

#include "../../include/spadot_model.h"
#include "per_device.h"
#include "feistel_perm.h"

#define NH_THREADS 256
#define NH_WAVES 4
#define NH_MAX_K 32
#define NH_DESC 12                 // int64 columns of a graph's descriptor (include/spadot_model.h)
#define NH_LDS_BYTES 163840        // one workgroup may take the whole LDS of a compute unit
#define NH_MAX_ITEMS 2147483647LL  // (graph, labeling) pairs of one call: gridDim.x

static inline long long nh_label_bytes(long long n, long long K) { return NH_WAVES * 4 * K * K + ((n + 15) & ~15LL); }

__global__ void __launch_bounds__(NH_THREADS) k_nhood(const int *__restrict__ src, const int *__restrict__ dst,
                                                      const unsigned char *__restrict__ labels,
                                                      const long long *__restrict__ desc, int G, int K_max,
                                                      long long lds_limit, int *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nh_lds[];
    const unsigned tid = threadIdx.x;
    const long long item = blockIdx.x;
    int lo = 0, hi = G - 1;                              // the graph of this item: item0 ascends, every graph has L >= 1
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(long long)mid * NH_DESC + 8] <= item) lo = mid; else hi = mid - 1;
    }
    const long long *dg = desc + (long long)lo * NH_DESC;
    const unsigned n = (unsigned)dg[1], E = (unsigned)dg[2];
    const int K = (int)dg[3];
    const long long p0 = dg[6];
    const unsigned long long l = (unsigned long long)(item - dg[8]);
    const bool perm = p0 >= 0;
    const int *es = src + dg[0], *ed = dst + dg[0];
    const unsigned char *glab = labels + dg[4] + (perm ? 0ull : l * n);       // PERM: the base labeling
    const int KK = K * K;
    int *hist = reinterpret_cast<int *>(nh_lds);
    unsigned char *lab = nh_lds + NH_WAVES * 4 * KK;
    const bool in_lds = NH_WAVES * 4 * (long long)KK + (((long long)n + 15) & ~15LL) <= lds_limit;
    NhPerm q;
    if (perm) q = nh_perm_setup((unsigned long long)dg[9], (unsigned long long)dg[7], (unsigned long long)p0 + l, n);

    for (int i = tid; i < NH_WAVES * KK; i += NH_THREADS) hist[i] = 0;
    if (in_lds) {
        for (unsigned i0 = tid * 4; i0 < n; i0 += NH_THREADS * 4) {
            unsigned w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned i = i0 + j;
                const unsigned v = i < n ? glab[perm ? nh_perm_at(q, i) : i] : 0u;
                w |= v << (8 * j);
            }
            *reinterpret_cast<unsigned *>(lab + i0) = w;
        }
    }
    __syncthreads();
    int *mine = hist + (tid >> 6) * KK;
    // an edge end or a label out of range is refused on the host before the launch; the guards keep every access inside its array
    if (in_lds) {
        for (unsigned e = tid; e < E; e += NH_THREADS) {
            const unsigned s = (unsigned)es[e], d = (unsigned)ed[e];
            if (s < n && d < n) {
                const int a = lab[s], b = lab[d];
                if (a < K && b < K) atomicAdd(mine + a * K + b, 1);
            }
        }
    } else if (!perm) {
        for (unsigned e = tid; e < E; e += NH_THREADS) {
            const unsigned s = (unsigned)es[e], d = (unsigned)ed[e];
            if (s < n && d < n) {
                const int a = glab[s], b = glab[d];
                if (a < K && b < K) atomicAdd(mine + a * K + b, 1);
            }
        }
    } else {
        for (unsigned e = tid; e < E; e += NH_THREADS) {
            const unsigned s = (unsigned)es[e], d = (unsigned)ed[e];
            if (s < n && d < n) {
                const int a = glab[nh_perm_at(q, s)], b = glab[nh_perm_at(q, d)];
                if (a < K && b < K) atomicAdd(mine + a * K + b, 1);
            }
        }
    }
    __syncthreads();
    int *o = out + item * (long long)(K_max * K_max);
    for (int idx = tid; idx < K_max * K_max; idx += NH_THREADS) {
        const int a = idx / K_max, b = idx - a * K_max;
        int v = 0;
        if (a < K && b < K) {
#pragma unroll
            for (int w = 0; w < NH_WAVES; ++w) v += hist[w * KK + a * K + b];
        }
        o[idx] = v;
    }
}

extern "C" int spadot_nhood_counts(const int *src, const int *dst, const unsigned char *labels, const long long *desc_host,
                                   const long long *desc_dev, int G, int K_max, long long lds_limit, int *out, void *stream) {
    if (!desc_host || !desc_dev || !out || G <= 0) return -22;
    if (K_max < 1 || K_max > NH_MAX_K) return -7;
    if (lds_limit < 0) return -22;
    if (lds_limit > NH_LDS_BYTES) lds_limit = NH_LDS_BYTES;
    long long items = 0, dyn = NH_WAVES * 4 * (long long)K_max * K_max;
    for (int g = 0; g < G; ++g) {
        const long long *d = desc_host + (long long)g * NH_DESC;
        const long long eoff = d[0], n = d[1], E = d[2], K = d[3], loff = d[4], L = d[5], p0 = d[6], gid = d[7];
        if (eoff < 0 || loff < 0 || n < 1 || E < 0 || L < 1 || p0 < -1 || gid < 0 || d[8] != items) return -22;
        if (n > 2147483647LL || E > 2147483647LL || K < 1 || K > K_max) return -7;
        if (p0 >= 0 && (p0 + L > 4294967296LL || gid > 2147483647LL)) return -7;
        if (E > 0 && (d[10] < 0 || d[11] >= n)) return -7;                   // the smallest and the largest edge end
        if (E > 0 && (!src || !dst)) return -22;
        if (!labels) return -22;
        items += L;
        if (items > NH_MAX_ITEMS) return -7;
        const long long need = nh_label_bytes(n, K);
        if (need <= lds_limit && need > dyn) dyn = need;
    }
    static PerDeviceFlag attr_set;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void *)k_nhood, hipFuncAttributeMaxDynamicSharedMemorySize, NH_LDS_BYTES) != hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL(k_nhood, dim3((unsigned)items), dim3(NH_THREADS), (size_t)dyn, (hipStream_t)stream, src, dst, labels,
                       desc_dev, G, K_max, lds_limit, out);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
