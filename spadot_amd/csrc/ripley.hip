// ripley.hip -- the integers behind Ripley's L, G and F of every (problem, domain, pattern) of a call in one launch (gfx950,
// wave64).  The definition is restated in numpy in tests/ripley_ref.py.
//
// A problem is n spots with fp64 coordinates (x, y) ordered by (label, index), K cluster offsets, B squared thresholds, S
// simulations, M probe points and a convex window W (its vertices counter-clockwise plus the cumulative areas of the fan
// triangles (V0, V_{k+1}, V_{k+2})).  Domain c of n_c spots has 1 + S patterns of n_c points each: pattern 0 its own spots,
// pattern s >= 1 either the spots that receive label c under the Feistel relabeling (seed, g, s - 1) of feistel_perm.h
// (point i is xy[pi^-1(off_c + i)]: a gather) or n_c points generated in W (rp_point, stream 1 + c S + s - 1).  Per pattern
// and threshold t:
//     Lc = #{ordered pairs i != j of the pattern : d2 <= r2[t]}
//     Gc = #{points of the pattern whose nearest other point has d2 <= r2[t]}
//     Fc = #{probe points (stream 0, shared by all patterns of the problem) whose nearest point of the pattern has d2 <= r2[t]}
// with d2 the five rounded fp64 operations of pc_d2 (pair_count.h, shared with cooccur.hip; no fused multiply-add).
//
// rp_point        a generated point is a pure function of (seed, g, stream, i): three splitmix words at counter 3 i + j,
//                 u_j = (w_j >> 11) 2^-53; the triangle is the first k with fl(u_0 cum[last]) < cum[k] (binary search, cum
//                 ascends), u_1 and u_2 are reflected into the triangle, the point is (A + u_1 (B - A)) + u_2 (C - A), every
//                 operation rounded once.  Nothing is stored: a simulated pattern never exists in global memory.
// k_ripley<BP>    one 256-thread workgroup per (problem, pattern, block of 256 query points).  The first blocks query the
//                 pattern's own points (self excluded) and feed L's register counters (BP int32, compile-time indices, as
//                 k_cooccur) and G's running minimum in one pass; the blocks after them query the probe set for F and keep
//                 the minimum alone.  The pattern streams through LDS in tiles of 256, every thread producing one target per
//                 tile from the pattern's source; every lane then reads the same address (a broadcast).  Thresholds are
//                 padded with -1 (no d2 is <= -1).  The minimum is order-free; the counters go through an LDS table of 64-bit
//                 integers onto the int64 output, which the call has zeroed: integer adds commute, so the result is the same
//                 alone, in any batch, run after run.
// k_ripley_points the generated points of one (problem, stream) written out, through the same rp_point.
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/spadot_model.h"
#include "feistel_perm.h"
#include "pair_count.h"

#define RP_DESC 48                 // int64 columns of a problem's descriptor (include/spadot_model.h)
#define RP_MAX_S 9999
#define RP_MAX_M 1048576
#define RP_MAX_V 256
#define RP_GOLD 0x9E3779B97F4A7C15ull
#define RP_SALT 0x52504C5953494D31ull                  // keeps the generator's keys apart from the Feistel round keys

__host__ __device__ static inline unsigned long long rp_key(unsigned long long seed, unsigned long long g, unsigned long long stream) {
    unsigned long long s = seed ^ (g << 32) ^ stream;
    return nh_splitmix(s) ^ RP_SALT;
}

// point i of the stream with this key in the window (hv: V vertices, hc: T = V - 2 cumulative fan areas)
__device__ __forceinline__ double2 rp_point(unsigned long long key, unsigned long long i, const double2 *hv, const double *hc, int T) {
#pragma clang fp contract(off)
    unsigned long long s = key + 3ull * i * RP_GOLD;     // nh_splitmix steps the counter: words 3 i, 3 i + 1, 3 i + 2
    const double u0 = (double)(nh_splitmix(s) >> 11) * 0x1.0p-53;
    double u1 = (double)(nh_splitmix(s) >> 11) * 0x1.0p-53;
    double u2 = (double)(nh_splitmix(s) >> 11) * 0x1.0p-53;
    const double w = u0 * hc[T - 1];
    int lo = 0, hi = T - 1;                              // the first k with w < cum[k], the last triangle where there is none
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (w < hc[mid]) hi = mid; else lo = mid + 1;
    }
    if (u1 + u2 > 1.0) {
        u1 = 1.0 - u1;
        u2 = 1.0 - u2;
    }
    const double2 A = hv[0], Bv = hv[lo + 1], C = hv[lo + 2];
    const double bx = Bv.x - A.x, by = Bv.y - A.y, cx = C.x - A.x, cy = C.y - A.y;
    const double px = u1 * bx, py = u1 * by, qx = u2 * cx, qy = u2 * cy;
    double2 r;
    r.x = (A.x + px) + qx;
    r.y = (A.y + py) + qy;
    return r;
}

template <int BP>
__global__ void __launch_bounds__(PC_THREADS) k_ripley(const double2 *__restrict__ xy, const long long *__restrict__ desc,
                                                        const double *__restrict__ r2, const double2 *__restrict__ hull,
                                                        const double *__restrict__ cum, unsigned long long seed, int K_max,
                                                        int S_max, int B_max, int qb_own, unsigned long long *__restrict__ out) {
    __shared__ double2 tile[PC_THREADS];
    __shared__ double2 hv[RP_MAX_V];
    __shared__ double hc[RP_MAX_V];
    __shared__ unsigned long long tab[3 * BP];
    const int p = blockIdx.z, tid = threadIdx.x;
    const long long *d = desc + (long long)p * RP_DESC;
    // the descriptor is refused on the host before the launch; the clamps keep every access inside its array
    const long long nl = d[1];
    const int K = min(max((int)d[2], 1), min(K_max, PC_MAX_K));
    const int B = min((int)d[3], min(B_max, BP));
    const int S = min(max((int)d[4], 1), S_max);
    const int M = (int)min(max(d[5], 1ll), (long long)RP_MAX_M);
    const int modes = (int)d[7];
    const int c = blockIdx.y / (1 + S), s = blockIdx.y - c * (1 + S);
    if (c >= K) return;                                  // uniform: the grid is sized for the largest problem
    const int lo = (int)min(max(d[12 + c], 0ll), nl), hi = (int)min(max(d[13 + c], (long long)lo), nl);
    const int nc = hi - lo;
    if (nc == 0) return;                                 // a label value without spots: its counts stay zero
    const bool own = (int)blockIdx.x < qb_own;
    const int q0 = ((int)blockIdx.x - (own ? 0 : qb_own)) * PC_THREADS;
    if (own ? ((modes & 3) == 0 || q0 >= nc) : ((modes & 4) == 0 || q0 >= M)) return;

    const int V = min(max((int)d[10], 3), RP_MAX_V), T = V - 2;
    for (int i = tid; i < V; i += PC_THREADS) {
        hv[i] = hull[d[9] + i];
        hc[i] = cum[d[9] + i];
    }
    for (int i = tid; i < 3 * BP; i += PC_THREADS) tab[i] = 0ull;
    __syncthreads();

    const double2 *pts = xy + d[0];
    const double *th = r2 + (long long)p * BP;
    const unsigned long long g = (unsigned long long)d[8];
    const int kind = s == 0 ? 0 : (d[6] != 0 ? 2 : 1);   // observed, relabeled, generated
    unsigned long long key = 0ull;                       // the generator's key, or the relabeling: what the pattern's kind needs
    NhPerm pi = {};
    if (kind == 2) key = rp_key(seed, g, 1ull + (unsigned long long)c * S + (s - 1));
    if (kind == 1) pi = nh_perm_setup(seed, g, (unsigned long long)(s - 1), (unsigned)nl);
    auto target = [&](int i) -> double2 {                // point i of the pattern, 0 <= i < nc
        if (kind == 0) return pts[lo + i];
        if (kind == 1) return pts[ac_perm_inv(pi, (unsigned)(lo + i))];
        return rp_point(key, (unsigned long long)i, hv, hc, T);
    };

    const int q = q0 + tid;
    const bool on = q < (own ? nc : M);                  // idle lanes follow a valid point and add nothing
    double2 me;
    if (own) me = target(on ? q : nc - 1);
    else me = rp_point(rp_key(seed, g, 0ull), (unsigned long long)(on ? q : M - 1), hv, hc, T);    // stream 0: the probe set
    const int self = own ? q : -1;                       // a point is never its own neighbour; a probe has no self
    const bool doL = own && (modes & 1);
    double mn = INFINITY;
    int cnt[BP];
#pragma unroll
    for (int t = 0; t < BP; ++t) cnt[t] = 0;

    for (int j0 = 0; j0 < nc; j0 += PC_THREADS) {
        const int m = min(PC_THREADS, nc - j0);
        __syncthreads();                                 // the previous tile is read
        if (tid < m) tile[tid] = target(j0 + tid);
        __syncthreads();
        int jj = 0;
        if (doL) {
            for (; jj + 4 <= m; jj += 4) {               // four points per pass over the thresholds
                mn = fmin(mn, pc_pass4<BP>(cnt, th, me, tile + jj, j0 + jj, self));
            }
            for (; jj < m; ++jj) {
                const double e = pc_dist(me, tile[jj], j0 + jj, self);
                mn = fmin(mn, e);
                pc_count1<BP>(cnt, th, e);
            }
        } else {
            for (; jj < m; ++jj) mn = fmin(mn, pc_dist(me, tile[jj], j0 + jj, self));     // the nearest point alone
        }
    }
    // the threads' counters into the table, the table onto the output
    if (doL) {                                           // written here: through pc_flush_counters BP = 16 changes its occupancy
#pragma unroll
        for (int t = 0; t < BP; ++t)
            if (on && cnt[t] != 0) atomicAdd(&tab[t], (unsigned long long)cnt[t]);
    }
    if (!own || (modes & 2)) {                           // a lone point keeps mn = inf and is never counted
        const int row = own ? BP : 2 * BP;
        for (int t = 0; t < BP; ++t) {
            const unsigned long long near = __ballot(on && mn <= th[t]);
            if ((tid & 63) == 0 && near != 0ull) atomicAdd(&tab[row + t], (unsigned long long)__popcll(near));
        }
    }
    __syncthreads();
    pc_flush_table<BP>(tab, 3, B, out + ((((long long)p * K_max + c) * (1 + S_max) + s) * 3) * B_max, B_max);
}

__global__ void __launch_bounds__(PC_THREADS) k_ripley_points(const double2 *__restrict__ hull, const double *__restrict__ cum, int V,
                                                               unsigned long long key, long long count, double2 *__restrict__ out) {
    __shared__ double2 hv[RP_MAX_V];
    __shared__ double hc[RP_MAX_V];
    V = min(max(V, 3), RP_MAX_V);
    for (int i = threadIdx.x; i < V; i += PC_THREADS) {
        hv[i] = hull[i];
        hc[i] = i < V - 2 ? cum[i] : 0.0;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * PC_THREADS + threadIdx.x;
    if (i < count) out[i] = rp_point(key, (unsigned long long)i, hv, hc, V - 2);
}

// a window from its host copies: 3 .. 256 finite vertices that never turn right and go round once, ascending areas >= 0
static int rp_window(const double *h, const double *c, long long V) {
    if (V > RP_MAX_V) return -7;
    if (V < 3) return -22;
    for (long long i = 0; i < 2 * V; ++i)
        if (!std::isfinite(h[i])) return -22;
    int flips_x = 0, flips_y = 0, last_x = 0, last_y = 0, first_x = 0, first_y = 0;
    for (long long i = 0; i < V; ++i) {
        const double *a = h + 2 * i, *b = h + 2 * ((i + 1) % V), *e = h + 2 * ((i + 2) % V);
        const double ux = b[0] - a[0], uy = b[1] - a[1], vx = e[0] - b[0], vy = e[1] - b[1];
        const double l = ux * vy, r = uy * vx;
        if (l < r) return -22;                           // a right turn: not convex, or clockwise
        const int sx = (ux > 0) - (ux < 0), sy = (uy > 0) - (uy < 0);
        if (sx) { if (last_x && sx != last_x) ++flips_x; if (!first_x) first_x = sx; last_x = sx; }
        if (sy) { if (last_y && sy != last_y) ++flips_y; if (!first_y) first_y = sy; last_y = sy; }
    }
    flips_x += last_x && first_x != last_x;
    flips_y += last_y && first_y != last_y;
    if (flips_x > 2 || flips_y > 2) return -22;          // left turns all the way, but more than once round
    for (long long k = 0; k < V - 2; ++k)
        if (!std::isfinite(c[k]) || c[k] < 0.0 || (k > 0 && c[k] < c[k - 1])) return -22;
    return 0;
}

extern "C" int spadot_ripley_counts(const double *xy, const long long *desc_host, const long long *desc_dev,
                                    const double *r2_host, const double *r2_dev, const double *hull_host,
                                    const double *hull_dev, const double *cum_host, const double *cum_dev, long long hull_rows,
                                    int P, int K_max, int S_max, int B_max, long long seed, long long *out, void *stream) {
    if (!xy || !desc_host || !desc_dev || !r2_host || !r2_dev || !hull_host || !hull_dev || !cum_host || !cum_dev || !out ||
        P <= 0 || hull_rows < 3)
        return -22;
    if (K_max < 1 || K_max > PC_MAX_K || B_max < 1 || B_max > PC_MAX_B || S_max < 1 || S_max > RP_MAX_S || P > PC_MAX_GRID)
        return -7;
    const int BP = pc_padded(B_max);
    long long first = 0, nc_max = 0, m_max = 0, y_max = 0;
    for (int p = 0; p < P; ++p) {
        const long long *d = desc_host + (long long)p * RP_DESC;
        const long long n = d[1], K = d[2], B = d[3], S = d[4], M = d[5], V = d[10];
        if (n < 1 || d[0] != first) return -22;          // the problems lie back to back in xy
        if (n > PC_MAX_N || K < 1 || K > K_max || B < 1 || B > B_max || S < 1 || S > S_max || M < 1 || M > RP_MAX_M ||
            K * (1 + S) > PC_MAX_GRID || V > RP_MAX_V)
            return -7;
        if ((d[6] != 0 && d[6] != 1) || d[7] < 1 || d[7] > 7 || d[8] < 0 || d[8] > PC_MAX_G) return -22;
        if (V < 3 || d[9] < 0 || d[9] + V > hull_rows) return -22;
        int rc = pc_offsets(d + 12, K, n);
        if (!rc) rc = rp_window(hull_host + 2 * d[9], cum_host + d[9], V);
        if (!rc) rc = pc_thresholds(r2_host + (long long)p * BP, B, BP);
        if (rc) return rc;
        for (int k = 0; k < K; ++k)                       // the largest domain that queries its own points
            if ((d[7] & 3) && d[13 + k] - d[12 + k] > nc_max) nc_max = d[13 + k] - d[12 + k];
        first += n;
        if ((d[7] & 4) && M > m_max) m_max = M;
        if (K * (1 + S) > y_max) y_max = K * (1 + S);
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, sizeof(long long) * (size_t)P * K_max * (1 + S_max) * 3 * B_max, st) != hipSuccess) return -5;
    const int qb_own = (int)((nc_max + PC_THREADS - 1) / PC_THREADS), qb_probe = (int)((m_max + PC_THREADS - 1) / PC_THREADS);
    const dim3 grid((unsigned)(qb_own + qb_probe), (unsigned)y_max, (unsigned)P);
    const unsigned long long sd = (unsigned long long)seed;
    return pc_dispatch(BP, [&](auto bp) {
        hipLaunchKernelGGL(k_ripley<decltype(bp)::value>, grid, dim3(PC_THREADS), 0, st, reinterpret_cast<const double2 *>(xy),
                           desc_dev, r2_dev, reinterpret_cast<const double2 *>(hull_dev), cum_dev, sd, K_max, S_max, B_max, qb_own,
                           reinterpret_cast<unsigned long long *>(out));
        return hipGetLastError() == hipSuccess ? 0 : -5;
    });
}

extern "C" int spadot_ripley_points(const double *hull_host, const double *hull_dev, const double *cum_host, const double *cum_dev,
                                    int V, long long seed, long long g, long long stream_id, long long count, double *out,
                                    void *stream) {
    if (!hull_host || !hull_dev || !cum_host || !cum_dev || !out) return -22;
    if (count < 1 || count > PC_MAX_N || stream_id < 0 || stream_id > 1ll + (long long)PC_MAX_K * RP_MAX_S) return -7;
    if (g < 0 || g > PC_MAX_G) return -22;
    const int rc = rp_window(hull_host, cum_host, V);
    if (rc) return rc;
    const unsigned long long key = rp_key((unsigned long long)seed, (unsigned long long)g, (unsigned long long)stream_id);
    hipLaunchKernelGGL(k_ripley_points, dim3((unsigned)((count + PC_THREADS - 1) / PC_THREADS)), dim3(PC_THREADS), 0,
                       (hipStream_t)stream, reinterpret_cast<const double2 *>(hull_dev), cum_dev, V, key, count,
                       reinterpret_cast<double2 *>(out));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
