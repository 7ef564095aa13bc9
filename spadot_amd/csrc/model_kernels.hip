// model_kernels.hip -- hand-written HIP kernels (gfx950, wave64) for the model side of the SpaDOT
// training step.  ABI and reference citations: include/spadot_model.h.
//
// GAT edge phase (the memory-bound part of the step): one 256-thread workgroup per target node,
// wave w owns heads w, w+4, ...; the 64 lanes of a wave split the C channels of a head, so a row
// gather h[j, head, :] is one or two coalesced wave-wide loads.  Softmax statistics are wave
// shuffles; the weighted sum is register-accumulated in fp32; no atomics anywhere (the source-side
// gradient uses the transposed CSR instead of scatter-add), so results are bitwise reproducible.
#include <hip/hip_runtime.h>
#include <cmath>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/spadot_model.h"
#include "per_device.h"

namespace {

constexpr int WAVE = 64;
constexpr float ATT_SLOPE = 0.2f;    // GATConv negative_slope
constexpr float ACT_SLOPE = 0.01f;   // F.leaky_relu default (encoder.py:56-57)

template <typename T> __device__ __forceinline__ float ld(const T *p);
template <> __device__ __forceinline__ float ld<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float ld<__bf16>(const __bf16 *p) { return (float)*p; }
template <typename T> __device__ __forceinline__ void st(T *p, float v);
template <> __device__ __forceinline__ void st<float>(float *p, float v) { *p = v; }
template <> __device__ __forceinline__ void st<__bf16>(__bf16 *p, float v) { *p = (__bf16)v; }

// VEC consecutive elements <-> fp32 registers; one 16-byte / 8-byte access for fp32 x 4, bf16 x 8, bf16 x 4
__device__ __forceinline__ unsigned bf16_pack2(float lo, float hi) {
    const unsigned short a = __builtin_bit_cast(unsigned short, (__bf16)lo), b = __builtin_bit_cast(unsigned short, (__bf16)hi);
    return (unsigned)a | ((unsigned)b << 16);
}
template <typename T, int VEC> __device__ __forceinline__ void ldv(const T *p, float *o) {
    if constexpr (VEC == 4 && sizeof(T) == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else if constexpr (VEC == 4 && sizeof(T) == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
        o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
    } else if constexpr (VEC == 8 && sizeof(T) == 2) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
        o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
        o[4] = __uint_as_float(v.z << 16); o[5] = __uint_as_float(v.z & 0xffff0000u);
        o[6] = __uint_as_float(v.w << 16); o[7] = __uint_as_float(v.w & 0xffff0000u);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; k++) o[k] = ld<T>(p + k);
    }
}
template <typename T, int VEC> __device__ __forceinline__ void stv(T *p, const float *o) {
    if constexpr (VEC == 4 && sizeof(T) == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(o[0], o[1], o[2], o[3]);
    } else if constexpr (VEC == 4 && sizeof(T) == 2) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(bf16_pack2(o[0], o[1]), bf16_pack2(o[2], o[3]));
    } else if constexpr (VEC == 8 && sizeof(T) == 2) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(bf16_pack2(o[0], o[1]), bf16_pack2(o[2], o[3]), bf16_pack2(o[4], o[5]),
                                                   bf16_pack2(o[6], o[7]));
    } else {
#pragma unroll
        for (int k = 0; k < VEC; k++) st<T>(p + k, o[k]);
    }
}

__device__ __forceinline__ float wave_sum_f(float x) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
    return x;   // all lanes
}
__device__ __forceinline__ float wave_max_f(float x) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, WAVE));
    return x;
}
__device__ __forceinline__ double wave_sum_d(double x) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
    return x;
}
__device__ __forceinline__ double block_sum_d(double x, double *sh) {
    x = wave_sum_d(x);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) sh[wid] = x;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < nw; k++) t += sh[k];
    return t;
}

__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.f ? z : slope * z; }

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share one, each XCD has its own L2):
// give every XCD a CONTIGUOUS range of nodes, so that with spatially ordered nodes the rows one XCD gathers
// overlap and stay in its L2.  Speed only -- any placement gives the same result.  Grid = 8 * ceil(n/8).
__device__ __forceinline__ int xcd_node(int n) {
    const int chunk = (n + 7) >> 3;
    return (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
}

// ------------------------------------------------------------------------------------------
// GAT forward.  NITER*64*VEC >= C; lane owns channels {(it*64 + lane)*VEC + k}.
// ------------------------------------------------------------------------------------------
template <typename T, int VEC, int NITER>
__global__ __launch_bounds__(256) void k_gat_fwd(const T *__restrict__ h, const float *__restrict__ s_src,
                                                 const float *__restrict__ s_dst,
                                                 const int *__restrict__ rowptr,
                                                 const int *__restrict__ col,
                                                 const float *__restrict__ bias, int n, int H, int C,
                                                 int concat, int act, T *__restrict__ out,
                                                 float *__restrict__ alpha_out) {
    extern __shared__ float smem[];   // mean mode: 4 * C floats
    const int i = xcd_node(n);
    if (i >= n) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int p0 = rowptr[i], deg = rowptr[i + 1] - p0;
    const size_t HC = (size_t)H * C;
    float macc[NITER][VEC];           // head-mean accumulator (concat == 0)
#pragma unroll
    for (int it = 0; it < NITER; it++)
#pragma unroll
        for (int k = 0; k < VEC; k++) macc[it][k] = 0.f;

    for (int hd = wid; hd < H; hd += 4) {
        const float sd = s_dst[(size_t)i * H + hd];
        // softmax statistics over the incoming edges (exp(e - max) / (sum + 1e-16))
        float m = -INFINITY;
        for (int t = lane; t < deg; t += WAVE)
            m = fmaxf(m, leaky(s_src[(size_t)col[p0 + t] * H + hd] + sd, ATT_SLOPE));
        m = wave_max_f(m);
        float ssum = 0.f;
        for (int t = lane; t < deg; t += WAVE)
            ssum += __expf(leaky(s_src[(size_t)col[p0 + t] * H + hd] + sd, ATT_SLOPE) - m);
        ssum = wave_sum_f(ssum) + 1e-16f;

        float acc[NITER][VEC];
#pragma unroll
        for (int it = 0; it < NITER; it++)
#pragma unroll
            for (int k = 0; k < VEC; k++) acc[it][k] = 0.f;
        for (int base = 0; base < deg; base += WAVE) {
            const int t = base + lane;
            int j = 0;
            float a = 0.f;
            if (t < deg) {
                j = col[p0 + t];
                a = __expf(leaky(s_src[(size_t)j * H + hd] + sd, ATT_SLOPE) - m) / ssum;
                alpha_out[(size_t)(p0 + t) * H + hd] = a;
            }
            const int cnt = min(WAVE, deg - base);
#pragma unroll 8
            for (int q = 0; q < cnt; q++) {
                const int jj = __shfl(j, q, WAVE);
                const float aa = __shfl(a, q, WAVE);
                const T *row = h + (size_t)jj * HC + (size_t)hd * C;
#pragma unroll
                for (int it = 0; it < NITER; it++) {
                    const int c = (it * WAVE + lane) * VEC;
                    if (c < C) {
                        float v[VEC];
                        ldv<T, VEC>(row + c, v);
#pragma unroll
                        for (int k = 0; k < VEC; k++) acc[it][k] = fmaf(aa, v[k], acc[it][k]);
                    }
                }
            }
        }
        if (concat) {
#pragma unroll
            for (int it = 0; it < NITER; it++) {
                const int c = (it * WAVE + lane) * VEC;
                if (c < C) {
                    float o[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; k++) {
                        const float v = acc[it][k] + bias[(size_t)hd * C + c + k];
                        o[k] = act ? leaky(v, ACT_SLOPE) : v;
                    }
                    stv<T, VEC>(out + (size_t)i * HC + (size_t)hd * C + c, o);
                }
            }
        } else {
#pragma unroll
            for (int it = 0; it < NITER; it++)
#pragma unroll
                for (int k = 0; k < VEC; k++) macc[it][k] += acc[it][k];
        }
    }
    if (!concat) {
#pragma unroll
        for (int it = 0; it < NITER; it++) {
            const int c = (it * WAVE + lane) * VEC;
            if (c < C)
#pragma unroll
                for (int k = 0; k < VEC; k++) smem[wid * C + c + k] = macc[it][k];
        }
        __syncthreads();
        if (wid == 0) {
#pragma unroll
            for (int it = 0; it < NITER; it++) {
                const int c = (it * WAVE + lane) * VEC;
                if (c < C) {
                    float o[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; k++) {
                        const float v = (smem[c + k] + smem[C + c + k] + smem[2 * C + c + k] + smem[3 * C + c + k]) / (float)H
                                        + bias[c + k];
                        o[k] = act ? leaky(v, ACT_SLOPE) : v;
                    }
                    stv<T, VEC>(out + (size_t)i * C + c, o);
                }
            }
        }
    }
}


// ------------------------------------------------------------------------------------------
// Attention logits straight from h: s_src[j,h] = sum_c h[j,h,c] att_src[h,c], s_dst likewise.
// One wave per (node, head); h is read once (coalesced), the two attention vectors stay in L2.
// ------------------------------------------------------------------------------------------
template <typename T, int VEC, int NITER>
__global__ __launch_bounds__(256) void k_gat_logits(const T *__restrict__ h, const float *__restrict__ att_src,
                                                    const float *__restrict__ att_dst, int n, int H, int C,
                                                    float *__restrict__ s_src, float *__restrict__ s_dst) {
    const int j = xcd_node(n);
    if (j >= n) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int hd = wid; hd < H; hd += 4) {
        const T *row = h + (size_t)j * H * C + (size_t)hd * C;
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int it = 0; it < NITER; it++) {
            const int c = (it * WAVE + lane) * VEC;
            if (c < C) {
                float v[VEC];
                ldv<T, VEC>(row + c, v);
#pragma unroll
                for (int k = 0; k < VEC; k++) {
                    a = fmaf(v[k], att_src[(size_t)hd * C + c + k], a);
                    b = fmaf(v[k], att_dst[(size_t)hd * C + c + k], b);
                }
            }
        }
        a = wave_sum_f(a); b = wave_sum_f(b);
        if (lane == 0) { s_src[(size_t)j * H + hd] = a; s_dst[(size_t)j * H + hd] = b; }
    }
}

// d(att_src)[h,c] = sum_j ds_src[j,h] h[j,h,c] (and dst): block partials over a slab of nodes, then
// k_colsum_parts adds the slabs in order (deterministic).  part: [nslab][2 or 3][H*C] fp32; with g_pre
// (n_pre rows) the third block is its column sum, i.e. the bias gradient, taken in the same pass.
template <typename T, int VEC, int NITER>
__global__ __launch_bounds__(256) void k_gat_datt_part(const T *__restrict__ h, const float *__restrict__ ds_src,
                                                       const float *__restrict__ ds_dst, int n, int H, int C,
                                                       int nodes_per_slab, float *__restrict__ part,
                                                       const T *__restrict__ g_pre, int n_pre) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int j0 = blockIdx.x * nodes_per_slab, j1 = min(n, j0 + nodes_per_slab);
    const size_t HC = (size_t)H * C;
    for (int hd = wid; hd < H; hd += 4) {
        float as[NITER][VEC], ad[NITER][VEC], ab[NITER][VEC];
#pragma unroll
        for (int it = 0; it < NITER; it++)
#pragma unroll
            for (int k = 0; k < VEC; k++) { as[it][k] = 0.f; ad[it][k] = 0.f; ab[it][k] = 0.f; }
        // four nodes per trip, all their row loads issued before the first is used (one node per trip left the
        // slab latency-bound: 34 us for 82 MB)
        constexpr int UJ = 4;
        for (int jb = j0; jb < j1; jb += UJ) {
            float ws[UJ], wd[UJ], v[UJ][NITER][VEC], gv[UJ][NITER][VEC];
            bool with_g[UJ];
#pragma unroll
            for (int u = 0; u < UJ; u++) {
                const int j = min(jb + u, j1 - 1);
                const bool live = jb + u < j1;
                ws[u] = live ? ds_src[(size_t)j * H + hd] : 0.f;
                wd[u] = live ? ds_dst[(size_t)j * H + hd] : 0.f;
                with_g[u] = live && g_pre != nullptr && j < n_pre;
                const T *row = h + (size_t)j * HC + (size_t)hd * C;
                const T *grow = g_pre + (size_t)(with_g[u] ? j : 0) * HC + (size_t)hd * C;
#pragma unroll
                for (int it = 0; it < NITER; it++) {
                    const int c = (it * WAVE + lane) * VEC;
#pragma unroll
                    for (int k = 0; k < VEC; k++) { v[u][it][k] = 0.f; gv[u][it][k] = 0.f; }
                    if (c < C) {
                        ldv<T, VEC>(row + c, v[u][it]);
                        if (with_g[u]) ldv<T, VEC>(grow + c, gv[u][it]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UJ; u++)
#pragma unroll
                for (int it = 0; it < NITER; it++)
#pragma unroll
                    for (int k = 0; k < VEC; k++) {
                        as[it][k] = fmaf(ws[u], v[u][it][k], as[it][k]);
                        ad[it][k] = fmaf(wd[u], v[u][it][k], ad[it][k]);
                        ab[it][k] += gv[u][it][k];
                    }
        }
        const int nblk = g_pre ? 3 : 2;
        float *ps = part + (size_t)blockIdx.x * nblk * HC + (size_t)hd * C;
#pragma unroll
        for (int it = 0; it < NITER; it++) {
            const int c = (it * WAVE + lane) * VEC;
            if (c < C)
#pragma unroll
                for (int k = 0; k < VEC; k++) {
                    ps[c + k] = as[it][k]; ps[HC + c + k] = ad[it][k];
                    if (g_pre) ps[2 * HC + c + k] = ab[it][k];
                }
        }
    }
}
// out[c] = sum_s part[s][c]: 64 columns x CS_GY slab-groups per workgroup, groups combined in fixed order.
// (16 groups = 1024 threads; the 256-thread form was tried for the side stream's sake -- see BN_RG -- and lost 2 % of
// the step on the same box: tools/ab_wgsize.sh)
constexpr int CS_GY = 16, CS_NT = 64 * CS_GY;
__global__ __launch_bounds__(CS_NT) void k_colsum_parts(const float *__restrict__ part, int nslab, int width,
                                                        float *__restrict__ out) {
    __shared__ float sh[CS_GY][65];
    const int cx = threadIdx.x & 63, gy = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    float acc = 0.f;
    {
        // sixteen loads in flight, added in ascending order.  UNCONDITIONAL loads from a clamped position, masked afterwards:
        // written as `(sb + u < s1) ? part[..] : 0` (until round 5) each load was a branch with the load queue drained at its
        // join -- 20 dependent round trips for the 312 block partials of a GAT layer, 56-63 us for 7.7 MB at the end of the
        // step's critical chain.
        const int cc = min(c, width - 1);
        const int per = (nslab + CS_GY - 1) / CS_GY;
        const int s0 = gy * per, s1 = min(nslab, s0 + per);
        for (int sb = s0; sb < s1; sb += 16) {
            float q[16];
#pragma unroll
            for (int u = 0; u < 16; u++) q[u] = part[(size_t)min(sb + u, nslab - 1) * width + cc];
#pragma unroll
            for (int u = 0; u < 16; u++) acc += (sb + u < s1) ? q[u] : 0.f;
        }
    }
    sh[gy][cx] = acc;
    __syncthreads();
    if (gy != 0 || c >= width) return;
    acc = 0.f;
#pragma unroll
    for (int g = 0; g < CS_GY; g++) acc += sh[g][cx];
    out[c] = acc;
}

// ------------------------------------------------------------------------------------------
// GAT backward, target side: g_pre, dz (per edge, per head), ds_dst.
// ------------------------------------------------------------------------------------------
template <typename T, int VEC, int NITER>
__global__ __launch_bounds__(256) void k_gat_bwd_target(
    const T *__restrict__ g_out, const T *__restrict__ out, const T *__restrict__ h,
    const float *__restrict__ s_src, const float *__restrict__ s_dst, const float *__restrict__ alpha,
    const int *__restrict__ rowptr, const int *__restrict__ col, int n, int H, int C, int concat, int act,
    T *__restrict__ g_pre, float *__restrict__ dz, float *__restrict__ ds_dst) {
    const int i = xcd_node(n);
    if (i >= n) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int p0 = rowptr[i], deg = rowptr[i + 1] - p0;
    const size_t HC = (size_t)H * C;
    for (int hd = wid; hd < H; hd += 4) {
        float g[NITER][VEC];
#pragma unroll
        for (int it = 0; it < NITER; it++) {
            const int c = (it * WAVE + lane) * VEC;
#pragma unroll
            for (int k = 0; k < VEC; k++) g[it][k] = 0.f;
            if (c < C) {
                float go[VEC], oo[VEC];
                const size_t off = concat ? (size_t)i * HC + (size_t)hd * C + c : (size_t)i * C + c;
                ldv<T, VEC>(g_out + off, go);
                if (act) ldv<T, VEC>(out + off, oo);
#pragma unroll
                for (int k = 0; k < VEC; k++) {
                    float v = go[k];
                    if (act && !(oo[k] > 0.f)) v *= ACT_SLOPE;
                    g[it][k] = concat ? v : v / (float)H;
                }
                stv<T, VEC>(g_pre + (size_t)i * HC + (size_t)hd * C + c, g[it]);
            }
        }
        const float sd = s_dst[(size_t)i * H + hd];
        // phase 1: d(alpha) per edge (parked in dz), and sum_k alpha_k d(alpha_k).  Edges go eight at a time:
        // their row loads are issued together, and the eight wave-wide dot products are reduced by ONE
        // butterfly (each exchange step halves the values a lane carries: 11 shuffles instead of 48).
        float dsum = 0.f;
        for (int base = 0; base < deg; base += WAVE) {
            const int t = base + lane;
            const int j = (t < deg) ? col[p0 + t] : 0;
            const int cnt = min(WAVE, deg - base);
            float da = 0.f;
            for (int q0 = 0; q0 < cnt; q0 += 8) {
                float p[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int jj = __shfl(j, min(q0 + u, cnt - 1), WAVE);
                    const T *row = h + (size_t)jj * HC + (size_t)hd * C;
                    float part = 0.f;
#pragma unroll
                    for (int it = 0; it < NITER; it++) {
                        const int c = (it * WAVE + lane) * VEC;
                        if (c < C) {
                            float v[VEC];
                            ldv<T, VEC>(row + c, v);
#pragma unroll
                            for (int k = 0; k < VEC; k++) part = fmaf(g[it][k], v[k], part);
                        }
                    }
                    p[u] = part;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const bool hi = (lane & 32) != 0;
                    const float keep = hi ? p[u + 4] : p[u], send = hi ? p[u] : p[u + 4];
                    p[u] = keep + __shfl_xor(send, 32, WAVE);
                }
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const bool hi = (lane & 16) != 0;
                    const float keep = hi ? p[u + 2] : p[u], send = hi ? p[u] : p[u + 2];
                    p[u] = keep + __shfl_xor(send, 16, WAVE);
                }
                {
                    const bool hi = (lane & 8) != 0;
                    const float keep = hi ? p[1] : p[0], send = hi ? p[0] : p[1];
                    p[0] = keep + __shfl_xor(send, 8, WAVE);
                }
                p[0] += __shfl_xor(p[0], 4, WAVE);
                p[0] += __shfl_xor(p[0], 2, WAVE);
                p[0] += __shfl_xor(p[0], 1, WAVE);
                // lane L now holds the dot product of edge q0 + ((L >> 3) & 7)
                const float mine = __shfl(p[0], ((lane - q0) & 7) << 3, WAVE);
                if (lane >= q0 && lane < q0 + 8) da = mine;
            }
            if (t < deg) {
                const float a = alpha[(size_t)(p0 + t) * H + hd];
                dsum += a * da;
                dz[(size_t)(p0 + t) * H + hd] = da;
            }
        }
        dsum = wave_sum_f(dsum);
        // phase 2: softmax + leaky backward
        float dsd = 0.f;
        for (int t = lane; t < deg; t += WAVE) {
            const size_t e = (size_t)(p0 + t) * H + hd;
            const float a = alpha[e];
            const float z = s_src[(size_t)col[p0 + t] * H + hd] + sd;
            const float d = a * (dz[e] - dsum) * (z > 0.f ? 1.f : ATT_SLOPE);
            dz[e] = d;
            dsd += d;
        }
        dsd = wave_sum_f(dsd);
        if (lane == 0) ds_dst[(size_t)i * H + hd] = dsd;
    }
}

// GAT backward, source side: gather over OUTGOING edges (transposed CSR).
template <typename T, int VEC, int NITER>
__global__ __launch_bounds__(256) void k_gat_bwd_source(
    const T *__restrict__ g_pre, const float *__restrict__ alpha, const float *__restrict__ dz,
    const int *__restrict__ rowptr_t, const int *__restrict__ col_t, const int *__restrict__ eid_t, int n,
    int H, int C, T *__restrict__ dh, float *__restrict__ ds_src, const float *__restrict__ ds_dst,
    const float *__restrict__ att_src, const float *__restrict__ att_dst) {
    const int j = xcd_node(n);
    if (j >= n) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int p0 = rowptr_t[j], deg = rowptr_t[j + 1] - p0;
    const size_t HC = (size_t)H * C;
    for (int hd = wid; hd < H; hd += 4) {
        float acc[NITER][VEC];
#pragma unroll
        for (int it = 0; it < NITER; it++)
#pragma unroll
            for (int k = 0; k < VEC; k++) acc[it][k] = 0.f;
        float sds = 0.f;
        for (int base = 0; base < deg; base += WAVE) {
            const int t = base + lane;
            int i = 0;
            float a = 0.f;
            if (t < deg) {
                i = col_t[p0 + t];
                const size_t e = (size_t)eid_t[p0 + t] * H + hd;
                a = alpha[e];
                sds += dz[e];
            }
            const int cnt = min(WAVE, deg - base);
#pragma unroll 8
            for (int q = 0; q < cnt; q++) {
                const int ii = __shfl(i, q, WAVE);
                const float aa = __shfl(a, q, WAVE);
                const T *row = g_pre + (size_t)ii * HC + (size_t)hd * C;
#pragma unroll
                for (int it = 0; it < NITER; it++) {
                    const int c = (it * WAVE + lane) * VEC;
                    if (c < C) {
                        float v[VEC];
                        ldv<T, VEC>(row + c, v);
#pragma unroll
                        for (int k = 0; k < VEC; k++) acc[it][k] = fmaf(aa, v[k], acc[it][k]);
                    }
                }
            }
        }
        sds = wave_sum_f(sds);
        if (lane == 0) ds_src[(size_t)j * H + hd] = sds;
        // logits were s = h . att (k_gat_logits): their gradient reaches h here, no extra pass over dh
        const float gsd = att_src ? ds_dst[(size_t)j * H + hd] : 0.f;
#pragma unroll
        for (int it = 0; it < NITER; it++) {
            const int c = (it * WAVE + lane) * VEC;
            if (c < C) {
                if (att_src) {
#pragma unroll
                    for (int k = 0; k < VEC; k++)
                        acc[it][k] += sds * att_src[(size_t)hd * C + c + k] + gsd * att_dst[(size_t)hd * C + c + k];
                }
                stv<T, VEC>(dh + (size_t)j * HC + (size_t)hd * C + c, acc[it]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Kernel matrix (svgp.py:110-125)
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_kernel_matrix(const T *__restrict__ x, const T *__restrict__ z,
                                                       int n, int m, int d, double scale, int kind,
                                                       T *__restrict__ K) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= m || i >= n) return;
    double d2 = 0.0;
    for (int k = 0; k < d; k++) {
        const double t = (double)x[(size_t)i * d + k] - (double)z[(size_t)j * d + k];
        d2 += t * t;
    }
    double r;
    if (kind == SPADOT_KERNEL_GAUSSIAN) r = exp(-d2 / scale);
    else if (kind == SPADOT_KERNEL_CAUCHY) r = 1.0 / (1.0 + d2 / scale);
    else r = 1.0 - d2 / (d2 + scale);
    K[(size_t)i * m + j] = (T)r;
}


// ------------------------------------------------------------------------------------------
// Batched SPD inverse + log-determinant (fp64) by the symmetric SWEEP operator, one 512-thread
// workgroup per matrix, the whole lower triangle resident in registers.
//   sweep(k): d = B_kk;  B_kk <- -1/d;  B_ik <- B_ik/d (i != k);  B_ij <- B_ij - B_ik B_kj / d.
// After sweeping k = 0..m-1:  B = -A^-1 and log|A| = sum_k log d_k (every pivot is a Schur
// complement, positive for an SPD matrix, so no pivoting is needed).
// Thread t owns tile (ti, tj), ti >= tj, of TS x TS entries (diagonal tiles keep the full square);
// column k travels through a double-buffered LDS vector, one barrier per sweep.
// Replaces the LU-based torch.linalg.inv / Cholesky chains on the L x (m x m) SVGP matrices
// (svgp.py:50,75,87-88): 2 launches instead of ~700 library kernels per training step.
// ------------------------------------------------------------------------------------------
// 512 threads (2 waves per SIMD, 256 VGPRs), tile grid T <= 31.  A TS x TS tile keeps its RS x RS core
// (RS = min(TS, SWEEP_RS)) in registers and the L-shaped rest in a thread-private LDS strip (slot-major, so the 64
// lanes of a wave touch 64 consecutive doubles: conflict-free): TS = 8, 9 reach m = 248, 279 without the
// compiler spilling the tile (a spilled build measured ~10x slower; a 256-thread / 512-register build 4-40x).
constexpr int SWEEP_NT = 512;
constexpr int SWEEP_RS = 9;

template <int TS, int RSMAX>
struct SweepTile {
    static constexpr int RS = TS < RSMAX ? TS : RSMAX;
    double a[RS][RS];
    double *bord;     // LDS strip of this thread: element slot s lives at bord[s * SWEEP_NT]
    // border slot of (r, c): row-major rank among the entries with r >= RS or c >= RS
    static __device__ __forceinline__ constexpr int slot(int r, int c) {
        return r < RS ? r * (TS - RS) + (c - RS) : RS * (TS - RS) + (r - RS) * TS + c;
    }
    __device__ __forceinline__ double get(int r, int c) const {
        if (r < RS && c < RS) return a[r < RS ? r : 0][c < RS ? c : 0];
        return bord[slot(r, c) * SWEEP_NT];
    }
    __device__ __forceinline__ void set(int r, int c, double v) {
        if (r < RS && c < RS) a[r < RS ? r : 0][c < RS ? c : 0] = v;
        else bord[slot(r, c) * SWEEP_NT] = v;
    }
};

template <int TS, int RSMAX = SWEEP_RS>
__global__ __launch_bounds__(SWEEP_NT) void k_spd_sweep(const double *__restrict__ A, int m, int T,
                                                        double *__restrict__ Ainv,
                                                        double *__restrict__ logdet, int Lsrc = 0,
                                                        const double *__restrict__ add0 = nullptr,
                                                        const double *__restrict__ add1 = nullptr) {
    extern __shared__ double colbuf[];          // 2 x (T*TS + 1) column buffers (+ 1/pivot), m pivots, 16 scratch, tile borders
    constexpr int CS = TS + ((TS & 1) ? 0 : 1);   // column-buffer stride per tile: odd, so lanes of consecutive tiles spread over the LDS banks
    const int mp = T * CS;
    double *piv = colbuf + 2 * (mp + 1);
    // matrix b = A[b mod Lsrc] + add0 (+ add1 for b >= Lsrc): the SVGP step inverts Sigma_l = G_l + (K + jI) and
    // Sigma_l + K^2/j for every latent dimension from ONE stored G (no copy / add launches in front of the sweep)
    const int src = Lsrc > 0 ? (int)(blockIdx.x % (unsigned)Lsrc) : (int)blockIdx.x;
    const bool hi = Lsrc > 0 && (int)blockIdx.x >= Lsrc;
    const double *Am = A + (size_t)src * m * m;
    double *Om = Ainv + (size_t)blockIdx.x * m * m;
    const int t = threadIdx.x;
    const int ntiles = T * (T + 1) / 2;
    int ti = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
    while (ti * (ti + 1) / 2 > t) ti--;
    const int tj = t - ti * (ti + 1) / 2;
    const bool live = t < ntiles;
    SweepTile<TS, RSMAX> tile;
    tile.bord = piv + m + 16 + t;
    // The tile arrives one row at a time through BUFFER loads: one 32-bit row offset per row, the column as an immediate, the
    // range check of the descriptor instead of a guard (what lies past the matrix reads as zero and is replaced by the identity
    // padding; a null add0 / add1 is a descriptor of zero bytes).  All 3 TS loads of a row are issued before the first is used.
    // The first form (`if (live && i < m && j < m) v = rowp[c]`, then two more guarded loads) made every element a chain of
    // branches the compiler drains the load queue at: 3 TS^2 = 243 dependent round trips at TS = 9, about half of the
    // kernel's 305 us in the step (profiles/r05/ab_unpredicated_loads.txt).
    const unsigned mbytes = (unsigned)m * (unsigned)m * 8u;
    const auto rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(Am), 0, mbytes, 0x00020000);
    const auto r0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(add0), 0, add0 ? mbytes : 0u, 0x00020000);
    const auto r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(add1), 0, (hi && add1) ? mbytes : 0u, 0x00020000);
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int r = 0; r < TS; r++) {
        const int i = ti * TS + r;
        const unsigned voff = ((unsigned)min(i, m - 1) * (unsigned)m + (unsigned)(tj * TS)) * 8u;
        u32x2 va[TS], v0[TS], v1[TS];
#pragma unroll
        for (int c = 0; c < TS; c++) {
            va[c] = __builtin_amdgcn_raw_buffer_load_b64(rA, voff + 8u * c, 0, 0);
            v0[c] = __builtin_amdgcn_raw_buffer_load_b64(r0, voff + 8u * c, 0, 0);
            v1[c] = __builtin_amdgcn_raw_buffer_load_b64(r1, voff + 8u * c, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < TS; c++) {
            const int j = tj * TS + c;
            // (an absent term reads as +0.0 through its empty descriptor: no branch in this phase)
            const double v = (__builtin_bit_cast(double, va[c]) + __builtin_bit_cast(double, v0[c])) + __builtin_bit_cast(double, v1[c]);
            tile.set(r, c, (live && i < m && j < m) ? v : ((i == j) ? 1.0 : 0.0));      // padding: identity
        }
        __builtin_amdgcn_sched_barrier(0);      // rows one after the other: all 3 TS^2 loads hoisted to the top spill the tile
    }
    // Pivot k = kt*TS + kr with kr unrolled: which register of a tile holds the pivot row / column is then
    // known at compile time (no per-element selects; the selects were ~80% of the instructions issued).
    for (int kt = 0; kt < T; kt++) {
#pragma unroll
        for (int kr = 0; kr < TS; kr++) {
            const int k = kt * TS + kr;
            if (k >= m) break;
            double *col = colbuf + (k & 1) * (mp + 1);
            if (live && tj == kt) {
#pragma unroll
                for (int r = 0; r < TS; r++) col[ti * CS + r] = tile.get(r, kr);
                if (ti == kt) col[mp] = 1.0 / tile.get(kr, kr);
            } else if (live && ti == kt) {
#pragma unroll
                for (int c = 0; c < TS; c++) col[tj * CS + c] = tile.get(kr, c);
            }
            __syncthreads();
            const double inv_d = col[mp];
            if (t == 0) piv[k] = col[kt * CS + kr];          // log|A| = sum log d_k, taken after the sweep
            if (live) {
                // generic rank-1 update for every entry: a_rc -= (c_r / d) c_c
                double sr[TS];
#pragma unroll
                for (int r = 0; r < TS; r++) sr[r] = -col[ti * CS + r] * inv_d;
#pragma unroll
                for (int c = 0; c < TS; c++) {
                    const double ccv = col[tj * CS + c];
#pragma unroll
                    for (int r = 0; r < TS; r++) tile.set(r, c, fma(sr[r], ccv, tile.get(r, c)));
                }
                // ... then the pivot column / row / pivot itself are overwritten with their closed forms
                if (tj == kt) {
#pragma unroll
                    for (int r = 0; r < TS; r++) tile.set(r, kr, -sr[r]);                 // c_r / d
                }
                if (ti == kt) {
#pragma unroll
                    for (int c = 0; c < TS; c++) tile.set(kr, c, col[tj * CS + c] * inv_d);
                    if (tj == kt) tile.set(kr, kr, -inv_d);
                }
            }
        }
    }
    if (live) {
        // lower tile: rows of the tile are contiguous in memory
#pragma unroll
        for (int r = 0; r < TS; r++) {
            const int i = ti * TS + r;
            double *rowp = Om + (size_t)min(i, m - 1) * m + tj * TS;
#pragma unroll
            for (int c = 0; c < TS; c++)
                if (i < m && tj * TS + c < m) rowp[c] = -tile.get(r, c);
        }
        // mirrored upper tile: columns of the tile become contiguous rows
        if (ti != tj) {
#pragma unroll
            for (int c = 0; c < TS; c++) {
                const int j = tj * TS + c;
                double *rowp = Om + (size_t)min(j, m - 1) * m + ti * TS;
#pragma unroll
                for (int r = 0; r < TS; r++)
                    if (j < m && ti * TS + r < m) rowp[r] = -tile.get(r, c);
            }
        }
    }
    __syncthreads();
    double ld = 0.0;
    for (int k = t; k < m; k += SWEEP_NT) ld += log(piv[k]);
    ld = block_sum_d(ld, piv + m);            // 16 scratch doubles behind the pivots
    if (t == 0) logdet[blockIdx.x] = ld;
}

// out[l,i] = sum_k A[l,i,k] B[i,k] : one wave per (l,i)
template <typename T>
__global__ __launch_bounds__(256) void k_rowdot_fwd(const T *__restrict__ A, const T *__restrict__ B, int L,
                                                    int n, int m, T *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long long)L * n) return;
    const int i = (int)(r % n);
    const T *a = A + (size_t)r * m, *b = B + (size_t)i * m;
    double acc = 0.0;
    for (int k = lane; k < m; k += WAVE) acc += (double)a[k] * (double)b[k];
    acc = wave_sum_d(acc);
    if (lane == 0) out[r] = (T)acc;
}
template <typename T>
__global__ __launch_bounds__(256) void k_rowdot_bwd(const T *__restrict__ g, const T *__restrict__ B, int L,
                                                    int n, int m, T *__restrict__ gA) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long tot = (long long)L * n * m;
    if (idx >= tot) return;
    const long long r = idx / m;
    const int k = (int)(idx % m), i = (int)(r % n);
    gA[idx] = (T)((double)g[r] * (double)B[(size_t)i * m + k]);
}

// q1[l, i] = sum_n G2T[l, n] T[l, n, i]^2 + 1/2 g_kl m0[l, i]      (T [L, 2 nh, b] in two halves, G2T [L, 2 nh], m0 and q1 [L, b]; fp64)
// = diag(K_nm S_l D_l S_l K_mn) of _SVGPCore.backward with D_l = X2^T diag(G2_l) X2 + g_kl/2 M, T_l = X2 S_l K_mn and
// m0_l = diag(K_nm S_l M S_l K_mn) formed ahead of the backward pass (they do not depend on the incoming gradients).
// Workgroup = 16 columns x 16 row slices; a slice walks its rows n = s, s + 16, ... in order, the slices are added in order.
__global__ __launch_bounds__(256) void k_svgp_q1t(const double *__restrict__ Ta, const double *__restrict__ Tb,
                                                  const double *__restrict__ G2T, const double *__restrict__ m0,
                                                  const double *__restrict__ g_kl, int nh, int b, double *__restrict__ q1) {
    __shared__ double part[16][17];
    const int l = blockIdx.y, c = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + c;
    // rows 0 .. nh-1 of T_l live in Ta [L, nh, b], rows nh .. 2 nh - 1 in Tb [L, nh, b]
    const double *Tal = Ta + (size_t)l * nh * b, *Tbl = Tb + (size_t)l * nh * b, *gl = G2T + (size_t)l * 2 * nh;
    double acc = 0.0;
    if (i < b) {
#pragma unroll 8
        for (int n = sl; n < nh; n += 16) {
            const double t = Tal[(size_t)n * b + i];
            acc = fma(gl[n] * t, t, acc);
        }
#pragma unroll 8
        for (int n = sl; n < nh; n += 16) {
            const double t = Tbl[(size_t)n * b + i];
            acc = fma(gl[nh + n] * t, t, acc);
        }
    }
    part[sl][c] = acc;
    __syncthreads();
    if (sl == 0 && i < b) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < 16; k++) a += part[k][c];
        q1[(size_t)l * b + i] = a + 0.5 * g_kl[0] * m0[(size_t)l * b + i];
    }
}

constexpr double LOG_2PI = 1.8378770664093453;   // SpaDOT.py:138

template <typename T>
__global__ __launch_bounds__(1024) void k_elbo_fwd(const T *mu, const T *var, const T *mv, const T *tr,
                                                   const T *pm, const T *pv, const T *kt, int b, int L,
                                                   T *out2) {
    __shared__ double sh[16];
    double l3 = 0.0, ce = 0.0;
    const int tot = b * L;
    for (int e = threadIdx.x; e < tot; e += blockDim.x) {
        const int i = e / L;
        const double v = var[e], m_ = mu[e], d = m_ - (double)mv[e];
        l3 += ((double)kt[i] + (double)tr[e]) / v + log(v) + LOG_2PI + d * d / v;
        const double p = pm[e];
        ce += LOG_2PI + log(v) + ((double)pv[e] + p * p - 2.0 * p * m_ + m_ * m_) / v;
    }
    l3 = block_sum_d(l3, sh);
    ce = block_sum_d(ce, sh);
    if (threadIdx.x == 0) { out2[0] = (T)(-0.5 * l3); out2[1] = (T)(-0.5 * ce); }
}

// ------------------------------------------------------------------------------------------
// SVGP branch after the batched inverse (fp64, single workgroup: b*L ~ 5k elements, L*m ~ 2.4k, m*m ~ 58k).
//   raw = X2 r^T [2b, L] with X2 = [K_nm; P];  rd = rowdot(X2 S, X2) [L, 2b];  r, Mr [L, m];  ld [2L];  sm [L]
//   p_m = c raw[:b], mv = c raw[b:], p_v = k~ + rd[:, :b]^T, tr = rd[:, b:]^T                         (svgp.py:62-84)
//   l3, ce as k_elbo_fwd; kl = sum_l 1/2 (kl_const + ld_l - ld_{L+l} + sm_l + c^2 Mr_l . r_l)        (svgp.py:86-104)
//   SVGP_KL = -|ce - (l3 - (b/N) kl)| / L                                                             (SpaDOT.py:72-77)
//   out4 = (l3, ce, kl, SVGP_KL)
__global__ __launch_bounds__(1024) void k_svgp_post_fwd(const double *__restrict__ raw, const double *__restrict__ rd,
                                                        const double *__restrict__ r, const double *__restrict__ Mr,
                                                        const double *__restrict__ ld, const double *__restrict__ sm,
                                                        const double *__restrict__ mu, const double *__restrict__ var,
                                                        const double *__restrict__ kt, int b, int L, int m, double c,
                                                        double kl_const, double b_over_N, double *__restrict__ p_m,
                                                        double *__restrict__ mv, double *__restrict__ p_v,
                                                        double *__restrict__ tr, double *__restrict__ out4,
                                                        float *__restrict__ skl32) {
    __shared__ double sh[16];
    double l3 = 0.0, ce = 0.0, kl = 0.0;
    const int tot = b * L;
#pragma unroll 5
    for (int e = threadIdx.x; e < tot; e += blockDim.x) {
        const int i = e / L, l = e - i * L;
        const double pm = c * raw[e], mvv = c * raw[(size_t)(b + i) * L + l];
        const double pv = kt[i] + rd[(size_t)l * 2 * b + i], trv = rd[(size_t)l * 2 * b + b + i];
        p_m[e] = pm; mv[e] = mvv; p_v[e] = pv; tr[e] = trv;
        const double v = var[e], m_ = mu[e], d = m_ - mvv;
        l3 += (kt[i] + trv) / v + log(v) + LOG_2PI + d * d / v;
        ce += LOG_2PI + log(v) + (pv + pm * pm - 2.0 * pm * m_ + m_ * m_) / v;
    }
#pragma unroll 3
    for (int e = threadIdx.x; e < L * m; e += blockDim.x) kl += c * c * Mr[e] * r[e];
    for (int l = threadIdx.x; l < L; l += blockDim.x) kl += kl_const + ld[l] - ld[L + l] + sm[l];
    l3 = -0.5 * block_sum_d(l3, sh);
    ce = -0.5 * block_sum_d(ce, sh);
    kl = 0.5 * block_sum_d(kl, sh);
    if (threadIdx.x == 0) {
        out4[0] = l3; out4[1] = ce; out4[2] = kl;
        out4[3] = -fabs(ce - (l3 - b_over_N * kl)) / L;
        if (skl32) skl32[0] = (float)out4[3];
    }
}

// The part of k_svgp_post_fwd the loss tail waits for: p_m = c raw[:b], p_v = k~ + diag(K_nm S_l K_mn) (rd_a [L, b]); the ELBO
// scalars (l3, ce, kl, SVGP_KL) and mv / tr follow later, off the step's critical chain (svgp.py: ELBO_LATE).
__global__ __launch_bounds__(256) void k_svgp_post_pmpv(const double *__restrict__ raw, const double *__restrict__ rd_a,
                                                        const double *__restrict__ kt, int b, int L, double c,
                                                        double *__restrict__ p_m, double *__restrict__ p_v) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= b * L) return;
    const int i = e / L, l = e - i * L;
    p_m[e] = c * raw[e];
    p_v[e] = kt[i] + rd_a[(size_t)l * b + i];
}

// Backward of the above: g_skl = d loss / d SVGP_KL (fp32 device scalar), G_pm / G_pv = upstream gradients of the
// posterior (from the latent head; may be null).  Writes the direct gradients g_mu, g_var [b, L], the two operands of
// the algebra's backward G1 = [dL/dp_m; dL/dmv] [2b, L] and G2T = [dL/dp_v | dL/dtr]^T [L, 2b], the scalar g_kl,
// gMr = g_kl c^2 Mr [L, m] and gM = g_kl/2 M [m, m].
__global__ __launch_bounds__(256) void k_svgp_post_bwd(const float *__restrict__ g_skl, const double *__restrict__ out4,
                                                       const double *__restrict__ G_pm, const double *__restrict__ G_pv,
                                                       const double *__restrict__ mu, const double *__restrict__ var,
                                                       const double *__restrict__ mv, const double *__restrict__ tr,
                                                       const double *__restrict__ pm, const double *__restrict__ pv,
                                                       const double *__restrict__ kt, const double *__restrict__ Mr,
                                                       const double *__restrict__ M, int b, int L, int m, double c,
                                                       double b_over_N, double *__restrict__ g_mu,
                                                       double *__restrict__ g_var, double *__restrict__ G1,
                                                       double *__restrict__ G2T, double *__restrict__ g_kl,
                                                       double *__restrict__ gMr, double *__restrict__ gM) {
    const double gs = g_skl ? (double)g_skl[0] : 0.0;
    const double dd = out4[1] - (out4[0] - b_over_N * out4[2]);
    const double sg = dd > 0.0 ? 1.0 : (dd < 0.0 ? -1.0 : 0.0);
    const double gl = -0.5 * (gs * sg / L), gc = -0.5 * (-gs * sg / L);     // through l3 = -1/2 sum, ce = -1/2 sum
    const double gk = -gs * sg * b_over_N / L;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx == 0) g_kl[0] = gk;
    if (idx < (long long)b * L) {
        const int e = (int)idx, i = e / L, l = e - i * L;
        const double v = var[e], m_ = mu[e], d = m_ - mv[e], p = pm[e];
        const double q = pv[e] + p * p - 2.0 * p * m_ + m_ * m_;
        const double a3 = kt[i] + tr[e];
        g_mu[e] = gl * (2.0 * d / v) + gc * ((2.0 * m_ - 2.0 * p) / v);
        g_var[e] = gl * (-a3 / (v * v) + 1.0 / v - d * d / (v * v)) + gc * (1.0 / v - q / (v * v));
        G1[e] = (G_pm ? G_pm[e] : 0.0) + gc * ((2.0 * p - 2.0 * m_) / v);
        G1[(size_t)(b + i) * L + l] = gl * (-2.0 * d / v);
        G2T[(size_t)l * 2 * b + i] = (G_pv ? G_pv[e] : 0.0) + gc / v;
        G2T[(size_t)l * 2 * b + b + i] = gl / v;
    }
    if (idx < (long long)L * m) gMr[idx] = gk * c * c * Mr[idx];
    if (idx < (long long)m * m) gM[idx] = 0.5 * gk * M[idx];
}

// z [b, 2L] fp32 = SVGP_fc output (mu | logvar)  ->  mu, var = exp(logvar), w = 1/var, mu*w  (all [b, L] fp64)
// k_svgp_pre plus A[l, i, :] = K_nm[i, :] / var[i, l] (the left factor of Sigma_l's batch term): one wave per (i, l)
__global__ __launch_bounds__(256) void k_svgp_pre2(const float *__restrict__ z, const double *__restrict__ Kn, int b, int L,
                                                   int m, double *__restrict__ mu, double *__restrict__ var,
                                                   double *__restrict__ w, double *__restrict__ muw, double *__restrict__ A) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= b * L) return;
    const int i = e / L, l = e - i * L;
    const double m_ = (double)z[(size_t)i * 2 * L + l];
    const double v = (double)expf(z[(size_t)i * 2 * L + L + l]);       // torch.exp in fp32, like the encoder's own
    const double wi = 1.0 / v;
    if (lane == 0) { mu[e] = m_; var[e] = v; w[e] = wi; muw[e] = m_ / v; }
    const double *kr = Kn + (size_t)i * m;
    double *ar = A + ((size_t)l * b + i) * m;
    for (int k = lane; k < m; k += 64) ar[k] = kr[k] * wi;
}

// The small products after the inverse, all latent dimensions at once (they were five library launches):
//   mid1: r_l = S_l t_l and the row parts of <S_l, M>            (one wave per row of S_l)
//   mid2: Mr_l = M r_l, raw[:, l] = X2 r_l, sm_l = <S_l, M>       (one wave per row of M / X2)
__global__ __launch_bounds__(256) void k_svgp_mid1(const double *__restrict__ S, const double *__restrict__ t,
                                                   const double *__restrict__ M, int m, double *__restrict__ r,
                                                   double *__restrict__ smpart) {
    const int l = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    double ar = 0.0, as = 0.0;
    if (i < m) {
        const double *srow = S + ((size_t)l * m + i) * m, *mrow = M + (size_t)i * m, *tl = t + (size_t)l * m;
#pragma unroll 4
        for (int j = lane; j < m; j += 64) {
            const double sv = srow[j];
            ar = fma(sv, tl[j], ar);
            as = fma(sv, mrow[j], as);
        }
    }
    ar = wave_sum_d(ar); as = wave_sum_d(as);
    if (lane == 0) {
        if (i < m) r[(size_t)l * m + i] = ar;
        smpart[(size_t)l * gridDim.x * 4 + blockIdx.x * 4 + (threadIdx.x >> 6)] = as;      // 0 for the rows past m
    }
}
__global__ __launch_bounds__(256) void k_svgp_mid2(const double *__restrict__ M, const double *__restrict__ X2,
                                                   const double *__restrict__ r, const double *__restrict__ smpart,
                                                   int nparts, int m, int rows2, int L, double *__restrict__ Mr,
                                                   double *__restrict__ raw, double *__restrict__ sm) {
    const int l = blockIdx.y, q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const double *rl = r + (size_t)l * m;
    if (q < m + rows2) {
        const double *row = q < m ? M + (size_t)q * m : X2 + (size_t)(q - m) * m;
        double acc = 0.0;
#pragma unroll 4
        for (int j = lane; j < m; j += 64) acc = fma(row[j], rl[j], acc);
        acc = wave_sum_d(acc);
        if (lane == 0) {
            if (q < m) Mr[(size_t)l * m + q] = acc;
            else raw[(size_t)(q - m) * L + l] = acc;
        }
    }
    if (blockIdx.x == 0 && (threadIdx.x >> 6) == 0) {
        double a = 0.0;
        for (int k = lane; k < nparts; k += 64) a += smpart[(size_t)l * nparts + k];
        a = wave_sum_d(a);
        if (lane == 0) sm[l] = a;
    }
}

__global__ __launch_bounds__(256) void k_svgp_pre(const float *__restrict__ z, int b, int L, double *__restrict__ mu,
                                                  double *__restrict__ var, double *__restrict__ w,
                                                  double *__restrict__ muw) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= b * L) return;
    const int i = e / L, l = e - i * L;
    const double m_ = (double)z[(size_t)i * 2 * L + l];
    const double v = (double)expf(z[(size_t)i * 2 * L + L + l]);       // torch.exp in fp32, like the encoder's own
    mu[e] = m_; var[e] = v; w[e] = 1.0 / v; muw[e] = m_ / v;
}

// Last step of the algebra's backward: q1 = diag(K_nm S D S K_mn) [L, b], q2 = diag(K_nm S2 K_mn) [L, b],
// Kdt = K_nm dt [b, L]:  dw = c (g_kl/2 (p_v - k~ - q2) - q1) + (mu - p_m) Kdt,  dmu = w Kdt + g_mu,  dvar = -dw w^2 + g_var.
__global__ __launch_bounds__(256) void k_svgp_grad_tail(const double *__restrict__ q1, const double *__restrict__ q2,
                                                        const double *__restrict__ Kdt, const double *__restrict__ pv,
                                                        const double *__restrict__ kt, const double *__restrict__ pm,
                                                        const double *__restrict__ mu, const double *__restrict__ w,
                                                        const double *__restrict__ g_kl, const double *__restrict__ g_mu,
                                                        const double *__restrict__ g_var, int b, int L, double c,
                                                        double *__restrict__ dmu, double *__restrict__ dvar,
                                                        float *__restrict__ dz) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= b * L) return;
    const int i = e / L, l = e - i * L;
    const double g = g_kl[0], ww = w[e], kd = Kdt[e];
    const double dw = c * (0.5 * g * (pv[e] - kt[i] - q2[(size_t)l * b + i]) - q1[(size_t)l * b + i]) + (mu[e] - pm[e]) * kd;
    const double dm = ww * kd + g_mu[e], dv = -dw * ww * ww + g_var[e];
    if (dmu) { dmu[e] = dm; dvar[e] = dv; }
    if (dz) {                                     // gradient w.r.t. (mu | logvar): d/dlogvar = d/dvar * var
        dz[(size_t)i * 2 * L + l] = (float)dm;
        dz[(size_t)i * 2 * L + L + l] = (float)(dv / ww);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_elbo_bwd(const T *g2, const T *mu, const T *var, const T *mv,
                                                  const T *tr, const T *pm, const T *pv, const T *kt, int b,
                                                  int L, T *g_mu, T *g_var, T *g_mv, T *g_tr, T *g_pm,
                                                  T *g_pv) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= b * L) return;
    const int i = e / L;
    const double gl = -0.5 * (double)g2[0], gc = -0.5 * (double)g2[1];
    const double v = var[e], m_ = mu[e], d = m_ - (double)mv[e], p = pm[e];
    const double q = (double)pv[e] + p * p - 2.0 * p * m_ + m_ * m_;
    const double a3 = (double)kt[i] + (double)tr[e];
    g_mu[e] = (T)(gl * (2.0 * d / v) + gc * ((2.0 * m_ - 2.0 * p) / v));
    g_var[e] = (T)(gl * (-a3 / (v * v) + 1.0 / v - d * d / (v * v)) + gc * (1.0 / v - q / (v * v)));
    g_mv[e] = (T)(gl * (-2.0 * d / v));
    g_tr[e] = (T)(gl / v);
    g_pm[e] = (T)(gc * ((2.0 * p - 2.0 * m_) / v));
    g_pv[e] = (T)(gc / v);
}

// sum of squared differences, two-stage
template <typename T>
__global__ __launch_bounds__(256) void k_sqerr_part(const T *__restrict__ y, const T *__restrict__ yh,
                                                    long long count, double *__restrict__ part) {
    __shared__ double sh[16];
    double acc = 0.0;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < count; k += (long long)gridDim.x * 256) {
        const double d = (double)y[k] - (double)yh[k];
        acc += d * d;
    }
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
template <typename T>
__global__ __launch_bounds__(1024) void k_final_sum(const double *__restrict__ part, int nparts, double scale,
                                                    T *__restrict__ out) {
    __shared__ double sh[16];
    double acc = 0.0;
    for (int k = threadIdx.x; k < nparts; k += blockDim.x) acc += part[k];
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) out[0] = (T)(acc * scale);
}
template <typename T>
__global__ __launch_bounds__(256) void k_sqerr_bwd(const T *g1, const T *__restrict__ y,
                                                   const T *__restrict__ yh, long long count, double inv_scale,
                                                   T *__restrict__ gy) {
    const double c = -2.0 * inv_scale * (double)g1[0];
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < count; k += (long long)gridDim.x * 256)
        gy[k] = (T)(c * ((double)y[k] - (double)yh[k]));
}

template <typename T>
__global__ __launch_bounds__(256) void k_kmeans_assign(const T *__restrict__ x, const T *__restrict__ cen,
                                                       int n, int kc, int d, int *__restrict__ labels) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double best = INFINITY;
    int arg = 0;
    for (int c = 0; c < kc; c++) {
        double s = 0.0;
        for (int k = 0; k < d; k++) {
            const double t = (double)x[(size_t)i * d + k] - (double)cen[(size_t)c * d + k];
            s += t * t;
        }
        if (s < best) { best = s; arg = c; }
    }
    labels[i] = arg;
}

// ------------------------------------------------------------------------------------------
// Exact k nearest neighbours by brute force (spatial graph construction, _utils.py:52-100): one thread per query
// point, candidates streamed through LDS in tiles of 256, the running k-best list of every thread in LDS
// ([slot][thread]: conflict-free), ordered by (squared distance in fp64, index).  out [n, kk] int32, self included.
// ------------------------------------------------------------------------------------------
constexpr int KNN_T = 256, KNN_MAXD = 4;
__global__ __launch_bounds__(KNN_T) void k_knn(const double *__restrict__ x, int n, int d, int kk,
                                               int *__restrict__ out) {
    extern __shared__ double knn_sh[];
    double *tile = knn_sh;                                   // [KNN_T][d] candidate coordinates
    double *bd = knn_sh + KNN_T * KNN_MAXD;                  // [kk][KNN_T] best distances
    int *bi = (int *)(bd + (size_t)kk * KNN_T);              // [kk][KNN_T] best indices
    const int t = threadIdx.x, i = blockIdx.x * KNN_T + t;
    double q[KNN_MAXD];
    for (int c = 0; c < KNN_MAXD; c++) q[c] = (i < n && c < d) ? x[(size_t)i * d + c] : 0.0;
    for (int s = 0; s < kk; s++) { bd[s * KNN_T + t] = INFINITY; bi[s * KNN_T + t] = 0x7fffffff; }
    double worst = INFINITY;
    int worst_i = 0x7fffffff;
    for (int j0 = 0; j0 < n; j0 += KNN_T) {
        __syncthreads();
        for (int e = t; e < KNN_T * d; e += KNN_T) {
            const int jj = j0 + e / d;
            tile[e] = jj < n ? x[(size_t)j0 * d + e] : 0.0;
        }
        __syncthreads();
        const int cnt = min(KNN_T, n - j0);
        if (i < n)
            for (int u = 0; u < cnt; u++) {
                double dist = 0.0;
                for (int c = 0; c < d; c++) { const double df = q[c] - tile[u * d + c]; dist += df * df; }
                const int j = j0 + u;
                if (dist < worst || (dist == worst && j < worst_i)) {
                    int pos = kk - 1;                                   // the worst entry drops out
                    while (pos > 0) {
                        const double pd = bd[(pos - 1) * KNN_T + t];
                        const int pi = bi[(pos - 1) * KNN_T + t];
                        if (pd < dist || (pd == dist && pi < j)) break;
                        bd[pos * KNN_T + t] = pd; bi[pos * KNN_T + t] = pi;
                        pos--;
                    }
                    bd[pos * KNN_T + t] = dist; bi[pos * KNN_T + t] = j;
                    worst = bd[(kk - 1) * KNN_T + t]; worst_i = bi[(kk - 1) * KNN_T + t];
                }
            }
    }
    if (i < n)
        for (int s = 0; s < kk; s++) out[(size_t)i * kk + s] = bi[s * KNN_T + t];
}

// ------------------------------------------------------------------------------------------
// Small fp32 products of the MLP stages (b x 256 -> 64 -> 20 and their gradients: a few MFLOP each) with a SMALL
// FOOTPRINT: 256 threads, 8.4 KB of LDS, ~40 registers.  The library runs some of these shapes with 256 x 64 macro tiles
// (80 KB of LDS, a quarter of a compute unit's registers per wave): eight such workgroups on the side stream waited
// 150-185 us for a whole compute unit to drain beside the first GAT layer's weight-gradient GEMM, and the optimizer
// waited for them (rocprofv3 timeline, round 3).  These tiles slot in wherever four waves fit.
//   C [M x N] = sum_k a(m, k) b(k, n) (+ bias[n]),  32 x 32 tile per workgroup, thread = 2 x 2 outputs, K in steps of 32:
//   MODE 0 (NN): a = A[m, k], b = B[k, n]      dx = g W
//   MODE 1 (NT): a = A[m, k], b = B[n, k]      y = x W^T (+ bias)
//   MODE 2 (TN): a = A[k, m], b = B[k, n]      dW = g^T x        (fixed summation order: k ascending)
// ------------------------------------------------------------------------------------------
// blockIdx.z = batch entry (operands and result advance by their batch strides): a long contraction is cut into slices
// whose partial results the caller adds in slice order.
template <int MODE>
__global__ __launch_bounds__(256) void k_sgemm_small(const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb,
                                                     float *__restrict__ C, int ldc, int M, int N, int K,
                                                     const float *__restrict__ bias, long long sA, long long sB, long long sC) {
    __shared__ float As[32][33], Bs[32][33];          // As[k][m], Bs[k][n]
    A += (size_t)blockIdx.z * sA; B += (size_t)blockIdx.z * sB; C += (size_t)blockIdx.z * sC;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const int lr = t >> 5, lc = t & 31;               // loader: rows lr + 8 r (r = 0..3), column lc (the contiguous index)
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    for (int k0 = 0; k0 < K; k0 += 32) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = lr + 8 * r;
            if (MODE == 2) {          // A[k, m]: m contiguous
                const int k = k0 + row, m = m0 + lc;
                As[row][lc] = (k < K && m < M) ? A[(size_t)k * lda + m] : 0.f;
            } else {                  // A[m, k]: k contiguous
                const int m = m0 + row, k = k0 + lc;
                As[lc][row] = (m < M && k < K) ? A[(size_t)m * lda + k] : 0.f;
            }
            if (MODE == 1) {          // B[n, k]: k contiguous
                const int n = n0 + row, k = k0 + lc;
                Bs[lc][row] = (n < N && k < K) ? B[(size_t)n * ldb + k] : 0.f;
            } else {                  // B[k, n]: n contiguous
                const int k = k0 + row, n = n0 + lc;
                Bs[row][lc] = (k < K && n < N) ? B[(size_t)k * ldb + n] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 32; k++) {
            const float a0 = As[k][2 * ty], a1 = As[k][2 * ty + 1];
            const float b0 = Bs[k][2 * tx], b1 = Bs[k][2 * tx + 1];
            acc[0][0] = fmaf(a0, b0, acc[0][0]); acc[0][1] = fmaf(a0, b1, acc[0][1]);
            acc[1][0] = fmaf(a1, b0, acc[1][0]); acc[1][1] = fmaf(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int m = m0 + 2 * ty + i, n = n0 + 2 * tx + j;
            if (m < M && n < N) C[(size_t)m * ldc + n] = acc[i][j] + (bias ? bias[n] : 0.f);
        }
}


// One device timestamp (constant-rate 100 MHz counter) into buf[slot]: a one-thread launch placed at the head and the end
// of a captured stage gives the stage's start / end on the GPU without a profiler attached (tools/stage_stamps.py).
__global__ void k_stamp(unsigned long long *buf, int slot) {
    if (threadIdx.x == 0) buf[slot] = wall_clock64();
}

// ------------------------------------------------------------------------------------------
// Lloyd iterations of K-means for R restarts at once (fp64, deterministic: no atomics).  Restart r belongs to data set
// rgrp[r] (rows xoff[g] .. xoff[g] + npts[g] - 1 of X) and has its own cluster count Kr[r] <= K; K is the padding of
// C [R, K, D] and of the partial-sum slots, and the grid is sized by the largest set (chunks past a set's end return at once).
//   k_lloyd_assign: block = (restart r, chunk of 256 points): nearest centre per point (first minimum wins),
//                   per-block cluster sums / counts / inertia in a fixed order -> part[r][chunk][K*(D+1) + 1]
//   k_lloyd_update: block = restart: partials summed in chunk order, centres moved (empty cluster: kept), squared
//                   shift compared with tol[g], `done` restarts frozen.
// Each restart loops over its own Kr[r] clusters only, so its arithmetic does not depend on the other restarts of the launch.
// ------------------------------------------------------------------------------------------
constexpr int LL_PTS = 256, LL_MAXK = 32, LL_MAXD = 32;
__global__ __launch_bounds__(LL_PTS) void k_lloyd_assign(const double *__restrict__ X, const double *__restrict__ C,
                                                         int D, int K, double *__restrict__ part,
                                                         const int *__restrict__ xoff, const int *__restrict__ npts,
                                                         const int *__restrict__ skip_done,
                                                         const int *__restrict__ Kr, const int *__restrict__ rgrp) {
    extern __shared__ double ll_dyn[];           // K*D centres, then 256*D point coordinates
    double *s_c = ll_dyn, *s_x = ll_dyn + (size_t)K * D;
    __shared__ int s_lab[LL_PTS];
    __shared__ double s_red[16];
    const int r = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    const int i = chunk * LL_PTS + t;
    const int nchunk = gridDim.x;
    if (skip_done != nullptr && skip_done[r] != 0) return;      // a restart that has converged: nothing reads its partials again
    const int g = rgrp[r], n = npts[g];
    X += (size_t)xoff[g] * D;
    if (chunk * LL_PTS >= n) return;            // (uniform for the workgroup)
    const int Kl = min(Kr[r], K);               // this restart's cluster count; K is the padded stride
    for (int e = t; e < Kl * D; e += LL_PTS) s_c[e] = C[(size_t)r * K * D + e];
    const int rows = min(LL_PTS, n - chunk * LL_PTS);
#pragma unroll 4
    for (int e = t; e < rows * D; e += LL_PTS) s_x[e] = X[(size_t)chunk * LL_PTS * D + e];
    __syncthreads();
    double best = INFINITY;
    int arg = -1;
    if (i < n) {
        for (int k = 0; k < Kl; k++) {
            double d2 = 0.0;
#pragma unroll 4
            for (int c = 0; c < D; c++) { const double df = s_x[t * D + c] - s_c[k * D + c]; d2 += df * df; }
            if (d2 < best) { best = d2; arg = k; }
        }
    }
    s_lab[t] = arg;
    const double inertia = block_sum_d(i < n ? best : 0.0, s_red);       // (includes the barrier after s_lab)
    double *out = part + ((size_t)r * nchunk + chunk) * ((size_t)K * (D + 1) + 1);
    for (int pq = t; pq < Kl * (D + 1); pq += LL_PTS) {
        const int k = pq / (D + 1), c = pq - k * (D + 1);
        double acc = 0.0;
#pragma unroll 8
        for (int u = 0; u < LL_PTS; u++) {
            const bool hit = s_lab[u] == k;
            acc += hit ? (c < D ? s_x[(u < rows ? u : 0) * D + c] : 1.0) : 0.0;
        }
        out[pq] = acc;
    }
    if (t == 0) out[(size_t)K * (D + 1)] = inertia;
}

__global__ __launch_bounds__(256) void k_lloyd_update(const double *__restrict__ part, int slots, int D, int K,
                                                      double *__restrict__ C, int *__restrict__ done,
                                                      double *__restrict__ inertia, const int *__restrict__ npts,
                                                      const double *__restrict__ tolv, int skip_done,
                                                      const int *__restrict__ Kr, const int *__restrict__ rgrp) {
    __shared__ double s_new[LL_MAXK * (LL_MAXD + 1)];
    __shared__ double s_red[16];
    const int r = blockIdx.x, t = threadIdx.x;
    if (skip_done && done[r] != 0) return;       // frozen: centres and inertia stay (the caller measures the final inertia with skip_done = 0)
    const size_t stride = (size_t)K * (D + 1) + 1;
    const int g = rgrp[r];
    const int nchunk = (npts[g] + LL_PTS - 1) / LL_PTS;     // this set's chunks of the `slots` per restart
    const double tol = tolv[g];
    const int Kl = min(Kr[r], K);
    for (int pq = t; pq < Kl * (D + 1); pq += 256) {
        double acc = 0.0;
        for (int ch = 0; ch < nchunk; ch++) acc += part[((size_t)r * slots + ch) * stride + pq];
        s_new[pq] = acc;
    }
    double in = 0.0;
    for (int ch = t; ch < nchunk; ch += 256) in += part[((size_t)r * slots + ch) * stride + K * (D + 1)];
    in = block_sum_d(in, s_red);
    __syncthreads();
    double sh = 0.0;
    const bool frozen = done[r] != 0;
    for (int e = t; e < Kl * D; e += 256) {
        const int k = e / D, c = e - k * D;
        const double cnt = s_new[k * (D + 1) + D], old = C[(size_t)r * K * D + e];
        const double nw = cnt > 0.0 ? s_new[k * (D + 1) + c] / cnt : old;
        sh += (nw - old) * (nw - old);
        if (!frozen) C[(size_t)r * K * D + e] = nw;
    }
    sh = block_sum_d(sh, s_red);
    if (t == 0) {
        inertia[r] = in;                     // inertia of the centres this iteration STARTED from
        if (!frozen && sh <= tol) done[r] = 1;
    }
}

// ------------------------------------------------------------------------------------------
// k-means++ seeding for many problems in one launch (every (data set, k, restart) triple of a plan of spadot_amd.kmeans is a
// problem).  Block = problem p: the k - 1 selection rounds of sklearn's k-means++ rule (2 + int(log k) candidates drawn by
// potential, the one with the smallest new potential wins, first minimum on ties; the torch rounds of kmeans._Plan state
// the same rule for small plans).  closest [n] lives
// in a global work space row (it outgrows LDS at 50 000 points).  Per round:
//   1. thread t owns the contiguous segment [t*seg, (t+1)*seg) of closest: its segment total, then a fixed-order
//      (Hillis-Steele) scan of the 256 totals gives each segment's base;
//   2. searchsorted (side left) of every draw u * pot: the thread walks its segment with a running sum from its base, the
//      first index whose prefix is >= the draw is kept, the block minimum of those (an integer: order-free) is the
//      candidate, clamped to n - 1;
//   3. each candidate's potential sum_i min(closest_i, |x_i - c|^2), distance in the expanded form xsq - 2 x.c + csq
//      clamped at 0 (the torch path's form), summed in a fixed order (block_sum_d);
//   4. closest updated with the best candidate's distances (recomputed by the same function: the same bits).
// No atomics on floating-point data: two runs are bitwise identical.  The prefix sums round in a different order from
// torch.cumsum, so a candidate index can differ from the torch path's only when a draw lies within rounding distance of
// a prefix boundary.
constexpr int KPP_T = 256, KPP_MAXTR = 8;

__device__ __forceinline__ int kpp_trials(int K) {      // 2 + int(log K) for 1 <= K <= 32 (e, e^2, e^3 = 2.72, 7.39, 20.09)
    return 2 + (K >= 3) + (K >= 8) + (K >= 21);
}

__device__ __forceinline__ double kpp_d2(const double *__restrict__ xr, const double *c, double csq, int D) {
    double xsq = 0.0, dot = 0.0;
    for (int e = 0; e < D; e++) { const double v = xr[e]; xsq += v * v; dot += v * c[e]; }
    return fmax(xsq - 2.0 * dot + csq, 0.0);
}

__global__ __launch_bounds__(KPP_T) void k_kmeanspp_seed(const double *__restrict__ X, const int *__restrict__ xoff,
                                                         const int *__restrict__ npts, int D, const int *__restrict__ pset,
                                                         const int *__restrict__ pK, const int *__restrict__ pfirst,
                                                         const int *__restrict__ puoff, const double *__restrict__ U, int K_max,
                                                         int n_max, double *__restrict__ closest, int *__restrict__ idx,
                                                         double *__restrict__ centers) {
    __shared__ double s_c[KPP_MAXTR * LL_MAXD];     // candidate rows (round 0: the first centre)
    __shared__ double s_csq[KPP_MAXTR];
    __shared__ double s_scan[KPP_T];
    __shared__ double s_red[16];
    __shared__ int s_cand[KPP_MAXTR];
    const int p = blockIdx.x, t = threadIdx.x;
    const int g = pset[p], K = pK[p], n = npts[g], first = pfirst[p];
    int *ip = idx + (size_t)p * K_max;
    double *cp = centers + (size_t)p * K_max * D;
    for (int e = t; e < K_max; e += KPP_T) ip[e] = -1;                       // padding rows (and failed problems)
    for (int e = t; e < K_max * D; e += KPP_T) cp[e] = 0.0;
    if (K < 1 || K > K_max || n < 1 || n > n_max || first < 0 || first >= n) return;     // (uniform for the workgroup)
    const double *Xg = X + (size_t)xoff[g] * D;
    double *cl = closest + (size_t)p * n_max;
    const double *Up = U + puoff[p];
    const int trials = kpp_trials(K);
    const int seg = (n + KPP_T - 1) / KPP_T, lo = min(t * seg, n), hi = min(lo + seg, n);

    for (int e = t; e < D; e += KPP_T) s_c[e] = Xg[(size_t)first * D + e];
    __syncthreads();
    if (t == 0) {
        double q = 0.0;
        for (int e = 0; e < D; e++) q += s_c[e] * s_c[e];
        s_csq[0] = q;
        ip[0] = first;
    }
    for (int e = t; e < D; e += KPP_T) cp[e] = s_c[e];
    __syncthreads();
    double acc = 0.0;
    for (int i = t; i < n; i += KPP_T) {
        const double d = kpp_d2(Xg + (size_t)i * D, s_c, s_csq[0], D);
        cl[i] = d;
        acc += d;
    }
    double pot = block_sum_d(acc, s_red);
    __syncthreads();                                 // (closest written by all threads before the segment walks)

    for (int c = 1; c < K; c++) {
        if (t < KPP_MAXTR) s_cand[t] = INT_MAX;
        double ssum = 0.0;
        for (int i = lo; i < hi; i++) ssum += cl[i];
        s_scan[t] = ssum;
        __syncthreads();
        for (int off = 1; off < KPP_T; off <<= 1) {                      // inclusive scan of the segment totals
            const double v = t >= off ? s_scan[t - off] : 0.0;
            __syncthreads();
            s_scan[t] += v;
            __syncthreads();
        }
        double run = t > 0 ? s_scan[t - 1] : 0.0;
        double rv[KPP_MAXTR];
        int found[KPP_MAXTR];
#pragma unroll
        for (int j = 0; j < KPP_MAXTR; j++) {
            rv[j] = j < trials ? Up[(size_t)(c - 1) * trials + j] * pot : 0.0;
            found[j] = INT_MAX;
        }
        for (int i = lo; i < hi; i++) {
            run += cl[i];
#pragma unroll
            for (int j = 0; j < KPP_MAXTR; j++)
                if (j < trials && found[j] == INT_MAX && run >= rv[j]) found[j] = i;
        }
#pragma unroll
        for (int j = 0; j < KPP_MAXTR; j++)
            if (j < trials && found[j] != INT_MAX) atomicMin(&s_cand[j], found[j]);
        __syncthreads();
        for (int e = t; e < trials * D; e += KPP_T) {
            const int j = e / D;
            s_c[e] = Xg[(size_t)min(s_cand[j], n - 1) * D + (e - j * D)];
        }
        __syncthreads();
        if (t < trials) {
            double q = 0.0;
            for (int e = 0; e < D; e++) q += s_c[t * D + e] * s_c[t * D + e];
            s_csq[t] = q;
        }
        __syncthreads();
        double lp[KPP_MAXTR];
#pragma unroll
        for (int j = 0; j < KPP_MAXTR; j++) lp[j] = 0.0;
        for (int i = t; i < n; i += KPP_T) {
            const double ci = cl[i];
            const double *xr = Xg + (size_t)i * D;
#pragma unroll
            for (int j = 0; j < KPP_MAXTR; j++)
                if (j < trials) lp[j] += fmin(kpp_d2(xr, s_c + j * D, s_csq[j], D), ci);
        }
        int best = 0;
        double bpot = 0.0;
#pragma unroll
        for (int j = 0; j < KPP_MAXTR; j++) {
            if (j < trials) {
                const double pj = block_sum_d(lp[j], s_red);
                if (j == 0 || pj < bpot) { bpot = pj; best = j; }
            }
        }
        pot = bpot;
        const double *cb = s_c + best * D;
        const double csqb = s_csq[best];
        for (int i = t; i < n; i += KPP_T) cl[i] = fmin(cl[i], kpp_d2(Xg + (size_t)i * D, cb, csqb, D));
        for (int e = t; e < D; e += KPP_T) cp[(size_t)c * D + e] = cb[e];
        if (t == 0) ip[c] = min(s_cand[best], n - 1);
        __syncthreads();                             // closest, s_c and s_cand are reused by the next round
    }
}

__global__ __launch_bounds__(256) void k_sumsq_part(const float *__restrict__ g, long long count,
                                                    double *__restrict__ part) {
    __shared__ double sh[16];
    double acc = 0.0;
    const long long n4 = count / 4;
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n4; k += (long long)gridDim.x * 256) {
        const float4 v = g4[k];
        acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
    if (blockIdx.x == 0)
        for (long long k = n4 * 4 + threadIdx.x; k < count; k += 256) acc += (double)g[k] * g[k];
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// Gradient sum of squares in ONE launch: per-workgroup partials, and the last workgroup to finish (device counter,
// reset for the next launch) adds them in workgroup order, writes the total and advances the optimizer's step count.
template <int U>
__global__ __launch_bounds__(256) void k_sumsq_last(const float *__restrict__ g, long long count, double *__restrict__ part,
                                                    float *__restrict__ sumsq, int *__restrict__ step_dev,
                                                    unsigned *__restrict__ counter) {
    __shared__ double sh[16];
    __shared__ bool last;
    double acc = 0.0;
    const long long n4 = count / 4;
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    // U independent 16-byte loads in flight per thread, fp64 accumulation in a fixed order
    const long long stride = (long long)gridDim.x * 256;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n4; k += U * stride) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            v[u] = (k + u * stride < n4) ? g4[k + u * stride] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < U; u++)
            acc += ((double)v[u].x * v[u].x + (double)v[u].y * v[u].y) + ((double)v[u].z * v[u].z + (double)v[u].w * v[u].w);
    }
    if (blockIdx.x == 0)
        for (long long k = n4 * 4 + threadIdx.x; k < count; k += 256) acc += (double)g[k] * g[k];
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = acc;
        __threadfence();
        last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double t = 0.0;
    {   // gridDim.x <= 2048 (launcher): at most eight partials per thread, loaded together, added in a fixed order
        double q[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int b = threadIdx.x + u * 256;
            q[u] = b < (int)gridDim.x ? __builtin_nontemporal_load(part + b) : 0.0;
        }
        t = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
    t = block_sum_d(t, sh);
    if (threadIdx.x == 0) { sumsq[0] = (float)t; if (step_dev) step_dev[0] += 1; *counter = 0u; }
}

__global__ void k_step_inc(int *step) { step[0] += 1; }

// The same sum as two launches: per-workgroup partials (no cross-workgroup hand-over, so any number of workgroups), then one
// workgroup adds them in order and advances the step count.  k_sumsq_last's hand-over needs a device-scope release per
// workgroup, which writes the XCD's L2 back -- right behind the backward pass that has just filled it with dirty gradient lines.
template <int U>
__global__ __launch_bounds__(256) void k_sumsq_part_u(const float *__restrict__ g, long long count, double *__restrict__ part) {
    __shared__ double sh[16];
    double acc = 0.0;
    const long long n4 = count / 4;
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    const long long stride = (long long)gridDim.x * 256;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n4; k += U * stride) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            v[u] = (k + u * stride < n4) ? g4[k + u * stride] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < U; u++)
            acc += ((double)v[u].x * v[u].x + (double)v[u].y * v[u].y) + ((double)v[u].z * v[u].z + (double)v[u].w * v[u].w);
    }
    if (blockIdx.x == 0)
        for (long long k = n4 * 4 + threadIdx.x; k < count; k += 256) acc += (double)g[k] * g[k];
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
__global__ __launch_bounds__(1024) void k_final_sum_step(const double *__restrict__ part, int nparts, float *__restrict__ out,
                                                         int *__restrict__ step_dev) {
    __shared__ double sh[16];
    double acc = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 1024) acc += part[k];
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) { out[0] = (float)acc; if (step_dev) step_dev[0] += 1; }
}

// One element of clip + AdamW.  Contraction into fused multiply-adds is switched OFF here so that every kernel that
// inlines this function (the scalar and the four-wide, image-writing form) performs the same roundings whatever the
// compiler makes of the code around it: their parameters stay bit-identical.
__device__ __forceinline__ void adamw_element(float g_, float &pp, float &mm, float &vv, float coef, float lr, float wd,
                                              float b1, float b2, float eps, float bc1, float bc2_sqrt) {
#pragma clang fp contract(off)
    const float gg = g_ * coef;
    float pn = pp * (1.f - lr * wd);
    const float mn = mm + (gg - mm) * (1.f - b1);          // lerp_(grad, 1 - beta1)
    const float vn = vv * b2 + gg * gg * (1.f - b2);
    const float denom = sqrtf(vn) / bc2_sqrt + eps;
    pn -= (lr / bc1) * (mn / denom);
    pp = pn; mm = mn; vv = vn;
}

// clip coefficient (times grad_scale), same care: identical in every kernel that calls it
__device__ __forceinline__ float adamw_clip_coef(float sumsq, float gs, float max_norm) {
#pragma clang fp contract(off)
    const float total = sqrtf(sumsq) * gs;
    return fminf(1.f, max_norm / (total + 1e-6f)) * gs;
}

__global__ __launch_bounds__(256) void k_adamw(float *__restrict__ p, const float *__restrict__ g,
                                               float *__restrict__ m, float *__restrict__ v,
                                               const float *__restrict__ sumsq, long long count, float lr,
                                               float b1, float b2, float eps, float wd, float max_norm,
                                               float bc1, float bc2_sqrt, const int *__restrict__ step_dev,
                                               const float *__restrict__ grad_scale) {
    if (step_dev) {   // step count lives on the device (hipGraph replays): bias corrections computed here
        const double t = (double)step_dev[0];
        bc1 = (float)(1.0 - pow((double)b1, t));
        bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, t));
    }
    // grad_scale (device scalar, optional): the buffer holds a SUM over replicas and stands for scale * g
    // (data-parallel steps: 1 / number of replicas that had a batch); the norm is clipped on the scaled gradient
    const float gs = grad_scale ? grad_scale[0] : 1.f;
    const float coef = adamw_clip_coef(sumsq[0], gs, max_norm);
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < count; k += (long long)gridDim.x * 256) {
        float pp = p[k], mm = m[k], vv = v[k];
        adamw_element(g[k], pp, mm, vv, coef, lr, wd, b1, b2, eps, bc1, bc2_sqrt);
        p[k] = pp; m[k] = mm; v[k] = vv;
    }
}

// The same update, four elements per thread (16-byte streams), which also keeps the bf16 IMAGES of registered weight
// matrices current: the dense maps of the GAT layers read W as a bf16 [rows x Kp] image (K zero-padded to Kp); casting
// the three of them took a 15-24 us launch at the head of every step's critical path.  The update already holds the new
// fp32 value in a register, so it stores the rounded copy too (2 more bytes per parameter on a ~450 MB pass).
// Segments start at multiples of 4 elements and K % 4 == 0, so the four elements of a thread lie in one row of one image.
// The arithmetic per element is k_adamw's, operation for operation.
__global__ __launch_bounds__(256) void k_adamw_img(float *__restrict__ p, const float *__restrict__ g,
                                                   float *__restrict__ m, float *__restrict__ v,
                                                   const float *__restrict__ sumsq, long long count, float lr,
                                                   float b1, float b2, float eps, float wd, float max_norm,
                                                   const int *__restrict__ step_dev, const float *__restrict__ grad_scale,
                                                   spadot_weight_images imgs, long long base) {
    // base: index of p[0] in the flat buffer the image offsets refer to (a launch over a sub-range of it)
    const double t = (double)step_dev[0];
    const float bc1 = (float)(1.0 - pow((double)b1, t));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, t));
    const float gs = grad_scale ? grad_scale[0] : 1.f;
    const float coef = adamw_clip_coef(sumsq[0], gs, max_norm);
    const long long n4 = count >> 2;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long long)gridDim.x * 256) {
        const long long k = q << 2;
        const float4 g4 = *reinterpret_cast<const float4 *>(g + k);
        const float4 p4 = *reinterpret_cast<const float4 *>(p + k);
        const float4 m4 = *reinterpret_cast<const float4 *>(m + k);
        const float4 v4 = *reinterpret_cast<const float4 *>(v + k);
        const float gi[4] = {g4.x, g4.y, g4.z, g4.w}, pi[4] = {p4.x, p4.y, p4.z, p4.w};
        const float mi[4] = {m4.x, m4.y, m4.z, m4.w}, vi[4] = {v4.x, v4.y, v4.z, v4.w};
        float po[4], mo[4], vo[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            po[e] = pi[e]; mo[e] = mi[e]; vo[e] = vi[e];
            adamw_element(gi[e], po[e], mo[e], vo[e], coef, lr, wd, b1, b2, eps, bc1, bc2_sqrt);
        }
        *reinterpret_cast<float4 *>(p + k) = make_float4(po[0], po[1], po[2], po[3]);
        *reinterpret_cast<float4 *>(m + k) = make_float4(mo[0], mo[1], mo[2], mo[3]);
        *reinterpret_cast<float4 *>(v + k) = make_float4(vo[0], vo[1], vo[2], vo[3]);
#pragma unroll
        for (int s_ = 0; s_ < 8; s_++) {
            if (s_ >= imgs.n) break;
            const spadot_weight_image W = imgs.w[s_];
            const unsigned long long d = (unsigned long long)(k + base - W.offset);
            if (d < (unsigned long long)W.rows * (unsigned long long)W.K) {
                const unsigned row = (unsigned)d / (unsigned)W.K;                    // (d < 2^31: checked on the host)
                const unsigned col = (unsigned)d - row * (unsigned)W.K;
                __bf16 *dst = reinterpret_cast<__bf16 *>(W.image) + (size_t)row * W.Kp + col;
                const unsigned lo = (unsigned)__builtin_bit_cast(unsigned short, (__bf16)po[0]) |
                                    ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)po[1]) << 16);
                const unsigned hi = (unsigned)__builtin_bit_cast(unsigned short, (__bf16)po[2]) |
                                    ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)po[3]) << 16);
                *reinterpret_cast<uint2 *>(dst) = make_uint2(lo, hi);
                break;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Small-MLP stages: BatchNorm1d (training) + LeakyReLU, LayerNorm + LeakyReLU, each ONE launch forward and one
// (LayerNorm: two) backward instead of the library's 4-5 and 3-4.  b rows <= a few thousand, F features <= 1024.
// ------------------------------------------------------------------------------------------
#ifndef BN_RG_DEF
#define BN_RG_DEF 16                                                 // (build define for A/B runs: 16 / 8 / 4 row lanes = 256 / 128 / 64 threads)
#endif
constexpr int BN_RPT = 512 / BN_RG_DEF;                              // rows a thread keeps in registers on the one-load path (b <= 512)
#ifndef BN_COLS_DEF
#define BN_COLS_DEF 16
#endif
constexpr int BN_COLS = BN_COLS_DEF, BN_RG = BN_RG_DEF, BN_NT = BN_COLS * BN_RG;      // 16 columns x 16 row lanes: 256-thread workgroups.  These
// launches run on the side stream beside the GAT branch's GEMMs, whose waves fill the register files: a new workgroup
// starts when a GEMM workgroup retires, and a 1024-thread one (64 row lanes, 30 % faster on an idle GPU) needs a whole
// compute unit to drain first -- it sat ~100 us in the queue (rocprofv3 timeline, profiles/r02).  Same box, same run
// (tools/ab_wgsize.sh): 479 steps/s with 64 row lanes, 494 with 16.
constexpr int LN_RG = 64, LN_NT = BN_COLS * LN_RG;                    // the LayerNorm column pass runs alone on the main stream

template <int RG = BN_RG>
__device__ __forceinline__ float bn_col_sum(float v, float (*sh)[BN_COLS + 1], int cl, int rg) {
    __syncthreads();
    sh[rg][cl] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll 8
    for (int g = 0; g < RG; g++) t += sh[g][cl];
    return t;
}

// y = leaky((x + lb - mean) invstd gamma + beta, slope); batch statistics over the b rows; running statistics
// updated like nn.BatchNorm1d (momentum, unbiased running variance); lb = bias of the preceding Linear or null.
template <typename TX>
__global__ __launch_bounds__(BN_NT) void k_bn_act_fwd(const TX *__restrict__ x, const float *__restrict__ lb,
                                                    const float *__restrict__ gamma, const float *__restrict__ beta,
                                                    float *__restrict__ run_mean, float *__restrict__ run_var,
                                                    long long *__restrict__ nbt, int b, int F, float momentum, float eps,
                                                    float slope, float *__restrict__ y, float *__restrict__ save_mean,
                                                    float *__restrict__ save_invstd) {
    __shared__ float sh[BN_RG][BN_COLS + 1];
    const int cl = threadIdx.x & (BN_COLS - 1), rg = threadIdx.x / BN_COLS;
    const int c = blockIdx.x * BN_COLS + cl;
    const bool on = c < F;
    const int c1 = min(c, F - 1);
    const float add_r = (lb ? lb : gamma)[c1];
    const float add = (on && lb) ? add_r : 0.f;
    if (b <= BN_RG * BN_RPT) {
        // up to 512 rows (the training batch): a thread's 32 rows are loaded ONCE, all loads in flight together, and the three
        // passes run out of registers -- the looped form below pays ~24 dependent memory latencies (18-33 us for 0.1-0.5 MB
        // beside the GAT branch's GEMM, at the head of the step's forward critical chain; rocprofv3 timeline, round 4).
        // Same values, same summation order: bit-identical to the looped form.
        // (UNCONDITIONAL loads from a clamped position, masked afterwards: a predicated load is a branch, and the compiler
        // drains the load queue at its join -- written as `(on && i < b) ? load : 0` these 32 loads were 32 round trips)
        float v[BN_RPT];
        const int cc = min(c, F - 1);
#pragma unroll
        for (int r = 0; r < BN_RPT; r++) v[r] = ld<TX>(x + (size_t)min(rg + r * BN_RG, b - 1) * F + cc);
        const float gam_r = gamma[cc], bet_r = beta[cc], rm_r = run_mean[cc], rv_r = run_var[cc];      // (ride with the rows)
#pragma unroll
        for (int r = 0; r < BN_RPT; r++) v[r] = (on && rg + r * BN_RG < b) ? v[r] + add : 0.f;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < BN_RPT; r++)
            if (rg + r * BN_RG < b) s += v[r];
        const float mean = bn_col_sum(s, sh, cl, rg) / (float)b;
        float ss = 0.f;
#pragma unroll
        for (int r = 0; r < BN_RPT; r++)
            if (rg + r * BN_RG < b) { const float d = v[r] - mean; ss += d * d; }
        const float var = bn_col_sum(ss, sh, cl, rg) / (float)b;
        const float invstd = rsqrtf(var + eps);
        if (on) {
            const float g = gam_r * invstd, o = bet_r;
#pragma unroll
            for (int r = 0; r < BN_RPT; r++) {
                const int i = rg + r * BN_RG;
                if (i < b) {
                    const float u = (v[r] - mean) * g + o;
                    y[(size_t)i * F + c] = u > 0.f ? u : slope * u;
                }
            }
            if (rg == 0) {
                save_mean[c] = mean; save_invstd[c] = invstd;
                run_mean[c] = (1.f - momentum) * rm_r + momentum * mean;
                run_var[c] = (1.f - momentum) * rv_r + momentum * var * ((float)b / (float)(b > 1 ? b - 1 : 1));
            }
        }
        if (nbt && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += 1;
        return;
    }
    float s = 0.f;
    if (on)
#pragma unroll 4
        for (int i = rg; i < b; i += BN_RG) s += ld<TX>(x + (size_t)i * F + c) + add;
    const float mean = bn_col_sum(s, sh, cl, rg) / (float)b;
    float ss = 0.f;
    if (on)
#pragma unroll 4
        for (int i = rg; i < b; i += BN_RG) { const float d = ld<TX>(x + (size_t)i * F + c) + add - mean; ss += d * d; }
    const float var = bn_col_sum(ss, sh, cl, rg) / (float)b;
    const float invstd = rsqrtf(var + eps);
    if (on) {
        const float g = gamma[c] * invstd, o = beta[c];
#pragma unroll 4
        for (int i = rg; i < b; i += BN_RG) {
            const float v = (ld<TX>(x + (size_t)i * F + c) + add - mean) * g + o;
            y[(size_t)i * F + c] = v > 0.f ? v : slope * v;
        }
        if (rg == 0) {
            save_mean[c] = mean; save_invstd[c] = invstd;
            run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mean;
            run_var[c] = (1.f - momentum) * run_var[c] + momentum * var * ((float)b / (float)(b > 1 ? b - 1 : 1));
        }
    }
    if (nbt && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += 1;
}

template <typename TX>
__global__ __launch_bounds__(BN_NT) void k_bn_act_bwd(const float *__restrict__ dy, const float *__restrict__ y,
                                                    const TX *__restrict__ x, const float *__restrict__ lb,
                                                    const float *__restrict__ gamma, const float *__restrict__ save_mean,
                                                    const float *__restrict__ save_invstd, int b, int F, float slope,
                                                    TX *__restrict__ dx, float *__restrict__ dgamma,
                                                    float *__restrict__ dbeta) {
    __shared__ float sh[BN_RG][BN_COLS + 1];
    const int cl = threadIdx.x & (BN_COLS - 1), rg = threadIdx.x / BN_COLS;
    const int c = blockIdx.x * BN_COLS + cl;
    const bool on = c < F;
    const int c1 = min(c, F - 1);
    const float add_r = (lb ? lb : gamma)[c1], mean_r = save_mean[c1], invstd_r = save_invstd[c1], gamma_r = gamma[c1];
    const float add = (on && lb) ? add_r : 0.f;
    const float mean = on ? mean_r : 0.f, invstd = on ? invstd_r : 0.f;
    if (b <= BN_RG * BN_RPT) {          // one load of the thread's rows, both passes out of registers (see k_bn_act_fwd)
        // unconditional loads from a clamped position, masked afterwards (see k_bn_act_fwd): 96 loads in three groups
        float dzv[BN_RPT], xh[BN_RPT];
        const int cc = min(c, F - 1);
#pragma unroll
        for (int r = 0; r < BN_RPT; r++) dzv[r] = dy[(size_t)min(rg + r * BN_RG, b - 1) * F + cc];
#pragma unroll
        for (int r = 0; r < BN_RPT; r++) {
            const float yv = y[(size_t)min(rg + r * BN_RG, b - 1) * F + cc];
            dzv[r] = (on && rg + r * BN_RG < b) ? dzv[r] * (yv > 0.f ? 1.f : slope) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < BN_RPT; r++) {
            const float xv = ld<TX>(x + (size_t)min(rg + r * BN_RG, b - 1) * F + cc);
            xh[r] = (xv + add - mean) * invstd;      // (rows past b: never summed, never stored)
        }
        float sb = 0.f, sg = 0.f;
#pragma unroll
        for (int r = 0; r < BN_RPT; r++)
            if (on && rg + r * BN_RG < b) { sb += dzv[r]; sg += dzv[r] * xh[r]; }
        sb = bn_col_sum(sb, sh, cl, rg);
        sg = bn_col_sum(sg, sh, cl, rg);
        if (on) {
            const float g = gamma_r * invstd, mb = sb / (float)b, mg = sg / (float)b;
#pragma unroll
            for (int r = 0; r < BN_RPT; r++) {
                const int i = rg + r * BN_RG;
                if (i < b) st<TX>(dx + (size_t)i * F + c, g * (dzv[r] - mb - xh[r] * mg));
            }
            if (rg == 0) { dgamma[c] = sg; dbeta[c] = sb; }
        }
        return;
    }
    float sb = 0.f, sg = 0.f;
    if (on)
#pragma unroll 4
        for (int i = rg; i < b; i += BN_RG) {
            const size_t e = (size_t)i * F + c;
            const float dz = dy[e] * (y[e] > 0.f ? 1.f : slope);
            sb += dz;
            sg += dz * (ld<TX>(x + e) + add - mean) * invstd;
        }
    sb = bn_col_sum(sb, sh, cl, rg);
    sg = bn_col_sum(sg, sh, cl, rg);
    if (on) {
        const float g = gamma[c] * invstd, mb = sb / (float)b, mg = sg / (float)b;
#pragma unroll 4
        for (int i = rg; i < b; i += BN_RG) {
            const size_t e = (size_t)i * F + c;
            const float dz = dy[e] * (y[e] > 0.f ? 1.f : slope);
            const float xh = (ld<TX>(x + e) + add - mean) * invstd;
            st<TX>(dx + e, g * (dz - mb - xh * mg));
        }
        if (rg == 0) { dgamma[c] = sg; dbeta[c] = sb; }
    }
}

// LayerNorm over the F features of a row + LeakyReLU: one wave per row.
__global__ __launch_bounds__(256) void k_ln_act_fwd(const float *__restrict__ x, const float *__restrict__ gamma,
                                                    const float *__restrict__ beta, int b, int F, float eps, float slope,
                                                    float *__restrict__ y, float *__restrict__ save_mean,
                                                    float *__restrict__ save_invstd) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= b) return;
    const float *xr = x + (size_t)i * F;
    float s = 0.f;
    for (int c = lane; c < F; c += WAVE) s += xr[c];
    const float mean = wave_sum_f(s) / (float)F;
    float ss = 0.f;
    for (int c = lane; c < F; c += WAVE) { const float d = xr[c] - mean; ss += d * d; }
    const float invstd = rsqrtf(wave_sum_f(ss) / (float)F + eps);
    for (int c = lane; c < F; c += WAVE) {
        const float v = (xr[c] - mean) * invstd * gamma[c] + beta[c];
        y[(size_t)i * F + c] = v > 0.f ? v : slope * v;
    }
    if (lane == 0) { save_mean[i] = mean; save_invstd[i] = invstd; }
}

__global__ __launch_bounds__(256) void k_ln_act_bwd_rows(const float *__restrict__ dy, const float *__restrict__ y,
                                                         const float *__restrict__ x, const float *__restrict__ gamma,
                                                         const float *__restrict__ save_mean,
                                                         const float *__restrict__ save_invstd, int b, int F, float slope,
                                                         float *__restrict__ dx) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= b) return;
    const size_t r = (size_t)i * F;
    const float mean = save_mean[i], invstd = save_invstd[i];
    float a = 0.f, bs = 0.f;
    for (int c = lane; c < F; c += WAVE) {
        const float dz = dy[r + c] * (y[r + c] > 0.f ? 1.f : slope) * gamma[c];
        a += dz;
        bs += dz * (x[r + c] - mean) * invstd;
    }
    a = wave_sum_f(a) / (float)F;
    bs = wave_sum_f(bs) / (float)F;
    for (int c = lane; c < F; c += WAVE) {
        const float dz = dy[r + c] * (y[r + c] > 0.f ? 1.f : slope) * gamma[c];
        dx[r + c] = invstd * (dz - a - (x[r + c] - mean) * invstd * bs);
    }
}

// dgamma[c] = sum_i dz x_hat, dbeta[c] = sum_i dz  (column reduction, same geometry as the BatchNorm kernels)
__global__ __launch_bounds__(LN_NT) void k_ln_act_bwd_cols(const float *__restrict__ dy, const float *__restrict__ y,
                                                         const float *__restrict__ x, const float *__restrict__ save_mean,
                                                         const float *__restrict__ save_invstd, int b, int F, float slope,
                                                         float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ float sh[LN_RG][BN_COLS + 1];
    const int cl = threadIdx.x & (BN_COLS - 1), rg = threadIdx.x / BN_COLS;
    const int c = blockIdx.x * BN_COLS + cl;
    const bool on = c < F;
    float sb = 0.f, sg = 0.f;
    if (on)
#pragma unroll 4
        for (int i = rg; i < b; i += LN_RG) {
            const size_t e = (size_t)i * F + c;
            const float dz = dy[e] * (y[e] > 0.f ? 1.f : slope);
            sb += dz;
            sg += dz * (x[e] - save_mean[i]) * save_invstd[i];
        }
    sb = bn_col_sum<LN_RG>(sb, sh, cl, rg);
    sg = bn_col_sum<LN_RG>(sg, sh, cl, rg);
    if (on && rg == 0) { dgamma[c] = sg; dbeta[c] = sb; }
}

// ------------------------------------------------------------------------------------------
// Loss tail of a training step: three single-workgroup kernels (b <= a few thousand seed rows, 20 latent
// columns, ~10 clusters) in place of ~130 tiny library launches.  Reductions are in a fixed order (fp64).

// Reparameterised samples of both branches, GAT KL and the alignment term (SpaDOT.py:78-93).
//   zg [b, 2*Lg] = GAT_fc output (mu | logvar), p_m / p_v [b, Ls] fp64 = SVGP posterior, eps [b, Ls+Lg].
//   latent [b, Ls+Lg] = (p_m + eps sqrt(p_v) | mu + eps sqrt(var)),  scal = (GAT_KL, alignment).
// 32 lanes per row (Ls + Lg <= 32 columns): coalesced accesses, row norms by shuffles inside the half wave.
__device__ __forceinline__ float half_wave_sum(float x) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
    return x;
}

// Counter-based standard normal: splitmix64 of (seed, launch counter, element index) -> two uniforms -> Box-Muller.
__device__ __forceinline__ float counter_randn(unsigned long long seed, unsigned long long ctr, unsigned long long idx) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (ctr * 0x100000001B3ull + idx + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const float u1 = ((float)(unsigned)(z >> 40) + 1.0f) * (1.0f / 16777216.0f);        // (0, 1]
    const float u2 = (float)(unsigned)((z >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);     // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.2831853071795865f * u2);
}

// 8 rows per 256-thread workgroup; the two scalars go through per-workgroup partials and the LAST workgroup to finish
// (device counter, reset for the next launch) adds them in workgroup order: one launch, reproducible.
__global__ __launch_bounds__(256) void k_latent_head_fwd(const float *__restrict__ zg, const double *__restrict__ p_m,
                                                         const double *__restrict__ p_v, float *__restrict__ eps,
                                                         int b, int Ls, int Lg, float *__restrict__ latent,
                                                         float *__restrict__ scal, double *__restrict__ partials,
                                                         unsigned *__restrict__ counter,
                                                         unsigned long long *__restrict__ rng /* (seed, launches) or null */) {
    __shared__ double sh[16];
    __shared__ bool last;
    const int D = Ls + Lg;
    const int c = threadIdx.x & 31, i = blockIdx.x * 8 + (threadIdx.x >> 5);
    float val = 0.f, klt = 0.f, e = 0.f;
    {
        // every operand in ONE round trip: unconditional loads from clamped positions (both branches' operands), selected afterwards
        const int ic = min(i, b - 1), cs = min(c, Ls - 1), lg = min(max(c - Ls, 0), Lg - 1), cd = min(c, D - 1);
        const unsigned long long r0 = rng ? rng[0] : 0ull, r1 = rng ? rng[1] : 0ull;
        const float e_in = eps[(size_t)ic * D + cd];
        const double pm = p_m[(size_t)ic * Ls + cs], pv = p_v[(size_t)ic * Ls + cs];
        const float mu = zg[(size_t)ic * 2 * Lg + lg], lv = zg[(size_t)ic * 2 * Lg + Lg + lg];
        if (i < b && c < D) {
            if (rng) { e = counter_randn(r0, r1, (unsigned long long)i * D + c); eps[(size_t)i * D + c] = e; }
            else e = e_in;
        }
        if (i < b && c < Ls) {
            val = (float)(pm + (double)e * sqrt(pv));
        } else if (i < b && c < D) {
            const float var = expf(lv);
            val = mu + e * sqrtf(var);
            klt = 1.f + logf(var) - mu * mu - var;
        }
    }
    if (i < b && c < D) latent[(size_t)i * D + c] = val;
    const float ns = half_wave_sum(c < Ls ? val * val : 0.f), ng = half_wave_sum(c >= Ls && c < D ? val * val : 0.f);
    double al = 0.0;
    if (c == 0 && i < b) { const float d = sqrtf(ns) / (float)Ls - sqrtf(ng) / (float)Lg; al = (double)d * d; }
    const double kl = block_sum_d((double)klt, sh);
    al = block_sum_d(al, sh);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = kl;
        partials[2 * blockIdx.x + 1] = al;
        __threadfence();
        last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double k2 = 0.0, a2 = 0.0;
    for (int g = threadIdx.x; g < (int)gridDim.x; g += blockDim.x) {
        k2 += __builtin_nontemporal_load(partials + 2 * g);
        a2 += __builtin_nontemporal_load(partials + 2 * g + 1);
    }
    k2 = block_sum_d(k2, sh);
    a2 = block_sum_d(a2, sh);
    if (threadIdx.x == 0) { scal[0] = (float)(-0.5 * k2 / Lg); scal[1] = (float)a2; *counter = 0u; if (rng) rng[1] += 1ull; }
}

// g_latent [b, Ls+Lg] (may be null), g_scal = device scalars (d loss / d GAT_KL, d loss / d alignment).
__global__ __launch_bounds__(256) void k_latent_head_bwd(const float *__restrict__ zg, const double *__restrict__ p_v,
                                                         const float *__restrict__ eps, const float *__restrict__ latent,
                                                         const float *__restrict__ g_latent, const float *__restrict__ g_kl,
                                                         const float *__restrict__ g_al, int b, int Ls, int Lg,
                                                         float *__restrict__ d_zg, double *__restrict__ d_pm,
                                                         double *__restrict__ d_pv) {
    const int D = Ls + Lg;
    const float gk = g_kl ? g_kl[0] : 0.f, ga = g_al ? g_al[0] : 0.f;
    const int c = threadIdx.x & 31, i = blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool on = i < b && c < D;
    const float lat = on ? latent[(size_t)i * D + c] : 0.f;
    const float ns = half_wave_sum(c < Ls ? lat * lat : 0.f), ng = half_wave_sum(c >= Ls && c < D ? lat * lat : 0.f);
    if (!on) return;
    const float rs = sqrtf(ns), rg = sqrtf(ng);
    const float d = rs / (float)Ls - rg / (float)Lg;
    const float gl = g_latent ? g_latent[(size_t)i * D + c] : 0.f;
    if (c < Ls) {
        const float cs = rs > 0.f ? ga * 2.f * d / ((float)Ls * rs) : 0.f;      // d align / d s = cs * s
        const double ds = (double)gl + (double)cs * lat;
        d_pm[(size_t)i * Ls + c] = ds;
        d_pv[(size_t)i * Ls + c] = ds * (double)eps[(size_t)i * D + c] * 0.5 / sqrt(p_v[(size_t)i * Ls + c]);
    } else {
        const int l = c - Ls;
        const float cg = rg > 0.f ? -ga * 2.f * d / ((float)Lg * rg) : 0.f;
        const float dg = gl + cg * lat;
        const float mu = zg[(size_t)i * 2 * Lg + l], var = expf(zg[(size_t)i * 2 * Lg + Lg + l]);
        const float dvar = dg * eps[(size_t)i * D + c] * 0.5f / sqrtf(var) - gk * 0.5f / (float)Lg * (1.f / var - 1.f);
        d_zg[(size_t)i * 2 * Lg + l] = dg + gk * mu / (float)Lg;
        d_zg[(size_t)i * 2 * Lg + Lg + l] = dvar * var;
    }
}

// K-means loss (_train_utils.py:240-253) and OT loss (:272-307) of one batch.
//   z [b, D] latent of the seeds; labels_all[seed_ids[i]] = cluster of seed i; centres [K, D] of this time point;
//   prev [Kp, D] centres of the previous time point; gamma [Kp, Kl] row-normalised plan; cluster_list [Kl].
//   work (saved for the backward): means [K*D] | cnt [K] | n_distinct | lab [b] (as floats).
constexpr int CL_MAXK = 64, CL_MAXD = 64, CL_KREG = 16;
constexpr int CL_MAX_DYN_LDS = 108 * 1024;        // 160 KiB less the kernel's static arrays (centres, previous centres, plan: 48.6 KiB)
// FB: the same launch also writes dz = d(g_km km + g_ot ot) / dz for gradient seeds that are known when the forward runs (the
// loss weights, device scalars): k_cluster_losses_bwd's arithmetic on the state this kernel has in LDS anyway.  Host-side
// conditions (spadot_cluster_losses_fb): the fast path (K <= CL_KREG, K * D <= 512), the whole batch in ONE chunk, and room for
// [centres | d means | distances] in the segment-partial buffer.
template <bool FB>
__global__ __launch_bounds__(512) void k_cluster_losses_fwd(const float *__restrict__ z, const long long *__restrict__ labels_all,
                                                            const long long *__restrict__ seed_ids, const float *__restrict__ centres,
                                                            const float *__restrict__ prev, const float *__restrict__ gamma,
                                                            const long long *__restrict__ cluster_list, int b, int D, int K, int Kp,
                                                            int Kl, int do_km, int do_ot, float *__restrict__ out2,
                                                            float *__restrict__ work, int chunk_rows,
                                                            const float *__restrict__ g_km = nullptr,
                                                            const float *__restrict__ g_ot = nullptr, float *__restrict__ dz = nullptr) {
    // Latency-bound single workgroup: everything that is scanned repeatedly sits in LDS and the scans are
    // branch-free and unrolled, so the LDS reads of successive rows are in flight together.
    // Global memory is read ONCE, at the top: every operand of the launch (centres, previous centres, plan, cluster list,
    // seed ids -> labels, the first chunk of the latent rows, the gradient seeds) is requested before the first is used, with
    // unconditional loads from clamped positions -- until round 5 each phase fetched what it needed where it needed it, mostly
    // through predicated loads (a branch each, the load queue drained at its join): ~40 dependent round trips in a 29 us kernel.
    __shared__ double sh[16];
    __shared__ float s_means[CL_MAXK * CL_MAXD];  // centres first, batch means once the sums are complete
    __shared__ float s_prev[CL_MAXK * CL_MAXD];   // previous centres
    __shared__ float s_gam[CL_MAXK * CL_MAXK];    // plan
    __shared__ int s_cl[CL_MAXK];                 // cluster list
    __shared__ int s_cnt[CL_MAXK];
    extern __shared__ float s_dyn[];              // chunk_rows * D latent values, then chunk_rows labels, then segment partials
    float *s_z = s_dyn;
    int *s_lab = (int *)(s_dyn + (size_t)chunk_rows * D);
    float *s_part = s_dyn + (size_t)chunk_rows * D + chunk_rows;       // [512 / D][K][D + 1] (fast path)
    float *w_means = work, *w_cnt = work + (size_t)K * D, *w_nd = w_cnt + K, *w_lab = w_nd + 1;
    const int t = threadIdx.x;
    constexpr int ZB = 20;                        // latent values per thread and batch (b = 512, D = 20: the whole chunk in one)
    const int KD = K * D, KpD = do_ot ? Kp * D : 1, KpKl = do_ot ? Kp * Kl : 1, Kl1 = do_ot ? Kl : 1;
    const float *prev_p = do_ot ? prev : centres, *gam_p = do_ot ? gamma : centres;
    const long long *cl_p = do_ot ? cluster_list : seed_ids;
    const int rows0 = min(chunk_rows, b);
    const long long sid0 = seed_ids[min(t, rows0 - 1)];
    const float c0 = centres[min(t, KD - 1)], p0 = prev_p[min(t, KpD - 1)], g0 = gam_p[min(t, KpKl - 1)];
    const int cl0 = (int)cl_p[min(t, Kl1 - 1)];
    float gk_r = 0.f, go_r = 0.f;
    if constexpr (FB) { gk_r = (g_km ? g_km : centres)[0]; go_r = (g_ot ? g_ot : centres)[0]; }
    float zr[ZB];
#pragma unroll
    for (int u = 0; u < ZB; u++) zr[u] = z[min(t + u * 512, rows0 * D - 1)];
    const int lab0 = (int)labels_all[sid0];
    if (t < KD) s_means[t] = c0;
    for (int e = t + 512; e < KD; e += 512) s_means[e] = centres[e];
    if (do_ot) {
        if (t < KpD) s_prev[t] = p0;
        for (int e = t + 512; e < KpD; e += 512) s_prev[e] = prev[e];
        if (t < KpKl) s_gam[t] = g0;
        for (int e = t + 512; e < KpKl; e += 512) s_gam[e] = gamma[e];
        if (t < Kl) s_cl[t] = cl0;
    }
    constexpr int PAIRS = (CL_MAXK * CL_MAXD + 511) / 512;
    float ps[PAIRS];
    int pc[PAIRS];
#pragma unroll
    for (int u = 0; u < PAIRS; u++) { ps[u] = 0.f; pc[u] = 0; }
    double km = 0.0;
    for (int r0 = 0; r0 < b; r0 += chunk_rows) {           // one chunk when the batch fits (b = 512, D = 20: 40 KB)
        const int rows = min(chunk_rows, b - r0);
        __syncthreads();
        if (r0 == 0) {                                          // the first chunk is in registers already
#pragma unroll
            for (int u = 0; u < ZB; u++)
                if (t + u * 512 < rows * D) s_z[t + u * 512] = zr[u];
            for (int e = t + ZB * 512; e < rows * D; e += 512) s_z[e] = z[e];
            if (t < chunk_rows) {
                const int lab = t < rows ? lab0 : -1;               // -1: matches no cluster
                s_lab[t] = lab;
                if (t < rows) w_lab[t] = (float)lab;
            }
            for (int i = t + 512; i < chunk_rows; i += 512) {
                const int lab = i < rows ? (int)labels_all[seed_ids[i]] : -1;
                s_lab[i] = lab;
                if (i < rows) w_lab[i] = (float)lab;
            }
        } else {
            for (int e0 = 0; e0 < rows * D; e0 += ZB * 512) {
                float zb[ZB];
#pragma unroll
                for (int u = 0; u < ZB; u++) zb[u] = z[(size_t)r0 * D + min(e0 + t + u * 512, rows * D - 1)];
#pragma unroll
                for (int u = 0; u < ZB; u++)
                    if (e0 + t + u * 512 < rows * D) s_z[e0 + t + u * 512] = zb[u];
            }
            for (int i = t; i < chunk_rows; i += 512) {
                const int lab = (int)labels_all[seed_ids[r0 + min(i, rows - 1)]];
                s_lab[i] = i < rows ? lab : -1;
                if (i < rows) w_lab[r0 + i] = (float)lab;
            }
        }
        __syncthreads();
        if (K <= CL_KREG && K * D <= (int)blockDim.x) {
            // fast path: thread = (row segment, column) keeps the K partial sums of its segment in registers;
            // the segments are then added in order (fixed order => reproducible), far fewer serial LDS reads.
            // The fold below fills PAIRS slot 0 only, so every (cluster, column) pair has to sit there: K * D <= 512.
            const int segs = (int)blockDim.x / D, seg = t / D, d = t - seg * D;
            const int per = (rows + segs - 1) / segs;
            float av[CL_KREG];
            int cv[CL_KREG];
#pragma unroll
            for (int k = 0; k < CL_KREG; k++) { av[k] = 0.f; cv[k] = 0; }
            if (seg < segs) {
                const int i1 = min(rows, (seg + 1) * per);
                for (int i = seg * per; i < i1; i++) {
                    const int lab = s_lab[i];
                    const float zv = s_z[i * D + d];
#pragma unroll
                    for (int k = 0; k < CL_KREG; k++) { av[k] += lab == k ? zv : 0.f; cv[k] += lab == k ? 1 : 0; }
                }
                float *pp = s_part + (size_t)seg * K * (D + 1);
                for (int k = 0; k < K; k++) {
                    float a = 0.f; int c = 0;
#pragma unroll
                    for (int kk = 0; kk < CL_KREG; kk++) if (kk == k) { a = av[kk]; c = cv[kk]; }
                    pp[k * (D + 1) + d] = a;
                    if (d == 0) pp[k * (D + 1) + D] = (float)c;
                }
            }
            __syncthreads();
            if (t < K * D) {                                 // PAIRS slot 0 owns pair t
                const int k = t / D, dd = t - k * D;
                float sacc = ps[0];
                int cacc = pc[0];
                for (int sg = 0; sg < segs; sg++) {
                    sacc += s_part[(size_t)sg * K * (D + 1) + k * (D + 1) + dd];
                    cacc += (int)s_part[(size_t)sg * K * (D + 1) + k * (D + 1) + D];
                }
                ps[0] = sacc; pc[0] = cacc;
            }
        } else {
        // per-cluster sums: one (cluster, column) pair per thread slot, rows in order
#pragma unroll
        for (int u = 0; u < PAIRS; u++) {
            const int pq = t + u * 512;
            if (pq < K * D) {
                const int k = pq / D, d = pq - k * D;
                float s = ps[u];
                int c = pc[u];
#pragma unroll 8
                for (int i = 0; i < chunk_rows; i++) {              // chunk_rows is a multiple of 8; pad rows carry label -1
                    const bool hit = s_lab[i] == k;
                    s += hit ? s_z[(i < rows ? i : 0) * D + d] : 0.f;
                    c += hit ? 1 : 0;
                }
                ps[u] = s; pc[u] = c;
            }
        }
        }
        // K-means term of this chunk's rows (centres still in s_means)
        if (do_km)
            for (int i = t; i < rows; i += blockDim.x) {
                const int k = s_lab[i];
                float a = 0.f;
#pragma unroll 4
                for (int d = 0; d < D; d++) { const float e = s_z[i * D + d] - s_means[k * D + d]; a += e * e; }
                km += a;
            }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PAIRS; u++) {
        const int pq = t + u * 512;
        if (pq < K * D) {
            const int k = pq / D, d = pq - k * D;
            if (pc[u] > 0) s_means[pq] = ps[u] / (float)pc[u];      // else: the stored centre stays
            if (d == 0) s_cnt[k] = pc[u];
        }
    }
    __syncthreads();
    int nd = 0;
    for (int k = 0; k < K; k++) nd += s_cnt[k] > 0;
    for (int pq = t; pq < K * D; pq += blockDim.x) w_means[pq] = s_means[pq];
    for (int k = t; k < K; k += blockDim.x) w_cnt[k] = (float)s_cnt[k];
    if (t == 0) w_nd[0] = (float)nd;
    km = block_sum_d(km, sh);
    double ot = 0.0;
    if (do_ot)
        for (int pq = t; pq < Kp * Kl; pq += blockDim.x) {
            const int p = pq / Kl, q = pq - p * Kl, k = s_cl[q];
            float a = 0.f;
#pragma unroll 4
            for (int d = 0; d < D; d++) { const float e = s_prev[p * D + d] - s_means[k * D + d]; a += e * e; }
            ot += (double)s_gam[pq] * (double)sqrtf(a);
        }
    ot = block_sum_d(ot, sh);
    if (t == 0) {
        out2[0] = do_km ? (float)(km / D / (nd > 0 ? nd : 1)) : 0.f;
        out2[1] = do_ot ? (float)(ot / ((double)Kp * Kl)) : 0.f;
    }
    if constexpr (FB) {
        // s_means = batch means, s_cnt = counts, s_prev = previous centres, s_z / s_lab = the batch's rows and labels (one chunk)
        float *s_cen = s_part, *s_dm = s_part + (size_t)K * D, *s_dist = s_part + 2 * (size_t)K * D;
        const float gk = (do_km && g_km) ? gk_r : 0.f, go = (do_ot && g_ot) ? go_r : 0.f;
        __syncthreads();                                  // (block_sum_d's scratch and s_part are free now)
        if (t < KD) { s_dm[t] = 0.f; s_cen[t] = c0; }
        for (int pq = t + 512; pq < K * D; pq += blockDim.x) { s_dm[pq] = 0.f; s_cen[pq] = centres[pq]; }
        if (do_ot)
            for (int pq = t; pq < Kp * Kl; pq += blockDim.x) {
                const int p = pq / Kl, q = pq - p * Kl, k = s_cl[q];
                float a = 0.f;
#pragma unroll 4
                for (int e = 0; e < D; e++) { const float df = s_means[k * D + e] - s_prev[p * D + e]; a += df * df; }
                s_dist[pq] = sqrtf(a);
            }
        __syncthreads();
        if (do_ot)
            for (int qd = t; qd < Kl * D; qd += blockDim.x) {
                const int q = qd / D, d = qd - q * D, k = s_cl[q];
                if (s_cnt[k] <= 0) continue;
                float acc = 0.f;
                for (int p = 0; p < Kp; p++) {
                    const float dist = s_dist[p * Kl + q];
                    if (dist > 0.f) acc += s_gam[p * Kl + q] * (s_means[k * D + d] - s_prev[p * D + d]) / dist;
                }
                s_dm[k * D + d] = go * acc / ((float)Kp * Kl) / (float)s_cnt[k];
            }
        __syncthreads();
        const float ndf = nd > 0 ? (float)nd : 1.f;
        const float ck = gk * 2.f / ((float)D * ndf);
#pragma unroll 4
        for (int e = t; e < b * D; e += blockDim.x) {
            const int i = e / D, d = e - i * D, k = s_lab[i];
            dz[e] = ck * (s_z[e] - s_cen[k * D + d]) + s_dm[k * D + d];
        }
    }
}

__global__ __launch_bounds__(512) void k_cluster_losses_bwd(const float *__restrict__ z, const float *__restrict__ centres,
                                                            const float *__restrict__ prev, const float *__restrict__ gamma,
                                                            const long long *__restrict__ cluster_list, const float *__restrict__ work,
                                                            const float *__restrict__ g_km, const float *__restrict__ g_ot, int b,
                                                            int D, int K, int Kp, int Kl, int do_km, int do_ot,
                                                            float *__restrict__ dz) {
    __shared__ float s_dm[CL_MAXK * CL_MAXD];     // d OT / d means[k, d], already divided by cnt[k]
    __shared__ float s_mean[CL_MAXK * CL_MAXD], s_prev[CL_MAXK * CL_MAXD], s_cen[CL_MAXK * CL_MAXD];
    __shared__ float s_dist[CL_MAXK * CL_MAXK];
    const float *w_means = work, *w_cnt = work + (size_t)K * D, *w_nd = w_cnt + K, *w_lab = w_nd + 1;
    const int t = threadIdx.x;
    const float gk = (do_km && g_km) ? g_km[0] : 0.f, go = (do_ot && g_ot) ? g_ot[0] : 0.f;
    for (int pq = t; pq < K * D; pq += blockDim.x) { s_dm[pq] = 0.f; s_mean[pq] = w_means[pq]; s_cen[pq] = centres[pq]; }
    if (do_ot)
        for (int pq = t; pq < Kp * D; pq += blockDim.x) s_prev[pq] = prev[pq];
    __syncthreads();
    if (do_ot) {
        for (int pq = t; pq < Kp * Kl; pq += blockDim.x) {                  // distances once, not once per column
            const int p = pq / Kl, q = pq - p * Kl, k = (int)cluster_list[q];
            float a = 0.f;
#pragma unroll 4
            for (int e = 0; e < D; e++) { const float df = s_mean[k * D + e] - s_prev[p * D + e]; a += df * df; }
            s_dist[pq] = sqrtf(a);
        }
        __syncthreads();
        for (int qd = t; qd < Kl * D; qd += blockDim.x) {
            const int q = qd / D, d = qd - q * D, k = (int)cluster_list[q];
            if (w_cnt[k] <= 0.f) continue;                      // the stored centre stands in: no gradient
            float acc = 0.f;
            for (int p = 0; p < Kp; p++) {
                const float dist = s_dist[p * Kl + q];
                if (dist > 0.f) acc += gamma[p * Kl + q] * (s_mean[k * D + d] - s_prev[p * D + d]) / dist;
            }
            s_dm[k * D + d] = go * acc / ((float)Kp * Kl) / w_cnt[k];
        }
    }
    __syncthreads();
    const float nd = w_nd[0] > 0.f ? w_nd[0] : 1.f;
    const float ck = gk * 2.f / ((float)D * nd);
#pragma unroll 4
    for (int e = t; e < b * D; e += blockDim.x) {               // element-parallel: coalesced over the [b, D] arrays
        const int i = e / D, d = e - i * D, k = (int)w_lab[i];
        dz[e] = ck * (z[e] - s_cen[k * D + d]) + s_dm[k * D + d];
    }
}

// elbo = sum_k w[k] * terms[k] over the six loss terms, and the 7-vector (elbo, terms...) for logging.
__global__ void k_mix_losses_fwd(const float *t0, const float *t1, const float *t2, const float *t3, const float *t4,
                                 const float *t5, const float *__restrict__ w, float *__restrict__ out7) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float v[6] = {t0[0], t1[0], t2[0], t3[0], t4[0], t5[0]};
    float e = 0.f;
    for (int k = 0; k < 6; k++) { e += w[k] * v[k]; out7[1 + k] = v[k]; }
    out7[0] = e;
    out7[7] = e;          // second copy: the differentiable output (out7[0..6] is the detached logging vector)
}
__global__ void k_mix_losses_bwd(const float *__restrict__ g, const float *__restrict__ w, float *__restrict__ g6) {
    const int k = threadIdx.x;
    if (k < 6) g6[k] = g[0] * w[k];
}

// dst[r, 0:K] = (bf16) src[r, 0:K] for up to 4 matrices in ONE launch (the compute-dtype images of the fp32 weights:
// one launch per stage instead of one per matrix); dst rows may be longer than K (zero padding written once, elsewhere).
struct CastSeg { const float *src; __bf16 *dst; int rows, K, Kp; long long first; };     // first = start in the flat index space
struct CastSegs { CastSeg s[4]; int n; long long total; };
__global__ __launch_bounds__(256) void k_cast_rows_multi(CastSegs segs) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < segs.total; q += (long long)gridDim.x * 256) {
        int k = 0;
#pragma unroll
        for (int t = 1; t < 4; t++)
            if (t < segs.n && q >= segs.s[t].first) k = t;
        const CastSeg &S = segs.s[k];
        const long long e = (q - S.first) * 4;                 // four consecutive elements of one row (K % 4 == 0)
        const int r = (int)(e / S.K), c = (int)(e - (long long)r * S.K);
        const float4 v = *reinterpret_cast<const float4 *>(S.src + (size_t)r * S.K + c);
        *reinterpret_cast<uint2 *>(S.dst + (size_t)r * S.Kp + c) = make_uint2(bf16_pack2(v.x, v.y), bf16_pack2(v.z, v.w));
    }
}

int pick_gat(int C, int &vec, int &niter, int dtype = -1) {
    // bf16 rows: 16-byte accesses (8 channels per lane) when a head's row is a multiple of 1 KiB
    if (dtype == SPADOT_DT_BF16 && C % 512 == 0 && C / 512 <= 2) { vec = 8; niter = C / 512; return 0; }
    if (C % 256 == 0 && C / 256 <= 4) { vec = 4; niter = C / 256; return 0; }
    if (C <= 512) { vec = 1; niter = (C + 63) / 64; return 0; }
    return -22;
}

}  // namespace

#define GAT_DISPATCH(KERNEL, T, ...)                                                            \
    do {                                                                                        \
        if (vec == 8 && niter == 1) hipLaunchKernelGGL((KERNEL<T, 8, 1>), __VA_ARGS__);          \
        else if (vec == 8) hipLaunchKernelGGL((KERNEL<T, 8, 2>), __VA_ARGS__);                   \
        else if (vec == 4 && niter == 1) hipLaunchKernelGGL((KERNEL<T, 4, 1>), __VA_ARGS__);     \
        else if (vec == 4 && niter == 2) hipLaunchKernelGGL((KERNEL<T, 4, 2>), __VA_ARGS__);     \
        else if (vec == 4 && niter == 3) hipLaunchKernelGGL((KERNEL<T, 4, 3>), __VA_ARGS__);     \
        else if (vec == 4 && niter == 4) hipLaunchKernelGGL((KERNEL<T, 4, 4>), __VA_ARGS__);     \
        else if (niter == 1) hipLaunchKernelGGL((KERNEL<T, 1, 1>), __VA_ARGS__);                 \
        else if (niter == 2) hipLaunchKernelGGL((KERNEL<T, 1, 2>), __VA_ARGS__);                 \
        else if (niter <= 4) hipLaunchKernelGGL((KERNEL<T, 1, 4>), __VA_ARGS__);                 \
        else hipLaunchKernelGGL((KERNEL<T, 1, 8>), __VA_ARGS__);                                 \
    } while (0)

extern "C" {

const char *spadot_model_version(void) { return "spadot_model 0.1 (gfx950)"; }

int spadot_gat_forward(const void *h, int dtype, const float *s_src, const float *s_dst, const int *rowptr,
                       const int *col, const float *bias, int n, int H, int C, int concat, int act, void *out,
                       float *alpha_out, void *stream) {
    int vec, niter;
    if (n <= 0 || H <= 0 || pick_gat(C, vec, niter, dtype)) return -22;
    if (!concat && H > 4) return -22;   // head-mean reduces over the workgroup's 4 waves
    hipStream_t st_ = (hipStream_t)stream;
    const size_t lds = concat ? 0 : sizeof(float) * 4 * (size_t)C;
    if (dtype == SPADOT_DT_F32)
        GAT_DISPATCH(k_gat_fwd, float, dim3(8 * ((n + 7) / 8)), dim3(256), lds, st_, (const float *)h, s_src, s_dst, rowptr, col,
                     bias, n, H, C, concat, act, (float *)out, alpha_out);
    else if (dtype == SPADOT_DT_BF16)
        GAT_DISPATCH(k_gat_fwd, __bf16, dim3(8 * ((n + 7) / 8)), dim3(256), lds, st_, (const __bf16 *)h, s_src, s_dst, rowptr, col,
                     bias, n, H, C, concat, act, (__bf16 *)out, alpha_out);
    else
        return -22;
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_gat_backward_target(const void *g_out, const void *out, const void *h, int dtype, const float *s_src,
                               const float *s_dst, const float *alpha, const int *rowptr, const int *col, int n,
                               int H, int C, int concat, int act, void *g_pre, float *dz, float *ds_dst,
                               void *stream) {
    int vec, niter;
    if (n <= 0 || H <= 0 || pick_gat(C, vec, niter, dtype)) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    if (dtype == SPADOT_DT_F32)
        GAT_DISPATCH(k_gat_bwd_target, float, dim3(8 * ((n + 7) / 8)), dim3(256), 0, st_, (const float *)g_out, (const float *)out,
                     (const float *)h, s_src, s_dst, alpha, rowptr, col, n, H, C, concat, act, (float *)g_pre, dz,
                     ds_dst);
    else if (dtype == SPADOT_DT_BF16)
        GAT_DISPATCH(k_gat_bwd_target, __bf16, dim3(8 * ((n + 7) / 8)), dim3(256), 0, st_, (const __bf16 *)g_out, (const __bf16 *)out,
                     (const __bf16 *)h, s_src, s_dst, alpha, rowptr, col, n, H, C, concat, act, (__bf16 *)g_pre, dz,
                     ds_dst);
    else
        return -22;
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_gat_logits(const void *h, int dtype, const float *att_src, const float *att_dst, int n, int H, int C,
                      float *s_src, float *s_dst, void *stream) {
    int vec, niter;
    if (n <= 0 || H <= 0 || pick_gat(C, vec, niter, dtype)) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    if (dtype == SPADOT_DT_F32)
        GAT_DISPATCH(k_gat_logits, float, dim3(8 * ((n + 7) / 8)), dim3(256), 0, st_, (const float *)h, att_src, att_dst, n, H, C, s_src, s_dst);
    else if (dtype == SPADOT_DT_BF16)
        GAT_DISPATCH(k_gat_logits, __bf16, dim3(8 * ((n + 7) / 8)), dim3(256), 0, st_, (const __bf16 *)h, att_src, att_dst, n, H, C, s_src, s_dst);
    else
        return -22;
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_gat_att_grad(const void *h, int dtype, const float *ds_src, const float *ds_dst, int n, int H, int C,
                        float *scratch, int scratch_floats, float *datt_src, float *datt_dst, const void *g_pre,
                        int n_pre, void *stream) {
    int vec, niter;
    if (n <= 0 || H <= 0 || pick_gat(C, vec, niter, dtype) || !scratch) return -22;
    if (g_pre && (n_pre <= 0 || n_pre > n)) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    const int width = (g_pre ? 3 : 2) * H * C;
    int nslab = (n + 15) / 16;       // 16 nodes per workgroup: enough workgroups to keep the row loads of ~80 MB in flight
    if ((long long)nslab * width > scratch_floats) nslab = scratch_floats / width;
    if (nslab < 1) return -22;
    const int per = (n + nslab - 1) / nslab;
    nslab = (n + per - 1) / per;
    if (dtype == SPADOT_DT_F32)
        GAT_DISPATCH(k_gat_datt_part, float, dim3(nslab), dim3(256), 0, st_, (const float *)h, ds_src, ds_dst, n, H, C, per, scratch, (const float *)g_pre, n_pre);
    else if (dtype == SPADOT_DT_BF16)
        GAT_DISPATCH(k_gat_datt_part, __bf16, dim3(nslab), dim3(256), 0, st_, (const __bf16 *)h, ds_src, ds_dst, n, H, C, per, scratch, (const __bf16 *)g_pre, n_pre);
    else
        return -22;
    // scratch rows are [slab][src H*C | dst H*C (| g_pre column sums H*C)]: one column sum writes all outputs (adjacent)
    hipLaunchKernelGGL(k_colsum_parts, dim3((width + 63) / 64), dim3(CS_NT), 0, st_, scratch, nslab, width, datt_src);
    (void)datt_dst;
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_cast_rows_multi(const float *const *src, void *const *dst, const int *rows, const int *K, const int *Kp, int n,
                           void *stream) {
    if (n < 1 || n > 4 || !src || !dst || !rows || !K || !Kp) return -22;
    CastSegs segs;
    long long tot = 0;
    for (int t = 0; t < n; t++) {
        if (rows[t] <= 0 || K[t] <= 0 || K[t] % 4 != 0 || Kp[t] < K[t] || Kp[t] % 4 != 0) return -22;
        if (((uintptr_t)src[t] & 15) != 0 || ((uintptr_t)dst[t] & 7) != 0) return -22;
        segs.s[t] = CastSeg{src[t], (__bf16 *)dst[t], rows[t], K[t], Kp[t], tot};
        tot += (long long)rows[t] * K[t] / 4;
    }
    for (int t = n; t < 4; t++) segs.s[t] = segs.s[0];
    segs.n = n; segs.total = tot;
    const long long want = (tot + 255) / 256;
    const int nb = (int)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(k_cast_rows_multi, dim3(nb), dim3(256), 0, (hipStream_t)stream, segs);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_colsum(const float *x, int rows, int width, float *out, void *stream) {
    if (rows <= 0 || width <= 0) return -22;
    hipLaunchKernelGGL(k_colsum_parts, dim3((width + 63) / 64), dim3(CS_NT), 0, (hipStream_t)stream, x, rows, width, out);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_gat_backward_source(const void *g_pre, int dtype, const float *alpha, const float *dz,
                               const int *rowptr_t, const int *col_t, const int *eid_t, int n, int H, int C,
                               void *dh, float *ds_src, const float *ds_dst, const float *att_src,
                               const float *att_dst, void *stream) {
    int vec, niter;
    if (n <= 0 || H <= 0 || pick_gat(C, vec, niter, dtype)) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    if (dtype == SPADOT_DT_F32)
        GAT_DISPATCH(k_gat_bwd_source, float, dim3(8 * ((n + 7) / 8)), dim3(256), 0, st_, (const float *)g_pre, alpha, dz, rowptr_t,
                     col_t, eid_t, n, H, C, (float *)dh, ds_src, ds_dst, att_src, att_dst);
    else if (dtype == SPADOT_DT_BF16)
        GAT_DISPATCH(k_gat_bwd_source, __bf16, dim3(8 * ((n + 7) / 8)), dim3(256), 0, st_, (const __bf16 *)g_pre, alpha, dz, rowptr_t,
                     col_t, eid_t, n, H, C, (__bf16 *)dh, ds_src, ds_dst, att_src, att_dst);
    else
        return -22;
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

#define FP_DISPATCH(dtype, CALL_F32, CALL_F64) \
    do { if ((dtype) == SPADOT_DT_F32) { CALL_F32; } else if ((dtype) == SPADOT_DT_F64) { CALL_F64; } else return -22; } while (0)

int spadot_kernel_matrix(const void *x, const void *z, int n, int m, int d, double scale, int kind, int dtype,
                         void *K, void *stream) {
    if (n <= 0 || m <= 0 || d <= 0 || kind < 0 || kind > 2 || n > 65535 * 64) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    // rows go through gridDim.y in slabs of <= 65535
    for (int r0 = 0; r0 < n; r0 += 65535) {
        const int rows = n - r0 < 65535 ? n - r0 : 65535;
        dim3 g((m + 255) / 256, rows);
        FP_DISPATCH(dtype,
                    hipLaunchKernelGGL(k_kernel_matrix<float>, g, dim3(256), 0, st_, (const float *)x + (size_t)r0 * d, (const float *)z, rows, m, d, scale, kind, (float *)K + (size_t)r0 * m),
                    hipLaunchKernelGGL(k_kernel_matrix<double>, g, dim3(256), 0, st_, (const double *)x + (size_t)r0 * d, (const double *)z, rows, m, d, scale, kind, (double *)K + (size_t)r0 * m));
    }
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_spd_inverse_logdet2(const double *A, int Lsrc, int L, int m, const double *add0, const double *add1, double *Ainv,
                               double *logdet, void *stream) {
    if (L <= 0 || m <= 0 || Lsrc < 0 || Lsrc > L) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    // smallest tile edge whose lower-triangular tile grid fits the workgroup: T <= 31 (T(T+1)/2 <= 512)
    const int TS = (m + 30) / 31;
    if (TS > 10) return -34;                      // m > 310: the caller uses the library's batched Cholesky
    const int T = (m + TS - 1) / TS;
    const int RS = TS < SWEEP_RS ? TS : SWEEP_RS;   // register core per tile edge; the rest of a tile lives in LDS
    const int CS = TS + ((TS & 1) ? 0 : 1);         // k_spd_sweep's column-buffer stride
    size_t lds = sizeof(double) * (2 * ((size_t)T * CS + 1) + (size_t)m + 16 + (size_t)(TS * TS - RS * RS) * SWEEP_NT);
    // (Asking for most of a compute unit's 160 KB of LDS, so that no GEMM or GAT workgroup is placed beside a sweep workgroup,
    // changed nothing -- 313 us in the step, 591.5 against 592.5 steps/s, round 4: the slow-down beside the GAT branch is the
    // chip's clock under matrix-core load, not a neighbour on the unit.)
#define SWEEP_CASE(N)                                                                                         \
    case N: {                                                                                                 \
        static PerDeviceFlag attr_set;                                                                              \
        if (!attr_set) { (void)hipFuncSetAttribute((const void *)k_spd_sweep<N>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr_set = true; } \
        hipLaunchKernelGGL(k_spd_sweep<N>, dim3(L), dim3(SWEEP_NT), lds, st_, A, m, T, Ainv, logdet, Lsrc, add0, add1);         \
    } break;
    switch (TS) {
        SWEEP_CASE(1) SWEEP_CASE(2) SWEEP_CASE(3) SWEEP_CASE(4) SWEEP_CASE(5) SWEEP_CASE(6) SWEEP_CASE(7)
        SWEEP_CASE(8) SWEEP_CASE(9) SWEEP_CASE(10)
        default: return -34;
    }
#undef SWEEP_CASE
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_spd_inverse_logdet(const double *A, int L, int m, double *Ainv, double *logdet, void *stream) {
    return spadot_spd_inverse_logdet2(A, 0, L, m, nullptr, nullptr, Ainv, logdet, stream);
}

int spadot_rowdot_forward(const void *A, const void *B, int L, int n, int m, int dtype, void *out, void *stream) {
    if (L <= 0 || n <= 0 || m <= 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    const long long rows = (long long)L * n;
    dim3 g((unsigned)((rows + 3) / 4));
    FP_DISPATCH(dtype,
                hipLaunchKernelGGL(k_rowdot_fwd<float>, g, dim3(256), 0, st_, (const float *)A, (const float *)B, L, n, m, (float *)out),
                hipLaunchKernelGGL(k_rowdot_fwd<double>, g, dim3(256), 0, st_, (const double *)A, (const double *)B, L, n, m, (double *)out));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_rowdot_backward(const void *g_, const void *B, int L, int n, int m, int dtype, void *gA, void *stream) {
    if (L <= 0 || n <= 0 || m <= 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    const long long tot = (long long)L * n * m;
    dim3 g((unsigned)((tot + 255) / 256));
    FP_DISPATCH(dtype,
                hipLaunchKernelGGL(k_rowdot_bwd<float>, g, dim3(256), 0, st_, (const float *)g_, (const float *)B, L, n, m, (float *)gA),
                hipLaunchKernelGGL(k_rowdot_bwd<double>, g, dim3(256), 0, st_, (const double *)g_, (const double *)B, L, n, m, (double *)gA));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_elbo_forward(const void *mu, const void *var, const void *mv, const void *tr, const void *pm,
                        const void *pv, const void *ktilde, int b, int L, int dtype, void *out2, void *stream) {
    if (b <= 0 || L <= 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    FP_DISPATCH(dtype,
                hipLaunchKernelGGL(k_elbo_fwd<float>, dim3(1), dim3(1024), 0, st_, (const float *)mu, (const float *)var, (const float *)mv, (const float *)tr, (const float *)pm, (const float *)pv, (const float *)ktilde, b, L, (float *)out2),
                hipLaunchKernelGGL(k_elbo_fwd<double>, dim3(1), dim3(1024), 0, st_, (const double *)mu, (const double *)var, (const double *)mv, (const double *)tr, (const double *)pm, (const double *)pv, (const double *)ktilde, b, L, (double *)out2));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_elbo_backward(const void *g2, const void *mu, const void *var, const void *mv, const void *tr,
                         const void *pm, const void *pv, const void *ktilde, int b, int L, int dtype, void *g_mu,
                         void *g_var, void *g_mv, void *g_tr, void *g_pm, void *g_pv, void *stream) {
    if (b <= 0 || L <= 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    dim3 g((b * L + 255) / 256);
    FP_DISPATCH(dtype,
                hipLaunchKernelGGL(k_elbo_bwd<float>, g, dim3(256), 0, st_, (const float *)g2, (const float *)mu, (const float *)var, (const float *)mv, (const float *)tr, (const float *)pm, (const float *)pv, (const float *)ktilde, b, L, (float *)g_mu, (float *)g_var, (float *)g_mv, (float *)g_tr, (float *)g_pm, (float *)g_pv),
                hipLaunchKernelGGL(k_elbo_bwd<double>, g, dim3(256), 0, st_, (const double *)g2, (const double *)mu, (const double *)var, (const double *)mv, (const double *)tr, (const double *)pm, (const double *)pv, (const double *)ktilde, b, L, (double *)g_mu, (double *)g_var, (double *)g_mv, (double *)g_tr, (double *)g_pm, (double *)g_pv));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_bn_act_forward(const void *x, int x_dtype, const float *lin_bias, const float *gamma, const float *beta,
                          float *running_mean, float *running_var, long long *num_batches_tracked, int b, int F,
                          double momentum, double eps, double slope, float *y, float *save_mean, float *save_invstd,
                          void *stream) {
    if (b <= 0 || F <= 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    dim3 g((F + BN_COLS - 1) / BN_COLS);
    if (x_dtype == SPADOT_DT_F32)
        hipLaunchKernelGGL(k_bn_act_fwd<float>, g, dim3(BN_NT), 0, st_, (const float *)x, lin_bias, gamma, beta, running_mean,
                           running_var, num_batches_tracked, b, F, (float)momentum, (float)eps, (float)slope, y, save_mean, save_invstd);
    else if (x_dtype == SPADOT_DT_BF16)
        hipLaunchKernelGGL(k_bn_act_fwd<__bf16>, g, dim3(BN_NT), 0, st_, (const __bf16 *)x, lin_bias, gamma, beta, running_mean,
                           running_var, num_batches_tracked, b, F, (float)momentum, (float)eps, (float)slope, y, save_mean, save_invstd);
    else
        return -22;
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_bn_act_backward(const float *dy, const float *y, const void *x, int x_dtype, const float *lin_bias,
                           const float *gamma, const float *save_mean, const float *save_invstd, int b, int F,
                           double slope, void *dx, float *dgamma, float *dbeta, void *stream) {
    if (b <= 0 || F <= 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    dim3 g((F + BN_COLS - 1) / BN_COLS);
    if (x_dtype == SPADOT_DT_F32)
        hipLaunchKernelGGL(k_bn_act_bwd<float>, g, dim3(BN_NT), 0, st_, dy, y, (const float *)x, lin_bias, gamma, save_mean,
                           save_invstd, b, F, (float)slope, (float *)dx, dgamma, dbeta);
    else if (x_dtype == SPADOT_DT_BF16)
        hipLaunchKernelGGL(k_bn_act_bwd<__bf16>, g, dim3(BN_NT), 0, st_, dy, y, (const __bf16 *)x, lin_bias, gamma, save_mean,
                           save_invstd, b, F, (float)slope, (__bf16 *)dx, dgamma, dbeta);
    else
        return -22;
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_ln_act_forward(const float *x, const float *gamma, const float *beta, int b, int F, double eps, double slope,
                          float *y, float *save_mean, float *save_invstd, void *stream) {
    if (b <= 0 || F <= 0) return -22;
    hipLaunchKernelGGL(k_ln_act_fwd, dim3((b + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, b, F, (float)eps,
                       (float)slope, y, save_mean, save_invstd);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_ln_act_backward(const float *dy, const float *y, const float *x, const float *gamma, const float *save_mean,
                           const float *save_invstd, int b, int F, double slope, float *dx, float *dgamma, float *dbeta,
                           void *stream) {
    if (b <= 0 || F <= 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ln_act_bwd_rows, dim3((b + 3) / 4), dim3(256), 0, st_, dy, y, x, gamma, save_mean, save_invstd, b, F,
                       (float)slope, dx);
    hipLaunchKernelGGL(k_ln_act_bwd_cols, dim3((F + BN_COLS - 1) / BN_COLS), dim3(LN_NT), 0, st_, dy, y, x, save_mean,
                       save_invstd, b, F, (float)slope, dgamma, dbeta);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_svgp_post_forward(const double *raw, const double *rd, const double *r, const double *Mr, const double *ld,
                             const double *sm, const double *mu, const double *var, const double *ktilde, int b, int L,
                             int m, double c, double kl_const, double b_over_N, double *p_m, double *mv, double *p_v,
                             double *tr, double *out4, float *skl32, void *stream) {
    if (b <= 0 || L <= 0 || m <= 0) return -22;
    hipLaunchKernelGGL(k_svgp_post_fwd, dim3(1), dim3(1024), 0, (hipStream_t)stream, raw, rd, r, Mr, ld, sm, mu, var, ktilde,
                       b, L, m, c, kl_const, b_over_N, p_m, mv, p_v, tr, out4, skl32);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
int spadot_svgp_pre2(const float *z, const double *Kn, int b, int L, int m, double *mu, double *var, double *w, double *muw,
                     double *A, void *stream) {
    if (b <= 0 || L <= 0 || m <= 0 || !Kn || !A) return -22;
    hipLaunchKernelGGL(k_svgp_pre2, dim3((b * L + 3) / 4), dim3(256), 0, (hipStream_t)stream, z, Kn, b, L, m, mu, var, w, muw, A);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
int spadot_svgp_mid(const double *S, const double *t, const double *M, const double *X2, int L, int m, int rows2,
                    double *r, double *Mr, double *raw, double *sm, double *smpart, int smpart_doubles, void *stream) {
    if (L <= 0 || m <= 0 || rows2 <= 0 || !smpart) return -22;
    const int gx = (m + 3) / 4, nparts = gx * 4;
    if ((long long)L * nparts > smpart_doubles) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    hipLaunchKernelGGL(k_svgp_mid1, dim3(gx, L), dim3(256), 0, st_, S, t, M, m, r, smpart);
    hipLaunchKernelGGL(k_svgp_mid2, dim3((m + rows2 + 3) / 4, L), dim3(256), 0, st_, M, X2, (const double *)r,
                       (const double *)smpart, nparts, m, rows2, L, Mr, raw, sm);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_svgp_post_pm_pv(const double *raw, const double *rd_a, const double *ktilde, int b, int L, double c, double *p_m,
                           double *p_v, void *stream) {
    if (b <= 0 || L <= 0 || !raw || !rd_a || !ktilde || !p_m || !p_v) return -22;
    hipLaunchKernelGGL(k_svgp_post_pmpv, dim3((b * L + 255) / 256), dim3(256), 0, (hipStream_t)stream, raw, rd_a, ktilde, b, L, c,
                       p_m, p_v);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_svgp_q1t(const double *Ta, const double *Tb, const double *G2T, const double *m0, const double *g_kl, int L, int nh,
                    int b, double *q1, void *stream) {
    if (L <= 0 || nh <= 0 || b <= 0 || !Ta || !Tb || !G2T || !m0 || !g_kl || !q1) return -22;
    hipLaunchKernelGGL(k_svgp_q1t, dim3((b + 15) / 16, L), dim3(256), 0, (hipStream_t)stream, Ta, Tb, G2T, m0, g_kl, nh, b, q1);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_svgp_post_backward(const float *g_skl, const double *out4, const double *G_pm, const double *G_pv,
                              const double *mu, const double *var, const double *mv, const double *tr, const double *p_m,
                              const double *p_v, const double *ktilde, const double *Mr, const double *M, int b, int L,
                              int m, double c, double b_over_N, double *g_mu, double *g_var, double *G1, double *G2T,
                              double *g_kl, double *gMr, double *gM, void *stream) {
    if (b <= 0 || L <= 0 || m <= 0) return -22;
    long long tot = (long long)b * L;
    if ((long long)L * m > tot) tot = (long long)L * m;
    if ((long long)m * m > tot) tot = (long long)m * m;
    hipLaunchKernelGGL(k_svgp_post_bwd, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g_skl, out4,
                       G_pm, G_pv, mu, var, mv, tr, p_m, p_v, ktilde, Mr, M, b, L, m, c, b_over_N, g_mu, g_var, G1, G2T,
                       g_kl, gMr, gM);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_svgp_grad_tail(const double *q1, const double *q2, const double *Kdt, const double *p_v, const double *ktilde,
                          const double *p_m, const double *mu, const double *w, const double *g_kl, const double *g_mu,
                          const double *g_var, int b, int L, double c, double *dmu, double *dvar, float *dz,
                          void *stream) {
    if (b <= 0 || L <= 0 || (!dz && !dmu) || (!dmu != !dvar)) return -22;      // (dmu and dvar go together: the kernel writes both)
    hipLaunchKernelGGL(k_svgp_grad_tail, dim3((b * L + 255) / 256), dim3(256), 0, (hipStream_t)stream, q1, q2, Kdt, p_v,
                       ktilde, p_m, mu, w, g_kl, g_mu, g_var, b, L, c, dmu, dvar, dz);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_svgp_pre(const float *z, int b, int L, double *mu, double *var, double *w, double *muw, void *stream) {
    if (b <= 0 || L <= 0) return -22;
    hipLaunchKernelGGL(k_svgp_pre, dim3((b * L + 255) / 256), dim3(256), 0, (hipStream_t)stream, z, b, L, mu, var, w, muw);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_latent_head_forward(const float *zg, const double *p_m, const double *p_v, float *eps, int b, int Ls,
                               int Lg, float *latent, float *scal2, double *partials, unsigned *counter,
                               unsigned long long *rng_state, void *stream) {
    if (b <= 0 || Ls <= 0 || Lg <= 0 || !partials || !counter || !eps) return -22;
    if (Ls + Lg > 32) return -22;                 // one half wave (32 lanes) per row
    hipLaunchKernelGGL(k_latent_head_fwd, dim3((b + 7) / 8), dim3(256), 0, (hipStream_t)stream, zg, p_m, p_v, eps, b, Ls, Lg,
                       latent, scal2, partials, counter, rng_state);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_latent_head_backward(const float *zg, const double *p_v, const float *eps, const float *latent,
                                const float *g_latent, const float *g_kl, const float *g_align, int b, int Ls, int Lg,
                                float *d_zg, double *d_pm, double *d_pv, void *stream) {
    if (b <= 0 || Ls <= 0 || Lg <= 0) return -22;
    if (Ls + Lg > 32) return -22;
    hipLaunchKernelGGL(k_latent_head_bwd, dim3((b + 7) / 8), dim3(256), 0, (hipStream_t)stream, zg, p_v, eps, latent,
                       g_latent, g_kl, g_align, b, Ls, Lg, d_zg, d_pm, d_pv);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_cluster_losses_forward(const float *z, const long long *labels_all, const long long *seed_ids,
                                  const float *centres, const float *prev_centres, const float *gamma,
                                  const long long *cluster_list, int b, int D, int K, int Kp, int Kl, int do_km,
                                  int do_ot, float *out2, float *work, void *stream) {
    if (b <= 0 || D <= 0 || K <= 0 || K > CL_MAXK || D > CL_MAXD) return -22;
    if (do_ot && (Kp <= 0 || Kp > CL_MAXK || Kl <= 0 || Kl > K || !prev_centres || !gamma || !cluster_list)) return -22;
    // rows staged per pass: the whole batch when it fits 40 KB, never fewer than the previous centres need
    int chunk = 10240 / D;
    if (chunk > b) chunk = b;
    if (chunk < CL_MAXK) chunk = CL_MAXK;
    chunk = (chunk + 7) / 8 * 8;
    size_t lds = sizeof(float) * (size_t)chunk * D + sizeof(int) * (size_t)chunk;
    if (K <= CL_KREG && K * D <= 512) lds += sizeof(float) * (size_t)(512 / D) * K * (D + 1);
    if (lds > (size_t)CL_MAX_DYN_LDS) return -22;
    static PerDeviceFlag attr_set;     
    if (!attr_set) { (void)hipFuncSetAttribute((const void *)k_cluster_losses_fwd<false>, hipFuncAttributeMaxDynamicSharedMemorySize, CL_MAX_DYN_LDS); attr_set = true; }
    hipLaunchKernelGGL(k_cluster_losses_fwd<false>, dim3(1), dim3(512), lds, (hipStream_t)stream, z, labels_all, seed_ids, centres,
                       prev_centres, gamma, cluster_list, b, D, K, Kp, Kl, do_km, do_ot, out2, work, chunk);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// Forward AND the gradient for given seeds in one launch; -95 (not supported: use forward + backward) unless the batch takes
// the kernel's fast path in one chunk.
int spadot_cluster_losses_fb(const float *z, const long long *labels_all, const long long *seed_ids, const float *centres,
                             const float *prev_centres, const float *gamma, const long long *cluster_list, int b, int D, int K,
                             int Kp, int Kl, int do_km, int do_ot, const float *g_km, const float *g_ot, float *out2,
                             float *work, float *dz, void *stream) {
    if (b <= 0 || D <= 0 || K <= 0 || K > CL_MAXK || D > CL_MAXD || !dz) return -22;
    if (do_ot && (Kp <= 0 || Kp > CL_MAXK || Kl <= 0 || Kl > K || !prev_centres || !gamma || !cluster_list)) return -22;
    int chunk = 10240 / D;
    if (chunk > b) chunk = b;
    if (chunk < CL_MAXK) chunk = CL_MAXK;
    chunk = (chunk + 7) / 8 * 8;
    const size_t part = (size_t)(512 / D) * K * (D + 1);
    if (K > CL_KREG || K * D > 512 || chunk < b || part < 2 * (size_t)K * D + (do_ot ? (size_t)Kp * Kl : 0)) return -95;
    const size_t lds = sizeof(float) * (size_t)chunk * D + sizeof(int) * (size_t)chunk + sizeof(float) * part;
    if (lds > (size_t)CL_MAX_DYN_LDS) return -95;
    static PerDeviceFlag attr_set;     
    if (!attr_set) { (void)hipFuncSetAttribute((const void *)k_cluster_losses_fwd<true>, hipFuncAttributeMaxDynamicSharedMemorySize, CL_MAX_DYN_LDS); attr_set = true; }
    hipLaunchKernelGGL(k_cluster_losses_fwd<true>, dim3(1), dim3(512), lds, (hipStream_t)stream, z, labels_all, seed_ids, centres,
                       prev_centres, gamma, cluster_list, b, D, K, Kp, Kl, do_km, do_ot, out2, work, chunk, g_km, g_ot, dz);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_cluster_losses_backward(const float *z, const float *centres, const float *prev_centres, const float *gamma,
                                   const long long *cluster_list, const float *work, const float *g_km,
                                   const float *g_ot, int b, int D, int K, int Kp, int Kl, int do_km, int do_ot,
                                   float *dz, void *stream) {
    if (b <= 0 || D <= 0 || K <= 0 || K > CL_MAXK || D > CL_MAXD) return -22;
    hipLaunchKernelGGL(k_cluster_losses_bwd, dim3(1), dim3(512), 0, (hipStream_t)stream, z, centres, prev_centres, gamma,
                       cluster_list, work, g_km, g_ot, b, D, K, Kp, Kl, do_km, do_ot, dz);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_mix_losses_forward(const float *const *terms6, const float *w6, float *out7, void *stream) {
    if (!terms6 || !w6 || !out7) return -22;
    hipLaunchKernelGGL(k_mix_losses_fwd, dim3(1), dim3(64), 0, (hipStream_t)stream, terms6[0], terms6[1], terms6[2],
                       terms6[3], terms6[4], terms6[5], w6, out7);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_mix_losses_backward(const float *g_elbo, const float *w6, float *g6, void *stream) {
    hipLaunchKernelGGL(k_mix_losses_bwd, dim3(1), dim3(64), 0, (hipStream_t)stream, g_elbo, w6, g6);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_sqerr_forward(const void *y, const void *yhat, long long count, double inv_scale, int dtype,
                         double *scratch, void *out1, void *stream) {
    if (count <= 0 || !scratch) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    const int nb = (int)((count + 255) / 256 < 2048 ? (count + 255) / 256 : 2048);
    FP_DISPATCH(dtype,
                { hipLaunchKernelGGL(k_sqerr_part<float>, dim3(nb), dim3(256), 0, st_, (const float *)y, (const float *)yhat, count, scratch);
                  hipLaunchKernelGGL(k_final_sum<float>, dim3(1), dim3(1024), 0, st_, scratch, nb, inv_scale, (float *)out1); },
                { hipLaunchKernelGGL(k_sqerr_part<double>, dim3(nb), dim3(256), 0, st_, (const double *)y, (const double *)yhat, count, scratch);
                  hipLaunchKernelGGL(k_final_sum<double>, dim3(1), dim3(1024), 0, st_, scratch, nb, inv_scale, (double *)out1); });
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_sqerr_backward(const void *g1, const void *y, const void *yhat, long long count, double inv_scale,
                          int dtype, void *g_yhat, void *stream) {
    if (count <= 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    const int nb = (int)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
    FP_DISPATCH(dtype,
                hipLaunchKernelGGL(k_sqerr_bwd<float>, dim3(nb), dim3(256), 0, st_, (const float *)g1, (const float *)y, (const float *)yhat, count, inv_scale, (float *)g_yhat),
                hipLaunchKernelGGL(k_sqerr_bwd<double>, dim3(nb), dim3(256), 0, st_, (const double *)g1, (const double *)y, (const double *)yhat, count, inv_scale, (double *)g_yhat));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_kmeans_assign(const void *x, const void *centers, int n, int k, int d, int dtype, int *labels,
                         void *stream) {
    if (n <= 0 || k <= 0 || d <= 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    dim3 g((n + 255) / 256);
    FP_DISPATCH(dtype,
                hipLaunchKernelGGL(k_kmeans_assign<float>, g, dim3(256), 0, st_, (const float *)x, (const float *)centers, n, k, d, labels),
                hipLaunchKernelGGL(k_kmeans_assign<double>, g, dim3(256), 0, st_, (const double *)x, (const double *)centers, n, k, d, labels));
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_sgemm_small(int mode, const float *A, int lda, const float *B, int ldb, float *C, int ldc, int M, int N, int K,
                       const float *bias, int batch, long long strideA, long long strideB, long long strideC, void *stream) {
    if (mode < 0 || mode > 2 || !A || !B || !C || M <= 0 || N <= 0 || K <= 0 || ldc < N) return -22;
    if ((mode == 2 ? lda < M : lda < K) || (mode == 1 ? ldb < K : ldb < N)) return -22;
    if (batch < 1 || batch > 65535 || strideA < 0 || strideB < 0 || strideC < 0) return -22;
    const dim3 grid((unsigned)((N + 31) / 32), (unsigned)((M + 31) / 32), (unsigned)batch);
    if (grid.y > 65535u) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    if (mode == 0) hipLaunchKernelGGL(k_sgemm_small<0>, grid, dim3(256), 0, st_, A, lda, B, ldb, C, ldc, M, N, K, bias, strideA, strideB, strideC);
    else if (mode == 1) hipLaunchKernelGGL(k_sgemm_small<1>, grid, dim3(256), 0, st_, A, lda, B, ldb, C, ldc, M, N, K, bias, strideA, strideB, strideC);
    else hipLaunchKernelGGL(k_sgemm_small<2>, grid, dim3(256), 0, st_, A, lda, B, ldb, C, ldc, M, N, K, bias, strideA, strideB, strideC);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_stamp(unsigned long long *buf, int slot, void *stream) {
    if (!buf || slot < 0) return -22;
    hipLaunchKernelGGL(k_stamp, dim3(1), dim3(64), 0, (hipStream_t)stream, buf, slot);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_knn(const double *x, int n, int d, int kk, int *out, void *stream) {
    if (n <= 0 || d <= 0 || d > KNN_MAXD || kk <= 0 || kk > n || kk > 128) return -22;
    const size_t lds = sizeof(double) * KNN_T * KNN_MAXD + (sizeof(double) + sizeof(int)) * (size_t)kk * KNN_T;
    static PerDeviceFlag attr_set;     
    if (!attr_set) { (void)hipFuncSetAttribute((const void *)k_knn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr_set = true; }
    hipLaunchKernelGGL(k_knn, dim3((n + KNN_T - 1) / KNN_T), dim3(KNN_T), lds, (hipStream_t)stream, x, n, d, kk, out);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_lloyd_step(const double *X, double *C, const int *xoff, const int *npts, int n_max, int R, const int *rgroup,
                      const int *Kr, int K_max, int D, const double *tol, double *part, int *done, double *inertia, int skip_done,
                      void *stream) {
    if (n_max <= 0 || R <= 0 || R > 65535 || D <= 0 || D > LL_MAXD || K_max <= 0 || K_max > LL_MAXK) return -22;
    if (!X || !C || !xoff || !npts || !rgroup || !Kr || !tol || !part || !done || !inertia) return -22;
    if ((size_t)K_max * D + (size_t)LL_PTS * D > 7936) return -22;     // dynamic LDS stays under 62 KB
    hipStream_t st_ = (hipStream_t)stream;
    const int nchunk = (n_max + LL_PTS - 1) / LL_PTS;
    const size_t lds = sizeof(double) * ((size_t)K_max * D + (size_t)LL_PTS * D);      // <= 8 KB + 64 KB
    hipLaunchKernelGGL(k_lloyd_assign, dim3(nchunk, R), dim3(LL_PTS), lds, st_, X, (const double *)C, D, K_max, part, xoff, npts,
                       skip_done ? (const int *)done : (const int *)nullptr, Kr, rgroup);
    hipLaunchKernelGGL(k_lloyd_update, dim3(R), dim3(256), 0, st_, (const double *)part, nchunk, D, K_max, C, done, inertia, npts,
                       tol, skip_done, Kr, rgroup);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_kmeanspp_seed(const double *X, const int *xoff, const int *npts, int D, int P, const int *pset, const int *pK,
                         const int *pfirst, const int *puoff, const double *U, int K_max, int n_max, double *closest, int *idx,
                         double *centers, void *stream) {
    if (P <= 0 || D <= 0 || D > LL_MAXD || K_max <= 0 || K_max > LL_MAXK || n_max <= 0) return -22;
    if (!X || !xoff || !npts || !pset || !pK || !pfirst || !puoff || !U || !closest || !idx || !centers) return -22;
    hipLaunchKernelGGL(k_kmeanspp_seed, dim3(P), dim3(KPP_T), 0, (hipStream_t)stream, X, xoff, npts, D, pset, pK, pfirst, puoff,
                       U, K_max, n_max, closest, idx, centers);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_grad_sumsq(const float *grad, long long count, double *scratch, float *sumsq, void *stream) {
    if (count <= 0 || !scratch) return -22;
    if (((uintptr_t)grad & 15) != 0) return -22;   // float4 path needs 16-byte alignment
    hipStream_t st_ = (hipStream_t)stream;
    const long long want = (count / 4 + 255) / 256;
    const int nb = (int)(want < 1 ? 1 : (want < 2048 ? want : 2048));
    hipLaunchKernelGGL(k_sumsq_part, dim3(nb), dim3(256), 0, st_, grad, count, scratch);
    hipLaunchKernelGGL(k_final_sum<float>, dim3(1), dim3(1024), 0, st_, scratch, nb, 1.0, sumsq);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_adamw_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const float *sumsq,
                          long long count, double lr, double beta1, double beta2, double eps, double weight_decay,
                          double max_norm, int *step_dev, void *stream) {
    if (count <= 0 || !step_dev) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    const long long want = (count + 255) / 256;
    const int nb = (int)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, st_, step_dev);
    hipLaunchKernelGGL(k_adamw, dim3(nb), dim3(256), 0, st_, param, grad, exp_avg, exp_avg_sq, sumsq, count,
                       (float)lr, (float)beta1, (float)beta2, (float)eps, (float)weight_decay, (float)max_norm,
                       1.f, 1.f, (const int *)step_dev, (const float *)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_clip_adamw_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long count, double lr,
                          double beta1, double beta2, double eps, double weight_decay, double max_norm, double *scratch,
                          float *sumsq, int *step_dev, unsigned *counter, const float *grad_scale_dev, void *stream) {
    if (count <= 0 || !step_dev || !scratch || !sumsq || !counter) return -22;
    if (((uintptr_t)grad & 15) != 0) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    const long long want4 = (count / 4 + 255) / 256;
    // 512 workgroups: every workgroup ends with an agent-scope release (L2 write-back) before its counter add, so
    // the launch got SLOWER with more of them (2048: 56 us, 512: 31 us for 64 MB; tools/adamw_bench.py)
    const int nbs = (int)(want4 < 1 ? 1 : (want4 < 512 ? want4 : 512));
    // 0: the one-launch form (same-box A/B: 1.972 -> 1.941 ms per step with 2048); clamped to the scratch buffer's
    // capacity (FlatAdamW.scratch: 4096 doubles, one partial per workgroup)
    constexpr int split = 2048;
    if (split > 0) {
        const int nb2 = (int)(want4 < 1 ? 1 : (want4 < split ? want4 : split));
        hipLaunchKernelGGL(k_sumsq_part_u<4>, dim3(nb2), dim3(256), 0, st_, grad, count, scratch);
        hipLaunchKernelGGL(k_final_sum_step, dim3(1), dim3(1024), 0, st_, (const double *)scratch, nb2, sumsq, step_dev);
    } else
        hipLaunchKernelGGL(k_sumsq_last<4>, dim3(nbs), dim3(256), 0, st_, grad, count, scratch, sumsq, step_dev, counter);
    const long long want = (count + 255) / 256;
    const int nb = (int)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(k_adamw, dim3(nb), dim3(256), 0, st_, param, grad, exp_avg, exp_avg_sq, (const float *)sumsq, count,
                       (float)lr, (float)beta1, (float)beta2, (float)eps, (float)weight_decay, (float)max_norm,
                       1.f, 1.f, (const int *)step_dev, grad_scale_dev);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_clip_adamw_images_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long count, double lr,
                                 double beta1, double beta2, double eps, double weight_decay, double max_norm, double *scratch,
                                 float *sumsq, int *step_dev, const float *grad_scale_dev, const spadot_weight_images *images,
                                 void *stream) {
    if (count <= 0 || (count & 3) || !step_dev || !scratch || !sumsq || !images) return -22;
    if (((uintptr_t)grad & 15) || ((uintptr_t)param & 15) || ((uintptr_t)exp_avg & 15) || ((uintptr_t)exp_avg_sq & 15)) return -22;
    if (images->n < 0 || images->n > 8) return -22;
    for (int s_ = 0; s_ < images->n; s_++) {
        const spadot_weight_image &W = images->w[s_];
        if (!W.image || ((uintptr_t)W.image & 7) || W.rows <= 0 || W.K <= 0 || (W.K & 3) || W.Kp < W.K || (W.Kp & 3) || (W.offset & 3) ||
            W.offset < 0 || W.offset + (long long)W.rows * W.K > count || (long long)W.rows * W.K >= (1ll << 31))
            return -22;
    }
    hipStream_t st_ = (hipStream_t)stream;
    const long long want4 = (count / 4 + 255) / 256;
    const int nb2 = (int)(want4 < 1 ? 1 : (want4 < 2048 ? want4 : 2048));
    hipLaunchKernelGGL(k_sumsq_part_u<4>, dim3(nb2), dim3(256), 0, st_, grad, count, scratch);
    hipLaunchKernelGGL(k_final_sum_step, dim3(1), dim3(1024), 0, st_, (const double *)scratch, nb2, sumsq, step_dev);
    const int nb = (int)(want4 < 4096 ? want4 : 4096);
    hipLaunchKernelGGL(k_adamw_img, dim3(nb), dim3(256), 0, st_, param, grad, exp_avg, exp_avg_sq, (const float *)sumsq, count,
                       (float)lr, (float)beta1, (float)beta2, (float)eps, (float)weight_decay, (float)max_norm,
                       (const int *)step_dev, grad_scale_dev, *images, 0ll);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// The two halves of spadot_clip_adamw_images_dev as entry points of their own, so that a caller can update a RANGE of the
// flat buffer first (and let whoever needs only those parameters start) and the rest afterwards: the same launches, the
// same arithmetic per element -- bit-identical parameters whatever the split.
int spadot_grad_norm_step_dev(const float *grad, long long count, double *scratch, float *sumsq, int *step_dev, void *stream) {
    if (count <= 0 || !scratch || !sumsq || !step_dev || ((uintptr_t)grad & 15)) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    const long long want4 = (count / 4 + 255) / 256;
    const int nb2 = (int)(want4 < 1 ? 1 : (want4 < 2048 ? want4 : 2048));
    hipLaunchKernelGGL(k_sumsq_part_u<4>, dim3(nb2), dim3(256), 0, st_, grad, count, scratch);
    hipLaunchKernelGGL(k_final_sum_step, dim3(1), dim3(1024), 0, st_, (const double *)scratch, nb2, sumsq, step_dev);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_adamw_range_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long offset, long long count,
                           double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                           const float *sumsq, const int *step_dev, const float *grad_scale_dev, const spadot_weight_images *images,
                           void *stream) {
    if (offset < 0 || count <= 0 || (offset & 3) || (count & 3) || !step_dev || !sumsq) return -22;
    if (((uintptr_t)grad & 15) || ((uintptr_t)param & 15) || ((uintptr_t)exp_avg & 15) || ((uintptr_t)exp_avg_sq & 15)) return -22;
    spadot_weight_images none;
    none.n = 0;
    const spadot_weight_images *tab = images ? images : &none;
    if (tab->n < 0 || tab->n > 8) return -22;
    for (int s_ = 0; s_ < tab->n; s_++) {
        const spadot_weight_image &W = tab->w[s_];
        if (!W.image || ((uintptr_t)W.image & 7) || W.rows <= 0 || W.K <= 0 || (W.K & 3) || W.Kp < W.K || (W.Kp & 3) || (W.offset & 3) ||
            W.offset < 0 || (long long)W.rows * W.K >= (1ll << 31))
            return -22;
    }
    hipStream_t st_ = (hipStream_t)stream;
    // SPADOT_ADAMW_MAX_WGS (default 512; 4096 until round 4): workgroups of the streaming update.  Two 256-thread workgroups per
    // compute unit stream as fast as sixteen (80 us for the 483 MB of cfg3 either way) and leave the wave slots to what runs
    // beside the update -- the next step's SVGP encoder, chained to the update's first part: 619.6 / 620.5 -> 624.5 / 627.3
    // steps/s (same box; 256 workgroups: 617)
    constexpr long long max_wgs = 512;
    const long long want4 = (count / 4 + 255) / 256;
    const int nb = (int)(want4 < max_wgs ? want4 : max_wgs);
    hipLaunchKernelGGL(k_adamw_img, dim3(nb), dim3(256), 0, st_, param + offset, grad + offset, exp_avg + offset, exp_avg_sq + offset,
                       sumsq, count, (float)lr, (float)beta1, (float)beta2, (float)eps, (float)weight_decay, (float)max_norm,
                       step_dev, grad_scale_dev, *tab, offset);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int spadot_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const float *sumsq,
                      long long count, double lr, double beta1, double beta2, double eps, double weight_decay,
                      double max_norm, int step, void *stream) {
    if (count <= 0 || step < 1) return -22;
    hipStream_t st_ = (hipStream_t)stream;
    const long long want = (count + 255) / 256;
    const int nb = (int)(want < 4096 ? want : 4096);
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    hipLaunchKernelGGL(k_adamw, dim3(nb), dim3(256), 0, st_, param, grad, exp_avg, exp_avg_sq, sumsq, count,
                       (float)lr, (float)beta1, (float)beta2, (float)eps, (float)weight_decay, (float)max_norm,
                       (float)bc1, (float)sqrt(bc2), (const int *)nullptr, (const float *)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
