// What v_mfma_f64_16x16x4_f64 sustains on this chip: back-to-back issue, four independent accumulators per wavefront, one or two
// wavefronts per SIMD on every compute unit.  The denominator of the Time paragraph of DESIGN 7m (tools/modules_time.py
// --peak-tflops).     hipcc -O3 --offload-arch=gfx950 tools/mfma_f64_peak.hip -o /tmp/mfma_f64_peak && /tmp/mfma_f64_peak
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int ITERS = 1 << 16;
__global__ void __launch_bounds__(256) peak(double *out, double a, double b) {
    d4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
    const double x = a + threadIdx.x * 1e-9, y = b - threadIdx.x * 1e-9;
    for (int i = 0; i < ITERS; ++i) {
        c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(y, x, c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, c2, 0, 0, 0);
        c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(y, y, c3, 0, 0, 0);
    }
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = c0[0] + c1[1] + c2[2] + c3[3];
}
int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 1;
    const int cus = p.multiProcessorCount;
    double *out;
    if (hipMalloc(&out, (size_t)cus * 2 * 256 * 8) != hipSuccess) return 1;
    for (int per = 1; per <= 2; ++per) {                                 // workgroups of four wavefronts per compute unit
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        hipLaunchKernelGGL(peak, dim3(cus * per), dim3(256), 0, 0, out, 1.0, 0.5);
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(peak, dim3(cus * per), dim3(256), 0, 0, out, 1.0, 0.5);
        (void)hipEventRecord(e1);
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        const double flop = 2.0 * 16 * 16 * 4 * 4.0 * ITERS * 4.0 * cus * per;
        printf("{\"what\": \"mfma_f64_peak\", \"compute_units\": %d, \"waves_per_simd\": %d, \"ms\": %.3f, \"tflops\": %.2f}\n", cus, per, ms,
               flop / (ms * 1e-3) / 1e12);
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
