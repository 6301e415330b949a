// The chip's float64 FMA rate by a plain loop of independent FMAs, as a shared library so that a Python tool can measure it
// in its own process (tools/region_xcorr_bench.py loads it through ctypes and builds it when it is missing):
//   hipcc -O3 --offload-arch=gfx950 -shared -fPIC tools/fma_f64_probe.hip -o tools/_ab/libfma_f64_probe.so
// Every thread keeps 16 accumulators that do not depend on each other, so the latency of one v_fma_f64 is covered sixteen
// times over; the caller's workgroups of 256 threads fill every SIMD with several waves.  The figure is FMAs per second (one FMA = one
// multiply-add = 2 flops), the fastest of `rounds` launches.
#include <hip/hip_runtime.h>

namespace {

constexpr int ACC = 16;

__global__ __launch_bounds__(256) void fma_loop(int iters, double seed, double *out)
{
    double a[ACC];
    const double x = 1.0 + 1e-9 * seed, y = 1e-12 * (threadIdx.x + 1);
#pragma unroll
    for (int k = 0; k < ACC; k++) a[k] = seed + k;
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int k = 0; k < ACC; k++) a[k] = fma(a[k], x, y);
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < ACC; k++) s += a[k];
    if (s == 12345.678) out[0] = s;                     // never true: keeps the loop alive without a store per thread
}

}  // namespace

extern "C" int fma_f64_probe(int blocks, int iters, int rounds, double *fma_per_second)
{
    double *out = nullptr;
    hipEvent_t e0, e1;
    if (hipMalloc(&out, sizeof(double)) != hipSuccess) return 1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 1;
    hipLaunchKernelGGL(fma_loop, dim3(blocks), dim3(256), 0, 0, iters, 1.0, out);
    float best = 1e30f;
    for (int r = 0; r < rounds; r++) {
        (void)hipEventRecord(e0, 0);
        hipLaunchKernelGGL(fma_loop, dim3(blocks), dim3(256), 0, 0, iters, 1.0, out);
        (void)hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess) return 1;
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        best = ms < best ? ms : best;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(out);
    *fma_per_second = (double)blocks * 256.0 * (double)iters * ACC / (best * 1e-3);
    return 0;
}
