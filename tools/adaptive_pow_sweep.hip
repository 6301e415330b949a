// The error of the device library's float64 pow() over the arguments hipdsp_spec_adapt's PCEN mode can reach, against
// powl() of the host (64-bit mantissa: the comparison resolves 2^-11 ulp of a double).  The one constant of the PCEN
// bound that cannot be derived (tests/adaptive_spectrogram_definition.py: POW_W); the log is
// profiles/adaptive_spectrogram_bound.log.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/adaptive_pow_sweep.hip -o tools/build/adaptive_pow_sweep
//   tools/build/adaptive_pow_sweep [samples per binade = 4096]
// Bases: every binade 2^-149 ... 2^277 (eps + M of float32 inputs: 2^-149 ... 2^128; G + bias reaches 2^128/2^-149);
// per binade the two ends, the neighbours of the ends and `samples` random mantissas.  One line per exponent: the worst
// error in units of w = 2^-53 relative to the true value (one ulp is between w and 2 w), and where.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

__global__ void pow_kernel(const double *base, double e, double *out, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pow(base[i], e);
}

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        hipError_t err_ = (x);                                                                    \
        if (err_ != hipSuccess) {                                                                 \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(err_));                             \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)

int main(int argc, char **argv)
{
    const int samples = argc > 1 ? atoi(argv[1]) : 4096;
    std::mt19937_64 rng(20261021);
    std::vector<double> base;
    for (int b = -149; b <= 277; b++) {
        const double lo = ldexp(1.0, b);
        base.push_back(lo);
        base.push_back(nextafter(lo, 2.0 * lo));
        base.push_back(nextafter(2.0 * lo, lo));
        for (int i = 0; i < samples; i++) base.push_back(ldexp(1.0 + (double)(rng() >> 11) * 0x1p-53, b));
    }
    const long long n = (long long)base.size();
    double *dbase = nullptr, *dout = nullptr;
    CHECK(hipMalloc(&dbase, n * sizeof(double)));
    CHECK(hipMalloc(&dout, n * sizeof(double)));
    CHECK(hipMemcpy(dbase, base.data(), n * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double> got(n);
    const double exps[] = {0.98, 0.5, 0.25, 1.0 / 3.0, 0.9, 2.0, 1e-3, 1.0};
    printf("float64 pow() of the device library against powl(): %lld bases, binades 2^-149 ... 2^277, %d random "
           "mantissas each\n", n, samples);
    double worst_all = 0.0;
    for (double e : exps) {
        hipLaunchKernelGGL(pow_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dbase, e, dout, n);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(got.data(), dout, n * sizeof(double), hipMemcpyDeviceToHost));
        double worst = 0.0, at = 0.0;
        long long nonfinite = 0;
        for (long long i = 0; i < n; i++) {
            const long double want = powl((long double)base[i], (long double)e);
            if (!(fabsl(want) <= 1.7976931348623157e308L) || want < 2.2250738585072014e-308L) continue;     // double's normal range
            if (!std::isfinite(got[i])) { nonfinite++; continue; }
            const double err = (double)(fabsl((long double)got[i] - want) / want) * 0x1p53;
            if (err > worst) worst = err, at = base[i];
        }
        printf("exponent %-22.17g worst %.4f w at base %a%s\n", e, worst, at, nonfinite ? "  NON-FINITE RESULTS" : "");
        if (nonfinite) printf("  %lld non-finite results where powl() is a normal double\n", nonfinite);
        if (worst > worst_all) worst_all = worst;
    }
    printf("worst of all exponents: %.4f w (w = 2^-53; 4 ulp of the working precision is 4 ... 8 w)\n", worst_all);
    CHECK(hipFree(dbase));
    CHECK(hipFree(dout));
    return 0;
}
