// hipdsp_spec_adapt: the adaptive normalisation of a spectrogram slab -- a running noise floor per bin and the slab
// divided by it, reduced by it, or compressed as per-channel energy normalisation (PCEN); the contract is in
// include/hip_dsp.h.
//
// The floor of one column (channel c, bin k) is the first-order smoother M_0 = x_0, M_t = a M_(t-1) + s x_t along TIME,
// the slow axis of the planar slab (channels, frames, nfreq): the values of a column lie nfreq floats apart, the columns
// of neighbouring bins are contiguous.  So the lanes run along the bins -- lane l of a wave owns column tile*64 + l, a
// row of the wave is one coalesced 256-byte read -- and time is serial per lane, the state in float64.  Time becomes
// parallel by chunks of HIPDSP_ADAPT_CHUNK = 256 frames counted from frame 0 (a function of `frames` alone) with an
// exact hand-over, three launches:
//   ad_summary   one wave per (channel, 64 bins, chunk) except the last chunk: the chunk's end value from ZERO state (chunk
//                0: from M_0 = x_0, its true state) into the context scratch, float64, [channel][chunk][bin].
//   ad_carry     one lane per column, serial over the chunks: M' = a^256 M + v in float64 replaces every v by the state
//                that ENTERS the next chunk.  a^256 comes from the host (long double, rounded once) by value.
//   ad_apply     the chunks that reach behind nbefore again: the recursion from the true entering state, the mode's
//                formula in float64, ONE rounding to float32, the store.  A lane reads a row's element before it writes
//                it, and nobody else touches that element: out may be spec itself.
// Ordering comes from the launches alone; no kernel waits for another workgroup, there are no atomics, every scalar
// travels by value.  AD_ROWS rows of loads are in flight per lane (4 KiB per wave: eight resident waves per CU hold
// the 32 KiB a CU needs to stream from HBM).  Rows start at any 4-byte address (nfreq = 1025: 4100-byte rows), so the
// accesses are dwords: a 16-byte access would need a row phase that is the same for every row.
#include <cmath>
#include "common.h"

namespace {

constexpr int AD_CHUNK = HIPDSP_ADAPT_CHUNK;
constexpr int AD_ROWS = 16;                          // rows of loads in flight per lane
constexpr long long AD_MAX_ELEMS = 1LL << 44;        // elements of a channel or a pitch, as in hipdsp_spec_equalize
static_assert(AD_CHUNK % AD_ROWS == 0, "a chunk is whole batches of rows");

struct AdArgs {                                      // by value in the kernel arguments
    const float *spec;
    float *out;
    long long spec_pitch, out_pitch, frames, nbefore, n_chunks, bin_tiles;
    int nfreq;
    double a, s, a_chunk;                            // 1 - smooth, smooth, a^AD_CHUNK
    double gain, bias, power, eps;
    double *carry;                                   // [channel][chunk < n_chunks - 1][bin]
};

// Runs the smoother of one lane's column over the rows [t0, t1) of its chunk, AD_ROWS loads in flight; `first` (chunk
// 0): row t0 IS the state.  use(t, x, M) sees every row with its floor.
template <typename Use>
__device__ __forceinline__ double ad_run(const float *p, long long row_stride, long long t0, long long t1, bool first,
                                         double M, double a, double s, Use use)
{
    for (long long t = t0; t < t1; t += AD_ROWS) {
        float x[AD_ROWS];
        // (rows behind the chunk's end repeat its last row and are not run)
#pragma unroll
        for (int u = 0; u < AD_ROWS; u++) {
            const long long r = t + u < t1 ? t + u : t1 - 1;
            x[u] = p[r * row_stride];
        }
#pragma unroll
        for (int u = 0; u < AD_ROWS; u++) {
            if (t + u < t1) {
                const double v = (double)x[u];
                M = (first && t + u == t0) ? v : a * M + s * v;
                use(t + u, v, M);
            }
        }
    }
    return M;
}

__global__ __launch_bounds__(64) void ad_summary(const AdArgs g)
{
    const int lane = threadIdx.x;
    const long long c = blockIdx.y, tile = blockIdx.x % g.bin_tiles, j = blockIdx.x / g.bin_tiles;
    const long long k = tile * 64 + lane;
    const bool live = k < g.nfreq;
    const float *p = g.spec + c * g.spec_pitch + (live ? k : tile * 64);
    const long long t0 = j * AD_CHUNK;                // (the last chunk has no summary: t0 + AD_CHUNK <= frames)
    const double v = ad_run(p, g.nfreq, t0, t0 + AD_CHUNK, j == 0, 0.0, g.a, g.s, [](long long, double, double) {});
    if (live) g.carry[(c * (g.n_chunks - 1) + j) * g.nfreq + k] = v;
}

__global__ __launch_bounds__(256) void ad_carry(const AdArgs g)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (k >= g.nfreq) return;
    double *v = g.carry + c * (g.n_chunks - 1) * g.nfreq + k;
    const long long n = g.n_chunks - 1, stride = g.nfreq;
    double M = 0.0;                                   // chunk 0's summary is its true end state: a^256 * 0 + v
    long long j = 0;
    for (; j + 8 <= n; j += 8) {
        double z[8];
#pragma unroll
        for (int u = 0; u < 8; u++) z[u] = v[(j + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            M = g.a_chunk * M + z[u];
            v[(j + u) * stride] = M;
        }
    }
    for (; j < n; j++) {
        M = g.a_chunk * M + v[j * stride];
        v[j * stride] = M;
    }
}

template <int MODE>
__device__ __forceinline__ float ad_value(const AdArgs &g, double bias_pow, double x, double M)
{
    if constexpr (MODE == HIPDSP_ADAPT_BACKGROUND) {
        return (float)M;
    } else if constexpr (MODE == HIPDSP_ADAPT_DIVIDE) {
        return (float)(x / (g.eps + M));
    } else if constexpr (MODE == HIPDSP_ADAPT_SUBTRACT) {
        const double d = x - M;
        return (float)(d < 0.0 ? 0.0 : d);            // (NaN stays NaN: the comparison is false)
    } else {
        const double G = x / pow(g.eps + M, g.gain);
        return (float)(pow(G + g.bias, g.power) - bias_pow);
    }
}

// (spec and out may be the same array: no __restrict__ on them)
template <int MODE>
__global__ __launch_bounds__(64) void ad_apply(const AdArgs g)
{
    const int lane = threadIdx.x;
    const long long c = blockIdx.y, tile = blockIdx.x % g.bin_tiles;
    const long long j = g.nbefore / AD_CHUNK + blockIdx.x / g.bin_tiles;      // the first chunk that reaches behind nbefore
    const long long k = tile * 64 + lane;
    const bool live = k < g.nfreq;
    const long long col = live ? k : tile * 64;
    const float *p = g.spec + c * g.spec_pitch + col;
    float *o = g.out + c * g.out_pitch + col;
    const long long t0 = j * AD_CHUNK;
    const long long t1 = t0 + AD_CHUNK < g.frames ? t0 + AD_CHUNK : g.frames;
    const double M0 = j == 0 ? 0.0 : g.carry[(c * (g.n_chunks - 1) + (j - 1)) * g.nfreq + col];
    const long long nbefore = g.nbefore, stride = g.nfreq;
    // bias^power by the same pow() as the elements': a zero frame (G = 0) gives exactly 0
    const double bias_pow = MODE == HIPDSP_ADAPT_PCEN ? pow(g.bias, g.power) : 0.0;
    ad_run(p, stride, t0, t1, j == 0, M0, g.a, g.s, [&](long long t, double x, double M) {
        if (live && t >= nbefore) o[(t - nbefore) * stride] = ad_value<MODE>(g, bias_pow, x, M);
    });
}

template <int MODE>
int ad_launch_apply(hipdsp_ctx *ctx, const AdArgs &g, const dim3 &grid)
{
    hipLaunchKernelGGL((ad_apply<MODE>), grid, dim3(64), 0, ctx->stream, g);
    return hd_launch_status("ad_apply");
}

}  // namespace

extern "C" int hipdsp_spec_adapt(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, float *out, int64_t out_pitch,
                                 int64_t channels, int64_t frames, int64_t nfreq, int64_t nbefore, double smooth, int mode,
                                 double gain, double bias, double power, double eps)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(channels >= 0 && frames >= 0 && nfreq >= 0 && spec_pitch >= 0 && out_pitch >= 0, "negative size");
    HD_REQUIRE(mode >= HIPDSP_ADAPT_BACKGROUND && mode <= HIPDSP_ADAPT_PCEN, "unknown mode %d", mode);
    HD_REQUIRE(smooth > 0.0 && smooth <= 1.0, "smooth must lie in (0, 1], got %g", smooth);
    const double huge = 1.7976931348623157e308;
    if (mode == HIPDSP_ADAPT_DIVIDE || mode == HIPDSP_ADAPT_PCEN)
        HD_REQUIRE(eps > 0.0 && eps <= huge, "eps must be a positive finite number, got %g", eps);
    if (mode == HIPDSP_ADAPT_PCEN)
        HD_REQUIRE(gain >= 0.0 && gain <= 1.0 && bias >= 0.0 && bias <= huge && power > 0.0 && power <= huge,
                   "PCEN needs 0 <= gain <= 1, bias >= 0 and power > 0 (finite), got %g, %g and %g", gain, bias, power);
    HD_REQUIRE(nbefore >= 0 && nbefore <= frames, "nbefore %lld not inside [0, %lld]", (long long)nbefore, (long long)frames);
    HD_REQUIRE(nfreq < (1LL << 30), "nfreq out of range");
    if (channels > 65535) {
        hipdsp_set_error("at most 65535 channels per call, got %lld", (long long)channels);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    HD_REQUIRE((nfreq == 0 || frames <= AD_MAX_ELEMS / nfreq) && spec_pitch <= AD_MAX_ELEMS && out_pitch <= AD_MAX_ELEMS,
               "frames * nfreq or a pitch out of range");
    const long long total = frames * nfreq, out_total = (frames - nbefore) * nfreq;
    if (spec_pitch == 0) spec_pitch = total;
    if (out_pitch == 0) out_pitch = out_total;
    HD_REQUIRE(spec_pitch >= total && out_pitch >= out_total, "a slab pitch is smaller than one channel");
    if (channels == 0 || out_total == 0) return HIPDSP_OK;
    HD_REQUIRE(spec != nullptr && out != nullptr, "NULL data pointer");
    HD_REQUIRE(((uintptr_t)spec & 3) == 0 && ((uintptr_t)out & 3) == 0, "misaligned pointer");
    HD_REQUIRE((out == spec && out_pitch == spec_pitch && nbefore == 0) ||
               !hd_planar_overlap(spec, spec_pitch, total, out, out_pitch, out_total, channels),
               "out must be spec itself (same pitch, nbefore 0) or not overlap it");

    AdArgs g;
    memset(&g, 0, sizeof(g));
    g.spec = spec, g.out = out, g.spec_pitch = spec_pitch, g.out_pitch = out_pitch, g.frames = frames, g.nbefore = nbefore;
    g.nfreq = (int)nfreq;
    g.n_chunks = (frames + AD_CHUNK - 1) / AD_CHUNK;
    g.bin_tiles = (nfreq + 63) / 64;
    g.s = smooth, g.a = 1.0 - smooth;
    // a^256 of the double a the kernels use, in long double, rounded once; where it underflows it is the smallest
    // positive double, so that an infinite floor stays infinite as it does step by step (0 * inf would be NaN)
    g.a_chunk = (double)powl((long double)g.a, (long double)AD_CHUNK);
    if (g.a > 0.0 && g.a_chunk == 0.0) g.a_chunk = 4.9406564584124654e-324;
    g.gain = gain, g.bias = bias, g.power = power, g.eps = eps;
    const long long first_chunk = nbefore / AD_CHUNK;
    HD_REQUIRE(g.n_chunks * g.bin_tiles <= 0x7fffffffLL, "too many (chunk, 64 bins) tiles for one call");

    HD_CHECK_HIP(hipSetDevice(ctx->device));
    if (g.n_chunks > 1) {
        // (refuses a scratch that would have to grow during a capture or under captured graphs: hipdsp_ctx_reserve first)
        void *work = nullptr;
        const int rc = hipdsp_scratch(ctx, (size_t)channels * (size_t)(g.n_chunks - 1) * (size_t)nfreq * sizeof(double), &work);
        if (rc != HIPDSP_OK) return rc;
        g.carry = (double *)work;
        hipLaunchKernelGGL(ad_summary, dim3((unsigned)((g.n_chunks - 1) * g.bin_tiles), (unsigned)channels), dim3(64), 0,
                           ctx->stream, g);
        int st = hd_launch_status("ad_summary");
        if (st != HIPDSP_OK) return st;
        hipLaunchKernelGGL(ad_carry, dim3((unsigned)((nfreq + 255) / 256), (unsigned)channels), dim3(256), 0, ctx->stream, g);
        st = hd_launch_status("ad_carry");
        if (st != HIPDSP_OK) return st;
    }
    const dim3 grid((unsigned)((g.n_chunks - first_chunk) * g.bin_tiles), (unsigned)channels);
    switch (mode) {
    case HIPDSP_ADAPT_BACKGROUND: return ad_launch_apply<HIPDSP_ADAPT_BACKGROUND>(ctx, g, grid);
    case HIPDSP_ADAPT_DIVIDE: return ad_launch_apply<HIPDSP_ADAPT_DIVIDE>(ctx, g, grid);
    case HIPDSP_ADAPT_SUBTRACT: return ad_launch_apply<HIPDSP_ADAPT_SUBTRACT>(ctx, g, grid);
    default: return ad_launch_apply<HIPDSP_ADAPT_PCEN>(ctx, g, grid);
    }
}
