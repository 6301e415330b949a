// hipdsp_spectral_features: per frame and channel of a planar spectrogram slab, where the power inside a band of bins
// sits in frequency -- peak bin, interpolated peak, peak power, centroid, bandwidth, flatness (Wiener entropy) and the
// band's extent above a fraction of the peak (include/hip_dsp.h has the definitions).
//
// A sibling of hipdsp_band_power in data flow (a strided row-segment reduction over (channels, frames, nfreq)
// float32, only the bins of the band are read), but every row needs two passes: the peak first, then the moments, the
// extents and the logarithms ABOUT it.  Between the passes the band of the row stays in LDS, so a bin comes from HBM
// once; only a band wider than a workgroup's LDS row (8448 bins) is read a second time.
//
// G threads share a row, thread t owns the bins k = t (mod G) by ABSOLUTE bin index and walks them in ascending
// order; the G partial results meet in a butterfly (__shfl_xor: every lane ends with the same bits) and, for G = 256,
// in LDS in the fixed order (w0 + w1) + (w2 + w3).  G is chosen by nfreq alone, never by the band or the mask:
//
//   nfreq <= 256      G = 8:   a workgroup takes 32 consecutive frames of a channel.  Their bands are contiguous or
//                              nearly so in memory: all 256 threads copy them into an LDS tile with coalesced loads
//                              (row stride n | 1), then 8 lanes work on each frame and the stores run along time.
//   nfreq <= 1056     G = 64:  a wave per frame, four frames per workgroup, 1056 floats of LDS each; a lane's whole
//                              share (at most 17 bins) is loaded before the first is used.
//   nfreq >  1056     G = 256: a workgroup per frame, 8448 floats of LDS.
//
// All arithmetic after the float32 comparisons of the peak search is float64 (-ffp-contract=off: no fused
// multiply-add), every stored value is rounded to float32 once.  log() runs once per bin only for FLATNESS (a template
// flag) and three times per row for PEAK_FREQ; a call that asks for bits 0..2 alone skips the second pass.  What a
// frame stores depends on its own band only: not on its neighbours, the pitches or the other requested features.
// No atomics, no scratch, all arguments by value: one kernel node under hipdsp_graph_begin/end.  Index arithmetic on
// the slab is 64-bit.
#include "common.h"
#include <cmath>

namespace {

constexpr int N_FEATURES = 8;
constexpr int SHORT_NFREQ = 256, WAVE_NFREQ = 1056;
constexpr int SHORT_ROWS = 32;              // frames per workgroup of the short rows' tile
constexpr int LONG_FLOATS = 8448;           // the LDS row of a workgroup per frame: 33 KiB, four workgroups per CU
// floats of LDS per workgroup: 32 rows of up to 257 (33 KiB), four rows of 1056 (16.5 KiB: eight workgroups, all 32 waves
// of a CU), one row of 8448
template <int G> constexpr int lds_floats() { return G == 8 ? SHORT_ROWS * (SHORT_NFREQ + 1) : (G == 64 ? 4 * WAVE_NFREQ : LONG_FLOATS); }
constexpr int NO_BIN = 0x7fffffff;

// np.argmax's order: the first NaN if there is one, else the first of the largest
__device__ __forceinline__ bool peak_better(float v2, int k2, float v1, int k1)
{
    if (k2 == NO_BIN) return false;
    if (k1 == NO_BIN) return true;
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 || n2) return n2 && (!n1 || k2 < k1);
    return v2 > v1 || (v2 == v1 && k2 < k1);
}

template <int G, bool FLAT>
__global__ __launch_bounds__(256) void feat_kernel(const float *__restrict__ spec, long long spec_pitch, long long frames,
                                                   int nfreq, int k0, int k1, unsigned features, double scale,
                                                   double min_power, double drop_ratio, float *__restrict__ out,
                                                   long long out_pitch, long long out_feature_pitch)
{
    constexpr int RPB = 256 / G;                        // rows (frames of one channel) per workgroup
    constexpr int W = G < 64 ? G : 64;                  // lanes of a wave that share a row
    __shared__ float tile[lds_floats<G>()];
    __shared__ float red_v[4];
    __shared__ int red_k[4], red_lo[4], red_hi[4];
    __shared__ double red_d[4][4];
    const int tid = threadIdx.x, t = tid % G, r = tid / G;
    const long long c = blockIdx.y;
    const long long f0 = (long long)blockIdx.x * RPB, f = f0 + r;
    const bool live = f < frames;
    const int n = k1 - k0;
    const int stride = G == 8 ? (n | 1) : lds_floats<G>() / RPB;
    const bool held = n <= stride;                      // the band of a row fits its LDS row (always for G = 8)
    const float *p = spec + c * spec_pitch + (live ? f : f0) * (long long)nfreq;   // the row; only [k0, k1) is read
    const float *band = p + k0;                         // band[k - k0], and the LDS copy of it
    float *row = tile + r * stride;
    const int first = k0 + ((t - k0 % G) + G) % G;      // the first bin >= k0 with k = t (mod G)

    if constexpr (G == 8) {
        const long long left = frames - f0;
        const int nr = left < RPB ? (int)left : RPB;
        const float *q = spec + c * spec_pitch + f0 * (long long)nfreq + k0;
#pragma unroll 4
        for (int i = tid; i < nr * n; i += 256) {
            const int rr = i / n, j = i - rr * n;
            tile[rr * stride + j] = q[(long long)rr * nfreq + j];
        }
    } else if constexpr (G == 64) {
        // every load of the lane's share in flight at once (at most 17 of them, predicated), then the LDS stores
        constexpr int SHARE = (WAVE_NFREQ + 63) / 64;
        float v[SHARE];
#pragma unroll
        for (int u = 0; u < SHARE; u++) {
            const int k = first + u * 64;
            v[u] = (live && k < k1) ? band[k - k0] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < SHARE; u++) {
            const int k = first + u * 64;
            if (live && k < k1) row[k - k0] = v[u];
        }
    } else if (held && live) {
#pragma unroll 8
        for (int k = first; k < k1; k += G) row[k - k0] = band[k - k0];
    }
    __syncthreads();

    // ---- pass 1: the peak ----
    float pv = 0.0f;
    int pk = NO_BIN;
    if (live) {
#pragma unroll 4
        for (int k = first; k < k1; k += G) {
            const float v = held ? row[k - k0] : band[k - k0];
            if (peak_better(v, k, pv, pk)) {
                pv = v;
                pk = k;
            }
        }
    }
    for (int d = W / 2; d >= 1; d >>= 1) {
        const float v2 = __shfl_xor(pv, d, 64);
        const int k2 = __shfl_xor(pk, d, 64);
        if (peak_better(v2, k2, pv, pk)) {
            pv = v2;
            pk = k2;
        }
    }
    if constexpr (G == 256) {
        if ((tid & 63) == 0) {
            red_v[tid >> 6] = pv;
            red_k[tid >> 6] = pk;
        }
        __syncthreads();
        pv = red_v[0];
        pk = red_k[0];
        for (int w = 1; w < 4; w++)
            if (peak_better(red_v[w], red_k[w], pv, pk)) {
                pv = red_v[w];
                pk = red_k[w];
            }
    }
    const float peak = pk == NO_BIN ? __builtin_nanf("") : pv;
    const bool valid = live && pk != NO_BIN && __builtin_isfinite(peak) && (double)peak > min_power;

    // ---- pass 2: moments about the peak, extents, logarithms ----
    double S = 0.0, M1 = 0.0, M2 = 0.0, L = 0.0;
    int klo = NO_BIN, khi = -1;
    if (valid && (features & 0xF8u)) {
        const double thr = drop_ratio * (double)peak;
#pragma unroll 2
        for (int k = first; k < k1; k += G) {
            const double v = (double)(held ? row[k - k0] : band[k - k0]);
            const double dk = (double)(k - pk);
            S += v;
            M1 += dk * v;
            M2 += (dk * dk) * v;
            if constexpr (FLAT) L += log(v);
            if (v >= thr) {
                if (klo == NO_BIN) klo = k;
                khi = k;
            }
        }
    }
    for (int d = W / 2; d >= 1; d >>= 1) {
        S += __shfl_xor(S, d, 64);
        M1 += __shfl_xor(M1, d, 64);
        M2 += __shfl_xor(M2, d, 64);
        if constexpr (FLAT) L += __shfl_xor(L, d, 64);
        const int lo2 = __shfl_xor(klo, d, 64), hi2 = __shfl_xor(khi, d, 64);
        klo = lo2 < klo ? lo2 : klo;
        khi = hi2 > khi ? hi2 : khi;
    }
    if constexpr (G == 256) {
        if ((tid & 63) == 0) {
            const int w = tid >> 6;
            red_d[0][w] = S;
            red_d[1][w] = M1;
            red_d[2][w] = M2;
            red_d[3][w] = L;
            red_lo[w] = klo;
            red_hi[w] = khi;
        }
        __syncthreads();
        S = (red_d[0][0] + red_d[0][1]) + (red_d[0][2] + red_d[0][3]);
        M1 = (red_d[1][0] + red_d[1][1]) + (red_d[1][2] + red_d[1][3]);
        M2 = (red_d[2][0] + red_d[2][1]) + (red_d[2][2] + red_d[2][3]);
        L = (red_d[3][0] + red_d[3][1]) + (red_d[3][2] + red_d[3][3]);
        for (int w = 0; w < 4; w++) {
            klo = red_lo[w] < klo ? red_lo[w] : klo;
            khi = red_hi[w] > khi ? red_hi[w] : khi;
        }
    }
    if (!live || t != 0) return;

    float val[N_FEATURES];
    const float nan32 = __builtin_nanf("");
#pragma unroll
    for (int b = 0; b < N_FEATURES; b++) val[b] = nan32;
    val[2] = peak;
    if (valid) {
        const double kp = (double)pk;
        val[0] = (float)(scale * kp);
        if (features & 2u) {
            double d = 0.0;
            if (pk - 1 >= k0 && pk + 1 < k1) {
                const float pa = held ? row[pk - 1 - k0] : band[pk - 1 - k0], pc = held ? row[pk + 1 - k0] : band[pk + 1 - k0];
                if (pa > 0.0f && pc > 0.0f) {
                    const double la = log((double)pa), lb = log((double)peak), lc = log((double)pc);
                    const double den = (la - 2.0 * lb) + lc;
                    if (den < 0.0) d = (0.5 * (la - lc)) / den;
                }
            }
            val[1] = (float)(scale * (kp + d));
        }
        if (features & 0xF8u) {
            const double m = M1 / S;
            const double var = M2 / S - m * m;
            val[3] = (float)(scale * (kp + m));
            val[4] = (float)(scale * sqrt(var > 0.0 ? var : 0.0));
            if constexpr (FLAT) val[5] = (float)(exp(L / (double)n) / (S / (double)n));
            val[6] = (float)(scale * (double)klo);
            val[7] = (float)(scale * (double)khi);
        }
    }
    float *o = out + c * out_pitch + f;
#pragma unroll
    for (int b = 0; b < N_FEATURES; b++)
        if (features >> b & 1u) {
            *o = val[b];
            o += out_feature_pitch;
        }
}

template <int G>
int feat_launch(hipdsp_ctx *ctx, const char *what, const float *spec, long long spec_pitch, long long channels,
                long long frames, int nfreq, int k0, int k1, unsigned features, double scale, double min_power,
                double drop_ratio, float *out, long long out_pitch, long long out_feature_pitch)
{
    constexpr int RPB = 256 / G;
    const dim3 grid((unsigned)((frames + RPB - 1) / RPB), (unsigned)channels);
    if (features & 32u)
        hipLaunchKernelGGL((feat_kernel<G, true>), grid, dim3(256), 0, ctx->stream, spec, spec_pitch, frames, nfreq, k0, k1,
                           features, scale, min_power, drop_ratio, out, out_pitch, out_feature_pitch);
    else
        hipLaunchKernelGGL((feat_kernel<G, false>), grid, dim3(256), 0, ctx->stream, spec, spec_pitch, frames, nfreq, k0, k1,
                           features, scale, min_power, drop_ratio, out, out_pitch, out_feature_pitch);
    return hd_launch_status(what);
}

}  // namespace

extern "C" int hipdsp_spectral_features(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, int64_t channels,
                                        int64_t frames, int64_t nfreq, int64_t k0, int64_t k1, unsigned features,
                                        double scale, double min_power, double drop_ratio, float *out, int64_t out_pitch,
                                        int64_t out_feature_pitch)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(channels >= 0 && frames >= 0 && nfreq >= 0, "negative size");
    HD_REQUIRE(nfreq <= (1LL << 26), "nfreq out of range");
    HD_REQUIRE(k0 >= 0 && k0 <= k1 && k1 <= nfreq, "band: bins [%lld, %lld) not inside [0, %lld]", (long long)k0,
               (long long)k1, (long long)nfreq);
    HD_REQUIRE(features != 0 && features < (1u << N_FEATURES), "features: mask 0x%x has no bit or bits above %d", features,
               N_FEATURES - 1);
    HD_REQUIRE(drop_ratio > 0.0 && drop_ratio <= 1.0, "drop_ratio %g not in (0, 1]", drop_ratio);
    HD_REQUIRE(spec_pitch >= 0 && out_pitch >= 0 && out_feature_pitch >= 0, "negative pitch");
    if (spec_pitch == 0) spec_pitch = frames * nfreq;
    if (out_pitch == 0) out_pitch = frames;
    if (out_feature_pitch == 0) out_feature_pitch = channels * out_pitch;
    HD_REQUIRE(spec_pitch >= frames * nfreq, "spec_pitch smaller than one channel");
    HD_REQUIRE(out_pitch >= frames, "out_pitch smaller than frames");
    if (frames == 0 || channels == 0) return HIPDSP_OK;
    HD_REQUIRE(out_feature_pitch >= (channels - 1) * out_pitch + frames, "out_feature_pitch smaller than one feature");
    HD_REQUIRE(spec != nullptr && out != nullptr, "NULL data pointer");
    HD_REQUIRE(channels <= 65535 && frames <= (nfreq <= SHORT_NFREQ ? 0xfffffffLL : 0xffffffLL),
               "too many channels or frames for one call");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    if (nfreq <= SHORT_NFREQ)
        return feat_launch<8>(ctx, "feat_kernel<8>", spec, spec_pitch, channels, frames, (int)nfreq, (int)k0, (int)k1,
                              features, scale, min_power, drop_ratio, out, out_pitch, out_feature_pitch);
    if (nfreq <= WAVE_NFREQ)
        return feat_launch<64>(ctx, "feat_kernel<64>", spec, spec_pitch, channels, frames, (int)nfreq, (int)k0, (int)k1,
                               features, scale, min_power, drop_ratio, out, out_pitch, out_feature_pitch);
    return feat_launch<256>(ctx, "feat_kernel<256>", spec, spec_pitch, channels, frames, (int)nfreq, (int)k0, (int)k1,
                            features, scale, min_power, drop_ratio, out, out_pitch, out_feature_pitch);
}
