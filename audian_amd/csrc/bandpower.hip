// hipdsp_band_power: power inside frequency bands of a planar spectrogram slab, per frame and channel -- the
// "envelope from visible frequency range of spectrogram" trace (include/hip_dsp.h).
//
// A strided row-segment reduction over (channels, frames, nfreq) float32: of every row only the bins the bands cover are
// read.  The host merges the bands into disjoint bin segments, so a bin that lies in several bands is loaded once and
// added to each of them.  Sums are carried in float64 and rounded to float32 once, after the scaling: that is the
// 1-ulp contract of the header (the kernel moves 4 B per add, the float64 VALU rate is not what limits it).
//
// The mapping is chosen by nfreq alone, never by the bands, and a lane's share of a row is fixed by the absolute bin
// index: the order in which a band's bins are added is therefore the same whatever other bands ride in the call, and
// a multi-band call gives bit for bit what one call per band gives.
//
//   nfreq <= 256      band_short_kernel: a workgroup takes 256 consecutive frames of a channel, stages 32-bin pieces of
//                     their segments in LDS with coalesced loads (the frames are contiguous in memory), then every lane
//                     sums ITS frame's bins in ascending order; the store is coalesced along time.
//   nfreq <  8192     band_rows_kernel<.., 64>: a wave per frame, lanes along frequency (lane l owns the bins = l mod 64),
//                     four loads in flight per lane, wave reduction by __shfl_down, lane 0 stores.
//   nfreq >= 8192     band_rows_kernel<.., 256>: a workgroup per frame, thread t owns the bins = t mod 256; the four
//                     waves' sums meet in LDS.
// Rows start at any 4-byte address (nfreq is odd, views begin at any frame): dword loads only, no alignment assumed;
// nothing outside the merged segments of a row is touched.  Index arithmetic on the slab is 64-bit.
#include "common.h"
#include "decibel.h"

namespace {

constexpr int MAX_BANDS = 16;

struct BandArgs {
    int k0[MAX_BANDS], k1[MAX_BANDS];   // the bands, in the caller's order; unused slots are empty (0, 0)
    int s0[MAX_BANDS], s1[MAX_BANDS];   // their union as disjoint ascending segments
    int n_bands, n_segs;
};

// dB in the arithmetic of hipdsp_decibel (decibel.h: decibel_of), so that dB here is bit for bit decibel(linear)
__device__ __forceinline__ float band_value(double sum, double scale, int db, const DbArgs &dba)
{
    const float v = (float)(scale * sum);
    return db ? decibel_of(v, dba) : v;
}

template <int NB>
__device__ __forceinline__ void band_add(double (&acc)[NB], const BandArgs &a, int k, float v)
{
    const double d = (double)v;
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] += (k >= a.k0[b] && k < a.k1[b]) ? d : 0.0;   // select, not multiply: NaN stays outside
}

template <int NB, int TPF>
__global__ __launch_bounds__(256) void band_rows_kernel(const float *__restrict__ spec, long long spec_pitch, long long frames,
                                                        int nfreq, BandArgs a, double scale, int db, DbArgs dba,
                                                        float *__restrict__ out, long long out_pitch,
                                                        long long out_band_pitch)
{
    constexpr int RPB = 256 / TPF;                      // rows (frames of one channel) per workgroup
    const int t = threadIdx.x % TPF;
    const long long c = blockIdx.y;
    const long long f = (long long)blockIdx.x * RPB + threadIdx.x / TPF;   // uniform over a wave
    const bool live = f < frames;
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = 0.0;
    if (live) {
        const float *p = spec + c * spec_pitch + f * (long long)nfreq;
        for (int i = 0; i < a.n_segs; i++) {
            const int s0 = a.s0[i], s1 = a.s1[i];
            for (int kb = (s0 / TPF) * TPF; kb < s1; kb += 4 * TPF) {
                // four loads in flight: a lane whose bin lies outside the segment re-reads the segment's nearest bin
                // (the same cache line, nothing outside the segment is touched) and drops it
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = kb + u * TPF + t;
                    v[u] = p[k < s0 ? s0 : (k >= s1 ? s1 - 1 : k)];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = kb + u * TPF + t;
                    band_add<NB>(acc, a, k, (k >= s0 && k < s1) ? v[u] : 0.0f);
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; b++)
        for (int d = 32; d >= 1; d >>= 1) acc[b] += __shfl_down(acc[b], d, 64);
    if constexpr (TPF == 256) {
        __shared__ double part[NB][4];
        if ((threadIdx.x & 63) == 0)
            for (int b = 0; b < NB; b++) part[b][threadIdx.x >> 6] = acc[b];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int b = 0; b < NB; b++) acc[b] = (part[b][0] + part[b][1]) + (part[b][2] + part[b][3]);
    }
    if (live && t == 0 && (TPF == 64 || threadIdx.x == 0)) {
#pragma unroll
        for (int b = 0; b < NB; b++)
            if (b < a.n_bands)
                out[b * out_band_pitch + c * out_pitch + f] = band_value(acc[b], scale, db, dba);
    }
}

constexpr int SHORT_FRAMES = 256, SHORT_BINS = 32;

template <int NB>
__global__ __launch_bounds__(256) void band_short_kernel(const float *__restrict__ spec, long long spec_pitch, long long frames,
                                                         int nfreq, BandArgs a, double scale, int db, DbArgs dba,
                                                         float *__restrict__ out, long long out_pitch,
                                                         long long out_band_pitch)
{
    __shared__ float tile[SHORT_FRAMES * (SHORT_BINS + 1)];      // +1: a lane walks its own row, rows on different banks
    const int tid = threadIdx.x;
    const long long c = blockIdx.y;
    const long long f0 = (long long)blockIdx.x * SHORT_FRAMES;
    const long long left = frames - f0;
    const int nf = left < SHORT_FRAMES ? (int)left : SHORT_FRAMES;
    const float *p = spec + c * spec_pitch + f0 * (long long)nfreq;
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = 0.0;
    for (int i = 0; i < a.n_segs; i++) {
        const int s1 = a.s1[i];
        for (int kt = a.s0[i]; kt < s1; kt += SHORT_BINS) {
            const int w = s1 - kt < SHORT_BINS ? s1 - kt : SHORT_BINS;
            const int kk = tid % SHORT_BINS, kc = kk < w ? kk : w - 1;
            for (int base = tid / SHORT_BINS; base < nf; base += 4 * (256 / SHORT_BINS)) {
                // four row pieces in flight per thread; a thread past the piece or the frames re-reads the last bin /
                // frame of the tile (inside the segment, inside the slab) and drops it
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int fr = base + u * (256 / SHORT_BINS);
                    v[u] = p[(long long)(fr < nf ? fr : nf - 1) * nfreq + kt + kc];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int fr = base + u * (256 / SHORT_BINS);
                    if (fr < nf && kk < w) tile[fr * (SHORT_BINS + 1) + kk] = v[u];
                }
            }
            __syncthreads();
            if (tid < nf)
                for (int j = 0; j < w; j++) band_add<NB>(acc, a, kt + j, tile[tid * (SHORT_BINS + 1) + j]);
            __syncthreads();
        }
    }
    if (tid < nf) {
#pragma unroll
        for (int b = 0; b < NB; b++)
            if (b < a.n_bands)
                out[b * out_band_pitch + c * out_pitch + f0 + tid] = band_value(acc[b], scale, db, dba);
    }
}

template <int NB>
int band_launch(hipdsp_ctx *ctx, const float *spec, long long spec_pitch, long long channels, long long frames, int nfreq,
                const BandArgs &a, double scale, int db, const DbArgs &dba, float *out, long long out_pitch,
                long long out_band_pitch)
{
    if (nfreq <= 256) {
        const dim3 grid((unsigned)((frames + SHORT_FRAMES - 1) / SHORT_FRAMES), (unsigned)channels);
        hipLaunchKernelGGL(band_short_kernel<NB>, grid, dim3(256), 0, ctx->stream, spec, spec_pitch, frames, nfreq, a,
                           scale, db, dba, out, out_pitch, out_band_pitch);
        return hd_launch_status("band_short_kernel");
    }
    if (nfreq < 8192) {
        const dim3 grid((unsigned)((frames + 3) / 4), (unsigned)channels);
        hipLaunchKernelGGL((band_rows_kernel<NB, 64>), grid, dim3(256), 0, ctx->stream, spec, spec_pitch, frames, nfreq, a,
                           scale, db, dba, out, out_pitch, out_band_pitch);
        return hd_launch_status("band_rows_kernel<64>");
    }
    const dim3 grid((unsigned)frames, (unsigned)channels);
    hipLaunchKernelGGL((band_rows_kernel<NB, 256>), grid, dim3(256), 0, ctx->stream, spec, spec_pitch, frames, nfreq, a,
                       scale, db, dba, out, out_pitch, out_band_pitch);
    return hd_launch_status("band_rows_kernel<256>");
}

}  // namespace

extern "C" int hipdsp_band_power(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, int64_t channels, int64_t frames,
                                 int64_t nfreq, const int64_t *host_k0, const int64_t *host_k1, int n_bands, double scale,
                                 int db, double ref_power, double min_power, float *out, int64_t out_pitch,
                                 int64_t out_band_pitch)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(channels >= 0 && frames >= 0 && nfreq >= 0, "negative size");
    HD_REQUIRE(n_bands >= 1, "at least one band, got %d", n_bands);
    if (n_bands > MAX_BANDS) {
        hipdsp_set_error("at most %d bands per call, got %d", MAX_BANDS, n_bands);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    HD_REQUIRE(host_k0 != nullptr && host_k1 != nullptr, "NULL band list");
    HD_REQUIRE(nfreq < (1LL << 30), "nfreq out of range");
    BandArgs a;
    memset(&a, 0, sizeof(a));
    a.n_bands = n_bands;
    for (int b = 0; b < n_bands; b++) {
        HD_REQUIRE(host_k0[b] >= 0 && host_k0[b] <= host_k1[b] && host_k1[b] <= nfreq,
                   "band %d: bins [%lld, %lld) not inside [0, %lld]", b, (long long)host_k0[b], (long long)host_k1[b],
                   (long long)nfreq);
        a.k0[b] = (int)host_k0[b];
        a.k1[b] = (int)host_k1[b];
    }
    HD_REQUIRE(!db || ref_power > 0, "ref_power must be positive");
    if (spec_pitch == 0) spec_pitch = frames * nfreq;
    if (out_pitch == 0) out_pitch = frames;
    if (out_band_pitch == 0) out_band_pitch = channels * out_pitch;
    HD_REQUIRE(spec_pitch >= frames * nfreq, "spec_pitch smaller than one channel");
    HD_REQUIRE(out_pitch >= frames, "out_pitch smaller than frames");
    if (frames == 0 || channels == 0) return HIPDSP_OK;
    HD_REQUIRE(out_band_pitch >= (channels - 1) * out_pitch + frames, "out_band_pitch smaller than one band");
    HD_REQUIRE(spec != nullptr && out != nullptr, "NULL data pointer");
    HD_REQUIRE(channels <= 65535 && frames <= (nfreq <= 256 ? 0x7fffffffLL : 0xffffffLL), "too many channels or frames for one call");
    // the union of the bands as disjoint ascending segments (insertion sort by start, then merge what touches)
    int order[MAX_BANDS], n = 0;
    for (int b = 0; b < n_bands; b++) {
        if (a.k1[b] <= a.k0[b]) continue;
        int j = n++;
        for (; j > 0 && a.k0[order[j - 1]] > a.k0[b]; j--) order[j] = order[j - 1];
        order[j] = b;
    }
    for (int j = 0; j < n; j++) {
        const int b = order[j];
        if (a.n_segs > 0 && a.k0[b] <= a.s1[a.n_segs - 1]) {
            if (a.k1[b] > a.s1[a.n_segs - 1]) a.s1[a.n_segs - 1] = a.k1[b];
        } else {
            a.s0[a.n_segs] = a.k0[b];
            a.s1[a.n_segs] = a.k1[b];
            a.n_segs++;
        }
    }
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    const DbArgs dba = db ? db_args(ref_power, min_power) : db_args(1.0, 0.0);
    if (n_bands == 1)
        return band_launch<1>(ctx, spec, spec_pitch, channels, frames, (int)nfreq, a, scale, db, dba,
                              out, out_pitch, out_band_pitch);
    if (n_bands <= 4)
        return band_launch<4>(ctx, spec, spec_pitch, channels, frames, (int)nfreq, a, scale, db, dba,
                              out, out_pitch, out_band_pitch);
    return band_launch<16>(ctx, spec, spec_pitch, channels, frames, (int)nfreq, a, scale, db, dba,
                           out, out_pitch, out_band_pitch);
}
