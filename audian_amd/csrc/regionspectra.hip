// hipdsp_region_spectra: the Welch power spectral density of many regions of a planar float32 array in one call -- per
// region the mean over its Hann-windowed, mean-free frames of the one-sided PSD, and the bin of its largest value; the
// step behind event detection in the reference's songdetector.py (env_freqs, songdetector.py:146-152; the contract is in
// include/hip_dsp.h).
//
// Two launches on the context's stream, over a work list the host sizes exactly from the region table:
//
//   region_spectra_kernel   one 256-thread workgroup per (region, frame group).  The groups of a region are anchored at
//                           the region's FIRST frame and hold SP_GROUP = 16 consecutive frames (the last one fewer), so
//                           what a group computes depends on nothing but the region and (nfft, hop, step).  The workgroup
//                           finds its region by hd_owner (rowpass.h) over the table's item offsets, builds exp(-2 pi i m /
//                           nfft), m < nfft/2, once in LDS (float64 sincospi, rounded to float32; the Hann window is
//                           0.5 -+ 0.5 cos from the same table) and then takes frame after frame: the samples x[start +
//                           (k*hop + i)*step] go to LDS while their float64 sum is reduced in a fixed order; the mean is
//                           subtracted in float64, the window applied in float32; the real transform runs as ONE complex
//                           radix-2 Stockham FFT of nfft/2 points on z[n] = v[2n] + i v[2n+1] plus the split step; |X|^2
//                           is added in float64 to the thread's own bins (bin f belongs to thread f % 256: at most 17
//                           running sums in registers).  A frame whose sum is not finite holds a NaN or an infinity: it
//                           is not transformed and flags the group.  No spectrum of a frame goes to memory; a group
//                           stores one partial row of F float64 sums and its flag.
//   region_spectra_finish   one workgroup per region: thread f % 256 adds the partial rows of bin f in ascending group
//                           order, scales (1 / (fs sum w^2 n_frames), twice that for bins 1 ... F-2), rounds to float32
//                           and stores; the first position of the largest stored value is reduced in a fixed order
//                           (wave shuffles, then the four waves through LDS).  A flagged group makes the row NaN and the
//                           position 0, a region without a whole frame gives NaN and -1.
//
// LDS: 12 * nfft bytes (two buffers of nfft/2 float2 and the table), 96 KB at nfft 8192.  No atomics at all: the same
// call gives the same bytes twice, whatever else rides in it.  Index arithmetic on the array is 64-bit.
#include "rowpass.h"
#include <vector>

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_GROUP = 16;                            // frames per work item
constexpr int SP_MAX_NFFT = 8192;
constexpr int SP_BINS = (SP_MAX_NFFT / 2 + 1 + SP_THREADS - 1) / SP_THREADS;   // bins per thread at most: 17

struct SpRegion {                                       // one row of the uploaded table; row n_regions: ibase = all items
    long long channel, start, n_frames, ibase;
};

__global__ __launch_bounds__(SP_THREADS) void region_spectra_kernel(const float *__restrict__ x, long long pitch,
                                                                    const SpRegion *__restrict__ tab, int n_regions, int nfft,
                                                                    int hop, long long step, double *__restrict__ part)
{
    extern __shared__ float2 sp_lds[];                  // A | B | table: nfft/2 float2 each
    __shared__ double red[4];
    const int t = threadIdx.x;
    const long long g = blockIdx.x;
    const int M = nfft >> 1, F = M + 1, half = M >> 1;
    float2 *A = sp_lds, *B = sp_lds + M, *tw = sp_lds + 2 * M;

    const SpRegion reg = tab[hd_owner(tab, &SpRegion::ibase, n_regions, g)];
    const long long k0 = (g - reg.ibase) * SP_GROUP;
    const long long left = reg.n_frames - k0;
    const int nk = left < SP_GROUP ? (int)left : SP_GROUP;
    const float *row = x + reg.channel * pitch + reg.start;

    for (int m = t; m < M; m += SP_THREADS) {
        double sn, cs;
        sincospi(-2.0 * (double)m / (double)nfft, &sn, &cs);
        tw[m] = make_float2((float)cs, (float)sn);
    }
    double acc[SP_BINS];
#pragma unroll
    for (int j = 0; j < SP_BINS; j++) acc[j] = 0.0;
    int bad = 0;
    __syncthreads();

    for (int k = 0; k < nk; k++) {
        const float *seg = row + (k0 + k) * (long long)hop * step;
        float *raw = (float *)A;                        // the frame's nfft samples, later z[n] = (v[2n], v[2n+1])
        double s = 0.0;
        for (int i = t; i < nfft; i += SP_THREADS) {
            const float v = seg[(long long)i * step];
            raw[i] = v;
            s += (double)v;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if ((t & 63) == 0) red[t >> 6] = s;
        __syncthreads();
        const double mean = ((red[0] + red[1]) + (red[2] + red[3])) / (double)nfft;
        if (!(fabs(mean) <= 1.7976931348623157e308)) {  // a NaN or an infinity among the samples (finite floats cannot
            bad = 1;                                    // overflow a float64 sum of 8192)
            __syncthreads();                            // red is read by all before the next frame writes it
            continue;
        }
        for (int i = t; i < nfft; i += SP_THREADS) {    // the thread's own samples again
            const float w = i < M ? 0.5f - 0.5f * tw[i].x : 0.5f + 0.5f * tw[i - M].x;   // periodic Hann
            raw[i] = (float)((double)raw[i] - mean) * w;
        }
        __syncthreads();
        float2 *in = A, *ou = B;
        for (int Ns = 1; Ns < M; Ns <<= 1) {
            const int tstep = M / Ns;                   // exp(-i pi k / Ns) = table[k * M / Ns]
            for (int j = t; j < half; j += SP_THREADS) {
                const int kk = j & (Ns - 1);
                const float2 w = tw[kk * tstep];
                const float2 v0 = in[j], v1 = in[j + half];
                const float2 p = make_float2(v1.x * w.x - v1.y * w.y, v1.x * w.y + v1.y * w.x);
                const int j0 = ((j - kk) << 1) + kk;
                ou[j0] = make_float2(v0.x + p.x, v0.y + p.y);
                ou[j0 + Ns] = make_float2(v0.x - p.x, v0.y - p.y);
            }
            __syncthreads();
            float2 *tmp = in;
            in = ou;
            ou = tmp;
        }
        // split step: X[f] = E[f] + W^f O[f], E = (Z[f] + conj Z[M-f]) / 2, O = (Z[f] - conj Z[M-f]) / (2i)
#pragma unroll
        for (int j = 0; j < SP_BINS; j++) {
            const int f = t + j * SP_THREADS;
            if (f < F) {
                float re, im;
                if (f == 0 || f == M) {
                    const float2 z = in[0];
                    re = f == 0 ? z.x + z.y : z.x - z.y;
                    im = 0.0f;
                } else {
                    const float2 zk = in[f], zm = in[M - f], w = tw[f];
                    const float er = 0.5f * (zk.x + zm.x), ei = 0.5f * (zk.y - zm.y);
                    const float orr = 0.5f * (zk.y + zm.y), oi = -0.5f * (zk.x - zm.x);
                    re = er + (orr * w.x - oi * w.y);
                    im = ei + (orr * w.y + oi * w.x);
                }
                acc[j] += (double)re * (double)re + (double)im * (double)im;
            }
        }
        __syncthreads();                                // all have read the spectrum before the next frame lands in A
    }

    double *prow = part + g * (long long)(F + 1);
#pragma unroll
    for (int j = 0; j < SP_BINS; j++) {
        const int f = t + j * SP_THREADS;
        if (f < F) prow[f] = acc[j];
    }
    if (t == 0) prow[F] = bad ? 1.0 : 0.0;
}

// (value, bin) pairs as np.argmax orders them: a NaN beats every number, equal values keep the earlier bin; -1 = none
__device__ __forceinline__ void sp_higher(float &v, int &i, float ov, int oi)
{
    if (oi < 0) return;
    bool take;
    if (i < 0) take = true;
    else if (ov != ov) take = v != v ? oi < i : true;
    else if (v != v) take = false;
    else take = ov > v || (ov == v && oi < i);
    if (take) {
        v = ov;
        i = oi;
    }
}

__global__ __launch_bounds__(SP_THREADS) void region_spectra_finish(const SpRegion *__restrict__ tab, int nfft, double scale,
                                                                    const double *__restrict__ part, float *__restrict__ out,
                                                                    long long out_pitch, int64_t *__restrict__ info)
{
    __shared__ float sh_v[4];
    __shared__ int sh_i[4];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const int F = nfft / 2 + 1;
    const SpRegion reg = tab[r];
    const long long ng = tab[r + 1].ibase - reg.ibase;
    const double *p0 = part + reg.ibase * (long long)(F + 1);
    float *orow = out + r * out_pitch;
    const float nan = __uint_as_float(0x7fc00000u);
    bool bad = reg.n_frames == 0;
    for (long long j = 0; j < ng; j++) bad = bad || p0[j * (F + 1) + F] != 0.0;
    if (bad) {
        for (int f = t; f < F; f += SP_THREADS) orow[f] = nan;
        if (t == 0) {
            info[2 * r] = reg.n_frames;
            info[2 * r + 1] = reg.n_frames == 0 ? -1 : 0;
        }
        return;
    }
    const double one = scale / (double)reg.n_frames;
    float bv = 0.0f;
    int bi = -1;
    for (int f = t; f < F; f += SP_THREADS) {           // ascending bins: a later equal value does not replace
        double s = 0.0;
        for (long long j = 0; j < ng; j++) s += p0[j * (F + 1) + f];
        const float v = (float)(s * (f != 0 && f != F - 1 ? 2.0 * one : one));
        orow[f] = v;
        sp_higher(bv, bi, v, f);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_down(bv, d, 64);
        const int oi = __shfl_down(bi, d, 64);
        sp_higher(bv, bi, ov, oi);
    }
    if ((t & 63) == 0) {
        sh_v[t >> 6] = bv;
        sh_i[t >> 6] = bi;
    }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; w++) sp_higher(bv, bi, sh_v[w], sh_i[w]);
        info[2 * r] = reg.n_frames;
        info[2 * r + 1] = bi;
    }
}

}  // namespace

extern "C" int hipdsp_region_spectra(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t frames,
                                     const int64_t *host_regions, int64_t n_regions, int nfft, int hop, int64_t step,
                                     double fs, float *out, int64_t out_pitch, int64_t *info)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(nfft >= 8 && nfft <= SP_MAX_NFFT && (nfft & (nfft - 1)) == 0, "nfft %d is not a power of two in [8, %d]", nfft,
               SP_MAX_NFFT);
    HD_REQUIRE(hop >= 1 && hop <= nfft, "hop %d not in [1, nfft = %d]", hop, nfft);
    HD_REQUIRE(step >= 1, "step %lld must be at least 1", (long long)step);
    HD_REQUIRE(fs > 0.0 && fs <= 1.7976931348623157e308, "fs must be positive and finite");
    HD_TRY(hd_check_table("hipdsp_region_spectra", ctx, x, x_pitch, channels, frames, host_regions, n_regions,
                          (1LL << 31) / 32));
    const int F = nfft / 2 + 1;
    if (out_pitch == 0) out_pitch = F;
    HD_REQUIRE(out_pitch >= F, "out_pitch smaller than nfft/2 + 1");
    if (n_regions == 0) return HIPDSP_OK;
    HD_REQUIRE(out != nullptr && info != nullptr, "NULL output");
    HD_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)info & 7) == 0, "misaligned pointer");
    std::vector<SpRegion> tab((size_t)n_regions + 1);
    long long items = 0;
    for (int64_t r = 0; r < n_regions; r++) {
        const int64_t a = host_regions[3 * r + 1], b = host_regions[3 * r + 2];
        const long long len = (b - a + step - 1) / step;                 // len(x[a:b:step])
        const long long nf = len >= nfft ? (len - nfft) / hop + 1 : 0;
        tab[r] = SpRegion{host_regions[3 * r], a, nf, items};
        items += (nf + SP_GROUP - 1) / SP_GROUP;
    }
    tab[n_regions] = SpRegion{0, 0, 0, items};
    HD_REQUIRE(items <= 0x7fffffffLL, "too many frames for one call");
    HD_REQUIRE(x != nullptr || items == 0, "NULL data pointer");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    const size_t tab_bytes = sizeof(SpRegion) * tab.size();
    void *work = nullptr;
    int rc = hipdsp_scratch(ctx, tab_bytes + sizeof(double) * (size_t)items * (size_t)(F + 1), &work);
    if (rc != HIPDSP_OK) return rc;
    const SpRegion *dtab = (const SpRegion *)work;
    double *part = (double *)((char *)work + tab_bytes);
    HD_TRY(hd_upload_table(ctx, work, tab.data(), tab_bytes));
    const double sw2 = hd_hann_sumsq(nfft);
    if (items > 0) {
        const size_t lds = sizeof(float2) * 3 * (size_t)(nfft / 2);
        if (lds > 48 * 1024)
            HD_CHECK_HIP(hipFuncSetAttribute((const void *)region_spectra_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds));
        hipLaunchKernelGGL(region_spectra_kernel, dim3((unsigned)items), dim3(SP_THREADS), lds, ctx->stream, x,
                           (long long)x_pitch, dtab, (int)n_regions, nfft, hop, (long long)step, part);
        rc = hd_launch_status("region_spectra_kernel");
        if (rc != HIPDSP_OK) return rc;
    }
    hipLaunchKernelGGL(region_spectra_finish, dim3((unsigned)n_regions), dim3(SP_THREADS), 0, ctx->stream, dtab, nfft,
                       1.0 / (fs * sw2), (const double *)part, out, (long long)out_pitch, info);
    return hd_launch_status("region_spectra_finish");
}
