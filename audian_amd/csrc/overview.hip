// Full-trace overview straight from the file's PCM (CompressedData, src/audian/compresseddata.py:25-52): the min/max
// envelope of a block of interleaved little-endian signed PCM (frames, channels), written in the reference's own layout
// -- float64 (2*nseg, channels), row 2j the minimum and row 2j+1 the maximum of frames [j*step, min((j+1)*step, frames))
// -- so that the device-to-host copy lands in CompressedData.datas as it is.  One read of the PCM bytes replaces
// hipdsp_pcm_unpack + hipdsp_minmax_decimate (2 B instead of about 10 B of HBM traffic per int16 sample).
//
// Layout of the work: a workgroup owns P runs ("parts") of `span` consecutive frames and CG channels (CG * P <= 256
// threads; thread = (channel, part)).  It walks its parts in slices of SF frames: each slice is a contiguous byte range
// of the file, staged in LDS with 16-byte loads of consecutive lanes whatever the frame width (the aligned 16-byte
// vectors that cover the range; the odd bytes around it lie in the same vectors, hence on mapped pages), then every
// thread walks its channel of its slice sequentially.  A thread flushes its running min/max whenever it crosses a
// segment boundary, with 32-bit atomic min/max into a key per (row, channel): order-independent, so segments that
// cross parts, slices and workgroups combine exactly.  A last kernel turns the keys into the float64 rows.
//
// Unwrap off: keys are the integer samples; the float64 value int * scale is formed once per segment (scale > 0 keeps
// the order; scale < 0 swaps min and max) -- bit-exact with (int64 * scale) in NumPy.
// Unwrap on (audioio's unwrap as hipdsp_unwrap restates it, elementwise.hip): x = (float)(int * scale); events
// (step between successive samples beyond +-thresh) are counted per part, scanned per channel, and the reducing pass
// redoes its part's events on top of the carried-in count, in the float32 arithmetic of unwrap_apply_kernel; keys are
// the float bits mapped to an order-preserving int.  The offset starts from zero at the first frame of the call.
#include "common.h"
#include <climits>
#include <cmath>

namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_LDS = 32768;           // bytes of slices per workgroup (four or five workgroups per CU)

struct OvGeom {
    long long frames, channels, step, nseg;
    long long span;                     // frames per part
    long long n_parts;                  // parts over the whole grid (gridDim.x * P): unwrap counts per channel
    int fb;                             // bytes per frame
    int cg, p;                          // channels per workgroup, parts per workgroup
    int sf;                             // frames per slice
    int slice;                          // LDS bytes per slice (multiple of 16)
    int nvec;                           // 16-byte vectors per slice
};

template <int B, bool ALIGNED>
__device__ __forceinline__ int ov_sample(const unsigned char *p)
{
    if (B == 2) {
        if (ALIGNED) return (int)*reinterpret_cast<const short *>(p);
        return (int)(short)((unsigned)p[0] | ((unsigned)p[1] << 8));
    } else if (B == 3) {
        return ((int)(((unsigned)p[0] << 8) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 24))) >> 8;
    } else {
        if (ALIGNED) return *reinterpret_cast<const int *>(p);
        return (int)((unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24));
    }
}

// float <-> int with the same order (finite values; the unwrapped samples of PCM are never NaN or -0)
__device__ __forceinline__ int ov_key(float v)
{
    const int b = __float_as_int(v);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float ov_unkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__device__ __forceinline__ float ov_value(int iv, double scale) { return (float)((double)iv * scale); }

__device__ __forceinline__ int ov_event(float cur, float prev, float thresh)
{
    const float d = cur - prev;
    return (d < -thresh ? 1 : 0) - (d > thresh ? 1 : 0);
}

__global__ __launch_bounds__(256) void ov_init_kernel(int *__restrict__ keys, long long rows, long long channels)
{
    const long long n = rows * channels;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        keys[i] = ((i / channels) & 1) ? INT_MIN : INT_MAX;
}

// MODE 0: min/max of the integers; 1: count unwrap events per (channel, part); 2: min/max of the unwrapped floats
template <int B, bool ALIGNED, int MODE>
__global__ __launch_bounds__(256) void ov_pcm_kernel(const unsigned char *__restrict__ pcm, OvGeom g, double scale,
                                                     float thresh, float ustep, int clips, float oscale,
                                                     int *__restrict__ keys, int *__restrict__ counts)
{
    extern __shared__ uint4 ov_lds[];
    unsigned char *lds = reinterpret_cast<unsigned char *>(ov_lds);
    const int tid = threadIdx.x;
    const int cl = tid % g.cg, p = tid / g.cg;
    const long long c = (long long)blockIdx.y * g.cg + cl;
    const bool active = p < g.p && c < g.channels;
    const long long w0 = (long long)blockIdx.x * g.p * g.span;          // first frame of the workgroup
    const long long f_lo = w0 + (long long)p * g.span;
    const long long f_hi = f_lo + g.span < g.frames ? f_lo + g.span : g.frames;
    const long long part = (long long)blockIdx.x * g.p + p;

    int mn = INT_MAX, mx = INT_MIN;
    int cnt = 0;
    if (MODE == 2 && active) cnt = counts[c * g.n_parts + part];
    float prev = 0.f;
    long long seg = f_lo / g.step, nb = (seg + 1) * g.step;           // current segment and its end

    const long long niter = (g.span + g.sf - 1) / g.sf;
    for (long long j = 0; j < niter; j++) {
        __syncthreads();                                               // the last slice has been read
        for (int idx = tid; idx < g.p * g.nvec; idx += OV_THREADS) {
            const int q = idx / g.nvec, v = idx % g.nvec;
            const long long qs = w0 + (long long)q * g.span + j * g.sf;
            long long qe = qs + g.sf;
            const long long qend = w0 + (long long)(q + 1) * g.span;
            if (qe > qend) qe = qend;
            if (qe > g.frames) qe = g.frames;
            if (qs >= qe) continue;
            const int lead = (MODE != 0 && j == 0 && qs > 0) ? 1 : 0; // the frame before the part: its first event
            const unsigned char *s = pcm + (qs - lead) * g.fb, *e = pcm + qe * g.fb;
            const uint4 *a = reinterpret_cast<const uint4 *>((uintptr_t)s & ~(uintptr_t)15);
            if (reinterpret_cast<const unsigned char *>(a + v) >= e) continue;
            *reinterpret_cast<uint4 *>(lds + q * g.slice + 16 * v) = a[v];
        }
        __syncthreads();
        if (!active) continue;
        const long long fs = f_lo + j * g.sf;
        const long long fe = fs + g.sf < f_hi ? fs + g.sf : f_hi;
        if (fs >= fe) continue;
        const int lead = (MODE != 0 && j == 0 && fs > 0) ? 1 : 0;
        const unsigned char *src = lds + p * g.slice + ((uintptr_t)(pcm + (fs - lead) * g.fb) & 15) + c * B;
        if (MODE != 0 && j == 0) {
            prev = ov_value(ov_sample<B, ALIGNED>(src), scale);        // (the first frame itself when lead = 0)
            src += lead * g.fb;
        }
        for (long long f = fs; f < fe; f++, src += g.fb) {
            const int iv = ov_sample<B, ALIGNED>(src);
            int k;
            if (MODE == 0) {
                k = iv;
            } else {
                const float x = ov_value(iv, scale);
                const int ev = f > 0 ? ov_event(x, prev, thresh) : 0;
                prev = x;
                cnt += ev;
                if (MODE == 1) continue;
                float o = x + ustep * (float)cnt;
                if (clips) o = o < -0.5f * ustep ? -0.5f * ustep : (o > 0.5f * ustep ? 0.5f * ustep : o);
                k = ov_key(o * oscale);
            }
            if (f == nb) {
                atomicMin(keys + (2 * seg) * g.channels + c, mn);
                atomicMax(keys + (2 * seg + 1) * g.channels + c, mx);
                mn = INT_MAX; mx = INT_MIN;
                seg++; nb += g.step;
            }
            mn = k < mn ? k : mn;
            mx = k > mx ? k : mx;
        }
    }
    if (!active || f_hi <= f_lo) return;
    if (MODE == 1) {
        counts[c * g.n_parts + part] = cnt;
    } else {
        atomicMin(keys + (2 * seg) * g.channels + c, mn);
        atomicMax(keys + (2 * seg + 1) * g.channels + c, mx);
    }
}

// counts[ch][part] -> events before the part (exclusive scan along a channel), in place
__global__ __launch_bounds__(256) void ov_scan_kernel(int *__restrict__ counts, long long n)
{
    __shared__ int part[256];
    int *cc = counts + (long long)blockIdx.x * n;
    const long long per = (n + 255) / 256;
    const long long a = per * threadIdx.x, b = a + per < n ? a + per : n;
    int s = 0;
    for (long long i = a; i < b; i++) s += cc[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; t++) { const int v = part[t]; part[t] = run; run += v; }
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (long long i = a; i < b; i++) { const int v = cc[i]; cc[i] = run; run += v; }
}

__global__ __launch_bounds__(256) void ov_finish_kernel(const int *__restrict__ keys, long long rows, long long channels,
                                                        int unwrap, double scale, double *__restrict__ out,
                                                        long long out_pitch)
{
    const long long n = rows * channels;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / channels, c = i - r * channels;
        double v;
        if (unwrap) {
            v = (double)ov_unkey(keys[i]);
        } else {
            const long long src = scale < 0 ? ((r ^ 1) * channels + c) : i;   // a negative scale swaps min and max
            v = (double)keys[src] * scale;
        }
        out[r * out_pitch + c] = v;
    }
}

}  // namespace

extern "C" {

int hipdsp_pcm_minmax(hipdsp_ctx *ctx, const void *pcm_tc, int sample_bytes, int64_t frames, int64_t channels,
                      int64_t step, double scale, double unwrap_thresh, double ampl_max, int clips, int down_scale,
                      double *out_rc, int64_t out_pitch)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(pcm_tc != nullptr && out_rc != nullptr, "NULL data pointer");
    HD_REQUIRE(sample_bytes == 2 || sample_bytes == 3 || sample_bytes == 4,
               "sample_bytes %d: signed PCM of 2, 3 or 4 bytes only", sample_bytes);
    HD_REQUIRE(frames >= 0 && channels >= 0, "negative size");
    HD_REQUIRE(step >= 1, "step %lld < 1", (long long)step);
    HD_REQUIRE(out_pitch >= channels, "out_pitch %lld < channels %lld", (long long)out_pitch, (long long)channels);
    HD_REQUIRE(std::isfinite(scale), "scale must be finite");
    const bool unwrap = unwrap_thresh > 1e-3;
    HD_REQUIRE(!unwrap || ampl_max > 0, "ampl_max must be positive");
    if (frames == 0 || channels == 0) return HIPDSP_OK;
    if (channels * sample_bytes > OV_LDS / 2) {
        hipdsp_set_error("frames of %lld bytes: at most %d", (long long)(channels * sample_bytes), OV_LDS / 2);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    HD_CHECK_HIP(hipSetDevice(ctx->device));

    OvGeom g;
    g.frames = frames; g.channels = channels; g.step = step;
    g.nseg = (frames + step - 1) / step;
    g.fb = (int)(channels * sample_bytes);
    g.cg = channels < OV_THREADS ? (int)channels : OV_THREADS;
    g.p = 1;
    while (2 * g.p * g.cg <= OV_THREADS) g.p *= 2;
    // frames per slice: the P slices (one leading frame of unwrap and 16 bytes of alignment slack each) fit OV_LDS
    long long sf = (OV_LDS / g.p - 32) / g.fb - 1;
    if (sf > 64) sf = 64;
    if (sf < 1) sf = 1;
    g.sf = (int)sf;
    g.nvec = (int)(((long long)(g.sf + 1) * g.fb + 15) / 16 + 1);
    g.slice = 16 * g.nvec;
    while (g.p > 1 && g.p * g.slice > OV_LDS) {                        // (only for frames near the limit)
        g.p /= 2;
    }
    // parts long enough that a grid of about 2048 workgroups covers the block, at least one slice
    long long span = (frames + (long long)g.p * 2048 - 1) / ((long long)g.p * 2048);
    if (span < g.sf) span = g.sf;
    if (span > 8192) span = 8192;
    g.span = span;
    const long long gx = (frames + (long long)g.p * span - 1) / ((long long)g.p * span);
    const long long gy = (channels + g.cg - 1) / g.cg;
    HD_REQUIRE(gx <= 0x7fffffffLL && gy <= 65535, "grid too large");
    g.n_parts = gx * g.p;

    const long long rows = 2 * g.nseg;
    const size_t key_bytes = sizeof(int) * (size_t)rows * (size_t)channels;
    const size_t key_pad = (key_bytes + 255) & ~(size_t)255;
    const size_t count_bytes = unwrap ? sizeof(int) * (size_t)g.n_parts * (size_t)channels : 0;
    void *work = nullptr;
    int rc = hipdsp_scratch(ctx, key_pad + count_bytes, &work);
    if (rc != HIPDSP_OK) return rc;
    int *keys = (int *)work;
    int *counts = unwrap ? (int *)((char *)work + key_pad) : nullptr;

    const unsigned fill_grid = (unsigned)((rows * channels + 255) / 256 < 8192 ? (rows * channels + 255) / 256 : 8192);
    hipLaunchKernelGGL(ov_init_kernel, dim3(fill_grid), dim3(256), 0, ctx->stream, keys, rows, (long long)channels);
    rc = hd_launch_status("ov_init_kernel");
    if (rc != HIPDSP_OK) return rc;

    const unsigned char *pcm = (const unsigned char *)pcm_tc;
    const bool aligned = ((uintptr_t)pcm & 15) == 0 && g.fb % 16 == 0 && sample_bytes != 3;
    const dim3 grid((unsigned)gx, (unsigned)gy), block(OV_THREADS);
    const size_t lds = (size_t)g.p * g.slice;
    const float thresh = (float)unwrap_thresh, ustep = (float)(2.0 * ampl_max);
    const float oscale = (clips || !down_scale) ? 1.0f : 0.5f;
#define HD_OV(MODE)                                                                                                     \
    do {                                                                                                                \
        if (sample_bytes == 2 && aligned)                                                                               \
            hipLaunchKernelGGL((ov_pcm_kernel<2, true, MODE>), grid, block, lds, ctx->stream, pcm, g, scale, thresh,   \
                               ustep, clips, oscale, keys, counts);                                                     \
        else if (sample_bytes == 2)                                                                                     \
            hipLaunchKernelGGL((ov_pcm_kernel<2, false, MODE>), grid, block, lds, ctx->stream, pcm, g, scale, thresh,  \
                               ustep, clips, oscale, keys, counts);                                                     \
        else if (sample_bytes == 3)                                                                                     \
            hipLaunchKernelGGL((ov_pcm_kernel<3, false, MODE>), grid, block, lds, ctx->stream, pcm, g, scale, thresh,  \
                               ustep, clips, oscale, keys, counts);                                                     \
        else if (aligned)                                                                                               \
            hipLaunchKernelGGL((ov_pcm_kernel<4, true, MODE>), grid, block, lds, ctx->stream, pcm, g, scale, thresh,   \
                               ustep, clips, oscale, keys, counts);                                                     \
        else                                                                                                            \
            hipLaunchKernelGGL((ov_pcm_kernel<4, false, MODE>), grid, block, lds, ctx->stream, pcm, g, scale, thresh,  \
                               ustep, clips, oscale, keys, counts);                                                     \
        rc = hd_launch_status("ov_pcm_kernel");                                                                         \
        if (rc != HIPDSP_OK) return rc;                                                                                 \
    } while (0)
    if (unwrap) {
        HD_OV(1);
        hipLaunchKernelGGL(ov_scan_kernel, dim3((unsigned)channels), dim3(256), 0, ctx->stream, counts, g.n_parts);
        rc = hd_launch_status("ov_scan_kernel");
        if (rc != HIPDSP_OK) return rc;
        HD_OV(2);
    } else {
        HD_OV(0);
    }
#undef HD_OV
    hipLaunchKernelGGL(ov_finish_kernel, dim3(fill_grid), dim3(256), 0, ctx->stream, (const int *)keys, rows,
                       (long long)channels, unwrap ? 1 : 0, scale, out_rc, (long long)out_pitch);
    return hd_launch_status("ov_finish_kernel");
}

}  // extern "C"
