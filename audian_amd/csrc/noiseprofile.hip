// hipdsp_bin_quantiles / hipdsp_spec_equalize: the per-bin noise profile of a spectrogram slab and the slab divided by
// (or reduced by) it (include/hip_dsp.h).
//
// bin_quantiles_kernel is an exact radix select per COLUMN of the planar slab (channels, frames, nfreq): the values of
// one column lie nfreq floats apart, the columns of neighbouring bins are contiguous.  A workgroup of 16 waves takes
// one channel and a tile of 64 consecutive bins; lane l of every wave owns column l of the tile, so a frame's 64 bins
// are one coalesced 256-byte read, and the 16 waves take the frames w, w + 16, ...  The float becomes an
// order-preserving 32-bit key (negative: ~bits, else bits | 2^31; -0 first becomes +0, NaN is left out) and the select
// runs from the most significant 8-bit digit down, four passes, each a read of the tile's elements:
//   hist[digit*64 + column]   256 x 64 counters in LDS.  The column is the fast index: the 64 lanes of a wave hit 64
//                             different banks and never the same counter, so the LDS atomics of one instruction never
//                             conflict; counters only meet across waves.
//   part[wave*64 + column]    the sum of the 16 digits wave w owns, per column: after it every thread finds, for ITS
//                             column, the 16-digit chunk and then the digit that holds the rank -- 16 + 16 LDS reads,
//                             lanes along the columns (conflict-free), the 16 waves redundantly: the selection state
//                             (prefix, rank) lives in registers and needs no broadcast.
// Both order statistics come out of the same passes: as long as rank k_hi = k_lo + 1 falls into the digit of k_lo they
// share the prefix; at the pass where it does not, v[k_hi] is the smallest key of the next non-empty digit: the later
// passes take that minimum with an LDS atomicMin per column beside the histogram (at the last pass the digit IS the
// key).  No global atomics, no scratch; every scalar travels by value.
//
// spec_equalize_kernel is a streaming pass: a workgroup takes 8192 consecutive elements of one channel, keeps the
// profile row in LDS (rows of up to 4096 bins; longer ones are read through the cache), and moves float4 where the row
// of the input and of the output reach 16-byte alignment at the same element, with a scalar head and tail; dwords else.
#include "common.h"

namespace {

constexpr int QT_COLS = 64, QT_WAVES = 16, QT_THREADS = QT_COLS * QT_WAVES, QT_DIGITS = 256;
constexpr int QT_CHUNK = QT_DIGITS / QT_WAVES;      // digits a wave sums per column
constexpr long long QT_MAX_ELEMS = 1LL << 44;       // elements of a channel or a pitch: 65535 of them at 4 bytes stay inside int64
constexpr int QT_LOADS = 8;                         // rows in flight per wave

// the order-preserving key of a float that is not NaN: negative values ~bits, the others bits | 2^31; -0 counts as +0
__device__ __forceinline__ unsigned qt_key(float v)
{
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    return b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
}

__device__ __forceinline__ float qt_value(unsigned key)
{
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__global__ __launch_bounds__(QT_THREADS) void bin_quantiles_kernel(const float *__restrict__ spec, long long spec_pitch,
                                                                   long long first_elem, long long row_stride, int n_frames,
                                                                   int k0, int k1, double q, float *__restrict__ out,
                                                                   int *__restrict__ out_count)
{
    __shared__ unsigned hist[QT_DIGITS * QT_COLS];
    __shared__ unsigned part[QT_WAVES * QT_COLS];
    __shared__ unsigned himin[QT_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long c = blockIdx.y;
    const int kt = k0 + (int)blockIdx.x * QT_COLS;
    const int col = kt + lane;
    const bool live = col < k1;
    const float *p = spec + c * spec_pitch + first_elem + (live ? col : kt);

    // the selection state of this thread's column (the same in all 16 waves): the digits chosen so far, in place in
    // `prefix`; once rank k_hi has left the digit of k_lo, the keys with (key & hmask) == hval hold v[k_hi] as their minimum
    unsigned prefix = 0, rank = 0, n = 0, delta = 0, hmask = 0, hval = 1, hi_key = 0;
    bool split = false, hi_known = false;

    if (threadIdx.x < QT_COLS) himin[threadIdx.x] = 0xffffffffu;
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        const unsigned above = pass == 0 ? 0u : 0xffffffffu << (shift + 8);     // the digits chosen in the passes before
        for (int i = threadIdx.x; i < QT_DIGITS * QT_COLS; i += QT_THREADS) hist[i] = 0u;
        __syncthreads();
        if (live) {
            // (a pointer that walks and no predicates in the body: the vector work per element is part of what a pass costs)
            auto take = [&](float v) {
                const unsigned key = qt_key(v);
                if (v == v) {
                    if ((key & above) == prefix) atomicAdd(&hist[((key >> shift) & 255u) * QT_COLS + lane], 1u);
                    if ((key & hmask) == hval) atomicMin(&himin[lane], key);
                }
            };
            const long long hop = QT_WAVES * row_stride;      // elements between a wave's consecutive frames
            const float *r = p + wave * row_stride;
            long long j = wave;
            for (; j + (QT_LOADS - 1) * QT_WAVES < n_frames; j += QT_LOADS * QT_WAVES, r += QT_LOADS * hop) {
                float v[QT_LOADS];
#pragma unroll
                for (int u = 0; u < QT_LOADS; u++) v[u] = r[u * hop];
#pragma unroll
                for (int u = 0; u < QT_LOADS; u++) take(v[u]);
            }
            for (; j < n_frames; j += QT_WAVES, r += hop) take(*r);
        }
        __syncthreads();
        {
            unsigned s = 0;
#pragma unroll
            for (int d = 0; d < QT_CHUNK; d++) s += hist[(wave * QT_CHUNK + d) * QT_COLS + lane];
            part[wave * QT_COLS + lane] = s;
        }
        __syncthreads();
        if (pass == 0) {
            for (int w = 0; w < QT_WAVES; w++) n += part[w * QT_COLS + lane];
            if (n > 0) {
                const double pos = q * (double)(n - 1);
                unsigned lo = (unsigned)floor(pos);
                if (lo > n - 1) lo = n - 1;
                rank = lo;
                delta = (lo + 1 <= n - 1) ? 1u : 0u;
            }
        }
        if (n > 0) {
            // the chunk of 16 digits, then the digit, that holds `rank`; cum = the elements below it
            unsigned cum = 0, cnt = 0;
            int wsel = QT_WAVES - 1, dsel = QT_DIGITS - 1;
            bool found = false;
            for (int w = 0; w < QT_WAVES; w++) {
                const unsigned pw = part[w * QT_COLS + lane];
                if (!found) {
                    if (rank < cum + pw) { found = true; wsel = w; }
                    else cum += pw;
                }
            }
            found = false;
            for (int d = 0; d < QT_CHUNK; d++) {
                const unsigned cd = hist[(wsel * QT_CHUNK + d) * QT_COLS + lane];
                if (!found) {
                    if (rank < cum + cd) { found = true; dsel = wsel * QT_CHUNK + d; cnt = cd; }
                    else cum += cd;
                }
            }
            if (delta && !split && !hi_known && !(rank - cum + 1u < cnt)) {
                // rank k_hi leaves the digit of k_lo: it is the smallest key of the next digit that holds anything
                int dn = -1;
                for (int e = dsel + 1; e < QT_DIGITS && dn < 0;) {
                    if ((e & (QT_CHUNK - 1)) == 0 && part[(e / QT_CHUNK) * QT_COLS + lane] == 0u) { e += QT_CHUNK; continue; }
                    if (hist[e * QT_COLS + lane] != 0u) dn = e;
                    else e++;
                }
                if (dn >= 0) {
                    if (pass < 3) { split = true; hmask = 0xffffffffu << shift; hval = prefix | ((unsigned)dn << shift); }
                    else { hi_known = true; hi_key = prefix | (unsigned)dn; }
                }
            }
            prefix |= (unsigned)dsel << shift;
            rank -= cum;
        }
        __syncthreads();
    }
    if (wave == 0 && live) {
        const long long i = c * (long long)(k1 - k0) + (col - k0);
        float lo = __uint_as_float(0x7fc00000u), hi = lo;
        if (n > 0) {
            lo = qt_value(prefix);
            hi = hi_known ? qt_value(hi_key) : (split ? qt_value(himin[lane]) : lo);
        }
        out[2 * i] = lo;
        out[2 * i + 1] = hi;
        if (out_count != nullptr) out_count[i] = (int)n;
    }
}

constexpr int EQ_THREADS = 256, EQ_UNROLL = 8, EQ_CHUNK = EQ_THREADS * 4 * EQ_UNROLL, EQ_LDS_BINS = 4096;

template <int MODE>
__device__ __forceinline__ float eq_value(float p, float n)
{
    if constexpr (MODE == HIPDSP_EQ_DIVIDE) {
        return (float)((double)p / (double)n);
    } else {
        const float d = p - n;
        return d < 0.0f ? 0.0f : d;
    }
}

// (spec and out may be the same array: no __restrict__ on them; a thread reads its elements before it writes them)
template <int MODE, bool IN_LDS>
__global__ __launch_bounds__(EQ_THREADS) void spec_equalize_kernel(const float *spec, long long spec_pitch, float *out,
                                                                  long long out_pitch, long long total, int nfreq,
                                                                  const float *__restrict__ profile, long long profile_pitch)
{
    __shared__ float prof_s[IN_LDS ? EQ_LDS_BINS : 1];
    const int tid = threadIdx.x;
    const long long c = blockIdx.y;
    const float *s = spec + c * spec_pitch;
    float *o = out + c * out_pitch;
    const float *pr = profile + c * profile_pitch;
    if constexpr (IN_LDS) {
        for (int i = tid; i < nfreq; i += EQ_THREADS) prof_s[i] = pr[i];
        __syncthreads();
    }
    auto prof = [&](unsigned k) -> float {
        if constexpr (IN_LDS) return prof_s[k];
        else return pr[k];
    };
    const unsigned F = (unsigned)nfreq;
    long long head = (long long)(((16u - (unsigned)((uintptr_t)s & 15u)) & 15u) >> 2);
    if (head > total) head = total;
    const bool vec_ok = (((uintptr_t)(o + head)) & 15u) == 0;
    if (!vec_ok) {
        // the two rows never reach 16-byte alignment together: dwords, coalesced
        const long long eb = (long long)blockIdx.x * EQ_CHUNK;
        if (eb >= total) return;
        const unsigned kb = (unsigned)(eb % nfreq);
#pragma unroll 4
        for (int u = 0; u < 4 * EQ_UNROLL; u++) {
            const unsigned off = (unsigned)(u * EQ_THREADS + tid);
            const long long e = eb + off;
            if (e < total) o[e] = eq_value<MODE>(s[e], prof((kb + off) % F));
        }
        return;
    }
    const long long nvec = (total - head) / 4;
    const long long tail0 = head + 4 * nvec;
    if (blockIdx.x == 0) {
        // up to three elements in front of the first aligned one and behind the last whole vector
        long long e = -1;
        if (tid < head) e = tid;
        else if (tid >= 64 && tail0 + (tid - 64) < total) e = tail0 + (tid - 64);
        if (e >= 0) o[e] = eq_value<MODE>(s[e], prof((unsigned)(e % nfreq)));
    }
    const long long vb = (long long)blockIdx.x * (EQ_CHUNK / 4);
    if (vb >= nvec) return;
    const unsigned kb = (unsigned)((head + 4 * vb) % nfreq);
    float4 x[EQ_UNROLL];
#pragma unroll
    for (int u = 0; u < EQ_UNROLL; u++) {
        const long long v = vb + u * EQ_THREADS + tid;
        x[u] = *(const float4 *)(s + head + 4 * (v < nvec ? v : vb));
    }
#pragma unroll
    for (int u = 0; u < EQ_UNROLL; u++) {
        const long long v = vb + u * EQ_THREADS + tid;
        if (v < nvec) {
            unsigned k = (kb + 4u * (unsigned)(u * EQ_THREADS + tid)) % F;
            float4 y;
            y.x = eq_value<MODE>(x[u].x, prof(k));
            k = k + 1 == F ? 0u : k + 1;
            y.y = eq_value<MODE>(x[u].y, prof(k));
            k = k + 1 == F ? 0u : k + 1;
            y.z = eq_value<MODE>(x[u].z, prof(k));
            k = k + 1 == F ? 0u : k + 1;
            y.w = eq_value<MODE>(x[u].w, prof(k));
            *(float4 *)(o + head + 4 * v) = y;
        }
    }
}

template <int MODE, bool IN_LDS>
int eq_launch(hipdsp_ctx *ctx, const float *spec, long long spec_pitch, float *out, long long out_pitch, long long channels,
              long long total, int nfreq, const float *profile, long long profile_pitch)
{
    const dim3 grid((unsigned)((total + EQ_CHUNK - 1) / EQ_CHUNK), (unsigned)channels);
    hipLaunchKernelGGL((spec_equalize_kernel<MODE, IN_LDS>), grid, dim3(EQ_THREADS), 0, ctx->stream, spec, spec_pitch, out,
                       out_pitch, total, nfreq, profile, profile_pitch);
    return hd_launch_status("spec_equalize_kernel");
}

}  // namespace

extern "C" int hipdsp_bin_quantiles(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, int64_t channels, int64_t frames,
                                    int64_t nfreq, int64_t first, int64_t n_frames, int64_t frame_step, int64_t k0,
                                    int64_t k1, double q, float *out_lo_hi, int32_t *out_count)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(channels >= 0 && frames >= 0 && nfreq >= 0 && n_frames >= 0 && spec_pitch >= 0, "negative size");
    HD_REQUIRE(q >= 0.0 && q <= 1.0, "q must lie in [0, 1], got %g", q);
    HD_REQUIRE(nfreq < (1LL << 30), "nfreq out of range");
    HD_REQUIRE(k0 >= 0 && k0 <= k1 && k1 <= nfreq, "bins [%lld, %lld) not inside [0, %lld]", (long long)k0, (long long)k1,
               (long long)nfreq);
    HD_REQUIRE(frame_step >= 1, "frame_step must be at least 1, got %lld", (long long)frame_step);
    if (n_frames >= (1LL << 31) || channels > 65535) {
        hipdsp_set_error("at most 2^31 - 1 frames and 65535 channels per call, got %lld and %lld", (long long)n_frames,
                         (long long)channels);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    // (frames * nfreq, first * nfreq and (channels - 1) * spec_pitch in bytes all stay inside int64)
    HD_REQUIRE((nfreq == 0 || frames <= QT_MAX_ELEMS / nfreq) && spec_pitch <= QT_MAX_ELEMS,
               "frames * nfreq or spec_pitch out of range");
    HD_REQUIRE(first >= 0 && (n_frames == 0 || (first < frames && (frames - 1 - first) / frame_step >= n_frames - 1)),
               "frames first %lld, count %lld, step %lld not inside [0, %lld)", (long long)first, (long long)n_frames,
               (long long)frame_step, (long long)frames);
    if (spec_pitch == 0) spec_pitch = frames * nfreq;
    HD_REQUIRE(spec_pitch >= frames * nfreq, "spec_pitch smaller than one channel");
    if (channels == 0 || k1 == k0) return HIPDSP_OK;
    HD_REQUIRE(out_lo_hi != nullptr && (spec != nullptr || n_frames == 0), "NULL data pointer");
    const long long cols = channels * (k1 - k0);
    const long long spec_bytes = 4 * ((channels - 1) * spec_pitch + frames * nfreq);
    HD_REQUIRE(!hd_bytes_overlap(out_lo_hi, 8 * cols, spec, spec_bytes) && !hd_bytes_overlap(out_count, 4 * cols, spec, spec_bytes) &&
               !hd_bytes_overlap(out_lo_hi, 8 * cols, out_count, 4 * cols), "the outputs must not overlap the slab or each other");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((k1 - k0 + QT_COLS - 1) / QT_COLS), (unsigned)channels);
    hipLaunchKernelGGL(bin_quantiles_kernel, grid, dim3(QT_THREADS), 0, ctx->stream, spec, (long long)spec_pitch,
                       (long long)(first * nfreq), (long long)(n_frames > 1 ? frame_step * nfreq : 0), (int)n_frames, (int)k0,
                       (int)k1, q, out_lo_hi, (int *)out_count);
    return hd_launch_status("bin_quantiles_kernel");
}

extern "C" int hipdsp_spec_equalize(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, float *out, int64_t out_pitch,
                                    int64_t channels, int64_t frames, int64_t nfreq, const float *profile,
                                    int64_t profile_pitch, int mode)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(channels >= 0 && frames >= 0 && nfreq >= 0 && spec_pitch >= 0 && out_pitch >= 0 && profile_pitch >= 0,
               "negative size");
    HD_REQUIRE(mode == HIPDSP_EQ_DIVIDE || mode == HIPDSP_EQ_SUBTRACT, "unknown mode %d", mode);
    HD_REQUIRE(nfreq < (1LL << 30), "nfreq out of range");
    if (channels > 65535) {
        hipdsp_set_error("at most 65535 channels per call, got %lld", (long long)channels);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    HD_REQUIRE((nfreq == 0 || frames <= QT_MAX_ELEMS / nfreq) && spec_pitch <= QT_MAX_ELEMS &&
               out_pitch <= QT_MAX_ELEMS && profile_pitch <= QT_MAX_ELEMS,
               "frames * nfreq or a pitch out of range");
    const long long total = frames * nfreq;
    if (spec_pitch == 0) spec_pitch = total;
    if (out_pitch == 0) out_pitch = total;
    if (profile_pitch == 0) profile_pitch = nfreq;
    HD_REQUIRE(spec_pitch >= total && out_pitch >= total, "a slab pitch is smaller than one channel");
    HD_REQUIRE(profile_pitch >= nfreq, "profile_pitch smaller than nfreq");
    if (channels == 0 || total == 0) return HIPDSP_OK;
    HD_REQUIRE(spec != nullptr && out != nullptr && profile != nullptr, "NULL data pointer");
    HD_REQUIRE((out == spec && out_pitch == spec_pitch) ||
               !hd_planar_overlap(spec, spec_pitch, total, out, out_pitch, total, channels),
               "out must be spec itself (same pitch) or not overlap it");
    HD_REQUIRE(!hd_planar_overlap(profile, profile_pitch, nfreq, out, out_pitch, total, channels),
               "out must not overlap the profile");
    HD_REQUIRE((total + EQ_CHUNK - 1) / EQ_CHUNK <= 0x7fffffffLL, "too many elements per channel for one call");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    const bool in_lds = nfreq <= EQ_LDS_BINS;
    if (mode == HIPDSP_EQ_DIVIDE)
        return in_lds ? eq_launch<HIPDSP_EQ_DIVIDE, true>(ctx, spec, spec_pitch, out, out_pitch, channels, total, (int)nfreq,
                                                          profile, profile_pitch)
                      : eq_launch<HIPDSP_EQ_DIVIDE, false>(ctx, spec, spec_pitch, out, out_pitch, channels, total, (int)nfreq,
                                                           profile, profile_pitch);
    return in_lds ? eq_launch<HIPDSP_EQ_SUBTRACT, true>(ctx, spec, spec_pitch, out, out_pitch, channels, total, (int)nfreq,
                                                        profile, profile_pitch)
                  : eq_launch<HIPDSP_EQ_SUBTRACT, false>(ctx, spec, spec_pitch, out, out_pitch, channels, total, (int)nfreq,
                                                         profile, profile_pitch);
}
