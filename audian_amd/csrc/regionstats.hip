// hipdsp_region_stats: count, mean, standard deviation, minimum, maximum and their first positions of element ranges of
// a planar float32 array, per region and channel -- what the reference's StatisticsAnalyzer (and any analyzer built
// on np.mean / np.std / np.min / np.max / np.argmin / np.argmax) computes of a selected region (include/hip_dsp.h).
//
// A read-once streaming reduction in two launches on the context's stream:
//
//   region_partial_kernel   one workgroup per (chunk, channel).  The chunk grid of a region is anchored at the region's
//                           OWN start and holds RS_CHUNK = 16384 elements per chunk (the last one fewer), so what a
//                           chunk computes depends on nothing but the region: not on the other regions of the call,
//                           not on the number of channels.  A thread holds its 64 samples of the chunk in registers
//                           (HdChunk, rowpass.h: sixteen 16-byte loads, all issued before the first use; the up to
//                           three samples before the first 16-byte boundary and after the last whole vector are loaded
//                           one by one), adds d = x - K and d*d in float64 (K = the region's first sample, the pivot of
//                           the header's accuracy contract) and tracks min, max and the largest |x| bit pattern.  The
//                           workgroup reduces these in a fixed order (wave shuffles, then the four waves through
//                           LDS).  Only then
//                           are positions resolved: a thread whose own minimum equals the workgroup's looks through
//                           its registers for the first such sample -- no select per sample in the streaming part --
//                           and the same for the maximum.  Only a chunk whose largest |x| pattern is not finite looks
//                           for NaN / +inf / -inf and the first NaN.  One 40-byte record per chunk goes to the scratch.
//   region_finish_kernel    one workgroup per (region, channel): thread t adds the records t, t + 256, ... in ascending
//                           order, the 256 threads meet in an LDS tree of fixed shape, thread 0 resolves the special
//                           values from the flags and stores the eight doubles.
//
// The kernel boundary is what makes the records visible to the second launch.  No float atomics anywhere (the LDS
// atomics are integer min / or, which commute), so the same call gives the same bits twice.
// Per sample: one f32->f64 conversion and four float64 operations, two float32 min/max and two integer operations
// against 4 bytes read; the float64 VALU rate is not what limits it.  Index arithmetic on the array is 64-bit.
#include "rowpass.h"

namespace {

constexpr int MAX_REGIONS = 16;
constexpr int RS_THREADS = 256;
constexpr int RS_VEC = 16;                              // 16-byte loads per thread and chunk
typedef HdChunk<RS_THREADS, RS_VEC> RsChunk;
constexpr int RS_CHUNK = RsChunk::CHUNK;                // elements per chunk
constexpr int RS_NONE = 0x7fffffff;                     // "no such sample in this chunk"
constexpr unsigned RS_INF_BITS = 0x7f800000u;
constexpr unsigned RS_NAN = 1, RS_PINF = 2, RS_NINF = 4;

struct RegionArgs {
    long long start[MAX_REGIONS], stop[MAX_REGIONS];
    long long cbase[MAX_REGIONS + 1];                   // first chunk of every region in the grid; [n_regions] = all chunks
    int n_regions;
};

struct RegionPartial {
    double s1, s2;                                      // sum of d, sum of d*d over the chunk
    float mn, mx;
    int imin, imax, inan;                               // first positions relative to the chunk's start, RS_NONE = none
    unsigned flags;
};

struct Lane {
    double s1[4], s2[4];
    float mn, mx;
    unsigned am;
};

__device__ __forceinline__ void rs_take(Lane &l, int k, float x, double K)
{
    const double d = (double)x - K;
    l.s1[k] += d;
    l.s2[k] += d * d;
    l.mn = fminf(l.mn, x);
    l.mx = fmaxf(l.mx, x);
    const unsigned a = __float_as_uint(x) & 0x7fffffffu;
    l.am = a > l.am ? a : l.am;
}

__global__ __launch_bounds__(RS_THREADS) void region_partial_kernel(const float *__restrict__ x, long long pitch, RegionArgs a,
                                                                    long long total_chunks, RegionPartial *__restrict__ part)
{
    __shared__ double sh_s1[4], sh_s2[4];
    __shared__ float sh_mn[4], sh_mx[4];
    __shared__ unsigned sh_am[4];
    __shared__ int sh_idx[3];
    __shared__ unsigned sh_flags;

    const int t = threadIdx.x;
    const long long g = blockIdx.x, c = blockIdx.y;
    int r = 0;
    while (g >= a.cbase[r + 1]) r++;                    // g < cbase[n_regions]; empty regions own no chunk
    const long long j = g - a.cbase[r];
    const float *row = x + c * pitch;
    const float Kf = row[a.start[r]];
    const double K = (double)Kf;
    const RsChunk s(row, a.start[r], a.stop[r], j);
    const int head = s.head, nvec = s.nvec, tail = s.tail;

    // a slot without a sample holds the pivot: d = 0 there, and K is a sample of the region, so min and max stay right
    float4 v[RS_VEC];
    float hx, tx;
    s.load(t, Kf, v, hx, tx);

    Lane l;
#pragma unroll
    for (int k = 0; k < 4; k++) l.s1[k] = l.s2[k] = 0.0;
    l.mn = INFINITY;
    l.mx = -INFINITY;
    l.am = 0;
#pragma unroll
    for (int u = 0; u < RS_VEC; u++) {
        rs_take(l, 0, v[u].x, K);
        rs_take(l, 1, v[u].y, K);
        rs_take(l, 2, v[u].z, K);
        rs_take(l, 3, v[u].w, K);
    }
    rs_take(l, 0, hx, K);
    rs_take(l, 1, tx, K);

    double s1 = (l.s1[0] + l.s1[1]) + (l.s1[2] + l.s1[3]);
    double s2 = (l.s2[0] + l.s2[1]) + (l.s2[2] + l.s2[3]);
    float mn = l.mn, mx = l.mx;
    unsigned am = l.am;
    for (int d = 32; d >= 1; d >>= 1) {
        s1 += __shfl_down(s1, d, 64);
        s2 += __shfl_down(s2, d, 64);
        mn = fminf(mn, __shfl_down(mn, d, 64));
        mx = fmaxf(mx, __shfl_down(mx, d, 64));
        const unsigned o = __shfl_down(am, d, 64);
        am = o > am ? o : am;
    }
    if ((t & 63) == 0) {
        sh_s1[t >> 6] = s1;
        sh_s2[t >> 6] = s2;
        sh_mn[t >> 6] = mn;
        sh_mx[t >> 6] = mx;
        sh_am[t >> 6] = am;
    }
    if (t < 3) sh_idx[t] = RS_NONE;
    if (t == 0) sh_flags = 0;
    __syncthreads();
    const float wmn = fminf(fminf(sh_mn[0], sh_mn[1]), fminf(sh_mn[2], sh_mn[3]));
    const float wmx = fmaxf(fmaxf(sh_mx[0], sh_mx[1]), fmaxf(sh_mx[2], sh_mx[3]));
    unsigned wam = sh_am[0] > sh_am[1] ? sh_am[0] : sh_am[1];
    wam = sh_am[2] > wam ? sh_am[2] : wam;
    wam = sh_am[3] > wam ? sh_am[3] : wam;

    // Positions.  A thread's samples in ascending position: hx (t), v[0] ... v[15] (head + 4*(u*256 + t) + k), tx;
    // they are looked through backwards so that the first match is what remains.
    const int tpos = head + 4 * nvec + t;
    if (l.mn == wmn) {
        int idx = RS_NONE;
        if (t < tail && tx == wmn) idx = tpos;
#pragma unroll
        for (int u = RS_VEC - 1; u >= 0; u--) {
            const int i = u * RS_THREADS + t, at = head + 4 * i;
            if (i < nvec) {
                if (v[u].w == wmn) idx = at + 3;
                if (v[u].z == wmn) idx = at + 2;
                if (v[u].y == wmn) idx = at + 1;
                if (v[u].x == wmn) idx = at;
            }
        }
        if (t < head && hx == wmn) idx = t;
        if (idx != RS_NONE) atomicMin(&sh_idx[0], idx);
    }
    if (l.mx == wmx) {
        int idx = RS_NONE;
        if (t < tail && tx == wmx) idx = tpos;
#pragma unroll
        for (int u = RS_VEC - 1; u >= 0; u--) {
            const int i = u * RS_THREADS + t, at = head + 4 * i;
            if (i < nvec) {
                if (v[u].w == wmx) idx = at + 3;
                if (v[u].z == wmx) idx = at + 2;
                if (v[u].y == wmx) idx = at + 1;
                if (v[u].x == wmx) idx = at;
            }
        }
        if (t < head && hx == wmx) idx = t;
        if (idx != RS_NONE) atomicMin(&sh_idx[1], idx);
    }
    if (wam >= RS_INF_BITS && l.am >= RS_INF_BITS) {
        // a non-finite sample, or the pivot in an empty slot: only real samples count
        int idx = RS_NONE;
        unsigned fl = 0;
        auto look = [&](float s, int at) {
            if (s != s) {
                fl |= RS_NAN;
                idx = at;
            } else if (s == INFINITY) {
                fl |= RS_PINF;
            } else if (s == -INFINITY) {
                fl |= RS_NINF;
            }
        };
        if (t < tail) look(tx, tpos);
#pragma unroll
        for (int u = RS_VEC - 1; u >= 0; u--) {
            const int i = u * RS_THREADS + t, at = head + 4 * i;
            if (i < nvec) {
                look(v[u].w, at + 3);
                look(v[u].z, at + 2);
                look(v[u].y, at + 1);
                look(v[u].x, at);
            }
        }
        if (t < head) look(hx, t);
        if (idx != RS_NONE) atomicMin(&sh_idx[2], idx);
        if (fl) atomicOr(&sh_flags, fl);
    }
    __syncthreads();
    if (t == 0) {
        RegionPartial q;
        hd_moments_block(sh_s1, sh_s2, q.s1, q.s2);
        q.mn = wmn;
        q.mx = wmx;
        q.imin = sh_idx[0];
        q.imax = sh_idx[1];
        q.inan = sh_idx[2];
        q.flags = sh_flags;
        part[c * total_chunks + g] = q;
    }
}

// what the threads of region_finish_kernel merge: sums, and extrema with their first positions in the region
struct Merge {
    double s1, s2;
    float mn, mx;
    long long imin, imax, inan;                         // -1 = none yet
    unsigned flags;
};

// (value, position) pairs: the smaller value wins, equal values keep the earlier position; -1 = no candidate
__device__ __forceinline__ void rs_lower(float &v, long long &i, float ov, long long oi)
{
    if (oi >= 0 && (i < 0 || ov < v || (ov == v && oi < i))) {
        v = ov;
        i = oi;
    }
}
__device__ __forceinline__ void rs_higher(float &v, long long &i, float ov, long long oi)
{
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) {
        v = ov;
        i = oi;
    }
}

__global__ __launch_bounds__(RS_THREADS) void region_finish_kernel(const float *__restrict__ x, long long pitch, RegionArgs a,
                                                                   long long total_chunks,
                                                                   const RegionPartial *__restrict__ part,
                                                                   double *__restrict__ out)
{
    __shared__ Merge sh[RS_THREADS];
    const int t = threadIdx.x;
    const int r = blockIdx.x;
    const long long c = blockIdx.y, channels = gridDim.y;
    const long long n = a.stop[r] - a.start[r];
    const long long nchunks = a.cbase[r + 1] - a.cbase[r];
    const RegionPartial *pp = part + c * total_chunks + a.cbase[r];
    Merge m;
    m.s1 = m.s2 = 0.0;
    m.mn = m.mx = 0.0f;
    m.imin = m.imax = m.inan = -1;
    m.flags = 0;
    for (long long j = t; j < nchunks; j += RS_THREADS) {
        const RegionPartial q = pp[j];
        const long long at = j * RS_CHUNK;
        m.s1 += q.s1;
        m.s2 += q.s2;
        rs_lower(m.mn, m.imin, q.mn, q.imin == RS_NONE ? -1 : at + q.imin);
        rs_higher(m.mx, m.imax, q.mx, q.imax == RS_NONE ? -1 : at + q.imax);
        if (q.inan != RS_NONE && m.inan < 0) m.inan = at + q.inan;
        m.flags |= q.flags;
    }
    sh[t] = m;
    __syncthreads();
    for (int d = RS_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d) {
            const Merge o = sh[t + d];
            m.s1 += o.s1;
            m.s2 += o.s2;
            rs_lower(m.mn, m.imin, o.mn, o.imin);
            rs_higher(m.mx, m.imax, o.mx, o.imax);
            if (o.inan >= 0 && (m.inan < 0 || o.inan < m.inan)) m.inan = o.inan;
            m.flags |= o.flags;
            sh[t] = m;
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double mean = nan, sd = nan, vmin = nan, vmax = nan, amin = -1.0, amax = -1.0;
    if (n > 0) {
        if (m.flags & RS_NAN) {
            amin = amax = (double)m.inan;
        } else {
            vmin = (double)m.mn;
            vmax = (double)m.mx;
            amin = (double)m.imin;
            amax = (double)m.imax;
            if (m.flags & (RS_PINF | RS_NINF)) {
                if (!(m.flags & RS_NINF)) mean = (double)INFINITY;
                else if (!(m.flags & RS_PINF)) mean = -(double)INFINITY;
            } else {
                hd_moments_finish(m.s1, m.s2, (double)n, (double)x[c * pitch + a.start[r]], mean, sd);
            }
        }
    }
    double *o = out + ((long long)r * channels + c) * 8;
    o[0] = (double)n;
    o[1] = mean;
    o[2] = sd;
    o[3] = vmin;
    o[4] = vmax;
    o[5] = amin;
    o[6] = amax;
    o[7] = 0.0;
}

}  // namespace

extern "C" int hipdsp_region_stats(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t frames,
                                   const int64_t *host_start, const int64_t *host_stop, int n_regions, double *out)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(channels >= 0 && frames >= 0, "negative size");
    HD_REQUIRE(n_regions >= 1, "at least one region, got %d", n_regions);
    if (n_regions > MAX_REGIONS) {
        hipdsp_set_error("at most %d regions per call, got %d", MAX_REGIONS, n_regions);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    HD_REQUIRE(host_start != nullptr && host_stop != nullptr, "NULL region list");
    HD_REQUIRE(channels <= HD_MAX_CHANNELS, "too many channels for one call (%lld > 65535)", (long long)channels);
    if (x_pitch == 0) x_pitch = frames;
    HD_REQUIRE(x_pitch >= frames, "x_pitch smaller than frames");
    RegionArgs a;
    memset(&a, 0, sizeof(a));
    a.n_regions = n_regions;
    for (int r = 0; r < n_regions; r++) {
        HD_REQUIRE(host_start[r] >= 0 && host_start[r] <= host_stop[r] && host_stop[r] <= frames,
                   "region %d: elements [%lld, %lld) not inside [0, %lld]", r, (long long)host_start[r],
                   (long long)host_stop[r], (long long)frames);
        a.start[r] = host_start[r];
        a.stop[r] = host_stop[r];
        a.cbase[r + 1] = a.cbase[r] + (host_stop[r] - host_start[r] + RS_CHUNK - 1) / RS_CHUNK;
    }
    for (int r = n_regions; r < MAX_REGIONS; r++) a.cbase[r + 1] = a.cbase[r];
    if (channels == 0) return HIPDSP_OK;
    const long long total = a.cbase[n_regions];
    HD_REQUIRE(out != nullptr && (x != nullptr || total == 0), "NULL data pointer");
    HD_REQUIRE(((uintptr_t)x & 3) == 0, "x is not aligned to 4 bytes");
    HD_REQUIRE(total <= 0x7fffffffLL, "too many elements for one call");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    void *work = nullptr;
    int rc = hipdsp_scratch(ctx, sizeof(RegionPartial) * (size_t)(total > 0 ? total : 1) * (size_t)channels, &work);
    if (rc != HIPDSP_OK) return rc;
    if (total > 0) {
        hipLaunchKernelGGL(region_partial_kernel, dim3((unsigned)total, (unsigned)channels), dim3(RS_THREADS), 0, ctx->stream,
                           x, (long long)x_pitch, a, total, (RegionPartial *)work);
        rc = hd_launch_status("region_partial_kernel");
        if (rc != HIPDSP_OK) return rc;
    }
    hipLaunchKernelGGL(region_finish_kernel, dim3((unsigned)n_regions, (unsigned)channels), dim3(RS_THREADS), 0, ctx->stream,
                       x, (long long)x_pitch, a, total, (const RegionPartial *)work, out);
    return hd_launch_status("region_finish_kernel");
}
