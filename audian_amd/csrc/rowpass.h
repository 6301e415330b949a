// What the analysis units (regionstats, histogram, events, peaks, regionspectra, regionfilter, regionxcorr) share: the
// 16-byte-phased chunk a thread holds in registers, wave reductions, the exclusive scan of one channel's [chunk] array, the
// four-wave sum and the finish of the two shifted moments, the owner lookup of a region table; on the host the row-range
// checks, the intake of a (channel, start, stop) table and the carving of the context scratch.  Every piece has at least two
// users.
#pragma once
#include "common.h"
#include <cmath>

constexpr long long HD_MAX_CHANNELS = 65535;            // grid.y
constexpr long long HD_MAX_FRAMES = 1LL << 40;          // stop - start of one call of the bit-word passes

#define HD_TRY(expr)                                                              \
    do {                                                                          \
        const int _rc = (expr);                                                   \
        if (_rc != HIPDSP_OK) return _rc;                                         \
    } while (0)

// ---- device: the chunk -------------------------------------------------------------------------------------------------

// Chunk j of the elements [start, stop) of a row, CHUNK elements (the last one fewer), as THREADS threads hold it in
// registers: [0, head) single samples up to the first 16-byte boundary, then nvec whole vectors, then tail < 4 samples.
template <int THREADS, int VEC>
struct HdChunk {
    static constexpr int CHUNK = THREADS * VEC * 4;
    const float *p;
    const float4 *vp;
    int head, nvec, tail;

    __device__ __forceinline__ HdChunk(const float *row, long long start, long long stop, long long j)
    {
        const long long b0 = start + j * CHUNK;
        const long long left = stop - b0;
        const int len = left < CHUNK ? (int)left : CHUNK;
        p = row + b0;
        head = (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u);
        if (head > len) head = len;
        nvec = (len - head) >> 2;
        tail = (len - head) & 3;                        // = len - head - 4 * nvec
        vp = (const float4 *)(p + head);
    }

    // thread t's samples: vector u * THREADS + t into v[u] (all VEC loads issued before the first use), sample t of the
    // head and of the tail; a slot without a sample holds `fill`
    __device__ __forceinline__ void load(int t, float fill, float4 (&v)[VEC], float &hx, float &tx) const
    {
#pragma unroll
        for (int u = 0; u < VEC; u++) {
            const int i = u * THREADS + t;
            v[u] = i < nvec ? vp[i] : make_float4(fill, fill, fill, fill);
        }
        hx = t < head ? p[t] : fill;
        tx = t < tail ? p[head + 4 * nvec + t] : fill;
    }
};

// ---- device: over the 64 lanes of a wave -------------------------------------------------------------------------------

__device__ __forceinline__ long long hd_wave_max(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ long long hd_wave_min(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ float hd_wave_fmin(float v)  // NaN operands are ignored
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ float hd_wave_fmax(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

// the sum of v over the lanes in front of this one
__device__ __forceinline__ int hd_wave_exclusive(int v, int lane)
{
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    return incl - v;
}

// ---- device: exclusive scan of one channel's [chunk] array by one workgroup -----------------------------------------------

struct HdMaxOp {
    __device__ __forceinline__ long long operator()(long long run, long long v) const { return v > run ? v : run; }
};
struct HdMinOp {
    __device__ __forceinline__ long long operator()(long long run, long long v) const { return v < run ? v : run; }
};
struct HdSumOp {
    __device__ __forceinline__ long long operator()(long long run, long long v) const { return run + v; }
};

// thread t owns the contiguous elements [a, b) of n (the last threads possibly none)
struct HdSlice {
    long long a, b;
};

template <int THREADS>
__device__ __forceinline__ HdSlice hd_slice(long long n, int t)
{
    const long long per = (n + THREADS - 1) / THREADS;
    HdSlice s;
    s.a = per * t < n ? per * t : n;
    s.b = s.a + per < n ? s.a + per : n;
    return s;
}

// `mine` = op over the thread's slice; returns op over the slices in front of it (BACK: behind it), `identity` for none:
// thread 0 joins the THREADS values serially in sh[THREADS].  *total (LDS, or NULL) receives op over all slices; it is
// visible to every thread on return.  The caller's barrier stands between two uses of one sh.
template <int THREADS, bool BACK, class Op>
__device__ __forceinline__ long long hd_scan_carry(long long *sh, int t, long long mine, long long identity, Op op,
                                                   long long *total = nullptr)
{
    sh[t] = mine;
    __syncthreads();
    if (t == 0) {
        long long run = identity;
        for (int i = 0; i < THREADS; i++) {
            const int k = BACK ? THREADS - 1 - i : i;
            const long long v = sh[k];
            sh[k] = run;
            run = op(run, v);
        }
        if (total) *total = run;
    }
    __syncthreads();
    return sh[t];
}

// v[i] <- op over v[0 .. i-1] (BACK: over v[i+1 ..]), in place
template <int THREADS, bool BACK, class Op>
__device__ __forceinline__ void hd_scan_exclusive(long long *v, long long n, long long *sh, int t, long long identity, Op op,
                                                  long long *total = nullptr)
{
    const HdSlice s = hd_slice<THREADS>(n, t);
    long long m = identity;
    for (long long i = s.a; i < s.b; i++) m = op(m, v[i]);
    long long run = hd_scan_carry<THREADS, BACK>(sh, t, m, identity, op, total);
    for (long long k = 0; k < s.b - s.a; k++) {
        const long long i = BACK ? s.b - 1 - k : s.a + k;
        const long long x = v[i];
        v[i] = run;
        run = op(run, x);
    }
}

// ---- device: the two shifted moments of a workgroup of four waves -------------------------------------------------------

// Sum of d = x - K and of d*d over a chunk: lane 0 of every wave has left its wave's sums in sh_s1/sh_s2[4] (the shuffle
// loop stays in the kernels, where it also reduces what only they track); after the barrier the four waves in a fixed order
__device__ __forceinline__ void hd_moments_block(const double *sh_s1, const double *sh_s2, double &s1, double &s2)
{
    s1 = (sh_s1[0] + sh_s1[1]) + (sh_s1[2] + sh_s1[3]);
    s2 = (sh_s2[0] + sh_s2[1]) + (sh_s2[2] + sh_s2[3]);
}

// mean and standard deviation of n > 0 samples from their moments about the pivot K
__device__ __forceinline__ void hd_moments_finish(double s1, double s2, double n, double K, double &mean, double &sd)
{
    const double md = s1 / n;
    double var = s2 / n - md * md;
    if (!(var > 0.0)) var = 0.0;
    mean = K + md;
    sd = sqrt(var);
}

// ---- device: region tables ---------------------------------------------------------------------------------------------

// The last of the n rows of an uploaded table whose first work item (column `base`, ascending) is <= g: the region that
// owns work item g (empty regions own none).
template <class Row>
__device__ __forceinline__ int hd_owner(const Row *__restrict__ tab, long long Row::*base, int n, long long g)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].*base <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- host: the calls over the elements [start, stop) of every row --------------------------------------------------------

// what they check first
static inline int hd_check_rows(hipdsp_ctx *ctx, int64_t channels, int64_t start, int64_t stop)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(channels >= 0, "negative number of channels");
    HD_REQUIRE(start >= 0 && start <= stop, "elements [%lld, %lld) are no range", (long long)start, (long long)stop);
    return HIPDSP_OK;
}

// what one call serves; max_frames 0: no limit on stop - start here
static inline int hd_check_rows_limits(int64_t channels, int64_t frames, long long max_frames)
{
    if (channels > HD_MAX_CHANNELS) {
        hipdsp_set_error("at most %lld channels per call, got %lld", HD_MAX_CHANNELS, (long long)channels);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    if (max_frames && frames > max_frames) {
        hipdsp_set_error("at most 2^40 elements per row and call, got %lld", (long long)frames);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    return HIPDSP_OK;
}

// the data pointer: needed unless there is nothing to read
static inline int hd_check_rows_x(const float *x, int64_t x_pitch, int64_t channels, int64_t start, int64_t stop)
{
    HD_REQUIRE(x_pitch >= stop || channels <= 1, "x_pitch smaller than stop");
    HD_REQUIRE(x != nullptr || stop == start || channels == 0, "NULL data pointer");
    HD_REQUIRE(((uintptr_t)x & 3) == 0, "x is not aligned to 4 bytes");
    return HIPDSP_OK;
}

// ---- host: a (channel, start, stop) table in host memory -----------------------------------------------------------------

// The checks of the calls that take one; x_pitch 0 becomes `frames`.  The table goes to the device by a copy the call
// waits for, so `who` is refused during stream capture.
static inline int hd_check_table(const char *who, hipdsp_ctx *ctx, const float *x, int64_t &x_pitch, int64_t channels,
                                 int64_t frames, const int64_t *host_regions, int64_t n_regions, long long max_regions)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(channels >= 0 && frames >= 0 && n_regions >= 0, "negative size");
    if (x_pitch == 0) x_pitch = frames;
    HD_REQUIRE(x_pitch >= frames, "x_pitch smaller than frames");
    if (n_regions == 0) return HIPDSP_OK;
    HD_REQUIRE(host_regions != nullptr, "NULL region table");
    HD_REQUIRE(((uintptr_t)x & 3) == 0, "misaligned pointer");
    HD_REQUIRE(n_regions < max_regions, "too many regions for one call (%lld)", (long long)n_regions);
    for (int64_t r = 0; r < n_regions; r++) {
        const int64_t c = host_regions[3 * r], a = host_regions[3 * r + 1], b = host_regions[3 * r + 2];
        HD_REQUIRE(c >= 0 && c < channels, "region %lld: channel %lld not in [0, %lld)", (long long)r, (long long)c,
                   (long long)channels);
        HD_REQUIRE(a >= 0 && a <= b && b <= frames, "region %lld: elements [%lld, %lld) not inside [0, %lld]", (long long)r,
                   (long long)a, (long long)b, (long long)frames);
    }
    if (hd_capturing(ctx)) {
        hipdsp_set_error("%s reads its region table from host memory: not during stream capture", who);
        return HIPDSP_ERR_INVALID;
    }
    return HIPDSP_OK;
}

// the caller's table to the front of its scratch; the table is a local: the copy has to be complete before it goes away
static inline int hd_upload_table(hipdsp_ctx *ctx, void *work, const void *tab, size_t bytes)
{
    HD_CHECK_HIP(hipMemcpyAsync(work, tab, bytes, hipMemcpyHostToDevice, ctx->stream));
    HD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return HIPDSP_OK;
}

// ---- host: the context scratch as typed arrays ---------------------------------------------------------------------------

// Hands out consecutive arrays of one block, each aligned for its type.  Over base 0 it only counts: a call lays its
// arrays out once with base 0 for bytes(), asks hipdsp_scratch() for that many and lays them out again over the block.
struct HdCarve {
    uintptr_t base;
    size_t used = 0;
    explicit HdCarve(void *block) : base((uintptr_t)block) {}
    template <class T>
    T *take(size_t n)
    {
        used = (used + alignof(T) - 1) / alignof(T) * alignof(T);
        T *p = (T *)(base + used);
        used += sizeof(T) * n;
        return p;
    }
    size_t bytes() const { return used; }
};
