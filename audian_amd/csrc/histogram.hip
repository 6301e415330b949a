// hipdsp_histogram and hipdsp_masked_stats: the amplitude histogram of every row of a planar float32 array over given
// bin edges, and count, mean and standard deviation of the samples of every row inside an amplitude window -- the two
// reductions the reference's histogram threshold is made of (threshold_estimates, songdetector.py:85-117: a 49-bin
// histogram, moments of the samples below a bin edge, the mean of the samples above mean + 3 std).  include/hip_dsp.h
// states both definitions.
//
// Both read the trace once, on the chunk grid of regionstats.hip: one workgroup of 256 threads per (chunk, channel), the
// grid anchored at `start`, HG_CHUNK = 16384 elements per chunk (the last one fewer).  A thread holds its 64 samples of
// the chunk in registers (HdChunk, rowpass.h).  What a chunk computes depends on nothing but [start, stop) and the row:
// not on the number of channels.
//
//   hg_edges_kernel    the edges travel to the device BY VALUE, 256 float64 per launch (at most five launches for 1025
//                      edges, one for the 50 of the reference): no upload, no host synchronisation, the host array is
//                      consumed when the call returns.  They land in the context scratch.
//   hg_zero_kernel     zeroes the (channels, n_bins + 3) counts.
//   hg_count_kernel    edges to LDS as float64; one table of n_bins + 3 32-bit counts PER WAVE in LDS.  A sample's bin:
//                      a guess k = (x - e[0]) * B / (e[B] - e[0]), corrected by comparing against e[k] and e[k+1] (two
//                      steps, then a binary search) -- exact for any edges, O(1) for uniform ones, where the guess
//                      holds but for a rounding and costs two LDS reads and two compares.  An envelope puts most
//                      samples into one or two bins and lanes that add to one LDS address serialise, so before the add
//                      the wave counts by ballot the lanes that share the bin of its first active lane -- in all four
//                      samples of the lanes' float4 at once -- and adds that count once; after HG_ROUNDS = 2 such
//                      rounds the remaining samples are added one by one.  The four tables are merged after a barrier
//                      and every non-zero bin is added to `out` with ONE 64-bit integer atomic per bin and workgroup.
//   mask_partial_kernel / mask_finish_kernel
//                      the region-stats reduction under the predicate lo < x < hi: d = x - pivot and d*d in float64 over
//                      the selected samples (an unselected sample adds exact zeros), four accumulators per lane, wave
//                      shuffles, the four waves through LDS, one 24-byte record (S1, S2, n) per chunk to the scratch;
//                      the second launch adds the records t, t + 256, ... per thread in ascending order and merges the
//                      256 threads in an LDS tree of fixed shape.
//
// Determinism: the only atomics are integer adds (LDS 32-bit, global 64-bit), whose sum does not depend on arrival order;
// the float64 sums are merged in a fixed order.  The same call gives the same bytes twice, and a workgroup never looks at
// another channel's data.  Index arithmetic on the array is 64-bit.
#include "rowpass.h"
#include <cmath>

namespace {

constexpr int HG_THREADS = 256;
constexpr int HG_VEC = 16;                              // 16-byte loads per thread and chunk
typedef HdChunk<HG_THREADS, HG_VEC> HgChunk;
constexpr int HG_CHUNK = HgChunk::CHUNK;                // elements per chunk
constexpr int HG_MAX_BINS = 1024;
constexpr int HG_ROUNDS = 2;                            // ballot rounds before the lanes add one by one
constexpr int HG_EDGE_BATCH = 256;                      // edges per hg_edges_kernel launch (2 KiB of kernel arguments)

typedef unsigned long long u64;

struct EdgeBatch {
    double e[HG_EDGE_BATCH];
};

__global__ __launch_bounds__(HG_EDGE_BATCH) void hg_edges_kernel(EdgeBatch b, int at, int n, double *__restrict__ dst)
{
    const int t = threadIdx.x;
    if (t < n) dst[at + t] = b.e[t];
}

__global__ __launch_bounds__(HG_THREADS) void hg_zero_kernel(u64 *__restrict__ out, long long out_pitch, int slots)
{
    for (int i = threadIdx.x; i < slots; i += HG_THREADS) out[(long long)blockIdx.x * out_pitch + i] = 0;
}

// The bin of a sample with e[0] <= v <= e[B] whose guess k did not hold: two steps towards it, then a binary search.
__device__ int hg_correct(double v, const double *e, int B, int k)
{
#pragma unroll
    for (int s = 0; s < 2; s++) {
        if (k > 0 && v < e[k]) k--;
        else if (k < B - 1 && v >= e[k + 1]) k++;
    }
    if ((k > 0 && v < e[k]) || (k < B - 1 && v >= e[k + 1])) {
        int lo = 0, hi = B - 1;                         // the largest i in [1, B-1] with e[i] <= v, or 0
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (e[mid] <= v) lo = mid;
            else hi = mid - 1;
        }
        k = lo;
    }
    return k;
}

// The slot of a sample: its bin (the number of interior edges e[1..B-1] that are <= x) when e[0] <= x <= e[B], else
// B (below), B + 1 (above) or B + 2 (NaN).  The bin k is the only one with (k == 0 or e[k] <= x) and (k == B-1 or
// x < e[k+1]), because the edges do not decrease; with e[0] <= x <= e[B] that is e[k] <= x and (x < e[k+1] or k == B-1).
__device__ __forceinline__ int hg_slot(float x, const double *e, int B, double e0, double eB, double scale)
{
    if (x != x) return B + 2;
    const double v = (double)x;
    if (v < e0) return B;
    if (v > eB) return B + 1;
    // fmax(NaN, 0) is 0: a zero or overflowing e[B] - e[0] leaves everything to hg_correct
    const int k = (int)fmin(fmax((v - e0) * scale, 0.0), (double)(B - 1));
    if (v >= e[k] && (v < e[k + 1] || k == B - 1)) return k;    // the guess holds: uniform edges, but for a rounding
    return hg_correct(v, e, B, k);
}

// Four samples per lane into the wave's table (a slot < 0: no sample).  All 64 lanes of the wave call this together.
// A round: the first lane that has a slot left names its first one, four ballots count the lanes that hold it in each
// of the four positions, the naming lane adds the sum once.  What is left after HG_ROUNDS rounds is added one by one.
__device__ __forceinline__ void hg_add4(unsigned *mine, int lane, int s0, int s1, int s2, int s3)
{
#pragma unroll
    for (int r = 0; r < HG_ROUNDS; r++) {
        const int left = s0 >= 0 ? s0 : s1 >= 0 ? s1 : s2 >= 0 ? s2 : s3;
        const u64 active = __ballot(left >= 0);
        if (active == 0) return;                        // the same for the whole wave
        const int first = __ffsll((long long)active) - 1;
        const int fs = __shfl(left, first, 64);
        const unsigned n = (unsigned)(__popcll(__ballot(s0 == fs)) + __popcll(__ballot(s1 == fs)) +
                                      __popcll(__ballot(s2 == fs)) + __popcll(__ballot(s3 == fs)));
        if (lane == first) atomicAdd(&mine[fs], n);
        s0 = s0 == fs ? -1 : s0;
        s1 = s1 == fs ? -1 : s1;
        s2 = s2 == fs ? -1 : s2;
        s3 = s3 == fs ? -1 : s3;
    }
    if (s0 >= 0) atomicAdd(&mine[s0], 1u);
    if (s1 >= 0) atomicAdd(&mine[s1], 1u);
    if (s2 >= 0) atomicAdd(&mine[s2], 1u);
    if (s3 >= 0) atomicAdd(&mine[s3], 1u);
}

__global__ __launch_bounds__(HG_THREADS) void hg_count_kernel(const float *__restrict__ x, long long pitch, long long start,
                                                              long long stop, const double *__restrict__ edges, int B,
                                                              u64 *__restrict__ out, long long out_pitch)
{
    extern __shared__ double hg_lds[];                  // B + 1 edges, then 4 tables of B + 3 counts
    double *e = hg_lds;
    unsigned *tab = (unsigned *)(hg_lds + B + 1);
    const int S = B + 3;
    const int t = threadIdx.x, lane = t & 63;
    const long long j = blockIdx.x, c = blockIdx.y;
    const HgChunk s(x + c * pitch, start, stop, j);

    const float nosample = __uint_as_float(0x7fc00000u);
    float4 v[HG_VEC];
    float hx, tx;
    s.load(t, nosample, v, hx, tx);

    for (int i = t; i <= B; i += HG_THREADS) e[i] = edges[i];
    for (int i = t; i < 4 * S; i += HG_THREADS) tab[i] = 0;
    __syncthreads();
    const double e0 = e[0], eB = e[B];
    const double scale = (double)B / (eB - e0);
    unsigned *mine = tab + (t >> 6) * S;
#pragma unroll
    for (int u = 0; u < HG_VEC; u++) {
        const bool has = u * HG_THREADS + t < s.nvec;
        hg_add4(mine, lane, has ? hg_slot(v[u].x, e, B, e0, eB, scale) : -1, has ? hg_slot(v[u].y, e, B, e0, eB, scale) : -1,
                has ? hg_slot(v[u].z, e, B, e0, eB, scale) : -1, has ? hg_slot(v[u].w, e, B, e0, eB, scale) : -1);
    }
    hg_add4(mine, lane, t < s.head ? hg_slot(hx, e, B, e0, eB, scale) : -1,
            t < s.tail ? hg_slot(tx, e, B, e0, eB, scale) : -1, -1, -1);
    __syncthreads();
    u64 *o = out + c * out_pitch;
    for (int i = t; i < S; i += HG_THREADS) {
        const unsigned n = (tab[i] + tab[S + i]) + (tab[2 * S + i] + tab[3 * S + i]);
        if (n) atomicAdd(&o[i], (u64)n);
    }
}

struct MaskPartial {
    double s1, s2;                                      // sum of d, sum of d*d over the selected samples of the chunk
    long long n;                                        // how many were selected
};

struct MaskLane {
    double s1[4], s2[4];
    int n;
};

__device__ __forceinline__ void mask_take(MaskLane &l, int k, float x, double lo, double hi, double K)
{
    const double v = (double)x;
    const bool sel = v > lo && v < hi;                  // NaN samples and NaN bounds: false; an infinite sample: false
    const double d = sel ? v - K : 0.0;
    l.s1[k] += d;
    l.s2[k] += d * d;
    l.n += sel ? 1 : 0;
}

__global__ __launch_bounds__(HG_THREADS) void mask_partial_kernel(const float *__restrict__ x, long long pitch,
                                                                  long long start, long long stop,
                                                                  const double *__restrict__ bounds, long long n_chunks,
                                                                  MaskPartial *__restrict__ part)
{
    __shared__ double sh_s1[4], sh_s2[4];
    __shared__ int sh_n[4];
    const int t = threadIdx.x;
    const long long j = blockIdx.x, c = blockIdx.y;
    const HgChunk s(x + c * pitch, start, stop, j);
    const double lo = bounds[3 * c], hi = bounds[3 * c + 1], K = bounds[3 * c + 2];

    const float nosample = __uint_as_float(0x7fc00000u);        // a NaN is never selected
    float4 v[HG_VEC];
    float hx, tx;
    s.load(t, nosample, v, hx, tx);

    MaskLane l;
#pragma unroll
    for (int k = 0; k < 4; k++) l.s1[k] = l.s2[k] = 0.0;
    l.n = 0;
#pragma unroll
    for (int u = 0; u < HG_VEC; u++) {
        mask_take(l, 0, v[u].x, lo, hi, K);
        mask_take(l, 1, v[u].y, lo, hi, K);
        mask_take(l, 2, v[u].z, lo, hi, K);
        mask_take(l, 3, v[u].w, lo, hi, K);
    }
    mask_take(l, 0, hx, lo, hi, K);
    mask_take(l, 1, tx, lo, hi, K);

    double s1 = (l.s1[0] + l.s1[1]) + (l.s1[2] + l.s1[3]);
    double s2 = (l.s2[0] + l.s2[1]) + (l.s2[2] + l.s2[3]);
    int n = l.n;
    for (int d = 32; d >= 1; d >>= 1) {
        s1 += __shfl_down(s1, d, 64);
        s2 += __shfl_down(s2, d, 64);
        n += __shfl_down(n, d, 64);
    }
    if ((t & 63) == 0) {
        sh_s1[t >> 6] = s1;
        sh_s2[t >> 6] = s2;
        sh_n[t >> 6] = n;
    }
    __syncthreads();
    if (t == 0) {
        MaskPartial q;
        hd_moments_block(sh_s1, sh_s2, q.s1, q.s2);
        q.n = (long long)((sh_n[0] + sh_n[1]) + (sh_n[2] + sh_n[3]));
        part[c * n_chunks + j] = q;
    }
}

__global__ __launch_bounds__(HG_THREADS) void mask_finish_kernel(const double *__restrict__ bounds, long long n_chunks,
                                                                 const MaskPartial *__restrict__ part,
                                                                 double *__restrict__ out)
{
    __shared__ double sh_s1[HG_THREADS], sh_s2[HG_THREADS];
    __shared__ long long sh_n[HG_THREADS];
    const int t = threadIdx.x;
    const long long c = blockIdx.x;
    const MaskPartial *pp = part + c * n_chunks;
    double s1 = 0.0, s2 = 0.0;
    long long n = 0;
    for (long long j = t; j < n_chunks; j += HG_THREADS) {
        const MaskPartial q = pp[j];
        s1 += q.s1;
        s2 += q.s2;
        n += q.n;
    }
    sh_s1[t] = s1;
    sh_s2[t] = s2;
    sh_n[t] = n;
    __syncthreads();
    for (int d = HG_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d) {
            s1 += sh_s1[t + d];
            s2 += sh_s2[t + d];
            n += sh_n[t + d];
            sh_s1[t] = s1;
            sh_s2[t] = s2;
            sh_n[t] = n;
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double mean = nan, sd = nan;
    if (n > 0) hd_moments_finish(s1, s2, (double)n, bounds[3 * c + 2], mean, sd);
    double *o = out + c * 4;
    o[0] = (double)n;
    o[1] = mean;
    o[2] = sd;
    o[3] = 0.0;
}

// what both entry points ask of x and the range; *n_chunks = chunks of [start, stop)
int hg_check_rows(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t start, int64_t stop,
                  long long *n_chunks)
{
    HD_TRY(hd_check_rows(ctx, channels, start, stop));
    HD_REQUIRE(x_pitch >= 0, "negative x_pitch");
    HD_TRY(hd_check_rows_limits(channels, stop - start, 0));
    HD_TRY(hd_check_rows_x(x, x_pitch, channels, start, stop));
    *n_chunks = (stop - start) / HG_CHUNK + ((stop - start) % HG_CHUNK != 0);
    HD_REQUIRE(*n_chunks <= 0x7fffffffLL, "too many elements for one call");
    return HIPDSP_OK;
}

}  // namespace

extern "C" int hipdsp_histogram(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t start,
                                int64_t stop, const double *host_edges, int n_bins, int64_t *out, int64_t out_pitch)
{
    long long n_chunks = 0;
    int rc = hg_check_rows(ctx, x, x_pitch, channels, start, stop, &n_chunks);
    if (rc != HIPDSP_OK) return rc;
    HD_REQUIRE(host_edges != nullptr, "host_edges is NULL");
    HD_REQUIRE(n_bins >= 1, "at least one bin, got %d", n_bins);
    if (n_bins > HG_MAX_BINS) {
        hipdsp_set_error("at most %d bins per call, got %d", HG_MAX_BINS, n_bins);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    for (int i = 0; i <= n_bins; i++) {
        HD_REQUIRE(std::isfinite(host_edges[i]), "edge %d is not finite", i);
        HD_REQUIRE(i == 0 || host_edges[i] >= host_edges[i - 1], "edge %d is smaller than edge %d", i, i - 1);
    }
    const int slots = n_bins + 3;
    if (out_pitch == 0) out_pitch = slots;
    HD_REQUIRE(out_pitch >= slots, "out_pitch smaller than n_bins + 3");
    if (channels == 0) return HIPDSP_OK;
    HD_REQUIRE(out != nullptr, "out is NULL");
    HD_REQUIRE(((uintptr_t)out & 7) == 0, "out is not aligned to 8 bytes");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(hg_zero_kernel, dim3((unsigned)channels), dim3(HG_THREADS), 0, ctx->stream, (u64 *)out,
                       (long long)out_pitch, slots);
    if (n_chunks == 0) return hd_launch_status("hg_zero_kernel");
    void *work = nullptr;
    rc = hipdsp_scratch(ctx, sizeof(double) * (size_t)(n_bins + 1), &work);
    if (rc != HIPDSP_OK) return rc;
    for (int at = 0; at <= n_bins; at += HG_EDGE_BATCH) {
        EdgeBatch b;
        const int n = n_bins + 1 - at < HG_EDGE_BATCH ? n_bins + 1 - at : HG_EDGE_BATCH;
        memset(&b, 0, sizeof(b));
        memcpy(b.e, host_edges + at, sizeof(double) * (size_t)n);
        hipLaunchKernelGGL(hg_edges_kernel, dim3(1), dim3(HG_EDGE_BATCH), 0, ctx->stream, b, at, n, (double *)work);
    }
    const size_t lds = sizeof(double) * (size_t)(n_bins + 1) + sizeof(unsigned) * 4 * (size_t)slots;
    hipLaunchKernelGGL(hg_count_kernel, dim3((unsigned)n_chunks, (unsigned)channels), dim3(HG_THREADS), lds, ctx->stream, x,
                       (long long)x_pitch, (long long)start, (long long)stop, (const double *)work, n_bins, (u64 *)out,
                       (long long)out_pitch);
    return hd_launch_status("histogram kernels");
}

extern "C" int hipdsp_masked_stats(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t start,
                                   int64_t stop, const double *dev_bounds, double *out)
{
    long long n_chunks = 0;
    int rc = hg_check_rows(ctx, x, x_pitch, channels, start, stop, &n_chunks);
    if (rc != HIPDSP_OK) return rc;
    if (channels == 0) return HIPDSP_OK;
    HD_REQUIRE(dev_bounds != nullptr && out != nullptr, "NULL bounds or output pointer");
    HD_REQUIRE(((uintptr_t)dev_bounds & 7) == 0 && ((uintptr_t)out & 7) == 0, "bounds or out not aligned to 8 bytes");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    void *work = nullptr;
    rc = hipdsp_scratch(ctx, sizeof(MaskPartial) * (size_t)(n_chunks > 0 ? n_chunks : 1) * (size_t)channels, &work);
    if (rc != HIPDSP_OK) return rc;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(mask_partial_kernel, dim3((unsigned)n_chunks, (unsigned)channels), dim3(HG_THREADS), 0,
                           ctx->stream, x, (long long)x_pitch, (long long)start, (long long)stop, dev_bounds, n_chunks,
                           (MaskPartial *)work);
        rc = hd_launch_status("mask_partial_kernel");
        if (rc != HIPDSP_OK) return rc;
    }
    hipLaunchKernelGGL(mask_finish_kernel, dim3((unsigned)channels), dim3(HG_THREADS), 0, ctx->stream, dev_bounds, n_chunks,
                       (const MaskPartial *)work, out);
    return hd_launch_status("mask_finish_kernel");
}
