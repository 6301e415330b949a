// hipdsp_detect_events: threshold events of the rows of a planar float32 array -- maximal runs of samples above a
// threshold, runs closer than a minimum gap merged, merged events shorter than a minimum length dropped -- as
// half-open (onset, offset) index pairs per channel, in ascending order (include/hip_dsp.h states the definition).
// It is the step the reference's songdetector.py takes between an envelope and its region analysis (detect_songs:
// threshold crossings, merge_events, remove_events, songdetector.py:113-139).  thunderlab, which supplies those three
// functions, is neither installed nor part of the reference tree: merging and filtering follow songdetector.py's USE
// of them -- UNVERIFIED against thunderlab (parity unpinned); the contract is the definition in the header.
//
// Merging looks sequential but is not: with above[i] = x[i] > thr,
//   i is the onset of a merged event      iff above[i] and the last above sample before i is absent or more than
//                                             min_gap samples that are not above lie between the two,
//   i is the last sample of a merged event iff above[i] and the same holds of the first above sample after i,
// onsets and last samples alternate along the row, and the length filter looks at one such pair.  So every chunk of
// EV_CHUNK = 4096 samples (the chunk grid is anchored at `start`) needs only four values from outside itself: the
// last above sample before it, the first one after it, the last onset before it and its first slot in the output.
// Five launches on the context's stream, one wave per (chunk, channel) in the three that touch samples:
//
//   ev_bits_kernel    reads the trace once: lane l of the wave loads sample 64*i + l in step i, the wave's ballot of
//                     x > thr is the chunk's i-th word of `above` bits, lane i keeps it.  64 words per chunk go to the
//                     scratch, with the first and last above position of the chunk (absolute, or none).
//   ev_carry_kernel   one workgroup per channel: exclusive prefix maximum of the last positions and exclusive suffix
//                     minimum of the first ones along the chunks, in place (hd_scan_exclusive, rowpass.h: a thread owns
//                     a contiguous span of chunks, thread 0 joins the 256 spans).
//   ev_count_kernel   from the bits and the two carried positions: the chunk's onsets and last samples, each last
//                     sample paired with the nearest onset at or before it; events whose pair lies in the chunk are
//                     counted if long enough.  The one event that can end in a chunk and begin before it is left
//                     pending (the position of its last sample), and the chunk's last onset is recorded.
//   ev_slots_kernel   one workgroup per channel: exclusive prefix maximum of the last onsets; with it the pending
//                     events are decided; exclusive prefix sum of the counts = every chunk's first slot; the sum = the
//                     channel's count.
//   ev_emit_kernel    ev_count_kernel's walk again, now with the carried onset; the lanes' counts are prefix-summed
//                     over the wave and every event is stored at slot (chunk's first slot + rank), if below capacity.
//
// An event is counted and stored by the chunk that holds its LAST sample.  Its slot comes from the two scans and the
// rank inside the chunk and from nothing else: no atomic anywhere, the same call gives the same bytes twice, and a
// channel's result depends on no other channel (a workgroup never looks at another channel's data).
//
// Traffic per sample and channel: 4 B read once, 1/8 B of bits written and 2/8 B read, 40 B of carries per chunk of
// 4096 samples: about 4.4 B where three passes over the trace would move 12.  Index arithmetic on the array is 64-bit.
#include "rowpass.h"

namespace {

constexpr int EV_WORDS = 64;                            // 64-bit words of `above` bits per chunk: one per lane
constexpr int EV_CHUNK = EV_WORDS * 64;                 // samples per chunk
constexpr int EV_SCAN_THREADS = 256;
constexpr long long EV_NONE_AFTER = 0x3fffffffffffffffLL;   // "no above sample after": further than any gap

typedef unsigned long long u64;

struct EvWork {                                         // the scratch of one call; [channel][chunk] each
    u64 *bits;                                          // [channel][chunk][EV_WORDS]
    long long *before;                                  // last above position of the chunk -> of everything before it
    long long *after;                                   // first above position of the chunk -> of everything after it
    long long *onset;                                   // last onset of the chunk -> of everything before it
    long long *pending;                                 // last sample of the event that ends here and began earlier, -1
    long long *slot;                                    // events counted in the chunk -> the chunk's first output slot

    size_t carve(void *block, size_t per)               // the arrays of `per` (channel, chunk) pairs over `block`: their bytes
    {
        HdCarve c(block);
        bits = c.take<u64>(per * EV_WORDS);
        before = c.take<long long>(per);
        after = c.take<long long>(per);
        onset = c.take<long long>(per);
        pending = c.take<long long>(per);
        slot = c.take<long long>(per);
        return c.bytes();
    }
};

__global__ __launch_bounds__(64) void ev_bits_kernel(const float *__restrict__ x, long long pitch, long long start,
                                                     long long stop, const float *__restrict__ thresholds, float threshold,
                                                     long long n_chunks, EvWork w)
{
    const int lane = threadIdx.x;
    const long long j = blockIdx.x, c = blockIdx.y;
    const float thr = thresholds ? thresholds[c] : threshold;
    const float *row = x + c * pitch;
    const long long base = start + j * EV_CHUNK;
    u64 word = 0;
    for (int i0 = 0; i0 < EV_WORDS; i0 += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const long long p = base + (long long)(i0 + u) * 64 + lane;
            v[u] = p < stop ? row[p] : -INFINITY;               // past `stop`: above no threshold
        }
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const u64 m = __ballot(v[u] > thr);                 // NaN is not above
            if (lane == i0 + u) word = m;
        }
    }
    const long long at = (c * n_chunks + j) * EV_WORDS + lane;
    w.bits[at] = word;
    const long long p0 = base + (long long)lane * 64;
    const long long first = hd_wave_min(word ? p0 + __ffsll((long long)word) - 1 : EV_NONE_AFTER);
    const long long last = hd_wave_max(word ? p0 + 63 - __clzll((long long)word) : -1);
    if (lane == 0) {
        w.after[c * n_chunks + j] = first;
        w.before[c * n_chunks + j] = last;
    }
}

// before[j] <- max of before[0 .. j-1] (-1 = none), after[j] <- min of after[j+1 ..] (EV_NONE_AFTER = none)
__global__ __launch_bounds__(EV_SCAN_THREADS) void ev_carry_kernel(long long n_chunks, EvWork w)
{
    __shared__ long long sh_b[EV_SCAN_THREADS], sh_a[EV_SCAN_THREADS];
    const int t = threadIdx.x;
    hd_scan_exclusive<EV_SCAN_THREADS, false>(w.before + (long long)blockIdx.x * n_chunks, n_chunks, sh_b, t, -1, HdMaxOp());
    hd_scan_exclusive<EV_SCAN_THREADS, true>(w.after + (long long)blockIdx.x * n_chunks, n_chunks, sh_a, t, EV_NONE_AFTER,
                                             HdMinOp());
}

// What a lane knows of its word (samples p0 .. p0 + 63 of the row) once the neighbours are in: the onsets and the last
// samples of merged events as bit masks, and the last onset before the word as far as the chunk knows it.
struct EvLane {
    u64 on, end;
    long long p0;
    long long on_before;                                // last onset in the earlier words of the chunk, or `carried`
};

__device__ __forceinline__ EvLane ev_lane(const EvWork &w, long long start, long long n_chunks, long long j, long long c,
                                          int lane, long long min_gap, long long carried_onset)
{
    const long long cj = c * n_chunks + j;
    const u64 word = w.bits[cj * EV_WORDS + lane];
    EvLane l;
    l.p0 = start + j * EV_CHUNK + (long long)lane * 64;
    // the last above sample before the word and the first one after it: over the earlier / later lanes, then the carries
    long long lb = word ? l.p0 + 63 - __clzll((long long)word) : -1;
    long long fa = word ? l.p0 + __ffsll((long long)word) - 1 : EV_NONE_AFTER;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long ob = __shfl_up(lb, d, 64), oa = __shfl_down(fa, d, 64);
        if (lane >= d && ob > lb) lb = ob;
        if (lane + d < 64 && oa < fa) fa = oa;
    }
    long long prev = __shfl_up(lb, 1, 64), next = __shfl_down(fa, 1, 64);
    const long long cb = w.before[cj], ca = w.after[cj];
    if (lane == 0) prev = -1;
    if (lane == 63) next = EV_NONE_AFTER;
    prev = cb > prev ? cb : prev;
    next = ca < next ? ca : next;

    // runs of the word: a run starts where the sample before is not above, ends where the sample after is not
    const u64 rs = word & ~((word << 1) | (u64)(prev >= 0 && prev == l.p0 - 1));    // (-1 = none, also when p0 is 0)
    const u64 re = word & ~((word >> 1) | ((u64)(next == l.p0 + 64) << 63));
    l.on = l.end = 0;
    for (u64 m = rs; m; m &= m - 1) {
        const int b = __ffsll((long long)m) - 1;
        const u64 below = word & (((u64)1 << b) - 1);
        const long long p = below ? l.p0 + 63 - __clzll((long long)below) : prev;
        if (p < 0 || l.p0 + b - p - 1 > min_gap) l.on |= (u64)1 << b;
    }
    for (u64 m = re; m; m &= m - 1) {
        const int b = __ffsll((long long)m) - 1;
        const u64 above = b < 63 ? word >> (b + 1) : 0;
        const long long p = above ? l.p0 + b + __ffsll((long long)above) : next;
        if (p == EV_NONE_AFTER || p - (l.p0 + b) - 1 > min_gap) l.end |= (u64)1 << b;
    }
    long long lo = l.on ? l.p0 + 63 - __clzll((long long)l.on) : -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(lo, d, 64);
        if (lane >= d && o > lo) lo = o;
    }
    l.on_before = __shfl_up(lo, 1, 64);
    if (lane == 0) l.on_before = -1;
    if (carried_onset > l.on_before) l.on_before = carried_onset;
    return l;
}

// the onset that belongs to the last sample at bit b of the lane's word: the nearest onset at or before it (-1: not
// in this chunk and nothing carried in)
__device__ __forceinline__ long long ev_onset_of(const EvLane &l, int b)
{
    const u64 upto = l.on & (b < 63 ? ((u64)1 << (b + 1)) - 1 : ~(u64)0);
    return upto ? l.p0 + 63 - __clzll((long long)upto) : l.on_before;
}

__global__ __launch_bounds__(64) void ev_count_kernel(long long start, long long n_chunks, long long min_gap,
                                                      long long min_len, EvWork w)
{
    const int lane = threadIdx.x;
    const long long j = blockIdx.x, c = blockIdx.y;
    const EvLane l = ev_lane(w, start, n_chunks, j, c, lane, min_gap, -1);
    long long kept = 0, pending = -1;
    for (u64 m = l.end; m; m &= m - 1) {
        const int b = __ffsll((long long)m) - 1;
        const long long on = ev_onset_of(l, b);
        if (on < 0) pending = l.p0 + b;                 // began in an earlier chunk: ev_slots_kernel decides
        else if (l.p0 + b + 1 - on >= min_len) kept++;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) kept += __shfl_xor(kept, d, 64);
    pending = hd_wave_max(pending);                     // at most one lane has one
    const long long last_on = hd_wave_max(l.on ? l.p0 + 63 - __clzll((long long)l.on) : -1);
    if (lane == 0) {
        w.slot[c * n_chunks + j] = kept;
        w.pending[c * n_chunks + j] = pending;
        w.onset[c * n_chunks + j] = last_on;
    }
}

// onset[j] <- max of onset[0 .. j-1]; slot[j] <- sum over the chunks before j of (counted + pending event kept);
// counts[channel] <- the sum over all chunks
__global__ __launch_bounds__(EV_SCAN_THREADS) void ev_slots_kernel(long long n_chunks, long long min_len, EvWork w,
                                                                   long long *__restrict__ counts)
{
    __shared__ long long sh[EV_SCAN_THREADS];
    __shared__ long long sh_total;
    const int t = threadIdx.x;
    long long *onset = w.onset + (long long)blockIdx.x * n_chunks;
    long long *slot = w.slot + (long long)blockIdx.x * n_chunks;
    const long long *pending = w.pending + (long long)blockIdx.x * n_chunks;
    const HdSlice s = hd_slice<EV_SCAN_THREADS>(n_chunks, t);
    long long m = -1;
    for (long long i = s.a; i < s.b; i++) m = onset[i] > m ? onset[i] : m;
    long long run = hd_scan_carry<EV_SCAN_THREADS, false>(sh, t, m, -1, HdMaxOp()), sum = 0;
    for (long long i = s.a; i < s.b; i++) {
        const long long v = onset[i], p = pending[i];
        onset[i] = run;
        // a pending event has its onset in an earlier chunk (onsets and last samples alternate): run >= 0 then
        if (p >= 0 && run >= 0 && p + 1 - run >= min_len) slot[i] += 1;
        sum += slot[i];
        run = v > run ? v : run;
    }
    __syncthreads();                                    // every thread has its onset carry out of sh
    run = hd_scan_carry<EV_SCAN_THREADS, false>(sh, t, sum, 0, HdSumOp(), &sh_total);
    for (long long i = s.a; i < s.b; i++) {
        const long long v = slot[i];
        slot[i] = run;
        run += v;
    }
    if (t == 0) counts[blockIdx.x] = sh_total;
}

__global__ __launch_bounds__(64) void ev_emit_kernel(long long start, long long n_chunks, long long min_gap,
                                                     long long min_len, EvWork w, long long capacity,
                                                     long long *__restrict__ events, long long events_pitch)
{
    const int lane = threadIdx.x;
    const long long j = blockIdx.x, c = blockIdx.y;
    const long long cj = c * n_chunks + j;
    const EvLane l = ev_lane(w, start, n_chunks, j, c, lane, min_gap, w.onset[cj]);
    int kept = 0;
    for (u64 m = l.end; m; m &= m - 1) {
        const int b = __ffsll((long long)m) - 1;
        const long long on = ev_onset_of(l, b);
        if (on >= 0 && l.p0 + b + 1 - on >= min_len) kept++;
    }
    long long at = w.slot[cj] + hd_wave_exclusive(kept, lane);
    long long *out = events + c * events_pitch;
    for (u64 m = l.end; m; m &= m - 1) {
        const int b = __ffsll((long long)m) - 1;
        const long long on = ev_onset_of(l, b);
        if (on >= 0 && l.p0 + b + 1 - on >= min_len) {
            if (at < capacity) {
                out[2 * at] = on;
                out[2 * at + 1] = l.p0 + b + 1;
            }
            at++;
        }
    }
}

}  // namespace

extern "C" int hipdsp_detect_events(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t start,
                                    int64_t stop, const float *dev_thresholds, double threshold, int64_t min_gap,
                                    int64_t min_len, int64_t capacity, int64_t *events, int64_t events_pitch,
                                    int64_t *counts)
{
    HD_TRY(hd_check_rows(ctx, channels, start, stop));
    HD_REQUIRE(min_gap >= 0 && min_len >= 0, "negative min_gap or min_len");
    HD_REQUIRE(capacity >= 0, "negative capacity");
    if (events_pitch == 0) events_pitch = 2 * capacity;
    HD_REQUIRE(events_pitch >= 2 * capacity, "events_pitch smaller than 2*capacity");
    HD_TRY(hd_check_rows_limits(channels, stop - start, HD_MAX_FRAMES));
    if (channels == 0) return HIPDSP_OK;
    HD_REQUIRE(counts != nullptr, "counts is NULL");
    HD_REQUIRE(events != nullptr || capacity == 0, "events is NULL with a capacity of %lld", (long long)capacity);
    HD_REQUIRE(((uintptr_t)counts & 7) == 0 && ((uintptr_t)events & 7) == 0, "counts or events not aligned to 8 bytes");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    if (stop == start) {
        HD_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)channels, ctx->stream));
        return HIPDSP_OK;
    }
    HD_TRY(hd_check_rows_x(x, x_pitch, channels, start, stop));
    const long long n_chunks = (stop - start + EV_CHUNK - 1) / EV_CHUNK;
    const size_t per = (size_t)n_chunks * (size_t)channels;
    EvWork w;
    void *work = nullptr;
    HD_TRY(hipdsp_scratch(ctx, w.carve(nullptr, per), &work));
    w.carve(work, per);
    const dim3 grid((unsigned)n_chunks, (unsigned)channels);
    hipLaunchKernelGGL(ev_bits_kernel, grid, dim3(64), 0, ctx->stream, x, (long long)x_pitch, (long long)start,
                       (long long)stop, dev_thresholds, (float)threshold, n_chunks, w);
    hipLaunchKernelGGL(ev_carry_kernel, dim3((unsigned)channels), dim3(EV_SCAN_THREADS), 0, ctx->stream, n_chunks, w);
    hipLaunchKernelGGL(ev_count_kernel, grid, dim3(64), 0, ctx->stream, (long long)start, n_chunks, (long long)min_gap,
                       (long long)min_len, w);
    hipLaunchKernelGGL(ev_slots_kernel, dim3((unsigned)channels), dim3(EV_SCAN_THREADS), 0, ctx->stream, n_chunks,
                       (long long)min_len, w, (long long *)counts);
    if (capacity > 0)
        hipLaunchKernelGGL(ev_emit_kernel, grid, dim3(64), 0, ctx->stream, (long long)start, n_chunks,
                           (long long)min_gap, (long long)min_len, w, (long long)capacity, (long long *)events,
                           (long long)events_pitch);
    return hd_launch_status("event detection kernels");
}
