// hipdsp_find_peaks: the local maxima of the rows of a planar float32 array -- flat peaks included, filtered by height,
// by the distance to the two neighbouring samples (threshold) and by prominence (with an optional window wlen) -- as
// ascending positions per channel, with height, prominence and the two bases of every peak (include/hip_dsp.h states
// the definition: scipy.signal.find_peaks with its height, threshold, prominence and wlen arguments).  It is the step
// the reference's songdetector.py takes with sig.find_peaks(envelopes[:,c]) (songdetector.py:110-115) and what fills
// the point events of the reference's README (lines 113-117).
//
// A peak is a run of equal samples v[l..r] with v[l-1] < v[l] and v[r+1] < v[r]; it belongs to the chunk that holds
// r.  Every chunk of PK_CHUNK = 4096 samples (the chunk grid is anchored at `start`) needs two things from outside
// itself: where the run that enters it began (a prefix maximum over the chunks) and its first slot in the output (a
// prefix sum).  v[r+1] is one sample of look-ahead, read by the pass that reads the trace.  Five launches on the
// context's stream, one wave per (chunk, channel) in the three that touch samples:
//
//   pk_bits_kernel    reads the trace once: lane l of the wave loads sample 64*i + l in step i; three ballots per step
//                     -- rise v[p-1] < v[p], fall v[p+1] < v[p], equal v[p] == v[p+1] -- are the chunk's i-th words,
//                     lane i keeps them.  With the tables asked for, the step's minimum and maximum (NaN if the block
//                     holds a NaN: nothing is <= NaN, so such a block is never skipped) go to the bottom level of the
//                     min/max table, and their reduction over the wave to the chunk level.  The chunk's last run start
//                     (a position whose predecessor is not equal to it) is recorded.
//   pk_carry_kernel   one workgroup per channel: exclusive prefix maximum of the last run starts along the chunks
//                     (hd_scan_exclusive, rowpass.h), and the table's top level, one entry per 64 chunks.
//   pk_count_kernel   per fall bit: l from the equal bits (or the carried run start), the rise bit at l, m = (l + r)/2,
//                     height and threshold at m, then -- only if a prominence border is closed -- the prominence.
//                     The peaks kept are counted and their bits stored.
//   pk_slots_kernel   one workgroup per channel: exclusive prefix sum of the counts = every chunk's first slot; the
//                     sum = the channel's count.
//   pk_emit_kernel    walks the kept bits: the lanes' counts are prefix-summed over the wave, every peak is stored at
//                     slot (chunk's first slot + rank) if below capacity, its properties (the search once more, for
//                     kept peaks only) beside it.
//
// The prominence search (pk_walk) is scipy's walk from m while v[i] <= h and inside the window, one thread per peak:
// single samples up to the border of the peak's 64-block, then whole blocks whose maximum is <= h (their minimum comes
// from the table), by 64, 4096 or 262144 samples where aligned and inside the window, then single samples inside the
// block that holds the stopper.  If the minimum came from a table entry its position is found by descending into the
// entry nearest to the peak that holds it.  Worst case per side: 63 + 64 samples, 2 * 63 bottom, 2 * 63 chunk entries
// and (stop - start) / 262144 top entries, then 3 * 64 reads to descend.
//
// A peak's slot comes from the scans and its rank inside its chunk and from nothing else: no atomic anywhere, the same
// call gives the same bytes twice, and a channel's result depends on no other channel.  All comparisons are float32
// comparisons of the samples, which are the float64 comparisons of the exactly converted samples; differences are taken
// in float64.  Index arithmetic on the array is 64-bit.
#include "rowpass.h"

namespace {

constexpr int PK_WORDS = 64;                            // 64-bit words of bits per chunk: one per lane
constexpr int PK_CHUNK = PK_WORDS * 64;                 // samples per chunk
constexpr long long PK_SUPER = 64LL * PK_CHUNK;         // samples per entry of the table's top level
constexpr int PK_SCAN_THREADS = 256;

typedef unsigned long long u64;

struct PkWork {                                         // the scratch of one call
    u64 *rise, *fall, *eq, *kept;                       // [channel][chunk][PK_WORDS]
    float *bmin, *bmax;                                 // [channel][chunk][PK_WORDS]: per 64-sample block
    float *cmin, *cmax;                                 // [channel][chunk]
    float *smin, *smax;                                 // [channel][n_super]: per 64 chunks
    long long *runstart;                                // last run start of the chunk -> of everything before it
    long long *slot;                                    // peaks kept in the chunk -> the chunk's first output slot

    // the arrays of `per` (channel, chunk) pairs and `sup` (channel, 64 chunks) pairs over `block`: their bytes
    size_t carve(void *block, size_t per, size_t sup)
    {
        HdCarve c(block);
        rise = c.take<u64>(per * PK_WORDS);
        fall = c.take<u64>(per * PK_WORDS);
        eq = c.take<u64>(per * PK_WORDS);
        kept = c.take<u64>(per * PK_WORDS);
        runstart = c.take<long long>(per);
        slot = c.take<long long>(per);
        bmin = c.take<float>(per * PK_WORDS);
        bmax = c.take<float>(per * PK_WORDS);
        cmin = c.take<float>(per);
        cmax = c.take<float>(per);
        smin = c.take<float>(sup);
        smax = c.take<float>(sup);
        return c.bytes();
    }
};

struct PkBorders {
    double v[6];                                        // hmin, hmax, tmin, tmax, pmin, pmax
};

struct PkTab {                                          // the min/max table of one channel
    const float *bmin, *bmax, *cmin, *cmax, *smin, *smax;
};

// run starts of a lane's word: positions whose predecessor is not equal to them; `before` = the equal bit of the sample
// before the word
__device__ __forceinline__ u64 pk_run_starts(u64 eq, bool before) { return ~((eq << 1) | (u64)before); }

template <bool TABLE>
__global__ __launch_bounds__(64) void pk_bits_kernel(const float *__restrict__ x, long long pitch, long long start,
                                                     long long stop, long long n_chunks, PkWork w)
{
    const int lane = threadIdx.x;
    const long long j = blockIdx.x, c = blockIdx.y;
    const float *row = x + c * pitch;
    const long long base = start + j * PK_CHUNK;
    u64 rise = 0, fall = 0, eq = 0;
    float mymin = NAN, mymax = NAN;
    for (int i0 = 0; i0 < PK_WORDS; i0 += 8) {
        float v[8], before[8], after[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const long long p = base + (long long)(i0 + u) * 64 + lane;
            v[u] = p < stop ? row[p] : NAN;                         // past `stop`: compares false with everything
            before[u] = after[u] = NAN;
            if (lane == 0 && p > start && p < stop) before[u] = row[p - 1];
            if (lane == 63 && p + 1 < stop) after[u] = row[p + 1];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const float up = __shfl_up(v[u], 1, 64), down = __shfl_down(v[u], 1, 64);
            const float prev = lane == 0 ? before[u] : up, next = lane == 63 ? after[u] : down;
            const u64 r = __ballot(prev < v[u]), f = __ballot(next < v[u]), e = __ballot(v[u] == next);
            if (lane == i0 + u) {
                rise = r;
                fall = f;
                eq = e;
            }
            if (TABLE) {
                const float lo = hd_wave_fmin(v[u]);
                const float hi = __ballot(v[u] != v[u]) ? NAN : hd_wave_fmax(v[u]);
                if (lane == i0 + u) {
                    mymin = lo;
                    mymax = hi;
                }
            }
        }
    }
    const long long cj = c * n_chunks + j;
    const long long at = cj * PK_WORDS + lane;
    w.rise[at] = rise;
    w.fall[at] = fall;
    w.eq[at] = eq;
    if (TABLE) {
        w.bmin[at] = mymin;
        w.bmax[at] = mymax;
        const float lo = hd_wave_fmin(mymin);
        const float hi = __ballot(mymax != mymax) ? NAN : hd_wave_fmax(mymax);
        if (lane == 0) {
            w.cmin[cj] = lo;
            w.cmax[cj] = hi;
        }
    }
    // the last run start of the chunk: the sample before the chunk is equal to its first one?
    const bool entered = j > 0 && row[base - 1] == row[base];
    const u64 up = __shfl_up(eq, 1, 64);
    const long long p0 = base + (long long)lane * 64;
    const u64 inside = stop - p0 >= 64 ? ~(u64)0 : stop - p0 <= 0 ? 0 : ((u64)1 << (stop - p0)) - 1;
    const u64 starts = pk_run_starts(eq, lane == 0 ? entered : (bool)(up >> 63)) & inside;
    const long long last = hd_wave_max(starts ? p0 + 63 - __clzll((long long)starts) : -1);
    if (lane == 0) w.runstart[cj] = last;
}

// runstart[j] <- max of runstart[0 .. j-1] (-1 = none); smin/smax[k] <- min/max of the chunk entries 64k .. 64k + 63
__global__ __launch_bounds__(PK_SCAN_THREADS) void pk_carry_kernel(long long n_chunks, long long n_super, int table, PkWork w)
{
    __shared__ long long sh[PK_SCAN_THREADS];
    const int t = threadIdx.x;
    hd_scan_exclusive<PK_SCAN_THREADS, false>(w.runstart + (long long)blockIdx.x * n_chunks, n_chunks, sh, t, -1, HdMaxOp());
    if (!table) return;
    const float *cmin = w.cmin + (long long)blockIdx.x * n_chunks, *cmax = w.cmax + (long long)blockIdx.x * n_chunks;
    for (long long k = t; k < n_super; k += PK_SCAN_THREADS) {
        float lo = NAN, hi = -INFINITY;
        bool nan = false;
        for (long long i = 64 * k; i < 64 * k + 64 && i < n_chunks; i++) {
            lo = fminf(lo, cmin[i]);
            hi = fmaxf(hi, cmax[i]);
            nan = nan || cmax[i] != cmax[i];
        }
        w.smin[(long long)blockIdx.x * n_super + k] = lo;
        w.smax[(long long)blockIdx.x * n_super + k] = nan ? NAN : hi;
    }
}

// scipy's walk of peak_prominences from m towards `lim` (DIR = +1: right, -1: left) while v[i] <= h: the minimum of
// the samples walked and its position, of equal minima the one nearest to m; m itself if nothing lower was walked.
template <int DIR>
__device__ void pk_walk(const float *__restrict__ row, long long start, long long m, long long lim, float h,
                        const PkTab &t, float &minv, long long &base)
{
    minv = h;
    base = m;
    int level = -1;                                     // the table level the minimum came from, -1: a sample
    long long entry = 0;
    long long i = m + DIR;
    while (DIR > 0 ? i <= lim : i >= lim) {
        const long long rel = i - start;
        const long long edge = DIR > 0 ? rel : rel + 1; // a block begins (ends, walking left) at i?
        if ((edge & 63) == 0 && (DIR > 0 ? i + 63 <= lim : i - 63 >= lim)) {
            if ((edge & (PK_CHUNK - 1)) == 0 && (DIR > 0 ? i + (PK_CHUNK - 1) <= lim : i - (PK_CHUNK - 1) >= lim)) {
                if ((edge & (PK_SUPER - 1)) == 0 && (DIR > 0 ? i + (PK_SUPER - 1) <= lim : i - (PK_SUPER - 1) >= lim)) {
                    const long long k = (DIR > 0 ? rel : rel - (PK_SUPER - 1)) >> 18;
                    if (t.smax[k] <= h) {
                        if (t.smin[k] < minv) {
                            minv = t.smin[k];
                            level = 2;
                            entry = k;
                        }
                        i += DIR * PK_SUPER;
                        continue;
                    }
                }
                const long long k = (DIR > 0 ? rel : rel - (PK_CHUNK - 1)) >> 12;
                if (t.cmax[k] <= h) {
                    if (t.cmin[k] < minv) {
                        minv = t.cmin[k];
                        level = 1;
                        entry = k;
                    }
                    i += DIR * PK_CHUNK;
                    continue;
                }
            }
            const long long k = (DIR > 0 ? rel : rel - 63) >> 6;
            if (t.bmax[k] <= h) {
                if (t.bmin[k] < minv) {
                    minv = t.bmin[k];
                    level = 0;
                    entry = k;
                }
                i += DIR * 64;
                continue;
            }
        }
        const float v = row[i];
        if (!(v <= h)) break;                           // a higher sample or a NaN
        if (v < minv) {
            minv = v;
            base = i;
            level = -1;
        }
        i += DIR;
    }
    // the position of a minimum that came from the table: the entry nearest to m that holds it, level by level
    if (level == 2) {
        long long k = DIR > 0 ? 64 * entry : 64 * entry + 63;
        for (int s = 0; s < 63 && !(t.cmin[k] == minv); s++) k += DIR;
        entry = k;
        level = 1;
    }
    if (level == 1) {
        long long k = DIR > 0 ? 64 * entry : 64 * entry + 63;
        for (int s = 0; s < 63 && !(t.bmin[k] == minv); s++) k += DIR;
        entry = k;
        level = 0;
    }
    if (level == 0) {
        long long p = start + (DIR > 0 ? 64 * entry : 64 * entry + 63);
        for (int s = 0; s < 63 && !(row[p] == minv); s++) p += DIR;
        base = p;
    }
}

// an open border (-inf below, +inf above) is not compared; a NaN border keeps nothing
__device__ __forceinline__ bool pk_inside(double v, double lo, double hi)
{
    return (lo == -INFINITY || lo <= v) && (hi == INFINITY || v <= hi);
}

__device__ __forceinline__ void pk_prominence(const float *__restrict__ row, long long start, long long stop, long long m,
                                              float h, long long wlen, const PkTab &t, double &prom, long long &lb,
                                              long long &rb)
{
    long long lo = start, hi = stop - 1;
    if (wlen >= 2) {
        lo = m - wlen / 2 > lo ? m - wlen / 2 : lo;
        hi = m + wlen / 2 < hi ? m + wlen / 2 : hi;
    }
    float lmin, rmin;
    pk_walk<-1>(row, start, m, lo, h, t, lmin, lb);
    pk_walk<+1>(row, start, m, hi, h, t, rmin, rb);
    prom = (double)h - (double)(lmin > rmin ? lmin : rmin);
}

// What a lane knows of its word (samples p0 .. p0 + 63 of the row): the fall bits, and what it takes to find the run
// start l and the rise bit there of the peak that ends at a fall bit.
struct PkLane {
    u64 rise, fall, starts;
    long long p0;
    long long start_before;                             // last run start in the earlier words of the chunk, or carried
};

__device__ __forceinline__ PkLane pk_lane(const PkWork &w, long long start, long long n_chunks, long long j, long long c,
                                          int lane)
{
    const long long cj = c * n_chunks + j;
    PkLane l;
    l.rise = w.rise[cj * PK_WORDS + lane];
    l.fall = w.fall[cj * PK_WORDS + lane];
    const u64 eq = w.eq[cj * PK_WORDS + lane];
    l.p0 = start + j * PK_CHUNK + (long long)lane * 64;
    const u64 up = __shfl_up(eq, 1, 64);
    const bool entered = j > 0 && (w.eq[cj * PK_WORDS - 1] >> 63);     // the last equal bit of the chunk before
    l.starts = pk_run_starts(eq, lane == 0 ? entered : (bool)(up >> 63));
    long long ls = l.starts ? l.p0 + 63 - __clzll((long long)l.starts) : -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(ls, d, 64);
        if (lane >= d && o > ls) ls = o;
    }
    l.start_before = __shfl_up(ls, 1, 64);
    const long long carried = w.runstart[cj];
    if (lane == 0 || carried > l.start_before) l.start_before = carried;
    return l;
}

// the peak whose run ends at bit b of the lane's word (a fall bit): false if the signal did not rise into the run,
// else its middle m
__device__ __forceinline__ bool pk_peak_at(const PkWork &w, const PkLane &l, long long start, long long n_chunks,
                                           long long c, int b, long long &m)
{
    const u64 upto = l.starts & (b < 63 ? ((u64)1 << (b + 1)) - 1 : ~(u64)0);
    const long long first = upto ? l.p0 + 63 - __clzll((long long)upto) : l.start_before;
    bool rose;
    if (first >= l.p0) rose = (l.rise >> (first - l.p0)) & 1;
    else {
        const long long rel = first - start;            // first >= start: the first sample of the range starts a run
        rose = (w.rise[c * n_chunks * PK_WORDS + (rel >> 6)] >> (rel & 63)) & 1;
    }
    m = (first + l.p0 + b) / 2;
    return rose;
}

__device__ __forceinline__ PkTab pk_table(const PkWork &w, long long n_chunks, long long n_super, long long c)
{
    PkTab t;
    t.bmin = w.bmin + c * n_chunks * PK_WORDS;
    t.bmax = w.bmax + c * n_chunks * PK_WORDS;
    t.cmin = w.cmin + c * n_chunks;
    t.cmax = w.cmax + c * n_chunks;
    t.smin = w.smin + c * n_super;
    t.smax = w.smax + c * n_super;
    return t;
}

__global__ __launch_bounds__(64) void pk_count_kernel(const float *__restrict__ x, long long pitch, long long start,
                                                      long long stop, long long n_chunks, long long n_super,
                                                      const double *__restrict__ dev_borders, PkBorders by_value,
                                                      long long wlen, PkWork w)
{
    const int lane = threadIdx.x;
    const long long j = blockIdx.x, c = blockIdx.y;
    const float *row = x + c * pitch;
    PkBorders bd = by_value;
    if (dev_borders)
        for (int k = 0; k < 6; k++) bd.v[k] = dev_borders[6 * c + k];
    const bool heights = !(bd.v[0] == -INFINITY && bd.v[1] == INFINITY);
    const bool thresholds = !(bd.v[2] == -INFINITY && bd.v[3] == INFINITY);
    const bool prominences = !(bd.v[4] == -INFINITY && bd.v[5] == INFINITY);
    const PkLane l = pk_lane(w, start, n_chunks, j, c, lane);
    const PkTab tab = pk_table(w, n_chunks, n_super, c);
    u64 kept = 0;
    for (u64 f = l.fall; f; f &= f - 1) {
        const int b = __ffsll((long long)f) - 1;
        long long m;
        if (!pk_peak_at(w, l, start, n_chunks, c, b, m)) continue;
        bool keep = true;
        if (heights || thresholds || prominences) {
            const float h = row[m];
            if (heights) keep = pk_inside((double)h, bd.v[0], bd.v[1]);
            if (keep && thresholds) {
                // min(tl, tr) and max(tl, tr) as numpy takes them: a NaN difference (inf - inf) fails a closed border
                const double tl = (double)h - (double)row[m - 1], tr = (double)h - (double)row[m + 1];
                keep = pk_inside(tl, bd.v[2], bd.v[3]) && pk_inside(tr, bd.v[2], bd.v[3]);
            }
            if (keep && prominences) {
                double prom;
                long long lb, rb;
                pk_prominence(row, start, stop, m, h, wlen, tab, prom, lb, rb);
                keep = pk_inside(prom, bd.v[4], bd.v[5]);
            }
        }
        if (keep) kept |= (u64)1 << b;
    }
    const long long cj = c * n_chunks + j;
    w.kept[cj * PK_WORDS + lane] = kept;
    long long n = __popcll(kept);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if (lane == 0) w.slot[cj] = n;
}

// slot[j] <- sum of slot[0 .. j-1]; counts[channel] <- the sum over all chunks
__global__ __launch_bounds__(PK_SCAN_THREADS) void pk_slots_kernel(long long n_chunks, PkWork w, long long *__restrict__ counts)
{
    __shared__ long long sh[PK_SCAN_THREADS];
    __shared__ long long sh_total;
    const int t = threadIdx.x;
    hd_scan_exclusive<PK_SCAN_THREADS, false>(w.slot + (long long)blockIdx.x * n_chunks, n_chunks, sh, t, 0, HdSumOp(),
                                              &sh_total);
    if (t == 0) counts[blockIdx.x] = sh_total;
}

__global__ __launch_bounds__(64) void pk_emit_kernel(const float *__restrict__ x, long long pitch, long long start,
                                                     long long stop, long long n_chunks, long long n_super,
                                                     long long wlen, PkWork w, long long capacity,
                                                     long long *__restrict__ peaks, long long peaks_pitch,
                                                     double *__restrict__ props, long long props_pitch)
{
    const int lane = threadIdx.x;
    const long long j = blockIdx.x, c = blockIdx.y;
    const long long cj = c * n_chunks + j;
    const float *row = x + c * pitch;
    const PkLane l = pk_lane(w, start, n_chunks, j, c, lane);
    const PkTab tab = pk_table(w, n_chunks, n_super, c);
    const u64 kept = w.kept[cj * PK_WORDS + lane];
    const int mine = __popcll(kept);
    long long at = w.slot[cj] + hd_wave_exclusive(mine, lane);
    for (u64 f = kept; f && at < capacity; f &= f - 1, at++) {
        const int b = __ffsll((long long)f) - 1;
        long long m;
        pk_peak_at(w, l, start, n_chunks, c, b, m);
        peaks[c * peaks_pitch + at] = m;
        if (props) {
            const float h = row[m];
            double prom;
            long long lb, rb;
            pk_prominence(row, start, stop, m, h, wlen, tab, prom, lb, rb);
            double *out = props + c * props_pitch + 4 * at;
            out[0] = (double)h;
            out[1] = prom;
            out[2] = (double)lb;
            out[3] = (double)rb;
        }
    }
}

}  // namespace

extern "C" int hipdsp_find_peaks(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t start,
                                 int64_t stop, const double *dev_borders, double hmin, double hmax, double tmin,
                                 double tmax, double pmin, double pmax, int64_t wlen, int64_t capacity, int64_t *peaks,
                                 int64_t peaks_pitch, double *props, int64_t props_pitch, int64_t *counts)
{
    HD_TRY(hd_check_rows(ctx, channels, start, stop));
    HD_REQUIRE(wlen >= 0, "negative wlen");
    HD_REQUIRE(capacity >= 0, "negative capacity");
    if (peaks_pitch == 0) peaks_pitch = capacity;
    if (props_pitch == 0) props_pitch = 4 * capacity;
    HD_REQUIRE(peaks_pitch >= capacity, "peaks_pitch smaller than capacity");
    HD_REQUIRE(props_pitch >= 4 * capacity, "props_pitch smaller than 4*capacity");
    HD_TRY(hd_check_rows_limits(channels, stop - start, HD_MAX_FRAMES));
    if (channels == 0) return HIPDSP_OK;
    HD_REQUIRE(counts != nullptr, "counts is NULL");
    HD_REQUIRE(peaks != nullptr || capacity == 0, "peaks is NULL with a capacity of %lld", (long long)capacity);
    HD_REQUIRE(((uintptr_t)counts & 7) == 0 && ((uintptr_t)peaks & 7) == 0 && ((uintptr_t)props & 7) == 0 &&
                   ((uintptr_t)dev_borders & 7) == 0,
               "counts, peaks, props or dev_borders not aligned to 8 bytes");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    if (stop == start) {
        HD_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)channels, ctx->stream));
        return HIPDSP_OK;
    }
    HD_TRY(hd_check_rows_x(x, x_pitch, channels, start, stop));
    if (capacity == 0) props = nullptr;
    const long long n_chunks = (stop - start + PK_CHUNK - 1) / PK_CHUNK;
    const long long n_super = (n_chunks + 63) / 64;
    const size_t per = (size_t)n_chunks * (size_t)channels, sup = (size_t)n_super * (size_t)channels;
    PkWork w;
    void *work = nullptr;
    HD_TRY(hipdsp_scratch(ctx, w.carve(nullptr, per, sup), &work));
    w.carve(work, per, sup);
    PkBorders bd = {{hmin, hmax, tmin, tmax, pmin, pmax}};
    // the min/max table serves the prominence search only: per-channel borders on the device may ask for it
    const bool table = props != nullptr || dev_borders != nullptr || !(pmin == -INFINITY && pmax == INFINITY);
    const dim3 grid((unsigned)n_chunks, (unsigned)channels);
    if (table)
        hipLaunchKernelGGL(pk_bits_kernel<true>, grid, dim3(64), 0, ctx->stream, x, (long long)x_pitch, (long long)start,
                           (long long)stop, n_chunks, w);
    else
        hipLaunchKernelGGL(pk_bits_kernel<false>, grid, dim3(64), 0, ctx->stream, x, (long long)x_pitch,
                           (long long)start, (long long)stop, n_chunks, w);
    hipLaunchKernelGGL(pk_carry_kernel, dim3((unsigned)channels), dim3(PK_SCAN_THREADS), 0, ctx->stream, n_chunks, n_super,
                       (int)table, w);
    hipLaunchKernelGGL(pk_count_kernel, grid, dim3(64), 0, ctx->stream, x, (long long)x_pitch, (long long)start,
                       (long long)stop, n_chunks, n_super, dev_borders, bd, (long long)wlen, w);
    hipLaunchKernelGGL(pk_slots_kernel, dim3((unsigned)channels), dim3(PK_SCAN_THREADS), 0, ctx->stream, n_chunks, w,
                       (long long *)counts);
    if (capacity > 0)
        hipLaunchKernelGGL(pk_emit_kernel, grid, dim3(64), 0, ctx->stream, x, (long long)x_pitch, (long long)start,
                           (long long)stop, n_chunks, n_super, (long long)wlen, w, (long long)capacity,
                           (long long *)peaks, (long long)peaks_pitch, props, (long long)props_pitch);
    return hd_launch_status("peak detection kernels");
}
