// Common-reference subtraction across channels (gfx950): y[c, t] = float(double(x[c, t]) - ref_g[t]) for the members c of
// group g, ref_g[t] the mean or the median over the group's reference channels at sample t (include/hip_dsp.h:
// hipdsp_common_reference).  The trace is planar, so the reduction runs across rows at one time index and lanes run along
// time.  Every sample leaves HBM once: the reference channels' time tile stays on chip between the reduction and the
// subtraction, and members that do not contribute (use == 0, pass-through copies) are streamed after the reference is known.
//
// Where the tile lives.  cref_reg_kernel (any median, means of up to 64 reference channels) keeps it in REGISTERS: a lane
// owns V consecutive frames of every reference row, NP x V floats for NP = 8/16/32/64 row slots -- V = 4 (16-byte
// accesses, 1024 frames per workgroup) up to 16 slots, V = 2 (8-byte accesses, 512 frames) for 32 and 64.  The register
// file has 512 entries per lane and wave: at NP = 64 the tile is 128 of them, the median's sort copy 64 more, and
// hipcc's schedule (it converts to float64 early) ends at 336 (mean) and 410 (median) VGPRs + AGPRs, no scratch: one
// wave per SIMD, which still has 64 x 8 B loads per lane in flight (128 KiB per CU).  With V = 4 there the allocation
// hit 512 and spilled, and a cap at two waves per SIMD spilled too.  At NP = 16 (four groups of 16) it is 152 ... 166
// registers, three waves per SIMD; at NP = 8 five.  The same tile in LDS would be 128 KiB per 256-thread workgroup at NP = 64
// and would add a 4 B LDS write and read per sample to a kernel whose only other traffic is the 8 B of HBM --
// registers need neither.  All loads of a tile are issued back to back before the first use (a slot beyond the
// group's reference count loads the last row again rather than sit under a branch: a load in a basic block of its own
// is waited for at the block's end, which ran the 64 rows one HBM latency after the other, 17.8 instead of 6.4 ms).
// cref_lds_kernel serves means over 65 ... 1024 reference channels, which no register file holds: 32 frames of up to 1024
// rows in 128 KiB of LDS (one workgroup per CU), 32 lanes add the rows up in channel order.  It is the limit case of
// the interface, not the tuned path.
//
// The median is a per-lane selection: Batcher's odd-even merge sort as straight-line v_min_f32 / v_max_f32 on registers
// with compile-time indices.  The n reference values are padded to NP slots with floor((NP - n) / 2) times -inf and
// the rest +inf, so that the two middle values always land in slots NP/2 - 1 and NP/2 whatever n is; only those two
// outputs are used and the compiler drops every exchange half that does not feed them.  min/max drop NaNs, so a flag
// rides along and makes the reference NaN (as numpy does).  -0 == +0 for min/max: the sign of a zero result is
// not specified.
//
// Rows may start at any 4-byte boundary (odd pitches): the 8- and 16-byte accesses are typed 4-byte aligned, which the
// hardware serves at any dword address -- with two odd pitches no head could align the rows of x and of y at once;
// a workgroup whose tile runs over the end of the rows takes the guarded form with single-float accesses.  Plain
// vector stores only, no atomics.
//
// The group table travels by value in the kernel arguments (CrefTable, 2.8 KB for up to 1024 channels): no upload, no
// scratch, legal inside a stream capture.
#include "common.h"
#include <cmath>

namespace {

constexpr int CR_MAXCH = 1024;
constexpr int CR_WORDS = (CR_MAXCH + 2) / 3;         // three 10-bit fields per word

// Jobs are the groups in ascending id and, out of place, one copy job of all pass-through channels.  `order` lists the
// channels job by job, within a job the reference channels in ascending order, then the other members in ascending
// order; `starts[j]` is the first position of job j; bit p of `use` says that position p is a reference channel.
struct CrefTable {
    unsigned int order[CR_WORDS];
    unsigned int starts[CR_WORDS];
    unsigned int use[CR_MAXCH / 32];
    int total, njobs, copy_job;                      // positions in use; jobs; index of the copy job or -1
};

__host__ __device__ __forceinline__ int cr_field(const unsigned int *w, int i) { return (int)((w[i / 3] >> (10 * (i % 3))) & 1023u); }

// reference channels of the job [s, e): the set bits of that range of `use`
__device__ __forceinline__ int cr_refs(const CrefTable &tab, int s, int e)
{
    int n = 0;
    for (int w = s >> 5; w <= (e - 1) >> 5; w++) {
        unsigned int m = tab.use[w];
        const int lo = w << 5;
        if (s > lo) m &= ~0u << (s - lo);
        if (e < lo + 32) m &= ~0u >> (lo + 32 - e);
        n += __builtin_popcount(m);
    }
    return n;
}

typedef float cr_f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float cr_f2 __attribute__((ext_vector_type(2), aligned(4)));

// V = 2 or 4 frames of a row from frame t on; FULL: all of them exist
template <int V, bool FULL>
__device__ __forceinline__ void cr_load(const float *p, int cnt, float *v)
{
    if (FULL && V == 4) {
        const cr_f4 q = *reinterpret_cast<const cr_f4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if (FULL) {
        const cr_f2 q = *reinterpret_cast<const cr_f2 *>(p);
        v[0] = q.x; v[1] = q.y;
    } else {
#pragma unroll
        for (int i = 0; i < V; i++) v[i] = i < cnt ? p[i] : 0.f;
    }
}

template <int V, bool FULL>
__device__ __forceinline__ void cr_store(float *p, int cnt, const float *v)
{
    if (FULL && V == 4) {
        cr_f4 q; q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *reinterpret_cast<cr_f4 *>(p) = q;
    } else if (FULL) {
        cr_f2 q; q.x = v[0]; q.y = v[1];
        *reinterpret_cast<cr_f2 *>(p) = q;
    } else {
#pragma unroll
        for (int i = 0; i < V; i++)
            if (i < cnt) p[i] = v[i];
    }
}

// ---- Batcher's odd-even merge sort on N = 2^k registers, ascending -------------------------------------------------
template <int I, int J>
__device__ __forceinline__ void cr_cx(float *w)
{
    const float a = w[I], b = w[J];
    w[I] = fminf(a, b);
    w[J] = fmaxf(a, b);
}

// Elements LO ... HI (inclusive), stride R (Batcher 1968: merges the two sorted halves of that sequence)
template <int HI, int R, int I>
__device__ __forceinline__ void cr_merge_row(float *w)
{
    if constexpr (I < HI - R) {
        cr_cx<I, I + R>(w);
        cr_merge_row<HI, R, I + 2 * R>(w);
    }
}

template <int LO, int HI, int R>
__device__ __forceinline__ void cr_merge(float *w)
{
    if constexpr (2 * R < HI - LO) {
        cr_merge<LO, HI, 2 * R>(w);
        cr_merge<LO + R, HI, 2 * R>(w);
        cr_merge_row<HI, R, LO + R>(w);
    } else {
        cr_cx<LO, LO + R>(w);
    }
}

template <int LO, int HI>
__device__ __forceinline__ void cr_sort(float *w)
{
    if constexpr (HI > LO) {
        constexpr int MID = LO + (HI - LO) / 2;
        cr_sort<LO, MID>(w);
        cr_sort<MID + 1, HI>(w);
        cr_merge<LO, HI, 1>(w);
    }
}

// frames per lane: four while the tile leaves room for several waves per SIMD, two for 32 and 64 row slots
__host__ __device__ constexpr int cr_v(int np) { return np <= 16 ? 4 : 2; }

// the rows of the copy job (pass-through channels, out of place), bit for bit
template <int V>
__device__ __forceinline__ void cref_copy_rows(const float *x, long long xp, float *y, long long yp, long long t, int cnt,
                                               const CrefTable &tab, int s, int e)
{
    for (int p = s; p < e; p++) {
        const long long c = cr_field(tab.order, p);
        float a[V];
        if (cnt == V) {
            cr_load<V, true>(x + c * xp + t, V, a);
            cr_store<V, true>(y + c * yp + t, V, a);
        } else {
            cr_load<V, false>(x + c * xp + t, cnt, a);
            cr_store<V, false>(y + c * yp + t, cnt, a);
        }
    }
}

template <int MODE, int NP, bool FULL>
__device__ __forceinline__ void cref_reg_body(const float *x, long long xp, float *y, long long yp,
                                              long long t, int cnt, const CrefTable &tab, int s, int e, int n)
{
    constexpr int V = cr_v(NP);
    // every slot loads, the slots beyond the n reference rows the last of them again (a hit in the cache): a load under
    // a branch of its own ends its basic block with s_waitcnt vmcnt(0), one HBM latency per row
    float v[NP][V];
#pragma unroll
    for (int k = 0; k < NP; k++)
        cr_load<V, FULL>(x + (long long)cr_field(tab.order, s + (k < n ? k : n - 1)) * xp + t, cnt, v[k]);
    double ref[V];
    if (MODE == HIPDSP_CREF_MEAN) {
        double sum[V];
#pragma unroll
        for (int q = 0; q < V; q++) sum[q] = 0.0;
#pragma unroll
        for (int k = 0; k < NP; k++) {
            if (k < n) {
#pragma unroll
                for (int q = 0; q < V; q++) sum[q] += (double)v[k][q];
            }
        }
        const double dn = (double)n;
#pragma unroll
        for (int q = 0; q < V; q++) ref[q] = sum[q] / dn;
    } else {
        const int n_low = (NP - n) >> 1;             // slots n ... n + n_low - 1 hold -inf, the rest +inf
        const bool odd = n & 1;
#pragma unroll
        for (int q = 0; q < V; q++) {
            float w[NP];
            bool bad = false;
#pragma unroll
            for (int k = 0; k < NP; k++) {
                w[k] = k < n ? v[k][q] : (k - n < n_low ? -INFINITY : INFINITY);
                bad = bad || w[k] != w[k];
            }
            cr_sort<0, NP - 1>(w);
            const double a = (double)w[NP / 2 - 1], b = (double)w[NP / 2];
            const double m = odd ? a : (a + b) * 0.5;
            ref[q] = bad ? (double)__builtin_nanf("") : m;
        }
    }
#pragma unroll
    for (int k = 0; k < NP; k++) {
        if (k < n) {
            float o[V];
#pragma unroll
            for (int q = 0; q < V; q++) o[q] = (float)((double)v[k][q] - ref[q]);
            cr_store<V, FULL>(y + (long long)cr_field(tab.order, s + k) * yp + t, cnt, o);
        }
    }
    // members that do not contribute
    for (int p = s + n; p < e; p++) {
        const long long c = cr_field(tab.order, p);
        float a[V], o[V];
        cr_load<V, FULL>(x + c * xp + t, cnt, a);
#pragma unroll
        for (int q = 0; q < V; q++) o[q] = (float)((double)a[q] - ref[q]);
        cr_store<V, FULL>(y + c * yp + t, cnt, o);
    }
}

template <int MODE, int NP>
__global__ __launch_bounds__(256) void cref_reg_kernel(const float *x, long long xp, float *y,      // (x may be y: no __restrict__)
                                                       long long yp, long long frames, CrefTable tab)
{
    constexpr int V = cr_v(NP), TILE = 256 * V;
    const int job = blockIdx.y;
    const int s = cr_field(tab.starts, job);
    const int e = job + 1 < tab.njobs ? cr_field(tab.starts, job + 1) : tab.total;
    const bool copy = job == tab.copy_job;
    const int n = copy ? 0 : cr_refs(tab, s, e);
    const long long t0 = (long long)blockIdx.x * TILE;
    const long long t = t0 + V * (long long)threadIdx.x;
    if (copy) {
        if (t < frames) cref_copy_rows<V>(x, xp, y, yp, t, frames - t < V ? (int)(frames - t) : V, tab, s, e);
    } else if (t0 + TILE <= frames) {
        cref_reg_body<MODE, NP, true>(x, xp, y, yp, t, V, tab, s, e, n);
    } else if (t < frames) {
        const int cnt = frames - t < V ? (int)(frames - t) : V;
        cref_reg_body<MODE, NP, false>(x, xp, y, yp, t, cnt, tab, s, e, n);
    }
}

// ---- means over more than 64 reference channels: the tile in LDS ---------------------------------------------------
constexpr int CR_LT = 32;                            // frames per workgroup

__global__ __launch_bounds__(256) void cref_lds_kernel(const float *x, long long xp, float *y,
                                                       long long yp, long long frames, CrefTable tab)
{
    __shared__ float tile[CR_MAXCH * CR_LT];
    __shared__ double ref[CR_LT];
    const int job = blockIdx.y;
    const int s = cr_field(tab.starts, job);
    const int e = job + 1 < tab.njobs ? cr_field(tab.starts, job + 1) : tab.total;
    const int n = cr_refs(tab, s, e);
    const bool copy = job == tab.copy_job;
    const int r = threadIdx.x >> 3, f = 4 * (threadIdx.x & 7);       // 32 rows x 8 quads per pass
    const long long t = (long long)blockIdx.x * CR_LT + f;
    const int cnt = t >= frames ? 0 : (frames - t < 4 ? (int)(frames - t) : 4);
#pragma unroll 4
    for (int k = r; k < n; k += 32) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        const float *p = x + (long long)cr_field(tab.order, s + k) * xp + t;
        if (cnt == 4) cr_load<4, true>(p, 4, a);
        else if (cnt > 0) cr_load<4, false>(p, cnt, a);
#pragma unroll
        for (int q = 0; q < 4; q++) tile[k * CR_LT + f + q] = a[q];
    }
    __syncthreads();
    if (threadIdx.x < CR_LT) {
        double sum = 0.0;
        for (int k = 0; k < n; k++) sum += (double)tile[k * CR_LT + threadIdx.x];
        ref[threadIdx.x] = sum / (double)n;
    }
    __syncthreads();
    if (cnt == 0) return;
    for (int k = r; k < e - s; k += 32) {
        const long long c = cr_field(tab.order, s + k);
        float a[4], o[4];
        if (k < n) {
#pragma unroll
            for (int q = 0; q < 4; q++) a[q] = tile[k * CR_LT + f + q];
        } else if (cnt == 4) {
            cr_load<4, true>(x + c * xp + t, 4, a);
        } else {
            cr_load<4, false>(x + c * xp + t, cnt, a);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = copy ? a[q] : (float)((double)a[q] - ref[f + q]);
        if (cnt == 4) cr_store<4, true>(y + c * yp + t, 4, o);
        else cr_store<4, false>(y + c * yp + t, cnt, o);
    }
}

inline void cr_put(unsigned int *w, int i, int v) { w[i / 3] |= (unsigned int)v << (10 * (i % 3)); }

}  // namespace

extern "C" int hipdsp_common_reference(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, float *y, int64_t y_pitch,
                                       int64_t channels, int64_t frames, const int *host_group,
                                       const unsigned char *host_use, int mode)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(channels >= 0 && frames >= 0, "negative size");
    HD_REQUIRE(mode == HIPDSP_CREF_MEAN || mode == HIPDSP_CREF_MEDIAN, "unknown mode %d", mode);
    if (channels > CR_MAXCH) {
        hipdsp_set_error("%lld channels: the group table holds up to %d", (long long)channels, CR_MAXCH);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    HD_REQUIRE(channels == 0 || host_group != nullptr, "NULL group table");
    if (x_pitch == 0) x_pitch = frames;
    if (y_pitch == 0) y_pitch = frames;
    HD_REQUIRE(x_pitch >= frames && y_pitch >= frames, "pitch smaller than row length");
    const int C = (int)channels;
    static thread_local int members[CR_MAXCH], refs[CR_MAXCH];       // per group id
    for (int g = 0; g < C; g++) members[g] = refs[g] = 0;
    int passing = 0, max_refs = 0;
    for (int c = 0; c < C; c++) {
        const int g = host_group[c];
        HD_REQUIRE(g >= -1 && g < C, "channel %d: group %d outside [-1, %d)", c, g, C);
        if (g < 0) { passing++; continue; }
        members[g]++;
        if (host_use == nullptr || host_use[c]) refs[g]++;
    }
    for (int g = 0; g < C; g++) {
        HD_REQUIRE(members[g] == 0 || refs[g] > 0, "group %d has %d members and no reference channel", g, members[g]);
        if (refs[g] > max_refs) max_refs = refs[g];
    }
    if (mode == HIPDSP_CREF_MEDIAN && max_refs > 64) {
        hipdsp_set_error("median over %d reference channels: up to 64 per group", max_refs);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    if (C == 0 || frames == 0) return HIPDSP_OK;
    HD_REQUIRE(x != nullptr && y != nullptr, "NULL data pointer");
    const bool in_place = (const float *)y == x && y_pitch == x_pitch;
    HD_REQUIRE(in_place || !hd_planar_overlap(x, x_pitch, frames, y, y_pitch, frames, channels),
               "x and y overlap other than y == x with equal pitches");

    // jobs: the groups in ascending id (reference channels first), then the pass-through rows when they need a copy
    CrefTable tab;
    memset(&tab, 0, sizeof(tab));
    int pos = 0, job = 0;
    for (int g = 0; g < C; g++) {
        if (members[g] == 0) continue;
        cr_put(tab.starts, job++, pos);
        for (int pass = 0; pass < 2; pass++)
            for (int c = 0; c < C; c++) {
                if (host_group[c] != g) continue;
                const bool used = host_use == nullptr || host_use[c];
                if (used != (pass == 0)) continue;
                if (used) tab.use[pos >> 5] |= 1u << (pos & 31);
                cr_put(tab.order, pos++, c);
            }
    }
    tab.copy_job = -1;
    if (passing > 0 && !in_place) {
        tab.copy_job = job;
        cr_put(tab.starts, job++, pos);
        for (int c = 0; c < C; c++)
            if (host_group[c] < 0) cr_put(tab.order, pos++, c);
    }
    tab.total = pos;
    tab.njobs = job;
    if (job == 0) return HIPDSP_OK;
    HD_CHECK_HIP(hipSetDevice(ctx->device));

    if (max_refs > 64) {
        const long long tiles = (frames + CR_LT - 1) / CR_LT;
        HD_REQUIRE(tiles <= 0x7fffffffLL, "grid too large");
        hipLaunchKernelGGL(cref_lds_kernel, dim3((unsigned)tiles, (unsigned)job), dim3(256), 0, ctx->stream, x,
                           (long long)x_pitch, y, (long long)y_pitch, (long long)frames, tab);
        return hd_launch_status("cref_lds_kernel");
    }
    const int tile = 256 * cr_v(max_refs);
    const long long tiles = (frames + tile - 1) / tile;
    HD_REQUIRE(tiles <= 0x7fffffffLL, "grid too large");
    const dim3 grid((unsigned)tiles, (unsigned)job);
#define HD_CREF(MODEV, NPV)                                                                                       \
    hipLaunchKernelGGL((cref_reg_kernel<MODEV, NPV>), grid, dim3(256), 0, ctx->stream, x, (long long)x_pitch, y, \
                       (long long)y_pitch, (long long)frames, tab)
    if (mode == HIPDSP_CREF_MEAN) {
        if (max_refs <= 8) HD_CREF(HIPDSP_CREF_MEAN, 8); else if (max_refs <= 16) HD_CREF(HIPDSP_CREF_MEAN, 16);
        else if (max_refs <= 32) HD_CREF(HIPDSP_CREF_MEAN, 32); else HD_CREF(HIPDSP_CREF_MEAN, 64);
    } else {
        if (max_refs <= 8) HD_CREF(HIPDSP_CREF_MEDIAN, 8); else if (max_refs <= 16) HD_CREF(HIPDSP_CREF_MEDIAN, 16);
        else if (max_refs <= 32) HD_CREF(HIPDSP_CREF_MEDIAN, 32); else HD_CREF(HIPDSP_CREF_MEDIAN, 64);
    }
#undef HD_CREF
    return hd_launch_status("cref_reg_kernel");
}
