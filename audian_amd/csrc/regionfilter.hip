// hipdsp_region_filtfilt and hipdsp_region_crossings: the two device steps of the reference's event refinement
// (filter_envelopes, songdetector.py:178-192, and analyse_songs, :195-244; the contracts are in include/hip_dsp.h).
// Both take a host table of (channel, start, stop) regions like hipdsp_region_spectra (hd_check_table, hd_upload_table
// and hd_owner of rowpass.h), size a flat work list exactly from it and compute a region from nothing but its own
// samples and parameters.
//
// hipdsp_region_filtfilt -- scipy.signal.sosfiltfilt of every region with the region's OWN one- or two-section filter.
// A region of L samples is extended oddly by padlen on both sides to E = L + 2 padlen samples; that sequence is cut into
// chunks of RF_CHUNK = 64 samples counted from ITS first sample (the backward pass: from its last), and 64 consecutive
// chunks make a tile, the work item of one wave.  Per direction three launches:
//
//   rf_pass<.., false>   a wave stages its tile in LDS with coalesced loads (64 rows of 64 float64, 65 apart); lane l then
//                        runs the cascade over row l from ZERO state to the end state z_l of its chunk, and a six-step scan
//                        over the lanes with A^64, A^128 ... A^2048 turns the z_l into v_l = sum_(m <= l) A^(64 (l - m)) z_m,
//                        what the tile adds to the state behind chunk l; the v_l are stored.  The forward pass forms the
//                        extension here, in float64 from the exactly converted samples, and a tile that holds a NaN or an
//                        infinity stores NaN.
//   rf_carry             one thread per region over its TILES: s_0 = zi * (first sample), s_(t+1) = A^4096 s_t + v_63(t), in
//                        float64 -- the exact hand-over of a linear recurrence.  The powers of A come from the host
//                        (squared in long double, each rounded once to float64).  A ragged last tile hands nothing on.
//   rf_pass<.., true>    the same tiles again, lane l from its true state A^(64 l) s_t + v_(l-1) (the power applied by
//                        the bits of l); the row is overwritten in LDS and stored coalesced: the forward pass as float64
//                        into the scratch (8 bytes per sample of the extended region: the backward pass reads float64),
//                        the backward pass as float32 into y, the extension trimmed, negative values clamped on request,
//                        NaN throughout for a marked region.
//
// x is read by the forward launches only and y written by the last launch only, so y == x is safe.  No atomics.
//
// hipdsp_region_crossings -- per region and threshold: how many samples are above, the first and last of them, the
// largest sample and its position.  rc_chunk: one 256-thread workgroup per chunk of RC_CHUNK = 4096 samples counted from
// the region's start reduces (count, first, last, max, argmax) in a fixed order; rc_finish: one thread per region merges
// the chunks in ascending order.  Integers and comparisons only: exact.
#include "rowpass.h"
#include <vector>
#include <algorithm>

namespace {

constexpr int RF_CHUNK = 64;                            // samples per lane and hand-over
constexpr int RF_TILE = 64 * RF_CHUNK;                  // samples per wave
constexpr int RF_ROW = RF_CHUNK + 1;                    // LDS row stride in float64
constexpr int RC_CHUNK = 4096;
constexpr int RC_THREADS = 256;

struct RfRegion {                                       // one row of the uploaded table
    long long channel, start, len, pad;
    long long ebase;                                    // first element of the region's forward pass in the scratch
    long long cbase;                                    // first chunk
    long long tbase;                                    // first tile; row n_regions: all tiles
    long long pad_;
    double c[2][5];                                     // b0 b1 b2 a1 a2
    double zi[4];
    double P[7][16];                                    // A^(64 * 2^b), b = 0 ... 6, row-major (2 S) x (2 S); P[6] = A^4096
};

static_assert(sizeof(RfRegion) == 1072, "the scratch formula in include/hip_dsp.h counts 1072 bytes per table row");

template <int S>
__device__ __forceinline__ double rf_step(const double (&c)[2][5], double (&z)[2 * S], double v)
{
#pragma unroll
    for (int s = 0; s < S; s++) {
        const double o = c[s][0] * v + z[2 * s];
        z[2 * s] = (c[s][1] * v - c[s][3] * o) + z[2 * s + 1];
        z[2 * s + 1] = c[s][2] * v - c[s][4] * o;
        v = o;
    }
    return v;
}

// a = M s for a row-major (2 S) x (2 S) matrix
template <int S>
__device__ __forceinline__ void rf_matvec(const double *__restrict__ M, const double (&s)[2 * S], double (&a)[2 * S])
{
#pragma unroll
    for (int i = 0; i < 2 * S; i++) {
        double t = M[i * (2 * S)] * s[0];
#pragma unroll
        for (int j = 1; j < 2 * S; j++) t += M[i * (2 * S) + j] * s[j];
        a[i] = t;
    }
}

// sample i of the region's extended sequence, float64 from the exactly converted float32 samples
__device__ __forceinline__ double rf_ext(const float *__restrict__ v, long long i, long long pad, long long len)
{
    if (i < pad) return 2.0 * (double)v[0] - (double)v[pad - i];
    if (i < pad + len) return (double)v[i - pad];
    return 2.0 * (double)v[len - 1] - (double)v[2 * len + pad - 2 - i];
}

// BWD: position j of the reversed forward pass, j = E - 1 - i.  WRITE: from the true states, storing the result.
template <int S, bool BWD, bool WRITE>
__global__ __launch_bounds__(64) void rf_pass(const float *__restrict__ x, long long x_pitch, float *__restrict__ y,
                                              long long y_pitch, const RfRegion *__restrict__ tab, int n_regions,
                                              double *__restrict__ fwd, double *__restrict__ states,
                                              const double *__restrict__ tstate, const int *__restrict__ bad, int clamp)
{
    __shared__ double tile[64 * RF_ROW];
    const int lane = threadIdx.x;
    const long long g = blockIdx.x;
    const int r = hd_owner(tab, &RfRegion::tbase, n_regions, g);
    const RfRegion &reg = tab[r];
    const long long len = reg.len, pad = reg.pad, E = len + 2 * pad;
    const long long t0 = (g - reg.tbase) * RF_TILE;     // first position of the tile
    const long long left = E - t0;
    const int nt = left < RF_TILE ? (int)left : RF_TILE;
    const float *v = x + reg.channel * x_pitch + reg.start;
    double *f = fwd + reg.ebase;

    // branch-free and unrolled, so that a batch of loads is in flight at once; positions behind the tile's end repeat its
    // last sample (their rows are never run)
    bool nonfinite = false;
    const double v_first = BWD ? 0.0 : (double)v[0], v_last = BWD ? 0.0 : (double)v[len - 1];
#pragma unroll 16
    for (int k = 0; k < 64; k++) {
        long long i = t0 + k * 64 + lane;
        if (i > E - 1) i = E - 1;
        double w;
        if (BWD) w = f[E - 1 - i];
        else {
            const bool left = i < pad, right = i >= pad + len;
            const long long idx = left ? pad - i : (right ? 2 * len + pad - 2 - i : i - pad);
            const double u = (double)v[idx];
            w = left ? 2.0 * v_first - u : (right ? 2.0 * v_last - u : u);
            nonfinite = nonfinite || !(fabs(w) <= 1.7976931348623157e308);
        }
        tile[k * RF_ROW + lane] = w;
    }
    __syncthreads();
    if (!BWD && !WRITE) {                               // rows are chunks: the lane that ran over the sample's chunk marks it
        const unsigned long long any = __ballot(nonfinite);
        nonfinite = any != 0;                           // (a tile with one bad sample marks all its chunks: the region is bad)
    }

    const int n = nt - lane * RF_CHUNK < 0 ? 0 : (nt - lane * RF_CHUNK < RF_CHUNK ? nt - lane * RF_CHUNK : RF_CHUNK);
    const long long chunk = reg.cbase + (g - reg.tbase) * 64 + lane;
    double c[2][5];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int j = 0; j < 5; j++) c[s][j] = reg.c[s][j];
    double z[2 * S];
#pragma unroll
    for (int j = 0; j < 2 * S; j++) z[j] = 0.0;
    if (WRITE && n > 0) {                               // A^(64 lane) (the tile's start state) + what the lanes in front add
#pragma unroll
        for (int j = 0; j < 2 * S; j++) z[j] = tstate[g * (2 * S) + j];
#pragma unroll
        for (int b = 0; b < 6; b++) {
            if ((lane >> b) & 1) {
                double a[2 * S];
                rf_matvec<S>(reg.P[b], z, a);
#pragma unroll
                for (int j = 0; j < 2 * S; j++) z[j] = a[j];
            }
        }
        if (lane > 0) {
#pragma unroll
            for (int j = 0; j < 2 * S; j++) z[j] += states[(chunk - 1) * (2 * S) + j];
        }
    }
    double *row = tile + lane * RF_ROW;
    if (n == RF_CHUNK) {
#pragma unroll 8
        for (int i = 0; i < RF_CHUNK; i++) {
            const double o = rf_step<S>(c, z, row[i]);
            if (WRITE) row[i] = o;
        }
    } else {
        for (int i = 0; i < n; i++) {
            const double o = rf_step<S>(c, z, row[i]);
            if (WRITE) row[i] = o;
        }
    }
    if (!WRITE) {
        // v_l = sum over the lanes m <= l of A^(64 (l - m)) z_m: what the tile adds to the state behind chunk l
        if (nonfinite) {
#pragma unroll
            for (int j = 0; j < 2 * S; j++) z[j] = __longlong_as_double(0x7ff8000000000000LL);
        }
#pragma unroll
        for (int b = 0; b < 6; b++) {
            double o[2 * S], a[2 * S];
#pragma unroll
            for (int j = 0; j < 2 * S; j++) o[j] = __shfl_up(z[j], 1 << b, 64);
            rf_matvec<S>(reg.P[b], o, a);
            if (lane >= (1 << b)) {
#pragma unroll
                for (int j = 0; j < 2 * S; j++) z[j] += a[j];
            }
        }
        if (n > 0) {
#pragma unroll
            for (int j = 0; j < 2 * S; j++) states[chunk * (2 * S) + j] = z[j];
        }
        return;
    }
    __syncthreads();
    if (!BWD) {
        for (int k = 0; k < 64; k++) {
            const int p = k * 64 + lane;
            if (p < nt) f[t0 + p] = tile[k * RF_ROW + lane];
        }
    } else {
        float *o = y + reg.channel * y_pitch + reg.start;
        const bool isbad = bad[r] != 0;
        for (int k = 0; k < 64; k++) {
            const int p = k * 64 + lane;
            const long long i = E - 1 - (t0 + p) - pad;         // position in the region
            if (p < nt && i >= 0 && i < len) {
                float w = (float)tile[k * RF_ROW + lane];
                if (clamp && w < 0.0f) w = 0.0f;
                o[i] = isbad ? __uint_as_float(0x7fc00000u) : w;
            }
        }
    }
}

// one thread per region: the start state of every tile, s_0 = zi * (first sample), s_(t+1) = A^4096 s_t + v_63(t)
template <int S, bool BWD>
__global__ __launch_bounds__(64) void rf_carry(const float *__restrict__ x, long long x_pitch,
                                               const RfRegion *__restrict__ tab, int n_regions,
                                               const double *__restrict__ fwd, const double *__restrict__ states,
                                               double *__restrict__ tstate, int *__restrict__ bad)
{
    const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
    if (r >= n_regions) return;
    const RfRegion &reg = tab[r];
    const long long E = reg.len + 2 * reg.pad;
    const long long nc = (E + RF_CHUNK - 1) / RF_CHUNK, ntiles = (E + RF_TILE - 1) / RF_TILE;
    double first;
    if (BWD) first = fwd[reg.ebase + E - 1];
    else first = rf_ext(x + reg.channel * x_pitch + reg.start, 0, reg.pad, reg.len);
    double s[2 * S], P[4 * S * S];
#pragma unroll
    for (int i = 0; i < 2 * S; i++) s[i] = reg.zi[i] * first;
#pragma unroll
    for (int i = 0; i < 4 * S * S; i++) P[i] = reg.P[6][i];
    const double *st = states + reg.cbase * (2 * S);
    double *ts = tstate + reg.tbase * (2 * S);
    bool nonfinite = false;
    for (long long t = 0; t < ntiles; t++) {
        const long long last = t * 64 + 63 < nc ? t * 64 + 63 : nc - 1;     // (a ragged tile hands nothing on: its flag only)
        double v[2 * S], nx[2 * S];
#pragma unroll
        for (int i = 0; i < 2 * S; i++) v[i] = st[last * (2 * S) + i];
        nonfinite = nonfinite || v[0] != v[0];
        rf_matvec<S>(P, s, nx);
#pragma unroll
        for (int i = 0; i < 2 * S; i++) {
            ts[t * (2 * S) + i] = s[i];
            s[i] = nx[i] + v[i];
        }
    }
    if (!BWD) bad[r] = nonfinite ? 1 : 0;
}

template <int S>
int rf_launch(hipdsp_ctx *ctx, const float *x, long long x_pitch, float *y, long long y_pitch, const RfRegion *dtab,
              int n_regions, long long tiles, double *fwd, double *states, double *tstate, int *bad, int clamp)
{
    const dim3 gt((unsigned)tiles), gr((unsigned)((n_regions + 63) / 64)), b(64);
    int rc;
    hipLaunchKernelGGL((rf_pass<S, false, false>), gt, b, 0, ctx->stream, x, x_pitch, y, y_pitch, dtab, n_regions, fwd, states,
                       (const double *)tstate, (const int *)bad, clamp);
    if ((rc = hd_launch_status("rf_pass (forward, end states)")) != HIPDSP_OK) return rc;
    hipLaunchKernelGGL((rf_carry<S, false>), gr, b, 0, ctx->stream, x, x_pitch, dtab, n_regions, (const double *)fwd,
                       (const double *)states, tstate, bad);
    if ((rc = hd_launch_status("rf_carry (forward)")) != HIPDSP_OK) return rc;
    hipLaunchKernelGGL((rf_pass<S, false, true>), gt, b, 0, ctx->stream, x, x_pitch, y, y_pitch, dtab, n_regions, fwd, states,
                       (const double *)tstate, (const int *)bad, clamp);
    if ((rc = hd_launch_status("rf_pass (forward)")) != HIPDSP_OK) return rc;
    hipLaunchKernelGGL((rf_pass<S, true, false>), gt, b, 0, ctx->stream, x, x_pitch, y, y_pitch, dtab, n_regions, fwd, states,
                       (const double *)tstate, (const int *)bad, clamp);
    if ((rc = hd_launch_status("rf_pass (backward, end states)")) != HIPDSP_OK) return rc;
    hipLaunchKernelGGL((rf_carry<S, true>), gr, b, 0, ctx->stream, x, x_pitch, dtab, n_regions, (const double *)fwd,
                       (const double *)states, tstate, bad);
    if ((rc = hd_launch_status("rf_carry (backward)")) != HIPDSP_OK) return rc;
    hipLaunchKernelGGL((rf_pass<S, true, true>), gt, b, 0, ctx->stream, x, x_pitch, y, y_pitch, dtab, n_regions, fwd, states,
                       (const double *)tstate, (const int *)bad, clamp);
    return hd_launch_status("rf_pass (backward)");
}

// A^(64 * 2^b), b = 0 ... 6, of the cascade's state transition (input zero), n = 2 S states: squared in long double, every
// power rounded once
void transition_powers(const double c[2][5], int S, double P[7][16])
{
    const int n = 2 * S;
    long double A[4][4] = {}, T[4][4];
    for (int j = 0; j < n; j++) {                       // column j: one step from the unit state e_j
        long double z[4] = {};
        z[j] = 1.0L;
        long double v = 0.0L;
        for (int s = 0; s < S; s++) {
            const long double o = (long double)c[s][0] * v + z[2 * s];
            z[2 * s] = ((long double)c[s][1] * v - (long double)c[s][3] * o) + z[2 * s + 1];
            z[2 * s + 1] = (long double)c[s][2] * v - (long double)c[s][4] * o;
            v = o;
        }
        for (int i = 0; i < n; i++) A[i][j] = z[i];
    }
    for (int sq = 1; sq <= 12; sq++) {                  // A^(2^sq); 2^6 = RF_CHUNK, 2^12 = RF_TILE
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                long double a = 0.0L;
                for (int k = 0; k < n; k++) a += A[i][k] * A[k][j];
                T[i][j] = a;
            }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) A[i][j] = T[i][j];
        if (sq >= 6)
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++) P[sq - 6][i * n + j] = (double)A[i][j];
    }
}
static_assert(RF_CHUNK == 64 && RF_TILE == 4096, "transition_powers stores the squarings 6 ... 12");

}  // namespace

extern "C" int hipdsp_region_filtfilt(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, float *y, int64_t y_pitch,
                                      int64_t channels, int64_t frames, const int64_t *host_regions, int64_t n_regions,
                                      const double *host_sos, int n_sections, int clamp)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    if (n_sections < 1 || n_sections > 2) {
        hipdsp_set_error("hipdsp_region_filtfilt: %d sections per region, 1 or 2 are served", n_sections);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    if (y_pitch == 0) y_pitch = frames;
    HD_TRY(hd_check_table("hipdsp_region_filtfilt", ctx, x, x_pitch, channels, frames, host_regions, n_regions,
                          (1LL << 31) / 64));
    HD_REQUIRE(y_pitch >= frames, "y_pitch smaller than frames");
    if (n_regions == 0) return HIPDSP_OK;
    HD_REQUIRE(x != nullptr, "NULL data pointer");
    HD_REQUIRE(y != nullptr && host_sos != nullptr, "NULL output or filter table");
    HD_REQUIRE(((uintptr_t)y & 3) == 0, "misaligned pointer");
    if (!((const float *)y == x && y_pitch == x_pitch))
        HD_NO_OVERLAP(x, x_pitch, frames, y, y_pitch, frames, channels, "x and y (other than y == x with equal pitches)");

    const int S = n_sections;
    std::vector<RfRegion> tab((size_t)n_regions + 1);
    long long samples = 0, chunks = 0, tiles = 0;
    bool too_short = false;
    long long short_r = 0, short_pad = 0;
    for (int64_t r = 0; r < n_regions; r++) {
        RfRegion &t = tab[r];
        memset(&t, 0, sizeof(t));
        const double *sos = host_sos + (size_t)r * S * 6;
        int zb = 0, za = 0;
        for (int s = 0; s < S; s++) {
            const double *q = sos + 6 * s;
            for (int j = 0; j < 6; j++)
                HD_REQUIRE(fabs(q[j]) <= 1.7976931348623157e308, "region %lld: a coefficient of section %d is not finite",
                           (long long)r, s);
            HD_REQUIRE(q[3] == 1.0, "region %lld: a0 of section %d is not 1", (long long)r, s);
            HD_REQUIRE(fabs(q[5]) < 1.0 && fabs(q[4]) < 1.0 + q[5], "region %lld: section %d has a pole on or outside the unit circle",
                       (long long)r, s);
            t.c[s][0] = q[0], t.c[s][1] = q[1], t.c[s][2] = q[2], t.c[s][3] = q[4], t.c[s][4] = q[5];
            zb += q[2] == 0.0;
            za += q[5] == 0.0;
        }
        const long long pad = 3 * (2 * S + 1 - std::min(zb, za));       // scipy's default padlen
        t.channel = host_regions[3 * r], t.start = host_regions[3 * r + 1];
        t.len = host_regions[3 * r + 2] - t.start, t.pad = pad;
        if (t.len <= pad && !too_short) too_short = true, short_r = r, short_pad = pad;
        // scipy.signal.sosfilt_zi: (I - A) zi = B per section, scaled by the DC gain of the sections in front
        double scale = 1.0;
        for (int s = 0; s < S; s++) {
            const double b0 = t.c[s][0], b1 = t.c[s][1], b2 = t.c[s][2], a1 = t.c[s][3], a2 = t.c[s][4];
            const double B0 = b1 - a1 * b0, B1 = b2 - a2 * b0, det = (1.0 + a1) + a2;
            t.zi[2 * s] = scale * (B0 + B1) / det;
            t.zi[2 * s + 1] = scale * ((1.0 + a1) * B1 - a2 * B0) / det;
            scale = scale * (b0 + b1 + b2) / (1.0 + a1 + a2);
        }
        transition_powers(t.c, S, t.P);
        const long long E = t.len + 2 * pad;
        t.ebase = samples, t.cbase = chunks, t.tbase = tiles;
        samples += E;
        chunks += (E + RF_CHUNK - 1) / RF_CHUNK;
        tiles += (E + RF_TILE - 1) / RF_TILE;
    }
    memset(&tab[n_regions], 0, sizeof(RfRegion));
    tab[n_regions].tbase = tiles;
    {   // two writers: regions of one channel must not overlap (stop == next start is fine)
        std::vector<int64_t> order((size_t)n_regions);
        for (int64_t r = 0; r < n_regions; r++) order[r] = r;
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
            if (tab[a].channel != tab[b].channel) return tab[a].channel < tab[b].channel;
            if (tab[a].start != tab[b].start) return tab[a].start < tab[b].start;
            return tab[a].len < tab[b].len;
        });
        for (int64_t i = 1; i < n_regions; i++) {
            const RfRegion &p = tab[order[i - 1]], &q = tab[order[i]];
            HD_REQUIRE(p.channel != q.channel || p.start + p.len <= q.start,
                       "regions %lld and %lld of channel %lld overlap", (long long)order[i - 1], (long long)order[i],
                       (long long)q.channel);
        }
    }
    if (too_short) {
        hipdsp_set_error("region %lld: the length of the input vector x must be greater than padlen, which is %lld",
                         short_r, short_pad);
        return HIPDSP_ERR_TOO_SHORT;
    }
    HD_REQUIRE(tiles <= 0x7fffffffLL, "too many samples for one call");

    HD_CHECK_HIP(hipSetDevice(ctx->device));
    const size_t tab_bytes = sizeof(RfRegion) * tab.size();
    const size_t fwd_bytes = sizeof(double) * (size_t)samples, st_bytes = sizeof(double) * 2 * S * (size_t)chunks;
    const size_t ts_bytes = sizeof(double) * 2 * S * (size_t)tiles;
    void *work = nullptr;
    HD_TRY(hipdsp_scratch(ctx, tab_bytes + fwd_bytes + st_bytes + ts_bytes + 8 * (size_t)n_regions, &work));
    const RfRegion *dtab = (const RfRegion *)work;
    double *fwd = (double *)((char *)work + tab_bytes);
    double *states = (double *)((char *)work + tab_bytes + fwd_bytes);
    double *tstate = (double *)((char *)work + tab_bytes + fwd_bytes + st_bytes);
    int *bad = (int *)((char *)work + tab_bytes + fwd_bytes + st_bytes + ts_bytes);
    HD_TRY(hd_upload_table(ctx, work, tab.data(), tab_bytes));
    if (S == 1)
        return rf_launch<1>(ctx, x, x_pitch, y, y_pitch, dtab, (int)n_regions, tiles, fwd, states, tstate, bad, clamp != 0);
    return rf_launch<2>(ctx, x, x_pitch, y, y_pitch, dtab, (int)n_regions, tiles, fwd, states, tstate, bad, clamp != 0);
}

// ---- hipdsp_region_crossings --------------------------------------------------------------------------------------------

namespace {

struct RcRegion {                                       // row n_regions: ibase = all chunks
    long long channel, start, len, ibase;
    float thr;
    int pad_;
};

struct RcPart {                                         // positions relative to the chunk's first sample; -1 = none
    int count, first, last, arg;
    float mx;
    int pad_;
};

// (value, position) as np.argmax orders them: a NaN beats every number, equal values keep the earlier position
__device__ __forceinline__ void rc_higher(float &v, int &i, float ov, int oi)
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

__device__ __forceinline__ void rc_merge(RcPart &a, const RcPart &b)      // b lies behind a or beside it
{
    a.count += b.count;
    if (b.first >= 0 && (a.first < 0 || b.first < a.first)) a.first = b.first;
    if (b.last > a.last) a.last = b.last;
    rc_higher(a.mx, a.arg, b.mx, b.arg);
}

__global__ __launch_bounds__(RC_THREADS) void rc_chunk(const float *__restrict__ x, long long pitch,
                                                       const RcRegion *__restrict__ tab, int n_regions,
                                                       RcPart *__restrict__ part)
{
    __shared__ RcPart sh[RC_THREADS / 64];
    const int t = threadIdx.x;
    const long long g = blockIdx.x;
    const RcRegion reg = tab[hd_owner(tab, &RcRegion::ibase, n_regions, g)];
    const long long c0 = (g - reg.ibase) * RC_CHUNK;
    const long long left = reg.len - c0;
    const int n = left < RC_CHUNK ? (int)left : RC_CHUNK;
    const float *v = x + reg.channel * pitch + reg.start + c0;
    RcPart p{0, -1, -1, -1, 0.0f, 0};
    for (int i = t; i < n; i += RC_THREADS) {           // ascending positions
        const float s = v[i];
        if (s > reg.thr) {
            p.count++;
            if (p.first < 0) p.first = i;
            p.last = i;
        }
        rc_higher(p.mx, p.arg, s, i);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        RcPart o;
        o.count = __shfl_down(p.count, d, 64);
        o.first = __shfl_down(p.first, d, 64);
        o.last = __shfl_down(p.last, d, 64);
        o.arg = __shfl_down(p.arg, d, 64);
        o.mx = __shfl_down(p.mx, d, 64);
        if ((t & 63) + d < 64) rc_merge(p, o);
    }
    if ((t & 63) == 0) sh[t >> 6] = p;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < RC_THREADS / 64; w++) rc_merge(p, sh[w]);
        part[g] = p;
    }
}

__global__ __launch_bounds__(64) void rc_finish(const RcRegion *__restrict__ tab, int n_regions,
                                                const RcPart *__restrict__ part, double *__restrict__ out)
{
    const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
    if (r >= n_regions) return;
    const RcRegion reg = tab[r];
    const long long ng = tab[r + 1].ibase - reg.ibase;
    long long count = 0, first = -1, last = -1, arg = -1;
    float mx = 0.0f;
    for (long long k = 0; k < ng; k++) {
        const RcPart p = part[reg.ibase + k];
        const long long base = reg.start + k * RC_CHUNK;
        count += p.count;
        if (p.first >= 0 && first < 0) first = base + p.first;
        if (p.last >= 0) last = base + p.last + 1;
        if (p.arg >= 0) {
            bool take;
            if (arg < 0) take = true;
            else if (p.mx != p.mx) take = !(mx != mx);  // the first NaN stays
            else if (mx != mx) take = false;
            else take = p.mx > mx;                      // an equal value behind does not replace
            if (take) {
                mx = p.mx;
                arg = base + p.arg;
            }
        }
    }
    double *o = out + r * 8;
    o[0] = (double)reg.len;
    o[1] = (double)count;
    o[2] = (double)first;
    o[3] = (double)last;
    o[4] = arg < 0 ? __longlong_as_double(0x7ff8000000000000LL) : (double)mx;
    o[5] = (double)arg;
    o[6] = 0.0;
    o[7] = 0.0;
}

}  // namespace

extern "C" int hipdsp_region_crossings(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t frames,
                                       const int64_t *host_regions, const double *host_thresholds, int64_t n_regions,
                                       double *out)
{
    HD_TRY(hd_check_table("hipdsp_region_crossings", ctx, x, x_pitch, channels, frames, host_regions, n_regions,
                          (1LL << 31) / 64));
    if (n_regions == 0) return HIPDSP_OK;
    HD_REQUIRE(x != nullptr, "NULL data pointer");
    HD_REQUIRE(host_thresholds != nullptr && out != nullptr, "NULL thresholds or output");
    HD_REQUIRE(((uintptr_t)out & 7) == 0, "misaligned pointer");
    std::vector<RcRegion> tab((size_t)n_regions + 1);
    long long items = 0;
    for (int64_t r = 0; r < n_regions; r++) {
        const long long len = host_regions[3 * r + 2] - host_regions[3 * r + 1];
        tab[r] = RcRegion{host_regions[3 * r], host_regions[3 * r + 1], len, items, (float)host_thresholds[r], 0};
        items += (len + RC_CHUNK - 1) / RC_CHUNK;
    }
    tab[n_regions] = RcRegion{0, 0, 0, items, 0.0f, 0};
    HD_REQUIRE(items <= 0x7fffffffLL, "too many samples for one call");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    const size_t tab_bytes = sizeof(RcRegion) * tab.size();
    void *work = nullptr;
    int rc = hipdsp_scratch(ctx, tab_bytes + sizeof(RcPart) * (size_t)items, &work);
    if (rc != HIPDSP_OK) return rc;
    const RcRegion *dtab = (const RcRegion *)work;
    RcPart *part = (RcPart *)((char *)work + tab_bytes);
    HD_TRY(hd_upload_table(ctx, work, tab.data(), tab_bytes));
    if (items > 0) {
        hipLaunchKernelGGL(rc_chunk, dim3((unsigned)items), dim3(RC_THREADS), 0, ctx->stream, x, (long long)x_pitch, dtab,
                           (int)n_regions, part);
        rc = hd_launch_status("rc_chunk");
        if (rc != HIPDSP_OK) return rc;
    }
    hipLaunchKernelGGL(rc_finish, dim3((unsigned)((n_regions + 63) / 64)), dim3(64), 0, ctx->stream, dtab, (int)n_regions,
                       (const RcPart *)part, out);
    return hd_launch_status("rc_finish");
}
