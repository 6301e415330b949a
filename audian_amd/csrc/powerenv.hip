// hipdsp_power_envelope: the first step of the reference's song detector -- envelope() (songdetector.py:57-69): the squares
// of a trace, a zero-phase low-pass of them (scipy's sosfiltfilt with its default odd extension), every step-th sample kept,
// the clamp at zero and the root.  The contract is in include/hip_dsp.h.
//
// A row of `frames` samples is extended oddly by padlen on both sides to E = frames + 2 padlen samples u_ext (the extension of
// the SQUARES, 2 u[0] - u[i], float64 from the exactly squared float32 samples).  That sequence is cut into chunks of PE_CHUNK
// = 64 samples counted from its first sample; 64 consecutive chunks are a tile, the work item of one wave.  Both passes use
// this one grid: the forward pass walks it upwards, the backward pass downwards, the ragged last tile first.  Three sweeps over
// x with two carries between them, nothing at full rate in memory:
//
//   pe_pass<S, 0>   a wave stages its tile's float32 samples in LDS with coalesced loads; lane l runs the cascade over chunk l
//                   from ZERO state (the chunk that holds sample 0 of the sequence: from zi * u_ext[0]) to its end state z_l,
//                   and a six-step scan over the lanes with A^64 ... A^2048 turns them into v_l = sum_(m <= l) A^(64 (l - m))
//                   z_m, what the tile adds to the state behind chunk l; the v_l are stored.  A tile with a NaN or an infinity
//                   stores NaN.
//   pe_carry<S, 0>  one wave per row over its tiles, 64 at a time: the same scan with A^4096 ... A^(2^17) and the hand-over
//                   s' = A^(2^18) s + v in float64 give every tile's entering state.  The exact recurrence: no warm-up.
//   pe_pass<S, 1>   the tile again: lane l recomputes the forward output of its chunk from its true entering state A^(64 l) s_t
//                   + v_(l-1) (which replaces v_l in the scratch) into 64 float64 REGISTERS and runs the cascade backwards
//                   over them from zero state (the chunk that holds the last sample: from zi * (the forward pass's last
//                   output)); the scan downwards over the lanes gives the backward summaries.
//   pe_carry<S, 1>  the backward hand-over, from the last tile down.
//   pe_pass<S, 2>   the same recomputation, backwards from the true state; gain * max(., 0) in float64, ONE rounding to
//                   float32 into the lane's LDS row; then the wave picks the samples on the grid first + j step out of the
//                   tile, takes the root and stores them coalesced in y.
//
// The powers of A come from the host (squared in long double, each rounded once).  All state, every hand-over and the forward
// output that feeds the backward pass are float64.  No atomics; a row's bytes depend on the row, the plan and (first, step,
// n_out, gain, root) alone.  Scratch: 32 S bytes per chunk and per tile, one flag per row.
#include "rowpass.h"
#include "sos_device.h"

namespace {

constexpr int PE_CHUNK = 64;                            // samples per lane and hand-over
constexpr int PE_TILE = 64 * PE_CHUNK;                  // samples per wave
constexpr int PE_ROW = PE_CHUNK + 1;                    // LDS row stride in float32
constexpr int PE_POWERS = 13;                           // A^(64 * 2^b), b = 0 ... 12

struct PePlan {                                         // by value in the kernel arguments
    double c[2][5];                                     // b0 b1 b2 a1 a2
    double zi[4];
    double P[PE_POWERS][16];                            // row-major (2 S) x (2 S); P[6] = A^4096, P[12] = A^(64 * 4096)
};

struct PeArgs {
    const float *x;
    float *y;
    long long x_pitch, y_pitch, frames, pad, n_tiles, first, step, n_out;
    double gain;
    int root;
    double *vf, *vb;                                    // [row][tile][lane][2 S]: forward (pe_pass<1>: entering states), backward
    double *tf, *tb;                                    // [row][tile][2 S]: the tiles' entering states
    int *bad;                                           // [row]: holds a NaN or an infinity
};

static_assert(sizeof(PePlan) + sizeof(PeArgs) <= 4096, "kernel arguments");

template <int S>
__device__ __forceinline__ double pe_step(const double (&c)[2][5], double (&z)[2 * S], double v)
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
__device__ __forceinline__ void pe_matvec(const double *M, const double (&s)[2 * S], double (&a)[2 * S])
{
#pragma unroll
    for (int i = 0; i < 2 * S; i++) {
        double t = M[i * (2 * S)] * s[0];
#pragma unroll
        for (int j = 1; j < 2 * S; j++) t += M[i * (2 * S) + j] * s[j];
        a[i] = t;
    }
}

// z_r <- sum over the ranks m <= r of A^(n (r - m)) z_m, n = 64 * 2^base; DOWN: rank r is lane 63 - r
template <int S, bool DOWN>
__device__ __forceinline__ void pe_scan(const PePlan &pl, int base, int rank, double (&z)[2 * S])
{
#pragma unroll
    for (int b = 0; b < 6; b++) {
        double o[2 * S], a[2 * S];
#pragma unroll
        for (int j = 0; j < 2 * S; j++) o[j] = DOWN ? __shfl_down(z[j], 1 << b, 64) : __shfl_up(z[j], 1 << b, 64);
        pe_matvec<S>(pl.P[base + b], o, a);
        if (rank >= (1 << b)) {
#pragma unroll
            for (int j = 0; j < 2 * S; j++) z[j] += a[j];
        }
    }
}

// s <- A^(n rank) s, the power applied by the bits of rank < 64
template <int S>
__device__ __forceinline__ void pe_advance(const PePlan &pl, int base, int rank, double (&s)[2 * S])
{
#pragma unroll
    for (int b = 0; b < 6; b++) {
        if ((rank >> b) & 1) {
            double a[2 * S];
            pe_matvec<S>(pl.P[base + b], s, a);
#pragma unroll
            for (int j = 0; j < 2 * S; j++) s[j] = a[j];
        }
    }
}

// MODE 0: forward summaries; 1: forward entering states and backward summaries; 2: the result
template <int S, int MODE>
__global__ __launch_bounds__(64) void pe_pass(const PePlan pl, const PeArgs a)
{
    __shared__ float tile[64 * PE_ROW];
    const int lane = threadIdx.x;
    const long long t = blockIdx.x, row = blockIdx.y;
    const long long frames = a.frames, pad = a.pad, E = frames + 2 * pad;
    const long long t0 = t * PE_TILE;                   // first position of the tile in the extended sequence
    const long long left = E - t0;
    const int nt = left < PE_TILE ? (int)left : PE_TILE;
    const float *v = a.x + row * a.x_pitch;

    // branch-free and unrolled, so that a batch of loads is in flight at once; positions behind the sequence's end repeat its
    // last sample (their chunks are never run)
    bool nonfinite = false;
#pragma unroll 16
    for (int k = 0; k < 64; k++) {
        long long i = t0 + k * 64 + lane;
        if (i > E - 1) i = E - 1;
        const long long idx = i < pad ? pad - i : (i >= pad + frames ? 2 * frames + pad - 2 - i : i - pad);
        const float s = v[idx];
        nonfinite = nonfinite || !(fabsf(s) <= 3.402823466e38f);
        tile[k * PE_ROW + lane] = s;
    }
    __syncthreads();

    const double x0 = (double)v[0], xl = (double)v[frames - 1];
    const double u_first = x0 * x0, u_last = xl * xl;   // exact: 24 + 24 bits
    const long long dl = pad - t0, dr = pad + frames - t0;
    const int ql = dl < 0 ? 0 : (dl > PE_TILE ? PE_TILE : (int)dl);     // in the tile: [0, ql) left extension,
    const int qr = dr < 0 ? 0 : (dr > PE_TILE ? PE_TILE : (int)dr);     // [qr, 4096) right extension
    const int q0 = lane * PE_CHUNK;
    const int n = nt - q0 < 0 ? 0 : (nt - q0 < PE_CHUNK ? nt - q0 : PE_CHUNK);
    const long long slot = ((row * a.n_tiles + t) * 64 + lane) * (2 * S);
    float *mine = tile + lane * PE_ROW;
    auto sample = [&](int i) -> double {                // sample q0 + i of the tile: the square, or its odd extension
        const double f = (double)mine[i];
        const double u = f * f;
        const int q = q0 + i;
        return q < ql ? 2.0 * u_first - u : (q >= qr ? 2.0 * u_last - u : u);
    };

    double c[2][5];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int j = 0; j < 5; j++) c[s][j] = pl.c[s][j];

    // the forward pass over the lane's chunk
    double z[2 * S];
    if (MODE == 2) {
#pragma unroll
        for (int j = 0; j < 2 * S; j++) z[j] = a.vf[slot + j];
    } else {
#pragma unroll
        for (int j = 0; j < 2 * S; j++) z[j] = 0.0;
        if (MODE == 1) {                                // A^(64 lane) (the tile's entering state) + what the lanes in front add
            double w[2 * S];
#pragma unroll
            for (int j = 0; j < 2 * S; j++) {
                z[j] = a.tf[(row * a.n_tiles + t) * (2 * S) + j];
                w[j] = __shfl_up(a.vf[slot + j], 1, 64);
            }
            pe_advance<S>(pl, 0, lane, z);
            if (lane > 0) {
#pragma unroll
                for (int j = 0; j < 2 * S; j++) z[j] += w[j];
            }
        }
        if (t == 0 && lane == 0) {                      // scipy's zi * (first sample of the extended sequence)
            const double w0 = sample(0);
#pragma unroll
            for (int j = 0; j < 2 * S; j++) z[j] += pl.zi[j] * w0;
        }
        if (MODE == 1) {
#pragma unroll
            for (int j = 0; j < 2 * S; j++) a.vf[slot + j] = z[j];
        }
    }

    if (MODE == 0) {
#pragma unroll 8
        for (int i = 0; i < PE_CHUNK; i++)
            if (i < n) pe_step<S>(c, z, sample(i));
        if (__ballot(nonfinite) != 0) {
#pragma unroll
            for (int j = 0; j < 2 * S; j++) z[j] = __longlong_as_double(0x7ff8000000000000LL);
        }
        pe_scan<S, false>(pl, 0, lane, z);
#pragma unroll
        for (int j = 0; j < 2 * S; j++) a.vf[slot + j] = z[j];
        return;
    }

    double yf[PE_CHUNK];                                // the forward output stays in registers, float64
    double y_end = 0.0;
#pragma unroll
    for (int i = 0; i < PE_CHUNK; i++) {
        yf[i] = 0.0;
        if (i < n) {
            yf[i] = pe_step<S>(c, z, sample(i));
            y_end = yf[i];
        }
    }

    // the backward pass over it; the chunk that holds the sequence's last sample starts from zi * (that forward output)
    const int rank = 63 - lane;
    double zb[2 * S];
#pragma unroll
    for (int j = 0; j < 2 * S; j++) zb[j] = 0.0;
    if (MODE == 2) {
        double w[2 * S];
#pragma unroll
        for (int j = 0; j < 2 * S; j++) {
            zb[j] = a.tb[(row * a.n_tiles + t) * (2 * S) + j];
            w[j] = __shfl_down(a.vb[slot + j], 1, 64);
        }
        pe_advance<S>(pl, 0, rank, zb);
        if (rank > 0) {
#pragma unroll
            for (int j = 0; j < 2 * S; j++) zb[j] += w[j];
        }
    }
    if (t == a.n_tiles - 1 && n > 0 && q0 + n == nt) {
#pragma unroll
        for (int j = 0; j < 2 * S; j++) zb[j] += pl.zi[j] * y_end;
    }

    if (MODE == 1) {
#pragma unroll
        for (int i = PE_CHUNK - 1; i >= 0; i--)
            if (i < n) pe_step<S>(c, zb, yf[i]);
        pe_scan<S, true>(pl, 0, rank, zb);
#pragma unroll
        for (int j = 0; j < 2 * S; j++) a.vb[slot + j] = zb[j];
        return;
    }

    const double gain = a.gain;
#pragma unroll
    for (int i = PE_CHUNK - 1; i >= 0; i--) {
        if (i < n) {
            const double o = pe_step<S>(c, zb, yf[i]);
            mine[i] = (float)(gain * (o > 0.0 ? o : 0.0));      // the product in float64, one rounding
        }
    }
    __syncthreads();

    // the tile holds the row's samples [r0, r0 + nt); of those inside the row, the ones on the grid first + j step, j < n_out
    const long long r0 = t0 - pad;
    const long long lo = r0 > a.first ? r0 : a.first, hi = r0 + nt < frames ? r0 + nt : frames;
    if (hi <= lo) return;
    const long long d = lo - a.first;
    const long long j_lo = d / a.step + (d % a.step != 0);
    long long j_hi = (hi - 1 - a.first) / a.step + 1;
    if (j_hi > a.n_out) j_hi = a.n_out;
    const bool isbad = a.bad[row] != 0;
    float *out = a.y + row * a.y_pitch;
    for (long long j = j_lo + lane; j < j_hi; j += 64) {
        const int q = (int)(a.first + j * a.step - r0);
        float p = tile[(q >> 6) * PE_ROW + (q & 63)];
        if (a.root) p = (float)sqrt((double)p);         // correctly rounded: 53 >= 2 * 24 + 2 bits
        out[j] = isbad ? __uint_as_float(0x7fc00000u) : p;
    }
}

// one wave per row: the entering state of every tile, 64 tiles at a time; DOWN: from the last tile
template <int S, bool DOWN>
__global__ __launch_bounds__(64) void pe_carry(const PePlan pl, const PeArgs a)
{
    const int lane = threadIdx.x;
    const long long row = blockIdx.x, n_tiles = a.n_tiles;
    const double *sums = (DOWN ? a.vb : a.vf) + row * n_tiles * 64 * (2 * S) + (DOWN ? 0 : 63) * (2 * S);
    double *enter = (DOWN ? a.tb : a.tf) + row * n_tiles * (2 * S);
    double s[2 * S];
#pragma unroll
    for (int j = 0; j < 2 * S; j++) s[j] = 0.0;
    bool nonfinite = false;
    for (long long k0 = 0; k0 < n_tiles; k0 += 64) {
        const long long k = k0 + lane;                  // in the pass's order
        const bool active = k < n_tiles;
        const long long t = DOWN ? n_tiles - 1 - k : k;
        double z[2 * S], e[2 * S], w[2 * S], nx[2 * S];
#pragma unroll
        for (int j = 0; j < 2 * S; j++) z[j] = active ? sums[t * 64 * (2 * S) + j] : 0.0;
        nonfinite = nonfinite || z[0] != z[0];
        pe_scan<S, false>(pl, 6, lane, z);
#pragma unroll
        for (int j = 0; j < 2 * S; j++) {
            e[j] = s[j];
            w[j] = __shfl_up(z[j], 1, 64);
        }
        pe_advance<S>(pl, 6, lane, e);
        if (active) {
#pragma unroll
            for (int j = 0; j < 2 * S; j++) enter[t * (2 * S) + j] = lane > 0 ? e[j] + w[j] : e[j];
        }
        pe_matvec<S>(pl.P[12], s, nx);
#pragma unroll
        for (int j = 0; j < 2 * S; j++) s[j] = nx[j] + __shfl(z[j], 63, 64);
    }
    if (!DOWN) {
        const bool any = __ballot(nonfinite) != 0;
        if (lane == 0) a.bad[row] = any ? 1 : 0;
    }
}

template <int S>
int pe_launch(hipdsp_ctx *ctx, const PePlan &pl, const PeArgs &a, long long channels)
{
    const dim3 gt((unsigned)a.n_tiles, (unsigned)channels), gr((unsigned)channels), b(64);
    hipLaunchKernelGGL((pe_pass<S, 0>), gt, b, 0, ctx->stream, pl, a);
    HD_TRY(hd_launch_status("pe_pass (forward summaries)"));
    hipLaunchKernelGGL((pe_carry<S, false>), gr, b, 0, ctx->stream, pl, a);
    HD_TRY(hd_launch_status("pe_carry (forward)"));
    hipLaunchKernelGGL((pe_pass<S, 1>), gt, b, 0, ctx->stream, pl, a);
    HD_TRY(hd_launch_status("pe_pass (backward summaries)"));
    hipLaunchKernelGGL((pe_carry<S, true>), gr, b, 0, ctx->stream, pl, a);
    HD_TRY(hd_launch_status("pe_carry (backward)"));
    hipLaunchKernelGGL((pe_pass<S, 2>), gt, b, 0, ctx->stream, pl, a);
    return hd_launch_status("pe_pass (result)");
}

// A^(64 * 2^b), b = 0 ... 12, of the cascade's state transition (input zero), n = 2 S states: squared in long double, every
// power rounded once
void pe_powers(const double c[2][5], int S, double P[PE_POWERS][16])
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
    for (int sq = 1; sq <= 6 + PE_POWERS - 1; sq++) {   // A^(2^sq); 2^6 = PE_CHUNK
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                long double acc = 0.0L;
                for (int k = 0; k < n; k++) acc += A[i][k] * A[k][j];
                T[i][j] = acc;
            }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) A[i][j] = T[i][j];
        if (sq >= 6)
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++) P[sq - 6][i * n + j] = (double)A[i][j];
    }
}
static_assert(PE_CHUNK == 64 && PE_TILE == 4096, "pe_powers stores the squarings from 6 on; pe_carry starts at P[6]");

}  // namespace

extern "C" int hipdsp_power_envelope(hipdsp_ctx *ctx, const hipdsp_sosplan *plan, const float *x, int64_t x_pitch,
                                     int64_t channels, int64_t frames, int64_t first, int64_t step, int64_t n_out,
                                     double gain, int root, float *y, int64_t y_pitch)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(plan != nullptr && plan->stage.valid, "hipdsp_power_envelope: no plan, or a plan that has not been set");
    HD_REQUIRE(channels >= 0 && frames >= 0 && n_out >= 0, "negative size");
    HD_REQUIRE(step >= 1, "step %lld < 1", (long long)step);
    HD_REQUIRE(first >= 0, "first %lld < 0", (long long)first);
    HD_REQUIRE(n_out == 0 || (first < frames && n_out - 1 <= (frames - 1 - first) / step),
               "sample first + (n_out - 1) step = %lld + %lld * %lld lies behind the row's %lld frames", (long long)first,
               (long long)(n_out - 1), (long long)step, (long long)frames);
    HD_REQUIRE(gain > 0.0 && gain <= 1.7976931348623157e308, "gain %g is not a positive finite number", gain);
    HD_REQUIRE(x_pitch >= frames, "x_pitch smaller than frames");
    HD_REQUIRE(y_pitch >= n_out, "y_pitch smaller than n_out");
    HD_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0, "misaligned pointer");
    HD_NO_OVERLAP(x, x_pitch, frames, y, y_pitch, n_out, channels, "x and y");
    HD_REQUIRE(!hd_capturing(ctx), "hipdsp_power_envelope sizes its scratch per call: not during stream capture");
    const SosPlanDev &host = *plan->host;
    const int S = host.n_sections;
    if (S < 1 || S > 2) {
        hipdsp_set_error("hipdsp_power_envelope: a plan of %d sections, 1 or 2 are served", S);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    HD_TRY(hd_check_rows_limits(channels, frames, HD_MAX_FRAMES));
    const long long pad = host.edge;
    if (frames <= pad) {
        hipdsp_set_error("the length of the input vector x must be greater than padlen, which is %lld", pad);
        return HIPDSP_ERR_TOO_SHORT;
    }
    if (channels == 0 || n_out == 0) return HIPDSP_OK;
    HD_REQUIRE(x != nullptr && y != nullptr, "NULL data pointer");

    PePlan pl;
    memset(&pl, 0, sizeof(pl));
    for (int s = 0; s < S; s++)
        for (int j = 0; j < 5; j++) pl.c[s][j] = host.coef[s][j];
    for (int j = 0; j < 2 * S; j++) pl.zi[j] = host.zi[j];
    pe_powers(pl.c, S, pl.P);

    PeArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x, a.y = y, a.x_pitch = x_pitch, a.y_pitch = y_pitch, a.frames = frames, a.pad = pad;
    a.n_tiles = (frames + 2 * pad + PE_TILE - 1) / PE_TILE;
    a.first = first, a.step = step, a.n_out = n_out, a.gain = gain, a.root = root != 0;
    HD_REQUIRE(a.n_tiles <= 0x7fffffffLL, "too many samples for one call");

    HD_CHECK_HIP(hipSetDevice(ctx->device));
    const size_t tiles = (size_t)channels * (size_t)a.n_tiles;
    HdCarve count(nullptr);
    count.take<double>(tiles * 64 * 2 * S), count.take<double>(tiles * 64 * 2 * S);
    count.take<double>(tiles * 2 * S), count.take<double>(tiles * 2 * S), count.take<int>((size_t)channels);
    void *work = nullptr;
    HD_TRY(hipdsp_scratch(ctx, count.bytes(), &work));
    HdCarve carve(work);
    a.vf = carve.take<double>(tiles * 64 * 2 * S), a.vb = carve.take<double>(tiles * 64 * 2 * S);
    a.tf = carve.take<double>(tiles * 2 * S), a.tb = carve.take<double>(tiles * 2 * S), a.bad = carve.take<int>((size_t)channels);
    return S == 1 ? pe_launch<1>(ctx, pl, a, channels) : pe_launch<2>(ctx, pl, a, channels);
}
