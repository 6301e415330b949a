// hipdsp_template_match: spectrogram cross-correlation -- up to 16 templates of one shape (Tt frames x Fb bins) slid
// along a band of bins of a planar spectrogram slab, raw (a 2-D correlation) or normalised (the Pearson coefficient of
// template and patch), one score row per template and channel (include/hip_dsp.h).
//
// A GEMM whose A matrix is never built: with n = Tt*Fb the patch matrix has one row of n values per window, and window
// t's row is the slab's frames t .. t+Tt-1.  The fragment layout, the walk over a frame's bins, the transpose of the
// accumulators and the store loop behind it, the raising of the LDS limit and the host's checks of the output block are
// mfma_bank.h's, shared with hipdsp_fir_bank (firbank.hip); the plan's staged block is plan_stage.h's.  What is here
// is the tile of the slab, the order of the slots, the band sums and the three epilogues.
// The products run on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain):
//     M = 16 window starts     lane l holds A[m = l & 15][k = l >> 4]: ONE LDS read at (frame m + a, bin b + (l >> 4))
//                              of the staged tile;
//     N = 16 templates         lane l holds B[k = l >> 4][n = l & 15]: the plan keeps the taps as (slot, template) rows
//                              of 16 floats in the order the slots are walked, so a k-step's B fragment is 64
//                              consecutive floats;
//     K = 4 bins of one frame per step.
// A workgroup of four waves owns TM = 64*MT = 256 consecutive windows of one channel; every wave carries MT = 4
// independent accumulators that share each B fragment (40 cycles of dependent latency against 32 of issue).  All 16
// template columns are always computed, unused ones hold zero taps.
//
// The band is cut into chunks of FC bins (the last one shorter, rounded up to a multiple of 4 with zero taps AND zero
// values).  Per chunk the (TM + Tt - 1) frames under the tile are staged once in LDS, rows RS = FC + 2 floats apart:
// RS/2 is odd, so the 32 lanes a ds_read_b32 serves at once (16 frames x 2 bins) fall on 32 different banks.  An
// element is converted while it is staged -- decibel_of (decibel.h), the floor, minus the pivot -- and never again.
// K is walked chunk by chunk, inside a chunk frame by frame, inside a frame in fours of bins: an order fixed by
// (Tt, Fb) alone (tm_shape), the same for every window, tile, channel and template count -- a 16-template call is bit
// for bit 16 one-template calls, and a window alone is the window inside a long call.
//
// Normalised mode: 16 lanes stage one frame's piece of the band and add (v - pivot) and its square in float64 (lane j
// the bins = j mod 16 of the chunk in ascending order, then a fixed xor tree, then chunk after chunk): S1, S2 and a
// finiteness flag per frame, in LDS.  Every window then adds ITS Tt frames directly, in ascending order -- no
// difference of prefix sums, which would lose the bound -- and the epilogue forms
//     r = (G - (S1/n) H0) / (sqrt(Q) sqrt(S2 - S1^2/n))
// in float64 from the accumulator G, rounded to float32 once.
//
// LDS: tile <= TILE_CAP floats (64 KB) + 8 KB of taps + (16 B + 4 B) per frame + 16 B per window.  The tile is always
// MT = 4 (256 windows: the halo of Tt - 1 frames is staged once per tile, the larger tile wins over the wider chunk);
// tm_shape takes the widest chunk (64, 32, 16 bins) whose tile fits -- 16 always does: two workgroups per CU up to
// Tt ~ 100 (32 x 128: 39 + 8 + 10 KB), one for the longest templates.
// Frames outside [0, frames) are staged as zeros (their windows store NaN); every global read is bounds-checked against
// frames and the band, every store against n_out and the template count.  Index arithmetic on the slab is 64-bit.
#include "mfma_bank.h"
#include "plan_stage.h"
#include "decibel.h"
#include <cmath>
#include <cstddef>
#include <vector>

namespace {

constexpr int MAX_TEMPLATES = 16;
constexpr int MAX_ROWS = 256;                 // Tt
constexpr int MAX_TAPS = 65536;               // Tt * Fb
constexpr int MAX_SLOTS = MAX_TAPS + 3 * MAX_ROWS;   // every frame of the last chunk padded to a multiple of 4
constexpr int TILE_CAP = 16384;               // floats of slab a tile may stage (64 KB)
constexpr int TM_MT = 4;                      // accumulators per wave: 64 windows each, 256 per workgroup

struct TmplHead {
    double h0[MAX_TEMPLATES];                 // sum of the rounded taps
    double sq[MAX_TEMPLATES];                 // sqrt(Q), Q = sum (g - mean g)^2 of the rounded taps
};

struct TmplTaps {
    TmplHead head;
    float taps[MAX_SLOTS * MAX_TEMPLATES];    // [slot][template]; zero in the padding and beyond n_templates
};

struct TmShape {
    int fc, rs, rows_lds;                     // bins per chunk, row stride, frames staged
    int n_slots;                              // tap slots of the whole walk
};

// the mapping: by (Tt, Fb) alone
TmShape tm_shape(int Tt, int Fb)
{
    TmShape s;
    const int fb4 = (Fb + 3) & ~3;
    s.rows_lds = 64 * TM_MT + Tt - 1;
    s.fc = fb4 < 16 ? fb4 : 16;               // always fits: (256 + 255) * 18 floats
    for (int fc = 64; fc > 16; fc >>= 1) {
        const int w = fb4 < fc ? fb4 : fc;
        if (s.rows_lds * (w + 2) <= TILE_CAP) { s.fc = w; break; }
    }
    s.rs = s.fc + 2;
    s.n_slots = Tt * fb4;                     // full chunks: Tt*fc each; the last: Tt * (its width rounded up to 4)
    return s;
}

// bytes of a plan of n_slots slots: what set_host writes and upload copies
size_t tm_used(int n_slots) { return offsetof(TmplTaps, taps) + sizeof(float) * 16 * (size_t)n_slots; }

struct TmArgs {
    long long spec_pitch, frames, first, n_out, out_pitch, out_template_pitch;
    int nfreq, k0, Tt, Fb, nk, fc, rs, rows_lds, a_floats, db;
    float floor, pivot;
    double thr;                               // n * min_std^2
    DbArgs dba;
};

template <bool NORM>
__global__ __launch_bounds__(256) void template_match_kernel(const TmplTaps *__restrict__ plan,
                                                             const float *__restrict__ spec, float *__restrict__ out,
                                                             TmArgs g)
{
    extern __shared__ double tm_lds[];
    constexpr int MT = TM_MT, TM = 64 * MT;
    const int RP = (g.rows_lds + 1) & ~1;
    double *S1 = tm_lds, *S2 = S1 + RP;        // per staged frame: band sums of (v - pivot) and its square
    double *OM = S2 + RP, *OD = OM + 256;      // per window: S1/n and sqrt(D) (NaN where the window is masked)
    int *BAD = (int *)(OD + 256);              // per staged frame: does the band hold a non-finite value?
    float *A = (float *)(BAD + RP);            // the tile; reused by the epilogue
    float *B = A + g.a_floats;                 // TAPS_KB x 16 taps
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c = blockIdx.y;
    const long long tile0 = (long long)blockIdx.x * TM;
    const long long left = g.n_out - tile0;
    const int rows = left < TM ? (int)left : TM;           // windows of this tile that exist
    const int Tt = g.Tt, RS = g.rs;
    const int rlive = rows + Tt - 1;                       // frames under them
    const long long t0 = g.first + tile0;                  // frame of staged row 0
    const float *sc = spec + c * g.spec_pitch;
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int mrow = wave * 16 * MT + (lane & 15), kq = lane >> 4;
    const int sub = tid & 15;

    for (int cb = 0; cb < g.Fb; cb += g.fc) {
        const int w = g.Fb - cb < g.fc ? g.Fb - cb : g.fc, w4 = (w + 3) & ~3;
        if (cb > 0) __syncthreads();                       // the previous chunk has been read
        for (int r0 = 0; r0 < rlive; r0 += 16) {           // 16 lanes per frame: uniform trip count, the shuffles need it
            const int r = r0 + (tid >> 4);
            const long long t = t0 + r;
            const bool inside = r < rlive && t >= 0 && t < g.frames;
            const float *row = sc + t * (long long)g.nfreq + g.k0 + cb;
            double s1 = 0.0, s2 = 0.0;
            int bad = 0;
            for (int b = sub; b < w4; b += 16) {
                float xf = 0.0f;
                if (inside && b < w) {
                    const float p = row[b];
                    float v = g.db ? decibel_of(p, g.dba) : p;
                    v = v < g.floor ? g.floor : v;             // a NaN stays
                    xf = v - g.pivot;
                    if (NORM) {
                        const double d = (double)v - (double)g.pivot;
                        s1 += d;
                        s2 += d * d;
                        bad |= !(fabsf(v) <= FLT_MAX);
                    }
                }
                if (r < rlive) A[r * RS + b] = xf;
            }
            if (NORM) {
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) {
                    s1 += __shfl_xor(s1, d, 16);
                    s2 += __shfl_xor(s2, d, 16);
                    bad |= __shfl_xor(bad, d, 16);
                }
                if (sub == 0 && r < rlive) {
                    S1[r] = cb > 0 ? S1[r] + s1 : s1;
                    S2[r] = cb > 0 ? S2[r] + s2 : s2;
                    BAD[r] = cb > 0 ? (BAD[r] | bad) : bad;
                }
            }
        }
        const int fa = TAPS_KB / w4;                       // whole frames per B stage (w4 <= 64: at least two)
        const long long slot0 = (long long)Tt * cb;
        for (int a0 = 0; a0 < Tt; a0 += fa) {
            const int na = Tt - a0 < fa ? Tt - a0 : fa;
            __syncthreads();                               // the tile is staged / the previous taps have been read
            for (int idx = tid; idx < na * w4 * 16; idx += 256) B[idx] = plan->taps[(slot0 + (long long)a0 * w4) * 16 + idx];
            __syncthreads();
            // windows past `rows` read LDS nobody staged: their results are never stored, and a row of the MFMA only
            // depends on its own A row
            for (int a = 0; a < na; a++) {
                const float *Ar = A + (mrow + a0 + a) * RS + kq;
                const float *Br = B + a * w4 * 16 + lane;
                mb_walk(w4, [&](int b) {
                    const float bv = Br[b * 16];
#pragma unroll
                    for (int mt = 0; mt < MT; mt++)
                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ar[16 * mt * RS + b], bv, acc[mt], 0, 0, 0);
                });
            }
        }
    }
    __syncthreads();
    if (NORM && tid < rows) {
        double s1 = 0.0, s2 = 0.0;
        int bad = 0;
        for (int a = 0; a < Tt; a++) {
            s1 += S1[tid + a];
            s2 += S2[tid + a];
            bad |= BAD[tid + a];
        }
        const double n = (double)Tt * (double)g.Fb;
        const double D = s2 - s1 * s1 / n;
        OM[tid] = s1 / n;
        OD[tid] = (bad || !(D > g.thr)) ? (double)NAN : sqrt(D);
    }
    constexpr int OT = 16 * MT;
    const float *O = mb_transpose<MT>(A, acc, wave, lane);
    mb_store<MT>(O, lane, g.nk, tile0 + wave * OT, g.n_out, out + c * g.out_pitch, g.out_template_pitch,
                 [&](float G, int n, int tl, long long i) -> float {
                     const long long t = g.first + i;
                     if (t < 0 || t + Tt > g.frames) return NAN;
                     if (NORM) {
                         const int o = wave * OT + tl;
                         const float v = (float)(((double)G - OM[o] * plan->head.h0[n]) / (plan->head.sq[n] * OD[o]));
                         return v > 1.0f ? 1.0f : (v < -1.0f ? -1.0f : v);      // a coefficient; NaN stays
                     }
                     return g.pivot == 0.0f ? G : (float)((double)G + (double)g.pivot * plan->head.h0[n]);
                 });
}

size_t tm_lds_bytes(int rows_lds, int a_floats)
{
    const int RP = (rows_lds + 1) & ~1;
    return (size_t)(2 * RP + 512) * sizeof(double) + (size_t)RP * sizeof(int) +
           (size_t)(a_floats + TAPS_KB * 16) * sizeof(float);
}

std::atomic<int> tm_raised[64];

int tm_raise_all(hipdsp_ctx *ctx)
{
    return mb_raise_lds(ctx, tm_raised, {(const void *)template_match_kernel<true>, (const void *)template_match_kernel<false>},
                        (int)tm_lds_bytes(256 + MAX_ROWS - 1, TILE_CAP));
}

template <bool NORM>
int tm_launch(hipdsp_ctx *ctx, const TmplTaps *dev, const float *spec, float *out, const TmArgs &g, long long channels)
{
    constexpr int TM = 64 * TM_MT;
    const dim3 grid((unsigned)((g.n_out + TM - 1) / TM), (unsigned)channels);
    hipLaunchKernelGGL(template_match_kernel<NORM>, grid, dim3(256), tm_lds_bytes(g.rows_lds, g.a_floats),
                       ctx->stream, dev, spec, out, g);
    return hd_launch_status("template_match_kernel");
}

}  // namespace

struct hipdsp_tmplplan {
    hd_plan_stage stage;   // a TmplTaps
    int n_templates, rows, cols, normalize;          // of the last set_host
    int up_templates, up_rows, up_cols, up_normalize; // of the last upload (0 before the first): what the device block holds
};

extern "C" {

int hipdsp_template_prepare_host(const double *templates, int n, int rows, int cols, int normalize, float *taps_out,
                                 double *sum_out, double *norm_out)
{
    HD_REQUIRE(templates != nullptr && taps_out != nullptr && sum_out != nullptr && norm_out != nullptr, "NULL argument");
    HD_REQUIRE(n >= 1 && rows >= 1 && cols >= 1, "n %d, rows %d and cols %d must be positive", n, rows, cols);
    if (n > MAX_TEMPLATES || rows > MAX_ROWS || (long long)rows * cols > MAX_TAPS) {
        hipdsp_set_error("at most %d templates of %d frames and %d values per plan, got %d of %d x %d", MAX_TEMPLATES,
                         MAX_ROWS, MAX_TAPS, n, rows, cols);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    const int m = rows * cols;
    for (int k = 0; k < n; k++) {
        const double *h = templates + (size_t)k * m;
        float *gk = taps_out + (size_t)k * m;
        double lo = h[0], hi = h[0];
        for (int i = 0; i < m; i++) {
            HD_REQUIRE(std::isfinite(h[i]), "template %d holds a non-finite value at element %d", k, i);
            lo = h[i] < lo ? h[i] : lo;
            hi = h[i] > hi ? h[i] : hi;
        }
        if (normalize) {
            HD_REQUIRE(hi > lo, "template %d is constant: it has no correlation coefficient", k);
            long double sum = 0.0L, ss = 0.0L;
            for (int i = 0; i < m; i++) sum += (long double)h[i];
            const long double mean = sum / (long double)m;
            for (int i = 0; i < m; i++) {
                const long double d = (long double)h[i] - mean;
                ss += d * d;
            }
            const long double norm = sqrtl(ss);
            HD_REQUIRE(norm > 0.0L && std::isfinite((double)norm), "template %d: variance is zero or overflows", k);
            for (int i = 0; i < m; i++) gk[i] = (float)(((long double)h[i] - mean) / norm);
        } else {
            for (int i = 0; i < m; i++) {
                gk[i] = (float)h[i];
                HD_REQUIRE(std::isfinite(gk[i]), "template %d: element %d overflows float32", k, i);
            }
        }
        long double h0 = 0.0L, q = 0.0L;
        for (int i = 0; i < m; i++) h0 += (long double)gk[i];
        const long double gm = h0 / (long double)m;
        for (int i = 0; i < m; i++) {
            const long double d = (long double)gk[i] - gm;
            q += d * d;
        }
        sum_out[k] = (double)h0;
        norm_out[k] = (double)q;
        HD_REQUIRE(!normalize || norm_out[k] > 0.0, "template %d: the rounded taps are constant", k);
    }
    return HIPDSP_OK;
}

int hipdsp_tmplplan_create(hipdsp_ctx *ctx, hipdsp_tmplplan **out)
{
    HD_REQUIRE(ctx != nullptr && out != nullptr, "NULL argument");
    *out = nullptr;
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    hipdsp_tmplplan *p = new hipdsp_tmplplan();
    int rc = hd_stage_create(ctx, &p->stage, sizeof(TmplTaps), true);   // uploads copy the used prefix only
    if (rc == HIPDSP_OK) rc = tm_raise_all(ctx);
    if (rc != HIPDSP_OK) {
        hd_stage_destroy(ctx, &p->stage);
        delete p;
        return rc;
    }
    *out = p;
    return HIPDSP_OK;
}

int hipdsp_tmplplan_destroy(hipdsp_ctx *ctx, hipdsp_tmplplan *plan)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    if (!plan) return HIPDSP_OK;
    hd_stage_destroy(ctx, &plan->stage);
    delete plan;
    return HIPDSP_OK;
}

int hipdsp_tmplplan_set_host(hipdsp_ctx *ctx, hipdsp_tmplplan *plan, const double *host_templates, int n_templates,
                             int rows, int cols, int normalize)
{
    HD_REQUIRE(ctx != nullptr && plan != nullptr && host_templates != nullptr, "NULL argument");
    HD_REQUIRE(n_templates >= 1 && rows >= 1 && cols >= 1, "n_templates %d, rows %d and cols %d must be positive",
               n_templates, rows, cols);
    if (n_templates > MAX_TEMPLATES || rows > MAX_ROWS || (long long)rows * cols > MAX_TAPS) {
        hipdsp_set_error("at most %d templates of %d frames and %d values per plan, got %d of %d x %d", MAX_TEMPLATES,
                         MAX_ROWS, MAX_TAPS, n_templates, rows, cols);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    // validated and prepared before the block is waited for or touched: a refused set leaves the plan as it was
    const size_t m = (size_t)rows * cols;
    std::vector<float> taps(m * n_templates);
    double h0[MAX_TEMPLATES], q[MAX_TEMPLATES];
    int rc = hipdsp_template_prepare_host(host_templates, n_templates, rows, cols, normalize, taps.data(), h0, q);
    if (rc == HIPDSP_OK) rc = hd_stage_host_free(&plan->stage);
    if (rc != HIPDSP_OK) return rc;
    TmplTaps *h = (TmplTaps *)plan->stage.host;
    const TmShape s = tm_shape(rows, cols);
    const int old_slots = plan->rows > 0 ? tm_shape(plan->rows, plan->cols).n_slots : 0;
    memset(h, 0, tm_used(s.n_slots > old_slots ? s.n_slots : old_slots));
    for (int k = 0; k < n_templates; k++) {
        h->head.h0[k] = h0[k];
        h->head.sq[k] = sqrt(q[k]);
        for (int cb = 0; cb < cols; cb += s.fc) {
            const int w = cols - cb < s.fc ? cols - cb : s.fc, w4 = (w + 3) & ~3;
            for (int a = 0; a < rows; a++)
                for (int b = 0; b < w; b++)
                    h->taps[((size_t)rows * cb + (size_t)a * w4 + b) * 16 + k] = taps[(size_t)k * m + (size_t)a * cols + cb + b];
        }
    }
    plan->n_templates = n_templates;
    plan->rows = rows;
    plan->cols = cols;
    plan->normalize = normalize ? 1 : 0;
    return HIPDSP_OK;
}

int hipdsp_tmplplan_upload(hipdsp_ctx *ctx, hipdsp_tmplplan *plan)
{
    HD_REQUIRE(ctx != nullptr && plan != nullptr, "NULL argument");
    HD_REQUIRE(plan->n_templates > 0, "plan has no templates yet");
    const int rc = hd_stage_upload(ctx, &plan->stage, tm_used(tm_shape(plan->rows, plan->cols).n_slots));
    if (rc != HIPDSP_OK) return rc;
    plan->up_templates = plan->n_templates;
    plan->up_rows = plan->rows;
    plan->up_cols = plan->cols;
    plan->up_normalize = plan->normalize;
    return HIPDSP_OK;
}

int hipdsp_tmplplan_set(hipdsp_ctx *ctx, hipdsp_tmplplan *plan, const double *host_templates, int n_templates, int rows,
                        int cols, int normalize)
{
    int rc = hipdsp_tmplplan_set_host(ctx, plan, host_templates, n_templates, rows, cols, normalize);
    if (rc != HIPDSP_OK) return rc;
    return hipdsp_tmplplan_upload(ctx, plan);
}

int hipdsp_template_match(hipdsp_ctx *ctx, const hipdsp_tmplplan *plan, const float *spec, int64_t spec_pitch,
                          int64_t channels, int64_t frames, int64_t nfreq, int64_t k0, int64_t first, int64_t n_out, int db,
                          double ref_power, double min_power, float floor, float pivot, double min_std, float *out,
                          int64_t out_pitch, int64_t out_template_pitch)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(plan != nullptr, "plan is NULL");
    HD_REQUIRE(plan->n_templates > 0, "plan has no templates yet");
    HD_REQUIRE(plan->up_templates == plan->n_templates && plan->up_rows == plan->rows && plan->up_cols == plan->cols &&
                   plan->up_normalize == plan->normalize,
               "the plan's %d templates of %d x %d have not been uploaded (the device holds %d of %d x %d)",
               plan->n_templates, plan->rows, plan->cols, plan->up_templates, plan->up_rows, plan->up_cols);
    HD_REQUIRE(channels >= 0 && frames >= 0 && nfreq >= 0 && n_out >= 0, "negative size");
    HD_REQUIRE(nfreq < (1LL << 30), "nfreq out of range");
    const int Tt = plan->rows, Fb = plan->cols, nk = plan->n_templates;
    HD_REQUIRE(k0 >= 0 && k0 + Fb <= nfreq, "band [%lld, %lld) not inside [0, %lld)", (long long)k0, (long long)k0 + Fb,
               (long long)nfreq);
    HD_REQUIRE(!db || ref_power > 0, "ref_power must be positive");
    HD_REQUIRE(floor == floor && pivot == pivot && fabsf(pivot) <= FLT_MAX, "floor is NaN or pivot is not finite");
    HD_REQUIRE(min_std >= 0 && min_std <= 1e150, "min_std %g must be >= 0 (and finite)", min_std);
    HD_REQUIRE(spec_pitch >= 0 && out_pitch >= 0 && out_template_pitch >= 0, "negative pitch");
    HD_REQUIRE(frames <= (1LL << 40), "too many frames");
    if (spec_pitch == 0) spec_pitch = frames * nfreq;
    HD_REQUIRE(spec_pitch >= frames * nfreq, "spec_pitch smaller than one channel");
    bool empty;
    int rc = mb_check_out("template", spec, frames, channels, n_out, out, &out_pitch, &out_template_pitch, &empty);
    if (rc != HIPDSP_OK || empty) return rc;
    HD_REQUIRE(first >= -(1LL << 60) && first <= (1LL << 60), "first out of range");
    HD_REQUIRE(frames == 0 || !mb_out_overlaps(spec, (channels - 1) * spec_pitch + frames * nfreq, out, nk, out_template_pitch,
                                               channels, out_pitch, n_out), "spec and out must not overlap");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    rc = tm_raise_all(ctx);
    if (rc != HIPDSP_OK) return rc;
    const TmShape s = tm_shape(Tt, Fb);
    TmArgs g;
    memset(&g, 0, sizeof(g));
    g.spec_pitch = spec_pitch; g.frames = frames; g.first = first; g.n_out = n_out;
    g.out_pitch = out_pitch; g.out_template_pitch = out_template_pitch;
    g.nfreq = (int)nfreq; g.k0 = (int)k0; g.Tt = Tt; g.Fb = Fb; g.nk = nk;
    g.fc = s.fc; g.rs = s.rs; g.rows_lds = s.rows_lds;
    g.a_floats = s.rows_lds * s.rs > OUT_FLOATS ? s.rows_lds * s.rs : OUT_FLOATS;
    g.db = db ? 1 : 0;
    g.floor = floor; g.pivot = pivot;
    g.thr = (double)Tt * (double)Fb * (min_std * min_std);
    g.dba = db ? db_args(ref_power, min_power) : db_args(1.0, 0.0);
    const TmplTaps *dev = (const TmplTaps *)plan->stage.dev;
    if (plan->normalize) return tm_launch<true>(ctx, dev, spec, out, g, channels);
    return tm_launch<false>(ctx, dev, spec, out, g, channels);
}

}  // extern "C"
