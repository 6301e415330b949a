// hipdsp_fir_bank: a bank of up to 16 FIR kernels over planar float32 traces, one feature trace per kernel -- the
// "feature expansion (kernel filter)" trace (include/hip_dsp.h).
//
// A sliding-window FIR bank is a GEMM whose A matrix is the Hankel matrix of the samples: with the taps reversed,
// g[i] = h[L-1-i], output time t is  sum_i g[i] * x[t + (L-1)/2 - (L-1) + i].  The products run on the f32-input matrix
// core, v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain, no wider accumulation):
//     M = 16 output times      lane l holds A[m = l & 15][k = l >> 4]: ONE LDS read at (row m, slot i + (l >> 4)) of the
//                              staged trace -- the Hankel matrix never exists;
//     N = 16 kernels           lane l holds B[k = l >> 4][n = l & 15] = g_n[i + (l >> 4)]: the plan keeps the taps as
//                              (slot, kernel) rows of 16 floats, so a k-step's B fragment is 64 consecutive floats;
//     K = 4 tap slots per step, L rounded up to a multiple of 4 with zero taps.
// A workgroup of four waves owns TM = 64*MT consecutive outputs of one channel; every wave carries MT independent
// accumulators (16 outputs each) that share each B fragment (40 cycles of dependent latency against 32 of issue: at
// least two are needed).  All 16 kernel columns are always computed -- unused ones hold zero taps -- and the tap slots
// are walked in ascending order whatever the tile, the layout or the chunking: the chain behind one output is the same
// everywhere, which is what makes a 16-kernel call bit for bit equal to 16 one-kernel calls.
//
// LDS layouts of the trace (chosen on the host by n_taps and step alone):
//   dense      the (rows-1)*step + L4 samples under the tile, staged once, each read from memory once (plus the halo);
//              output m, slot i sits at p = m*step + i.  step == 1: p itself (a wave's read covers 19 consecutive
//              words).  step > 1: p + (p >> 5), which spreads the rows over the banks when step is even.
//              MT = 4, 2 or 1: the largest tile whose span fits DENSE_CAP floats (two workgroups per CU).
//   window     for larger steps the span of even 64 outputs does not fit: every output gets its own row of 32 slots
//              (34 floats apart: the 32 lanes a ds_read_b32 serves at once -- 16 outputs x 2 slots -- fall on the 32
//              banks 2m + i), restaged for every 32 taps.
// The taps go through LDS in pieces of TAPS_KB slots.  The epilogue (threshold, max) runs on the VALU; the accumulators
// are transposed through LDS so that a kernel's row is stored along time.  The slot walk, the transpose, the store
// loop and the host's checks of the output block are mfma_bank.h's, shared with templatematch.hip; the plan's staged
// block is plan_stage.h's.
// Samples outside [0, frames) are zeros; every global read is bounds-checked against frames, every store against
// n_out and n_kernels.  Index arithmetic on the traces is 64-bit.
#include "mfma_bank.h"
#include "plan_stage.h"
#include <cstddef>

namespace {

constexpr int MAX_KERNELS = 16;
constexpr int MAX_TAPS = 4097;
constexpr int MAX_TAPS4 = (MAX_TAPS + 3) / 4 * 4;
constexpr int WIN_K = 32, WIN_RS = 34;        // window layout: slots per row, floats between rows
constexpr int DENSE_CAP = 17408;              // floats of trace a dense tile may stage (68 KB)

struct FirTaps {
    float threshold[MAX_KERNELS];
    float taps[MAX_TAPS4 * MAX_KERNELS];      // [slot i][kernel n] = float32(h_n[L-1-i]); zero beyond L and beyond n_kernels
};

// bytes of a plan of L taps: what set_host writes and upload copies
size_t fir_used(int L) { return offsetof(FirTaps, taps) + sizeof(float) * 16 * (size_t)((L + 3) & ~3); }

enum { FIR_DENSE1 = 0, FIR_DENSE = 1, FIR_WINDOW = 2 };

template <int MODE>
__device__ __forceinline__ int fir_slot(int m, int i, int step)
{
    if constexpr (MODE == FIR_WINDOW) return m * WIN_RS + i;
    const int p = m * step + i;
    if constexpr (MODE == FIR_DENSE) return p + (p >> 5);
    return p;
}

template <int MT, int MODE>
__global__ __launch_bounds__(256) void fir_bank_kernel(const FirTaps *__restrict__ plan, const float *__restrict__ x,
                                                       long long x_pitch, long long frames, long long first, long long step,
                                                       long long n_out, int L, int nk, int rectify, float *__restrict__ out,
                                                       long long out_pitch, long long out_kernel_pitch, int a_floats)
{
    extern __shared__ float fir_lds[];
    float *A = fir_lds;                         // the trace under this tile; reused by the epilogue
    float *B = fir_lds + a_floats;              // TAPS_KB x 16 taps
    constexpr int TM = 64 * MT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c = blockIdx.y;
    const long long tile0 = (long long)blockIdx.x * TM;
    const long long left = n_out - tile0;
    const int rows = left < TM ? (int)left : TM;           // outputs of this tile that exist
    const int L4 = (L + 3) & ~3;
    const int KA = MODE == FIR_WINDOW ? WIN_K : L4;       // tap slots per stage of the trace
    const int istep = (int)step;                           // dense layouts only: (TM-1)*step < DENSE_CAP
    // slot i of output m reads sample s0 + m*step + i
    const long long s0 = first + tile0 * step + (L - 1) / 2 - (L - 1);
    const float *xc = x + c * x_pitch;
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int mrow = wave * 16 * MT + (lane & 15), kq = lane >> 4;

    for (int ka = 0; ka < L4; ka += KA) {
        const int na = L4 - ka < KA ? L4 - ka : KA;
        if (ka > 0) __syncthreads();                       // the previous stage has been read
        if constexpr (MODE == FIR_WINDOW) {
            for (int idx = tid; idx < rows * WIN_K; idx += 256) {
                const int m = idx >> 5, i = idx & 31;
                const long long s = s0 + ka + (long long)m * step + i;
                if (i < na) A[m * WIN_RS + i] = (s >= 0 && s < frames) ? xc[s] : 0.0f;
            }
        } else {
            const int span = (rows - 1) * istep + na;
            for (int p = tid; p < span; p += 256) {
                const long long s = s0 + p;
                A[MODE == FIR_DENSE ? p + (p >> 5) : p] = (s >= 0 && s < frames) ? xc[s] : 0.0f;
            }
        }
        for (int kb = 0; kb < na; kb += TAPS_KB) {
            const int nb = na - kb < TAPS_KB ? na - kb : TAPS_KB;
            if (kb > 0) __syncthreads();
            for (int idx = tid; idx < nb * 16; idx += 256) B[idx] = plan->taps[(ka + kb) * 16 + idx];
            __syncthreads();
            // rows past `rows` read LDS nobody staged: their results are never stored, and a row of the MFMA only
            // depends on its own A row
            mb_walk(nb, [&](int k) {
                const float b = B[k * 16 + lane];
#pragma unroll
                for (int mt = 0; mt < MT; mt++) {
                    const float a = A[fir_slot<MODE>(mrow + 16 * mt, kb + k + kq, istep)];
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[mt], 0, 0, 0);
                }
            });
        }
    }
    __syncthreads();                                       // the trace has been read: the transpose takes its place
    const float *O = mb_transpose<MT>(A, acc, wave, lane);
    mb_store<MT>(O, lane, nk, tile0 + wave * 16 * MT, n_out, out + c * out_pitch, out_kernel_pitch,
                 [&](float v, int n, int, long long) {
                     if (!rectify) return v;
                     const float d = v - plan->threshold[n];
                     return (d > 0.0f || d != d) ? d : 0.0f;    // NaN stays NaN, as np.maximum
                 });
}

std::atomic<int> fir_raised[64];

int fir_raise_all(hipdsp_ctx *ctx)
{
    return mb_raise_lds(ctx, fir_raised,
                        {(const void *)fir_bank_kernel<4, FIR_DENSE1>, (const void *)fir_bank_kernel<4, FIR_DENSE>,
                         (const void *)fir_bank_kernel<2, FIR_DENSE>, (const void *)fir_bank_kernel<1, FIR_DENSE>,
                         (const void *)fir_bank_kernel<4, FIR_WINDOW>},
                        (DENSE_CAP + DENSE_CAP / 32 + 64 + TAPS_KB * 16) * (int)sizeof(float));
}

template <int MT, int MODE>
int fir_launch(hipdsp_ctx *ctx, const FirTaps *dev, const float *x, long long x_pitch, long long channels, long long frames,
               long long first, long long step, long long n_out, int L, int nk, int rectify, float *out, long long out_pitch,
               long long out_kernel_pitch, int a_floats)
{
    constexpr int TM = 64 * MT;
    const size_t lds = (size_t)(a_floats + TAPS_KB * 16) * sizeof(float);
    const dim3 grid((unsigned)((n_out + TM - 1) / TM), (unsigned)channels);
    hipLaunchKernelGGL((fir_bank_kernel<MT, MODE>), grid, dim3(256), lds, ctx->stream, dev, x, x_pitch, frames, first, step,
                       n_out, L, nk, rectify, out, out_pitch, out_kernel_pitch, a_floats);
    return hd_launch_status("fir_bank_kernel");
}

}  // namespace

struct hipdsp_firplan {
    hd_plan_stage stage;   // a FirTaps
    int n_kernels, n_taps; // of the last set_host
    int up_kernels, up_taps; // of the last upload (0 before the first): what the device block holds
};

extern "C" {

int hipdsp_firplan_create(hipdsp_ctx *ctx, hipdsp_firplan **out)
{
    HD_REQUIRE(ctx != nullptr && out != nullptr, "NULL argument");
    *out = nullptr;
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    hipdsp_firplan *p = new hipdsp_firplan();
    int rc = hd_stage_create(ctx, &p->stage, sizeof(FirTaps), true);   // uploads copy the used prefix only
    if (rc == HIPDSP_OK) rc = fir_raise_all(ctx);
    if (rc != HIPDSP_OK) {
        hd_stage_destroy(ctx, &p->stage);
        delete p;
        return rc;
    }
    *out = p;
    return HIPDSP_OK;
}

int hipdsp_firplan_destroy(hipdsp_ctx *ctx, hipdsp_firplan *plan)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    if (!plan) return HIPDSP_OK;
    hd_stage_destroy(ctx, &plan->stage);
    delete plan;
    return HIPDSP_OK;
}

int hipdsp_firplan_set_host(hipdsp_ctx *ctx, hipdsp_firplan *plan, const double *host_taps, int n_kernels, int n_taps,
                            const double *host_threshold)
{
    HD_REQUIRE(ctx != nullptr && plan != nullptr && host_taps != nullptr, "NULL argument");
    HD_REQUIRE(n_kernels >= 1 && n_taps >= 1, "n_kernels %d and n_taps %d must be positive", n_kernels, n_taps);
    if (n_kernels > MAX_KERNELS || n_taps > MAX_TAPS) {
        hipdsp_set_error("at most %d kernels of %d taps per plan, got %d of %d", MAX_KERNELS, MAX_TAPS, n_kernels, n_taps);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    const int rc = hd_stage_host_free(&plan->stage);
    if (rc != HIPDSP_OK) return rc;
    FirTaps *h = (FirTaps *)plan->stage.host;
    memset(h, 0, fir_used(n_taps > plan->n_taps ? n_taps : plan->n_taps));
    for (int n = 0; n < n_kernels; n++) {
        h->threshold[n] = host_threshold ? (float)host_threshold[n] : 0.0f;
        for (int i = 0; i < n_taps; i++) h->taps[i * 16 + n] = (float)host_taps[(size_t)n * n_taps + (n_taps - 1 - i)];
    }
    plan->n_kernels = n_kernels;
    plan->n_taps = n_taps;
    return HIPDSP_OK;
}

int hipdsp_firplan_upload(hipdsp_ctx *ctx, hipdsp_firplan *plan)
{
    HD_REQUIRE(ctx != nullptr && plan != nullptr, "NULL argument");
    HD_REQUIRE(plan->n_kernels > 0, "plan has no taps yet");
    const int rc = hd_stage_upload(ctx, &plan->stage, fir_used(plan->n_taps));
    if (rc != HIPDSP_OK) return rc;
    plan->up_kernels = plan->n_kernels;
    plan->up_taps = plan->n_taps;
    return HIPDSP_OK;
}

int hipdsp_firplan_set(hipdsp_ctx *ctx, hipdsp_firplan *plan, const double *host_taps, int n_kernels, int n_taps,
                       const double *host_threshold)
{
    int rc = hipdsp_firplan_set_host(ctx, plan, host_taps, n_kernels, n_taps, host_threshold);
    if (rc != HIPDSP_OK) return rc;
    return hipdsp_firplan_upload(ctx, plan);
}

int hipdsp_fir_bank(hipdsp_ctx *ctx, const hipdsp_firplan *plan, const float *x, int64_t x_pitch, int64_t channels,
                    int64_t frames, int64_t first, int64_t step, int64_t n_out, int rectify, float *out, int64_t out_pitch,
                    int64_t out_kernel_pitch)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(plan != nullptr, "plan is NULL");
    HD_REQUIRE(plan->n_kernels > 0, "plan has no taps yet");
    HD_REQUIRE(plan->up_kernels == plan->n_kernels && plan->up_taps == plan->n_taps,
               "the plan's %d kernels of %d taps have not been uploaded (the device holds %d of %d)", plan->n_kernels,
               plan->n_taps, plan->up_kernels, plan->up_taps);
    HD_REQUIRE(channels >= 0 && frames >= 0 && n_out >= 0, "negative size");
    HD_REQUIRE(first >= 0, "first %lld is negative", (long long)first);
    HD_REQUIRE(step >= 1, "step %lld must be at least 1", (long long)step);
    const int L = plan->n_taps, nk = plan->n_kernels;
    if (x_pitch == 0) x_pitch = frames;
    HD_REQUIRE(x_pitch >= frames, "x_pitch smaller than frames");
    bool empty;
    int rc = mb_check_out("kernel", x, frames, channels, n_out, out, &out_pitch, &out_kernel_pitch, &empty);
    if (rc != HIPDSP_OK || empty) return rc;
    HD_REQUIRE(first <= (1LL << 60) && n_out <= ((1LL << 60) - first) / step, "first + n_out*step out of range");
    HD_REQUIRE(frames == 0 || !mb_out_overlaps(x, (channels - 1) * x_pitch + frames, out, nk, out_kernel_pitch, channels,
                                               out_pitch, n_out), "x and out must not overlap");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    rc = fir_raise_all(ctx);
    if (rc != HIPDSP_OK) return rc;
    const int L4 = (L + 3) & ~3;
    const FirTaps *dev = (const FirTaps *)plan->stage.dev;
#define FIR_GO(MT, MODE, AF)                                                                                            \
    return fir_launch<MT, MODE>(ctx, dev, x, x_pitch, channels, frames, first, step, n_out, L, nk, rectify ? 1 : 0, out, \
                                out_pitch, out_kernel_pitch, (AF))
    if (step == 1) FIR_GO(4, FIR_DENSE1, 255 + L4 > OUT_FLOATS ? 255 + L4 : OUT_FLOATS);
    for (int mt = 4; mt >= 1; mt >>= 1) {
        const long long span = (64LL * mt - 1) * step + L4;
        if (span > DENSE_CAP) continue;
        int af = (int)(span + (span >> 5) + 1);
        if (af < OUT_FLOATS) af = OUT_FLOATS;
        if (mt == 4) FIR_GO(4, FIR_DENSE, af);
        if (mt == 2) FIR_GO(2, FIR_DENSE, af);
        FIR_GO(1, FIR_DENSE, af);
    }
    FIR_GO(4, FIR_WINDOW, 256 * WIN_RS);
#undef FIR_GO
}

}  // extern "C"
