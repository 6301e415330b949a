// mfma_bank.h -- what the two "bank" kernels on the f32 matrix core share: fir_bank_kernel (firbank.hip, a bank of FIR
// kernels over traces) and template_match_kernel (templatematch.hip, a bank of templates over a spectrogram slab).
// Both are GEMMs whose A matrix is read out of a staged LDS tile, with v_mfma_f32_16x16x4_f32:
//     M = 16 outputs (times, window starts), N = 16 bank members (kernels, templates), K = 4 tap slots per step;
//     lane l holds A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; the plans keep the taps as (slot, member)
//     rows of 16 floats in the order the slots are walked, so a step's B fragment is 64 consecutive floats;
//     a workgroup of four waves, MT accumulators of 16 outputs per wave that share each B fragment.
// Here: the walk over the tap slots, the transpose of the accumulators through LDS and the store loop behind it, the
// raising of the dynamic LDS limit, and the host checks of the output block.  How the tile is staged and laid out, the
// epilogue's arithmetic and the dispatch are each kernel's own.  Everything sits in an anonymous namespace.
#pragma once
#include "common.h"
#include <atomic>
#include <initializer_list>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TAPS_KB = 128;                  // tap slots per B stage (8 KB)
constexpr int OUT_FLOATS = 4 * 16 * 72;       // the transpose of a workgroup, MT = 4

// The steps k = 0, 4, ... < n (n a multiple of 4) in ascending order, four steps' LDS reads in flight.  The order is
// the order of the fmaf chain behind an output: it must not depend on anything but n.
template <class Step>
__device__ __forceinline__ void mb_walk(int n, const Step &step)
{
    int k = 0;
    for (; k + 16 <= n; k += 16) {
        step(k); step(k + 4); step(k + 8); step(k + 12);
    }
    for (; k < n; k += 4) step(k);
}

// C layout: member n = lane & 15, output = 4*(lane >> 4) + r of accumulator mt.  Transposed per wave: row n of O[wave]
// holds the wave's 16*MT outputs from column n >> 2 on, rows ORS = 8 (mod 32) floats apart: the 32 lanes a ds_write_b32
// serves at once (16 members x 2 values of lane >> 4) fall on the banks 8*(n & 3) + 4*(lane >> 4) + (n >> 2) (+ r +
// 16*mt) mod 32, each once; the reads walk a row.
template <int MT>
constexpr int mb_ors = MT == 4 ? 72 : 40;

// the tile has been read by every wave (the caller's barrier) -> O[wave] of this wave, behind a barrier
template <int MT>
__device__ __forceinline__ float *mb_transpose(float *tile, const f32x4 (&acc)[MT], int wave, int lane)
{
    constexpr int ORS = mb_ors<MT>;
    float *O = tile + wave * 16 * ORS;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) O[(lane & 15) * ORS + ((lane & 15) >> 2) + mt * 16 + 4 * (lane >> 4) + r] = acc[mt][r];
    __syncthreads();
    return O;
}

// out[n * pitch + i0 + tl] = value(G, n, tl, i0 + tl) for the members n < nk and the wave's outputs tl with
// i0 + tl < n_out, G the accumulated product: a member's row is stored along the outputs
template <int MT, class Value>
__device__ __forceinline__ void mb_store(const float *O, int lane, int nk, long long i0, long long n_out, float *out,
                                         long long pitch, const Value &value)
{
    constexpr int OT = 16 * MT, ORS = mb_ors<MT>;
    for (int idx = lane; idx < nk * OT; idx += 64) {
        const int n = idx / OT, tl = idx % OT;
        const long long i = i0 + tl;
        if (i < n_out) out[n * pitch + i] = value(O[n * ORS + (n >> 2) + tl], n, tl, i);
    }
}

// More than 64 KB of dynamic LDS has to be asked for, per kernel: done for all of a unit's instantiations when a
// device's first plan is created (and checked again at every call), so that no launch ever does it inside a capture.
// `raised`: the unit's flag per device index.
inline int mb_raise_lds(hipdsp_ctx *ctx, std::atomic<int> (&raised)[64], std::initializer_list<const void *> kernels, int bytes)
{
    std::atomic<int> &done = raised[ctx->device & 63];
    if (done.load(std::memory_order_acquire)) return HIPDSP_OK;
    for (const void *k : kernels) HD_CHECK_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.store(1, std::memory_order_release);
    return HIPDSP_OK;
}

// The output block of a call: n_out outputs per channel and member, channels `*out_pitch` apart (0: n_out), members
// `*bank_pitch` apart (0: channels * out_pitch).  `noun` names a member in the messages.  *empty: nothing to compute.
inline int mb_check_out(const char *noun, const void *in, long long frames, long long channels, long long n_out,
                        const float *out, int64_t *out_pitch, int64_t *bank_pitch, bool *empty)
{
    *empty = true;
    if (*out_pitch == 0) *out_pitch = n_out;
    if (*bank_pitch == 0) *bank_pitch = channels * *out_pitch;
    HD_REQUIRE(*out_pitch >= n_out, "out_pitch smaller than n_out");
    if (n_out == 0 || channels == 0) return HIPDSP_OK;
    HD_REQUIRE(*bank_pitch >= (channels - 1) * *out_pitch + n_out, "out_%s_pitch smaller than one %s's block", noun, noun);
    HD_REQUIRE(out != nullptr && (in != nullptr || frames == 0), "NULL data pointer");
    HD_REQUIRE(channels <= 65535 && n_out <= (1LL << 36), "too many channels or outputs for one call");
    *empty = false;
    return HIPDSP_OK;
}

// does that block, of nk members, share memory with the in_floats floats at `in`?
inline bool mb_out_overlaps(const float *in, long long in_floats, const float *out, int nk, long long bank_pitch,
                            long long channels, long long out_pitch, long long n_out)
{
    return hd_bytes_overlap(in, 4 * in_floats, out, 4 * ((nk - 1) * bank_pitch + (channels - 1) * out_pitch + n_out));
}

}  // namespace
