/*
 * hip_dsp.h -- C ABI of libhip_dsp.so: MI355X (gfx950) kernels for audian's
 * BufferedData DSP hot path.
 *
 * The reference (bendalab/audian) is pure Python and has no FFI of its own; each
 * entry point below names the reference call (file:line under /root/reference)
 * whose arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no exceptions across the boundary.
 *   - Every call returns an int status (HIPDSP_OK == 0); hipdsp_last_error()
 *     returns a thread-local message for the last failing call.
 *   - All data pointers are DEVICE pointers unless the name says "host"; buffers
 *     are caller-owned.  Work is enqueued on the context's HIP stream and is
 *     asynchronous; hipdsp_ctx_synchronize() waits for it.
 *   - Device-native layout is planar float32: a trace is (channels, frames) with
 *     a row pitch in elements; a spectrogram is (channels, frames', F) compact.
 *     The reference's layouts are time-major float64 (T, C) / (T', C, F)
 *     (src/audian/buffereddata.py:46-48,70); the pack/unpack entry points convert
 *     at the edge.
 *   - IIR coefficients and state are float64 (mandatory); HBM I/O is
 *     float32.
 */
#ifndef HIP_DSP_H
#define HIP_DSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPDSP_VERSION 102          /* 0.1.2 */

#define HIPDSP_OK               0
#define HIPDSP_ERR_INVALID      1   /* bad argument */
#define HIPDSP_ERR_HIP          2   /* HIP runtime failure (message has detail) */
#define HIPDSP_ERR_UNSUPPORTED  3   /* valid in the reference, not implemented here */
#define HIPDSP_ERR_TOO_SHORT    4   /* sosfiltfilt: frames <= padlen (scipy: ValueError) */
#define HIPDSP_ERR_NOMEM        5

#define HIPDSP_MAX_SECTIONS     4   /* second-order sections per plan (cascade longer ones) */

typedef struct hipdsp_ctx hipdsp_ctx;
typedef struct hipdsp_sosplan hipdsp_sosplan;
typedef struct hipdsp_firplan hipdsp_firplan;

/* ---- library / context ------------------------------------------------- */

int hipdsp_version(void);
const char *hipdsp_last_error(void);
int hipdsp_device_count(int *count);

/* `stream` is a hipStream_t (NULL = the legacy default stream). */
int hipdsp_ctx_create(int device, void *stream, hipdsp_ctx **out);
int hipdsp_ctx_destroy(hipdsp_ctx *ctx);
int hipdsp_ctx_set_stream(hipdsp_ctx *ctx, void *stream);
int hipdsp_ctx_synchronize(hipdsp_ctx *ctx);
/* Tuning knob: upper bound on time segments per channel of the block-parallel
 * IIR (0 = automatic).  Results do not depend on it beyond fp64 rounding. */
int hipdsp_ctx_set_max_segments(hipdsp_ctx *ctx, int max_segments);
/* Named tuning/testing options (results do not depend on them beyond rounding):
 *   "max_segments"       as hipdsp_ctx_set_max_segments
 *   "sos_waves_per_cu"   most resident waves per CU the IIR segment planner uses (16; see hipdsp_sos_segments_host);
 *                        "sos_waves_min" >= that: exactly that many (experiments); "chain_pairs" (8): most pairs of
 *                        waves per CU of the fused sweeps
 *   "pool_limit_mb"      bytes (MiB) hipdsp_free may keep cached for hipdsp_malloc (1024); blocks of up to 256 MiB are
 *                        cached, with a larger limit blocks of up to the limit
 *   "sos_prefetch"       0: envelope sweeps without the register prefetch of the next tile (1)
 *   "chain_split_frames" non-zero: hipdsp_chain_forward (2048/1024, no db_out) leaves the odd frames to hipdsp_chain_backward
 *   "chain_reserve_cus"  CUs hipdsp_chain_forward plans no workgroup for (0): its 1024-thread workgroups want a
 *                        whole CU each, so a kernel that stays resident next to it (RCCL's all-gather in the
 *                        multi-GPU step) needs CUs of its own or a second round of workgroups forms
 *   "force_generic_fft"  non-zero: every nfft takes the generic radix-2 / four-step kernels
 *   "spec_kernel"        cross-check paths (results equal within the parity bar): 0 = default per size, 2 = the kernel a
 *                        size's default replaced (two-stage FFT, workgroup per frame, four-step path through HBM), 3 = the
 *                        other of a size's two candidates (nfft 256, 512: one frame per lane group instead of the stream
 *                        through LDS; 1024: the stream for every hop; 4096: one wave per frame); tools/spec_kernel_ab.py
 *   "spec_fpw"           consecutive frames per wave (0 = automatic)
 *   "spec_no_half"       non-zero: do not reuse the overlapped half frame at 50 % overlap
 *   "chain_debug"        measurements only (results become wrong): 1 = the FFT waves of
 *                        hipdsp_chain_forward only copy their tiles, 2 = its IIR waves skip the cascades;
 *                        4 (results unchanged) = workgroup barriers instead of pairwise LDS flags;
 *                        8 = one FFT wave withholds one hand-over (test of the fault report below);
 *                        16 = clock counters of one wave into the first 16 bytes of the PSD;
 *                        32 = diagnostic build: db_out receives 16 clock sums per wave (tools/chain_stamps.py);
 *                        64 = no issue priorities at all; 128 (results unchanged) = FFT waves above IIR waves
 *                        only, without the progress words that keep the waves of a SIMD in step
 *   "scratch_fill"       testing only (0 = off, the default): v in 1 ... 256 fills the context's whole scratch with
 *                        byte v - 1 every time a call asks for it, and the segment flags of the IIR sweeps likewise,
 *                        by one stream-ordered memset before the call's kernels (never the tile states a forward sweep
 *                        parked for its backward sweep, and not while the stream is capturing).  Results must not
 *                        depend on it at all, not even in rounding: what a call reads from the scratch it has written
 * Any other name is refused with HIPDSP_ERR_INVALID, the retired experiment switches of the envelope's backward sweep
 * and of the short-window spectrogram kernel included ("sos_split", "sos_single_wave_wg", "sos_no_pin", "sos_trace",
 * "sos_trace_rows", "sos_fair", "sos_debug", "spec_debug"; their verdicts: DESIGN.md, "Retired experiments").
 * Device-side faults: the waits between the waves of hipdsp_chain_forward's kernel are bounded; a wave
 * whose wait runs out writes a fault word owned by the context and ends the launch early.
 * hipdsp_ctx_synchronize, hipdsp_memcpy_d2h, hipdsp_event_elapsed_ms and the next
 * hipdsp_chain_forward / hipdsp_sosfilt_envelope on the context then return HIPDSP_ERR_HIP (once,
 * with a message): no path returns HIPDSP_OK for a launch that gave up. */
int hipdsp_ctx_set_option(hipdsp_ctx *ctx, const char *name, long long value);
/* Pre-size the internal scratch (envelope state checkpoints: 16 * n_sections bytes per
 * 2048-sample tile and channel, for ceil((frames + padlen) / 2048) + 1 tiles; four-step FFT work area) so that later calls do not
 * allocate; required before stream capture into a hipGraph.  While a graph captured on the context
 * is alive the scratch cannot grow (the graph holds its address): a call that would need more returns
 * HIPDSP_ERR_INVALID -- reserve the largest size before capturing. */
int hipdsp_ctx_reserve(hipdsp_ctx *ctx, size_t bytes);

/* ---- streams and hipGraph capture (interactive recompute, BASELINE configs[4]) ---- */

/* A non-blocking HIP stream owned by the library (stream capture cannot run on the
 * legacy default stream).  Pass it to hipdsp_ctx_set_stream. */
int hipdsp_stream_create(hipdsp_ctx *ctx, void **stream);
int hipdsp_stream_destroy(hipdsp_ctx *ctx, void *stream);

/* Capture everything enqueued on the context's stream between _begin and _end into an
 * executable graph; hipdsp_graph_launch replays it on the context's stream.  Run each
 * call once before capturing (FFT tables, scratch: hipdsp_ctx_reserve) -- nothing may
 * allocate during capture.  Filter cut-offs change between replays through
 * hipdsp_sosplan_set_host + a captured hipdsp_sosplan_upload (DataBrowser.update_filter
 * -> BufferedFilter.update -> recompute_all, databrowser.py:1264-1288).  The time segmentation and the
 * number of warm-up tiles are those of the plans AT CAPTURE TIME (the state hand-over between segments
 * is recomputed on the device from the plan it finds): capture with the slowest-decaying filters of the
 * sweep -- lowest high-pass and lowest envelope cut-off -- or a replay with a longer memory than the
 * captured warm-up starts its segments with a history that has not fully decayed. */
typedef struct hipdsp_graph hipdsp_graph;
int hipdsp_graph_begin(hipdsp_ctx *ctx);
int hipdsp_graph_end(hipdsp_ctx *ctx, hipdsp_graph **out);
int hipdsp_graph_launch(hipdsp_ctx *ctx, hipdsp_graph *graph);
int hipdsp_graph_destroy(hipdsp_ctx *ctx, hipdsp_graph *graph);

/* ---- device memory helpers (so a non-torch host can keep stages resident) */

/* hipdsp_free keeps blocks of up to 256 MiB (or "pool_limit_mb", if that is larger) in a per-context cache (at most "pool_limit_mb",
 * default 1024; 0 turns it off) and hipdsp_malloc hands them out again, because hipMalloc /
 * hipFree synchronise the device and an interactive redraw needs temporaries.  The cache is
 * stream-ordered: free a block through a context whose stream is behind all work on it (order
 * other contexts' streams with hipdsp_event_record / hipdsp_event_wait first).  A cached block
 * remembers the stream it was freed on: handed out again after hipdsp_ctx_set_stream, the new
 * stream first waits for an event recorded at the free. */
int hipdsp_malloc(hipdsp_ctx *ctx, size_t bytes, void **dptr);
int hipdsp_free(hipdsp_ctx *ctx, void *dptr);
/* A block for a trace that kernels WRITE (the buffers BufferedData.allocate_buffer creates, src/audian/buffereddata.py:69-70,
 * 112-114): up to `tries` (<= 8) blocks are allocated side by side, a memset over each is timed on the context's stream
 * (which is synchronised), the fastest stays, the others go back through hipdsp_free.  Which physical pages a block got
 * moves a write stream into it by up to 12 % on this part (the envelope's backward sweep: 5.5 ... 6.2 ms into blocks of
 * one process, and the memset predicts it); nothing in user space chooses them, but it can choose among them.  Blocks
 * under 64 MiB, tries <= 1 and calls inside a stream capture are plain hipdsp_malloc calls.  The block is zeroed. */
int hipdsp_malloc_probed(hipdsp_ctx *ctx, size_t bytes, int tries, void **dptr);
/* Cache statistics (any pointer may be NULL) / give every cached block back to the driver -- and the context's scratch,
 * which only grows otherwise (hipdsp_envelope_multi parks two slabs of the trace's size there), unless a captured graph
 * of the context is alive (it holds the scratch's address). */
int hipdsp_pool_stats(hipdsp_ctx *ctx, size_t *cached_bytes, uint64_t *hits, uint64_t *misses);
int hipdsp_pool_trim(hipdsp_ctx *ctx);
int hipdsp_memset(hipdsp_ctx *ctx, void *dptr, int value, size_t bytes);
int hipdsp_memcpy_h2d(hipdsp_ctx *ctx, void *dst, const void *host_src, size_t bytes);
int hipdsp_memcpy_d2h(hipdsp_ctx *ctx, void *host_dst, const void *src, size_t bytes);
int hipdsp_memcpy_d2d(hipdsp_ctx *ctx, void *dst, const void *src, size_t bytes);
/* Page-locked host staging (CompressedData's block reader, audian_amd/compresseddata.py): _host_malloc returns
 * `bytes` of pinned host memory (hipHostMalloc; the context names the device), _host_free gives it back.  Unlike
 * hipdsp_memcpy_h2d, hipdsp_memcpy_h2d_async does NOT wait: the copy is ordered on the context's stream and
 * `host_src` must be page-locked (from hipdsp_host_malloc) and left untouched until the stream has passed the
 * copy (hipdsp_event_record + a wait, or hipdsp_ctx_synchronize). */
int hipdsp_host_malloc(hipdsp_ctx *ctx, size_t bytes, void **host_ptr);
int hipdsp_host_free(hipdsp_ctx *ctx, void *host_ptr);
int hipdsp_memcpy_h2d_async(hipdsp_ctx *ctx, void *dst, const void *host_src, size_t bytes);
/* `height` rows of `width` bytes between pitched device blocks (ring-buffer recycling
 * of the device mirror, buffereddata.py:87). */
int hipdsp_memcpy2d_d2d(hipdsp_ctx *ctx, void *dst, size_t dst_pitch, const void *src,
                        size_t src_pitch, size_t width, size_t height);

/* HIP events on the context's stream (bench.py times kernels with these). */
int hipdsp_event_create(hipdsp_ctx *ctx, void **event);
int hipdsp_event_destroy(hipdsp_ctx *ctx, void *event);
int hipdsp_event_record(hipdsp_ctx *ctx, void *event);
/* Work queued on the context's stream after this call waits for `event` (recorded on any stream
 * of the device): orders two contexts that run on streams of their own. */
int hipdsp_event_wait(hipdsp_ctx *ctx, void *event);
int hipdsp_event_elapsed_ms(hipdsp_ctx *ctx, void *start, void *stop, float *ms);

/* Profiling hook: when set (non-NULL), hipdsp_envelope records this event between
 * its forward and backward kernels, so a bench can time the two separately. */
int hipdsp_ctx_set_mid_event(hipdsp_ctx *ctx, void *event);

/* ---- layout conversion at the edge -------------------------------------- */

/* (T, C) interleaved float64 / float32 -> planar (C, dst_pitch) float32.
 * Replaces the implicit layout of BufferedArray buffers (buffereddata.py:70). */
int hipdsp_pack_f64(hipdsp_ctx *ctx, const double *src_tc, float *dst, int64_t dst_pitch,
                    int64_t frames, int64_t channels);
int hipdsp_pack_f32(hipdsp_ctx *ctx, const float *src_tc, float *dst, int64_t dst_pitch,
                    int64_t frames, int64_t channels);
/* planar (C, src_pitch) float32 -> (T, C) interleaved float64. */
int hipdsp_unpack_f64(hipdsp_ctx *ctx, const float *src, int64_t src_pitch, double *dst_tc,
                      int64_t frames, int64_t channels);
/* (C, T', F) float32 -> (T', C, F) float64: the reference's
 * Sxx.transpose((1, 2, 0)) (bufferedspectrogram.py:58).  src_pitch = elements
 * between consecutive channels of src (>= frames*nfreq). */
int hipdsp_unpack_spectrum_f64(hipdsp_ctx *ctx, const float *src, int64_t src_pitch,
                               double *dst_tcf, int64_t frames, int64_t channels,
                               int64_t nfreq);

/* ---- IIR filter plans ---------------------------------------------------- */

/* A plan holds, in device memory, everything the block-parallel biquad cascade
 * needs for one SOS table: coefficients, block transition matrices, steady-state
 * initial conditions (scipy sosfilt_zi) and the warm-up length.  Updating a plan
 * (hipdsp_sosplan_set) is an async copy on the stream, so a captured hipGraph
 * replays under new cut-offs. */
int hipdsp_sosplan_create(hipdsp_ctx *ctx, hipdsp_sosplan **out);
int hipdsp_sosplan_destroy(hipdsp_ctx *ctx, hipdsp_sosplan *plan);
/* host_sos: (n_sections, 6) float64 rows [b0 b1 b2 a0 a1 a2], a0 == 1, exactly
 * what scipy.signal.butter(..., output='sos') returns
 * (bufferedfilter.py:44-52, bufferedenvelope.py:47-52). */
int hipdsp_sosplan_set(hipdsp_ctx *ctx, hipdsp_sosplan *plan, const double *host_sos,
                       int n_sections);
/* The two halves of hipdsp_sosplan_set, for hipGraph use: _set_host computes the
 * plan into pinned host memory (no stream work); _upload enqueues the copy to the
 * device block and may be captured, so each replay picks up the latest _set_host. */
int hipdsp_sosplan_set_host(hipdsp_ctx *ctx, hipdsp_sosplan *plan, const double *host_sos,
                            int n_sections);
int hipdsp_sosplan_upload(hipdsp_ctx *ctx, hipdsp_sosplan *plan);
/* The host half of a plan without any device: warm-up length (smallest multiple of the
 * 2048-sample tile with ||A^warm||_inf < 2^-60; 2^50 tiles when the filter does not decay),
 * scipy's sosfiltfilt pad length and sosfilt_zi (2*n_sections values); any output may be NULL. */
int hipdsp_sos_plan_host(const double *host_sos, int n_sections, int64_t *warmup, int *edge,
                         double *zi);
/* How the block-parallel IIR cuts `frames` samples of `channels` channels into time segments
 * (one wave per channel and segment) on `n_cus` compute units that hold up to `waves_max` such
 * waves each ("sos_waves_per_cu", 16; the fused sweeps: 8 pairs), when a segment has to re-read
 * `warmup` samples before its range.  The count minimises
 *     rounds x (segment + warm-up) x cost of a tile step at w waves per CU
 * (rounds of n_cus x waves_max units when there are more).  per_simd selects the sweep's measured cost table:
 * 4 (the envelope's backward sweep, four SIMDs per CU): memory-bound from two waves per SIMD on, so a tile step
 * costs ceil(w / 4) / 2, and 0.65 at one wave per SIMD (profiles/r03_occupancy_sweep.log): 8 waves per CU are
 * preferred to 16, short jobs get 4.  0 (the fused sweeps): waves_max x (1 + 0.25 (1 - w / waves_max)) -- the
 * CU is filled whenever the job allows.  -1 (the band-pass alone, no prefetch): 7 + 0.5625 w, and -2 (band-pass +
 * envelope states, prefetching): 1.4 + 0.9125 w (profiles/r03_sos_waves.log) -- both fill the CU for long jobs.
 * segment_frames is a multiple of the 2048-sample tile.
 * Host only (tests, capacity planning). */
int hipdsp_sos_segments_host(int64_t n_cus, int waves_max, int per_simd, int max_segments, int64_t frames,
                             int64_t channels, int64_t warmup, int64_t *segment_frames,
                             int *n_segments);
/* Introspection (tests): warm-up length in samples, sosfiltfilt pad length. */
int hipdsp_sosplan_info(hipdsp_ctx *ctx, hipdsp_sosplan *plan, int64_t *warmup, int *edge);

/* ---- the hot path --------------------------------------------------------- */

/* Non-finite samples (NaN, +-Inf) in x, every entry point below: as in the reference, i.e. as scipy does -- the
 * filtered trace of that channel is NaN from the sample on TO THE END of the call's slab (sosfilt's state stays
 * NaN), every spectrogram frame that reaches that far is NaN in every bin (dB: NaN), the envelope of that channel
 * is NaN everywhere (sosfiltfilt's backward pass starts from the NaN end); other channels are not affected.  The
 * time segments a sweep is cut into do not show (csrc/sos_device.h: FloodArgs). */

/* Input and output of a sweep must not overlap (HIPDSP_ERR_INVALID): a sweep is cut into time segments that run
 * concurrently and re-read their warm-up from the input -- the reference never filters in place either
 * (dest is a view of the trace's own ring buffer).  hipdsp_envelope_multi copies its input first and may. */

/* BufferedFilter.process (bufferedfilter.py:31-36):
 *   y[c, :] = sosfilt(sos, x[c, :])[skip:]      zero initial state, per channel.
 * x: (channels, x_pitch) with `frames` valid samples; y: (channels, y_pitch) with
 * frames - skip valid samples.  plan == NULL copies x[skip:] (the sos-is-None
 * pass-through branch, bufferedfilter.py:32-33). */
int hipdsp_sosfilt(hipdsp_ctx *ctx, const hipdsp_sosplan *plan, const float *x,
                   int64_t x_pitch, float *y, int64_t y_pitch, int64_t channels,
                   int64_t frames, int64_t skip);

/* BufferedEnvelope.process (bufferedenvelope.py:34-41):
 *   y = sosfiltfilt(sos, gain*|x|, axis=0)[skip:]; if clamp: y[y < 0] = 0
 * with scipy's default odd padding of 3*ntaps samples, sosfilt_zi-scaled initial
 * conditions, forward then backward pass.  `rectify` != 0 applies gain*|x|
 * (gain = pi/2 in the reference), rectify == 0 filters x itself (plain
 * sosfiltfilt, e.g. the playback chain databrowser.py:1718-1729).
 * Returns HIPDSP_ERR_TOO_SHORT when frames <= padlen (scipy raises ValueError).
 * plan == NULL writes zeros (bufferedenvelope.py:35-36). */
int hipdsp_envelope(hipdsp_ctx *ctx, const hipdsp_sosplan *plan, const float *x,
                    int64_t x_pitch, float *y, int64_t y_pitch, int64_t channels,
                    int64_t frames, int64_t skip, int rectify, double gain, int clamp);

/* Batch form of the two calls above for a whole slab (the envelope is taken of the SAME
 * frames the filter produces, skip = 0):
 *   yf  = sosfilt(fplan, x)                          (BufferedFilter.process)
 *   env = sosfiltfilt(eplan, gain*|yf|) [clamped]    (BufferedEnvelope.process on yf)
 * One sweep over x writes yf and, instead of the forward output of sosfiltfilt, only the
 * envelope cascade's state at every 2048-sample tile border (context scratch); the backward
 * sweep re-reads yf, recomputes the forward output tile by tile from those states and filters
 * it backwards: 8 + 8 bytes per sample instead of 8 + 16.  Results equal the two separate calls
 * up to float64 rounding of the IIR state.
 * phase: 0 = both sweeps; 1 = forward sweep only (yf complete, states parked in the context
 * scratch); 2 = backward sweep only (env from yf and those states) -- so that other work on yf
 * (the spectrogram) can be enqueued in between; no call that uses the scratch of THIS context
 * (envelope, envelope_multi, nfft > 32768, mean_spectrum_db) may come between phase 1 and phase 2.
 * env_first: the envelope is taken of yf[env_first:] -- env rows hold frames - env_first samples, env[i] belongs
 * to sample env_first + i of yf -- which is what BufferedEnvelope's buffer is after a scroll (its second of
 * pre-roll trimmed by BufferedData.align_buffer, buffereddata.py:75-88; sosfiltfilt then pads and starts at that
 * sample).  Phase 2 must be given the env_first of the forward sweep whose tile states it consumes (phase 1 or
 * hipdsp_chain_forward; HIPDSP_ERR_INVALID otherwise).  HIPDSP_ERR_TOO_SHORT when frames - env_first <= padlen. */
int hipdsp_sosfilt_envelope(hipdsp_ctx *ctx, const hipdsp_sosplan *fplan,
                            const hipdsp_sosplan *eplan, const float *x, int64_t x_pitch,
                            float *yf, int64_t yf_pitch, float *env, int64_t env_pitch,
                            int64_t channels, int64_t frames, int rectify, double gain, int clamp,
                            int phase, int64_t env_first);

/* BufferedEnvelope.process for cascades LONGER than HIPDSP_MAX_SECTIONS (the reference accepts any
 * filter_order: bufferedenvelope.py:13-16,44-55; a band-pass envelope of order >= 5 or a low-pass of
 * order >= 9 has more than four sections): the SOS table is split over `n_plans` plans (in cascade order,
 * each <= HIPDSP_MAX_SECTIONS sections) and scipy's sosfiltfilt (scipy/signal/_signaltools.py:4807-4828) is
 * run step by step -- odd extension by padlen of the WHOLE cascade, forward pass from zi * ext[0], time
 * reversal, forward pass from zi * y[-1], reversal and trim -- where every plan starts from its own
 * sosfilt_zi scaled by the DC gain of the sections in front of it, exactly as sosfilt_zi of the whole table
 * would give.  The hand-over between plans is float32.  Same arguments and errors as hipdsp_envelope
 * (HIPDSP_ERR_TOO_SHORT when frames <= padlen); 56 instead of 16 bytes per sample, two temporaries of
 * (channels, frames + 2 padlen) floats in the context's scratch (which grows to hold them once and keeps its size
 * until hipdsp_pool_trim(): like every call that uses the scratch, not between hipdsp_sosfilt_envelope's phases 1
 * and 2 -- a backward sweep behind it returns HIPDSP_ERR_INVALID, the tile states are gone). */
int hipdsp_envelope_multi(hipdsp_ctx *ctx, const hipdsp_sosplan *const *plans, int n_plans, const float *x,
                          int64_t x_pitch, float *y, int64_t y_pitch, int64_t channels, int64_t frames,
                          int64_t skip, int rectify, double gain, int clamp);

/* The forward half of the batch chain in ONE pass over x: BufferedFilter.process
 * (bufferedfilter.py:31-36) writes yf, the envelope's forward sweep parks its tile states in the
 * context scratch exactly like hipdsp_sosfilt_envelope(..., phase = 1), and
 * BufferedSpectrogram.process (bufferedspectrogram.py:45-59) of yf goes to psd -- the spectrogram
 * takes the filtered tiles from on-chip memory instead of reading yf back (12 instead of 16 bytes
 * per sample).  Follow with hipdsp_sosfilt_envelope(..., phase = 2) for the envelope.  Results
 * equal hipdsp_sosfilt_envelope(phase 1) + hipdsp_spectrogram up to float32 rounding of the
 * frames that straddle an internal segment border.
 * Covers the window lengths whose frames are register windows of the sweep's 2048-sample tiles -- nfft / hop
 * 2048/1024, 2048/512, 1024/512, 1024/256, 512/256 and 256/128 (the reference's overlap selector offers 50 % and 75 %,
 * databrowser.py:516-540; BASELINE configs[1] is 1024/256; 256/128 is BufferedSpectrogram's default,
 * bufferedspectrogram.py:14-16) -- band-pass plans of up to four and envelope
 * plans of up to two decaying sections, and frames >= 8192; anything else returns HIPDSP_ERR_UNSUPPORTED
 * (use the separate calls).  psd layout, the zero tail and the optional db_out (decibel(psd), fused epilogue:
 * what SpecItem.update_plot shows, specitem.py:36) as in hipdsp_spectrogram, for every window of the list.
 * eplan == NULL: no envelope behind the filter (the reference's default trace set is filter + spectrogram,
 * src/audian/plugins.py:11-13) -- band-pass and spectrogram only, nothing is parked in the scratch.
 * spec_frames: the spectrogram is handed only the first spec_frames samples of yf (0 = all `frames`): through
 * BufferedData.load_buffer (buffereddata.py:91-109) BufferedSpectrogram.process sees its own frames times hop
 * plus ONE sample of the filtered buffer, so its last frame(s) are zero although the filter has the samples;
 * this is what lets one launch serve BufferedFilter.recompute_all() (buffereddata.py:149-153).
 * spec_first, env_first: where the derived traces start inside the filtered buffer once the user has scrolled
 * (DataBrowser.set_times -> Data.update_times -> align_buffer, buffereddata.py:75-88, data.py:225-236): the filtered
 * buffer then starts at an arbitrary sample of the recording, the spectrogram's frame 0 at the next multiple of hop
 * -- sample spec_first = ceil(offset / hop) hop - offset of yf, frame k = yf[spec_first + k hop : + nfft], and
 * spec_frames counts from there -- and the envelope is taken of yf[env_first:] only (its one second of pre-roll is
 * trimmed: sosfiltfilt's odd extension and zi * ext[0] sit at sample env_first; the tile states parked for
 * hipdsp_sosfilt_envelope(..., phase = 2, env_first) belong to that envelope).  Any 0 <= spec_first, env_first <=
 * frames; the sweep shifts its tile grid (by less than one tile of zeros in front of the trace) so that frames stay
 * register windows of its tiles, and the tile the envelope starts in holds the odd extension in front of sample
 * env_first and the extension's first value in front of that, for which zi * value is the cascade's steady state.
 * The sweep counts tiles and frames in 32 bits: frames_out < 2^31 - 65536 (HIPDSP_ERR_INVALID beyond; a spectrogram of
 * that many frames is terabytes).  The spectrogram's frame means come from the band-pass's own float64 arithmetic (the
 * reference's float64 mean, detrend='constant'), not from a float32 sum. */
int hipdsp_chain_forward(hipdsp_ctx *ctx, const hipdsp_sosplan *fplan,
                         const hipdsp_sosplan *eplan, const float *x, int64_t x_pitch, float *yf,
                         int64_t yf_pitch, int64_t channels, int64_t frames, int rectify,
                         double gain, int nfft, int hop, double fs, float *psd, float *db_out,
                         int64_t frames_out, int64_t psd_pitch, int64_t spec_frames, int64_t spec_first,
                         int64_t env_first);

/* Frame split of the batch chain (nfft 2048 / hop 1024): with the context option "chain_split_frames" set,
 * hipdsp_chain_forward writes only the EVEN frames 2t of psd (frame 2t is tile t of its sweep) and this call,
 * which replaces hipdsp_sosfilt_envelope(..., phase = 2) behind it, writes the envelope
 * (BufferedEnvelope.process, bufferedenvelope.py:34-41: the backward half of sosfiltfilt from the tile states
 * the forward sweep parked in the context scratch) AND the ODD frames 2t+1 (second half of tile t, first half
 * of tile t+1) of BufferedSpectrogram.process (bufferedspectrogram.py:45-59) -- both launches then carry one
 * FFT per tile instead of two in the forward sweep (which is bound by VALU issue) and none in the backward
 * sweep (which is not), and move 10 bytes per sample each.  Same psd / frames_out / psd_pitch as the
 * forward call; together the two calls write every frame below n_valid, the forward call the zero tail.
 * Covers envelope plans of one or two decaying sections; HIPDSP_ERR_UNSUPPORTED otherwise.  The forward call behind
 * it must have walked the unshifted grid (spec_first = env_first = 0, the same channels / frames / sections) and
 * nothing may have used the context's scratch in between: HIPDSP_ERR_INVALID otherwise. */
int hipdsp_chain_backward(hipdsp_ctx *ctx, const hipdsp_sosplan *eplan, const float *yf, int64_t yf_pitch,
                          float *env, int64_t env_pitch, int64_t channels, int64_t frames, int rectify,
                          double gain, int clamp, int nfft, int hop, double fs, float *psd,
                          int64_t frames_out, int64_t psd_pitch);

/* The time segmentation hipdsp_chain_forward uses for `channels` x `frames` with these plans
 * (one IIR wave per channel and segment): segment s covers frames [s * segment_frames,
 * (s + 1) * segment_frames).  For tests and integrators that want to look at the seams; the
 * results do not depend on it beyond float32 rounding of the frames that straddle a border. */
int hipdsp_chain_plan(hipdsp_ctx *ctx, const hipdsp_sosplan *fplan, const hipdsp_sosplan *eplan,
                      int64_t channels, int64_t frames, int64_t *segment_frames, int *n_segments);

/* The same for hipdsp_chain_backward, whose segments are counted from the END of the trace: segment s covers
 * frames [first_border - s * segment_frames, first_border - (s - 1) * segment_frames), s = 0 the last one. */
int hipdsp_chain_backward_plan(hipdsp_ctx *ctx, const hipdsp_sosplan *eplan, int64_t channels, int64_t frames,
                               int64_t *first_border, int64_t *segment_frames, int *n_segments);

/* BufferedSpectrogram.process (bufferedspectrogram.py:45-59) ==
 * scipy.signal.spectrogram(x, fs, 'hann', nperseg=nfft, noverlap=nfft-hop,
 * detrend='constant', scaling='density', mode='psd'):
 *   out[c, k, :] = one-sided PSD of x[c, k*hop : k*hop + nfft] for k < n_valid,
 *   zeros for n_valid <= k < frames_out,
 * where n_valid = (nsource - (nfft - hop)) / hop and
 * nsource = min((frames_out - 1)*hop + nfft, frames)  (0 valid frames when
 * nsource < nfft).  out is (channels, frames_out, nfft/2 + 1) float32 with out_pitch
 * elements between consecutive channels (0 = compact, frames_out*(nfft/2 + 1)).
 * If db_out != NULL it additionally receives decibel(out) (fused epilogue,
 * specitem.py:36) in the same layout.  nfft: any power of two in [8, 524288] (the reference's
 * nfft selector, databrowser.py:516; 65536 in the registers of one workgroup, 131072 of two, 262144 and 524288 as tasks of one or two passes of such a workgroup)
 * and, for the values the reference's clamp to len(source)//2 can produce, any other size up
 * to 131072 (direct DFT, O(nfft^2), meant for the rare short recording).
 * nfft 262144 and 524288 (windows of 2.7 and 5.5 s at 96 kHz) are covered, not streamed: NOT roofline kernels --
 * every task re-reads the frame and the first pass parks its points in `out` and reads them back (4.8 x / 8.1 x the
 * algorithmic bytes, 0.6 / 0.4 TB/s).  For these two sizes `out` is therefore also a WORK AREA while the call runs:
 * ordinary device memory, nobody else reading or writing it until the call has completed on the context's stream.
 * nfft 131072 has the two workgroups of a frame own interleaved bins (one radix-2 step in front of the transform):
 * they share every 32-byte sector of the output, 1.1 x the algorithmic bytes for the PSD, 1.4 x with db_out. */
int hipdsp_spectrogram(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels,
                       int64_t frames, int nfft, int hop, double fs, float *out,
                       float *db_out, int64_t frames_out, int64_t out_pitch);

/* thunderlab.powerspectrum.decibel (specitem.py:28,36; spectrogramplot.py:159;
 * bufferedspectrogram.py:116-117): out = 10*log10(p/ref_power), -inf where
 * p <= min_power.  The same rules hold for every entry point that takes ref_power and min_power
 * (the two image calls below, hipdsp_mean_spectrum_db, hipdsp_band_power with db):
 *  - the threshold is compared as written, p against the double min_power: a power equal to
 *    (float)min_power is finite when that cast rounded up (1e-7, 0.1, 1e-10 do).  NaN stays NaN,
 *    +inf gives +inf;
 *  - ref_power is any positive finite double.  Where p * (float)(1/ref_power) is a normal float the
 *    result is 10*log10f of that product (at ref_power == 1 of p itself): within
 *    a*(10/ln 10)*2^-24 + 3 ulp of the exact value, a = 2 roundings of the argument, 0 at
 *    ref_power == 1.  Elsewhere -- a reciprocal or product outside float32's normal range, a
 *    denormal p -- the quotient is taken in float64 and the result is within 1 ulp.
 * tests/decibel_bound.py holds every element to this. */
int hipdsp_decibel(hipdsp_ctx *ctx, const float *p, float *out, int64_t n, double ref_power,
                   double min_power);
/* SpecItem.update_plot (specitem.py:36): decibel(buffer[:, ch, :].T) -- one
 * channel's (frames, nfreq) slab to a (nfreq, frames) dB image. */
int hipdsp_decibel_image(hipdsp_ctx *ctx, const float *spec_tf, float *image_ft,
                         int64_t frames, int64_t nfreq, double ref_power, double min_power);
/* The same image at screen resolution: column c = decibel(max over the frames
 * [start + c*step, min(start + (c+1)*step, stop)) ), i.e. np.maximum.reduceat over the
 * segments arange(0, stop - start, step) -- the min/max screen decimation TraceItem.update_plot
 * applies to traces (traceitem.py:42-61), applied to the spectrogram image (the reference's
 * README TODO "Implement downsampling of spectrograms", README.md:96).  image_fc is
 * (nfreq, ceil((stop - start) / step)); NaN propagates like np.maximum. */
int hipdsp_decibel_image_decimate(hipdsp_ctx *ctx, const float *spec_tf, float *image_fc,
                                  int64_t frames, int64_t nfreq, int64_t start, int64_t stop,
                                  int64_t step, double ref_power, double min_power);

/* ---- next rows --------------------------------------------------- */

/* Screen-resolution decimation of traces on the device (TraceItem.update_plot,
 * traceitem.py:55-61; the same reduction fills the overview cache, compresseddata.py:48-52):
 *   segments = arange(0, stop - start, step)
 *   out[c, 0::2] = np.minimum.reduceat(x[c, start:stop], segments)
 *   out[c, 1::2] = np.maximum.reduceat(x[c, start:stop], segments)
 * for every channel; out is (channels, out_pitch) float32 with 2*ceil((stop-start)/step)
 * valid values per row.  Only the few thousand plot points then cross PCIe (or xGMI). */
int hipdsp_minmax_decimate(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels,
                           int64_t start, int64_t stop, int64_t step, float *out,
                           int64_t out_pitch);

/* Playback chain (DataBrowser.play_region, databrowser.py:1711-1729): out[k] = mean over the
 * listed channels of x[c, start + k], k < n, optionally times the heterodyne carrier
 * sin(2 pi k * heterodyne_cycles_per_sample) (0 = none).  The low-pass that follows is
 * hipdsp_envelope(rectify = 0, clamp = 0), i.e. plain sosfiltfilt, and `[::nstep]` is
 * hipdsp_stride_copy (out[i] = x[i*step], ceil(n/step) values). */
int hipdsp_channel_mean(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, const int *host_channels,
                        int count, int64_t start, int64_t n, double heterodyne_cycles_per_sample,
                        float *out);
int hipdsp_stride_copy(hipdsp_ctx *ctx, const float *x, int64_t n, int64_t step, float *out);

/* Common-reference subtraction across the channels of a planar trace (the reference's "Subtract common mean" plug-in,
 * and the median that arrays use instead).  host_group[c] is the group of channel c, an id in [0, channels), or -1 for
 * a channel that passes through; host_use[c] != 0 (NULL: every channel) makes c a reference channel of its group.
 * Per group g and sample t, with members(g) = {c : group[c] == g} and refs(g) = {c in members(g) : use[c]} in
 * ascending c:
 *   y[c, t] = (float)((double)x[c, t] - ref_g[t])   for every member c -- one rounding, at the end;
 *   HIPDSP_CREF_MEAN:   ref = s / n, s the float64 sum of (double)x[k, t] over refs(g), added one by one in ascending
 *                       channel order from 0.0, n = |refs(g)| as a double (the library is built with
 *                       -ffp-contract=off: reproducible bit for bit);
 *   HIPDSP_CREF_MEDIAN: the refs values at t ordered by value: the middle one for odd n, ((double)a + (double)b) * 0.5
 *                       of the two middle ones for even n.
 * A NaN among the refs values at t makes ref NaN (as numpy's mean and median do); infinities follow IEEE arithmetic
 * (inf - inf = NaN); -0 and +0 compare equal, the sign of a zero RESULT is not specified.  A member with use == 0 gets
 * the reference taken off without contributing to it (a dead or clipping channel).  Channels of group -1 are copied;
 * in place they are neither read nor written.
 * In place (y == x with y_pitch == x_pitch) is allowed: all inputs of a sample are read before any of its outputs is
 * written; any other overlap is refused.  A pitch of 0 means `frames`; rows need no alignment beyond 4 bytes.
 * HIPDSP_ERR_INVALID: a group id outside [-1, channels), a group with members but no reference channel, an unknown
 * mode, a pitch below frames, a partial overlap, NULL pointers.  HIPDSP_ERR_UNSUPPORTED: channels > 1024, a median over
 * more than 64 reference channels in one group.
 * The group table travels by value in the kernel arguments: one kernel launch, no context scratch, no host
 * synchronisation, nothing uploaded -- legal inside hipdsp_graph_begin/end.  No atomics: a group's output bytes
 * depend on that group's rows alone.  HIPDSP_CREF_TILE is the largest number of frames one workgroup covers: 1024 when
 * no group has more than 16 reference channels, 512 up to 64, 32 beyond (means only). */
#define HIPDSP_CREF_MEAN   0
#define HIPDSP_CREF_MEDIAN 1
#define HIPDSP_CREF_TILE   1024
int hipdsp_common_reference(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, float *y, int64_t y_pitch,
                            int64_t channels, int64_t frames, const int *host_group,
                            const unsigned char *host_use, int mode);

/* Maximum of n non-negative floats (PSD values) into out[0]; with the strided gather of
 * hipdsp_memcpy2d_d2d it serves BufferedSpectrogram.estimate_noiselevels
 * (bufferedspectrogram.py:109-126: max dB = decibel(max power), P95 of the top 1/16 band). */
int hipdsp_max_nonneg(hipdsp_ctx *ctx, const float *x, int64_t n, float *out);

/* out2[0], out2[1] = the order statistics of rank `rank` and `rank + 1` (zero based, ascending; the second
 * clamped to the last) of the rows x cols non-negative floats x[i * row_stride + j] -- what
 * np.percentile(..., 95) interpolates between in BufferedSpectrogram.estimate_noiselevels
 * (bufferedspectrogram.py:115-117: the top F/16 bins of one channel's (frames, F) slab; decibel is
 * monotonic, so the percentile of the dB values is the interpolation of the dB of these two).  Exact
 * (radix select on the float bits), one workgroup, nothing but two floats leaves the device. */
int hipdsp_band_order_stats(hipdsp_ctx *ctx, const float *x, int64_t rows, int64_t cols, int64_t row_stride,
                            int64_t rank, float *out2);

/* audioio's unwrap() of clipped recordings, which the reference arms on its raw loader for every buffer
 * it loads (Data.open -> self.data.set_unwrap(unwrap, unwrap_clip, False, unit), src/audian/data.py:180;
 * CLI -u / -U, src/audian/audian.py:1485-1512, default threshold 1.5): a step between successive samples
 * beyond `thresh` is a wrap-around of a signal that left [-ampl_max, ampl_max); from there on 2 * ampl_max
 * is subtracted (step up) or added (step down), cumulatively along time, per channel, starting from
 * zero at the first frame of the slab.  Then `clips`: clip to +-ampl_max; else `down_scale`: halve.
 * Planar float32 in and out; x and y must not overlap (a chunk reads the last sample of the chunk
 * before it while that one is being written).  audioio's source is neither in the reference tree nor
 * in this image: restated from its documentation and the reference's call sites, parity unpinned.
 * Uses the context scratch (4 bytes per 16384 frames and channel). */
int hipdsp_unwrap(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t frames,
                  double thresh, double ampl_max, int clips, int down_scale, float *y, int64_t y_pitch);

/* PCM ingest: interleaved little-endian signed PCM (frames, channels) of 2, 3 or 4 bytes per
 * sample -> planar float32 times `scale` (1/2^(bits-1) reproduces the [-1, 1) floats that
 * audioio / thunderlab's DataLoader give audian, data.py:172).  Uploading the file's own
 * integers instead of float64 cuts the PCIe volume of the raw slab 2.7-4x. */
int hipdsp_pcm_unpack(hipdsp_ctx *ctx, const void *pcm_tc, int sample_bytes, int64_t frames,
                      int64_t channels, double scale, float *dst, int64_t dst_pitch);

/* Full-trace overview straight from the file's PCM (CompressedData.start / down_sample_worker,
 * src/audian/compresseddata.py:25-52, 102-113): the min/max envelope of interleaved little-endian signed PCM
 * (frames, channels) of 2, 3 or 4 bytes per sample, in the reference's layout: out_rc is float64
 * (2*nseg, channels) with row pitch out_pitch (elements), nseg = ceil(frames/step), row 2j the minimum and row
 * 2j+1 the maximum of frames [j*step, min((j+1)*step, frames)).  One read of the PCM bytes (hipdsp_pcm_unpack +
 * hipdsp_minmax_decimate move about 10 B per int16 sample).  Bit-exact:
 *   unwrap_thresh <= 1e-3: the values are int * scale in float64 (reduced as integers, scaled once per segment);
 *   else: hipdsp_unwrap's arithmetic on x = (float)(int * scale) -- events beyond +-unwrap_thresh shift by
 *         -+2*ampl_max from zero at the call's first frame, then clip to +-ampl_max (clips) or halve (down_scale) --
 *         and the min/max of those float32 values, widened.  The PCM is read twice (count, then reduce).
 * Any step >= 1 (step = 1: twice as many output rows as frames; step > frames: one segment).  Frames of at most
 * 16384 bytes (channels * sample_bytes; HIPDSP_ERR_UNSUPPORTED beyond).  Uses the context scratch (8 bytes per
 * segment and channel, plus 4 bytes per channel and run of frames a thread walks, with unwrap). */
int hipdsp_pcm_minmax(hipdsp_ctx *ctx, const void *pcm_tc, int sample_bytes, int64_t frames, int64_t channels,
                      int64_t step, double scale, double unwrap_thresh, double ampl_max, int clips, int down_scale,
                      double *out_rc, int64_t out_pitch);

/* Power spectrum of the visible window (SpectrogramPlot.update_plot,
 * spectrogramplot.py:158-160):
 *   power = np.mean(spec[i0:i1, :], axis=0); power = decibel(power); power[power < floor] = floor
 * on one channel's (frames, nfreq) slab; out gets nfreq float32 values (floor_db = -200 in
 * the reference).  Uses the context scratch (shared with the envelope). */
int hipdsp_mean_spectrum_db(hipdsp_ctx *ctx, const float *spec_tf, int64_t nfreq, int64_t i0,
                            int64_t i1, double ref_power, double min_power, double floor_db,
                            float *out);

/* Band power: the derived trace whose source is the spectrogram, the reference's open plug-in test "Envelope from
 * visible frequency range of spectrogram" (README.md:63).  spec is the planar slab the spectrogram entry points write,
 * (channels, frames, nfreq) float32 with spec_pitch elements between channels (0 = compact); for every band b, channel
 * c and frame t
 *   out[b*out_band_pitch + c*out_pitch + t] = scale * sum(spec[c, t, k0[b]:k1[b]])            (float32)
 * (out_pitch 0 = frames, out_band_pitch 0 = channels*out_pitch); with db != 0 the value stored is
 * decibel(that, ref_power, min_power) in exactly hipdsp_decibel's arithmetic (-inf at or below min_power).  With
 * scale = the bin width in Hz this is the integral of the PSD over the band, in the signal's squared unit.
 * host_k0 / host_k1 are HOST arrays of n_bands bin ranges, 0 <= k0 <= k1 <= nfreq (k0 == k1: an empty band, 0 or -inf);
 * they travel to the kernel by value: no upload, no host synchronisation, legal inside hipdsp_graph_begin/end.  Up to
 * 16 bands per call (more: HIPDSP_ERR_UNSUPPORTED), all served by ONE pass: of every row only the bins the union of
 * the bands covers are read, and a bin that lies in several bands is read once.  A multi-band call gives bit for bit
 * what one call per band gives.  NaN and +-inf propagate as in np.sum, to their own frame's value only.  frames == 0
 * or channels == 0: nothing is written.  No alignment is assumed (rows of nfreq = nfft/2 + 1 floats start at any
 * 4-byte address); at most 65535 channels and 2^24 - 1 frames per call (2^31 - 1 with nfreq <= 256).
 * Accuracy: the bins are summed in float64 and the scaled sum is rounded to float32 once.  A float64 sum of at most
 * 2^18 + 1 float32 terms of one sign is off by less than 2^-34 relative, so for non-negative input the linear result
 * is within 1 float32 ulp of float32(scale * S), S the exact sum of the bins. */
int hipdsp_band_power(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, int64_t channels,
                      int64_t frames, int64_t nfreq, const int64_t *host_k0, const int64_t *host_k1,
                      int n_bands, double scale, int db, double ref_power, double min_power,
                      float *out, int64_t out_pitch, int64_t out_band_pitch);

/* Spectral contour features: where the power inside a band of bins sits in frequency, per frame and channel -- what a
 * user reads off a spectrogram (peak frequency, its sweep inside a call, tonal or noisy) without the slab leaving the
 * device.  spec, spec_pitch and the alignment-free rows are those of hipdsp_band_power; the band is the bins [k0, k1),
 * 0 <= k0 <= k1 <= nfreq.  `features` is a mask of the HIPDSP_FEATURE_ bits below; the rows of the requested features
 * are stored in ascending bit order,
 *   out[j*out_feature_pitch + c*out_pitch + t],   j = number of set bits below the feature's own
 * (out_pitch 0 = frames, out_feature_pitch 0 = channels*out_pitch).  scale is the bin width in Hz (1.0: bins).
 * With P[k] the float32 bin, n = k1 - k0, sums over the band, and all arithmetic in float64 (no fused multiply-add),
 * every stored value rounded to float32 once:
 *   bit 0 PEAK_BIN_FREQ  scale*kp, kp = np.argmax(P[k0:k1]) + k0: the first of equal maxima, the first NaN if any
 *   bit 1 PEAK_FREQ      scale*(kp + d), d = 0.5*(a - c)/((a - 2b) + c) with a, b, c = ln P[kp-1], ln P[kp], ln P[kp+1]
 *                        if kp-1 >= k0, kp+1 < k1, both neighbours > 0 and (a - 2b) + c < 0; else d = 0 (a peak at the
 *                        band's edge, a zero neighbour, a plateau of three equal bins)
 *   bit 2 PEAK_POWER     P[kp] exactly
 *   bit 3 CENTROID       scale*(kp + M1/S), S = sum P[k], M1 = sum (k - kp) P[k]
 *   bit 4 BANDWIDTH      scale*sqrt(max(M2/S - (M1/S)^2, 0)), M2 = sum (k - kp)^2 P[k]: the moments are taken about
 *                        the peak, which keeps the subtraction conditioned for a narrow line anywhere in the band
 *   bit 5 FLATNESS       exp(sum(ln P[k])/n) / (S/n), the Wiener entropy: 1 for a flat band, 0 once a bin is 0
 *   bit 6 FREQ_LOW       scale*klo, klo the first k with (double)P[k] >= drop_ratio*(double)P[kp]
 *   bit 7 FREQ_HIGH      scale*khi, khi the last such k;  0 < drop_ratio <= 1 (10^(-dB/10), from the host)
 * Masking: if P[kp] is not finite or not > min_power -- NaN or +inf in the band, an empty band, a silent frame, the
 * spectrogram's zero tail frames with min_power >= 0 -- every feature except PEAK_POWER is NaN; PEAK_POWER is P[kp]
 * as it is, NaN for an empty band.  The input contract is non-negative bins, as every spectrogram entry point writes
 * them.
 * HIPDSP_ERR_INVALID: NULL ctx, NULL spec or out with work to do, a negative size or pitch, a band outside [0, nfreq],
 * features == 0 or bits above 7, drop_ratio outside (0, 1], a pitch too small for the sizes.  frames == 0 or
 * channels == 0: nothing is written.  Limits: at most 65535 channels, nfreq <= 2^26 (all of nfft 8 ... 2^19 and
 * beyond), 2^24 - 1 frames per call (2^28 - 1 with nfreq <= 256).
 * Promises: no atomics; no context scratch and no upload -- all arguments travel by value, the call is one kernel node
 * inside hipdsp_graph_begin/end; the same call gives the same bits twice; what a frame stores depends on that frame's
 * band alone, not on the other channels or frames of the call, the pitches or which other features are requested (the
 * mapping is chosen by nfreq alone, a thread's share of a row by the absolute bin index); only bins inside the band
 * are read, nothing outside the requested rows is written; index arithmetic on the slab is 64-bit.  A band of up to
 * 8448 bins is read from memory once (it waits in LDS between the two passes), a wider one twice.  log() is
 * evaluated once per bin only with FLATNESS and three times per row with PEAK_FREQ. */
#define HIPDSP_FEATURE_PEAK_BIN_FREQ 1u
#define HIPDSP_FEATURE_PEAK_FREQ 2u
#define HIPDSP_FEATURE_PEAK_POWER 4u
#define HIPDSP_FEATURE_CENTROID 8u
#define HIPDSP_FEATURE_BANDWIDTH 16u
#define HIPDSP_FEATURE_FLATNESS 32u
#define HIPDSP_FEATURE_FREQ_LOW 64u
#define HIPDSP_FEATURE_FREQ_HIGH 128u
int hipdsp_spectral_features(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, int64_t channels,
                             int64_t frames, int64_t nfreq, int64_t k0, int64_t k1, unsigned features,
                             double scale, double min_power, double drop_ratio, float *out, int64_t out_pitch,
                             int64_t out_feature_pitch);

/* Per-bin order statistics over time: the noise profile of a spectrogram (a percentile of every frequency bin, which a
 * stationary band -- mains hum, an insect chorus, microphone noise -- dominates and a call does not).  spec, spec_pitch
 * and the alignment-free rows are those of hipdsp_band_power.  For channel c and bin k in [k0, k1) the input set is
 *   spec[c, first + j*frame_step, k],  j < n_frames         (first >= 0, first + (n_frames-1)*frame_step < frames)
 * with the NaNs dropped: n values remain, v[0..n-1] ascending by value (infinities included, -0 equal to +0).  With
 *   pos = q*(double)(n - 1)   (one double multiply),   k_lo = floor(pos),   k_hi = min(k_lo + 1, n - 1)
 * the call stores, at column i = c*(k1 - k0) + (k - k0),
 *   out_lo_hi[2*i] = v[k_lo],  out_lo_hi[2*i + 1] = v[k_hi],  out_count[i] = n      (out_count may be NULL)
 * and NaN, NaN, 0 for a column without a value (n == 0, also n_frames == 0).  Both values are elements of the input,
 * bit for bit; the sign of a returned zero is unspecified.  The host finishes the percentile as np.percentile does:
 * frac = pos - k_lo, the result is lo when frac == 0 or hi == lo, else lo + frac*(hi - lo) in float64.  The profile is
 * the percentile itself: no bias correction of a median towards the mean of periodogram values is applied.
 * HIPDSP_ERR_INVALID: NULL ctx, q outside [0, 1] or NaN, a band outside [0, nfreq], frame_step < 1, a frame range
 * outside [0, frames), a negative size, a pitch too small, NULL spec or out_lo_hi with work to do, an output that
 * overlaps the slab or the other output, frames*nfreq or spec_pitch beyond 2^44 elements.
 * HIPDSP_ERR_UNSUPPORTED: n_frames >= 2^31 (the counters are 32-bit), more than 65535 channels.  channels == 0 or
 * k1 == k0: nothing is written.  A refused call writes nothing.
 * Promises: an exact radix select, four passes of 8-bit digits over an order-preserving 32-bit key, each a read of the
 * columns' elements (the requested frames of the band are read four times); no atomics on global memory (LDS
 * counters only) and no context scratch; all scalars travel by value, the call is one kernel node inside
 * hipdsp_graph_begin/end; the same call gives the same bits twice; a column's result depends on its own values alone,
 * not on the other channels, on k0 / k1, on the pitch or on the tile of bins it falls in; only the requested elements
 * are read and nothing outside the output rows is written; index arithmetic on the slab is 64-bit, rows start at any
 * 4-byte address. */
int hipdsp_bin_quantiles(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, int64_t channels, int64_t frames,
                         int64_t nfreq, int64_t first, int64_t n_frames, int64_t frame_step, int64_t k0, int64_t k1,
                         double q, float *out_lo_hi, int32_t *out_count);

/* Equalise a spectrogram slab by a per-channel, per-bin profile (hipdsp_bin_quantiles, finished on the host):
 *   HIPDSP_EQ_DIVIDE    out[c, t, k] = float32((double)spec[c, t, k] / (double)profile[c, k])  -- the correctly rounded
 *                       float32 quotient (53 >= 2*24 + 2), the whitened image
 *   HIPDSP_EQ_SUBTRACT  out[c, t, k] = float32(spec[c, t, k] - profile[c, k]), then 0 where that is < 0 -- spectral
 *                       subtraction
 * NaN stays NaN, infinities and denormals as IEEE 754 and numpy's float32 arithmetic have them: both modes are bit for
 * bit numpy's.  spec and out are planar (channels, frames, nfreq) slabs with spec_pitch / out_pitch elements between
 * channels (0 = frames*nfreq); profile is a DEVICE array (channels, nfreq) float32 with profile_pitch elements between
 * channels (0 = nfreq).  In place (out == spec with equal pitch) is allowed, any other overlap of out with spec or with
 * the profile is HIPDSP_ERR_INVALID, as are NULL pointers with work to do, negative sizes, a pitch too small, frames*nfreq
 * or a pitch beyond 2^44 elements and an unknown mode; more than 65535 channels is HIPDSP_ERR_UNSUPPORTED.  A refused call writes nothing; channels, frames or
 * nfreq == 0 writes nothing.  Promises: one streaming pass, one kernel node inside hipdsp_graph_begin/end, no atomics,
 * no context scratch, the same bits twice, a value depends on its own element and its profile entry alone, 64-bit index
 * arithmetic, rows at any 4-byte address (16-byte accesses only where both slabs allow them). */
#define HIPDSP_EQ_DIVIDE 0
#define HIPDSP_EQ_SUBTRACT 1
int hipdsp_spec_equalize(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, float *out, int64_t out_pitch,
                         int64_t channels, int64_t frames, int64_t nfreq, const float *profile, int64_t profile_pitch,
                         int mode);

/* Adaptive normalisation of a spectrogram slab: a RUNNING noise floor per channel and bin, and the slab normalised by
 * it -- for backgrounds that are not stationary (wind, rain, a passing car, a chorus that swells), where the one
 * profile of hipdsp_spec_equalize is either raised by them or lies below them.  For one column (channel c, bin k) with
 * x_t = spec[c, t, k], s = smooth, a = 1 - s (one double subtraction):
 *   M_0 = x_0,   M_t = a*M_(t-1) + s*x_t   (t >= 1)
 * (scipy.signal.lfilter([s], [1, s-1], x, zi=lfilter_zi(...)*x[0]), the smoother of librosa's pcen).  The first
 * nbefore rows are warm-up only; output row i belongs to t = nbefore + i, out[c, i, k] = float32(...) of
 *   HIPDSP_ADAPT_BACKGROUND   M_t                                               the floor itself
 *   HIPDSP_ADAPT_DIVIDE       x_t / (eps + M_t)
 *   HIPDSP_ADAPT_SUBTRACT     max(x_t - M_t, 0)
 *   HIPDSP_ADAPT_PCEN         (x_t / (eps + M_t)**gain + bias)**power - bias**power
 * evaluated in float64 (state, hand-over and the mode's formula; pow() of the device library twice per element in
 * PCEN) and rounded to float32 once.  0 < smooth <= 1; eps > 0 for DIVIDE and PCEN (the spectrogram's zero tail
 * frames give 0, not 0/0); 0 <= gain <= 1, bias >= 0, power > 0 for PCEN (the logarithmic power -> 0 variant is not
 * served); parameters a mode does not use are not looked at.  A NaN or an infinity at (c, t0, k) gives from t0 on, in
 * that column alone, the NaN / +inf / -inf / finite pattern of the sequential float64 evaluation of these formulas.
 * spec holds `frames` rows per channel, out holds frames - nbefore; spec_pitch / out_pitch are elements between
 * channels (0 = dense: frames*nfreq and (frames - nbefore)*nfreq).  In place (out == spec, equal pitch) is allowed with
 * nbefore == 0; any other overlap of out with spec is HIPDSP_ERR_INVALID, as are a NULL ctx, NULL pointers with work to
 * do, a pointer off the 4-byte grid, negative sizes, nbefore > frames, a pitch too small, frames*nfreq or a pitch
 * beyond 2^44 elements, an unknown mode and parameters outside the ranges above (NaN included); more than 65535
 * channels is HIPDSP_ERR_UNSUPPORTED.  A refused call writes nothing; channels, nfreq == 0 or nbefore == frames writes
 * nothing.
 * Time is cut into chunks of HIPDSP_ADAPT_CHUNK frames counted from row 0 -- a function of `frames` alone, never of
 * channels, nfreq, the pitches or the device -- with an exact hand-over M' = a^CHUNK*M + v (a^CHUNK from the host,
 * long double, rounded once; v the chunk's end value from zero state), three launches ordered by the stream: the
 * summaries v, the scan of the carries, the result (a call of one chunk is the last launch alone).  256 frames: the
 * carries are 1/128 of the slab's bytes and a 56250-frame slab still gives every CU hundreds of waves.
 * Promises: no kernel waits for another workgroup, no atomics; all scalars travel by value, the call is up to three
 * kernel nodes inside hipdsp_graph_begin/end; it uses the context scratch (8 bytes per channel, bin and chunk but the
 * last), which cannot grow during a capture or next to captured graphs of the context (HIPDSP_ERR_INVALID then):
 * hipdsp_ctx_reserve() it before; the same call gives the same bits twice and nothing depends on what the scratch
 * held; a column's bytes depend on that column, nbefore and the parameters alone, not on the other channels or bins of
 * the call or the pitches; 64-bit index arithmetic, rows at any 4-byte address (dword accesses); the slab is read
 * twice (less its last chunk and, the second time, the chunks in front of nbefore) and written once. */
#define HIPDSP_ADAPT_BACKGROUND 0
#define HIPDSP_ADAPT_DIVIDE 1
#define HIPDSP_ADAPT_SUBTRACT 2
#define HIPDSP_ADAPT_PCEN 3
#define HIPDSP_ADAPT_CHUNK 256
int hipdsp_spec_adapt(hipdsp_ctx *ctx, const float *spec, int64_t spec_pitch, float *out, int64_t out_pitch,
                      int64_t channels, int64_t frames, int64_t nfreq, int64_t nbefore, double smooth, int mode,
                      double gain, double bias, double power, double eps);

/* ---- FIR kernel bank ("feature expansion (kernel filter)") ----------------- */

/* A plan holds, in device memory, the taps and thresholds of up to 16 FIR kernels of one common length, as
 * hipdsp_sosplan holds an SOS table: hipdsp_firplan_set is hipdsp_firplan_set_host (rounds and lays the taps out in
 * pinned host memory, no stream work) followed by hipdsp_firplan_upload (an async copy on the stream, which may be
 * captured), so a captured hipGraph replays under new kernels.  hipdsp_fir_bank reads n_kernels and n_taps from
 * the host side of the plan at call time (a captured call keeps those of capture time: replay it only under tap sets
 * of the same counts), and returns HIPDSP_ERR_INVALID while they differ from what was last uploaded, i.e. after a
 * hipdsp_firplan_set_host with new counts and no upload.  With equal counts the device keeps the previously uploaded
 * taps until the next upload.  hipdsp_firplan_set_host waits for the last upload enqueued
 * outside a capture before it rewrites the pinned block; a replayed graph's copy is not known to it, so the caller
 * synchronises the stream between a replay and the next hipdsp_firplan_set_host.
 * host_taps: (n_kernels, n_taps) float64, row k = kernel k; host_threshold: n_kernels float64, or NULL for zeros.
 * 1 <= n_kernels <= 16 and 1 <= n_taps <= 4097: larger counts give HIPDSP_ERR_UNSUPPORTED, zero or negative ones
 * HIPDSP_ERR_INVALID. */
int hipdsp_firplan_create(hipdsp_ctx *ctx, hipdsp_firplan **out);
int hipdsp_firplan_destroy(hipdsp_ctx *ctx, hipdsp_firplan *plan);
int hipdsp_firplan_set(hipdsp_ctx *ctx, hipdsp_firplan *plan, const double *host_taps, int n_kernels,
                       int n_taps, const double *host_threshold);
int hipdsp_firplan_set_host(hipdsp_ctx *ctx, hipdsp_firplan *plan, const double *host_taps, int n_kernels,
                            int n_taps, const double *host_threshold);
int hipdsp_firplan_upload(hipdsp_ctx *ctx, hipdsp_firplan *plan);

/* One feature trace per kernel of the plan.  With x[c, i] = 0 for i outside [0, frames), h = taps[k], L = n_taps:
 *     y[k, c, t] = sum_{j=0}^{L-1} h[j] * x[c, t + (L-1)/2 - j]     (integer division; for frames >= L this is
 *                                                                     np.convolve(x[c], h, 'same')[t])
 *     out[k*out_kernel_pitch + c*out_pitch + i] = y[k, c, first + i*step],   i < n_out
 * and with rectify != 0  max(y - threshold[k], 0)  (a NaN stays NaN, as np.maximum).
 * x is planar float32 with x_pitch floats per channel (0 = frames); out_pitch 0 means n_out, out_kernel_pitch 0
 * means channels*out_pitch (the layout of hipdsp_band_power).  Any first >= 0 is allowed, also first + i*step >=
 * frames: such windows are partly or wholly zeros.  step >= 1; a negative first or size is HIPDSP_ERR_INVALID; x and
 * out must not overlap (HIPDSP_ERR_INVALID); n_out == 0 or channels == 0 writes nothing; frames == 0 gives zeros
 * (rectified zeros).  At most 65535 channels and 2^36 outputs per call; index arithmetic is 64-bit.  Legal inside
 * hipdsp_graph_begin/end (nothing is allocated or configured by the call).
 *
 * Arithmetic contract.  Taps and thresholds are rounded to float32 once, on the host.  The products run on the
 * f32-input matrix core (v_mfma_f32_16x16x4_f32): every output is a float32 sum of float32 products with one rounding
 * per step -- an fmaf chain over the taps in some fixed order, the same for every output, or a regrouping of one.
 * For any summation order that gives, with u = 2^-24, n = L + 2 and M = sum_j |h[j]| * |x[..]| (the same window with
 * absolute values),
 *     |out - y_float64| <= n*u / (1 - n*u) * M,
 * and with rectify  (n+1)*u / (1 - (n+1)*u) * (M + |threshold|).  When every tap, sample and partial sum is an integer
 * below 2^24 in magnitude the result is therefore exact.
 * Determinism: the value for kernel k does not depend on which other kernels ride in the call (the mapping is chosen
 * by n_taps and step, never by n_kernels): a 16-kernel call gives bit for bit what 16 one-kernel calls give; the same
 * call gives the same bits twice.
 * Non-finite samples: an output is non-finite if its L-sample window contains a non-finite sample (without rectify;
 * max(-inf, 0) is 0); zero padding of the taps (to a multiple of 4) may carry that at most 16 samples further; an
 * output whose window is at least 16 samples clear of every non-finite sample equals what it is without that
 * sample, and other channels are not affected. */
int hipdsp_fir_bank(hipdsp_ctx *ctx, const hipdsp_firplan *plan, const float *x, int64_t x_pitch,
                    int64_t channels, int64_t frames, int64_t first, int64_t step, int64_t n_out, int rectify,
                    float *out, int64_t out_pitch, int64_t out_kernel_pitch);

/* ---- spectrogram template matching ("interface for event detectors") ------- */

/* Spectrogram cross-correlation: one example call, cut out of a spectrogram, is slid along the spectrogram of every
 * channel; the score of a window is the correlation of the template with the patch under it.
 *
 * Values.  spec is the planar slab (channels, frames, nfreq) float32 every spectrogram entry point writes, spec_pitch
 * elements between channels (0 = frames*nfreq).  Of every frame only the band of bins [k0, k0 + Fb) is read.  Per
 * element P the value is  v = decibel(P, ref_power, min_power)  with db != 0 -- bit for bit hipdsp_decibel's value --
 * and v = P without; then v = floor where v < floor (floor a float, -inf for none; a NaN stays NaN).
 *
 * Templates.  K templates of one common shape (Tt, Fb): Tt frames of Fb bins.  hipdsp_template_prepare_host prepares
 * the taps on the host, needs no context and no device:
 *   raw mode (normalize == 0)   g = float32(h);
 *   normalised mode             g = float32((h - mean h) / ||h - mean h||), mean and norm in extended precision;
 * for both  sum_out[k] = H0 = sum g  and  norm_out[k] = Q = sum (g - mean g)^2  of the ROUNDED taps, summed in
 * extended precision in row-major order and rounded to float64 once.  templates is (n, rows, cols) float64, taps_out
 * (n, rows, cols) float32.  A template with a non-finite value (or, raw, one that overflows float32) is
 * HIPDSP_ERR_INVALID; in normalised mode so is a template of zero variance (all values equal).  1 <= n <= 16,
 * 1 <= rows <= 256, 1 <= cols, rows*cols <= 65536: larger is HIPDSP_ERR_UNSUPPORTED, zero or negative
 * HIPDSP_ERR_INVALID.
 *
 * Score of template k, channel c, window start t = first + i, with n = Tt*Fb and w[a, b] = v[c, t + a, k0 + b]:
 *   raw         s = sum g[a, b] * w[a, b]
 *   normalised  r = sum g[a, b] * (w[a, b] - mean w) / sqrt(Q * D),  D = sum (w - mean w)^2: the Pearson coefficient of
 *               the rounded template and the patch (np.corrcoef(g.ravel(), w.ravel())[0, 1]), |r| <= 1
 *   out[k*out_template_pitch + c*out_pitch + i],  i < n_out   (out_pitch 0 = n_out, out_template_pitch 0 =
 *   channels*out_pitch: the pitch defaults of hipdsp_band_power).
 * NaN in both modes where the window does not lie inside [0, frames): first may be negative and first + i + Tt may
 * pass frames.  NaN in normalised mode where the window holds a NaN or an infinity, or where D <= n*min_std^2 -- a patch
 * too flat to match: silence at the floor, the spectrogram's zero tail frames; min_std >= 0 is in v's unit.  In raw
 * mode non-finite values follow IEEE arithmetic.  Only the band's bins are ever read: the zero padding of the matrix
 * core's K dimension is zeros in the values as well as in the taps, a NaN in bin k0 + Fb cannot leak in.  A window
 * clear of every non-finite element gives what it gives without that element; other channels are not affected.
 *
 * pivot is a float the caller chooses, near the level of the values (the template's mean, the noise floor): the matrix
 * core sees float32(v - pivot), which keeps dB values near -90 from costing the float32 accumulation its bits.  The
 * definition's result does not depend on pivot, only the bound below does.
 *
 * The plan.  hipdsp_tmplplan_* hold the prepared taps in device memory as hipdsp_firplan_* hold FIR taps, with the
 * same capture rules: hipdsp_tmplplan_set is hipdsp_tmplplan_set_host (hipdsp_template_prepare_host, then the taps laid
 * out in pinned host memory; no stream work) followed by hipdsp_tmplplan_upload (an async copy on the stream, which
 * may be captured), so a captured hipGraph replays under new templates.  hipdsp_template_match reads the template
 * count, the shape and the mode from the host side of the plan at call time (a captured call keeps those of capture
 * time: replay it only under template sets of the same count, shape and mode), and returns HIPDSP_ERR_INVALID while
 * they differ from what was last uploaded.  hipdsp_tmplplan_set_host waits for the last upload enqueued outside a
 * capture before it rewrites the pinned block; a replayed graph's copy is not known to it, so the caller synchronises
 * the stream between a replay and the next hipdsp_tmplplan_set_host.  Normalised or raw is a property of the plan.
 *
 * HIPDSP_ERR_INVALID: a NULL ctx or plan, NULL spec or out with work to do, a negative size or pitch, a band outside
 * [0, nfreq], a plan set but not uploaded, spec and out overlapping, min_std < 0, a NaN floor or a non-finite pivot, a
 * pitch too small for the sizes.  A refused call writes nothing.  n_out == 0 or channels == 0 writes nothing.  At most
 * 65535 channels and 2^36 windows per call.
 *
 * Arithmetic.  The products run on the f32-input matrix core (v_mfma_f32_16x16x4_f32), 16 windows x 16 templates per
 * instruction; all 16 columns are always computed, the mapping is chosen by (Tt, Fb) alone, never by K, and the n
 * products of a window are added in one fixed order (chunks of the band, inside a chunk frame by frame, bins in
 * fours).  Normalised: per frame and channel the band sums S1 = sum (v - pivot) and S2 = sum (v - pivot)^2 are taken
 * in float64 (v - pivot is exact there), added per window over its Tt frames directly, D = S2 - S1^2/n, numerator
 * G - (S1/n)*H0 with G the float32 accumulator, one rounding to float32 at the end (and a clamp to [-1, 1]).  Raw:
 * float32(G + pivot*H0) in float64, G itself at pivot == 0.
 * Accuracy, with u = 2^-24, m = n + 3, gamma = m*u/(1 - m*u), e = 2^-53, M = sum |g| * |float32(v - pivot)| over the
 * window, S2 as above (exact), every element held to it:
 *   raw         |out - s| <= gamma*M + 4*e*|pivot*H0| + (pivot != 0: u*|s|, the float32 store)
 *               exact when taps, values and all partial sums are integers below 2^24 and pivot == 0;
 *   normalised  |out - r| <= gamma*M/sqrt(Q*D) + (n + 4)*e*sqrt(S2/n)*|H0|/sqrt(Q*D) + (3*n + 6)*e*(S2/D)*|r|
 *                            + (u + 8*e)*|r| + 2^-149
 * (tests/template_match_definition.py derives it).  The mask D <= n*min_std^2 is exact except for windows with
 * |D - n*min_std^2| <= (3*n + 6)*e*S2 + 4*e*n*min_std^2.
 * Promises: no atomics, no context scratch, all scalars by value: one kernel node inside hipdsp_graph_begin/end; the
 * same call gives the same bits twice; a 16-template call gives bit for bit what 16 one-template calls give; a
 * channel's or window's value does not depend on the other channels, on first, on n_out, on the pitches or on the tile
 * it falls in; nothing outside the requested rows is written; index arithmetic on the slab is 64-bit and rows start at
 * any 4-byte address. */
typedef struct hipdsp_tmplplan hipdsp_tmplplan;
int hipdsp_template_prepare_host(const double *templates, int n, int rows, int cols, int normalize,
                                 float *taps_out, double *sum_out, double *norm_out);
int hipdsp_tmplplan_create(hipdsp_ctx *ctx, hipdsp_tmplplan **out);
int hipdsp_tmplplan_destroy(hipdsp_ctx *ctx, hipdsp_tmplplan *plan);
int hipdsp_tmplplan_set(hipdsp_ctx *ctx, hipdsp_tmplplan *plan, const double *host_templates, int n_templates,
                        int rows, int cols, int normalize);
int hipdsp_tmplplan_set_host(hipdsp_ctx *ctx, hipdsp_tmplplan *plan, const double *host_templates,
                             int n_templates, int rows, int cols, int normalize);
int hipdsp_tmplplan_upload(hipdsp_ctx *ctx, hipdsp_tmplplan *plan);
int hipdsp_template_match(hipdsp_ctx *ctx, const hipdsp_tmplplan *plan, const float *spec, int64_t spec_pitch,
                          int64_t channels, int64_t frames, int64_t nfreq, int64_t k0, int64_t first,
                          int64_t n_out, int db, double ref_power, double min_power, float floor, float pivot,
                          double min_std, float *out, int64_t out_pitch, int64_t out_template_pitch);

/* ---- region analysis -------------------------------------------------------- */

/* Statistics of selected regions, reduced on the device: what the reference computes after the user selects a region.
 * DataBrowser.analyze_region (src/audian/databrowser.py:1759-1775) cuts every trace to the region with
 * Data.get_region(t0, t1, channel) (src/audian/data.py:102-118) and hands the cuts to every
 * Analyzer.analyze(t0, t1, channel, traces) (src/audian/analyzer.py:100); the analyzer enabled by default,
 * StatisticsAnalyzer (src/audian/statisticsanalyzer.py:18-20), stores np.mean(source), np.std(source).
 * x is planar float32: `channels` rows of `frames` valid elements, x_pitch elements apart (0 = frames).  A spectrogram
 * slab (channels, frames', F) is the same thing with frames = frames' * F: a frame range of one channel is contiguous.
 * host_start / host_stop are HOST arrays of n_regions element ranges, 0 <= start <= stop <= frames; they travel to the
 * kernels by value: no upload, no host synchronisation.  out is a DEVICE array (n_regions, channels, 8) float64,
 * compact.  For region r, channel c and v = x[c, start:stop], out[r][c] holds
 *   [0] n = stop - start        [1] np.mean(v) (float64)    [2] np.std(v) (ddof 0)      [3] np.min(v)
 *   [4] np.max(v)               [5] np.argmin(v)            [6] np.argmax(v)            [7] 0 (reserved)
 * (positions: the first occurrence, relative to start).  Up to 16 regions per call (more: HIPDSP_ERR_UNSUPPORTED).
 * HIPDSP_ERR_INVALID: n_regions < 1, a NULL list, a range outside [0, frames] or with stop < start, more than 65535
 * channels.  channels == 0 writes nothing.  Rows and regions start at any 4-byte address; index arithmetic is 64-bit;
 * at most 2^31 - 1 chunks of 16384 elements per call, all regions together.
 * Uses the context scratch: 40 bytes per channel and 16384-element chunk, sum over the regions of
 * ceil((stop - start) / 16384) chunks (at least 40 bytes per channel) -- like hipdsp_mean_spectrum_db it may not come
 * between phase 1 and phase 2 of hipdsp_sosfilt_envelope.
 *
 * Special values (numpy's own results, tested against numpy):
 *   n == 0                 [1]-[4] NaN, [5] and [6] -1.
 *   a NaN in the region    [1]-[4] NaN, [5] and [6] the position of the first NaN.
 *   +-inf and no NaN       [2] NaN; [1] +inf, -inf, or NaN when both signs occur; [3]-[6] by ordinary comparison.
 * They are carried as flags (saw NaN, saw +inf, saw -inf, first NaN) beside the sums and resolved in the last step;
 * other channels and other regions are not affected.
 *
 * Accuracy contract for finite input.  The sums are pivot-shifted and carried in float64: with K = x[c, start],
 * d_i = x_i - K, S1 = sum d_i and S2 = sum d_i^2, mean = K + S1/n and std^2 = max(S2/n - (S1/n)^2, 0).  For EVERY
 * summation order of S1 and S2, with u = 2^-53, g = (n+3)u / (1 - (n+3)u), D1 = mean |d_i|, D2 = mean d_i^2 and mu,
 * sigma^2 the exact mean and variance of the float32 values,
 *     |mean - mu|             <= g*D1 + u*|mu|
 *     |std^2 - sigma^2| = E   <= 3g*D2 + 4u*sigma^2          (|mean d| * D1 <= D1^2 <= D2)
 *     |std - sigma|           <= min(sqrt(E), E / sigma)
 * and [0], [3]-[6] are exact.  (float32 accumulation does not satisfy this, nor does an unshifted E[x^2] - mean^2
 * under a DC offset.)
 * Determinism: no float atomics; the same call gives the same bits twice.  The chunk grid of a region is anchored at
 * the region's own start and sized by its length, and the chunks are merged in an order fixed by their count: a
 * region's eight values do not depend on which other regions ride in the call nor on how many channels it has -- a
 * 16-region call gives bit for bit what 16 one-region calls give. */
int hipdsp_region_stats(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t frames,
                        const int64_t *host_start, const int64_t *host_stop, int n_regions, double *out);

/* ---- event detection -------------------------------------------------------- */

/* Threshold events of a device-resident trace: the step between an envelope (or band-power, or kernel-filter) trace
 * and the analysis of its events' regions, the reference's open item "Add events ... / Provide interface for event
 * detectors" (README.md:66-69) as its songdetector.py does it (detect_songs, songdetector.py:113-139: threshold
 * crossings, merge_events, remove_events).  x is planar float32, `channels` rows x_pitch elements apart (x_pitch >=
 * stop, unless there is one channel); of every row the elements [start, stop) are looked at, 0 <= start <= stop.
 * The threshold of channel c is dev_thresholds[c] (a DEVICE array of `channels` floats) or, with dev_thresholds ==
 * NULL, (float)threshold for all.  min_gap >= 0 and min_len >= 0 are counts of elements.  Per row:
 *   1. above[i] = x[i] > thr, as a float32 comparison: NaN is not above, +inf is above any finite thr, a sample equal
 *      to thr is not above (and nothing is above a NaN or +inf threshold).
 *   2. A raw event is a maximal run of above samples, half-open [onset, offset).  A run that touches start or stop is
 *      reported with onset == start or offset == stop; it is not dropped -- the indices show that it is cut off.
 *   3. Two consecutive raw events are merged when next.onset - prev.offset <= min_gap, the left side being the number
 *      of not-above samples between them.  With min_gap == 0 nothing merges.
 *   4. After merging, an event is kept when offset - onset >= min_len.
 *   5. The events of a row come out in ascending order; indices are positions in the row, not relative to start.
 * thunderlab, whose merge_events / remove_events songdetector.py calls, is neither in the reference tree nor in this
 * image: steps 3 and 4 restate songdetector.py's use of them, parity with thunderlab is unpinned.  The contract is the
 * definition above; every output is an integer and tests/events_definition.py reproduces it exactly.
 * Output: counts is a DEVICE array of `channels` int64 and receives the number of events of every row, also when that
 * exceeds capacity.  events is a DEVICE array (channels, capacity, 2) int64 of (onset, offset) pairs, events_pitch
 * elements between channels (0 = 2*capacity); only the first min(count, capacity) pairs of a channel are written,
 * nothing beyond them is touched.  capacity == 0 with events == NULL is legal and gives the counts only.  stop ==
 * start gives zero counts and writes nothing else; channels == 0 writes nothing.
 * HIPDSP_ERR_INVALID: a NULL ctx, counts or (with capacity > 0) events, negative sizes, start > stop, x_pitch < stop
 * with more than one channel, events_pitch < 2*capacity, misaligned pointers.  HIPDSP_ERR_UNSUPPORTED: more than 65535
 * channels or stop - start > 2^40 elements per call.  Index arithmetic is 64-bit; rows start at any 4-byte address.
 * No host synchronisation, nothing is read back, legal inside hipdsp_graph_begin/end once the scratch is reserved.
 * Uses the context scratch: 552 bytes per channel and 4096-element chunk of [start, stop) (the above bits, 1 bit per
 * sample, and five 8-byte carries per chunk) -- like hipdsp_region_stats it may not come between phase 1 and phase 2
 * of hipdsp_sosfilt_envelope.  The trace is read once: about 4.4 bytes per sample move in all.
 * Determinism: the slot of every event comes from prefix scans over the chunks and its rank inside its chunk; there is
 * no atomic.  The same call gives the same bytes twice, and a channel's result does not depend on which other channels
 * ride in the call. */
int hipdsp_detect_events(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t start,
                         int64_t stop, const float *dev_thresholds, double threshold, int64_t min_gap,
                         int64_t min_len, int64_t capacity, int64_t *events, int64_t events_pitch, int64_t *counts);

/* ---- peak detection --------------------------------------------------------- */

/* Local maxima of a device-resident trace with their prominences: the other kind of event of the reference, "Events
 * are channel specific points. Plotted as dot at data amplitude. Many events per label. Result from some analysis."
 * (README.md:113-117), found as its songdetector.py finds them, sig.find_peaks(envelopes[:,c]) (songdetector.py:
 * 110-115).  The call is scipy.signal.find_peaks with its height, threshold, prominence and wlen arguments (pinned to
 * scipy 1.15.3 by tests/golden/find_peaks.npz).  distance, width, rel_height and plateau_size are NOT part of it:
 * distance is a greedy pass in order of height that scipy applies before the prominence; it belongs on a compacted
 * list and needs an entry point of its own.  thunderlab's detect_peaks is neither in the reference tree nor in this
 * image: parity with it is unpinned.  The contract is the definition below; tests/peaks_definition.py restates it.
 * x is planar float32, `channels` rows x_pitch elements apart (x_pitch >= stop, unless there is one channel); of every
 * row the elements v = x[c, start:stop], n = stop - start, are looked at, 0 <= start <= stop.  Every sample is
 * converted exactly to float64 and every comparison is a float64 comparison.  Per row:
 *   1. A run of equal samples v[l..r] (l <= r) is a peak when l >= 1, r <= n-2, v[l-1] < v[l] and v[r+1] < v[r]; its
 *      position is m = (l + r) / 2, rounded down.  The first and the last sample of the range are never peaks, nor is a
 *      run that reaches either end.  A NaN is never a peak and neither is a sample next to one; -0.0 == 0.0.
 *   2. Height h = v[m]: kept when hmin <= h <= hmax.
 *   3. Threshold tl = h - v[m-1], tr = h - v[m+1]: kept when tmin <= min(tl, tr) and max(tl, tr) <= tmax, a NaN
 *      difference (inf - inf) failing either comparison as in numpy.
 *   4. Prominence, scipy's peak_prominences.  lo = 0 and hi = n-1; with wlen >= 2, lo = max(m - wlen/2, 0) and hi =
 *      min(m + wlen/2, n-1) (wlen/2 rounded down; wlen 0 and 1 mean the whole range).  Left: walk i = m, m-1, ... while
 *      i >= lo and v[i] <= h (a NaN or a higher sample stops the walk); left_min is the minimum of the samples walked,
 *      left_base its position, of equal minima the one nearest to m, and m itself if nothing lower than h was walked.
 *      Right: the same with i = m, m+1, ... while i <= hi.  prominence = h - max(left_min, right_min), a float64
 *      subtraction; kept when pmin <= prominence <= pmax.
 *   5. A border that is -inf (lower) or +inf (upper) is open: that comparison is not made.  So a NaN prominence (it
 *      arises only for a +inf plateau wider than wlen) passes open borders and fails any real one; a NaN border keeps
 *      nothing; with all six borders open every local maximum is a peak.
 *   6. Peaks come out in ascending position; positions and bases are positions in the row, not relative to start.
 * The six borders hmin, hmax, tmin, tmax, pmin, pmax of channel c are dev_borders[6*c .. 6*c + 5] (a DEVICE array
 * (channels, 6) of float64) or, with dev_borders == NULL, the six arguments for all channels.
 * Output: counts is a DEVICE array of `channels` int64 and receives the number of peaks of every row, also when that
 * exceeds capacity.  peaks is a DEVICE array (channels, capacity) int64, peaks_pitch elements between channels (0 =
 * capacity).  props (optional, may be NULL) is a DEVICE array (channels, capacity, 4) float64, props_pitch elements
 * between channels (0 = 4*capacity), of [height, prominence, left_base, right_base] (the bases are exact in float64).
 * Only the first min(count, capacity) entries of a channel are written, nothing beyond them is touched.  capacity == 0
 * with peaks == NULL is legal and gives the counts only (props is ignored then).  stop == start gives zero counts and
 * writes nothing else; channels == 0 writes nothing.
 * HIPDSP_ERR_INVALID: a NULL ctx, counts or (with capacity > 0) peaks, negative sizes, a negative wlen, start > stop,
 * x_pitch < stop with more than one channel, peaks_pitch < capacity, props_pitch < 4*capacity, misaligned pointers.
 * HIPDSP_ERR_UNSUPPORTED: more than 65535 channels or stop - start > 2^40 elements per call.  Index arithmetic is
 * 64-bit; rows start at any 4-byte address.
 * No host synchronisation, nothing is read back, legal inside hipdsp_graph_begin/end once the scratch is reserved.
 * Uses the context scratch: 2584 bytes per channel and 4096-element chunk of [start, stop) (four words of bits per 64
 * samples: rise, fall, equal, kept; a float minimum and maximum per 64 samples and per chunk; two 8-byte carries per
 * chunk) plus 8 bytes per channel and 64 chunks (the top of the min/max table) -- 0.63 bytes per sample, whatever the
 * number of peaks.  Like hipdsp_region_stats it may not come between phase 1 and phase 2 of hipdsp_sosfilt_envelope.
 * Work: the trace is read once for the maxima.  The prominence search runs only for peaks that passed height and
 * threshold, and only when a prominence border is closed (in the counting pass) or props is given (in the storing
 * pass, for the peaks kept and below capacity); with open prominence borders and no props no search runs and the
 * min/max table is not built.  A search is one thread's: per side it reads at most 127 samples, 126 + 126 entries of
 * the two lower table levels (64 and 4096 samples) and (stop - start) / 262144 entries of the top level, then 192
 * values to place the base -- some 800 reads per side at 2^26 samples, which the highest peaks of a row pay and a
 * typical peak of white noise (a higher sample a few samples away) does not.  The lanes of a wave search in turn for
 * the peaks of their 64 samples, so a wave takes as long as its slowest lane.
 * Determinism: the slot of every peak comes from prefix scans over the chunks and its rank inside its chunk; there is
 * no atomic and no float reduction whose order could vary (minima and maxima are exact).  The same call gives the same
 * bytes twice, and a channel's result does not depend on which other channels ride in the call. */
int hipdsp_find_peaks(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t start, int64_t stop,
                      const double *dev_borders, double hmin, double hmax, double tmin, double tmax, double pmin,
                      double pmax, int64_t wlen, int64_t capacity, int64_t *peaks, int64_t peaks_pitch, double *props,
                      int64_t props_pitch, int64_t *counts);

/* ---- amplitude histograms and moments inside an amplitude window ----------- */

/* The two reductions of the reference's histogram threshold (threshold_estimates, songdetector.py:85-117): a 49-bin
 * amplitude histogram per channel between 0 and the global maximum, mean and std of the samples below a bin edge
 * derived from the histogram's mode, the mean of the samples above mean + 3 std, and from these 0.5*(mean + uppermean)
 * or maxe + std.  BufferedData.threshold_estimates (audian_amd/buffereddata.py) builds that function on the two calls
 * below and hipdsp_region_stats (for the maximum); the integer bookkeeping between them runs on the host.
 *
 * hipdsp_histogram.  x is planar float32, `channels` rows x_pitch elements apart (x_pitch >= stop, unless there is one
 * channel); of every row the elements [start, stop) are looked at, 0 <= start <= stop.  host_edges is a HOST array of
 * n_bins + 1 finite, non-decreasing float64 values e[0..B], B = n_bins, 1 <= n_bins <= 1024.  The edges travel to the
 * kernels by value (256 per launch of a small kernel that stores them in the context scratch): the array is consumed
 * when the call returns, there is no upload and no host synchronisation, and the call is legal inside
 * hipdsp_graph_begin/end once the scratch is reserved (a replay counts with the edges of capture time).
 * out is a DEVICE array (channels, n_bins + 3) of int64, out_pitch elements between channels (0 = n_bins + 3), aligned
 * to 8 bytes; the call overwrites all n_bins + 3 slots of every channel and touches nothing else.
 * Counts are those of np.histogram(v.astype(float64), bins=edges), which is this rule: a sample x, converted exactly to
 * float64, is counted in a bin when e[0] <= x <= e[B], and its bin is the number of interior edges e[1..B-1] that are
 * <= x.  So every bin is [e[i], e[i+1]), the last bin is closed on the right, and a bin of zero width is empty unless it
 * is the last one and x == e[B].  Three more slots take the rest:
 *   out[c][B]     samples < e[0], -inf included
 *   out[c][B+1]   samples > e[B], +inf included
 *   out[c][B+2]   NaN samples
 * so every row of out sums to stop - start.  All comparisons are float64 comparisons of exactly converted samples with
 * the edges as given (the library is built without floating-point contraction); a first guess of the bin from
 * (x - e[0]) * B / (e[B] - e[0]) is corrected against e[k] and e[k+1] until the rule holds, so the result is exact for
 * any edges and costs O(1) for uniform ones.
 * HIPDSP_ERR_INVALID: a NULL ctx, host_edges or out, a decreasing or non-finite edge, n_bins < 1, negative sizes,
 * start > stop, x_pitch < stop with more than one channel, out_pitch < n_bins + 3 (other than 0), misaligned pointers.
 * HIPDSP_ERR_UNSUPPORTED: n_bins > 1024, more than 65535 channels.  stop == start writes zeros; channels == 0 writes
 * nothing.  Index arithmetic is 64-bit; rows start at any 4-byte address; at most 2^31 - 1 chunks of 16384 elements
 * per row.  The trace is read once.
 * Uses the context scratch: 8 * (n_bins + 1) bytes (the edges) -- like hipdsp_region_stats it may not come between
 * phase 1 and phase 2 of hipdsp_sosfilt_envelope.
 *
 * hipdsp_masked_stats.  x, x_pitch, channels, start, stop as above.  dev_bounds is a DEVICE array (channels, 3) of
 * float64: lo, hi, pivot of every channel.  A sample is selected when lo < x < hi, x converted exactly to float64, both
 * comparisons strict; lo = -inf or hi = +inf switches that side off.  NaN samples and infinite samples are never
 * selected; a NaN bound selects nothing.  out is a DEVICE array (channels, 4) of float64, compact:
 *   [0] the number of selected samples    [1] their mean    [2] their std (ddof 0)    [3] 0 (reserved)
 * With nothing selected (also stop == start) [1] and [2] are NaN.  pivot must be finite ([1] and [2] mean nothing
 * otherwise); a good pivot is a value near the selected samples, such as the finite one of the two bounds.
 * HIPDSP_ERR_INVALID: a NULL ctx, dev_bounds or out, negative sizes, start > stop, x_pitch < stop with more than one
 * channel, misaligned pointers.  HIPDSP_ERR_UNSUPPORTED: more than 65535 channels.  channels == 0 writes nothing.
 * No host synchronisation, nothing is read back, legal inside hipdsp_graph_begin/end once the scratch is reserved.
 * Uses the context scratch under the same rule: 24 bytes per channel and 16384-element chunk of [start, stop) (at
 * least 24 bytes per channel).
 *
 * Accuracy contract of hipdsp_masked_stats for finite selected samples -- the one of hipdsp_region_stats with K =
 * pivot.  The sums are pivot-shifted and carried in float64: over the n selected samples d_i = x_i - K, S1 = sum d_i,
 * S2 = sum d_i^2, mean = K + S1/n and std^2 = max(S2/n - (S1/n)^2, 0).  For EVERY summation order of S1 and S2, with
 * u = 2^-53, N = stop - start, g = (N+3)u / (1 - (N+3)u) (N, not n: an unselected sample adds an exact zero to both
 * sums, which costs no accuracy but is a term of the sum), D1 = mean |d_i|, D2 = mean d_i^2 and mu, sigma^2 the exact
 * mean and variance of the selected float32 values,
 *     |mean - mu|             <= g*D1 + u*|mu|
 *     |std^2 - sigma^2| = E   <= 3g*D2 + 4u*sigma^2
 *     |std - sigma|           <= min(sqrt(E), E / sigma)
 * and [0] is exact.
 *
 * Determinism, both calls: no float atomics.  The histogram's only atomics are integer adds (32-bit in LDS, one 64-bit
 * add per non-empty bin and workgroup to out), whose sums do not depend on arrival order; the float64 sums of
 * hipdsp_masked_stats are merged in an order fixed by the number of chunks.  The chunk grid is anchored at `start`:
 * the same call gives the same bytes twice, and a channel's row does not depend on which other channels ride in the
 * call. */
int hipdsp_histogram(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t start, int64_t stop,
                     const double *host_edges, int n_bins, int64_t *out, int64_t out_pitch);
int hipdsp_masked_stats(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t start,
                        int64_t stop, const double *dev_bounds, double *out);

/* ---- event spectra ---------------------------------------------------------- */

/* Welch power spectral densities of many regions in one call: the frequency content of detected events, the step that
 * follows event detection in the reference's songdetector.py (env_freqs, songdetector.py:146-152, called at :761: the
 * power spectrum of the envelope inside every song and its main peak, the pulse rate; on the filtered trace the same
 * gives the carrier of every call).  thunderlab, whose psd and peak_freqs songdetector.py calls, is neither in the
 * reference tree nor in this image: its choice of nfft and its peak detector are restated (audian_amd/spectra.py),
 * parity with thunderlab is unpinned.  The contract is the definition below; tests/spectra_definition.py restates it
 * and tests/golden/region_spectra.npz pins it to scipy.signal.welch (scipy 1.15.3).
 * x is planar float32: `channels` rows of `frames` valid elements, x_pitch elements apart (0 = frames).  host_regions is
 * a HOST array (n_regions, 3) of int64: channel, start, stop, with 0 <= channel < channels and 0 <= start <= stop <=
 * frames; regions may overlap or repeat.  nfft is a power of two in [8, 8192], 1 <= hop <= nfft, step >= 1, fs > 0.
 * Per region, with v = x[channel, start:stop:step] (len(v) = ceil((stop - start) / step)) converted exactly to float64:
 *   n_frames = (len(v) - nfft) / hop + 1 (rounded down) when len(v) >= nfft, else 0; frame k is v[k*hop : k*hop + nfft];
 *   the samples behind the last whole frame are not used (and not read).
 *   Per frame, exactly what hipdsp_spectrogram does per frame: subtract the frame's mean, multiply by the periodic Hann
 *   window w[i] = 0.5 - 0.5 cos(2 pi i / nfft), take the real transform X, P = |X|^2 / (fs * sum w^2), bins 1 ... F-2
 *   doubled, F = nfft/2 + 1.
 *   The region's row is the mean of its frames' P: scipy.signal.welch(v, fs, 'hann', nperseg=nfft, noverlap=nfft - hop,
 *   detrend='constant', scaling='density').  fs is taken as given (the rate of v, not of x).
 * out is a DEVICE array (n_regions, F) float32, out_pitch elements between rows (0 = F); info is a DEVICE array
 * (n_regions, 2) of int64 and receives n_frames and np.argmax(row), the first position of the largest stored value.
 * Special values:
 *   n_frames == 0                           a row of NaN, argmax -1.
 *   a NaN or +-inf in a sample of a frame   the whole row NaN, argmax 0 (numpy's argmax of an all-NaN row); other
 *                                           regions are not affected, nor is the region by such samples behind its last
 *                                           whole frame.
 *   every used frame constant               the row is exactly 0.0 (the mean of equal samples is exact in float64).
 * HIPDSP_ERR_INVALID: a NULL ctx, an nfft that is not a power of two in [8, 8192], hop outside [1, nfft], step < 1, fs
 * not positive and finite, negative sizes, x_pitch < frames, out_pitch < F (other than 0), a NULL table or output, a
 * region with its channel outside [0, channels) or its range outside [0, frames] or with stop < start, misaligned
 * pointers, more than 2^31 - 1 frame groups in all.  All of this is decided on the host before anything is launched.
 * n_regions == 0 writes nothing.
 * The call reads host memory (the table) and uploads it itself, waiting once for the context's stream while the copy
 * completes: it is NOT legal inside hipdsp_graph_begin/end (HIPDSP_ERR_INVALID there).
 * Work: a flat list of (region, frame group) items, sized exactly from the table -- a group is 16 consecutive frames of
 * one region, counted from the region's first frame -- one workgroup per item, so short events launch nothing for long
 * ones.  Only samples of the listed regions are read, each at most ceil(nfft / hop) times per region that holds it.  A
 * workgroup transforms its frames one after the other in LDS (a complex radix-2 Stockham transform of nfft/2 points and a
 * split step, twiddles and window from one float32 table built once per workgroup from float64 values; 12 * nfft bytes
 * of LDS) and keeps the bins' running sums on chip, in float64: no spectrum of a single frame goes to memory.  The frame
 * mean is summed and subtracted in float64 before the sample is rounded to float32, so a DC offset of 10^4 times the
 * signal costs nothing.  A second launch, one workgroup per region, merges the groups' partial rows in ascending order.
 * Uses the context scratch: 32 * (n_regions + 1) bytes (the table) plus 8 * (F + 1) bytes per frame group (one float64
 * partial row and the group's flag), sum over the regions of ceil(n_frames / 16) groups -- like hipdsp_region_stats it
 * may not come between phase 1 and phase 2 of hipdsp_sosfilt_envelope.
 * Accuracy: every frame's spectrum meets the per-bin bound every spectrogram kernel is held to (tests/spectral_bound.py:
 * |a^ - a| <= beta_max * eps * (a + log2(nfft) * r) in amplitudes); the row adds the float64 mean and one rounding to
 * float32.  tests/test_gpu_regionspectra.py holds every bin to the bound that follows.
 * Determinism: no atomics.  Frame groups are anchored at the region's first frame and sized by a constant, and partial
 * rows are merged in an order fixed by their count: a region's row and info depend on its samples and on (nfft, hop,
 * step, fs) only -- not on which other regions ride in the call, on their order, on n_regions or on channels -- and the
 * same call gives the same bytes twice.  Index arithmetic is 64-bit; rows and regions start at any 4-byte address. */
int hipdsp_region_spectra(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t frames,
                          const int64_t *host_regions, int64_t n_regions, int nfft, int hop, int64_t step, double fs,
                          float *out, int64_t out_pitch, int64_t *info);

/* ---- event refinement ------------------------------------------------------- */

/* Zero-phase filtering of many regions in one call, every region with a filter of its own: the step behind the pulse
 * rates in the reference's songdetector.py (filter_envelopes, songdetector.py:178-192, called at :765: the envelope
 * inside every widened song is smoothed by lowpass_filter -- scipy.signal.filtfilt(*butter(1, Wn), v) -- at four times
 * that song's own pulse rate, in place).
 * x and y are planar float32: `channels` rows of `frames` valid elements, x_pitch / y_pitch elements apart (0 = frames).
 * host_regions is a HOST array (n_regions, 3) of int64: channel, start, stop, with 0 <= channel < channels and 0 <=
 * start <= stop <= frames.  host_sos is a HOST array (n_regions, n_sections, 6) of float64 rows [b0 b1 b2 1 a1 a2]:
 * region r is filtered with host_sos[r]; n_sections is shared by the call and is 1 or 2.
 * Per region, with v = x[channel, start:stop] converted exactly to float64:
 *   y[channel, start:stop] = float32(scipy.signal.sosfiltfilt(sos_r, v))       default padtype 'odd', default padlen
 * that is: padlen = 3 * (2 n_sections + 1 - min(#sections with b2 == 0, #sections with a2 == 0)); the odd extension
 * 2 v[0] - v[padlen:0:-1] | v | 2 v[-1] - v[-2:-padlen-2:-1]; a forward pass from sosfilt_zi * ext[0]; reversal; a
 * forward pass from sosfilt_zi * (its first sample); reversal; the extension trimmed.  tests/iir_bound.py restates it
 * (sosfiltfilt with gain 1, no rectification, no clamp).  For the reference's filter, butter(1, Wn) as ONE section with
 * b2 = a2 = 0 (padlen 6), this is scipy.signal.filtfilt(b, a, v); tests/golden/region_filtfilt.npz pins both to scipy
 * 1.15.3.  With clamp != 0 negative results become 0.  No other element of y is written.
 * y == x with equal pitches is legal (the reference filters in place): x is read by the forward pass only, which is
 * complete before the backward pass writes.  Otherwise x and y must not overlap.
 * Errors, all decided on the host before anything is launched or written:
 *   HIPDSP_ERR_TOO_SHORT    a region with stop - start <= padlen(sos_r) (scipy raises ValueError).
 *   HIPDSP_ERR_INVALID      a NULL argument; a0 != 1; a coefficient that is not finite; a section whose poles are not
 *                           inside the unit circle (|a2| < 1 and |a1| < 1 + a2 fail); a region outside [0, frames] or with
 *                           stop < start; a channel outside [0, channels); two regions of one channel that overlap (two
 *                           writers; stop == next start is fine); pitches below frames; misaligned pointers; x and y
 *                           that overlap other than y == x with equal pitches; a call inside hipdsp_graph_begin/end (the
 *                           call reads the host tables and uploads them itself, waiting once for the context's stream,
 *                           like hipdsp_region_spectra).
 *   HIPDSP_ERR_UNSUPPORTED  n_sections outside 1 ... 2.
 * n_regions == 0 writes nothing.
 * Non-finite samples: a region that holds a NaN or +-inf sample comes out all NaN; other regions are not affected.
 * (scipy gives NaN or infinities there, depending on the filter: an infinity times a zero coefficient, or the difference
 * of two infinities, is what decides.)
 * Accuracy: float64 coefficients and state, ONE rounding to float32.  The extension is formed in float64 from the
 * exactly converted samples and the forward pass reaches the backward pass as float64, so the contract is the one of
 * tests/iir_bound.py without its extension_term and between_term: e_w <= (1 + 16 q) 2^-24 r_w for every window of 64
 * samples counted from the region's own start, q the case's allowance.  A region's history starts at its own extension:
 * there is no warm-up.  Where the extended sequence is cut into chunks the state is handed over exactly, state_out =
 * A^L state_in + (the zero-state end state of the L samples), in float64 -- over a chunk, over the 1, 2, 4 ... 32 chunks
 * of a scan over a tile's lanes, and over a tile; the powers of A are computed on the host (squared in long double,
 * each rounded once).
 * Work: the extended sequence of a region (E = stop - start + 2 padlen samples) is cut into chunks of 64 samples
 * counted from its first sample -- for the backward pass from its last -- and 64 consecutive chunks are the tile of one
 * wave; the flat list of (region, tile) items is sized exactly from the table.  Per direction three launches: every
 * chunk's zero-state end state (one lane per chunk, the tile staged in LDS with coalesced loads) and a scan of them over
 * the tile's lanes; one thread per region walking the tiles' hand-overs; every chunk again from its true state, writing.
 * Uses the context scratch: 1072 * (n_regions + 1) + 8 * n_regions bytes (the table and one flag per region) plus, summed
 * over the regions, 8 * E bytes (the forward pass, float64) and 16 * n_sections * (ceil(E / 64) + ceil(E / 4096)) bytes
 * (the states of the chunks and of the tiles) -- like hipdsp_region_stats it may not come between phase 1 and phase 2 of hipdsp_sosfilt_envelope.
 * Determinism: no atomics.  The chunk grid is anchored at the first (last) sample of the region's extended sequence and
 * sized by a constant: a region's output depends on its samples, its filter and clamp only -- not on which other regions
 * ride in the call, on their order, on n_regions or on channels -- and the same call gives the same bytes twice.  Index
 * arithmetic is 64-bit; rows and regions start at any 4-byte address. */
int hipdsp_region_filtfilt(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, float *y, int64_t y_pitch,
                           int64_t channels, int64_t frames, const int64_t *host_regions, int64_t n_regions,
                           const double *host_sos, int n_sections, int clamp);

/* Threshold crossings and the maximum of many regions in one call, one threshold per REGION: the device step of the
 * reference's analyse_songs (songdetector.py:195-244, called at :767): the largest envelope value in the noise windows
 * beside every song gives a local threshold, and the song's borders are found again as the first and last sample above
 * it inside the widened song.
 * x and host_regions are as in hipdsp_region_filtfilt; regions may overlap or repeat.  host_thresholds is a HOST array
 * of n_regions float64.  out is a DEVICE array (n_regions, 8) of float64, compact.  For v = x[channel, start:stop]:
 *   [0] n = stop - start    [1] number of samples above      [2] position of the first sample above, -1 if none
 *   [3] one past the position of the last sample above, -1   [4] np.max(v)     [5] np.argmax(v) as a position in the row
 *   [6], [7] 0 (reserved)
 * "Above" is rule 1 of hipdsp_detect_events: x[i] > (float)threshold as a float32 comparison; NaN is not above, a
 * sample equal to the threshold is not above, nothing is above a NaN or +inf threshold -- so a call with NaN
 * thresholds gives the maxima alone.  Positions are positions in the row, as in hipdsp_detect_events.  [4] and [5]
 * follow hipdsp_region_stats: a NaN in the region gives NaN and the first NaN's position, n == 0 gives NaN and -1,
 * otherwise the first occurrence of the largest value.  Everything is exact.
 * HIPDSP_ERR_INVALID: a NULL argument, negative sizes, x_pitch < frames, a region outside [0, frames] or with stop <
 * start, a channel outside [0, channels), misaligned pointers, a call inside hipdsp_graph_begin/end (the call reads the
 * host tables and uploads them itself, waiting once for the context's stream); all decided on the host before anything
 * is launched.  n_regions == 0 writes nothing.
 * Work: one workgroup per chunk of 4096 samples counted from the region's start, then one thread per region merging its
 * chunks in ascending order.  Uses the context scratch: 40 * (n_regions + 1) bytes (the table) plus 24 bytes per chunk,
 * sum over the regions of ceil(n / 4096) chunks, under the same rule as above.
 * Determinism: no atomics; a region's eight values depend on its samples and its threshold only, and the same call
 * gives the same bytes twice. */
int hipdsp_region_crossings(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t frames,
                            const int64_t *host_regions, const double *host_thresholds, int64_t n_regions, double *out);

/* The windowed cross-correlation coefficient of many regions against a list of partner channels, over the lags -L ... L:
 * which channel an event belongs to and how much later it arrives elsewhere.  The reference has no code for this; its
 * songdetector.py ends on the problem ("crosstalk in front of songs in trace 0").  The contract is pinned to numpy.
 * x and host_regions are as in hipdsp_region_spectra: planar float32, `channels` rows of `frames` valid elements, x_pitch
 * apart (0 = frames); a HOST array (n_regions, 3) of int64 channel, start, stop with 0 <= channel < channels and 0 <= start
 * <= stop <= frames.  Regions may overlap or repeat; an empty region is allowed.  host_partners is a HOST list of n_partners
 * channel ids in [0, channels); repeats are allowed, and so is the region's own channel.  L = max_lag, 0 <= L <= 1024, W =
 * 2 L + 1.  out is a DEVICE array (n_regions, n_partners, W) float32, its rows out_pitch elements apart (0 = W); info is a
 * DEVICE array (n_regions, n_partners, 4) float64, compact.
 * For region (c, start, stop), partner p and lag l in [-L, L], with n = stop - start, a = float64(x[c, start:stop]) and
 * b_l = float64(x[p, start+l : stop+l]):
 *   lag l is VALID iff n >= 1, start + l >= 0 and stop + l <= frames.  An invalid lag gives out[.., L + l] = NaN; no
 *   sample outside [0, frames) of a row is ever read.
 *   For a valid lag out[.., L + l] = float32(clamp(r, -1, 1)), r = cov(a, b_l) / (std(a) std(b_l)) with population
 *   moments: np.corrcoef(a, b_l)[0, 1].
 *   r is NaN where the computed variance of a or of b_l is 0: a constant window (numpy gives NaN there too).
 *   A NaN or +-inf among the samples of a makes the whole row NaN; one among the samples of b_l makes that lag NaN.
 *   info[.., 0]  the number of lags whose value is not NaN
 *   info[.., 1]  the position in [0, W) of the largest value that is not NaN, first occurrence, or -1
 *   info[.., 2]  std(a); NaN for n == 0 and for a window with a NaN or +-inf
 *   info[.., 3]  std(b_l) at the position [1], NaN when [1] is -1
 * Sign convention: a POSITIVE peak lag means the partner carries the same waveform LATER -- x[p, i + l] ~ x[c, i] -- so
 * the event's channel leads.
 * Errors, all decided on the host before anything is launched or written:
 *   HIPDSP_ERR_INVALID      a NULL argument; negative sizes; x_pitch < frames; out_pitch < W (other than 0); a region with
 *                           its channel outside [0, channels) or its range outside [0, frames] or with stop < start; a
 *                           partner outside [0, channels); max_lag < 0; misaligned pointers; more than 2^31 - 1 work items
 *                           or (region, partner) pairs; a call inside hipdsp_graph_begin/end (the call reads the host
 *                           tables and uploads them itself, waiting once for the context's stream, like
 *                           hipdsp_region_spectra).
 *   HIPDSP_ERR_UNSUPPORTED  max_lag > 1024.
 * n_regions == 0 or n_partners == 0 writes nothing.
 * Non-finite samples are carried as flags beside the sums, not left to inf - inf: a sample that is not finite enters the
 * sums as a NaN, which no float64 sum loses, so "the window of a (of b_l) held one" is exactly "its sum of samples is NaN";
 * the event window's flag is stored as such, a lag's is its NaN sum, and nothing else of a flagged row or lag is used.  Other
 * lags, partners and regions are not affected.  A pivot (below) that is not finite is replaced by 0.
 * Accuracy contract for finite input.  The sums are pivot-shifted and carried in float64, as in hipdsp_region_stats: with
 * K_a = x[c, start], K_b = x[p, start], d = a - K_a, e = b_l - K_b (each one rounding to float64),
 *   A1 = sum d, A2 = sum d^2, B1[l] = sum e, B2[l] = sum e^2, C[l] = sum d e        full sums per lag, fma for the products
 *   va = max(A2/n - (A1/n)^2, 0), vb[l] likewise, cov = C/n - (A1/n)(B1/n), r = cov / (sqrt(va) sqrt(vb))
 * For EVERY summation order, with u = 2^-53, g = (n+3)u / (1 - (n+3)u), D2 = mean d^2, E2 = mean e^2 (exact, of the exact
 * shifted samples), sigma_a^2, sigma_b^2, cov the exact moments:
 *     |va^ - sigma_a^2| = Ea  <= 4g*D2 + u*sigma_a^2          |vb^ - sigma_b^2| = Eb  <= 4g*E2 + u*sigma_b^2
 *     |cov^ - cov|      = Ec  <= 4g*sqrt(D2*E2) + u*|cov|     (mean |d e| <= sqrt(D2 E2); |mean d| |mean e| likewise)
 *     eta = (1 + Ea/sigma_a^2)(1 + Eb/sigma_b^2)(1 + u)^4 - 1                  the denominator is within 1 +- eta, eta < 1
 *     |r^ - r| (1 + 2^-24) <= T = (1 + 2^-24) (Ec / (sigma_a sigma_b) + |r| eta) / (1 - eta)
 * (each sum of n products carries n + 2 roundings, (1+u)^(n+2) <= 1 + g; the two means enter cov with 2g + g^2; the
 * divisions by n, the product of the means and the subtraction add less than g between them; the clamp moves r^ only
 * towards [-1, 1], where r lies.)  The stored value adds ONE rounding to float32, of r^: |out - r| <= 2^-24 |r^| + |r^ - r| <=
 * 2^-24 |r| + T, which is why T carries the factor 1 + 2^-24.
 * tests/xcorr_definition.py restates T; for every input of tests/test_gpu_region_xcorr.py T < 2^-30.  (float32 sums at n =
 * 65536 under a DC offset are off by a hundred float32 roundings.)  info[2] and info[3] meet hipdsp_region_stats' bound on
 * the standard deviation with Ea, Eb above; info[0] and [1] are exact functions of the stored row.
 * Work (csrc/regionxcorr.hip): a flat list of (region, partner, chunk) items sized exactly from the table -- a chunk is
 * 65536 consecutive samples of the event window counted from start -- one workgroup per item, so short events launch
 * nothing for long ones.  A workgroup takes its chunk in tiles of 2048 samples: the tile of a and the 2048 + (valid lags) - 1
 * samples of b it meets are converted and shifted ONCE and kept in LDS as float64; a thread owns 9 consecutive lags and a
 * segment of the tile and feeds 27 float64 accumulators from registers.  Only the valid lags are staged and computed: the
 * cost follows the lags asked for.  A second launch, one workgroup per (region, partner), adds the chunks in ascending
 * order and forms the row and its info.  Per partner each sample of a is read once and each sample of b (2048 + valid lags - 1) / 2048 times.
 * Uses the context scratch: 48 * (n_regions + 1) + 4 * n_partners bytes (the tables), rounded up to a multiple of 8, plus
 * 8 * (4 + 27 * ceil(W / 9)) bytes per item (the float64 partial row), n_partners * sum over the regions of ceil(n /
 * 65536) items -- like hipdsp_region_stats it may not come between phase 1 and phase 2 of hipdsp_sosfilt_envelope.
 * Determinism: no atomics.  The chunk and tile grids are anchored at the region's own start and sized by constants, the
 * split of a tile among threads depends on max_lag alone, and tiles, segments and chunks are added in ascending order: a
 * (region, partner) row and its info depend on those two rows' samples, on frames and on max_lag only -- not on which
 * other regions or partners ride in the call, on their order, or on channels -- and the same call gives the same bytes
 * twice.  Index arithmetic is 64-bit; rows start at any 4-byte address. */
int hipdsp_region_xcorr(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t frames,
                        const int64_t *host_regions, int64_t n_regions, const int *host_partners, int n_partners,
                        int max_lag, float *out, int64_t out_pitch, double *info);

/* The power envelope at the envelope rate: the first step of the reference's song detector, envelope()
 * (songdetector.py:57-69) -- the squares of a band-passed trace, a zero-phase low-pass of them, every step-th sample, the
 * clamp at zero and the root -- in one call that never writes anything at full rate.
 * x is planar float32: `channels` rows of `frames` valid elements, x_pitch apart; y: `channels` rows of n_out elements,
 * y_pitch apart.  For one row v and the plan's table sos (one or two sections):
 *   u    = float64(v)**2                                        exact
 *   f    = scipy.signal.sosfiltfilt(sos, u)                     default odd extension OF u by the default padlen, forward
 *                                                               pass from sosfilt_zi * ext[0], reversal, forward pass from
 *                                                               sosfilt_zi * (its first sample), reversal, trim
 *   p[j] = float32(gain * max(f[first + j step], 0)), j < n_out the product in float64, ONE rounding
 *   y[j] = p[j] (root == 0), the correctly rounded float32 square root of p[j] (root != 0)
 * tests/power_envelope_definition.py restates it.  The reference's envelope(data, rate, freq) is root = 1, gain = 4
 * (sqrt(2 f) sqrt(2) = 2 sqrt(f)), first = 0, step = round(rate / min(10 freq, rate)), n_out = ceil(frames / step), with the
 * plan of butter(1, freq) as ONE section with b2 = a2 = 0 (padlen 6: scipy.signal.filtfilt(b, a, u)); its edata[::step] is
 * root = 0, gain = 2.  tests/golden/power_envelope.npz pins both to the reference's own function.
 * Errors, all decided on the host before anything is launched or written:
 *   HIPDSP_ERR_TOO_SHORT    frames <= padlen (scipy raises ValueError).
 *   HIPDSP_ERR_UNSUPPORTED  a plan of more than two sections; more than 65535 channels or 2^40 frames.
 *   HIPDSP_ERR_INVALID      step < 1; first < 0; first + (n_out - 1) step >= frames with n_out > 0; a gain that is not
 *                           finite or <= 0; a NULL ctx or plan (or a plan never set); negative sizes; x_pitch < frames or
 *                           y_pitch < n_out; misaligned pointers; y overlapping x; a stream capture in progress (the call
 *                           sizes its scratch itself).
 * n_out == 0 or channels == 0 writes nothing.  Nothing outside y[c y_pitch + j], j < n_out, is written.
 * Non-finite samples: a row that holds a NaN or an infinity comes out NaN in every element; other rows keep their bits.
 * (For infinities scipy gives NaN or infinities depending on the filter, as in hipdsp_region_filtfilt.)
 * Accuracy: squares, extension, coefficients, state, every hand-over and the forward output that feeds the backward pass
 * are float64; one rounding to float32 at the store, then the root.  The contract is the one of tests/iir_bound.py without
 * its extension_term and between_term: with root = 0, gain = 1, step = 1, e_w <= (1 + 16 q) 2^-24 r_w for every window of 64
 * samples, q the case's allowance.  There is no warm-up: where the extended sequence is cut the state is handed over
 * exactly, state_out = A^L state_in + (the zero-state end state of the L samples), the powers of A computed on the host
 * (squared in long double, each rounded once).  hipdsp_ctx_set_max_segments has nothing to reach: rows are not cut into
 * segments that could start anywhere but at the row's own extension.
 * Work (csrc/powerenv.hip): the extended sequence of a row (E = frames + 2 padlen samples) is cut into chunks of 64 samples
 * counted from its first sample, 64 consecutive chunks are the tile of one wave.  Three sweeps over x and two carries: every
 * chunk's zero-state end state and a scan over the tile's lanes; one wave per row handing the tiles' states on, 64 tiles
 * per step; every chunk's forward output again from its true state, kept in registers, run backwards from zero state and
 * scanned; the backward hand-over; the same again from the true states, writing the samples on the grid.  12 bytes read
 * per sample, 4 / step written.  Uses the context scratch: 32 S bytes per chunk slot (64 per tile) and per tile plus 4 per
 * row, S the number of sections -- S / 2 bytes per sample; like every call that uses the scratch, not between phase 1 and
 * phase 2 of hipdsp_sosfilt_envelope.
 * Determinism: no atomics.  The grid is anchored at the row's own extended sequence and sized by constants: a row's bytes
 * depend on the row, the plan and (first, step, n_out, gain, root) alone, and the same call gives the same bytes twice.
 * Index arithmetic is 64-bit; rows start at any 4-byte address. */
int hipdsp_power_envelope(hipdsp_ctx *ctx, const hipdsp_sosplan *plan, const float *x, int64_t x_pitch,
                          int64_t channels, int64_t frames, int64_t first, int64_t step, int64_t n_out,
                          double gain, int root, float *y, int64_t y_pitch);

/* ---- multi-GPU exchange ---------------------------------------- */

/* One process per GPU, channels sharded in contiguous blocks of the planar layout, so
 * the merged spectrogram tile is ONE all-gather of contiguous per-rank chunks (RCCL over
 * xGMI).  Rank 0 obtains a 128-byte id (hipdsp_comm_unique_id) and hands it to the other
 * ranks by whatever channel the host has (file, socket, torch store); every rank then
 * creates its communicator.  RCCL is loaded on first use. */
#define HIPDSP_UNIQUE_ID_BYTES 128
typedef struct hipdsp_comm hipdsp_comm;
int hipdsp_comm_unique_id(void *id_out);
int hipdsp_comm_create(hipdsp_ctx *ctx, const void *unique_id, int rank, int nranks,
                       hipdsp_comm **out);
int hipdsp_comm_destroy(hipdsp_ctx *ctx, hipdsp_comm *comm);
/* recv[r*count : (r+1)*count] = rank r's send[0:count], on the context's stream. */
int hipdsp_allgather_f32(hipdsp_ctx *ctx, hipdsp_comm *comm, const float *send, float *recv,
                         int64_t count_per_rank);

/* ---- measurement aid ("also report a measured device-copy ceiling") ---- */

/* dst[0:bytes] = src[0:bytes] by the copy pattern that reaches this part's streaming ceiling: one float4 per
 * thread, 256-thread blocks, no loop (MI355X_MICROARCH.md: 6.29 TB/s read + write; grid-stride copies and
 * hipMemcpy D2D stay at 4.7-5.1).  bytes must be a multiple of 16; the buffers must not overlap.  bench.py
 * times it as `roofline.device_copy_GBps`. */
int hipdsp_copy_probe(hipdsp_ctx *ctx, void *dst, const void *src, size_t bytes);

/* ---- synthetic input (bench / tests) --------------------------- */

/* x[c, t] = 0.5*u(seed, c, t) + 0.5*sin(2*pi*1000*(1 + (c0 + c)/c_total)*t/rate),
 * u uniform in [-1, 1) from a counter-based hash; generated on device. */
int hipdsp_synth(hipdsp_ctx *ctx, float *x, int64_t x_pitch, int64_t channels,
                 int64_t frames, double rate, uint64_t seed, int64_t c0, int64_t c_total);

#ifdef __cplusplus
}
#endif
#endif /* HIP_DSP_H */
