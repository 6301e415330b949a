// plan_stage.h -- the staged block behind the device-resident plans (hipdsp_sosplan, hipdsp_firplan, hipdsp_tmplplan):
// a pinned host block the plan is written into, a device block of the same size the kernels read, and the event of
// the last upload, which says when the host block may be written again.  Host only, no device code.
#pragma once
#include "common.h"

struct hd_plan_stage {
    void *host;            // pinned
    void *dev;
    size_t bytes;          // of either block
    hipEvent_t uploaded;   // behind the last upload that was not captured
    bool valid;            // `uploaded` has been recorded
};

// NULL-safe, and safe on a stage whose creation failed; what the stream still reads of the blocks is waited for
static inline void hd_stage_destroy(hipdsp_ctx *ctx, hd_plan_stage *s)
{
    if (!s) return;
    (void)hipStreamSynchronize(ctx->stream);
    if (s->uploaded) (void)hipEventDestroy(s->uploaded);
    if (s->host) (void)hipHostFree(s->host);
    if (s->dev) (void)hipFree(s->dev);
    *s = hd_plan_stage{};
}

// Both blocks of `bytes` and the event, the host block zeroed.  zero_dev: the device block too -- on the context's
// stream and waited for, so ordered before every later upload and launch, whatever kind of stream it is (for plans
// whose uploads copy a prefix only).  A step that fails frees what the steps before it made.
static inline int hd_stage_create(hipdsp_ctx *ctx, hd_plan_stage *s, size_t bytes, bool zero_dev)
{
    *s = hd_plan_stage{};
    s->bytes = bytes;
    hipError_t e = hipHostMalloc(&s->host, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&s->dev, bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->uploaded, hipEventDisableTiming);
    if (e == hipSuccess) memset(s->host, 0, bytes);
    if (e == hipSuccess && zero_dev) e = hipMemsetAsync(s->dev, 0, bytes, ctx->stream);
    if (e == hipSuccess && zero_dev) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) hd_stage_destroy(ctx, s);
    HD_CHECK_HIP(e);
    return HIPDSP_OK;
}

// the previous upload must have left the pinned block before it is rewritten
static inline int hd_stage_host_free(hd_plan_stage *s)
{
    if (s->valid) HD_CHECK_HIP(hipEventSynchronize(s->uploaded));
    return HIPDSP_OK;
}

// The first n bytes, on the context's stream.  Inside a capture no event can be recorded: `uploaded` and `valid` stay
// what the last upload outside one left.
static inline int hd_stage_upload(hipdsp_ctx *ctx, hd_plan_stage *s, size_t n)
{
    HD_REQUIRE(n <= s->bytes, "upload of %zu bytes from a block of %zu", n, s->bytes);
    HD_CHECK_HIP(hipMemcpyAsync(s->dev, s->host, n, hipMemcpyHostToDevice, ctx->stream));
    if (!hd_capturing(ctx)) {
        HD_CHECK_HIP(hipEventRecord(s->uploaded, ctx->stream));
        s->valid = true;
    }
    return HIPDSP_OK;
}
