// api_window.hip -- the Kernel / rank / mode filter entries of the C ABI (include/aej.h): aej_window_* (window.hip).  Host code only.
#include "aej_ctx.h"

using namespace aej;

extern "C" int aej_window_geometry_host(int32_t *out)
{
    if (!out) return AEJ_ERR_ARG;
    const int32_t g[5] = { kWnTileW, kWnTileH, kWnKernelHalo, kWnRankHalo, kWnModeHalo };
    memcpy(out, g, sizeof g);
    return 0;
}

static int window_layout(aej_ctx *ctx, const char *fn, const aej_window_desc *descs_host, int n, WnPlan &plan)
{
    return plan_or_refuse(ctx, fn, n, [&](int *bad, const char **why) { return window_plan(descs_host, n, plan, bad, why); });
}

static unsigned long long window_carve(void *base, const WnPlan &plan, unsigned char *&blob)
{
    Carver c(base);
    blob = c.take<unsigned char>((long long)(plan.entries.size() * sizeof(WnEntry)));
    return c.bytes();
}

extern "C" uint64_t aej_window_workspace_bytes(aej_ctx *ctx, const aej_window_desc *descs_host, int n)
{
    WnPlan plan;
    if (!ctx || !descs_host || window_layout(ctx, nullptr, descs_host, n, plan)) return 0;
    unsigned char *blob;
    return window_carve(nullptr, plan, blob);
}

extern "C" int aej_window_batch(aej_ctx *ctx, const aej_window_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, uint8_t *dst,
                                uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!descs_host || !src || !dst || !workspace) return null_buffer(ctx, fn);
    WnPlan plan;
    AEJ_TRY(window_layout(ctx, fn, descs_host, n, plan));
    AEJ_TRY(check_spans(ctx, fn, plan.spans, src, src_bytes, dst, dst_bytes));
    unsigned char *blob_dev;
    AEJ_TRY(check_workspace(ctx, window_carve(workspace, plan, blob_dev), workspace_bytes));
    std::vector<WnEntry> blob;
    window_blob(plan, src, dst, blob);
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_window(ctx->stream, plan, blob_dev, blob.data()));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps `blob` alive until its upload has run
    return 0;
}
