// api_filter.hip -- the filter entries of the C ABI (include/aej.h): aej_filter_* (filter.hip).  Host code only.
#include "aej_ctx.h"

using namespace aej;

extern "C" int aej_filter_plan_host(int kind, float xradius, float yradius, aej_filter_plan *out)
{
    if (!out) return AEJ_ERR_ARG;
    return filter_weights(kind, xradius, yradius, *out);
}

extern "C" int aej_filter_geometry_host(int32_t *out)
{
    if (!out) return AEJ_ERR_ARG;
    const int32_t g[6] = { kFtTileW, kFtTileH, kFtHalo, kFtRowSpan, kFtColBand, kFtColBytes };
    memcpy(out, g, sizeof g);
    return 0;
}

static int filter_layout(aej_ctx *ctx, const char *fn, const aej_filter_desc *descs_host, int n, int path, FtPlan &plan)
{
    return plan_or_refuse(ctx, fn, n, [&](int *bad, const char **why) { return filter_plan(descs_host, n, path, plan, bad, why); });
}

extern "C" uint64_t aej_filter_workspace_bytes(aej_ctx *ctx, const aej_filter_desc *descs_host, int n, int path)
{
    FtPlan plan;
    if (!ctx || !descs_host || filter_layout(ctx, nullptr, descs_host, n, path, plan)) return 0;
    FtBufs w;
    return filter_carve(nullptr, plan, w);
}

extern "C" int aej_filter_batch(aej_ctx *ctx, const aej_filter_desc *descs_host, int n, int path, const uint8_t *src, uint64_t src_bytes,
                                uint8_t *dst, uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!descs_host || !src || !dst || !workspace) return null_buffer(ctx, fn);
    FtPlan plan;
    AEJ_TRY(filter_layout(ctx, fn, descs_host, n, path, plan));
    AEJ_TRY(check_spans(ctx, fn, plan.spans, src, src_bytes, dst, dst_bytes));
    FtBufs w;
    AEJ_TRY(check_workspace(ctx, filter_carve(workspace, plan, w), workspace_bytes));
    std::vector<FtEntry> blob;
    filter_blob(plan, w, src, dst, blob);
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_filter(ctx->stream, plan, w, blob.data()));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps `blob` alive until its upload has run
    return 0;
}
