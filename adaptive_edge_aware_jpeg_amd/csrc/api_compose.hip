// api_compose.hip -- the Image.paste / alpha_composite / blend / composite / ImageChops entries of the C ABI (include/aej.h):
// aej_compose_* (compose.hip).  Host code only.
#include "aej_ctx.h"

using namespace aej;

extern "C" int aej_compose_geometry_host(int32_t *out)
{
    if (!out) return AEJ_ERR_ARG;
    const int32_t g[3] = { kCpChunk, kCpThreads, kCpMaxGrid };
    memcpy(out, g, sizeof g);
    return 0;
}

extern "C" int aej_compose_plan_host(const aej_compose_desc *desc, aej_compose_plan *out)
{
    if (!desc || !out) return AEJ_ERR_ARG;
    const char *why = nullptr;
    return compose_resolve(*desc, *out, &why);
}

static int compose_layout(aej_ctx *ctx, const char *fn, const aej_compose_desc *descs_host, int n, void *workspace, const uint8_t *src,
                          uint8_t *dst, CpPlan &plan)
{
    return plan_or_refuse(ctx, fn, n, [&](int *bad, const char **why) { return compose_plan(descs_host, n, workspace, src, dst, plan, bad, why); });
}

extern "C" uint64_t aej_compose_workspace_bytes(aej_ctx *ctx, const aej_compose_desc *descs_host, int n)
{
    CpPlan plan;
    if (!ctx || !descs_host || n < 1) return 0;
    if (compose_layout(ctx, nullptr, descs_host, n, nullptr, nullptr, nullptr, plan)) return 0;
    return plan.bytes;
}

extern "C" int aej_compose_batch(aej_ctx *ctx, const aej_compose_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, uint8_t *dst,
                                 uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!descs_host || !src || !dst || !workspace) return null_buffer(ctx, fn);
    CpPlan plan;
    AEJ_TRY(compose_layout(ctx, fn, descs_host, n, nullptr, nullptr, nullptr, plan));      // the checks and the size
    AEJ_TRY(check_spans(ctx, fn, plan.spans, src, src_bytes, dst, dst_bytes));
    AEJ_TRY(check_workspace(ctx, plan.bytes, workspace_bytes));
    AEJ_TRY(compose_layout(ctx, fn, descs_host, n, workspace, src, dst, plan));             // the same plan, with its pointers
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_compose(ctx->stream, plan));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps the plan's entries alive until their upload has run
    return 0;
}
