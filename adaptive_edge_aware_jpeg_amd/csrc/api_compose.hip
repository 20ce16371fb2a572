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

// the plan of a call, or the refusal of its first bad descriptor (fn NULL: quietly, for the size query)
static int compose_layout(aej_ctx *ctx, const char *fn, const aej_compose_desc *descs_host, int n, void *workspace, const uint8_t *src,
                          uint8_t *dst, CpPlan &plan)
{
    if (n < 1) return fn ? fail(ctx, AEJ_ERR_ARG, "%s: no images", fn) : AEJ_ERR_ARG;
    const char *why = nullptr;
    int bad = -1;
    const int code = compose_plan(descs_host, n, workspace, src, dst, plan, &bad, &why);
    if (!code || !fn) return code;
    return bad >= 0 ? fail(ctx, code, "%s: image %d: %s", fn, bad, why) : fail(ctx, code, "%s: %s", fn, why);
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
    for (const CpPlan::Read &r : plan.reads) {
        if ((uint64_t)r.offset + (uint64_t)r.bytes > src_bytes) return fail(ctx, AEJ_ERR_ARG, "%s: image %d: source outside the input", fn, r.element);
        const uintptr_t a = (uintptr_t)src + (uintptr_t)r.offset, d = (uintptr_t)dst;
        if (a < d + dst_bytes && d < a + (uintptr_t)r.bytes) return fail(ctx, AEJ_ERR_ARG, "%s: image %d: source inside the output", fn, r.element);
    }
    for (int i = 0; i < n; i++)
        if ((uint64_t)plan.dst_offset[i] + (uint64_t)plan.dst_bytes[i] > dst_bytes) return fail(ctx, AEJ_ERR_ARG, "%s: image %d: image outside the output", fn, i);
    AEJ_TRY(check_workspace(ctx, plan.bytes, workspace_bytes));
    AEJ_TRY(compose_layout(ctx, fn, descs_host, n, workspace, src, dst, plan));             // the same plan, with its pointers
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_compose(ctx->stream, plan));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps the plan's entries alive until their upload has run
    return 0;
}
