// api_convert.hip -- the Image.convert / hue / ImageOps.colorize entries of the C ABI (include/aej.h): aej_convert_* (convert.hip).
// Host code only.
#include "aej_ctx.h"

using namespace aej;

extern "C" int aej_convert_geometry_host(int32_t *out)
{
    if (!out) return AEJ_ERR_ARG;
    const int32_t g[3] = { kCvChunk, kCvThreads, kCvMaxGrid };
    memcpy(out, g, sizeof g);
    return 0;
}

extern "C" int aej_convert_plan_host(const aej_convert_desc *desc, aej_convert_plan *out)
{
    if (!desc || !out) return AEJ_ERR_ARG;
    const char *why = nullptr;
    return convert_resolve(*desc, -1, *out, &why);
}

static int convert_layout(aej_ctx *ctx, const char *fn, const aej_convert_desc *descs_host, int n, const uint8_t *tables_host, int n_tables,
                          void *workspace, const uint8_t *src, uint8_t *dst, CvPlan &plan)
{
    return plan_or_refuse(ctx, fn, n, [&](int *bad, const char **why) {
        return convert_plan(descs_host, n, tables_host, n_tables, workspace, src, dst, plan, bad, why);
    });
}

extern "C" uint64_t aej_convert_workspace_bytes(aej_ctx *ctx, const aej_convert_desc *descs_host, int n)
{
    CvPlan plan;
    if (!ctx || !descs_host || n < 1) return 0;
    if (convert_layout(ctx, nullptr, descs_host, n, nullptr, -1, nullptr, nullptr, nullptr, plan)) return 0;
    return plan.bytes;
}

extern "C" int aej_convert_batch(aej_ctx *ctx, const aej_convert_desc *descs_host, int n, const uint8_t *tables_host, int n_tables,
                                 const uint8_t *src, uint64_t src_bytes, uint8_t *dst, uint64_t dst_bytes, void *workspace,
                                 uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!descs_host || !src || !dst || !workspace || (n_tables > 0 && !tables_host)) return null_buffer(ctx, fn);
    if (n_tables < 0) return fail(ctx, AEJ_ERR_ARG, "%s: a negative number of tables", fn);
    CvPlan plan;
    AEJ_TRY(convert_layout(ctx, fn, descs_host, n, tables_host, n_tables, nullptr, nullptr, nullptr, plan));      // the checks and the size
    AEJ_TRY(check_spans(ctx, fn, plan.spans, src, src_bytes, dst, dst_bytes));
    AEJ_TRY(check_workspace(ctx, plan.bytes, workspace_bytes));
    AEJ_TRY(convert_layout(ctx, fn, descs_host, n, tables_host, n_tables, workspace, src, dst, plan));             // the same plan, with its pointers
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_convert(ctx->stream, plan));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps the plan's entries and tables alive until their uploads have run
    return 0;
}
