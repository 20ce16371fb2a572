// api_adjust.hip -- the ImageEnhance / ImageOps / Image.histogram entries of the C ABI (include/aej.h): aej_adjust_*, aej_histogram_batch
// (adjust.hip).  Host code only.
#include "aej_ctx.h"

using namespace aej;

extern "C" int aej_adjust_geometry_host(int32_t *out)
{
    if (!out) return AEJ_ERR_ARG;
    const int32_t g[4] = { kAdChunk, kAdThreads, kAdMaxGrid, AEJ_ADJUST_TABLE_BYTES };
    memcpy(out, g, sizeof g);
    return 0;
}

extern "C" int aej_adjust_plan_host(const aej_adjust_desc *desc, aej_adjust_plan *out)
{
    if (!desc || !out) return AEJ_ERR_ARG;
    const char *why = nullptr;
    return adjust_resolve(*desc, -1, *out, &why);
}

static int adjust_layout(aej_ctx *ctx, const char *fn, const aej_adjust_desc *descs_host, int n, const uint8_t *tables_host, int n_tables,
                         bool histogram, void *workspace, const uint8_t *src, uint8_t *dst, AdPlan &plan)
{
    return plan_or_refuse(ctx, fn, n, [&](int *bad, const char **why) {
        return adjust_plan(descs_host, n, tables_host, n_tables, histogram, workspace, src, dst, plan, bad, why);
    });
}

extern "C" uint64_t aej_adjust_workspace_bytes(aej_ctx *ctx, const aej_adjust_desc *descs_host, int n)
{
    AdPlan plan;
    if (!ctx || !descs_host || n < 1) return 0;
    const bool histogram = descs_host[0].n_ops == 0;          // (a call is all of one kind: the other kind's descriptors are refused)
    if (adjust_layout(ctx, nullptr, descs_host, n, nullptr, -1, histogram, nullptr, nullptr, nullptr, plan)) return 0;
    return plan.bytes;
}

// what both entries do once their arguments are known to be there
static int adjust_run(aej_ctx *ctx, const char *fn, const aej_adjust_desc *descs_host, int n, const uint8_t *tables_host, int n_tables,
                      bool histogram, const uint8_t *src, uint64_t src_bytes, uint8_t *dst, uint64_t dst_elements, void *workspace,
                      uint64_t workspace_bytes)
{
    AdPlan plan;
    AEJ_TRY(adjust_layout(ctx, fn, descs_host, n, tables_host, n_tables, histogram, nullptr, nullptr, nullptr, plan));      // the checks and the size
    AEJ_TRY(check_spans(ctx, fn, plan.spans, src, src_bytes, dst, dst_elements, histogram ? sizeof(int64_t) : 1));
    AEJ_TRY(check_workspace(ctx, plan.bytes, workspace_bytes));
    AEJ_TRY(adjust_layout(ctx, fn, descs_host, n, tables_host, n_tables, histogram, workspace, src, dst, plan));             // the same plan, with its pointers
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_adjust(ctx->stream, plan));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps the plan's entries, tables and SMOOTH entries alive until their uploads have run
    return 0;
}

extern "C" int aej_adjust_batch(aej_ctx *ctx, const aej_adjust_desc *descs_host, int n, const uint8_t *tables_host, int n_tables,
                                const uint8_t *src, uint64_t src_bytes, uint8_t *dst, uint64_t dst_bytes, void *workspace,
                                uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!descs_host || !src || !dst || !workspace || (n_tables > 0 && !tables_host)) return null_buffer(ctx, fn);
    if (n_tables < 0) return fail(ctx, AEJ_ERR_ARG, "%s: a negative number of tables", fn);
    return adjust_run(ctx, fn, descs_host, n, tables_host, n_tables, false, src, src_bytes, dst, dst_bytes, workspace, workspace_bytes);
}

extern "C" int aej_histogram_batch(aej_ctx *ctx, const aej_adjust_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes,
                                   int64_t *hist, uint64_t hist_elements, void *workspace, uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!descs_host || !src || !hist || !workspace) return null_buffer(ctx, fn);
    return adjust_run(ctx, fn, descs_host, n, nullptr, 0, true, src, src_bytes, (uint8_t *)hist, hist_elements, workspace, workspace_bytes);
}
