// api_warp.hip -- the Image.transform / rotate / transpose entries of the C ABI (include/aej.h): aej_warp_* (warp.hip).  Host code only.
#include "aej_ctx.h"

using namespace aej;

extern "C" int aej_warp_geometry_host(int32_t *out)
{
    if (!out) return AEJ_ERR_ARG;
    const int32_t g[6] = { kWpTileW, kWpTileH, kWpFlipBytes, kWpFlipRows, kWpSwapTile, kWpSwapTile };
    memcpy(out, g, sizeof g);
    return 0;
}

extern "C" int aej_warp_plan_host(const aej_warp_desc *desc, aej_warp_plan *out, int32_t *tables, int64_t tables_len)
{
    if (!desc || !out) return AEJ_ERR_ARG;
    const char *why = nullptr;
    std::vector<int> tab;
    AEJ_TRY(warp_resolve(*desc, *out, &tab, &why));
    if (tab.empty()) return 0;
    if (!tables || tables_len < (int64_t)tab.size()) return AEJ_ERR_CAPACITY;
    memcpy(tables, tab.data(), tab.size() * sizeof(int));
    return 0;
}

static int warp_layout(aej_ctx *ctx, const char *fn, const aej_warp_desc *descs_host, int n, WpPlan &plan)
{
    return plan_or_refuse(ctx, fn, n, [&](int *bad, const char **why) { return warp_plan(descs_host, n, plan, bad, why); });
}

static unsigned long long warp_carve(void *base, const WpPlan &plan, unsigned char *&blob, int *&tables)
{
    Carver c(base);
    blob = c.take<unsigned char>((long long)(plan.entries.size() * sizeof(WpEntry)));
    tables = c.take<int>((long long)plan.tables.size());
    return c.bytes();
}

extern "C" uint64_t aej_warp_workspace_bytes(aej_ctx *ctx, const aej_warp_desc *descs_host, int n)
{
    WpPlan plan;
    if (!ctx || !descs_host || warp_layout(ctx, nullptr, descs_host, n, plan)) return 0;
    unsigned char *blob;
    int *tables;
    return warp_carve(nullptr, plan, blob, tables);
}

extern "C" int aej_warp_batch(aej_ctx *ctx, const aej_warp_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, uint8_t *dst,
                              uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!descs_host || !src || !dst || !workspace) return null_buffer(ctx, fn);
    WpPlan plan;
    AEJ_TRY(warp_layout(ctx, fn, descs_host, n, plan));
    AEJ_TRY(check_spans(ctx, fn, plan.spans, src, src_bytes, dst, dst_bytes));
    unsigned char *blob_dev;
    int *tables_dev;
    AEJ_TRY(check_workspace(ctx, warp_carve(workspace, plan, blob_dev, tables_dev), workspace_bytes));
    std::vector<WpEntry> blob;
    warp_blob(plan, src, dst, tables_dev, blob);
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_warp(ctx->stream, plan, blob_dev, blob.data(), tables_dev));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps `blob` and the plan's tables alive until their uploads have run
    return 0;
}
