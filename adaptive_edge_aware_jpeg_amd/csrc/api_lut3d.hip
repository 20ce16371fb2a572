// api_lut3d.hip -- the Color3DLUT entries of the C ABI (include/aej.h): aej_lut3d_* (lut3d.hip).  Host code only.
#include "aej_ctx.h"

using namespace aej;

extern "C" int aej_lut3d_prepare_host(const float *table, int64_t n, int16_t *out)
{
    if (!table || !out || n < 0) return AEJ_ERR_ARG;
    return lut3d_prepare(table, n, out);
}

extern "C" int aej_lut3d_geometry_host(int32_t *out)
{
    if (!out) return AEJ_ERR_ARG;
    const int32_t g[3] = { kLtThreads, kLtRun, kLtTile };
    memcpy(out, g, sizeof g);
    return 0;
}

static int lut3d_layout(aej_ctx *ctx, const char *fn, const aej_lut3d_desc *descs_host, int n, const int64_t *table_offsets, int n_tables,
                        LtPlan &plan)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "table_offsets are read as long long");
    return plan_or_refuse(ctx, fn, n, [&](int *bad, const char **why) {
        return lut3d_plan(descs_host, n, (const long long *)table_offsets, n_tables, plan, bad, why);
    });
}

struct LtBufs { unsigned char *blob; uint2 *tables; };

static unsigned long long lut3d_carve(void *base, const LtPlan &plan, LtBufs &w)
{
    Carver c(base);
    w.blob = c.take<unsigned char>((long long)(plan.entries.size() * sizeof(LtEntry)));
    w.tables = c.take<uint2>(plan.table_at.back());
    return c.bytes();
}

extern "C" uint64_t aej_lut3d_workspace_bytes(aej_ctx *ctx, const aej_lut3d_desc *descs_host, int n)
{
    LtPlan plan;
    if (!ctx || !descs_host || lut3d_layout(ctx, nullptr, descs_host, n, nullptr, 0, plan)) return 0;
    LtBufs w;
    return lut3d_carve(nullptr, plan, w);
}

extern "C" int aej_lut3d_batch(aej_ctx *ctx, const aej_lut3d_desc *descs_host, int n, const int16_t *tables_host,
                               const int64_t *table_offsets, int n_tables, const uint8_t *src, uint64_t src_bytes, uint8_t *dst,
                               uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!descs_host || !tables_host || !table_offsets || !src || !dst || !workspace) return null_buffer(ctx, fn);
    if (n_tables < 1) return fail(ctx, AEJ_ERR_ARG, "%s: no tables", fn);
    for (int t = 0; t < n_tables; t++)
        if (table_offsets[t] < 0 || table_offsets[t + 1] < table_offsets[t]) return fail(ctx, AEJ_ERR_ARG, "%s: table %d: offsets must not decrease", fn, t);
    LtPlan plan;
    AEJ_TRY(lut3d_layout(ctx, fn, descs_host, n, table_offsets, n_tables, plan));
    AEJ_TRY(check_spans(ctx, fn, plan.spans, src, src_bytes, dst, dst_bytes));
    LtBufs w;
    AEJ_TRY(check_workspace(ctx, lut3d_carve(workspace, plan, w), workspace_bytes));
    std::vector<LtEntry> blob;
    std::vector<short> padded;
    lut3d_blob(plan, descs_host, tables_host, (const long long *)table_offsets, src, dst, w.tables, blob, padded);
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_lut3d(ctx->stream, plan, w.blob, blob.data(), w.tables, padded.data()));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps `blob` and `padded` alive until their uploads have run
    return 0;
}
