// api_resample.hip -- the resampling entries of the C ABI (include/aej.h): aej_resample_* (resample.hip).  Host code only.
#include "aej_ctx.h"

using namespace aej;

extern "C" int aej_resample_taps_host(int in_size, float in0, float in1, int out_size, int filter, int32_t *bounds_host, int32_t *taps_host,
                                      int64_t taps_capacity)
{
    if (rs_support(filter) == 0.0 || in_size < 1 || out_size < 1 || !(in1 - in0 > 0) || !(in0 >= 0) || !(in1 <= (float)in_size)) return AEJ_ERR_ARG;
    if ((!bounds_host) != (!taps_host)) return AEJ_ERR_ARG;
    const int ksize = rs_ksize(in0, in1, out_size, filter);
    if (!taps_host) return ksize;
    if (taps_capacity < (int64_t)out_size * ksize) return AEJ_ERR_CAPACITY;
    rs_taps(in_size, in0, in1, out_size, filter, ksize, bounds_host, taps_host);
    return ksize;
}

// the plan of a call, or the refusal of its first bad descriptor (fn NULL: quietly, for the size query)
static int resample_layout(aej_ctx *ctx, const char *fn, const aej_resample_desc *descs_host, int n, bool fill, RsPlan &plan, const int *channels_host,
                           const int32_t *windows_host = nullptr)
{
    AEJ_TRY(plan_or_refuse(ctx, fn, n, [&](int *bad, const char **why) {
        int code = AEJ_ERR_ARG;
        *bad = resample_plan(descs_host, n, fill, plan, why, &code, channels_host, windows_host);      // (the image at fault, or -1)
        return *bad >= 0 ? code : 0;
    }));
    for (int s = 0; s < 6; s++)
        if (plan.tiles[s / 3][s % 3] > 0x7fffffffLL) return fn ? fail(ctx, AEJ_ERR_UNSUPPORTED, "%s: more than 2^31 workgroups in one launch", fn) : AEJ_ERR_UNSUPPORTED;
    return 0;
}

static uint64_t resample_workspace(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const int *channels_host, const int32_t *windows_host = nullptr)
{
    RsPlan plan;
    if (!ctx || !descs_host || resample_layout(ctx, nullptr, descs_host, n, false, plan, channels_host, windows_host)) return 0;
    RsBufs w;
    return resample_carve(nullptr, plan, w);
}

extern "C" uint64_t aej_resample_workspace_bytes(aej_ctx *ctx, const aej_resample_desc *descs_host, int n)
{
    return resample_workspace(ctx, descs_host, n, nullptr);
}

extern "C" uint64_t aej_resample_workspace_bytes_ch(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const int *channels_host)
{
    return resample_workspace(ctx, descs_host, n, channels_host);
}

extern "C" uint64_t aej_resample_workspace_bytes_win(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const int *channels_host,
                                                     const int32_t *windows_host)
{
    return resample_workspace(ctx, descs_host, n, channels_host, windows_host);
}

// aej_resample_batch (channels_host NULL: every image three channels), aej_resample_batch_ch and aej_resample_batch_win (windows_host)
static int resample_batch(aej_ctx *ctx, const char *fn, const aej_resample_desc *descs_host, int n, const int *channels_host, const uint8_t *src,
                          uint64_t src_bytes, uint8_t *dst, uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes,
                          const int32_t *windows_host = nullptr)
{
    AEJ_TRY(enter(ctx, fn));
    if (!descs_host || !src || !dst || !workspace) return null_buffer(ctx, fn);
    RsPlan plan;
    AEJ_TRY(resample_layout(ctx, fn, descs_host, n, true, plan, channels_host, windows_host));
    AEJ_TRY(check_spans(ctx, fn, plan.spans, src, src_bytes, dst, dst_bytes));
    RsBufs w;
    AEJ_TRY(check_workspace(ctx, resample_carve(workspace, plan, w), workspace_bytes));
    std::vector<unsigned char> blob;
    resample_blob(plan, w, src, dst, blob);
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_resample(ctx->stream, plan, w, blob.data(), blob.size()));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps `blob` alive until its upload has run
    return 0;
}

extern "C" int aej_resample_batch(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, uint8_t *dst,
                                  uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes)
{
    return resample_batch(ctx, __func__, descs_host, n, nullptr, src, src_bytes, dst, dst_bytes, workspace, workspace_bytes);
}

extern "C" int aej_resample_batch_ch(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const int *channels_host, const uint8_t *src,
                                     uint64_t src_bytes, uint8_t *dst, uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes)
{
    return resample_batch(ctx, __func__, descs_host, n, channels_host, src, src_bytes, dst, dst_bytes, workspace, workspace_bytes);
}

extern "C" int aej_resample_batch_win(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const int *channels_host, const int32_t *windows_host,
                                      const uint8_t *src, uint64_t src_bytes, uint8_t *dst, uint64_t dst_bytes, void *workspace,
                                      uint64_t workspace_bytes)
{
    return resample_batch(ctx, __func__, descs_host, n, channels_host, src, src_bytes, dst, dst_bytes, workspace, workspace_bytes, windows_host);
}
