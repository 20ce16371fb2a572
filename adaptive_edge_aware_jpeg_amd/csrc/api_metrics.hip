// api_metrics.hip -- the evaluation entries of the C ABI (include/aej.h): aej_metrics_* and aej_lpips_*.  Host code only.
#include "aej_ctx.h"

using namespace aej;

// ---- evaluation metrics (evaluation_metrics.py:50-89) ------------------------------------------------------------
struct MetricsWs {
    double *part;                // [B][parts.stride] partial sums (aej_launch.h)
    MetricParts parts;
    unsigned char *ga, *gb;
    float *xa, *xb;
    float *pyr[2][4];            // MS-SSIM scales 1..4 of both images, planar [B][3][h][w]
    int f, hp, wp;
    int lh[5], lw[5], lp[5];     // scale dimensions; lp[l] = padding applied when going from scale l-1 to l
    unsigned long long bytes;
};

static void carve_metrics(void *base, int B, int H, int W, MetricsWs &w)
{
    Carver c(base);
    w.ga = c.take<unsigned char>((long long)B * H * W);
    w.gb = c.take<unsigned char>((long long)B * H * W);
    // piq.ssim: f = max(1, round(min(H, W) / 256)) -- Python round(): ties to even
    w.f = (int)nearbyint((double)(H < W ? H : W) / 256.0);
    if (w.f < 1) w.f = 1;
    w.hp = H / w.f; w.wp = W / w.f;
    w.xa = c.take<float>((long long)B * w.hp * w.wp);
    w.xb = c.take<float>((long long)B * w.hp * w.wp);
    w.lh[0] = H; w.lw[0] = W; w.lp[0] = 0;
    for (int l = 1; l < 5; l++) {
        const int p = (w.lh[l - 1] % 2) > (w.lw[l - 1] % 2) ? (w.lh[l - 1] % 2) : (w.lw[l - 1] % 2);
        w.lp[l] = p;
        w.lh[l] = (w.lh[l - 1] + p) / 2;
        w.lw[l] = (w.lw[l - 1] + p) / 2;
        for (int i = 0; i < 2; i++) w.pyr[i][l - 1] = c.take<float>((long long)B * 3 * w.lh[l] * w.lw[l]);
    }
    MetricParts &P = w.parts;
    P.psnr_n = metric_prep_blocks((long long)H * W);
    P.grey_off = P.psnr_n;
    P.grey_n = ssim_partials(w.hp, w.wp);
    long long n = P.grey_off + P.grey_n;
    for (int l = 0; l < 5; l++) { P.lvl_off[l] = n; P.lvl_n[l] = ssim_partials(w.lh[l], w.lw[l]); n += 3 * P.lvl_n[l]; }
    P.stride = n;
    w.part = c.take<double>((long long)B * n);
    w.bytes = c.bytes();
}

extern "C" uint64_t aej_metrics_workspace_bytes(int batch, int H, int W)
{
    if (batch < 1 || H < 1 || W < 1) return 0;
    MetricsWs w;
    carve_metrics(nullptr, batch, H, W, w);
    return w.bytes;
}

extern "C" int aej_metrics_batch(aej_ctx *ctx, const float *img_a, const float *img_b, int batch, int H, int W, int which, double *out,
                                 void *workspace, uint64_t workspace_bytes)
{
    AEJ_TRY(enter(ctx, __func__));
    if (!img_a || !img_b || !out || !workspace) return null_buffer(ctx);
    if (batch < 1 || H < 1 || W < 1) return fail(ctx, AEJ_ERR_ARG, "bad shape %d x %d x %d", batch, H, W);
    if ((which & ~7) || !(which & 7)) return fail(ctx, AEJ_ERR_ARG, "which must be a combination of AEJ_METRIC_PSNR | AEJ_METRIC_SSIM | AEJ_METRIC_MS_SSIM");
    AEJ_TRY(bind_device(ctx));
    MetricsWs w;
    carve_metrics(workspace, batch, H, W, w);
    AEJ_TRY(check_workspace(ctx, w.bytes, workspace_bytes));
    const bool want_ssim = which & AEJ_METRIC_SSIM, want_ms = which & AEJ_METRIC_MS_SSIM;
    // piq/ssim.py _ssim_per_channel / piq/ms_ssim.py _multi_scale_ssim raise ValueError for these
    if (want_ssim && (w.hp < 11 || w.wp < 11)) return fail(ctx, AEJ_ERR_ARG, "Kernel size can't be greater than actual input size. Input size: %dx%d. Kernel size: 11x11", w.hp, w.wp);
    if (want_ms && (H < 161 || W < 161)) return fail(ctx, AEJ_ERR_ARG, "Invalid size of the input images, expected at least 161x161.");
    hipStream_t st = ctx->stream;
    float g11[11];
    {
        double e[11], sum = 0.0;
        for (int i = 0; i < 11; i++) { double c = (double)i - 5.0; e[i] = exp(-(c * c) / (2.0 * 1.5 * 1.5)); sum += e[i]; }
        for (int i = 0; i < 11; i++) g11[i] = (float)(e[i] / sum);
    }
    // every partial k_metric_final reads is written below (no accumulation, no clearing)
    launch_metric_prep(st, img_a, img_b, batch, (long long)H * W, w.part, w.parts.stride, want_ssim ? w.ga : nullptr, want_ssim ? w.gb : nullptr);
    long long n_ssim = 0, n_level[5] = { 0, 0, 0, 0, 0 };
    if (want_ssim) {
        launch_metric_pool_grey(st, w.ga, w.gb, batch, H, W, w.f, w.hp, w.wp, w.xa, w.xb);
        launch_ssim_level(st, false, w.xa, w.xb, batch, 1, w.hp, w.wp, g11, w.part, w.parts.stride, w.parts.grey_off, true);
        n_ssim = (long long)(w.hp - 10) * (w.wp - 10);
    }
    if (want_ms) {
        for (int l = 0; l < 5; l++) {
            const float *xa = l == 0 ? img_a : w.pyr[0][l - 1], *xb = l == 0 ? img_b : w.pyr[1][l - 1];
            if (l > 0) {
                const float *pa = l == 1 ? img_a : w.pyr[0][l - 2], *pb = l == 1 ? img_b : w.pyr[1][l - 2];
                if (l == 1) {
                    // even sizes: scale 0's SSIM kernel has written scale 1 on its way (no padding to replicate)
                    if (w.lp[1] != 0) launch_pool2_rgb(st, pa, pb, batch, w.lh[0], w.lw[0], w.lp[1], w.lh[1], w.lw[1], w.pyr[0][0], w.pyr[1][0]);
                } else {
                    launch_pool2(st, false, pa, batch, 3, w.lh[l - 1], w.lw[l - 1], w.lp[l], w.lh[l], w.lw[l], w.pyr[0][l - 1]);
                    launch_pool2(st, false, pb, batch, 3, w.lh[l - 1], w.lw[l - 1], w.lp[l], w.lh[l], w.lw[l], w.pyr[1][l - 1]);
                }
            }
            const bool fused_pool = l == 0 && w.lp[1] == 0;
            launch_ssim_level(st, l == 0, xa, xb, batch, 3, w.lh[l], w.lw[l], g11, w.part, w.parts.stride, w.parts.lvl_off[l], l == 4,
                              fused_pool ? w.pyr[0][0] : nullptr, fused_pool ? w.pyr[1][0] : nullptr);
            n_level[l] = (long long)(w.lh[l] - 10) * (w.lw[l] - 10);
        }
    }
    launch_metric_final(st, w.part, w.parts, batch, (long long)H * W, n_ssim, n_level, out);
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- LPIPS(net='alex') (lpips.hip) ---------------------------------------------------------------------------------------------
struct LpipsWs {
    float *x, *y, *feats;      // ping-pong activations, the normalised taps of img_a (aej_lpips_batch with img_a only)
    double *partial;
    unsigned long long bytes;
};

static void carve_lpips(void *base, int B, const LpipsGeom &g, LpipsWs &w)
{
    Carver c(base);
    w.x = c.take<float>((long long)B * g.x_elems);
    w.y = c.take<float>((long long)B * g.y_elems);
    w.partial = c.take<double>((long long)B * kLpipsTaps * g.max_blk);
    w.bytes = c.bytes();
    w.feats = c.take<float>((long long)B * g.feat_elems);      // beyond w.bytes: only aej_lpips_batch with img_a needs it
}

extern "C" uint64_t aej_lpips_weights_bytes(void)
{
    long long off[kLpipsTaps][3];
    return (uint64_t)lpips_packed_floats(off) * 4;
}

extern "C" int64_t aej_lpips_param_count(void) { return lpips_param_floats(); }

extern "C" int aej_lpips_pack_weights_host(const float *params, int64_t n_params, void *packed_host)
{
    if (!params || !packed_host) return AEJ_ERR_ARG;
    if (n_params != lpips_param_floats()) return AEJ_ERR_ARG;
    lpips_pack_host(params, (float *)packed_host);
    return 0;
}

extern "C" uint64_t aej_lpips_features_bytes(int batch, int H, int W)
{
    LpipsGeom g;
    if (batch < 1 || !lpips_geom(H, W, g)) return 0;
    return (uint64_t)batch * g.feat_elems * 4;
}

extern "C" uint64_t aej_lpips_workspace_bytes(int batch, int H, int W)
{
    LpipsGeom g;
    if (batch < 1 || !lpips_geom(H, W, g)) return 0;
    LpipsWs w;
    carve_lpips(nullptr, batch, g, w);
    return w.bytes;
}

static int lpips_args(aej_ctx *ctx, const char *fn, const void *weights, int batch, int H, int W, LpipsGeom &g)
{
    AEJ_TRY(enter(ctx, fn));
    if (!weights) return fail(ctx, AEJ_ERR_ARG, "%s: NULL weights", fn);
    if (batch < 1 || H < 1 || W < 1) return fail(ctx, AEJ_ERR_ARG, "%s: bad shape %d x %d x %d", fn, batch, H, W);
    if (!lpips_geom(H, W, g))
        return fail(ctx, AEJ_ERR_ARG, "%s: LPIPS needs images of at least 31x31 (got %dx%d): AlexNet's second maxpool would have no output", fn, H, W);
    return 0;
}

extern "C" int aej_lpips_features(aej_ctx *ctx, const void *weights, const float *img, int batch, int H, int W, float *feats, void *workspace,
                                  uint64_t workspace_bytes)
{
    LpipsGeom g;
    AEJ_TRY(lpips_args(ctx, __func__, weights, batch, H, W, g));
    if (!img || !feats || !workspace) return null_buffer(ctx);
    LpipsWs w;
    carve_lpips(workspace, batch, g, w);
    AEJ_TRY(check_workspace(ctx, w.bytes, workspace_bytes));
    AEJ_TRY(bind_device(ctx));
    launch_lpips(ctx->stream, (const float *)weights, img, batch, g, w.x, w.y, feats, nullptr, nullptr, nullptr);
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int aej_lpips_batch(aej_ctx *ctx, const void *weights, const float *img_a, const float *feats_a, const float *img_b, int batch, int H, int W,
                               double *out, void *workspace, uint64_t workspace_bytes)
{
    LpipsGeom g;
    AEJ_TRY(lpips_args(ctx, __func__, weights, batch, H, W, g));
    if (!img_a == !feats_a) return fail(ctx, AEJ_ERR_ARG, "exactly one of img_a and feats_a must be given");
    if (!img_b || !out || !workspace) return null_buffer(ctx);
    LpipsWs w;
    carve_lpips(workspace, batch, g, w);
    if (img_a) w.bytes += (unsigned long long)batch * g.feat_elems * 4;
    AEJ_TRY(check_workspace(ctx, w.bytes, workspace_bytes));
    AEJ_TRY(bind_device(ctx));
    const float *wpk = (const float *)weights;
    if (img_a) {      // the same two passes as aej_lpips_features + aej_lpips_batch(feats_a): bit-identical results
        launch_lpips(ctx->stream, wpk, img_a, batch, g, w.x, w.y, w.feats, nullptr, nullptr, nullptr);
        feats_a = w.feats;
    }
    launch_lpips(ctx->stream, wpk, img_b, batch, g, w.x, w.y, nullptr, feats_a, w.partial, out);
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}
