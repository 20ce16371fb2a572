// api.hip -- the core of the C ABI of libaejpeg_hip.so (include/aej.h): context lifetime, settings and their tables, options, stream,
// profiling and diagnostics, the constant tables and the geometry builders.  Its siblings hold the entry points of one subsystem each:
// api_encode.hip, api_decode.hip, api_metrics.hip, api_jpeg.hip.  Host code only; gfx950 kernels live in the other .hip files.
#include "aej_ctx.h"

using namespace aej;

int aej::hip_fail(aej_ctx *ctx, hipError_t e, const char *expr, const char *file, int line)
{
    return fail(ctx, AEJ_ERR_HIP, "%s failed: %s (%s:%d)", expr, hipGetErrorString(e), file, line);
}

// ---- constant tables ---------------------------------------------------------------------------------
// down-sampling ratios (rh, rw) per layer: JpegCompressionSettings.COLOR_SPACE_SETTINGS, jpeg.py:62-147
static const int kRatios[7][3][2] = {
    { { 1, 1 }, { 2, 2 }, { 2, 2 } },  // YCbCr
    { { 1, 1 }, { 2, 2 }, { 2, 2 } },  // YCoCg
    { { 1, 1 }, { 2, 2 }, { 2, 2 } },  // YCoCg-R
    { { 1, 1 }, { 2, 2 }, { 2, 2 } },  // OKLAB
    { { 1, 1 }, { 1, 4 }, { 1, 4 } },  // ICtCp
    { { 1, 1 }, { 1, 4 }, { 1, 4 } },  // ICaCb
    { { 1, 1 }, { 2, 2 }, { 2, 2 } },  // JzAzBz
};
// MIDPOINTS / SCALE_FACTORS: float32 of the Python literals (ycbcr.py:41-42, ycocg.py:41-42,62-63, oklab.py:51-52,
// ictcp.py:162-163, icacb.py:162-163, jzazbz.py:211-212)
const double kMid[7][3] = {
    { 0.5000000037252903, 7.450580596923828e-09, 0.0 }, { 0.5, 0.0, 0.0 }, { 0.5, 0.0, 0.0 },
    { 0.4999999, 0.021152213, -0.056563325 }, { 0.07497266, -0.0008235276, 0.023989676 },
    { 0.07498085, 0.02180194, -0.018250957 }, { 0.0087900255, 0.00048353244, -0.0020741792 },
};
const double kScale[7][3] = {
    { 253.99999810755253, 254.000003784895, 254.0 }, { 254.0, 254.0, 254.0 }, { 254.0, 127.0, 127.0 },
    { 254.00005, 497.9055, 497.94604 }, { 1693.9674, 1133.9044, 1694.004 },
    { 1693.7823, 1838.5665, 1330.3855 }, { 14448.194, 7590.505, 5552.201 },
};


// quadtree.py:89-90 + utils.py:36-41: largest_power_of_2(max(H, W)) * 2
static int root_size_of(int h, int w)
{
    int n = h > w ? h : w;
    int lp;
    if (n <= 2) lp = n;
    else { lp = 1; while (lp * 2 < n) lp *= 2; }
    return lp * 2;
}

static void fill_clahe_geom(Geom &g)
{
    long long bp = 0;
    for (int l = 0; l < g.nl; l++) {
        g.wpr[l] = (g.w[l] + 63) / 64;
        g.bpoff[l] = bp;
        bp += bp_words(g.h[l], g.wpr[l]);
    }
    g.bpstride = bp;
    for (int l = 0; l < g.nl; l++) {
        int w = g.w[l], h = g.h[l];
        int wp = w, hp = h;
        if ((w % 4) != 0 || (h % 4) != 0) { wp = w + (4 - w % 4); hp = h + (4 - h % 4); }   // clahe.cpp copyMakeBorder
        g.ctw[l] = wp / 4;
        g.cth[l] = hp / 4;
    }
}

int check_image_size(aej_ctx *ctx, const char *what, int H, int W)
{
    if (H > 65535 || W > 65535) return fail(ctx, AEJ_ERR_UNSUPPORTED, "%s %dx%d: sides above 65535 pixels are not built (leaf origins travel as 16-bit pairs, LeafWork)", what, H, W);
    if ((long long)H * W > kMaxImagePixels)
        return fail(ctx, AEJ_ERR_UNSUPPORTED, "%s %dx%d: more than 2^29 = %lld pixels in one image are not built (element indices and plane byte offsets are 32-bit)",
                    what, H, W, kMaxImagePixels);
    return 0;
}

int make_geom(aej_ctx *ctx, int space, int B, int H, int W, Geom &g)
{
    memset(&g, 0, sizeof g);
    AEJ_TRY(check_image_size(ctx, "image", H, W));
    g.B = B; g.nl = 3; g.H = H; g.W = W;
    long long off = 0;
    for (int l = 0; l < 3; l++) {
        g.rh[l] = kRatios[space][l][0];
        g.rw[l] = kRatios[space][l][1];
        g.h[l] = H / g.rh[l];
        g.w[l] = W / g.rw[l];
        if (g.h[l] < 1 || g.w[l] < 1) return fail(ctx, AEJ_ERR_ARG, "image %dx%d too small for the down-sampling ratios", H, W);
        g.poff[l] = off;
        off += align_up((long long)g.h[l] * g.w[l], 64);
    }
    g.pstride = off;
    fill_clahe_geom(g);
    return 0;
}

void make_plane_geom(int H, int W, Geom &g)   // one stand-alone plane as "layer 0"
{
    memset(&g, 0, sizeof g);
    g.B = 1; g.nl = 1; g.H = H; g.W = W;
    g.h[0] = H; g.w[0] = W; g.rh[0] = g.rw[0] = 1;
    g.poff[0] = 0;
    g.pstride = align_up((long long)H * W, 64);
    fill_clahe_geom(g);
}

int make_qtgeom(aej_ctx *ctx, const Geom &g, int bmin, int bmax, QtGeom &q, bool allow_small_root)
{
    memset(&q, 0, sizeof q);
    if (!is_pow2(bmin) || !is_pow2(bmax) || bmin > bmax || bmin < 1)
        return fail(ctx, AEJ_ERR_ARG, "block sizes must be powers of two with min <= max (got %d, %d)", bmin, bmax);
    q.bmin = bmin; q.bmax = bmax; q.cell = bmin;
    long long pyr = 0, chunks = 0, co = 0, lo = 0, so = 0;
    for (int l = 0; l < g.nl; l++) {
        int root = root_size_of(g.h[l], g.w[l]);
        if (root < bmin) {
            // the whole layer is one leaf of size `root` (quadtree.py:116-118); the codec has no tables for that size
            if (!allow_small_root || g.nl != 1) return fail(ctx, AEJ_ERR_UNSUPPORTED, "layer %d (%dx%d): root %d smaller than min block %d", l, g.h[l], g.w[l], root, bmin);
            q.cell = root;
        }
        q.root[l] = root;
        q.ncell[l] = root / q.cell;
        q.ltot[l] = ilog2(q.ncell[l]);
        if (q.ltot[l] > 14) return fail(ctx, AEJ_ERR_UNSUPPORTED, "quadtree deeper than 14 levels");
        q.pyr_off[l] = pyr;
        long long states = 0;
        for (int j = 0; j <= q.ltot[l]; j++) { long long s = q.ncell[l] >> j; states += s * s; }
        pyr += align_up(states, 256);
        long long nc2 = (long long)q.ncell[l] * q.ncell[l];
        q.nchunk[l] = (int)(nc2 / 256 > 0 ? nc2 / 256 : 1);
        q.chunk_off[l] = chunks;
        chunks += q.nchunk[l];
        int top = bmax < root ? bmax : root;
        long long wc = align_up(g.w[l], top), hc = align_up(g.h[l], top);
        if (wc > root) wc = root;
        if (hc > root) hc = root;
        q.coeff_cap[l] = wc * hc;
        q.leaf_cap[l] = (wc / q.cell) * (hc / q.cell);
        q.state_cap[l] = states;
        q.coeff_off[l] = co; co += align_up(q.coeff_cap[l], 64);
        q.leaf_off[l] = lo;  lo += align_up(q.leaf_cap[l], 16);
        q.state_off[l] = so; so += align_up(q.state_cap[l], 64);
    }
    q.pyr_stride = pyr; q.chunk_stride = chunks;
    q.coeff_stride = co; q.leaf_stride = lo; q.state_stride = so;
    // per-size work lists: worst-case leaves of size s per layer
    int k = 0;
    for (int s = bmin; s <= bmax && k < kMaxSizes; s *= 2, k++) {
        long long off = 0;
        for (int l = 0; l < g.nl; l++) {
            q.work_off[l][k] = off;
            if (s > q.root[l]) continue;
            int top = bmax < q.root[l] ? bmax : q.root[l];
            long long wc = align_up(g.w[l], top), hc = align_up(g.h[l], top);
            if (wc > q.root[l]) wc = q.root[l];
            if (hc > q.root[l]) hc = q.root[l];
            off += ((wc + s - 1) / s) * ((hc + s - 1) / s);
        }
        q.work_stride[k] = off;
    }
    q.nsizes = k;
    return 0;
}

long long big_scratch_floats(int bmax)      // the launches of different sizes run one after the other: one scratch, sized for the largest
{
    long long m = 0;
    for (int s = 256; s <= bmax; s *= 2) m = std::max(m, big_scratch_floats_for(s));
    return m;
}

int check_encode_args(aej_ctx *ctx, int batch, int H, int W)
{
    if (!ctx) return AEJ_ERR_ARG;
    if (!ctx->has_settings) return fail(ctx, AEJ_ERR_STATE, "aej_set_settings has not been called");
    if (batch < 1 || H < 1 || W < 1) return fail(ctx, AEJ_ERR_ARG, "batch, H, W must be positive");
    if (batch * 3 > kMaxPlanes) return fail(ctx, AEJ_ERR_UNSUPPORTED, "batch %d too large for one call (max %d images)", batch, kMaxPlanes / 3);
    return 0;
}

int make_geoms(aej_ctx *ctx, int batch, int H, int W, Geom &g, QtGeom &q)
{
    AEJ_TRY(make_geom(ctx, ctx->space, batch, H, W, g));
    return make_qtgeom(ctx, g, ctx->bmin, ctx->bmax, q);
}

// ---- lifetime ---------------------------------------------------------------------------------------------
extern "C" int aej_abi_version(void) { return AEJ_ABI_VERSION; }

extern "C" aej_ctx *aej_create(int device, void *hip_stream)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n || device >= kMaxDevices) return nullptr;      // (the per-device chain state is indexed by it)
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    aej_ctx *ctx = new aej_ctx();
    ctx->device = device;
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    if (hipHostMalloc(reinterpret_cast<void **>(&ctx->h_flag), kFlagWords * sizeof(int), hipHostMallocDefault) != hipSuccess) { delete ctx; return nullptr; }
    return ctx;
}

extern "C" void aej_destroy(aej_ctx *ctx)
{
    if (!ctx) return;
    (void)bind_device(ctx);
    release_encode_state(ctx);
    if (ctx->gstream) (void)hipStreamDestroy(ctx->gstream);
    if (ctx->gevent) (void)hipEventDestroy(ctx->gevent);
    if (ctx->tables) (void)hipFree(ctx->tables);
    if (ctx->d_bilateral) (void)hipFree(ctx->d_bilateral);
    for (int i = 0; i < aej_ctx::kMaxSub; i++) {
        if (ctx->sub_stream[i]) (void)hipStreamDestroy(ctx->sub_stream[i]);
        if (ctx->sub_color_done[i]) (void)hipEventDestroy(ctx->sub_color_done[i]);
        if (ctx->sub_flag[i]) (void)hipHostFree(ctx->sub_flag[i]);
    }
    if (ctx->sub_in) (void)hipEventDestroy(ctx->sub_in);
    if (ctx->h_flag) (void)hipHostFree(ctx->h_flag);
    for (int i = 0; i < 24; i++) if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    delete ctx;
}

extern "C" const char *aej_last_error(aej_ctx *ctx)
{
    if (!ctx) return "aej: no context (aej_create failed: no such HIP device?)";
    return ctx->err.c_str();
}

extern "C" int aej_synchronize(aej_ctx *ctx)
{
    AEJ_TRY(enter(ctx, __func__));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- settings ---------------------------------------------------------------------------------------------
// Jpeg._zigzag_ordering (jpeg.py:726-766) as an anti-diagonal walk: even diagonals run bottom-left -> top-right
static void zigzag_order(int s, std::vector<int> &zz)
{
    zz.resize((size_t)s * s);
    int i = 0;
    for (int d = 0; d < 2 * s - 1; d++) {
        int lo = d - s + 1 > 0 ? d - s + 1 : 0, hi = d < s - 1 ? d : s - 1;
        if (d % 2) for (int r = lo; r <= hi; r++) zz[i++] = r * s + (d - r);
        else for (int r = hi; r >= lo; r--) zz[i++] = r * s + (d - r);
    }
}

extern "C" int aej_set_settings(aej_ctx *ctx, int space, int bmin, int bmax, const int32_t *qmats_host)
{
    AEJ_TRY(enter(ctx, __func__));
    if (space < 0 || space > 6) return fail(ctx, AEJ_ERR_ARG, "Unsupported color space id: %d", space);
    if (!is_pow2(bmin) || !is_pow2(bmax) || bmin > bmax || bmin < 2)
        return fail(ctx, AEJ_ERR_ARG, "block size range (%d, %d): powers of two with 2 <= min <= max required", bmin, bmax);
    if (bmax > kMaxBlock)
        return fail(ctx, AEJ_ERR_UNSUPPORTED, "block size range (%d, %d): no kernel for blocks above %d", bmin, bmax, kMaxBlock);
    if (ilog2(bmax) - ilog2(bmin) + 1 > kMaxSizes)
        return fail(ctx, AEJ_ERR_UNSUPPORTED, "block size range (%d, %d) spans more than %d sizes", bmin, bmax, kMaxSizes);
    if (!qmats_host) return fail(ctx, AEJ_ERR_ARG, "qmats_host is NULL");
    AEJ_TRY(bind_device(ctx));
    int nsizes = 0;
    for (int s = bmin; s <= bmax; s *= 2) nsizes++;
    // host image of all tables
    std::vector<char> blob;
    auto put = [&](const void *p, size_t bytes) {
        size_t o = (blob.size() + 255) & ~(size_t)255;
        blob.resize(o + bytes);
        memcpy(blob.data() + o, p, bytes);
        return o;
    };
    size_t oD[kMaxSizes], oZ[kMaxSizes], oZf[kMaxSizes], oQ[3][kMaxSizes];
    int k = 0;
    size_t qpos = 0;
    std::vector<size_t> qoff_layer_size;
    for (int s = bmin; s <= bmax; s *= 2, k++) {
        std::vector<float> D((size_t)s * s);
        for (int u = 0; u < s; u++) {
            double alpha = u == 0 ? sqrt(1.0 / (double)s) : sqrt(2.0 / (double)s);
            for (int n = 0; n < s; n++) D[(size_t)u * s + n] = (float)(alpha * cos(3.14159265358979323846 * (double)(2 * n + 1) * (double)u / (2.0 * (double)s)));
        }
        oD[k] = put(D.data(), D.size() * 4);
        std::vector<int> zz, inv((size_t)s * s);
        zigzag_order(s, zz);
        for (int i = 0; i < s * s; i++) inv[zz[i]] = i;
        oZ[k] = put(inv.data(), inv.size() * 4);
        oZf[k] = put(zz.data(), zz.size() * 4);
    }
    for (int l = 0; l < 3; l++) {
        k = 0;
        for (int s = bmin; s <= bmax; s *= 2, k++) {
            for (int i = 0; i < s * s; i++)
                if (qmats_host[qpos + i] < 1) return fail(ctx, AEJ_ERR_ARG, "quantisation matrix entries must be >= 1");
            oQ[l][k] = put(qmats_host + qpos, (size_t)s * s * 4);
            qpos += (size_t)s * s;
        }
    }
    const int zero_words[64] = {};
    const size_t oCheck = put(zero_words, sizeof zero_words);
    drop_graphs(ctx);                  // captured kernel arguments point into the old tables
    if (ctx->tables) { AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream)); AEJ_HIP_CHECK(hipFree(ctx->tables)); ctx->tables = nullptr; }
    AEJ_HIP_CHECK(hipMalloc(&ctx->tables, blob.size()));
    AEJ_HIP_CHECK(hipMemcpy(ctx->tables, blob.data(), blob.size(), hipMemcpyHostToDevice));
    char *base = static_cast<char *>(ctx->tables);
    for (int i = 0; i < kMaxSizes; i++) {
        ctx->d_D[i] = nullptr; ctx->d_zzinv[i] = nullptr; ctx->d_zz[i] = nullptr;
        for (int l = 0; l < 3; l++) ctx->d_qm[l][i] = nullptr;
    }
    for (int i = 0; i < nsizes; i++) {
        ctx->d_D[i] = reinterpret_cast<const float *>(base + oD[i]);
        ctx->d_zzinv[i] = reinterpret_cast<const int *>(base + oZ[i]);
        ctx->d_zz[i] = reinterpret_cast<const int *>(base + oZf[i]);
        for (int l = 0; l < 3; l++) ctx->d_qm[l][i] = reinterpret_cast<const int *>(base + oQ[l][i]);
    }
    ctx->d_check = reinterpret_cast<int *>(base + oCheck);
    ctx->space = space; ctx->bmin = bmin; ctx->bmax = bmax; ctx->nsizes = nsizes;
    ctx->has_settings = true;
    return 0;
}

extern "C" int aej_set_canny_params(aej_ctx *ctx, const aej_canny_params *p)
{
    AEJ_TRY(enter(ctx, __func__));
    const aej_canny_params def = { 0.10, 0.30, 0.75, 75.0, 75.0, 1 };
    const aej_canny_params v = p ? *p : def;
    if (!(v.canny_low_ratio >= 0.0 && v.canny_low_ratio <= 1.0 && v.canny_high_ratio >= 0.0 && v.canny_high_ratio <= 1.0))
        return fail(ctx, AEJ_ERR_ARG, "Canny threshold ratios must lie in [0, 1] (np.percentile takes 0..100)");
    if (!(v.clahe_clip_limit == v.clahe_clip_limit) || !(v.bilateral_sigma_color == v.bilateral_sigma_color) || !(v.bilateral_sigma_space == v.bilateral_sigma_space))
        return fail(ctx, AEJ_ERR_ARG, "NaN Canny hyper-parameter");
    const bool tables_change = v.bilateral_sigma_color != ctx->canny.bilateral_sigma_color || v.bilateral_sigma_space != ctx->canny.bilateral_sigma_space;
    ctx->canny = v;
    drop_graphs(ctx);                      // captured kernel arguments carry the old values
    if (tables_change) { ctx->d_color_w = nullptr; ctx->d_space_w = nullptr; }
    return 0;
}

extern "C" int aej_get_hysteresis_stats(aej_ctx *ctx, int64_t *out_host)
{
    if (!ctx || !out_host) return AEJ_ERR_ARG;
    out_host[0] = ctx->n_encode_calls;
    out_host[1] = ctx->last_hyst_queued;
    return 0;
}

extern "C" int aej_set_graph_mode(aej_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return AEJ_ERR_ARG;
    AEJ_TRY(refuse_in_flight(ctx, __func__));
    ctx->graph_mode = mode;
    if (mode == 0) drop_graphs(ctx);
    return 0;
}

extern "C" int aej_set_sub_batches(aej_ctx *ctx, int n)
{
    if (!ctx || n < 0 || n > aej_ctx::kMaxSub) return AEJ_ERR_ARG;
    ctx->sub_mode = n;
    return 0;
}

extern "C" int64_t aej_get_split_calls(aej_ctx *ctx) { return ctx ? (int64_t)ctx->n_split_calls : -1; }

extern "C" int aej_set_hw_queues(aej_ctx *ctx, int n)
{
    if (!ctx || n < 1) return AEJ_ERR_ARG;
    if (aej::priorities_refused(ctx->stream_priorities, ctx->stream_priority_pattern, n))
        return fail(ctx, AEJ_ERR_ARG, "aej_set_hw_queues: %d queues on each of %d priority levels (stream_priorities = 2) are more than the %d a process may hold",
                    n, aej::priority_levels(ctx->stream_priority_pattern), aej::kMaxProcessQueues);
    ctx->hw_queues = n;
    return 0;
}

// ---- options: every tuning / A-B choice of the library is a per-context value set through this entry (include/aej.h has the table) ----
namespace {
struct OptionDef { const char *name; int aej::Tuning::*field; int aej_ctx::*ctx_field; long long lo, hi; bool drops_graphs; };
const OptionDef kOptions[] = {
    { "color_strip", &aej::Tuning::color_strip, nullptr, 0, 1, true },
    { "color_strip_rows", &aej::Tuning::color_strip_rows, nullptr, 0, 64, true },
    { "color_workgroups", &aej::Tuning::color_workgroups, nullptr, 0, 1 << 16, true },
    { "planes_row_major", &aej::Tuning::planes_row_major, nullptr, 0, 1, true },
    { "dct64_kernel", &aej::Tuning::dct64_kernel, nullptr, 0, 4, true },
    { "dct_small_workgroups", &aej::Tuning::dct_small_workgroups, nullptr, 0, 1 << 16, true },
    { "sobel_lds", &aej::Tuning::sobel_lds, nullptr, 0, 1, true },
    { "sobel_xcd", &aej::Tuning::sobel_xcd, nullptr, 0, 1, true },
    { "dct_multi", &aej::Tuning::dct_multi, nullptr, 0, 1, true },
    { "qt_chunks", &aej::Tuning::qt_chunks, nullptr, 0, 1, true },
    { "qt_chunk_run", &aej::Tuning::qt_chunk_run, nullptr, 0, 16, true },
    { "qt_chunk_launches", nullptr, &aej_ctx::qt_chunk_launches, 0, 0x7fffffff, false },
    { "sub_chain", nullptr, &aej_ctx::sub_chain, -1, 3, false },
    { "stream_priorities", nullptr, &aej_ctx::stream_priorities, 0, 2, false },
    { "stream_priority_pattern", nullptr, &aej_ctx::stream_priority_pattern, 0, aej::kPriorityPatterns - 1, false },
    { "priority_streams", nullptr, &aej_ctx::n_priority_streams, 0, 0, false },
    { "jpegdec_subseq_bits", nullptr, &aej_ctx::jd_subseq_bits, 32, 1 << 20, false },
};
const OptionDef *find_option(const char *name)
{
    if (!name) return nullptr;
    for (const OptionDef &o : kOptions) if (!strcmp(o.name, name)) return &o;
    return nullptr;
}
}  // namespace

extern "C" int aej_set_option(aej_ctx *ctx, const char *name, int64_t value)
{
    AEJ_TRY(enter(ctx, __func__));
    const OptionDef *o = find_option(name);
    if (!o) return fail(ctx, AEJ_ERR_ARG, "aej_set_option: unknown option '%s'", name ? name : "(null)");
    if (value < o->lo || value > o->hi || (o->field == &aej::Tuning::dct64_kernel && value != 0 && value != 1 && value != 4))
        return fail(ctx, AEJ_ERR_ARG, "aej_set_option: %s = %lld outside its range [%lld, %lld]", name, (long long)value, o->lo, o->hi);
    if (o->ctx_field == &aej_ctx::n_priority_streams) return fail(ctx, AEJ_ERR_ARG, "aej_set_option: %s is read-only", name);
    if (o->ctx_field == &aej_ctx::stream_priorities || o->ctx_field == &aej_ctx::stream_priority_pattern) {
        // "always" is refused where it would take the process past the queues it may hold (aej_sched.h)
        const int mode = o->ctx_field == &aej_ctx::stream_priorities ? (int)value : ctx->stream_priorities;
        const int pattern = o->ctx_field == &aej_ctx::stream_priority_pattern ? (int)value : ctx->stream_priority_pattern;
        if (aej::priorities_refused(mode, pattern, ctx->hw_queues))
            return fail(ctx, AEJ_ERR_ARG, "aej_set_option: %s = %lld: %d queues on each of %d priority levels are more than the %d a process may hold", name,
                        (long long)value, ctx->hw_queues, aej::priority_levels(pattern), aej::kMaxProcessQueues);
    }
    if (o->field) ctx->tune.*(o->field) = (int)value;
    else ctx->*(o->ctx_field) = (int)value;
    if (o->drops_graphs) drop_graphs(ctx);      // a captured graph holds the launches the old value chose
    return 0;
}

extern "C" int aej_get_option(aej_ctx *ctx, const char *name, int64_t *value_host)
{
    if (!ctx || !value_host) return AEJ_ERR_ARG;
    const OptionDef *o = find_option(name);
    if (!o) return fail(ctx, AEJ_ERR_ARG, "aej_get_option: unknown option '%s'", name ? name : "(null)");
    *value_host = o->field ? ctx->tune.*(o->field) : ctx->*(o->ctx_field);
    return 0;
}

extern "C" int aej_test_fail_after_stage(aej_ctx *ctx, int stage)
{
    if (!ctx || stage < -1 || stage >= AEJ_N_STAGES) return AEJ_ERR_ARG;
    ctx->fail_after = stage;
    return 0;
}

extern "C" int aej_get_graph_stats(aej_ctx *ctx, int64_t *out_host)
{
    if (!ctx || !out_host) return AEJ_ERR_ARG;
    out_host[0] = (int64_t)ctx->n_graph_launches;
    out_host[1] = (int64_t)ctx->n_graph_captures;
    out_host[2] = (int64_t)ctx->graphs.size();
    return 0;
}

extern "C" int aej_set_stream(aej_ctx *ctx, void *hip_stream)
{
    AEJ_TRY(enter(ctx, __func__));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (s == ctx->stream) return 0;
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));     // nothing of ours is left running on the stream we leave
    ctx->stream = s;
    return 0;
}

extern "C" int aej_set_profiling(aej_ctx *ctx, int enable)
{
    AEJ_TRY(enter(ctx, __func__));
    ctx->profiling = enable != 0;
    return 0;
}

extern "C" int aej_get_stage_ms(aej_ctx *ctx, float *ms_host)
{
    if (!ctx || !ms_host) return AEJ_ERR_ARG;
    for (int i = 0; i < AEJ_N_STAGES; i++) ms_host[i] = ctx->stage_ms[i];
    return 0;
}

extern "C" const char *aej_stage_name(int i)
{
    static const char *names[AEJ_N_STAGES] = { "clear", "color_planes", "clahe_lut", "clahe_blur", "thresholds", "sobel_nms",
                                               "hysteresis", "quadtree", "dct2", "dct4", "dct8", "dct16", "dct32", "dct64", "dct128", "dct256", "dct512", "dct1024" };
    return i >= 0 && i < AEJ_N_STAGES ? names[i] : "";
}
