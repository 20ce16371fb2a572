// api_encode.hip -- the encode side of the C ABI (include/aej.h): workspaces and kernel sequence of the whole path, graph capture,
// sub-batch pipelining, aej_encode_batch* and the stand-alone stage entries.  Host code only.
#include "aej_ctx.h"

using namespace aej;

static void mark(aej_ctx *ctx, int stage)
{
    if (!ctx->profiling || ctx->n_ev >= 24) return;
    if (!ctx->ev[ctx->n_ev] && hipEventCreate(&ctx->ev[ctx->n_ev]) != hipSuccess) return;
    ctx->ev_stage[ctx->n_ev] = stage;   // the stage that ENDS at this event
    (void)hipEventRecord(ctx->ev[ctx->n_ev], ctx->stream);
    ctx->n_ev++;
}

// test instrumentation (aej_test_fail_after_stage): one-shot failure right after `stage` has been enqueued
static int injected_failure(aej_ctx *ctx, int stage)
{
    if (ctx->fail_after != stage) return 0;
    ctx->fail_after = -1;
    ctx->err = std::string("injected failure after stage ") + aej_stage_name(stage);
    return AEJ_ERR_STATE;
}

static void collect_marks(aej_ctx *ctx)
{
    for (int i = 0; i < AEJ_N_STAGES; i++) ctx->stage_ms[i] = 0.f;
    for (int i = 1; i < ctx->n_ev; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev[i - 1], ctx->ev[i]) == hipSuccess && ctx->ev_stage[i] >= 0) ctx->stage_ms[ctx->ev_stage[i]] += ms;
    }
}

// The colour stage of every encode part (a whole call or a sub-batch) waits for the colour stage of the part enqueued before it on
// the same device -- by any context -- and publishes its own completion here.  Within one call this staggers the sub-batches;
// across contexts it keeps two calls in flight out of phase (begun together they would run their HBM-bound stages side by side
// and their issue-bound stages side by side, which gains nothing; one stage apart, colour planes / DCT of one run beside blur /
// Sobel of the other).  Waiting on an event that has long completed costs nothing.
static std::mutex g_chain_mutex;
static hipEvent_t g_last_color_done[kMaxDevices] = {};      // per device; owned by the context that recorded it
static int g_calls_in_flight[kMaxDevices] = {};             // per device: calls between aej_encode_batch_begin and _end (guarded by g_chain_mutex)
static unsigned long long g_priority_streams_dealt = 0;     // part streams the process has created with a priority (guarded by g_chain_mutex): the
                                                            // levels are dealt in creation order, so that parts which run together spread over them

void drop_graphs(aej_ctx *ctx)
{
    for (auto &e : ctx->graphs) if (e.exec) (void)hipGraphExecDestroy(e.exec);
    ctx->graphs.clear();
}

struct CannyWs {
    CannyBuffers cb;
    char *zero_begin, *zero_end;     // region cleared at the start of every call
};

static void carve_canny(Carver &c, const Geom &g, CannyWs &w)
{
    memset(&w, 0, sizeof w);
    long long planes = (long long)g.B * g.pstride;
    long long tiles = hyst_tiles_per_image(g) * g.B;
    w.cb.u8a = c.take<unsigned char>(planes);
    w.cb.u8b = c.take<unsigned char>(planes);
    w.cb.weak = c.take<unsigned long long>((long long)g.B * g.bpstride);
    w.cb.strong = c.take<unsigned long long>((long long)g.B * g.bpstride);
    w.cb.lut = c.take<unsigned char>((long long)g.B * 3 * 16 * 256);
    w.cb.thr = c.take<int>((long long)g.B * 3 * 2);
    w.zero_begin = reinterpret_cast<char *>(c.take<int>(0));
    w.cb.hlist = c.take<int>(hyst_ring_slots(g));
    w.cb.tile_hist = c.take<int>((long long)g.B * 3 * 16 * 256);
    w.cb.blur_hist = c.take<int>((long long)g.B * 3 * 256);
    w.cb.pass_count = c.take<int>(kHystCounters);
    w.cb.hflags = c.take<int>(2 * tiles);
    c.take<int>(0);
    w.zero_end = c.base ? c.base + c.off : nullptr;
}

struct QtWs {
    QtBuffers qb;
    char *zero_begin, *zero_end;
};

static void carve_qt(Carver &c, const Geom &g, const QtGeom &q, bool with_work, QtWs &w)
{
    memset(&w, 0, sizeof w);
    w.zero_begin = reinterpret_cast<char *>(c.take<int>(0));
    w.qb.pyr = c.take<unsigned char>((long long)g.B * q.pyr_stride);
    w.qb.overflow = c.take<int>(1);
    c.take<int>(0);
    w.zero_end = c.base ? c.base + c.off : nullptr;
    w.qb.chunk_cnt = c.take<int>((long long)g.B * q.chunk_stride * kChunkInts);
    w.qb.lane_code = c.take<unsigned short>((long long)g.B * q.chunk_stride * 64);
    if (with_work) {
        w.qb.work_count = c.take<int>((long long)g.B * 3 * kMaxSizes);
        for (int k = 0; k < q.nsizes; k++) {
            long long cap = q.work_stride[k] * g.B;
            w.qb.work_cap[k] = cap;
            w.qb.work[k] = c.take<LeafWork>(cap > 0 ? cap : 1);
        }
    } else {
        w.qb.work_count = nullptr;
    }
}

// bilateralFilter(d = 5, sigmaColor, sigmaSpace) weights (edge_detection.py:37-39,78; OpenCV bilateral_filter): (float)exp(double)
// tables built on the host, once per parameter set
static int ensure_canny_tables(aej_ctx *ctx)
{
    if (ctx->d_color_w) return 0;
    float tab[16 + 256] = { 0 };
    double sigc = ctx->canny.bilateral_sigma_color, sigs = ctx->canny.bilateral_sigma_space;
    if (sigc <= 0) sigc = 1;
    if (sigs <= 0) sigs = 1;
    const double cc = -0.5 / (sigc * sigc), sc = -0.5 / (sigs * sigs);
    for (int i = 0; i < 256; i++) tab[16 + i] = (float)exp((double)i * (double)i * cc);
    int t = 0;
    for (int i = -2; i <= 2; i++)
        for (int j = -2; j <= 2; j++) {
            double r = sqrt((double)i * i + (double)j * j);
            if (r > 2.0) continue;
            tab[t++] = (float)exp(r * r * sc);
        }
    if (!ctx->d_bilateral) AEJ_HIP_CHECK(hipMalloc(&ctx->d_bilateral, sizeof tab));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    AEJ_HIP_CHECK(hipMemcpy(ctx->d_bilateral, tab, sizeof tab, hipMemcpyHostToDevice));
    ctx->d_space_w = ctx->d_bilateral;
    ctx->d_color_w = ctx->d_bilateral + 16;
    return 0;
}

static void apply_canny_params(const aej_ctx *ctx, CannyBuffers &cb)
{
    cb.space_w = ctx->d_space_w;
    cb.color_w = ctx->d_color_w;
    cb.low_q = ctx->canny.canny_low_ratio * 100;       // `canny_low_ratio * 100`, edge_detection.py:81-82
    cb.high_q = ctx->canny.canny_high_ratio * 100;
    cb.clip_limit = ctx->canny.clahe_clip_limit;
    cb.l2 = ctx->canny.use_l2_gradient ? 1 : 0;
}

// ---- Canny chain on a prepared uint8 buffer (cb.u8a) ------------------------------------------------------
// The hysteresis is two launches whatever the image holds: a pass over every tile, then the queue of dirtied tiles drained to the
// fix-point on the device (canny.hip k_hyst_drain) -- no pass count for the host to guess, nothing to read back, nothing to repair.
static int run_canny_chain(aej_ctx *ctx, const Geom &g, CannyWs &w)
{
    hipStream_t st = ctx->stream;
    launch_clahe_pad_hist(st, g, w.cb);
    launch_clahe_lut(st, g, w.cb);
    mark(ctx, AEJ_STAGE_CLAHE_LUT);
    auto publish = [&]() {
        std::lock_guard<std::mutex> lock(g_chain_mutex);
        if (hipEventRecord(ctx->chain_event, st) == hipSuccess) g_last_color_done[ctx->device] = ctx->chain_event;
    };
    launch_clahe_blur(st, g, w.cb);
    mark(ctx, AEJ_STAGE_CLAHE_BLUR);
    if (ctx->chain_hook == 2) publish();
    launch_thresholds(st, g, w.cb);
    mark(ctx, AEJ_STAGE_THRESHOLDS);
    launch_sobel_nms(st, g, w.cb, ctx->tune);
    mark(ctx, AEJ_STAGE_SOBEL_NMS);
    if (ctx->chain_hook == 3) publish();
    launch_hysteresis(st, g, w.cb);
    mark(ctx, AEJ_STAGE_HYSTERESIS);
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}

// The zero-fills are kernels while a hipGraph is being captured: the shipped graph holds kernel nodes only (a graph that also held the
// runtime's memset / memcpy nodes faulted on its second replay inside a PyTorch process in round 2; the record of that is
// profiles/r03_graph_memcpy_nodes_fault.txt, the stand-alone replay of the same node types tools/ubench/graph_memcpy_replay.hip).
static int clear_canny_ws(aej_ctx *ctx, const CannyWs &w)
{
    if (ctx->capturing) launch_zero(ctx->stream, w.zero_begin, (size_t)(w.zero_end - w.zero_begin));       // both ends are 256-byte aligned (Carver)
    else AEJ_HIP_CHECK(hipMemsetAsync(w.zero_begin, 0, (size_t)(w.zero_end - w.zero_begin), ctx->stream));
    return 0;
}

static int run_quadtree(aej_ctx *ctx, const Geom &g, const QtGeom &q, QtWs &w, const unsigned long long *edge_bits)
{
    hipStream_t st = ctx->stream;
    // The fill clears the upper pyramid and the overflow flag.  The pyramid is only read when k_qt_upper runs, and the chunk-run count
    // kernel clears the flag itself: a call that needs neither (the codec's 4 .. 64 blocks) has no fill in front of its quadtree.
    QtRuns runs_of_call;
    const QtRuns *runs = qt_chunk_runs(g, q, ctx->tune, runs_of_call) ? &runs_of_call : nullptr;      // which kernel set serves the call: decided here, once
    if (ctx->capturing) launch_zero(st, w.zero_begin, (size_t)(w.zero_end - w.zero_begin));
    else if (qt_needs_upper(g, q) || !runs) AEJ_HIP_CHECK(hipMemsetAsync(w.zero_begin, 0, (size_t)(w.zero_end - w.zero_begin), st));
    w.qb.edge_bits = edge_bits;
    launch_qt_cells(st, g, q, edge_bits, w.qb);
    launch_qt_count(st, g, q, w.qb, runs);
    launch_qt_scan(st, g, q, w.qb, runs);
    launch_qt_emit(st, g, q, w.qb, runs);
    if (runs) ctx->qt_chunk_launches++;
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- colour planes: fast 4x2-patch kernel when the shape allows it, generic kernel otherwise ---------------------------
// OpenCV resize.cpp computeResizeAreaTab: taps of destination index d are entries off[d]..off[d+1]
static void area_tab(int ssize, int dsize, double scale, std::vector<int> &off, std::vector<int> &si, std::vector<float> &alpha)
{
    off.assign((size_t)dsize + 1, 0); si.clear(); alpha.clear();
    for (int dx = 0; dx < dsize; dx++) {
        double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        double cell = scale < ssize - fsx1 ? scale : ssize - fsx1;
        int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
        if (sx2 > ssize - 1) sx2 = ssize - 1;
        if (sx1 > sx2) sx1 = sx2;
        off[dx] = (int)si.size();
        if (sx1 - fsx1 > 1e-3) { si.push_back(sx1 - 1); alpha.push_back((float)((sx1 - fsx1) / cell)); }
        for (int sx = sx1; sx < sx2; sx++) { si.push_back(sx); alpha.push_back((float)(1.0 / cell)); }
        if (fsx2 - sx2 > 1e-3) {
            double a = fsx2 - sx2;
            if (a > 1.) a = 1.;
            if (a > cell) a = cell;
            si.push_back(sx2); alpha.push_back((float)(a / cell));
        }
    }
    off[dsize] = (int)si.size();
}

static long long area_tab_ints(const Geom &g)      // workspace ints reserved for the tables (upper bound)
{
    return 2LL * (g.w[1] + 1 + g.h[1] + 1) + 2LL * (g.W + 2 * g.w[1] + 2) + 2LL * (g.H + 2 * g.h[1] + 2) + 64;
}

static bool planes_fast_ok(const Geom &g)
{
    bool ok = (g.W % 4) == 0 && (g.H % 2) == 0;
    for (int l = 1; l < 3; l++) ok = ok && g.h[l] * g.rh[l] == g.H && g.w[l] * g.rw[l] == g.W;
    return ok;
}

static int run_color_planes(aej_ctx *ctx, const void *rgb, bool in_u8, const Geom &g, float *raw, float *norm, unsigned char *u8, int *hist,
                            int *tab_ws)
{
    float mid[3], scale[3];
    for (int i = 0; i < 3; i++) { mid[i] = (float)kMid[ctx->space][i]; scale[i] = (float)kScale[ctx->space][i]; }
    if (planes_fast_ok(g)) {
        // the persistent colour streamer beside other parts' kernels (sub-batches, calls in flight): 224 instead of 256 workgroups -- a few CUs
        // without a colour workgroup let the foreground kernels' largest workgroups in sooner (interleaved 3 x: 5.87-5.91 against 5.92-5.97 ms per
        // 64 x 4K step; 192: 5.89-5.91; 160: 5.95-6.06; alone the kernel wants all 256: blocking calls 6.54-6.75 against 6.56-6.68)
        Tuning t = ctx->tune;
        if (t.color_workgroups == 0 && ctx->dct_crowded && ctx->space < 3) t.color_workgroups = 224;
        if (launch_color_planes(ctx->stream, ctx->space, rgb, in_u8, g, mid, scale, raw, norm, u8, hist, t)) return fail(ctx, AEJ_ERR_ARG, "bad colour space");
        return 0;
    }
    AreaTabs t;
    memset(&t, 0, sizeof t);
    // resize(): scale = 1 / (dsize / ssize) in double; the fast integer paths need BOTH scales integral
    double sx = 1.0 / ((double)g.w[1] / (double)g.W), sy = 1.0 / ((double)g.h[1] / (double)g.H);
    int isx = (int)lrint(sx), isy = (int)lrint(sy);
    bool fast = fabs(sx - isx) < 2.220446049250313e-16 && fabs(sy - isy) < 2.220446049250313e-16;
    t.isx = isx; t.isy = isy;
    if (fast) t.mode = (isx == 2 && isy == 2) ? 0 : 1;
    else {
        t.mode = 2;
        if (!tab_ws) return fail(ctx, AEJ_ERR_STATE, "no workspace for the INTER_AREA tables");
        std::vector<int> xoff, xsi, yoff, ysi;
        std::vector<float> xal, yal;
        area_tab(g.W, g.w[1], sx, xoff, xsi, xal);
        area_tab(g.H, g.h[1], sy, yoff, ysi, yal);
        std::vector<int> blob;
        auto put_i = [&](const std::vector<int> &v) { size_t o = blob.size(); blob.insert(blob.end(), v.begin(), v.end()); return o; };
        auto put_f = [&](const std::vector<float> &v) { size_t o = blob.size(); blob.resize(o + v.size()); memcpy(blob.data() + o, v.data(), v.size() * 4); return o; };
        size_t o1 = put_i(xoff), o2 = put_i(xsi), o3 = put_f(xal), o4 = put_i(yoff), o5 = put_i(ysi), o6 = put_f(yal);
        if ((long long)blob.size() > area_tab_ints(g)) return fail(ctx, AEJ_ERR_CAPACITY, "INTER_AREA tables larger than reserved");
        AEJ_HIP_CHECK(hipMemcpyAsync(tab_ws, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));     // blob is a host temporary
        t.xoff = tab_ws + o1; t.xsi = tab_ws + o2; t.xal = reinterpret_cast<const float *>(tab_ws + o3);
        t.yoff = tab_ws + o4; t.ysi = tab_ws + o5; t.yal = reinterpret_cast<const float *>(tab_ws + o6);
    }
    if (launch_color_planes_generic(ctx->stream, ctx->space, rgb, in_u8, g, mid, scale, t, raw, norm, u8, hist)) return fail(ctx, AEJ_ERR_ARG, "bad colour space");
    return 0;
}

// ---- whole path ---------------------------------------------------------------------------------------------
struct EncodeWs {
    float *big;              // scratch of the 256 x 256 DCT kernel (null unless the settings allow that size)
    float *norm;
    int *area_tabs;
    CannyWs canny;
    QtWs qt;
    unsigned long long bytes;
};

static void carve_encode(void *base, const Geom &g, const QtGeom &q, EncodeWs &w)
{
    Carver c(base);
    w.norm = c.take<float>((long long)g.B * g.pstride);
    w.area_tabs = c.take<int>(area_tab_ints(g));
    carve_canny(c, g, w.canny);
    carve_qt(c, g, q, true, w.qt);
    w.big = big_scratch_floats(q.bmax) ? c.take<float>(big_scratch_floats(q.bmax)) : nullptr;
    w.bytes = c.bytes();
}

// bytes of the workspace slice of one sub-batch (sized for the largest of them)
static unsigned long long sub_ws_bytes(Geom g, const QtGeom &q, int nsub)
{
    g.B = (g.B + nsub - 1) / nsub;
    EncodeWs w;
    carve_encode(nullptr, g, q, w);
    return w.bytes;
}

extern "C" int aej_encode_plan(aej_ctx *ctx, int batch, int H, int W, aej_plan *plan)
{
    AEJ_TRY(check_encode_args(ctx, batch, H, W));
    if (!plan) return fail(ctx, AEJ_ERR_ARG, "plan is NULL");
    Geom g;
    QtGeom q;
    AEJ_TRY(make_geoms(ctx, batch, H, W, g, q));
    EncodeWs w;
    carve_encode(nullptr, g, q, w);
    memset(plan, 0, sizeof *plan);
    plan->batch = batch; plan->H = H; plan->W = W;
    for (int l = 0; l < 3; l++) {
        plan->layer_h[l] = g.h[l]; plan->layer_w[l] = g.w[l]; plan->root_size[l] = q.root[l];
        plan->coeff_off[l] = q.coeff_off[l]; plan->leaf_off[l] = q.leaf_off[l]; plan->state_off[l] = q.state_off[l];
    }
    plan->coeff_stride = q.coeff_stride; plan->leaf_stride = q.leaf_stride; plan->state_stride = q.state_stride;
    plan->workspace_bytes = w.bytes;
    // a call that is cut into sub-batches uses one slice per sub-batch (their fixed parts make the sum slightly larger); with the
    // automatic mode the decision can change with later settings, so the plan covers every split the context could choose
    for (int n = 2; n <= aej_ctx::kMaxSub && n <= batch; n++)
        plan->workspace_bytes = std::max<uint64_t>(plan->workspace_bytes, sub_ws_bytes(g, q, n) * (unsigned long long)n);
    return 0;
}

// everything behind the hysteresis: quadtree, then one DCT launch per block size
constexpr long long kGraphAutoPixels = 8LL << 20;      // latency-sized calls: at most 8 Mpx (automatic graph mode, the one-launch DCT)

static int enqueue_back(aej_ctx *ctx, const Geom &g, const QtGeom &q, EncodeWs &w, int32_t *coeffs, float *dct_f32)
{
    hipStream_t st = ctx->stream;
    AEJ_TRY(run_quadtree(ctx, g, q, w.qt, w.canny.cb.strong));
    mark(ctx, AEJ_STAGE_QUADTREE);
    DctArgs args[kMaxSizes];
    int k = 0;
    for (int s = q.bmin; s <= q.bmax; s *= 2, k++) {
        DctArgs &a = args[k];
        a.norm = w.norm; a.coeffs = coeffs; a.dct_f32 = dct_f32;
        a.work = w.qt.qb.work[k]; a.work_count = w.qt.qb.work_count; a.k = k; a.nplanes = g.B * 3;
        a.scratch = w.big;
        a.D = ctx->d_D[k]; a.zzinv = ctx->d_zzinv[k];
        a.crowded = ctx->dct_crowded;
        for (int l = 0; l < 3; l++) a.qm[l] = ctx->d_qm[l][k];
    }
    // latency-sized, unprofiled calls: every size in one launch (per-size stage times need per-size launches)
    const bool one_launch = ctx->tune.dct_multi && !ctx->profiling && (long long)g.B * g.H * g.W <= kGraphAutoPixels;
    if (!(one_launch && launch_dct_multi(st, g, q, args, w.qt.qb.work_cap) == 0)) {
        k = 0;
        for (int s = q.bmin; s <= q.bmax; s *= 2, k++) {
            if (launch_dct(st, s, g, q, args[k], w.qt.qb.work_cap[k], ctx->tune)) return fail(ctx, AEJ_ERR_UNSUPPORTED, "no DCT kernel for block size %d with %d planes", s, args[k].nplanes);
            mark(ctx, AEJ_STAGE_DCT_2 + ilog2(s) - 1);
        }
    }
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}

// the counters one call reads back: the quadtree's overflow flag and (a diagnostic) how many tiles went through the hysteresis queue
static int enqueue_readback(aej_ctx *ctx, EncodeWs &w)
{
    AEJ_HIP_CHECK(hipMemcpyAsync(ctx->h_flag, w.qt.qb.overflow, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    AEJ_HIP_CHECK(hipMemcpyAsync(ctx->h_flag + 1, w.canny.cb.pass_count + 32 /* kQTail */, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

constexpr size_t kMaxGraphs = 8;

// Launch-latency path: the whole sequence (about 20 launches for 4-64 blocks) as ONE hipGraphLaunch.  The graph is captured
// on a private stream (the caller's may be the legacy null stream, which cannot be captured) ordered behind the caller's stream
// by an event, and cached under every pointer / shape its kernel arguments contain.
static int encode_graph(aej_ctx *ctx, const void *rgb, bool in_u8, const Geom &g, const QtGeom &q, EncodeWs &w, int32_t *coeffs, int32_t *leaves,
                        uint8_t *states, int64_t *counts, float *dct_f32, void *workspace, bool &used)
{
    used = false;
    if (!ctx->gstream) {
        AEJ_HIP_CHECK(hipStreamCreateWithFlags(&ctx->gstream, hipStreamNonBlocking));
        AEJ_HIP_CHECK(hipEventCreateWithFlags(&ctx->gevent, hipEventDisableTiming));
    }
    aej_ctx::GraphEntry *hit = nullptr;
    for (auto &e : ctx->graphs)
        if (e.rgb == rgb && e.coeffs == coeffs && e.leaves == leaves && e.states == states && e.counts == counts && e.dct == dct_f32 && e.ws == workspace &&
            e.batch == g.B && e.H == g.H && e.W == g.W && e.in_u8 == (int)in_u8) { hit = &e; break; }
    hipStream_t user = ctx->stream;
    if (!hit) {
        // first sight of this combination of buffers: only remember it and let the caller run the ordinary path -- a caller that
        // allocates fresh outputs for every call would otherwise pay a capture per call; the second sight captures
        if (ctx->graphs.size() >= kMaxGraphs) {           // evict the least recently used
            size_t lru = 0;
            for (size_t i = 1; i < ctx->graphs.size(); i++) if (ctx->graphs[i].last_use < ctx->graphs[lru].last_use) lru = i;
            if (ctx->graphs[lru].exec) (void)hipGraphExecDestroy(ctx->graphs[lru].exec);
            ctx->graphs.erase(ctx->graphs.begin() + (long)lru);
        }
        ctx->graphs.push_back({ rgb, coeffs, leaves, states, counts, dct_f32, workspace, g.B, g.H, g.W, (int)in_u8, nullptr, ++ctx->graph_clock });
        return 0;
    }
    if (!hit->exec) {
        hipGraph_t graph = nullptr;
        ctx->stream = ctx->gstream;                       // every enqueue below goes to the capturing stream
        ctx->capturing = true;
        hipError_t e = hipStreamBeginCapture(ctx->gstream, hipStreamCaptureModeThreadLocal);
        int rc = e == hipSuccess ? 0 : hip_fail(ctx, e, "hipStreamBeginCapture", __FILE__, __LINE__);
        if (!rc) rc = clear_canny_ws(ctx, w.canny);
        if (!rc) rc = run_color_planes(ctx, rgb, in_u8, g, nullptr, w.norm, w.canny.cb.u8a, w.canny.cb.tile_hist, w.area_tabs);
        if (!rc) {
            hipStream_t st = ctx->stream;
            launch_clahe_pad_hist(st, g, w.canny.cb);
            launch_clahe_lut(st, g, w.canny.cb);
            launch_clahe_blur(st, g, w.canny.cb);
            launch_thresholds(st, g, w.canny.cb);
            launch_sobel_nms(st, g, w.canny.cb, ctx->tune);
            launch_hysteresis(st, g, w.canny.cb);
            rc = enqueue_back(ctx, g, q, w, coeffs, dct_f32);
        }
        hipError_t e2 = e == hipSuccess ? hipStreamEndCapture(ctx->gstream, &graph) : hipSuccess;
        ctx->stream = user;
        ctx->capturing = false;
        if (rc || e2 != hipSuccess || !graph) {
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            return rc ? rc : 0;                           // not captured: the caller runs the ordinary path
        }
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess || !exec) { (void)hipGetLastError(); return 0; }
        hit->exec = exec;
        ctx->n_graph_captures++;
    }
    hit->last_use = ++ctx->graph_clock;
    AEJ_HIP_CHECK(hipEventRecord(ctx->gevent, user));     // inputs produced on the caller's stream are complete before the graph reads them
    AEJ_HIP_CHECK(hipStreamWaitEvent(ctx->gstream, ctx->gevent, 0));
    AEJ_HIP_CHECK(hipGraphLaunch(hit->exec, ctx->gstream));
    // the counter read-back stays outside the graph (ordinary copies behind it on the same stream): kernel nodes only, see clear_canny_ws
    ctx->stream = ctx->gstream;
    const int rb = enqueue_readback(ctx, w);
    ctx->stream = user;
    if (rb) return rb;
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->gstream));
    ctx->n_graph_launches++;
    used = true;
    return 0;
}

// ---- sub-batch pipelining ------------------------------------------------------------------------------------
// How many sub-batches a call is cut into (automatic mode: by call size and by how many hardware queues the process has, below;
// smaller calls have too few workgroups per kernel to share the chip).  Never for profiled calls (the
// stage timings describe the serial chain), graph replay, or shapes that need the host-built INTER_AREA tables.
static int sub_batches(const aej_ctx *ctx, const Geom &g, int hw_queues, bool as_if_unprofiled = false)
{
    if (ctx->sub_mode == 1 || (ctx->profiling && !as_if_unprofiled) || ctx->graph_mode == 2 || !planes_fast_ok(g)) return 1;
    int n = ctx->sub_mode;
    if (n == 0) {
        const long long px = (long long)g.B * g.H * g.W;
        if (hw_queues >= 8) {
            // every stream has a hardware queue of its own: four chains for a 64 x 4K call, two for a 64 x 1080p or 8 x 8K one, also
            // beside a call in flight on another context (64 x 4K, two contexts: 7.45 ms with 4 sub-batches each, 7.5 with 2, 7.75 with
            // none, 8.2 with 8; 64 x 1080p: 2.11 ms with 2, 2.26 with 4)
            n = (px >= (384LL << 20) && g.B >= 16) ? 4 : (px >= (64LL << 20) && g.B >= 8) ? 2 : 1;
        } else {
            // HIP's default of 4 hardware queues: streams start to share queues (two streams on one queue run one after the other), so
            // two sub-batches, and only for a call that has the device to itself (with 4 queues: 4 sub-batches 8.4 ms, 2: 8.1 ms).
            // Stream priorities (ensure_sub_streams) give those two streams queues of their own; the count stays at two, because a
            // context that had made four would keep two idle streams on the queues that the parts of other contexts then have to
            // share (profiles/stream_priorities_ab.txt: 5.96 against 5.62 ms per pipelined step).
            bool alone;
            { std::lock_guard<std::mutex> lock(g_chain_mutex); alone = g_calls_in_flight[ctx->device] == 0; }
            n = (alone && px >= (64LL << 20) && g.B >= 8) ? 2 : 1;
        }
    }
    if (n > aej_ctx::kMaxSub) n = aej_ctx::kMaxSub;
    if (n > g.B) n = g.B;
    return n;
}

// One call in flight: everything aej_encode_batch_end needs to complete and check what aej_encode_batch_begin enqueued.  Part 0 is the
// whole batch on the context's stream, or parts 0..n-1 are the sub-batches.
struct EncodePart { Geom g; EncodeWs w; bool whole_call = false; int32_t *coeffs = nullptr; float *dct = nullptr; hipStream_t stream = nullptr; int *flag = nullptr; bool used = false; };
struct aej_pending {
    bool active = false, complete = false;     // complete: already synchronised and verified (graph replay)
    QtGeom q;
    std::vector<EncodePart> parts;
};

bool call_in_flight(const aej_ctx *ctx) { return ctx->pending && ctx->pending->active; }

void release_encode_state(aej_ctx *ctx)
{
    if (call_in_flight(ctx)) {
        (void)hipDeviceSynchronize();
        std::lock_guard<std::mutex> lock(g_chain_mutex);
        if (g_calls_in_flight[ctx->device] > 0) g_calls_in_flight[ctx->device]--;
    }
    delete ctx->pending;
    ctx->pending = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_chain_mutex);
        for (int i = 0; i < aej_ctx::kMaxSub; i++)
            if (ctx->sub_color_done[i] && g_last_color_done[ctx->device] == ctx->sub_color_done[i]) g_last_color_done[ctx->device] = nullptr;
    }
    drop_graphs(ctx);
}

static aej_pending &pending_of(aej_ctx *ctx)
{
    if (!ctx->pending) ctx->pending = new aej_pending;
    return *ctx->pending;
}

// the launch sequence of one part on ctx->stream / ctx->h_flag (both set by the caller): clear, colour planes, Canny chain, quadtree,
// DCT, counter read-back.  `after` / `done`: sub-batch staggering (null for the unsplit call).
static int enqueue_part(aej_ctx *ctx, EncodePart &p, const QtGeom &q, const void *rgb, bool in_u8, hipEvent_t done)
{
    int rc;
    mark(ctx, -1);
    AEJ_TRY(clear_canny_ws(ctx, p.w.canny));
    mark(ctx, AEJ_STAGE_CLEAR);
    // one stage behind the part enqueued before this one (g_last_color_done): its colour stage (HBM-bound) has finished, its blur
    // (issue-bound) is starting
    const bool chain = ctx->sub_chain && done && !ctx->profiling;
    const int chain_mode = ctx->sub_chain > 0 ? ctx->sub_chain : 1;
    if (chain) {
        std::lock_guard<std::mutex> lock(g_chain_mutex);
        if (hipEvent_t after = g_last_color_done[ctx->device]) AEJ_HIP_CHECK(hipStreamWaitEvent(ctx->stream, after, 0));
    }
    AEJ_TRY(run_color_planes(ctx, rgb, in_u8, p.g, nullptr, p.w.norm, p.w.canny.cb.u8a, p.w.canny.cb.tile_hist, p.w.area_tabs));
    mark(ctx, AEJ_STAGE_COLOR_PLANES);
    AEJ_TRY(injected_failure(ctx, AEJ_STAGE_COLOR_PLANES));
    auto publish = [&]() -> int {
        std::lock_guard<std::mutex> lock(g_chain_mutex);
        AEJ_HIP_CHECK(hipEventRecord(done, ctx->stream));
        g_last_color_done[ctx->device] = done;
        return 0;
    };
    if (chain && chain_mode == 1 && (rc = publish())) return rc;
    // (the hook is cleared on every exit: a later stand-alone aej_canny on this context must not re-record the shared chain event)
    struct HookGuard { aej_ctx *c; ~HookGuard() { c->chain_hook = 0; } } hook_guard{ ctx };
    ctx->chain_hook = (chain && chain_mode > 1) ? chain_mode : 0;
    ctx->chain_event = done;
    AEJ_TRY(run_canny_chain(ctx, p.g, p.w.canny));
    ctx->chain_hook = 0;
    AEJ_TRY(injected_failure(ctx, AEJ_STAGE_HYSTERESIS));
    AEJ_TRY(enqueue_back(ctx, p.g, q, p.w, p.coeffs, p.dct));
    AEJ_TRY(injected_failure(ctx, AEJ_STAGE_DCT_64));
    return enqueue_readback(ctx, p.w);      // one read-back for the whole part
}

// (the streams are idle: no call of the context is in flight; aej_destroy frees whatever is left)
static void destroy_sub_streams(aej_ctx *ctx)
{
    for (int i = 0; i < aej_ctx::kMaxSub; i++)
        if (ctx->sub_stream[i]) { (void)hipStreamDestroy(ctx->sub_stream[i]); ctx->sub_stream[i] = nullptr; }
    ctx->n_priority_streams = 0;
}

// The part streams of a call cut into nsub.  Those that are missing are all created here, in one go: streams that run together are
// created together (EXPERIMENTS.md R5-8, R5-9).  With fewer than 8 hardware queues (aej_sched.h priorities_in_use) they are created with
// priorities, dealt process-wide in creation order, and the runtime serves each level from a queue pool of its own; with 8 or more
// they are created as they always were.  Streams made under another setting of the option are replaced (they are idle: no call of
// this context is in flight).
static int ensure_sub_streams(aej_ctx *ctx, int nsub)
{
    const bool prio = priorities_in_use(ctx->stream_priorities, ctx->hw_queues);
    const int key = prio ? 1 + ctx->stream_priority_pattern : 0;
    if (key != ctx->sub_stream_key) destroy_sub_streams(ctx);
    ctx->sub_stream_key = key;
    int value_of[3] = { 0, 0, 0 };      // PriorityLevel -> the runtime's number (normal is 0, a smaller number is a higher priority)
    if (prio) {
        int least = 0, greatest = 0;
        AEJ_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        value_of[kPrioHigh] = greatest;
        value_of[kPrioLow] = least;
    }
    std::lock_guard<std::mutex> lock(g_chain_mutex);
    for (int i = 0; i < nsub; i++) {
        if (ctx->sub_stream[i]) continue;
        if (prio) {
            const int level = priority_level_of(ctx->stream_priority_pattern, g_priority_streams_dealt);
            AEJ_HIP_CHECK(hipStreamCreateWithPriority(&ctx->sub_stream[i], hipStreamNonBlocking, value_of[level]));
            g_priority_streams_dealt++;
            ctx->n_priority_streams++;
        } else {
            AEJ_HIP_CHECK(hipStreamCreateWithFlags(&ctx->sub_stream[i], hipStreamNonBlocking));
        }
    }
    return 0;
}

static int encode_begin_impl(aej_ctx *ctx, const void *rgb, bool in_u8, int batch, int H, int W, int32_t *coeffs, int32_t *leaves,
                             uint8_t *states, int64_t *counts, float *dct_f32, void *workspace, uint64_t workspace_bytes, bool &started)
{
    started = false;            // true once this call has put something in flight (then aej_encode_batch_end has to follow, also after an error)
    AEJ_TRY(check_encode_args(ctx, batch, H, W));
    if (!rgb || !coeffs || !leaves || !states || !counts || !workspace) return null_buffer(ctx);
    aej_pending &pd = pending_of(ctx);
    if (pd.active) return fail(ctx, AEJ_ERR_STATE, "aej_encode_batch_begin: the previous call has not been ended (aej_encode_batch_end)");
    AEJ_TRY(bind_device(ctx));
    Geom g;
    AEJ_TRY(make_geoms(ctx, batch, H, W, g, pd.q));
    const QtGeom &q = pd.q;
    AEJ_TRY(ensure_canny_tables(ctx));
    ctx->n_ev = 0;
    ctx->n_encode_calls++;
    const int nsub = sub_batches(ctx, g, ctx->hw_queues);
    {
        std::lock_guard<std::mutex> lock(g_chain_mutex);
        ctx->dct_crowded = nsub > 1 || g_calls_in_flight[ctx->device] > 0;
    }
    // (a profiled call runs unsplit so that its stage times describe the serial chain, but with the kernels the same call uses unprofiled)
    if (ctx->profiling && sub_batches(ctx, g, ctx->hw_queues, true) > 1) ctx->dct_crowded = 1;
    pd.parts.assign((size_t)nsub, EncodePart());
    pd.complete = false;
    hipStream_t user = ctx->stream;
    int *user_flag = ctx->h_flag;
    int rc = 0;

    if (nsub == 1) {
        EncodePart &p = pd.parts[0];
        p.g = g; p.coeffs = coeffs; p.dct = dct_f32; p.stream = user; p.flag = user_flag; p.used = true; p.whole_call = true;
        p.g.tiled = planes_fast_ok(p.g) && color_planes_can_tile(p.g, ctx->space, in_u8, ctx->tune);
        carve_encode(workspace, g, q, p.w);
        AEJ_TRY(check_workspace(ctx, p.w.bytes, workspace_bytes));
        apply_canny_params(ctx, p.w.canny.cb);
        p.w.qt.qb.leaves = leaves;
        p.w.qt.qb.states = states;
        p.w.qt.qb.counts = reinterpret_cast<long long *>(counts);
        bool graphed = false;
        const bool want_graph = ctx->graph_mode != 0 && !ctx->profiling && planes_fast_ok(g) &&
                                (ctx->graph_mode == 2 || (long long)batch * H * W <= kGraphAutoPixels);
        // (p.g, not g: capture, replay and a miss repair in encode_end_impl must share one plane layout -- Geom::tiled)
        if (want_graph && (rc = encode_graph(ctx, rgb, in_u8, p.g, q, p.w, coeffs, leaves, states, counts, dct_f32, workspace, graphed))) {
            if (ctx->gstream) (void)hipStreamSynchronize(ctx->gstream);       // a replay whose read-back failed may still be running
            return rc;
        }
        if (graphed) pd.complete = true;      // the replay path has synchronised its own stream
        else {
            if (!ctx->sub_color_done[0]) AEJ_HIP_CHECK(hipEventCreateWithFlags(&ctx->sub_color_done[0], hipEventDisableTiming));
            rc = enqueue_part(ctx, p, q, rgb, in_u8, hyst_tiles_per_image(g) * g.B <= 4096 ? nullptr : ctx->sub_color_done[0]);      // (latency-sized calls stay out of the chain)
        }
        // also after an error: whatever enqueue_part had already put on the stream is drained by the caller (encode_end_impl), exactly as
        // on the sub-batch path below
        pd.active = started = true;
        { std::lock_guard<std::mutex> lock(g_chain_mutex); g_calls_in_flight[ctx->device]++; }
        return rc;
    }

    // ---- sub-batches on private streams
    const unsigned long long slice = sub_ws_bytes(g, q, nsub);
    if (slice * (unsigned long long)nsub > workspace_bytes)
        return fail(ctx, AEJ_ERR_CAPACITY, "workspace too small for %d sub-batches: need %llu bytes, got %llu", nsub, slice * (unsigned long long)nsub,
                    (unsigned long long)workspace_bytes);
    AEJ_TRY(ensure_sub_streams(ctx, nsub));
    for (int i = 0; i < nsub; i++) {
        if (!ctx->sub_color_done[i]) AEJ_HIP_CHECK(hipEventCreateWithFlags(&ctx->sub_color_done[i], hipEventDisableTiming));
        if (!ctx->sub_flag[i]) AEJ_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&ctx->sub_flag[i]), kFlagWords * sizeof(int), hipHostMallocDefault));
    }
    if (!ctx->sub_in) AEJ_HIP_CHECK(hipEventCreateWithFlags(&ctx->sub_in, hipEventDisableTiming));
    AEJ_HIP_CHECK(hipEventRecord(ctx->sub_in, user));          // inputs produced on the caller's stream are complete before any sub-batch reads them
    ctx->n_split_calls++;
    const size_t px_bytes = in_u8 ? 1 : sizeof(float);
    for (int i = 0; i < nsub && !rc; i++) {
        EncodePart &p = pd.parts[(size_t)i];
        const int b0 = (int)((long long)g.B * i / nsub), b1 = (int)((long long)g.B * (i + 1) / nsub);
        p.g = g;
        p.g.B = b1 - b0;
        p.g.tiled = planes_fast_ok(p.g) && color_planes_can_tile(p.g, ctx->space, in_u8, ctx->tune);      // (decided per part: the strip height depends on the part's batch)
        carve_encode(static_cast<char *>(workspace) + (size_t)i * slice, p.g, q, p.w);
        apply_canny_params(ctx, p.w.canny.cb);
        p.w.qt.qb.leaves = leaves + (long long)b0 * q.leaf_stride * 4;
        p.w.qt.qb.states = states + (long long)b0 * q.state_stride;
        p.w.qt.qb.counts = reinterpret_cast<long long *>(counts) + (long long)b0 * 12;
        p.coeffs = coeffs + (long long)b0 * q.coeff_stride;
        p.dct = dct_f32 ? dct_f32 + (long long)b0 * q.coeff_stride : nullptr;
        p.stream = ctx->sub_stream[i];
        p.flag = ctx->sub_flag[i];
        p.used = true;
        const void *in = static_cast<const char *>(rgb) + (size_t)b0 * g.H * g.W * 3 * px_bytes;
        ctx->stream = p.stream;
        ctx->h_flag = p.flag;
        hipError_t e = hipStreamWaitEvent(ctx->stream, ctx->sub_in, 0);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamWaitEvent", __FILE__, __LINE__);
        else rc = enqueue_part(ctx, p, q, in, in_u8, ctx->sub_color_done[i]);
    }
    ctx->stream = user;
    ctx->h_flag = user_flag;
    pd.active = started = true;  // also after an error: the caller drains whatever was enqueued
    { std::lock_guard<std::mutex> lock(g_chain_mutex); g_calls_in_flight[ctx->device]++; }
    return rc;
}

// completion of the call in flight: every stream it used is drained (also after an error: nothing may still be running when the
// caller sees the result) and the device-side counters are checked
static int encode_end_impl(aej_ctx *ctx, int rc_begin)
{
    if (!ctx) return AEJ_ERR_ARG;
    aej_pending &pd = pending_of(ctx);
    if (!pd.active) return rc_begin ? rc_begin : fail(ctx, AEJ_ERR_STATE, "aej_encode_batch_end without a call in flight");
    pd.active = false;
    { std::lock_guard<std::mutex> lock(g_chain_mutex); if (g_calls_in_flight[ctx->device] > 0) g_calls_in_flight[ctx->device]--; }
    (void)bind_device(ctx);
    int rc = rc_begin;
    long long queued = 0;
    for (EncodePart &p : pd.parts) {
        if (!p.used) continue;                    // not reached by a failed begin
        hipError_t e = pd.complete ? hipSuccess : hipStreamSynchronize(p.stream);
        if (e != hipSuccess && !rc) rc = hip_fail(ctx, e, "hipStreamSynchronize", __FILE__, __LINE__);
        if (rc) continue;
        if (p.flag[0]) { rc = fail(ctx, AEJ_ERR_CAPACITY, "internal capacity exceeded in the quadtree emit pass"); continue; }
        // (bit 30 of the queue's tail counter: a wave of the hysteresis work queue waited longer than any correct run can make it -- canny.hip kQPoison)
        if (p.flag[1] & 0x40000000) { rc = fail(ctx, AEJ_ERR_STATE, "the hysteresis work queue did not drain (internal error): the edge maps of this call are not trustworthy"); continue; }
        queued += p.flag[1];
    }
    if (rc) return rc;
    ctx->last_hyst_queued = queued;
    if (ctx->profiling) collect_marks(ctx);
    return 0;
}

static int encode_batch_impl(aej_ctx *ctx, const void *rgb, bool in_u8, int batch, int H, int W, int32_t *coeffs, int32_t *leaves,
                             uint8_t *states, int64_t *counts, float *dct_f32, void *workspace, uint64_t workspace_bytes)
{
    bool started;
    const int rc = encode_begin_impl(ctx, rgb, in_u8, batch, H, W, coeffs, leaves, states, counts, dct_f32, workspace, workspace_bytes, started);
    return started ? encode_end_impl(ctx, rc) : rc;
}

extern "C" int aej_encode_batch_begin(aej_ctx *ctx, const void *rgb, int rgb_is_u8, int batch, int H, int W, int32_t *coeffs, int32_t *leaves,
                                      uint8_t *states, int64_t *counts, float *dct_f32, void *workspace, uint64_t workspace_bytes)
{
    bool started;
    const int rc = encode_begin_impl(ctx, rgb, rgb_is_u8 != 0, batch, H, W, coeffs, leaves, states, counts, dct_f32, workspace, workspace_bytes, started);
    return rc && started ? encode_end_impl(ctx, rc) : rc;      // a failed begin leaves nothing of its own in flight
}

extern "C" int aej_encode_batch_end(aej_ctx *ctx) { return encode_end_impl(ctx, 0); }

extern "C" int aej_encode_batch(aej_ctx *ctx, const float *rgb, int batch, int H, int W, int32_t *coeffs, int32_t *leaves,
                                uint8_t *states, int64_t *counts, float *dct_f32, void *workspace, uint64_t workspace_bytes)
{
    return encode_batch_impl(ctx, rgb, false, batch, H, W, coeffs, leaves, states, counts, dct_f32, workspace, workspace_bytes);
}

extern "C" int aej_encode_batch_u8(aej_ctx *ctx, const uint8_t *rgb_u8, int batch, int H, int W, int32_t *coeffs, int32_t *leaves,
                                   uint8_t *states, int64_t *counts, float *dct_f32, void *workspace, uint64_t workspace_bytes)
{
    return encode_batch_impl(ctx, rgb_u8, true, batch, H, W, coeffs, leaves, states, counts, dct_f32, workspace, workspace_bytes);
}

// ---- stage entry points ---------------------------------------------------------------------------------------
// the pointwise transform and its inverse (the decode side's): the same checks around either launch
static int color_convert(aej_ctx *ctx, const char *fn, decltype(launch_color_convert) *launch, int space, const float *in, float *out, int64_t n)
{
    AEJ_TRY(enter(ctx, fn));
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, AEJ_ERR_ARG, "bad buffer");
    if (n == 0) return 0;
    AEJ_TRY(bind_device(ctx));
    if (launch(ctx->stream, space, in, out, n)) return fail(ctx, AEJ_ERR_ARG, "Invalid color space id %d", space);
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int aej_color_convert(aej_ctx *ctx, int space, const float *rgb, float *out, int64_t n)
{
    return color_convert(ctx, __func__, launch_color_convert, space, rgb, out, n);
}

extern "C" int aej_color_convert_inverse(aej_ctx *ctx, int space, const float *in, float *out_rgb, int64_t n)
{
    return color_convert(ctx, __func__, launch_color_inverse, space, in, out_rgb, n);
}

extern "C" int aej_color_planes(aej_ctx *ctx, const float *rgb, int batch, int H, int W, float *planes_raw, float *planes_norm,
                                uint8_t *planes_u8)
{
    AEJ_TRY(check_encode_args(ctx, batch, H, W));
    AEJ_TRY(refuse_in_flight(ctx, __func__));
    AEJ_TRY(bind_device(ctx));
    Geom g;
    AEJ_TRY(make_geom(ctx, ctx->space, batch, H, W, g));
    int *tabs = nullptr;
    if (!planes_fast_ok(g)) AEJ_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&tabs), (size_t)area_tab_ints(g) * 4));   // stage entry only
    const int rc = run_color_planes(ctx, rgb, false, g, planes_raw, planes_norm, planes_u8, nullptr, tabs);
    if (tabs) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(tabs); }
    if (rc) return rc;
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" uint64_t aej_canny_workspace_bytes(int H, int W)
{
    if (H < 1 || W < 1) return 0;
    Geom g;
    make_plane_geom(H, W, g);
    Carver c(nullptr);
    CannyWs w;
    carve_canny(c, g, w);
    return c.bytes();
}

extern "C" int aej_canny(aej_ctx *ctx, const float *plane, int H, int W, uint8_t *edge, uint8_t *stages, int32_t *thresholds,
                         void *workspace, uint64_t workspace_bytes)
{
    AEJ_TRY(enter(ctx, __func__));
    if (H < 1 || W < 1) return fail(ctx, AEJ_ERR_ARG, "Input array must be a 2D.");
    AEJ_TRY(check_image_size(ctx, "plane", H, W));
    if (!plane || !edge || !workspace) return null_buffer(ctx);
    if (workspace_bytes < aej_canny_workspace_bytes(H, W)) return fail(ctx, AEJ_ERR_CAPACITY, "workspace too small");
    AEJ_TRY(bind_device(ctx));
    AEJ_TRY(ensure_canny_tables(ctx));
    Geom g;
    make_plane_geom(H, W, g);
    Carver c(workspace);
    CannyWs w;
    carve_canny(c, g, w);
    apply_canny_params(ctx, w.cb);
    long long n = (long long)H * W;
    if (stages) { w.cb.dump_clahe = stages + n; w.cb.dump_gauss = stages + 2 * n; }
    AEJ_TRY(clear_canny_ws(ctx, w));
    launch_plane_u8(ctx->stream, plane, g, w.cb.u8a, w.cb.tile_hist);
    // stage dumps are H*W bytes each; the plane buffers are padded to 64, so copy exactly n bytes
    hipStream_t st = ctx->stream;
    if (stages) AEJ_HIP_CHECK(hipMemcpyAsync(stages, w.cb.u8a, n, hipMemcpyDeviceToDevice, st));
    launch_clahe_pad_hist(st, g, w.cb);
    launch_clahe_lut(st, g, w.cb);
    launch_clahe_blur(st, g, w.cb);
    if (stages) AEJ_HIP_CHECK(hipMemcpyAsync(stages + 3 * n, w.cb.u8b, n, hipMemcpyDeviceToDevice, st));
    launch_thresholds(st, g, w.cb);
    if (thresholds) AEJ_HIP_CHECK(hipMemcpyAsync(thresholds, w.cb.thr, 2 * sizeof(int), hipMemcpyDeviceToDevice, st));
    launch_sobel_nms(st, g, w.cb, ctx->tune);
    Geom ge = g;
    ge.pstride = n;   // uint8 outputs are exactly H*W
    if (stages) launch_bits_to_map(st, ge, w.cb.weak, w.cb.strong, stages + 4 * n);
    launch_hysteresis(st, g, w.cb);
    launch_bits_to_edge(st, ge, w.cb.strong, edge);
    AEJ_HIP_CHECK(hipGetLastError());
    AEJ_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int aej_quadtree_capacity(int H, int W, int min_size, int max_size, int64_t *leaf_cap, int64_t *state_cap, int64_t *coeff_cap)
{
    if (H < 1 || W < 1) return AEJ_ERR_ARG;
    Geom g;
    make_plane_geom(H, W, g);
    QtGeom q;
    AEJ_TRY(make_qtgeom(nullptr, g, min_size, max_size, q, true));
    if (leaf_cap) *leaf_cap = q.leaf_cap[0];
    if (state_cap) *state_cap = q.state_cap[0];
    if (coeff_cap) *coeff_cap = q.coeff_cap[0];
    return 0;
}

extern "C" uint64_t aej_quadtree_workspace_bytes(int H, int W, int min_size, int max_size)
{
    if (H < 1 || W < 1) return 0;
    Geom g;
    make_plane_geom(H, W, g);
    QtGeom q;
    if (make_qtgeom(nullptr, g, min_size, max_size, q, true)) return 0;
    Carver c(nullptr);
    QtWs w;
    carve_qt(c, g, q, false, w);
    c.take<unsigned long long>(g.bpstride);
    return c.bytes();
}

extern "C" int aej_quadtree(aej_ctx *ctx, const uint8_t *edge, int H, int W, int min_size, int max_size, int32_t *leaves,
                            uint8_t *states, int64_t *counts, void *workspace, uint64_t workspace_bytes)
{
    AEJ_TRY(enter(ctx, __func__));
    if (H < 1 || W < 1) return fail(ctx, AEJ_ERR_ARG, "Input array must be a 2D with a single channel.");
    AEJ_TRY(check_image_size(ctx, "edge map", H, W));
    if (!edge || !leaves || !states || !counts || !workspace) return null_buffer(ctx);
    AEJ_TRY(bind_device(ctx));
    Geom g;
    make_plane_geom(H, W, g);
    g.pstride = (long long)H * W;
    QtGeom q;
    AEJ_TRY(make_qtgeom(ctx, g, min_size, max_size, q, true));
    Carver c(workspace);
    QtWs w;
    carve_qt(c, g, q, false, w);
    unsigned long long *bits = c.take<unsigned long long>(g.bpstride);
    if (c.bytes() > workspace_bytes) return fail(ctx, AEJ_ERR_CAPACITY, "workspace too small");
    w.qb.leaves = leaves; w.qb.states = states; w.qb.counts = reinterpret_cast<long long *>(counts);
    launch_pack_edge_bits(ctx->stream, g, edge, bits);
    AEJ_TRY(run_quadtree(ctx, g, q, w, bits));
    AEJ_HIP_CHECK(hipMemcpyAsync(ctx->h_flag, w.qb.overflow, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (*ctx->h_flag) return fail(ctx, AEJ_ERR_CAPACITY, "leaf/state capacity exceeded");
    return 0;
}

extern "C" int aej_dct_quant_zigzag(aej_ctx *ctx, const float *norm, int H, int W, int layer, const int32_t *leaves, int64_t n_leaves,
                                    int32_t *coeffs, float *dct_f32)
{
    AEJ_TRY(enter(ctx, __func__));
    if (!ctx->has_settings) return fail(ctx, AEJ_ERR_STATE, "aej_set_settings has not been called");
    if (H < 1 || W < 1 || layer < 0 || layer > 2 || n_leaves < 0) return fail(ctx, AEJ_ERR_ARG, "bad argument");
    AEJ_TRY(check_image_size(ctx, "plane", H, W));
    if (n_leaves == 0) return 0;
    if (!norm || !leaves || !coeffs) return null_buffer(ctx);
    AEJ_TRY(bind_device(ctx));
    hipStream_t st = ctx->stream;
    // geometry: a single image whose `layer` is the given plane
    Geom g;
    memset(&g, 0, sizeof g);
    g.B = 1; g.nl = 3; g.H = H; g.W = W;
    for (int l = 0; l < 3; l++) { g.h[l] = H; g.w[l] = W; g.rh[l] = g.rw[l] = 1; g.poff[l] = 0; }
    g.pstride = (long long)H * W;
    QtGeom q;
    memset(&q, 0, sizeof q);
    q.bmin = ctx->bmin; q.bmax = ctx->bmax; q.cell = ctx->bmin; q.nsizes = ctx->nsizes;   // work_off / work_stride stay 0
    // stage-only scratch (not on the hot path): per-size work lists
    char *scratch = nullptr;
    size_t list_bytes = (size_t)n_leaves * sizeof(LeafWork);
    size_t total = 256 + (size_t)ctx->nsizes * ((list_bytes + 255) & ~(size_t)255);   // 256 B = [3 planes][kMaxSizes] counters
    const size_t big_off = total;
    total += (size_t)big_scratch_floats(ctx->bmax) * sizeof(float);
    AEJ_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&scratch), total));
    int *work_count = reinterpret_cast<int *>(scratch);
    LeafWork *work[kMaxSizes] = {};
    for (int k = 0; k < ctx->nsizes; k++) work[k] = reinterpret_cast<LeafWork *>(scratch + 256 + (size_t)k * ((list_bytes + 255) & ~(size_t)255));
    hipError_t e = hipMemsetAsync(scratch, 0, 256, st);
    if (e == hipSuccess) {
        launch_work_from_leaves(st, leaves, n_leaves, ctx->bmin, layer, work, work_count);
        int k = 0;
        for (int s = ctx->bmin; s <= ctx->bmax; s *= 2, k++) {
            DctArgs a;
            a.norm = norm; a.coeffs = coeffs; a.dct_f32 = dct_f32;
            a.work = work[k]; a.work_count = work_count; a.k = k; a.nplanes = 3;
            a.scratch = big_scratch_floats(ctx->bmax) ? reinterpret_cast<float *>(scratch + big_off) : nullptr;
            a.D = ctx->d_D[k]; a.zzinv = ctx->d_zzinv[k];
            for (int l = 0; l < 3; l++) a.qm[l] = ctx->d_qm[l][k];
            if (launch_dct(st, s, g, q, a, n_leaves, ctx->tune)) { e = hipErrorInvalidValue; break; }
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipFree(scratch);
    if (e != hipSuccess) return fail(ctx, AEJ_ERR_HIP, "aej_dct_quant_zigzag: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int aej_get_schedule_host(aej_ctx *ctx, int batch, int H, int W, int32_t *out_host)
{
    AEJ_TRY(check_encode_args(ctx, batch, H, W));
    if (!out_host) return fail(ctx, AEJ_ERR_ARG, "out_host is NULL");
    Geom g;
    AEJ_TRY(make_geom(ctx, ctx->space, batch, H, W, g));
    const int n = sub_batches(ctx, g, ctx->hw_queues), n_wide = sub_batches(ctx, g, 16);
    out_host[0] = ctx->hw_queues;
    out_host[1] = n;
    out_host[2] = (ctx->hw_queues < kWideScheduleQueues && n_wide > n) ? 1 : 0;
    out_host[3] = effective_hw_queues(ctx->stream_priorities, ctx->stream_priority_pattern, ctx->hw_queues);      // queues the part streams spread over
    return 0;
}
