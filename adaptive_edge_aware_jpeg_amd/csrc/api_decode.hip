// api_decode.hip -- the decode side of the C ABI (include/aej.h): .ajpg containers (inflate, headers, aej_decode_batch*), requantisation
// and the deflate entries.  Host code only.
#include "aej_ctx.h"

using namespace aej;

// ---- decode path (next-scope row: jpeg.py:274-297) -------------------------------------------------------------
// host helper: Jpeg._block_merge's walk (jpeg.py:424-448): leaf positions from the leaf sizes and the layer geometry
extern "C" int64_t aej_leaf_positions_host(const int32_t *sizes_host, int64_t n, int root, int H, int W, int32_t *xy_host)
{
    if (!sizes_host || !xy_host || n < 0 || root < 1) return -1;
    struct It { int x, y, s; };
    std::vector<It> stack;
    stack.push_back({ 0, 0, root });
    int64_t li = 0;
    while (!stack.empty()) {
        It it = stack.back();
        stack.pop_back();
        if (it.x >= W || it.y >= H || it.s == 0) continue;
        if (li >= n) return -2;      // a node inside the layer is left without a leaf: the sizes do not tile it
        if (it.s == sizes_host[li]) { xy_host[2 * li] = it.x; xy_host[2 * li + 1] = it.y; li++; }
        else {
            int h = it.s / 2;
            stack.push_back({ it.x + h, it.y + h, h });
            stack.push_back({ it.x, it.y + h, h });
            stack.push_back({ it.x + h, it.y, h });
            stack.push_back({ it.x, it.y, h });
        }
    }
    return li;
}

// ---- .ajpg containers decoded on the device (inflate.hip, headers.hip) ----------------------------------------------------------------
extern "C" int aej_inflate_batch(aej_ctx *ctx, const uint8_t *src, const int64_t *streams, int n, uint8_t *dst, uint64_t dst_bytes,
                                 int64_t *out_bytes, int32_t *status)
{
    AEJ_TRY(enter(ctx, __func__));
    if (n < 0) return fail(ctx, AEJ_ERR_ARG, "negative stream count");
    if (n == 0) return 0;
    if (!src || !streams || !dst || !out_bytes || !status) return null_buffer(ctx);
    if (reinterpret_cast<uintptr_t>(src) & 3 || reinterpret_cast<uintptr_t>(dst) & 3) return fail(ctx, AEJ_ERR_ARG, "src and dst must be 4-byte aligned");
    if (dst_bytes > (uint64_t)INT64_MAX) return fail(ctx, AEJ_ERR_ARG, "dst_bytes too large");
    AEJ_TRY(bind_device(ctx));
    launch_inflate(ctx->stream, src, reinterpret_cast<const long long *>(streams), n, dst, (long long)dst_bytes,
                   reinterpret_cast<long long *>(out_bytes), status);
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" uint64_t aej_decode_headers_workspace_bytes(aej_ctx *ctx, int batch, int H, int W)
{
    Geom g;
    QtGeom q;
    if (check_encode_args(ctx, batch, H, W) || make_geoms(ctx, batch, H, W, g, q)) return 0;
    return ((unsigned long long)batch * q.leaf_stride + 255) & ~255ull;         // one log2(size) byte per leaf slot
}

extern "C" int aej_decode_headers(aej_ctx *ctx, const uint8_t *states, const int64_t *layers, const int64_t *inflated_bytes, int batch, int H, int W,
                                  int32_t *leaves, int64_t *counts, int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    AEJ_TRY(check_encode_args(ctx, batch, H, W));
    AEJ_TRY(refuse_in_flight(ctx, __func__));
    if (!states || !layers || !inflated_bytes || !leaves || !counts || !status || !workspace) return null_buffer(ctx);
    if (reinterpret_cast<uintptr_t>(leaves) & 15 || reinterpret_cast<uintptr_t>(workspace) & 15) return fail(ctx, AEJ_ERR_ARG, "leaves and workspace must be 16-byte aligned");
    AEJ_TRY(bind_device(ctx));
    Geom g;
    QtGeom q;
    AEJ_TRY(make_geoms(ctx, batch, H, W, g, q));
    if ((unsigned long long)batch * q.leaf_stride > workspace_bytes)
        return fail(ctx, AEJ_ERR_CAPACITY, "workspace too small: need %llu bytes", (unsigned long long)batch * q.leaf_stride);
    HdrGeom hg;
    hg.bmin = q.bmin;
    hg.bmax = q.bmax;
    for (int l = 0; l < 3; l++) {
        hg.h[l] = g.h[l];
        hg.w[l] = g.w[l];
        hg.proot[l] = q.root[l];
        hg.leaf_off[l] = q.leaf_off[l];
        hg.leaf_span[l] = (l < 2 ? q.leaf_off[l + 1] : q.leaf_stride) - q.leaf_off[l];
        hg.coeff_span[l] = (l < 2 ? q.coeff_off[l + 1] : q.coeff_stride) - q.coeff_off[l];
    }
    hg.leaf_stride = q.leaf_stride;
    launch_headers(ctx->stream, states, reinterpret_cast<const long long *>(layers), reinterpret_cast<const long long *>(inflated_bytes), batch * 3, hg,
                   static_cast<unsigned char *>(workspace), leaves, reinterpret_cast<long long *>(counts), status);
    AEJ_HIP_CHECK(hipGetLastError());
    return 0;
}

struct DecodeWs {
    float *big;
    float *planes;
    int *work_count;
    LeafWork *work[kMaxSizes];
    long long work_cap[kMaxSizes];
    unsigned long long bytes;
};

static void carve_decode(void *base, const Geom &g, const QtGeom &q, DecodeWs &w)
{
    Carver c(base);
    w.planes = c.take<float>((long long)g.B * g.pstride);
    w.work_count = c.take<int>((long long)g.B * 3 * kMaxSizes + 1);       // + 1: the "tables do not fit the plan" flag
    for (int k = 0; k < kMaxSizes; k++) { w.work[k] = nullptr; w.work_cap[k] = 0; }
    for (int k = 0; k < q.nsizes; k++) {
        w.work_cap[k] = q.work_stride[k] * g.B;
        w.work[k] = c.take<LeafWork>(w.work_cap[k] > 0 ? w.work_cap[k] : 1);
    }
    w.big = big_scratch_floats(q.bmax) ? c.take<float>(big_scratch_floats(q.bmax)) : nullptr;
    w.bytes = c.bytes();
}

extern "C" uint64_t aej_decode_workspace_bytes(aej_ctx *ctx, int batch, int H, int W)
{
    Geom g;
    QtGeom q;
    if (check_encode_args(ctx, batch, H, W) || make_geoms(ctx, batch, H, W, g, q)) return 0;
    DecodeWs w;
    carve_decode(nullptr, g, q, w);
    return w.bytes;
}

// aej_decode_batch with the dequantisation tables qm[layer][size index] (the context's, or one set of a device blob)
static int decode_batch_impl(aej_ctx *ctx, const char *who, const int32_t *coeffs, const int32_t *leaves, const int64_t *counts, int batch, int H, int W,
                             const int *const qm[3][kMaxSizes], float *rgb_out, void *workspace, uint64_t workspace_bytes)
{
    AEJ_TRY(check_encode_args(ctx, batch, H, W));
    AEJ_TRY(refuse_in_flight(ctx, who));
    if (!coeffs || !leaves || !counts || !rgb_out || !workspace) return null_buffer(ctx);
    AEJ_TRY(bind_device(ctx));
    Geom g;
    QtGeom q;
    AEJ_TRY(make_geoms(ctx, batch, H, W, g, q));
    DecodeWs w;
    carve_decode(workspace, g, q, w);
    if (w.bytes > workspace_bytes) return fail(ctx, AEJ_ERR_CAPACITY, "workspace too small: need %llu bytes", w.bytes);
    hipStream_t st = ctx->stream;
    int *bad = w.work_count + (size_t)batch * 3 * kMaxSizes;
    AEJ_HIP_CHECK(hipMemsetAsync(w.work_count, 0, ((size_t)batch * 3 * kMaxSizes + 1) * sizeof(int), st));
    launch_work_from_tables(st, g, q, leaves, reinterpret_cast<const long long *>(counts), w.work, w.work_count, bad);
    int k = 0;
    for (int s = q.bmin; s <= q.bmax; s *= 2, k++) {
        IdctArgs a;
        a.coeffs = coeffs; a.planes = w.planes; a.work = w.work[k]; a.work_count = w.work_count; a.k = k; a.nplanes = batch * 3;
        a.scratch = w.big;
        a.D = ctx->d_D[k]; a.zz = ctx->d_zz[k]; a.zzinv = ctx->d_zzinv[k];
        for (int l = 0; l < 3; l++) { a.qm[l] = qm[l][k]; a.mid[l] = (float)kMid[ctx->space][l]; a.scale[l] = (float)kScale[ctx->space][l]; }
        if (launch_idct(st, s, g, q, a, w.work_cap[k])) return fail(ctx, AEJ_ERR_UNSUPPORTED, "no IDCT kernel for block size %d with %d planes", s, a.nplanes);
    }
    if (launch_upsample_color(st, ctx->space, g, w.planes, rgb_out)) return fail(ctx, AEJ_ERR_ARG, "bad colour space");
    AEJ_HIP_CHECK(hipGetLastError());
    AEJ_HIP_CHECK(hipMemcpyAsync(ctx->h_flag, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    AEJ_HIP_CHECK(hipStreamSynchronize(st));
    if (*ctx->h_flag) return fail(ctx, AEJ_ERR_ARG, "corrupt stream: the leaf tables do not fit the plan (leaf count, block size outside %d-%d, or too many leaves of one size)", q.bmin, q.bmax);
    return 0;
}

extern "C" int aej_decode_batch(aej_ctx *ctx, const int32_t *coeffs, const int32_t *leaves, const int64_t *counts, int batch, int H, int W,
                                float *rgb_out, void *workspace, uint64_t workspace_bytes)
{
    if (!ctx) return AEJ_ERR_ARG;
    return decode_batch_impl(ctx, __func__, coeffs, leaves, counts, batch, H, W, ctx->d_qm, rgb_out, workspace, workspace_bytes);
}

// the per-layer, per-size quantiser pointers of one set of a [layer][size][s*s] blob laid out for the bound block range
static void qm_of_set(const aej_ctx *ctx, const int32_t *set, const int *qm[3][kMaxSizes])
{
    long long lw = 0;
    for (int s = ctx->bmin; s <= ctx->bmax; s *= 2) lw += (long long)s * s;
    for (int l = 0; l < 3; l++) {
        long long o = l * lw;
        for (int k = 0; k < kMaxSizes; k++) {
            const int s = ctx->bmin << k;
            qm[l][k] = k < ctx->nsizes ? set + o : nullptr;
            if (k < ctx->nsizes) o += (long long)s * s;
        }
    }
}

extern "C" int aej_decode_batch_tables(aej_ctx *ctx, const int32_t *coeffs, const int32_t *leaves, const int64_t *counts, int batch, int H, int W,
                                       const int32_t *qmats_dev, float *rgb_out, void *workspace, uint64_t workspace_bytes)
{
    AEJ_TRY(check_encode_args(ctx, batch, H, W));
    if (!qmats_dev) return null_buffer(ctx);
    const int *qm[3][kMaxSizes];
    qm_of_set(ctx, qmats_dev, qm);
    return decode_batch_impl(ctx, __func__, coeffs, leaves, counts, batch, H, W, qm, rgb_out, workspace, workspace_bytes);
}

// ---- requantisation of stored DCT values (requant.hip) --------------------------------------------------------------------
extern "C" int aej_requantise_batch(aej_ctx *ctx, const float *dct_f32, const int32_t *leaves, const int64_t *counts, int batch, int H, int W,
                                    int n_sets, const int32_t *qmats_dev, int32_t *coeffs_out, uint64_t set_stride_elems)
{
    AEJ_TRY(check_encode_args(ctx, batch, H, W));
    AEJ_TRY(refuse_in_flight(ctx, __func__));
    if (!dct_f32 || !leaves || !counts || !qmats_dev || !coeffs_out) return null_buffer(ctx);
    if (n_sets < 1) return fail(ctx, AEJ_ERR_ARG, "n_sets must be at least 1 (got %d)", n_sets);
    AEJ_TRY(bind_device(ctx));
    Geom g;
    QtGeom q;
    AEJ_TRY(make_geoms(ctx, batch, H, W, g, q));
    const unsigned long long need = (unsigned long long)batch * q.coeff_stride;
    if (n_sets > 1 && set_stride_elems < need)
        return fail(ctx, AEJ_ERR_ARG, "set_stride_elems %llu is smaller than the batch's coefficients (%llu)", (unsigned long long)set_stride_elems, need);
    long long lw = 0;
    for (int s = ctx->bmin; s <= ctx->bmax; s *= 2) lw += (long long)s * s;
    long long maxcap = 0;
    for (int l = 0; l < 3; l++) maxcap = std::max(maxcap, q.coeff_cap[l]);
    const int blocks = (int)std::min<long long>(512, std::max<long long>(1, (maxcap + 16383) / 16384));
    hipStream_t st = ctx->stream;
    AEJ_HIP_CHECK(hipMemsetAsync(ctx->d_check, 0, sizeof(int), st));
    launch_requant_check(st, g, q, leaves, reinterpret_cast<const long long *>(counts), qmats_dev, (long long)n_sets * 3 * lw, ctx->d_check);
    launch_requant(st, g, q, dct_f32, leaves, reinterpret_cast<const long long *>(counts), n_sets, qmats_dev, ctx->d_zz, coeffs_out,
                   (long long)set_stride_elems, ctx->d_check, blocks);
    AEJ_HIP_CHECK(hipGetLastError());
    AEJ_HIP_CHECK(hipMemcpyAsync(ctx->h_flag, ctx->d_check, sizeof(int), hipMemcpyDeviceToHost, st));
    AEJ_HIP_CHECK(hipStreamSynchronize(st));
    if (*ctx->h_flag == 2) return fail(ctx, AEJ_ERR_ARG, "quantisation matrix entries must be >= 1");
    if (*ctx->h_flag) return fail(ctx, AEJ_ERR_ARG, "the leaf tables do not fit the plan (leaf count, block size outside %d-%d, origin or coefficient offset outside the layer)", q.bmin, q.bmax);
    return 0;
}

// ---- opt-in GPU entropy stage (deflate.hip) -----------------------------------------------------------------------
static int deflate_geometry(aej_ctx *ctx, int batch, int H, int W, QtGeom &q)
{
    AEJ_TRY(check_encode_args(ctx, batch, H, W));
    Geom g;
    return make_geoms(ctx, batch, H, W, g, q);
}

extern "C" uint64_t aej_deflate_stream_bound(uint64_t raw_bytes) { return deflate_stream_bound(raw_bytes); }

// host only (no context, no device): the per-layer dynamic codes from the histograms aej_deflate_histogram counted
namespace aej { int deflate_build_table_host(const int *hist /* [320] */, int cover_all, unsigned *table /* [448] */); }      // deflate.hip
extern "C" int aej_deflate_build_tables(const int32_t *hist_host, const int32_t *cover_all, uint32_t *tables_host)
{
    if (!hist_host || !tables_host) return AEJ_ERR_ARG;
    for (int l = 0; l < 3; l++)
        if (deflate_build_table_host(hist_host + l * AEJ_DEFLATE_HIST_BINS, cover_all ? cover_all[l] : 1, tables_host + l * AEJ_DEFLATE_TABLE_WORDS)) return AEJ_ERR_CAPACITY;
    return 0;
}

// host only: 8-bit ingest of a host float32 batch (include/aej.h)
extern "C" int aej_pack_u8_levels_host(const float *rgb_host, int64_t n, uint8_t *u8_host, int threads)
{
    if (!rgb_host || !u8_host || n < 0) return AEJ_ERR_ARG;
    float lut[256];
    for (int k = 0; k < 256; k++) lut[k] = (float)k / 255.0f;        // the quotients Image.load forms (image.py:80) and the ingest kernel's table
    const int64_t kBlock = 1 << 16;
    const int64_t nblocks = (n + kBlock - 1) / kBlock;
    int nt = threads < 1 ? 1 : threads > 64 ? 64 : threads;
    if ((int64_t)nt > nblocks) nt = nblocks > 0 ? (int)nblocks : 1;
    std::atomic<int64_t> next(0);
    std::atomic<int> exact(1);
    auto work = [&]() {
        for (;;) {
            const int64_t blk = next.fetch_add(1);
            if (blk >= nblocks || !exact.load(std::memory_order_relaxed)) return;      // (another thread met a value that is no level: stop early)
            const int64_t lo = blk * kBlock, hi = std::min(n, lo + kBlock);
            unsigned bad = 0;
            for (int64_t i = lo; i < hi; i++) {
                const float x = rgb_host[i];
                // x * 255 is within half a unit of k for x = float32(k) / 255; anything outside [0, 255] (or NaN) maps to an entry that cannot compare equal
                float y = x * 255.0f + 0.5f;
                y = y >= 0.0f ? y : 0.0f;                                              // (NaN -> 0: lut[0] == NaN is false)
                const int k = y < 255.5f ? (int)y : 255;
                uint32_t a, b;
                memcpy(&a, &x, 4);
                memcpy(&b, &lut[k], 4);
                bad |= a ^ b;                                                          // bit-exact: -0.0f is not a level either
                u8_host[i] = (uint8_t)k;
            }
            if (bad) { exact.store(0, std::memory_order_relaxed); return; }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    return exact.load();
}

extern "C" uint64_t aej_deflate_workspace_bytes(aej_ctx *ctx, int batch, int H, int W)
{
    QtGeom q;
    if (deflate_geometry(ctx, batch, H, W, q)) return 0;
    return deflate_workspace_bytes(batch, q.coeff_cap);
}

static int deflate_check(aej_ctx *ctx, const char *who, const void *a, const void *b, const void *ws, uint64_t ws_bytes, int batch, const QtGeom &q)
{
    AEJ_TRY(refuse_in_flight(ctx, who));
    if (!a || !b || !ws) return null_buffer(ctx);
    if (ws_bytes < deflate_workspace_bytes(batch, q.coeff_cap)) return fail(ctx, AEJ_ERR_CAPACITY, "workspace too small");
    return 0;
}

// the error word is the workspace's first: 1 = a stream does not fit, 2 = a count beyond its layer's capacity
static int deflate_finish(aej_ctx *ctx, void *workspace, uint64_t stream_stride)
{
    AEJ_HIP_CHECK(hipGetLastError());
    AEJ_HIP_CHECK(hipMemcpyAsync(ctx->h_flag, workspace, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (*ctx->h_flag == 2) return fail(ctx, AEJ_ERR_ARG, "counts: a layer's coefficient count is negative or exceeds the capacity the plan gives it (corrupt or stale counts buffer)");
    if (*ctx->h_flag) return fail(ctx, AEJ_ERR_CAPACITY, "a deflate stream does not fit stream_stride = %llu bytes (aej_deflate_stream_bound gives a safe size)", (unsigned long long)stream_stride);
    return 0;
}

extern "C" int aej_deflate_histogram(aej_ctx *ctx, const int32_t *coeffs, const int64_t *counts, int batch, int H, int W, int32_t *hist, void *workspace,
                                     uint64_t workspace_bytes)
{
    QtGeom q;
    AEJ_TRY(deflate_geometry(ctx, batch, H, W, q));
    if (!hist) return null_buffer(ctx);
    AEJ_TRY(deflate_check(ctx, __func__, coeffs, counts, workspace, workspace_bytes, batch, q));
    AEJ_TRY(bind_device(ctx));
    launch_deflate_parse(ctx->stream, coeffs, reinterpret_cast<const long long *>(counts), batch, q.coeff_stride, q.coeff_off, q.coeff_cap, hist, workspace);
    return deflate_finish(ctx, workspace, 0);
}

extern "C" int aej_deflate_batch(aej_ctx *ctx, const int32_t *coeffs, const int64_t *counts, int batch, int H, int W, const uint32_t *tables, int reuse_parse,
                                 uint8_t *streams, uint64_t stream_stride, int64_t *sizes, void *workspace, uint64_t workspace_bytes)
{
    QtGeom q;
    AEJ_TRY(deflate_geometry(ctx, batch, H, W, q));
    if (!streams || !sizes) return null_buffer(ctx);
    AEJ_TRY(deflate_check(ctx, __func__, coeffs, counts, workspace, workspace_bytes, batch, q));
    if (stream_stride < 16 || (stream_stride & 3)) return fail(ctx, AEJ_ERR_CAPACITY, "stream_stride must be a multiple of 4 and at least 16");
    if ((reinterpret_cast<uintptr_t>(streams) & 3) != 0) return fail(ctx, AEJ_ERR_ARG, "streams must be 4-byte aligned");
    AEJ_TRY(bind_device(ctx));
    launch_deflate(ctx->stream, coeffs, reinterpret_cast<const long long *>(counts), batch, q.coeff_stride, q.coeff_off, q.coeff_cap, tables, reuse_parse ? 1 : 0,
                   streams, stream_stride, reinterpret_cast<long long *>(sizes), workspace);
    return deflate_finish(ctx, workspace, stream_stride);
}

// ---- the deflate of byte streams (csrc/deflate.hip, k_bz_*).  descs_host: [n][6] int64 = offset in `in`, bytes, bytes per pixel, bytes
// per scanline, offset in `out`, bytes of the slot in `out` (the last two are read by aej_deflate_bytes_batch alone)
namespace {
constexpr long long kBzMaxBytes = 1ll << 40;
int bz_files(aej_ctx *ctx, const char *fn, const int64_t *descs, int n, uint64_t in_bytes, bool with_out, uint64_t out_bytes, std::vector<BzFile> &files)
{
    if (n < 1 || !descs) return fail(ctx, AEJ_ERR_ARG, "%s: no streams", fn);
    files.resize((size_t)n);
    long long chunks = 0;
    for (int i = 0; i < n; i++) {
        const int64_t *d = descs + 6 * (int64_t)i;
        BzFile &f = files[(size_t)i];
        if (d[1] < 1 || d[1] > kBzMaxBytes) return fail(ctx, AEJ_ERR_ARG, "%s: stream %d: %lld bytes (1 .. 2^40)", fn, i, (long long)d[1]);
        const unsigned long long whole = ((unsigned long long)d[1] + 3ull) & ~3ull;
        if (d[0] < 0 || (d[0] & 3) || (unsigned long long)d[0] > in_bytes || whole > in_bytes - (unsigned long long)d[0])
            return fail(ctx, AEJ_ERR_ARG, "%s: stream %d: outside the input (whole dwords), or an offset that is no multiple of 4", fn, i);
        if (d[2] < 1 || d[2] > 4 || d[3] < 1 || d[3] > (1 << 26)) return fail(ctx, AEJ_ERR_ARG, "%s: stream %d: bytes per pixel %lld, per scanline %lld", fn, i, (long long)d[2], (long long)d[3]);
        f.in_off = d[0]; f.n_bytes = d[1]; f.bpp = (int)d[2]; f.stride = (int)d[3]; f.out_off = 0; f.out_cap = 0; f.pad = 0;
        if (with_out) {
            if (d[4] < 0 || (d[4] & 3) || d[5] < 16 || (d[5] & 3) || (unsigned long long)d[4] > out_bytes || (unsigned long long)d[5] > out_bytes - (unsigned long long)d[4])
                return fail(ctx, AEJ_ERR_ARG, "%s: stream %d: a slot outside the output, below 16 bytes, or no multiple of 4", fn, i);
            f.out_off = d[4]; f.out_cap = d[5];
        }
        f.chunk0 = (int)chunks;
        chunks += deflate_bytes_chunks(d[1]);
        if (chunks > INT32_MAX) return fail(ctx, AEJ_ERR_ARG, "%s: more than 2^31 chunks in one call", fn);
    }
    return 0;
}
int bz_finish(aej_ctx *ctx, const char *fn, void *workspace)
{
    AEJ_HIP_CHECK(hipGetLastError());
    AEJ_HIP_CHECK(hipMemcpyAsync(ctx->h_flag, workspace, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (*ctx->h_flag) return fail(ctx, AEJ_ERR_CAPACITY, "%s: a deflate stream does not fit its slot (aej_deflate_stream_bound gives a safe size)", fn);
    return 0;
}
}  // namespace

extern "C" uint64_t aej_deflate_bytes_workspace_bytes(const int64_t *descs_host, int n)
{
    if (!descs_host || n < 1) return 0;
    long long chunks = 0;
    for (int i = 0; i < n; i++) {
        const long long b = descs_host[6 * (int64_t)i + 1];
        if (b < 1 || b > kBzMaxBytes) return 0;
        chunks += deflate_bytes_chunks(b);
        if (chunks > INT32_MAX) return 0;
    }
    return deflate_bytes_workspace_bytes(chunks, n);
}

extern "C" int aej_deflate_bytes_build_tables(const int32_t *hist_host, int n, uint32_t *tables_host)
{
    if (!hist_host || !tables_host || n < 1) return AEJ_ERR_ARG;
    for (int i = 0; i < n; i++)
        if (deflate_build_table_host(hist_host + (int64_t)i * AEJ_DEFLATE_HIST_BINS, 0, tables_host + (int64_t)i * AEJ_DEFLATE_TABLE_WORDS)) return AEJ_ERR_CAPACITY;
    return 0;
}

extern "C" int aej_deflate_bytes_histogram(aej_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const int64_t *descs_host, int n, int32_t *hist, void *workspace,
                                           uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!in || !hist || !workspace) return null_buffer(ctx, fn);
    if ((reinterpret_cast<uintptr_t>(in) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return fail(ctx, AEJ_ERR_ARG, "%s: in must be 4-byte and workspace 256-byte aligned", fn);
    std::vector<BzFile> files;
    AEJ_TRY(bz_files(ctx, fn, descs_host, n, in_bytes, false, 0, files));
    AEJ_TRY(check_workspace(ctx, aej_deflate_bytes_workspace_bytes(descs_host, n), workspace_bytes));
    AEJ_TRY(bind_device(ctx));
    launch_deflate_bytes_parse(ctx->stream, in, files.data(), n, hist, workspace);
    return bz_finish(ctx, fn, workspace);
}

extern "C" int aej_deflate_bytes_batch(aej_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const int64_t *descs_host, int n, const uint32_t *tables, int reuse_parse,
                                       uint8_t *out, uint64_t out_bytes, int64_t *sizes, void *workspace, uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (!in || !out || !sizes || !workspace) return null_buffer(ctx, fn);
    if ((reinterpret_cast<uintptr_t>(in) & 3) || (reinterpret_cast<uintptr_t>(out) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(ctx, AEJ_ERR_ARG, "%s: in and out must be 4-byte and workspace 256-byte aligned", fn);
    std::vector<BzFile> files;
    AEJ_TRY(bz_files(ctx, fn, descs_host, n, in_bytes, true, out_bytes, files));
    AEJ_TRY(check_workspace(ctx, aej_deflate_bytes_workspace_bytes(descs_host, n), workspace_bytes));
    AEJ_TRY(bind_device(ctx));
    if (!reuse_parse) launch_deflate_bytes_parse(ctx->stream, in, files.data(), n, nullptr, workspace);
    launch_deflate_bytes(ctx->stream, in, files.data(), n, tables, out, reinterpret_cast<long long *>(sizes), workspace);
    return bz_finish(ctx, fn, workspace);
}
