// api_jpeg.hip -- the standard-JPEG entries of the C ABI (include/aej.h): baseline and progressive files written (aej_jfif_*) and
// decoded (aej_jpegdec_*, aej_jpegprog_*).  Host code only.
#include "aej_ctx.h"
#include "jfif_restart_core.h"
#include "jfif_stream_core.h"

using namespace aej;

// ---- baseline JPEG as Pillow / libjpeg-turbo writes it (jfif.hip) --------------------------------------------------------------------
static int jfif_args(aej_ctx *ctx, const char *fn, int batch, int H, int W, int n_q, int ss, int opt, JfifGeom &g)
{
    AEJ_TRY(enter(ctx, fn));
    if (ss < 0 || ss > 2) return fail(ctx, AEJ_ERR_ARG, "%s: subsampling %d (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)", fn, ss);
    if (opt != 0 && opt != 1) return fail(ctx, AEJ_ERR_ARG, "%s: optimize %d (0 or 1)", fn, opt);
    if (!jfif_geom(batch, H, W, n_q, g, ss, opt))
        return fail(ctx, AEJ_ERR_ARG, "%s: bad shape %d x %d x %d with %d qualities (1 <= H, W <= 65535)", fn, batch, H, W, n_q);
    return 0;
}

extern "C" uint64_t aej_jfif_workspace_bytes_opt(int batch, int H, int W, int n_q, int subsampling, int optimize)
{
    JfifGeom g;
    if ((optimize != 0 && optimize != 1) || !jfif_geom(batch, H, W, n_q, g, subsampling, optimize)) return 0;
    JfifBufs w;
    return jfif_carve(nullptr, g, w);
}

extern "C" uint64_t aej_jfif_workspace_bytes(int batch, int H, int W, int n_q) { return aej_jfif_workspace_bytes_opt(batch, H, W, n_q, 2, 0); }

extern "C" int aej_jfif_headers_host_opt(int quality, int H, int W, int subsampling, uint8_t *out_host, int capacity)
{
    JfifGeom g;
    if (quality < 1 || quality > 100 || !jfif_geom(1, H, W, 1, g, subsampling, 0) || !out_host) return AEJ_ERR_ARG;
    JfifParams p;
    jfif_params_host(quality, H, W, p, subsampling);
    if (capacity < p.hdr_len) return AEJ_ERR_CAPACITY;
    memcpy(out_host, p.hdr, p.hdr_len);
    return p.hdr_len;
}

extern "C" int aej_jfif_headers_grey_host(int quality, int H, int W, uint8_t *out_host, int capacity)
{
    JfifGeom g;
    if (quality < 1 || quality > 100 || !jfif_geom(1, H, W, 1, g, 0, 0, 1) || !out_host) return AEJ_ERR_ARG;
    JfifParams p;
    jfif_params_host(quality, H, W, p, 0, 1);
    if (capacity < p.hdr_len) return AEJ_ERR_CAPACITY;
    memcpy(out_host, p.hdr, p.hdr_len);
    return p.hdr_len;
}

extern "C" int aej_jfif_headers_host(int quality, int H, int W, uint8_t *out_host, int capacity)
{
    return aej_jfif_headers_host_opt(quality, H, W, 2, out_host, capacity);
}

extern "C" int aej_jfif_huffman_host(const int64_t *counts_host, uint8_t *bits_host, uint8_t *huffval_host, int capacity)
{
    if (!counts_host || !bits_host || !huffval_host || capacity < 0) return AEJ_ERR_ARG;
    unsigned char bits[16], vals[256];
    const int n = jfif_huffman_host((const long long *)counts_host, bits, vals);
    if (n < 0) return AEJ_ERR_ARG;
    if (n > capacity) return AEJ_ERR_CAPACITY;
    memcpy(bits_host, bits, 16);
    memcpy(huffval_host, vals, n);
    return n;
}

// One routine writes the baseline files (optimize 0 / 1) and the progressive ones: `prog` adds the scan geometry, carves jfifprog.hip's
// buffers behind the shared ones, turns the frame marker SOF0 into SOF2 and launches the progressive coder.
static int jfif_encode(aej_ctx *ctx, const char *fn, bool prog, const uint8_t *rgb, int batch, int H, int W, int n_q, const int32_t *qualities_host,
                       int subsampling, int optimize, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host,
                       void *workspace, uint64_t workspace_bytes)
{
    JfifGeom g;
    JfpGeom p;
    AEJ_TRY(jfif_args(ctx, fn, batch, H, W, n_q, subsampling, optimize, g));
    if (prog && !jfifprog_geom(g, p)) return fail(ctx, AEJ_ERR_ARG, "%s: bad shape", fn);
    if (!rgb || !qualities_host || !offsets || !lengths || !total_host || !workspace) return null_buffer(ctx, fn);
    std::vector<JfifParams> par(n_q);
    for (int i = 0; i < n_q; i++) {
        if (qualities_host[i] < 1 || qualities_host[i] > 100) return fail(ctx, AEJ_ERR_ARG, "%s: quality %d outside 1..100", fn, qualities_host[i]);
        jfif_params_host(qualities_host[i], H, W, par[i], subsampling);
        if (!prog) continue;
        unsigned char *sof = par[i].hdr + par[i].dht_off - 19;      // the frame header is the last segment before the tables: SOF0 -> SOF2
        if (par[i].dht_off < 19 || sof[0] != 0xFF || sof[1] != 0xC0) return fail(ctx, AEJ_ERR_STATE, "%s: no SOF0 segment before the tables", fn);
        sof[1] = 0xC2;
    }
    JfifBufs w;
    JfpBufs pw;
    AEJ_TRY(check_workspace(ctx, prog ? jfifprog_carve(workspace, g, p, w, pw) : jfif_carve(workspace, g, w), workspace_bytes));
    AEJ_TRY(bind_device(ctx));
    if (prog) AEJ_HIP_CHECK(launch_jfifprog_encode(ctx->stream, g, p, w, pw, par.data(), rgb, out, out_capacity, (long long *)lengths, (long long *)offsets));
    else AEJ_HIP_CHECK(launch_jfif_encode(ctx->stream, g, w, par.data(), rgb, out, out_capacity, (long long *)lengths, (long long *)offsets));
    long long total = 0;
    AEJ_HIP_CHECK(hipMemcpyAsync(&total, w.total, 8, hipMemcpyDeviceToHost, ctx->stream));      // (the progressive carve points w.total at its own word)
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));     // also keeps `par` alive until its upload has run
    *total_host = (uint64_t)total;
    if (out && (uint64_t)total > out_capacity)
        return fail(ctx, AEJ_ERR_CAPACITY, "%s: the files need %lld bytes, the output holds %llu (nothing was written)", fn, total,
                    (unsigned long long)out_capacity);
    return 0;
}

extern "C" int aej_jfif_encode_batch_opt(aej_ctx *ctx, const uint8_t *rgb, int batch, int H, int W, int n_q, const int32_t *qualities_host,
                                         int subsampling, int optimize, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths,
                                         uint64_t *total_host, void *workspace, uint64_t workspace_bytes)
{
    return jfif_encode(ctx, __func__, false, rgb, batch, H, W, n_q, qualities_host, subsampling, optimize, out, out_capacity, offsets, lengths, total_host,
                       workspace, workspace_bytes);
}

extern "C" int aej_jfif_encode_batch(aej_ctx *ctx, const uint8_t *rgb, int batch, int H, int W, int n_q, const int32_t *qualities_host, uint8_t *out,
                                     uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host, void *workspace,
                                     uint64_t workspace_bytes)
{
    return aej_jfif_encode_batch_opt(ctx, rgb, batch, H, W, n_q, qualities_host, 2, 0, out, out_capacity, offsets, lengths, total_host, workspace,
                                     workspace_bytes);
}

// the reconstruction reads the quantised coefficients either encode left in the workspace: only the carve differs
static int jfif_recon(aej_ctx *ctx, const char *fn, bool prog, int batch, int H, int W, int n_q, int subsampling, int optimize, uint8_t *rgb_out,
                      void *workspace, uint64_t workspace_bytes)
{
    JfifGeom g;
    JfpGeom p;
    AEJ_TRY(jfif_args(ctx, fn, batch, H, W, n_q, subsampling, optimize, g));
    if (prog && !jfifprog_geom(g, p)) return fail(ctx, AEJ_ERR_ARG, "%s: bad shape", fn);
    if (!rgb_out || !workspace) return null_buffer(ctx, fn);
    JfifBufs w;
    JfpBufs pw;
    AEJ_TRY(check_workspace(ctx, prog ? jfifprog_carve(workspace, g, p, w, pw) : jfif_carve(workspace, g, w), workspace_bytes));
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_jfif_recon(ctx->stream, g, w, rgb_out));
    return 0;
}

extern "C" int aej_jfif_recon_batch_opt(aej_ctx *ctx, int batch, int H, int W, int n_q, int subsampling, int optimize, uint8_t *rgb_out,
                                        void *workspace, uint64_t workspace_bytes)
{
    return jfif_recon(ctx, __func__, false, batch, H, W, n_q, subsampling, optimize, rgb_out, workspace, workspace_bytes);
}

extern "C" int aej_jfif_recon_batch(aej_ctx *ctx, int batch, int H, int W, int n_q, uint8_t *rgb_out, void *workspace, uint64_t workspace_bytes)
{
    return aej_jfif_recon_batch_opt(ctx, batch, H, W, n_q, 2, 0, rgb_out, workspace, workspace_bytes);
}

// ---- the progressive file of the same coefficients (jfifprog.hip) --------------------------------------------------------------------------
extern "C" uint64_t aej_jfif_workspace_bytes_prog(int batch, int H, int W, int n_q, int subsampling)
{
    JfifGeom g;
    JfpGeom p;
    if (!jfif_geom(batch, H, W, n_q, g, subsampling, 0) || !jfifprog_geom(g, p)) return 0;
    JfifBufs w;
    JfpBufs pw;
    return jfifprog_carve(nullptr, g, p, w, pw);
}

extern "C" int aej_jfif_encode_batch_prog(aej_ctx *ctx, const uint8_t *rgb, int batch, int H, int W, int n_q, const int32_t *qualities_host,
                                          int subsampling, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths,
                                          uint64_t *total_host, void *workspace, uint64_t workspace_bytes)
{
    return jfif_encode(ctx, __func__, true, rgb, batch, H, W, n_q, qualities_host, subsampling, 0, out, out_capacity, offsets, lengths, total_host, workspace,
                       workspace_bytes);
}

extern "C" int aej_jfif_recon_batch_prog(aej_ctx *ctx, int batch, int H, int W, int n_q, int subsampling, uint8_t *rgb_out, void *workspace,
                                         uint64_t workspace_bytes)
{
    return jfif_recon(ctx, __func__, true, batch, H, W, n_q, subsampling, 0, rgb_out, workspace, workspace_bytes);
}

extern "C" int aej_test_jfif_prog_scan_host(const int16_t *coefs_host, int64_t n_blocks, int Ss, int Se, int Ah, int Al, uint8_t *out_host,
                                            uint64_t capacity, uint64_t *out_len_host, int64_t *counts_host, int64_t *cuts_host)
{
    unsigned long long len = 0;
    const int rc = jfifprog_scan_host(coefs_host, n_blocks, Ss, Se, Ah, Al, out_host, capacity, &len, (long long *)counts_host, (long long *)cuts_host);
    if (out_len_host) *out_len_host = len;
    return rc;
}

extern "C" int aej_test_jfif_seq_scan_host(const int16_t *coefs_host, int64_t n_mcu, int hs, int vs, int ncomp, int restart_interval, int optimize,
                                           int64_t *hist_host, uint8_t *out_host, uint64_t capacity, uint64_t *out_len_host)
{
    if (!out_len_host) return AEJ_ERR_ARG;
    unsigned long long len = 0;
    const int rc = jfif_seq_scan_host(coefs_host, n_mcu, hs, vs, ncomp, restart_interval, optimize, (long long *)hist_host, out_host, capacity, &len);
    *out_len_host = len;
    return rc;
}

extern "C" int aej_test_jfif_prog_scan(aej_ctx *ctx, const int16_t *coefs_host, int64_t n_blocks, int Ss, int Se, int Ah, int Al, uint8_t *out_host,
                                       uint64_t capacity, uint64_t *out_len_host, int64_t *counts_host, int64_t *cuts_host)
{
    AEJ_TRY(enter(ctx, __func__));
    AEJ_TRY(bind_device(ctx));
    unsigned long long len = 0;
    hipError_t e = hipSuccess;
    const int rc = jfifprog_scan_device(ctx->stream, coefs_host, n_blocks, Ss, Se, Ah, Al, out_host, capacity, &len, (long long *)counts_host,
                                        (long long *)cuts_host, &e);
    if (out_len_host) *out_len_host = len;
    if (rc == AEJ_ERR_HIP) AEJ_HIP_CHECK(e);
    if (rc == AEJ_ERR_ARG) return fail(ctx, rc, "%s: bad scan parameters or coefficients", __func__);
    if (rc == AEJ_ERR_CAPACITY) return fail(ctx, rc, "%s: the scan needs %llu bytes", __func__, len);
    return rc;
}

// ---- baseline JPEG files decoded on the device (jpegdec.hip; the marker walk: jpegparse.hip) --------------------------------------------------------------------------
static int jd_parse_host(const uint8_t *data_host, uint64_t nbytes, aej_jpegdec_desc *desc_host, char *msg, int msg_capacity, int layout_440,
                         aej_jpeg_adobe *adobe_host)
{
    if (!desc_host || (layout_440 != 0 && layout_440 != 1)) return AEJ_ERR_ARG;
    std::string m;
    const int rc = jpegdec_parse(data_host, nbytes, *desc_host, m, layout_440 != 0, adobe_host);
    copy_msg(m, msg, msg_capacity);
    return rc;
}

extern "C" int aej_jpegdec_parse_host(const uint8_t *data_host, uint64_t nbytes, aej_jpegdec_desc *desc_host, char *msg, int msg_capacity)
{
    return jd_parse_host(data_host, nbytes, desc_host, msg, msg_capacity, 0, nullptr);
}

extern "C" int aej_jpegdec_parse_host_440(const uint8_t *data_host, uint64_t nbytes, aej_jpegdec_desc *desc_host, char *msg, int msg_capacity,
                                          int layout_440)
{
    return jd_parse_host(data_host, nbytes, desc_host, msg, msg_capacity, layout_440, nullptr);
}

extern "C" int aej_jpegdec_parse_host_adobe(const uint8_t *data_host, uint64_t nbytes, aej_jpegdec_desc *desc_host, aej_jpeg_adobe *adobe_host,
                                            char *msg, int msg_capacity, int layout_440)
{
    if (!adobe_host) return AEJ_ERR_ARG;
    return jd_parse_host(data_host, nbytes, desc_host, msg, msg_capacity, layout_440, adobe_host);
}

// ---- what a call's offsets must satisfy (shared by the decoders and the transcoder) -------------------------------------------------------
static bool inside(long long off, long long len, uint64_t bytes) { return off >= 0 && (uint64_t)off + (uint64_t)len <= bytes; }

// the scan offset of baseline file i checked against the scans buffer and entered into the layout
static int jpegdec_scan_offset(aej_ctx *ctx, const char *fn, const aej_jpegdec_desc &d, int i, uint64_t scans_bytes, long long so, JdFile &file)
{
    if (!inside(so, d.scan_length, scans_bytes)) return fail(ctx, AEJ_ERR_ARG, "%s: file %d: scan outside the scans buffer", fn, i);
    file.scan_off = so;
    return 0;
}

// the same for every scan of the progressive files of a call (data_offsets_host is in the caller's scan order)
static int jpegprog_scan_offsets(aej_ctx *ctx, const char *fn, JpLayout &y, uint64_t data_bytes, const int64_t *data_offsets_host)
{
    for (size_t t = 0; t < y.scans.size(); t++) {
        const long long so = data_offsets_host[y.src[t]];
        if (!inside(so, y.sfiles[t].scan_len, data_bytes)) return fail(ctx, AEJ_ERR_ARG, "%s: scan %d: bytes outside the data buffer", fn, y.src[t]);
        y.sfiles[t].scan_off = so;
    }
    return 0;
}

// the image of file i (RGB, or its luma plane: file.shift) checked against the output and entered into the layout
static int image_offset(aej_ctx *ctx, const char *fn, int i, uint64_t out_bytes, long long oo, JdFile &file)
{
    const long long bytes = (long long)file.ow * file.oh * ((file.shift & kJdCmyk) ? 4 : (file.shift & kJdLuma) ? 1 : 3);
    if (!inside(oo, bytes, out_bytes)) return fail(ctx, AEJ_ERR_ARG, "%s: file %d: image outside the output", fn, i);
    file.out_off = oo;
    return 0;
}

// ---- the options of a decoder call: one set, resolved by one routine for the size query and the call alike ------------------------------
// scales (NULL: every file at full size): 1, 2, 4 or 8 per file.  components (NULL: every file as RGB): 3, 1 for a file that leaves as
// its luma plane, or -- with adobe alone -- 4 for a four-component file that leaves as Pillow's mode "CMYK" image.  boxes (NULL: none):
// [n][4] left, top, right, bottom, in pixels of the full-size image, where only the whole image is taken at scale 2, 4 or 8, or (sbox) in
// pixels of the file's image at its scale, ceil(width / s) x ceil(height / s).  adobe (NULL: none): what the _adobe parsers wrote.
struct JdOptions { const int *scales, *components; const int32_t *boxes; const aej_jpeg_adobe *adobe; bool sbox; };
enum { kJdrOk, kJdrNoFrames, kJdrFour, kJdrComponents, kJdrScale, kJdrBox, kJdrBoxScaled, kJdrAdobeLuma, kJdrAdobeScale, kJdrAdobeBox };
struct JdRefusal { int kind = kJdrOk, file = 0, v[6] = {}; };      // v: the offending value, or the box and the size of its image

// -> what jpegdec_layout / jpegprog_layout take, or the first thing refused, in the order the entries always reported them.  The frames are
// read only for boxes and adobe (aej_jpegprog_*: they are checked only later, by jpegprog_layout).  D: aej_jpegdec_desc or aej_jpegprog_frame
template <class D>
static JdRefusal jd_resolve(const D *frames, int n, const JdOptions &o, JdResolved &r)
{
    std::vector<int> &shifts = r.shifts;
    const bool no_frames = !frames || n < 1;
    r.boxes = o.boxes; r.adobe = o.adobe;
    shifts.assign(n > 0 ? n : 0, 0);
    if (o.adobe && no_frames) return { kJdrNoFrames };
    for (int i = 0; o.adobe && o.components && i < n; i++)
        if (o.components[i] == 4 && (frames[i].ncomp != 4 || !jpeg_adobe_new(o.adobe + i))) return { kJdrFour, i };
    for (int i = 0; o.scales && i < n; i++)
        if ((shifts[i] = jpeg_scale_shift(o.scales[i])) < 0) return { kJdrScale, i, { o.scales[i] } };
    for (int i = 0; o.components && i < n; i++) {
        if (o.components[i] == 1) shifts[i] |= kJdLuma;
        else if (o.components[i] != 3 && !(o.components[i] == 4 && o.adobe)) return { kJdrComponents, i, { o.components[i] } };
    }
    if (o.boxes && no_frames) return { kJdrNoFrames };
    for (int i = 0; o.boxes && i < n; i++) {
        const int32_t *b = o.boxes + 4 * i;
        const int sh = shifts[i] & (kJdLuma - 1), s = o.sbox ? sh : 0, ow = (frames[i].width + (1 << s) - 1) >> s, oh = (frames[i].height + (1 << s) - 1) >> s;
        if (!(0 <= b[0] && b[0] < b[2] && b[2] <= ow && 0 <= b[1] && b[1] < b[3] && b[3] <= oh)) return { kJdrBox, i, { b[0], b[1], b[2], b[3], ow, oh } };
        if (!sh || (b[0] == 0 && b[1] == 0 && b[2] == ow && b[3] == oh)) continue;      // at scale 1 the two kinds of box coincide, and the whole image is no box
        if (!o.sbox) return { kJdrBoxScaled, i };
        shifts[i] |= kJdSbox;                                // a box of the scaled image (jpeg_recon_layout)
    }
    for (int i = 0; o.adobe && i < n; i++) {                 // a four-component or RGB-coded file: full size, whole, in colour
        if (!jpeg_adobe_new(o.adobe + i)) continue;
        if (shifts[i] & kJdLuma) return { kJdrAdobeLuma, i };
        if (shifts[i] & (kJdLuma - 1)) return { kJdrAdobeScale, i };
        if (o.boxes && !jpeg_box_whole(frames[i], o.boxes + 4 * i)) return { kJdrAdobeBox, i };
        if (o.components && o.components[i] == 4) shifts[i] |= kJdCmyk;
    }
    return {};
}

// a refusal in the entry's words (0: none).  The size queries do not come here: they answer 0 and leave the context's last error alone
static int jd_refuse(aej_ctx *ctx, const char *fn, const JdRefusal &r)
{
    const int i = r.file, *v = r.v;
    switch (r.kind) {
    case kJdrOk: return 0;
    case kJdrNoFrames: return fail(ctx, AEJ_ERR_ARG, "%s: no files, or descriptors aej_jpegprog_parse_host did not write", fn);
    case kJdrFour: return fail(ctx, AEJ_ERR_ARG, "%s: file %d: 4 output components for a file that does not have four", fn, i);
    case kJdrComponents: return fail(ctx, AEJ_ERR_ARG, "%s: file %d: %d output components (3: RGB, 1: luma)", fn, i, v[0]);
    case kJdrScale: return fail(ctx, AEJ_ERR_ARG, "%s: file %d: scale %d (1, 2, 4 or 8)", fn, i, v[0]);
    case kJdrBox:
        return fail(ctx, AEJ_ERR_ARG, "%s: file %d: box (%d, %d, %d, %d) is empty or leaves the %d x %d image", fn, i, v[0], v[1], v[2], v[3], v[4], v[5]);
    case kJdrBoxScaled: return fail(ctx, AEJ_ERR_UNSUPPORTED, "%s: file %d: a box at scale 2, 4 or 8 is not built", fn, i);
    }
    return fail(ctx, AEJ_ERR_UNSUPPORTED, "%s: file %d: %s of a four-component / RGB-coded file is not built", fn, i,
                r.kind == kJdrAdobeLuma ? "luma output" : r.kind == kJdrAdobeScale ? "a scale other than 1" : "a box");
}

// jd_sbox_window behind its four public entries: the box in pixels of the image at `scale` (the _box_ entries: 1)
static int sbox_window_host(int width, int height, int hs, int vs, int ncomp, int scale, const int32_t *box4_host, int32_t *window4_out_host)
{
    const int sh = jpeg_scale_shift(scale);
    if (sh < 0 || !box4_host || !window4_out_host || width < 1 || height < 1 || (ncomp != 1 && ncomp != 3)) return AEJ_ERR_ARG;
    if (ncomp == 3 && ((hs != 1 && hs != 2) || (vs != 1 && vs != 2))) return AEJ_ERR_ARG;
    const int ow = (width + scale - 1) >> sh, oh = (height + scale - 1) >> sh;
    if (!(0 <= box4_host[0] && box4_host[0] < box4_host[2] && box4_host[2] <= ow && 0 <= box4_host[1] && box4_host[1] < box4_host[3] && box4_host[3] <= oh))
        return AEJ_ERR_ARG;
    jd_sbox_window(width, height, hs, vs, ncomp, false, sh, box4_host, window4_out_host);
    return 0;
}

extern "C" int aej_jpegdec_sbox_window_host(const aej_jpegdec_desc *desc_host, int scale, const int32_t *box4_host, int32_t *window4_out_host)
{
    if (!desc_host) return AEJ_ERR_ARG;
    return sbox_window_host(desc_host->width, desc_host->height, desc_host->hs, desc_host->vs, desc_host->ncomp, scale, box4_host, window4_out_host);
}

extern "C" int aej_jpegprog_sbox_window_host(const aej_jpegprog_frame *frame_host, int scale, const int32_t *box4_host, int32_t *window4_out_host)
{
    if (!frame_host) return AEJ_ERR_ARG;
    return sbox_window_host(frame_host->width, frame_host->height, frame_host->hs, frame_host->vs, frame_host->ncomp, scale, box4_host, window4_out_host);
}

extern "C" int aej_jpegdec_box_window_host(const aej_jpegdec_desc *desc_host, const int32_t *box4_host, int32_t *window4_out_host)
{
    if (!desc_host) return AEJ_ERR_ARG;
    return sbox_window_host(desc_host->width, desc_host->height, desc_host->hs, desc_host->vs, desc_host->ncomp, 1, box4_host, window4_out_host);
}

extern "C" int aej_jpegprog_box_window_host(const aej_jpegprog_frame *frame_host, const int32_t *box4_host, int32_t *window4_out_host)
{
    if (!frame_host) return AEJ_ERR_ARG;
    return sbox_window_host(frame_host->width, frame_host->height, frame_host->hs, frame_host->vs, frame_host->ncomp, 1, box4_host, window4_out_host);
}

extern "C" int aej_jpegdec_box_stats(aej_ctx *ctx, int64_t *out3_host)
{
    if (!ctx || !out3_host) return AEJ_ERR_ARG;
    for (int v = 0; v < 3; v++) out3_host[v] = ctx->jd_box_stats[v];
    return 0;
}

static uint64_t jpegdec_workspace(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const JdOptions &o)
{
    JdResolved r;
    if (!ctx || !jpegdec_descs_ok(descs_host, n, o.adobe) || jd_resolve(descs_host, n, o, r).kind) return 0;
    std::vector<JdFile> files;
    JdBufSizes z;
    jpegdec_layout(descs_host, n, ctx->jd_subseq_bits, files, z, r);
    JdBufs w;
    return jpegdec_carve(nullptr, n, z, w);
}

extern "C" uint64_t aej_jpegdec_workspace_bytes(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n)
{
    return jpegdec_workspace(ctx, descs_host, n, {});
}

extern "C" uint64_t aej_jpegdec_workspace_bytes_scaled(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host)
{
    return scales_host ? jpegdec_workspace(ctx, descs_host, n, { scales_host }) : 0;
}

extern "C" uint64_t aej_jpegdec_workspace_bytes_mode(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host,
                                                     const int *components_host)
{
    return jpegdec_workspace(ctx, descs_host, n, { scales_host, components_host });
}

extern "C" uint64_t aej_jpegdec_workspace_bytes_box(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host,
                                                    const int *components_host, const int32_t *boxes_host)
{
    return jpegdec_workspace(ctx, descs_host, n, { scales_host, components_host, boxes_host });
}

extern "C" uint64_t aej_jpegdec_workspace_bytes_sbox(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host,
                                                     const int *components_host, const int32_t *boxes_host)
{
    return jpegdec_workspace(ctx, descs_host, n, { scales_host, components_host, boxes_host, nullptr, true });
}

extern "C" uint64_t aej_jpegdec_workspace_bytes_adobe(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host,
                                                      const int *components_host, const int32_t *boxes_host, const aej_jpeg_adobe *adobe_host)
{
    return jpegdec_workspace(ctx, descs_host, n, { scales_host, components_host, boxes_host, adobe_host });
}

// the entropy decode of n baseline files up to the fixed point of the sync rounds: everything of aej_jpegdec_batch before the
// coefficient write (`files` carries the scan offsets; the caller has carved `w`)
static int jpegdec_decode(aej_ctx *ctx, const char *fn, const aej_jpegdec_desc *descs_host, int n, const std::vector<JdFile> &files, const JdBufSizes &z,
                          const JdBufs &w, const uint8_t *scans, int32_t *status, const aej_jpeg_adobe *adobe_host)
{
    const int S = ctx->jd_subseq_bits;
    // one upload: files, descriptors, the "last round that changed" word (-1)
    std::vector<unsigned char> blob(sizeof(JdFile) * n + sizeof(aej_jpegdec_desc) * n + sizeof(int));
    memcpy(blob.data(), files.data(), sizeof(JdFile) * n);
    memcpy(blob.data() + sizeof(JdFile) * n, descs_host, sizeof(aej_jpegdec_desc) * n);
    const int minus1 = -1;
    memcpy(blob.data() + blob.size() - sizeof(int), &minus1, sizeof(int));
    long long max_slots = 0;
    for (const JdFile &f : files) max_slots = std::max(max_slots, f.n_slots);
    AEJ_TRY(bind_device(ctx));
    if (z.grpa > 0) {                                 // a call with a four-component or RGB-coded file: the kernels of such a call read these
        AEJ_HIP_CHECK(hipMemcpyAsync(w.adobe, adobe_host, sizeof(aej_jpeg_adobe) * n, hipMemcpyHostToDevice, ctx->stream));
    } else if (w.adobe) {                             // the kFour slot kernels for a uniform three-component file alone: no file has a component 3
        AEJ_HIP_CHECK(hipMemsetAsync(w.adobe, 0, sizeof(aej_jpeg_adobe) * n, ctx->stream));      // (jd_comp4), so nothing reads these; zeros all the same
    }
    AEJ_HIP_CHECK(launch_jpegdec_begin(ctx->stream, n, z, w, blob.data(), blob.size(), scans, S, status));
    // sync rounds: kJdSyncBatch launches, then one word read back; more only while the last launched round still changed something.
    // Each round settles at least the first unsettled subsequence of every segment, so max_slots rounds always suffice.
    int launched = 0, last = -1;
    for (;;) {
        AEJ_HIP_CHECK(launch_jpegdec_sync(ctx->stream, n, z, w, S, launched + 1, kJdSyncBatch));
        launched += kJdSyncBatch;
        AEJ_HIP_CHECK(hipMemcpyAsync(ctx->h_flag, w.last_change, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));     // also keeps `blob` alive until its upload has run
        last = ctx->h_flag[0];
        if (last < launched) break;
        if (launched > max_slots + kJdSyncBatch)
            return fail(ctx, AEJ_ERR_STATE, "%s: the Huffman decode did not settle after %d rounds", fn, launched);
    }
    ctx->jd_sync_rounds = last + 1;
    return 0;
}

// every aej_jpegdec_batch* entry: descriptors, then null buffers, then the options, then offsets, then the workspace
static int jpegdec_batch(aej_ctx *ctx, const char *fn, const aej_jpegdec_desc *descs_host, int n, const JdOptions &o, const uint8_t *scans,
                         uint64_t scans_bytes, const int64_t *scan_offsets_host, uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host,
                         int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    AEJ_TRY(enter(ctx, fn));
    if (!jpegdec_descs_ok(descs_host, n, o.adobe))
        return fail(ctx, AEJ_ERR_ARG, "%s: no files, or a descriptor aej_jpegdec_parse_host did not write", fn);
    if (!scans || !scan_offsets_host || !out || !out_offsets_host || !status || !workspace) return null_buffer(ctx, fn);
    JdResolved r;
    AEJ_TRY(jd_refuse(ctx, fn, jd_resolve(descs_host, n, o, r)));
    const int S = ctx->jd_subseq_bits;
    std::vector<JdFile> files;
    JdBufSizes z;
    jpegdec_layout(descs_host, n, S, files, z, r);
    if (jpeg_any_box(z)) {                                   // aej_jpegdec_box_stats: from the descriptors and the windows alone
        long long total = 0, decoded = 0;
        for (int i = 0; i < n; i++) {
            const aej_jpegdec_desc &d = descs_host[i];
            total += d.n_segments;
            if (!(files[i].shift & kJdBox)) { decoded += d.n_segments; continue; }
            const long long mcus = (long long)d.mcux * d.mcuy, ri = d.restart_interval ? d.restart_interval : mcus;
            const long long lo = (long long)files[i].win[1] * d.mcux, hi = (long long)files[i].win[3] * d.mcux;      // the window's MCUs: segment g holds [g * ri, g * ri + ri)
            decoded += std::min<long long>((hi + ri - 1) / ri, d.n_segments) - lo / ri;
        }
        ctx->jd_box_stats[0] = total; ctx->jd_box_stats[1] = decoded; ctx->jd_box_stats[2] = z.blocks;
    }
    for (int i = 0; i < n; i++) {                            // file by file, scan before image, as the errors were always reported
        const aej_jpegdec_desc &d = descs_host[i];
        AEJ_TRY(jpegdec_scan_offset(ctx, fn, d, i, scans_bytes, scan_offsets_host[i], files[i]));
        AEJ_TRY(image_offset(ctx, fn, i, out_bytes, out_offsets_host[i], files[i]));
    }
    JdBufs w;
    const unsigned long long need = jpegdec_carve(workspace, n, z, w);
    AEJ_TRY(check_workspace(ctx, need, workspace_bytes));
    AEJ_TRY(jpegdec_decode(ctx, fn, descs_host, n, files, z, w, scans, status, o.adobe));
    AEJ_HIP_CHECK(launch_jpegdec_finish(ctx->stream, n, z, w, S, out, status));
    return 0;
}

extern "C" int aej_jpegdec_batch(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const uint8_t *scans, uint64_t scans_bytes,
                                 const int64_t *scan_offsets_host, uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host,
                                 int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    return jpegdec_batch(ctx, __func__, descs_host, n, {}, scans, scans_bytes, scan_offsets_host, out, out_bytes, out_offsets_host, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegdec_batch_scaled(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const uint8_t *scans,
                                        uint64_t scans_bytes, const int64_t *scan_offsets_host, uint8_t *out, uint64_t out_bytes,
                                        const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    if (!scales_host) return ctx ? null_buffer(ctx, __func__) : AEJ_ERR_ARG;
    return jpegdec_batch(ctx, __func__, descs_host, n, { scales_host }, scans, scans_bytes, scan_offsets_host, out, out_bytes, out_offsets_host, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegdec_batch_mode(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const int *components_host,
                                      const uint8_t *scans, uint64_t scans_bytes, const int64_t *scan_offsets_host, uint8_t *out, uint64_t out_bytes,
                                      const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    return jpegdec_batch(ctx, __func__, descs_host, n, { scales_host, components_host }, scans, scans_bytes, scan_offsets_host, out, out_bytes, out_offsets_host, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegdec_batch_box(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const int *components_host,
                                     const int32_t *boxes_host, const uint8_t *scans, uint64_t scans_bytes, const int64_t *scan_offsets_host,
                                     uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host, int32_t *status, void *workspace,
                                     uint64_t workspace_bytes)
{
    return jpegdec_batch(ctx, __func__, descs_host, n, { scales_host, components_host, boxes_host },
                         scans, scans_bytes, scan_offsets_host, out, out_bytes, out_offsets_host, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegdec_batch_sbox(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const int *components_host,
                                      const int32_t *boxes_host, const uint8_t *scans, uint64_t scans_bytes, const int64_t *scan_offsets_host,
                                      uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host, int32_t *status, void *workspace,
                                      uint64_t workspace_bytes)
{
    return jpegdec_batch(ctx, __func__, descs_host, n, { scales_host, components_host, boxes_host, nullptr, true },
                         scans, scans_bytes, scan_offsets_host, out, out_bytes, out_offsets_host, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegdec_batch_adobe(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const int *components_host,
                                       const int32_t *boxes_host, const aej_jpeg_adobe *adobe_host, const uint8_t *scans, uint64_t scans_bytes,
                                       const int64_t *scan_offsets_host, uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host,
                                       int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    return jpegdec_batch(ctx, __func__, descs_host, n, { scales_host, components_host, boxes_host, adobe_host },
                         scans, scans_bytes, scan_offsets_host, out, out_bytes, out_offsets_host, status, workspace, workspace_bytes);
}

// the host twins of the per-pixel colour rules of k_jd_adobe (jpegdec_core.h), for the tests: n pixels of four samples -> n pixels of
// `components` (3 or 4) channels under `colour` (AEJ_JPEG_RGB, _CMYK, _YCCK)
extern "C" int aej_test_jpeg_adobe_pixels_host(const uint8_t *samples4_host, int64_t n, int colour, int components, uint8_t *out_host)
{
    if (!samples4_host || !out_host || n < 0 || colour < AEJ_JPEG_RGB || colour > AEJ_JPEG_YCCK || (components != 3 && components != 4)) return AEJ_ERR_ARG;
    if (components == 4 && colour == AEJ_JPEG_RGB) return AEJ_ERR_ARG;
    for (int64_t i = 0; i < n; i++) {
        const int s[4] = { samples4_host[4 * i], samples4_host[4 * i + 1], samples4_host[4 * i + 2], samples4_host[4 * i + 3] };
        jd_adobe_pixel(colour, components == 4, s, out_host + i * components);
    }
    return 0;
}

// the host twin of the chroma up-sampling rule (jd_up_chroma, jpegdec_core.h), for the tests: the rule's samples for the output pixels
// [y0, y1) x [x0, x1), row after row
extern "C" int aej_test_jpeg_upsample_host(const uint8_t *part_host, int64_t stride, int64_t off, int uh, int uv, int fancy, int wc, int hc,
                                           int x0, int y0, int x1, int y1, uint8_t *out_host)
{
    if (!part_host || !out_host || (uh != 1 && uh != 2) || (uv != 1 && uv != 2) || (uh == 2 && uv == 2 && !fancy)) return AEJ_ERR_ARG;
    if (wc < 1 || hc < 1 || x0 < 0 || x0 > x1 || x1 > uh * wc || y0 < 0 || y0 > y1 || y1 > uv * hc) return AEJ_ERR_ARG;
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) *out_host++ = (uint8_t)jd_up_chroma(part_host, stride, off, uh, uv, fancy != 0, wc, hc, y, x);
    return 0;
}

extern "C" int aej_test_jpegdec_idct_host(const int16_t *coef_host, const uint16_t *qt_host, int size, uint8_t *out_host)
{
    if (!coef_host || !qt_host || !out_host || (size != 1 && size != 2 && size != 4)) return AEJ_ERR_ARG;
    jd_idct_sized(coef_host, qt_host, size, out_host, size);
    return 0;
}

extern "C" int aej_test_jpegdec_coefs_host(const aej_jpegdec_desc *desc_host, const uint8_t *file_host, uint64_t nbytes, int16_t *coef_out_host,
                                           uint64_t coef_blocks)
{
    if (!desc_host || !file_host || !coef_out_host) return AEJ_ERR_ARG;
    return jpegdec_coefs_host(*desc_host, file_host, nbytes, coef_out_host, coef_blocks);
}

extern "C" int64_t aej_jpegdec_sync_rounds(aej_ctx *ctx)
{
    if (!ctx) return AEJ_ERR_ARG;
    return ctx->jd_sync_rounds;
}

// ---- progressive JPEG files decoded on the device (jpegprog.hip) ----------------------------------------------------------------------
static int jp_parse_host(const uint8_t *data_host, uint64_t nbytes, aej_jpegprog_frame *frame_host, aej_jpegprog_scan *scans_host, int scan_capacity,
                         char *msg, int msg_capacity, int layout_440, aej_jpeg_adobe *adobe_host)
{
    if (!frame_host || (layout_440 != 0 && layout_440 != 1)) return AEJ_ERR_ARG;
    std::string m;
    std::vector<aej_jpegprog_scan> scans;
    int rc = jpegprog_parse(data_host, nbytes, *frame_host, scans, m, layout_440 != 0, adobe_host);
    if (rc == 0 && scans_host) {
        if (scan_capacity < (int)scans.size()) { rc = AEJ_ERR_CAPACITY; m = "scan capacity below the file's " + std::to_string(scans.size()) + " scans"; }
        else memcpy(scans_host, scans.data(), sizeof(aej_jpegprog_scan) * scans.size());
    }
    copy_msg(m, msg, msg_capacity);
    return rc;
}

extern "C" int aej_jpegprog_parse_host(const uint8_t *data_host, uint64_t nbytes, aej_jpegprog_frame *frame_host, aej_jpegprog_scan *scans_host,
                                       int scan_capacity, char *msg, int msg_capacity)
{
    return jp_parse_host(data_host, nbytes, frame_host, scans_host, scan_capacity, msg, msg_capacity, 0, nullptr);
}

extern "C" int aej_jpegprog_parse_host_440(const uint8_t *data_host, uint64_t nbytes, aej_jpegprog_frame *frame_host, aej_jpegprog_scan *scans_host,
                                           int scan_capacity, char *msg, int msg_capacity, int layout_440)
{
    return jp_parse_host(data_host, nbytes, frame_host, scans_host, scan_capacity, msg, msg_capacity, layout_440, nullptr);
}

extern "C" int aej_jpegprog_parse_host_adobe(const uint8_t *data_host, uint64_t nbytes, aej_jpegprog_frame *frame_host, aej_jpegprog_scan *scans_host,
                                             int scan_capacity, aej_jpeg_adobe *adobe_host, char *msg, int msg_capacity, int layout_440)
{
    if (!adobe_host) return AEJ_ERR_ARG;
    return jp_parse_host(data_host, nbytes, frame_host, scans_host, scan_capacity, msg, msg_capacity, layout_440, adobe_host);
}

static uint64_t jpegprog_workspace(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n, const JdOptions &o)
{
    JpLayout y;
    JdResolved r;
    if (!ctx || jd_resolve(frames_host, n, o, r).kind || !jpegprog_layout(frames_host, scans_host, n, y, r)) return 0;
    JpBufs w;
    return jpegprog_carve(nullptr, y, w);
}

extern "C" uint64_t aej_jpegprog_workspace_bytes(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n)
{
    return jpegprog_workspace(ctx, frames_host, scans_host, n, {});
}

extern "C" uint64_t aej_jpegprog_workspace_bytes_scaled(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                        const int *scales_host)
{
    return scales_host ? jpegprog_workspace(ctx, frames_host, scans_host, n, { scales_host }) : 0;
}

extern "C" uint64_t aej_jpegprog_workspace_bytes_mode(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                      const int *scales_host, const int *components_host)
{
    return jpegprog_workspace(ctx, frames_host, scans_host, n, { scales_host, components_host });
}

extern "C" uint64_t aej_jpegprog_workspace_bytes_box(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                     const int *scales_host, const int *components_host, const int32_t *boxes_host)
{
    return jpegprog_workspace(ctx, frames_host, scans_host, n, { scales_host, components_host, boxes_host });
}

extern "C" uint64_t aej_jpegprog_workspace_bytes_sbox(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                      const int *scales_host, const int *components_host, const int32_t *boxes_host)
{
    return jpegprog_workspace(ctx, frames_host, scans_host, n, { scales_host, components_host, boxes_host, nullptr, true });
}

extern "C" uint64_t aej_jpegprog_workspace_bytes_adobe(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                       const int *scales_host, const int *components_host, const int32_t *boxes_host,
                                                       const aej_jpeg_adobe *adobe_host)
{
    return jpegprog_workspace(ctx, frames_host, scans_host, n, { scales_host, components_host, boxes_host, adobe_host });
}

// levels [0, n_levels) of the entropy stage, then either the reconstruction into `out` or (tests) a copy of the coefficients.  The
// options first, then the descriptors (jpegprog_layout), then null buffers, then offsets, then the workspace
static int jpegprog_run(aej_ctx *ctx, const char *fn, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                        const JdOptions &o, const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host, int n_levels, uint8_t *out,
                        uint64_t out_bytes, const int64_t *out_offsets_host, int16_t *coef_out, uint64_t coef_blocks, int32_t *status, void *workspace,
                        uint64_t workspace_bytes)
{
    if (!ctx) return AEJ_ERR_ARG;
    AEJ_TRY(refuse_in_flight(ctx, fn));
    JpLayout y;
    JdResolved r;
    AEJ_TRY(jd_refuse(ctx, fn, jd_resolve(frames_host, n, o, r)));
    if (!jpegprog_layout(frames_host, scans_host, n, y, r))
        return fail(ctx, AEJ_ERR_ARG, "%s: no files, or descriptors aej_jpegprog_parse_host did not write", fn);
    if (!data || !data_offsets_host || !status || !workspace || (!out && !coef_out) || (out && !out_offsets_host))
        return null_buffer(ctx, fn);
    AEJ_TRY(jpegprog_scan_offsets(ctx, fn, y, data_bytes, data_offsets_host));
    for (int i = 0; out && i < n; i++)
        AEJ_TRY(image_offset(ctx, fn, i, out_bytes, out_offsets_host[i], y.ffiles[i]));
    if (coef_out && (uint64_t)y.fz.blocks > coef_blocks) return fail(ctx, AEJ_ERR_CAPACITY, "%s: %lld coefficient blocks, room for %llu", fn, y.fz.blocks, (unsigned long long)coef_blocks);
    JpBufs w;
    const unsigned long long need = jpegprog_carve(workspace, y, w);
    AEJ_TRY(check_workspace(ctx, need, workspace_bytes));
    std::vector<unsigned char> blob;
    jpegprog_blob(y, &blob);
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_jpegprog_entropy(ctx->stream, y, w, blob.data(), blob.size(), data, n_levels, status));
    if (out) AEJ_HIP_CHECK(launch_jpegprog_recon(ctx->stream, y, w, out));
    if (coef_out) AEJ_HIP_CHECK(hipMemcpyAsync(coef_out, w.f.coef, (size_t)y.fz.blocks * 128, hipMemcpyDeviceToDevice, ctx->stream));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // keeps `blob` alive until its upload has run
    return 0;
}

extern "C" int aej_jpegprog_batch(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                  const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host, uint8_t *out, uint64_t out_bytes,
                                  const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    if (!out) return ctx ? null_buffer(ctx, __func__) : AEJ_ERR_ARG;
    return jpegprog_run(ctx, __func__, frames_host, scans_host, n, {}, data, data_bytes, data_offsets_host, 1 << 30, out, out_bytes,
                        out_offsets_host, nullptr, 0, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegprog_batch_scaled(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                         const int *scales_host, const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host,
                                         uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host, int32_t *status, void *workspace,
                                         uint64_t workspace_bytes)
{
    if (!out || !scales_host) return ctx ? null_buffer(ctx, __func__) : AEJ_ERR_ARG;
    return jpegprog_run(ctx, __func__, frames_host, scans_host, n, { scales_host }, data, data_bytes, data_offsets_host, 1 << 30, out, out_bytes,
                        out_offsets_host, nullptr, 0, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegprog_batch_mode(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                       const int *scales_host, const int *components_host, const uint8_t *data, uint64_t data_bytes,
                                       const int64_t *data_offsets_host, uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host,
                                       int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    if (!out) return ctx ? null_buffer(ctx, __func__) : AEJ_ERR_ARG;
    return jpegprog_run(ctx, __func__, frames_host, scans_host, n, { scales_host, components_host }, data, data_bytes, data_offsets_host, 1 << 30, out, out_bytes,
                        out_offsets_host, nullptr, 0, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegprog_batch_box(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                      const int *scales_host, const int *components_host, const int32_t *boxes_host, const uint8_t *data,
                                      uint64_t data_bytes, const int64_t *data_offsets_host, uint8_t *out, uint64_t out_bytes,
                                      const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    if (!out) return ctx ? null_buffer(ctx, __func__) : AEJ_ERR_ARG;
    return jpegprog_run(ctx, __func__, frames_host, scans_host, n, { scales_host, components_host, boxes_host }, data, data_bytes, data_offsets_host, 1 << 30, out, out_bytes,
                        out_offsets_host, nullptr, 0, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegprog_batch_sbox(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                       const int *scales_host, const int *components_host, const int32_t *boxes_host, const uint8_t *data,
                                       uint64_t data_bytes, const int64_t *data_offsets_host, uint8_t *out, uint64_t out_bytes,
                                       const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    if (!out) return ctx ? null_buffer(ctx, __func__) : AEJ_ERR_ARG;
    return jpegprog_run(ctx, __func__, frames_host, scans_host, n, { scales_host, components_host, boxes_host, nullptr, true }, data, data_bytes, data_offsets_host, 1 << 30, out, out_bytes,
                        out_offsets_host, nullptr, 0, status, workspace, workspace_bytes);
}

extern "C" int aej_jpegprog_batch_adobe(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                        const int *scales_host, const int *components_host, const int32_t *boxes_host,
                                        const aej_jpeg_adobe *adobe_host, const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host,
                                        uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host, int32_t *status, void *workspace,
                                        uint64_t workspace_bytes)
{
    if (!out) return ctx ? null_buffer(ctx, __func__) : AEJ_ERR_ARG;
    return jpegprog_run(ctx, __func__, frames_host, scans_host, n, { scales_host, components_host, boxes_host, adobe_host }, data, data_bytes, data_offsets_host, 1 << 30, out, out_bytes,
                        out_offsets_host, nullptr, 0, status, workspace, workspace_bytes);
}

extern "C" int aej_test_jpegprog_coefs(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                       const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host, int n_levels,
                                       int16_t *coef_out, uint64_t coef_blocks, int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    if (!coef_out) return ctx ? null_buffer(ctx, __func__) : AEJ_ERR_ARG;
    return jpegprog_run(ctx, __func__, frames_host, scans_host, n, {}, data, data_bytes, data_offsets_host, n_levels, nullptr, 0, nullptr, coef_out,
                        coef_blocks, status, workspace, workspace_bytes);
}

extern "C" int aej_test_jpegprog_coefs_host(const aej_jpegprog_frame *frame_host, const aej_jpegprog_scan *scans_host, const uint8_t *file_host,
                                            uint64_t nbytes, int n_levels, int16_t *coef_out_host, uint64_t coef_blocks)
{
    if (!frame_host || !scans_host || !file_host || !coef_out_host) return AEJ_ERR_ARG;
    return jpegprog_coefs_host(*frame_host, scans_host, file_host, nbytes, n_levels, coef_out_host, coef_blocks);
}

// ---- lossless transcode and transform (jfiftrans.hip): the decoders' entropy stages, the bridge, the encoders' entropy stages ----------------
// One routine each serves aej_jfif_transcode_* and aej_jfif_transform_*: the transcoder is the transform "none" of every file (xf NULL).
template <class D>
static bool jt_source_ok(const D &d)
{
    if ((d.ncomp != 3 && d.ncomp != 1) || d.precision16) return false;
    for (int c = 0; c < d.ncomp; c++)
        for (int i = 0; i < 64; i++)
            if (d.qt[c][i] < 1 || d.qt[c][i] > 255) return false;
    return true;
}

// the call's layout: baseline files first, then progressive ones.  -> 0, or the error (ctx is never NULL: the entries check it first)
struct JtCall {
    std::vector<JdFile> files; JdBufSizes z{};      // baseline decode
    JpLayout y;                                     // progressive decode
    JtPlan plan;
    std::vector<JtSource> src;
};
static bool rst_ok(int blocks, int rows) { return blocks >= 0 && blocks <= kJrMaxInterval && rows >= 0 && rows <= kJrMaxInterval; }

// The options of a transcode / transform call, as the entries state them ({}: the plain transcode).  xf: one transform code per file
// (NULL: kJxNone for every file; need_xf: the entry refuses that).  boxes: NULL, or jx_geom's crop box of every file (right == 0: none).
// The one-file host routines take the same set: xf and boxes point at that file's code and box.
struct JtOptions { const int32_t *xf; int trim, rst_blocks, rst_rows, allow440; const int32_t *boxes; int drop; bool need_xf; };

static int jt_layout(aej_ctx *ctx, const char *fn, const aej_jpegdec_desc *descs, int n_base, const aej_jpegprog_frame *frames,
                     const aej_jpegprog_scan *pscans, int n_prog, const uint16_t *density, int progressive, const JtOptions &o, JtCall &c)
{
    if (o.allow440 != 0 && o.allow440 != 1) return fail(ctx, AEJ_ERR_ARG, "%s: layout_440 %d (0 or 1)", fn, o.allow440);
    if (o.drop != 0 && o.drop != 1) return fail(ctx, AEJ_ERR_ARG, "%s: drop_chroma %d (0 or 1)", fn, o.drop);
    if (o.trim != 0 && o.trim != 1) return fail(ctx, AEJ_ERR_ARG, "%s: trim %d (0 or 1)", fn, o.trim);
    if (!rst_ok(o.rst_blocks, o.rst_rows)) return fail(ctx, AEJ_ERR_ARG, "%s: restart_blocks %d, restart_rows %d (0 .. 65535)", fn, o.rst_blocks, o.rst_rows);
    if (n_base < 0 || n_prog < 0 || n_base + n_prog < 1 || (long long)n_base + n_prog > 65535 || (progressive != 0 && progressive != 1))
        return fail(ctx, AEJ_ERR_ARG, "%s: 1 .. 65535 files and progressive 0 or 1 required", fn);
    if (n_base && !jpegdec_descs_ok(descs, n_base)) return fail(ctx, AEJ_ERR_ARG, "%s: a descriptor aej_jpegdec_parse_host did not write", fn);
    if (n_prog && !jpegprog_layout(frames, pscans, n_prog, c.y, {})) return fail(ctx, AEJ_ERR_ARG, "%s: descriptors aej_jpegprog_parse_host did not write", fn);
    const int n = n_base + n_prog;
    c.src.assign(n, JtSource{});
    std::vector<long long> nblk(n);
    if (n_base) jpegdec_layout(descs, n_base, ctx->jd_subseq_bits, c.files, c.z, {});
    c.z.planes = c.z.px = 0;                                 // no reconstruction: no sample planes
    c.y.fz.planes = c.y.fz.px = 0;
    for (int i = 0; i < n; i++) {
        const bool ok = i < n_base ? jt_source_ok(descs[i]) : jt_source_ok(frames[i - n_base]);
        if (!ok) return fail(ctx, AEJ_ERR_UNSUPPORTED, "%s: file %d: three components or one, with 8-bit quantisation tables, required", fn, i);
        if (i < n_base) jfiftrans_source(descs[i], c.src[i]); else jfiftrans_source(frames[i - n_base], c.src[i]);
        if (!o.allow440 && c.src[i].ncomp == 3 && c.src[i].hs == 1 && c.src[i].vs == 2)
            return fail(ctx, AEJ_ERR_UNSUPPORTED, "%s: file %d: a 4:4:0 file, which the entries with layout_440 take", fn, i);
        nblk[i] = i < n_base ? c.files[i].n_blocks : c.y.ffiles[i - n_base].n_blocks;
        if (density) { c.src[i].units = density[3 * i] & 255; c.src[i].xdensity = density[3 * i + 1]; c.src[i].ydensity = density[3 * i + 2]; }
    }
    int why = kJxOk;
    const int bad = jfiftrans_plan(c.src, nblk, progressive != 0, o.xf, o.trim, c.plan, &why, o.rst_blocks, o.rst_rows, o.allow440 != 0, o.boxes, o.drop != 0);
    if (bad < 0) return 0;
    if (why == kJxCropRange)
        return fail(ctx, AEJ_ERR_ARG, "%s: file %d: crop box (%d, %d, %d, %d) does not lie inside the transformed image", fn, bad, o.boxes[4 * bad],
                    o.boxes[4 * bad + 1], o.boxes[4 * bad + 2], o.boxes[4 * bad + 3]);
    if (why == kJxLayout)
        return fail(ctx, AEJ_ERR_UNSUPPORTED, "%s: file %d: a transposing transform of a 4:2:2 file would be a 4:4:0 file, which is not built", fn, bad);      // (the entries with layout_440 write it)
    if (why == kJxNotPerfect)
        return fail(ctx, AEJ_ERR_ARG, "%s: file %d: transform %d mirrors an axis that is not a whole number of MCUs (trim = 1 drops the partial ones)", fn,
                    bad, o.xf ? o.xf[bad] : 0);
    if (why == kJxTrimsToZero) return fail(ctx, AEJ_ERR_ARG, "%s: file %d: nothing is left of the mirrored axis after the trim", fn, bad);
    return fail(ctx, AEJ_ERR_ARG, "%s: file %d: a transform code outside 0 .. 7, or descriptors whose sampling or block counts do not fit", fn, bad);
}

struct JtWorkspace { JdBufs wb; JpBufs wp; unsigned long long bytes; };
static JtWorkspace jt_carve(void *workspace, int n_base, int n_prog, JtCall &c)
{
    JtWorkspace r{};
    char *base = static_cast<char *>(workspace);
    unsigned long long off = 0;
    if (n_base) off += jpegdec_carve(base ? base + off : nullptr, n_base, c.z, r.wb);
    if (n_prog) off += jpegprog_carve(base ? base + off : nullptr, c.y, r.wp);
    off += jfiftrans_carve(base ? base + off : nullptr, c.plan);
    r.bytes = off;
    return r;
}

static int jt_headers(const aej_jpegdec_desc *desc_host, const aej_jpegprog_frame *frame_host, const uint16_t *density3_host, int progressive,
                      const JtOptions &o, uint8_t *out_host, int capacity)
{
    if ((o.allow440 != 0 && o.allow440 != 1) || (o.drop != 0 && o.drop != 1)) return AEJ_ERR_ARG;
    if ((!desc_host) == (!frame_host) || !out_host || capacity < 0 || (progressive != 0 && progressive != 1) || (o.trim != 0 && o.trim != 1)) return AEJ_ERR_ARG;
    if (!(desc_host ? jt_source_ok(*desc_host) : jt_source_ok(*frame_host))) return AEJ_ERR_UNSUPPORTED;
    JtSource s;
    if (desc_host) jfiftrans_source(*desc_host, s); else jfiftrans_source(*frame_host, s);
    if (density3_host) { s.units = density3_host[0] & 255; s.xdensity = density3_host[1]; s.ydensity = density3_host[2]; }
    JxGeom x;
    if (!o.allow440 && s.ncomp == 3 && s.hs == 1 && s.vs == 2) return AEJ_ERR_UNSUPPORTED;
    const int rc = jx_geom(s.height, s.width, s.hs, s.vs, o.xf ? *o.xf : kJxNone, o.trim, x, s.ncomp, o.allow440 != 0, o.boxes, o.drop != 0);
    if (rc != kJxOk) return rc == kJxLayout ? AEJ_ERR_UNSUPPORTED : AEJ_ERR_ARG;
    const int n = jfiftrans_prefix_host(jfiftrans_transformed(s, x), progressive != 0, out_host, capacity);
    return n < 0 ? AEJ_ERR_CAPACITY : n;
}

extern "C" int aej_jfif_transcode_headers_host(const aej_jpegdec_desc *desc_host, const aej_jpegprog_frame *frame_host, const uint16_t *density3_host,
                                               int progressive, uint8_t *out_host, int capacity)
{
    return jt_headers(desc_host, frame_host, density3_host, progressive, {}, out_host, capacity);
}

extern "C" int aej_jfif_transform_headers_host(const aej_jpegdec_desc *desc_host, const aej_jpegprog_frame *frame_host, const uint16_t *density3_host,
                                               int progressive, int transform, int trim, uint8_t *out_host, int capacity)
{
    return jt_headers(desc_host, frame_host, density3_host, progressive, { &transform, trim }, out_host, capacity);
}

extern "C" int aej_jfif_transform_headers_host_440(const aej_jpegdec_desc *desc_host, const aej_jpegprog_frame *frame_host, const uint16_t *density3_host,
                                                   int progressive, int transform, int trim, int layout_440, uint8_t *out_host, int capacity)
{
    return jt_headers(desc_host, frame_host, density3_host, progressive, { &transform, trim, 0, 0, layout_440 }, out_host, capacity);
}

extern "C" int aej_jfif_transform_headers_host_cut(const aej_jpegdec_desc *desc_host, const aej_jpegprog_frame *frame_host, const uint16_t *density3_host,
                                                   int progressive, int transform, int trim, int layout_440, const int32_t *box4_host, int drop_chroma,
                                                   uint8_t *out_host, int capacity)
{
    return jt_headers(desc_host, frame_host, density3_host, progressive, { &transform, trim, 0, 0, layout_440, box4_host, drop_chroma }, out_host, capacity);
}

// out4_host (may be NULL): the output's height, width and sampling factors; corner2 (may be NULL): the crop's corner in output pixels
static int jt_geometry_host(int H, int W, int hs, int vs, int nc, const JtOptions &o, int32_t *out4_host, int32_t *corner2)
{
    JxGeom x;
    const int trim = o.trim;
    if ((o.allow440 != 0 && o.allow440 != 1) || (o.drop != 0 && o.drop != 1)) return AEJ_ERR_ARG;
    const int rc = jx_geom(H, W, hs, vs, *o.xf, trim != 0, x, nc, o.allow440 != 0, o.boxes, o.drop != 0);
    if ((trim != 0 && trim != 1) || rc == kJxBadArg) return AEJ_ERR_ARG;
    if (rc == kJxLayout) return AEJ_ERR_UNSUPPORTED;
    if (rc == kJxCropRange) return AEJ_JFIF_TRANSFORM_CROP_RANGE;
    if (rc != kJxOk) return rc == kJxNotPerfect ? AEJ_JFIF_TRANSFORM_NOT_PERFECT : AEJ_JFIF_TRANSFORM_TRIMS_TO_ZERO;
    if (out4_host) { out4_host[0] = x.oH; out4_host[1] = x.oW; out4_host[2] = x.ohs; out4_host[3] = x.ovs; }
    if (corner2) { corner2[0] = x.cx * 8 * x.ohs; corner2[1] = x.cy * 8 * x.ovs; }
    return 0;
}

extern "C" int aej_jfif_transform_geometry_host_cut(int H, int W, int hs, int vs, int components, int transform, int trim, int layout_440,
                                                    const int32_t *box4_host, int drop_chroma, int32_t *out6_host)
{
    int32_t o[6] = { 0, 0, 0, 0, 0, 0 };
    const int rc = jt_geometry_host(H, W, hs, vs, components, { &transform, trim, 0, 0, layout_440, box4_host, drop_chroma }, o, o + 4);
    if (rc == 0 && out6_host) memcpy(out6_host, o, sizeof o);
    return rc;
}

extern "C" int aej_jfif_transform_geometry_host(int H, int W, int hs, int vs, int transform, int trim, int32_t *out4_host)
{
    return jt_geometry_host(H, W, hs, vs, 3, { &transform, trim }, out4_host, nullptr);
}

extern "C" int aej_jfif_transform_geometry_host_440(int H, int W, int hs, int vs, int transform, int trim, int layout_440, int32_t *out4_host)
{
    return jt_geometry_host(H, W, hs, vs, 3, { &transform, trim, 0, 0, layout_440 }, out4_host, nullptr);
}

static int64_t jt_coefs_host(int H, int W, int hs, int vs, int nc, const JtOptions &o, const int16_t *src_host, int64_t src_blocks, int16_t *dst_host,
                             int64_t dst_blocks)
{
    JxGeom x;
    const int rc = jt_geometry_host(H, W, hs, vs, nc, o, nullptr, nullptr);
    if (rc) return rc;
    jx_geom(H, W, hs, vs, *o.xf, o.trim, x, nc, o.allow440 != 0, o.boxes, o.drop != 0);
    if (!src_host && !dst_host) return x.n_out;              // a size query
    if (!src_host || !dst_host || src_blocks != x.n_src) return AEJ_ERR_ARG;
    if (dst_blocks < x.n_out) return AEJ_ERR_CAPACITY;
    jfiftrans_coefs_host(x, src_host, dst_host);
    return x.n_out;
}

extern "C" int64_t aej_jfif_transform_coefs_host(int H, int W, int hs, int vs, int transform, int trim, const int16_t *src_host, int64_t src_blocks,
                                                 int16_t *dst_host, int64_t dst_blocks)
{
    return jt_coefs_host(H, W, hs, vs, 3, { &transform, trim }, src_host, src_blocks, dst_host, dst_blocks);
}

extern "C" int64_t aej_jfif_transform_coefs_host_440(int H, int W, int hs, int vs, int transform, int trim, int layout_440, const int16_t *src_host,
                                                     int64_t src_blocks, int16_t *dst_host, int64_t dst_blocks)
{
    return jt_coefs_host(H, W, hs, vs, 3, { &transform, trim, 0, 0, layout_440 }, src_host, src_blocks, dst_host, dst_blocks);
}

extern "C" int64_t aej_jfif_transform_coefs_host_cut(int H, int W, int hs, int vs, int components, int transform, int trim, int layout_440,
                                                     const int32_t *box4_host, int drop_chroma, const int16_t *src_host, int64_t src_blocks,
                                                     int16_t *dst_host, int64_t dst_blocks)
{
    const JtOptions o{ &transform, trim, 0, 0, layout_440, box4_host, drop_chroma };
    const int64_t rc = jt_coefs_host(H, W, hs, vs, components, o, src_host, src_blocks, dst_host, dst_blocks);
    const bool refused = jt_geometry_host(H, W, hs, vs, components, o, nullptr, nullptr) > 0;
    return refused ? AEJ_ERR_ARG : rc;                        // a cropped file can have 1, 2 or 3 blocks: no positive refusal codes here
}

extern "C" int64_t aej_jfif_transform_coefs_grey_host(int H, int W, int transform, int trim, const int16_t *src_host, int64_t src_blocks,
                                                      int16_t *dst_host, int64_t dst_blocks)
{
    const int64_t rc = jt_coefs_host(H, W, 1, 1, 1, { &transform, trim }, src_host, src_blocks, dst_host, dst_blocks);
    const bool refused = aej_jfif_transform_geometry_host(H, W, 1, 1, transform, trim, nullptr) > 0;
    return refused ? AEJ_ERR_ARG : rc;                        // a one-component file can have 1 or 2 blocks: no positive refusal codes here
}

static uint64_t jt_workspace_bytes(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const aej_jpegprog_frame *frames_host,
                                   const aej_jpegprog_scan *pscans_host, int n_prog, int progressive, const JtOptions &o)
{
    if (!ctx || (o.need_xf && !o.xf) || (n_base > 0 && !descs_host) || (n_prog > 0 && (!frames_host || !pscans_host))) return 0;
    JtCall c;
    const std::string keep = ctx->err;
    const int rc = jt_layout(ctx, "", descs_host, n_base, frames_host, pscans_host, n_prog, nullptr, progressive, o, c);
    ctx->err = keep;                                         // a size query leaves the context's last error alone
    return rc ? 0 : jt_carve(nullptr, n_base, n_prog, c).bytes;
}

extern "C" uint64_t aej_jfif_transcode_workspace_bytes_rst(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                           const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                           int progressive, int restart_blocks, int restart_rows)
{
    return jt_workspace_bytes(ctx, descs_host, n_base, frames_host, pscans_host, n_prog, progressive, { nullptr, 0, restart_blocks, restart_rows });
}

extern "C" uint64_t aej_jfif_transcode_workspace_bytes(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                       const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                       int progressive)
{
    return jt_workspace_bytes(ctx, descs_host, n_base, frames_host, pscans_host, n_prog, progressive, {});
}

extern "C" uint64_t aej_jfif_transform_workspace_bytes_rst(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                           const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                           int progressive, const int32_t *transforms_host, int trim, int restart_blocks,
                                                           int restart_rows)
{
    return jt_workspace_bytes(ctx, descs_host, n_base, frames_host, pscans_host, n_prog, progressive, { transforms_host, trim, restart_blocks, restart_rows, 0, nullptr, 0, true });
}

extern "C" uint64_t aej_jfif_transform_workspace_bytes_440(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                           const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                           int progressive, const int32_t *transforms_host, int trim, int restart_blocks,
                                                           int restart_rows, int layout_440)
{
    return jt_workspace_bytes(ctx, descs_host, n_base, frames_host, pscans_host, n_prog, progressive, { transforms_host, trim, restart_blocks, restart_rows, layout_440 });
}

extern "C" uint64_t aej_jfif_transform_workspace_bytes_cut(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                           const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                           int progressive, const int32_t *transforms_host, int trim, int restart_blocks,
                                                           int restart_rows, int layout_440, const int32_t *boxes4_host, int drop_chroma)
{
    return jt_workspace_bytes(ctx, descs_host, n_base, frames_host, pscans_host, n_prog, progressive, { transforms_host, trim, restart_blocks, restart_rows, layout_440, boxes4_host, drop_chroma });
}

extern "C" uint64_t aej_jfif_transform_workspace_bytes(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                       const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                       int progressive, const int32_t *transforms_host, int trim)
{
    return jt_workspace_bytes(ctx, descs_host, n_base, frames_host, pscans_host, n_prog, progressive, { transforms_host, trim, 0, 0, 0, nullptr, 0, true });
}

static int jt_batch(aej_ctx *ctx, const char *fn, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                    const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                    const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host, const uint16_t *density_host, int progressive,
                    const JtOptions &o, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host, int32_t *status,
                    int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes)
{
    AEJ_TRY(enter(ctx, fn));
    if (o.need_xf && !o.xf) return null_buffer(ctx, fn);
    if ((n_base > 0 && (!descs_host || !scans || !scan_offsets_host)) || (n_prog > 0 && (!frames_host || !pscans_host || !data || !data_offsets_host)) ||
        !offsets || !lengths || !total_host || !status || !workspace)
        return null_buffer(ctx, fn);
    JtCall c;
    AEJ_TRY(jt_layout(ctx, fn, descs_host, n_base, frames_host, pscans_host, n_prog, density_host, progressive, o, c));
    for (int i = 0; i < n_base; i++) AEJ_TRY(jpegdec_scan_offset(ctx, fn, descs_host[i], i, scans_bytes, scan_offsets_host[i], c.files[i]));
    AEJ_TRY(jpegprog_scan_offsets(ctx, fn, c.y, data_bytes, data_offsets_host));
    const JtWorkspace ws = jt_carve(workspace, n_base, n_prog, c);
    AEJ_TRY(check_workspace(ctx, ws.bytes, workspace_bytes));
    const int n = n_base + n_prog;
    for (int i = 0; i < n; i++) {
        JtFile &F = c.plan.files[i];
        F.src = i < n_base ? ws.wb.coef + c.files[i].blk_base * 64 : ws.wp.f.coef + c.y.ffiles[i - n_base].blk_base * 64;
        F.status_index = i;
    }
    if (n_groups_host) *n_groups_host = (int32_t)c.plan.groups.size();
    std::vector<unsigned char> blob;
    if (n_base) {
        AEJ_TRY(jpegdec_decode(ctx, fn, descs_host, n_base, c.files, c.z, ws.wb, scans, status, nullptr));
        AEJ_HIP_CHECK(launch_jpegdec_write(ctx->stream, n_base, c.z, ws.wb, ctx->jd_subseq_bits, status));
    } else {
        AEJ_TRY(bind_device(ctx));
    }
    if (n_prog) {
        jpegprog_blob(c.y, &blob);
        AEJ_HIP_CHECK(launch_jpegprog_entropy(ctx->stream, c.y, ws.wp, blob.data(), blob.size(), data, 1 << 30, status + n_base));
    }
    AEJ_HIP_CHECK(launch_jfiftrans(ctx->stream, c.plan, status, out, out_capacity, (long long *)lengths, (long long *)offsets));
    long long total = 0;
    AEJ_HIP_CHECK(hipMemcpyAsync(&total, c.plan.total, 8, hipMemcpyDeviceToHost, ctx->stream));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // also keeps `blob` and the plan's tables alive until their uploads have run
    *total_host = (uint64_t)total;
    if (out && (uint64_t)total > out_capacity)
        return fail(ctx, AEJ_ERR_CAPACITY, "%s: the files need %lld bytes, the output holds %llu", fn, total, (unsigned long long)out_capacity);
    return 0;
}

extern "C" int aej_jfif_transcode_batch_rst(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                            const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                            const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                            const int64_t *data_offsets_host, const uint16_t *density_host, int progressive, int restart_blocks,
                                            int restart_rows, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths,
                                            uint64_t *total_host, int32_t *status, int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes)
{
    return jt_batch(ctx, __func__, descs_host, n_base, scans, scans_bytes, scan_offsets_host, frames_host, pscans_host, n_prog, data, data_bytes,
                    data_offsets_host, density_host, progressive, { nullptr, 0, restart_blocks, restart_rows }, out, out_capacity, offsets, lengths, total_host, status, n_groups_host,
                    workspace, workspace_bytes);
}

extern "C" int aej_jfif_transcode_batch(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                        const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                        const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                        const int64_t *data_offsets_host, const uint16_t *density_host, int progressive, uint8_t *out,
                                        uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host, int32_t *status,
                                        int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes)
{
    return jt_batch(ctx, __func__, descs_host, n_base, scans, scans_bytes, scan_offsets_host, frames_host, pscans_host, n_prog, data, data_bytes,
                    data_offsets_host, density_host, progressive, {}, out, out_capacity, offsets, lengths, total_host, status, n_groups_host,
                    workspace, workspace_bytes);
}

extern "C" int aej_jfif_transform_batch_rst(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                            const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                            const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                            const int64_t *data_offsets_host, const uint16_t *density_host, int progressive,
                                            const int32_t *transforms_host, int trim, int restart_blocks, int restart_rows, uint8_t *out,
                                            uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host, int32_t *status,
                                            int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes)
{
    return jt_batch(ctx, __func__, descs_host, n_base, scans, scans_bytes, scan_offsets_host, frames_host, pscans_host, n_prog, data, data_bytes,
                    data_offsets_host, density_host, progressive, { transforms_host, trim, restart_blocks, restart_rows, 0, nullptr, 0, true }, out, out_capacity, offsets, lengths, total_host, status, n_groups_host,
                    workspace, workspace_bytes);
}

extern "C" int aej_jfif_transform_batch_440(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                            const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                            const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                            const int64_t *data_offsets_host, const uint16_t *density_host, int progressive,
                                            const int32_t *transforms_host, int trim, int restart_blocks, int restart_rows, int layout_440,
                                            uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host,
                                            int32_t *status, int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes)
{
    return jt_batch(ctx, __func__, descs_host, n_base, scans, scans_bytes, scan_offsets_host, frames_host, pscans_host, n_prog, data, data_bytes,
                    data_offsets_host, density_host, progressive, { transforms_host, trim, restart_blocks, restart_rows, layout_440 }, out, out_capacity, offsets, lengths, total_host, status, n_groups_host,
                    workspace, workspace_bytes);
}

extern "C" int aej_jfif_transform_batch_cut(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                            const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                            const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                            const int64_t *data_offsets_host, const uint16_t *density_host, int progressive,
                                            const int32_t *transforms_host, int trim, int restart_blocks, int restart_rows, int layout_440,
                                            const int32_t *boxes4_host, int drop_chroma, uint8_t *out, uint64_t out_capacity, int64_t *offsets,
                                            int64_t *lengths, uint64_t *total_host, int32_t *status, int32_t *n_groups_host, void *workspace,
                                            uint64_t workspace_bytes)
{
    return jt_batch(ctx, __func__, descs_host, n_base, scans, scans_bytes, scan_offsets_host, frames_host, pscans_host, n_prog, data, data_bytes,
                    data_offsets_host, density_host, progressive, { transforms_host, trim, restart_blocks, restart_rows, layout_440, boxes4_host, drop_chroma }, out, out_capacity, offsets, lengths, total_host, status, n_groups_host,
                    workspace, workspace_bytes);
}

extern "C" int aej_jfif_transform_batch(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                        const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                        const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                        const int64_t *data_offsets_host, const uint16_t *density_host, int progressive,
                                        const int32_t *transforms_host, int trim, uint8_t *out, uint64_t out_capacity, int64_t *offsets,
                                        int64_t *lengths, uint64_t *total_host, int32_t *status, int32_t *n_groups_host, void *workspace,
                                        uint64_t workspace_bytes)
{
    return jt_batch(ctx, __func__, descs_host, n_base, scans, scans_bytes, scan_offsets_host, frames_host, pscans_host, n_prog, data, data_bytes,
                    data_offsets_host, density_host, progressive, { transforms_host, trim, 0, 0, 0, nullptr, 0, true }, out, out_capacity, offsets, lengths, total_host, status, n_groups_host,
                    workspace, workspace_bytes);
}

// ---- images of mixed sizes and qualities in one call (jfifmany.hip): the ragged front end, then the transcoder's chains --------------------
static bool jm_flags_ok(int optimize, int progressive) { return (optimize == 0 || optimize == 1) && (progressive == 0 || progressive == 1); }

extern "C" uint64_t aej_jfif_many_workspace_bytes_rst(aej_ctx *, const aej_jfif_many_desc *descs_host, int n, int subsampling, int optimize,
                                                      int progressive, int restart_blocks, int restart_rows)
{
    JmPlan plan;
    if (!jm_flags_ok(optimize, progressive) || !rst_ok(restart_blocks, restart_rows) ||
        jfifmany_plan(descs_host, n, -1, subsampling, optimize != 0, progressive != 0, plan, nullptr, restart_blocks, restart_rows) >= 0)
        return 0;
    return jfifmany_carve(nullptr, plan);
}

extern "C" uint64_t aej_jfif_many_workspace_bytes(aej_ctx *ctx, const aej_jfif_many_desc *descs_host, int n, int subsampling, int optimize,
                                                  int progressive)
{
    return aej_jfif_many_workspace_bytes_rst(ctx, descs_host, n, subsampling, optimize, progressive, 0, 0);
}

static int jm_encode(aej_ctx *ctx, const char *fn, const aej_jfif_many_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, int subsampling,
                     int optimize, int progressive, int rst_blocks, int rst_rows, uint8_t *out, uint64_t out_capacity, int64_t *offsets,
                     int64_t *lengths, uint64_t *total_host, int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes)
{
    AEJ_TRY(enter(ctx, fn));
    if (!jm_flags_ok(optimize, progressive)) return fail(ctx, AEJ_ERR_ARG, "%s: optimize %d, progressive %d (0 or 1)", fn, optimize, progressive);
    if (!rst_ok(rst_blocks, rst_rows)) return fail(ctx, AEJ_ERR_ARG, "%s: restart_blocks %d, restart_rows %d (0 .. 65535)", fn, rst_blocks, rst_rows);
    if (!descs_host || !src || !offsets || !lengths || !total_host || !workspace) return null_buffer(ctx, fn);
    JmPlan plan;
    const char *why = "";
    const long long limit = (long long)std::min<uint64_t>(src_bytes, (uint64_t)INT64_MAX);
    const int bad = jfifmany_plan(descs_host, n, limit, subsampling, optimize != 0, progressive != 0, plan, &why, rst_blocks, rst_rows);
    if (bad >= 0) return fail(ctx, AEJ_ERR_ARG, "%s: image %d: %s", fn, bad, why);
    AEJ_TRY(check_workspace(ctx, jfifmany_carve(workspace, plan), workspace_bytes));
    if (n_groups_host) *n_groups_host = (int32_t)plan.t.groups.size();
    AEJ_TRY(bind_device(ctx));
    AEJ_HIP_CHECK(launch_jfifmany(ctx->stream, plan, src, out, out_capacity, (long long *)lengths, (long long *)offsets));
    long long total = 0;
    AEJ_HIP_CHECK(hipMemcpyAsync(&total, plan.t.total, 8, hipMemcpyDeviceToHost, ctx->stream));
    AEJ_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // also keeps the plan's tables alive until their uploads have run
    *total_host = (uint64_t)total;
    if (out && (uint64_t)total > out_capacity)
        return fail(ctx, AEJ_ERR_CAPACITY, "%s: the files need %lld bytes, the output holds %llu", fn, total, (unsigned long long)out_capacity);
    return 0;
}

extern "C" int aej_jfif_many_encode_rst(aej_ctx *ctx, const aej_jfif_many_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes,
                                        int subsampling, int optimize, int progressive, int restart_blocks, int restart_rows, uint8_t *out,
                                        uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host, int32_t *n_groups_host,
                                        void *workspace, uint64_t workspace_bytes)
{
    return jm_encode(ctx, __func__, descs_host, n, src, src_bytes, subsampling, optimize, progressive, restart_blocks, restart_rows, out, out_capacity,
                     offsets, lengths, total_host, n_groups_host, workspace, workspace_bytes);
}

extern "C" int aej_jfif_many_encode(aej_ctx *ctx, const aej_jfif_many_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, int subsampling,
                                    int optimize, int progressive, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths,
                                    uint64_t *total_host, int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes)
{
    return jm_encode(ctx, __func__, descs_host, n, src, src_bytes, subsampling, optimize, progressive, 0, 0, out, out_capacity, offsets, lengths,
                     total_host, n_groups_host, workspace, workspace_bytes);
}

// ---- restart markers: the Annex K markers with the DRI, and the index rules on the host (jfif_restart_core.h) -------------------------------
extern "C" int aej_jfif_headers_rst_host(int quality, int H, int W, int subsampling, int components, int restart_blocks, int restart_rows,
                                         uint8_t *out_host, int capacity)
{
    JfifGeom g;
    const int nc = components == 1 ? 1 : 3;
    if ((components != 0 && components != 1 && components != 3) || quality < 1 || quality > 100 || !out_host) return AEJ_ERR_ARG;
    if (!jfif_geom(1, H, W, 1, g, subsampling, 1, nc) || !jfif_geom_restart(g, restart_blocks, restart_rows)) return AEJ_ERR_ARG;
    JfifParams p;
    jfif_params_host(quality, H, W, p, subsampling, nc, g.R);
    if (capacity < p.hdr_len) return AEJ_ERR_CAPACITY;
    memcpy(out_host, p.hdr, p.hdr_len);
    return p.hdr_len;
}

extern "C" int aej_jfif_restart_map_host(int H, int W, int subsampling, int components, int restart_blocks, int restart_rows, int progressive,
                                         int32_t *scan_r_host, int32_t *scan_dri_host, int32_t *interval_host, uint8_t *reset_host,
                                         int64_t block_capacity, uint8_t *marker_host, int64_t marker_capacity, int64_t *counts2_host)
{
    JfifGeom g;
    JfpGeom p;
    const int nc = components == 1 ? 1 : 3;
    if ((components != 0 && components != 1 && components != 3) || (progressive != 0 && progressive != 1) || !scan_r_host || !scan_dri_host)
        return AEJ_ERR_ARG;
    if (!jfif_geom(1, H, W, 1, g, subsampling, 1, nc) || !jfif_geom_restart(g, restart_blocks, restart_rows)) return AEJ_ERR_ARG;
    int nscan = 1;
    scan_r_host[0] = g.R;
    scan_dri_host[0] = g.R != 0;
    if (progressive) {
        if (!jfifprog_geom(g, p, restart_blocks, restart_rows)) return AEJ_ERR_ARG;
        nscan = p.nscan;
        for (int i = 0; i < nscan; i++) { scan_r_host[i] = p.sc[i].R; scan_dri_host[i] = p.sc[i].dri; }
    }
    // the first scan (the baseline file's only one): every block's interval and whether its DC predictor is reset; every interval's marker
    const int R = scan_r_host[0], NL = g.hs * g.vs, BPM = NL + nc - 1;
    const long long niv = R ? jr_count(g.n_mcu, R) : 1;
    if (counts2_host) { counts2_host[0] = g.nblk; counts2_host[1] = niv; }
    if (interval_host || reset_host) {
        if (block_capacity < g.nblk) return AEJ_ERR_CAPACITY;
        for (long long b = 0; b < g.nblk; b++) {
            const long long m = b / BPM, pb = js_prev(NL, BPM, m, (int)(b % BPM));
            if (interval_host) interval_host[b] = R ? (int32_t)jr_interval_of(m, R) : 0;
            if (reset_host) reset_host[b] = pb < 0 || jr_resets(m, pb, BPM, R);
        }
    }
    if (marker_host) {
        if (marker_capacity < niv) return AEJ_ERR_CAPACITY;
        marker_host[0] = 0;                                  // no marker before the first interval
        for (long long k = 1; k < niv; k++) marker_host[k] = (uint8_t)jr_marker(k);
    }
    return nscan;
}

static int64_t jm_coefs_host(int width, int height, int quality, int subsampling, int nc, const uint8_t *src_host, int16_t *dst_host, int64_t dst_blocks)
{
    const long long nb = jfifmany_coefs_host(width, height, quality, subsampling, nullptr, nullptr, nc);
    if (nb < 0 || (!src_host) != (!dst_host)) return AEJ_ERR_ARG;
    if (!src_host) return nb;                                // a size query
    if (dst_blocks < nb) return AEJ_ERR_CAPACITY;
    return jfifmany_coefs_host(width, height, quality, subsampling, src_host, dst_host, nc);
}

extern "C" int64_t aej_jfif_many_coefs_host(int width, int height, int quality, int subsampling, const uint8_t *rgb_host, int16_t *dst_host,
                                            int64_t dst_blocks)
{
    return jm_coefs_host(width, height, quality, subsampling, 3, rgb_host, dst_host, dst_blocks);
}

extern "C" int64_t aej_jfif_many_coefs_grey_host(int width, int height, int quality, const uint8_t *grey_host, int16_t *dst_host, int64_t dst_blocks)
{
    return jm_coefs_host(width, height, quality, 0, 1, grey_host, dst_host, dst_blocks);
}
