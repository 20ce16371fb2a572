// api_png.hip -- the PNG entries of the C ABI (include/aej.h): the host chunk walk (aej_png_parse_host, aej_png_parse_host_accept) and the
// launch of the scanline un-filter, layout conversion and Adam7 interleave of csrc/png.hip (aej_png_unfilter_batch), and of its scanline
// filter (aej_png_filter_batch).  Host code only.
#include "aej_ctx.h"

using namespace aej;

namespace {

constexpr int kPngMaxSide = 1 << 24;     // keeps every in-row index of the kernel inside an int (row bytes <= 2^27: 16-bit RGBA)

uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// CRC-32 of ISO 3309 as the PNG specification's annex D computes it, over a chunk's type and data
uint32_t png_crc(const uint8_t *p, size_t n)
{
    static uint32_t table[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
    });
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

int refuse(int code, const std::string &m, char *msg, int cap)
{
    copy_msg(m, msg, cap);
    return code;
}

// samples per pixel of a colour type, 0 for a value that is none
int png_channels(int ct) { return ct == 0 || ct == 3 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : ct == 6 ? 4 : 0; }

bool png_desc_ok(const aej_png_desc &d)
{
    const int ch = png_channels(d.colour_type);
    if (!ch || d.channels != ch || (d.interlace != 0 && d.interlace != 1)) return false;
    if (d.width < 1 || d.height < 1 || d.width > kPngMaxSide || d.height > kPngMaxSide) return false;
    const bool packed = d.bit_depth == 1 || d.bit_depth == 2 || d.bit_depth == 4;
    if (!(d.bit_depth == 8 || (d.bit_depth == 16 && d.colour_type != 3) || (packed && (d.colour_type == 0 || d.colour_type == 3)))) return false;
    if (d.row_bytes != (int)(((long long)d.width * ch * d.bit_depth + 7) / 8)) return false;
    return d.palette_len >= 0 && d.palette_len <= 256 && (d.colour_type != 3 || d.palette_len > 0);
}

int png_bpp(const aej_png_desc &d) { return d.bit_depth == 16 ? 2 * d.channels : d.bit_depth == 8 ? d.channels : 1; }

// bytes per pixel of the image written.  16-bit files under AEJ_PNG_AUTO: Pillow's "I;16" (the two bytes of a uint16), "RGB", and "RGBA"
// for grey + alpha as for RGBA
int png_out_channels(const aej_png_desc &d, int layout)
{
    if (layout == AEJ_PNG_RGB || d.colour_type == 3) return 3;
    if (d.bit_depth == 16) return d.colour_type == 0 ? 2 : d.colour_type == 2 ? 3 : 4;
    return d.channels;
}

int png_row_bytes(const aej_png_desc &d, int width) { return (int)(((long long)width * d.channels * d.bit_depth + 7) / 8); }

// the inflated size the file must have: every non-empty pass of an interlaced file is an image of its own, filter bytes included
unsigned long long png_raw_bytes(const aej_png_desc &d)
{
    if (!d.interlace) return (unsigned long long)d.height * (1ull + (unsigned long long)d.row_bytes);      // < 2^51
    unsigned long long total = 0;
    for (int p = 0; p < 7; p++) {
        const Adam7Pass a = adam7_pass(d.width, d.height, p);
        if (a.w > 0) total += (unsigned long long)a.h * (1ull + (unsigned long long)png_row_bytes(d, a.w));
    }
    return total;
}

// The workspace of aej_png_unfilter_batch: eight status words for every interlaced file (one per pass) at its start, rounded up to 256
// bytes; the carried scanline of every work item; the pass images of every interlaced file (each rounded up to 4 bytes, a file's to 256).
// Calls without interlaced files have the carried scanlines alone, as they always had.
unsigned long long png_status_bytes(int interlaced) { return ((unsigned long long)interlaced * 32 + 255) & ~255ull; }

unsigned long long png_item_bytes(const aej_png_desc &d)      // carried scanlines of the file's work items
{
    if (!d.interlace) return (unsigned long long)png_carry_bytes(d.row_bytes, png_bpp(d));
    unsigned long long total = 0;
    for (int p = 0; p < 7; p++) {
        const Adam7Pass a = adam7_pass(d.width, d.height, p);
        if (a.w > 0) total += (unsigned long long)png_carry_bytes(png_row_bytes(d, a.w), png_bpp(d));
    }
    return total;
}

unsigned long long png_pass_image_bytes(const aej_png_desc &d, int oc)
{
    unsigned long long total = 0;
    for (int p = 0; p < 7; p++) {
        const Adam7Pass a = adam7_pass(d.width, d.height, p);
        total += ((unsigned long long)a.w * a.h * oc + 3) & ~3ull;
    }
    return (total + 255) & ~255ull;
}

}  // namespace

extern "C" int aej_png_parse_host(const uint8_t *data_host, uint64_t nbytes, aej_png_desc *desc_host, int64_t *spans_host, int span_capacity,
                                  char *msg, int msg_capacity)
{
    return aej_png_parse_host_accept(data_host, nbytes, 0, desc_host, spans_host, span_capacity, msg, msg_capacity);
}

extern "C" uint64_t aej_png_raw_bytes(const aej_png_desc *desc_host) { return desc_host && png_desc_ok(*desc_host) ? png_raw_bytes(*desc_host) : 0; }

extern "C" int aej_png_adam7_passes_host(int width, int height, int32_t *passes_host)
{
    if (!passes_host || width < 1 || height < 1) return AEJ_ERR_ARG;
    for (int p = 0; p < 7; p++) {
        const Adam7Pass a = adam7_pass(width, height, p);
        const int32_t row[6] = { a.x0, a.y0, 1 << a.sx, 1 << a.sy, a.w, a.h };
        memcpy(passes_host + 6 * p, row, sizeof row);
    }
    return 0;
}

extern "C" int aej_png_parse_host_accept(const uint8_t *data_host, uint64_t nbytes, uint32_t accept, aej_png_desc *desc_host, int64_t *spans_host,
                                         int span_capacity, char *msg, int msg_capacity)
{
    if (accept & ~(uint32_t)(AEJ_PNG_ACCEPT_ADAM7 | AEJ_PNG_ACCEPT_16BIT)) return refuse(AEJ_ERR_ARG, "unknown accept flags", msg, msg_capacity);
    if (!data_host || !desc_host || span_capacity < 0) return refuse(AEJ_ERR_ARG, "NULL buffer", msg, msg_capacity);
    aej_png_desc &d = *desc_host;
    memset(&d, 0, sizeof d);
    static const uint8_t kSig[8] = { 0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a };
    if (nbytes < 8 || memcmp(data_host, kSig, 8) != 0) return refuse(AEJ_ERR_ARG, "not a PNG file: bad signature", msg, msg_capacity);
    uint64_t pos = 8;
    bool have_ihdr = false, have_plte = false, ended = false;
    while (!ended && pos < nbytes) {
        if (nbytes - pos < 12) return refuse(AEJ_ERR_ARG, "truncated file: a chunk header runs past the end", msg, msg_capacity);
        const uint64_t len = be32(data_host + pos);
        const uint8_t *type = data_host + pos + 4;
        const std::string name(reinterpret_cast<const char *>(type), 4);
        if (len > nbytes - pos - 12) return refuse(AEJ_ERR_ARG, "truncated file: the length of chunk " + name + " runs past the end", msg, msg_capacity);
        const uint8_t *body = type + 4;
        auto named = [&](const char *t) { return memcmp(type, t, 4) == 0; };
        auto crc_ok = [&] { return png_crc(type, 4 + (size_t)len) == be32(body + len); };
        if (!have_ihdr) {
            if (!named("IHDR") || len != 13) return refuse(AEJ_ERR_ARG, "missing IHDR: the first chunk is " + name, msg, msg_capacity);
            if (!crc_ok()) return refuse(AEJ_ERR_ARG, "bad CRC on IHDR", msg, msg_capacity);
            have_ihdr = true;
            const uint32_t w = be32(body), h = be32(body + 4);
            d.bit_depth = body[8];
            d.colour_type = body[9];
            d.interlace = body[12];
            d.channels = png_channels(d.colour_type);
            if (w == 0 || h == 0) return refuse(AEJ_ERR_ARG, "zero width or height", msg, msg_capacity);
            if (w > 0x7fffffffu || h > 0x7fffffffu) return refuse(AEJ_ERR_ARG, "width or height above 2^31 - 1", msg, msg_capacity);
            d.width = (int32_t)w;
            d.height = (int32_t)h;
            const int bd = d.bit_depth;
            const bool depth_known = bd == 1 || bd == 2 || bd == 4 || bd == 8 || bd == 16;
            const bool depth_allowed = depth_known && (d.colour_type == 0 || (d.colour_type == 3 && bd != 16) || ((d.colour_type == 2 || d.colour_type == 4 || d.colour_type == 6) && bd >= 8));
            if (!d.channels || !depth_allowed)
                return refuse(AEJ_ERR_ARG, "colour type " + std::to_string(d.colour_type) + " with bit depth " + std::to_string(bd) + " is not a PNG image type", msg, msg_capacity);
            if (body[10] != 0 || body[11] != 0 || body[12] > 1) return refuse(AEJ_ERR_ARG, "unknown compression, filter or interlace method", msg, msg_capacity);
            const char *mode = d.colour_type == 0 ? (bd == 1 ? "1" : bd == 16 ? "I;16" : "L") : d.colour_type == 2 ? "RGB" : d.colour_type == 3 ? "P"
                             : d.colour_type == 4 ? (bd == 16 ? "RGBA" : "LA") : "RGBA";
            snprintf(d.mode, sizeof d.mode, "%s", mode);
            if (bd == 16 && !(accept & AEJ_PNG_ACCEPT_16BIT)) return refuse(AEJ_ERR_UNSUPPORTED, "16-bit samples are not built", msg, msg_capacity);
            if (d.interlace && !(accept & AEJ_PNG_ACCEPT_ADAM7)) return refuse(AEJ_ERR_UNSUPPORTED, "Adam7 interlace is not built", msg, msg_capacity);
            if (d.width > kPngMaxSide || d.height > kPngMaxSide) return refuse(AEJ_ERR_UNSUPPORTED, "a side above 2^24 pixels is not built", msg, msg_capacity);
            d.row_bytes = (int32_t)(((long long)d.width * d.channels * bd + 7) / 8);
        } else if (named("IHDR")) {
            return refuse(AEJ_ERR_ARG, "a second IHDR", msg, msg_capacity);
        } else if (named("PLTE")) {
            if (!crc_ok()) return refuse(AEJ_ERR_ARG, "bad CRC on PLTE", msg, msg_capacity);
            if (have_plte || len == 0 || len % 3 != 0 || len > 768) return refuse(AEJ_ERR_ARG, "a PLTE chunk that is repeated, empty, longer than 256 entries or no multiple of 3", msg, msg_capacity);
            have_plte = true;
            d.palette_len = (int32_t)(len / 3);
            memcpy(d.palette, body, (size_t)len);
        } else if (named("tRNS")) {
            if (!crc_ok()) return refuse(AEJ_ERR_ARG, "bad CRC on tRNS", msg, msg_capacity);
            d.has_trns = 1;
        } else if (named("IDAT")) {
            if (d.colour_type == 3 && !have_plte) return refuse(AEJ_ERR_ARG, "missing PLTE before the first IDAT", msg, msg_capacity);
            if (d.n_idat == INT32_MAX) return refuse(AEJ_ERR_ARG, "too many IDAT chunks", msg, msg_capacity);
            if (spans_host && d.n_idat < span_capacity) {
                spans_host[2 * (int64_t)d.n_idat] = (int64_t)(pos + 8);
                spans_host[2 * (int64_t)d.n_idat + 1] = (int64_t)len;
            }
            d.n_idat++;
            d.idat_bytes += (int64_t)len;
        } else if (named("IEND")) {
            ended = true;
        } else if (named("acTL") || named("fcTL") || named("fdAT")) {
            return refuse(AEJ_ERR_UNSUPPORTED, "APNG frames (chunk " + name + ") are not built", msg, msg_capacity);
        } else if (!(type[0] & 0x20)) {
            return refuse(AEJ_ERR_UNSUPPORTED, "unknown critical chunk " + name, msg, msg_capacity);
        }
        pos += 12 + len;
    }
    if (!have_ihdr) return refuse(AEJ_ERR_ARG, "missing IHDR", msg, msg_capacity);
    if (d.colour_type == 3 && !have_plte) return refuse(AEJ_ERR_ARG, "missing PLTE", msg, msg_capacity);
    if (d.n_idat == 0) return refuse(AEJ_ERR_ARG, "missing IDAT", msg, msg_capacity);
    if (spans_host && d.n_idat > span_capacity) return refuse(AEJ_ERR_CAPACITY, "more IDAT chunks than the span list holds", msg, msg_capacity);
    copy_msg("", msg, msg_capacity);
    return 0;
}

extern "C" uint64_t aej_png_workspace_bytes(aej_ctx *ctx, const aej_png_desc *descs_host, int n)
{
    if (!ctx || !descs_host || n < 1) return 0;
    unsigned long long total = 0;
    int interlaced = 0;
    for (int i = 0; i < n; i++) {
        const aej_png_desc &d = descs_host[i];
        if (!png_desc_ok(d)) return 0;
        total += png_item_bytes(d);
        if (d.interlace) {                               // (the layouts are not known here: the larger of the two images)
            interlaced++;
            total += png_pass_image_bytes(d, std::max(png_out_channels(d, AEJ_PNG_RGB), png_out_channels(d, AEJ_PNG_AUTO)));
        }
    }
    return total + png_status_bytes(interlaced);
}

extern "C" int aej_png_unfilter_batch(aej_ctx *ctx, const aej_png_desc *descs_host, int n, const uint8_t *inflated, uint64_t inflated_bytes,
                                      const int64_t *in_offsets_host, const int64_t *inflate_out_bytes, const int32_t *inflate_status,
                                      const uint8_t *palettes, const int32_t *layouts_host, uint8_t *out, uint64_t out_bytes,
                                      const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (n < 1 || !descs_host) return fail(ctx, AEJ_ERR_ARG, "%s: no files", fn);
    if (!inflated || !in_offsets_host || !out || !out_offsets_host || !status || !workspace) return null_buffer(ctx, fn);
    if ((inflate_out_bytes == nullptr) != (inflate_status == nullptr))
        return fail(ctx, AEJ_ERR_ARG, "%s: inflate_out_bytes and inflate_status go together", fn);
    if (reinterpret_cast<uintptr_t>(inflated) & 3 || reinterpret_cast<uintptr_t>(palettes) & 3 || reinterpret_cast<uintptr_t>(workspace) & 3)
        return fail(ctx, AEJ_ERR_ARG, "%s: inflated, palettes and workspace must be 4-byte aligned", fn);
    int interlaced = 0;
    unsigned long long carries = 0;
    for (int i = 0; i < n; i++) {
        if (!png_desc_ok(descs_host[i])) return fail(ctx, AEJ_ERR_ARG, "%s: file %d: a descriptor aej_png_parse_host did not write", fn, i);
        interlaced += descs_host[i].interlace;
        carries += png_item_bytes(descs_host[i]);
    }
    // workspace layout: png_status_bytes
    std::vector<PngFile> files(n);
    std::vector<PngAdam7File> woven;
    unsigned long long carry = png_status_bytes(interlaced), image = carry + carries;
    for (int i = 0; i < n; i++) {
        const aej_png_desc &d = descs_host[i];
        const int layout = layouts_host ? layouts_host[i] : AEJ_PNG_RGB;
        if (layout != AEJ_PNG_RGB && layout != AEJ_PNG_AUTO) return fail(ctx, AEJ_ERR_ARG, "%s: file %d: layout %d", fn, i, layout);
        if (d.colour_type == 3 && !palettes) return fail(ctx, AEJ_ERR_ARG, "%s: file %d: a palette file and no palettes", fn, i);
        PngFile &f = files[i];
        f.W = d.width;
        f.H = d.height;
        f.rb = d.row_bytes;
        f.bpp = (unsigned char)png_bpp(d);
        f.depth = (unsigned char)d.bit_depth;
        f.ct = (unsigned char)d.colour_type;
        f.oc = (unsigned char)png_out_channels(d, layout);
        const unsigned long long raw = png_raw_bytes(d);
        const unsigned long long pixels = (unsigned long long)d.height * (unsigned long long)d.width * f.oc;
        const long long io = in_offsets_host[i], oo = out_offsets_host[i];
        if (io < 0 || (io & 3) || (unsigned long long)io > inflated_bytes || ((raw + 3) & ~3ull) > inflated_bytes - (unsigned long long)io)
            return fail(ctx, AEJ_ERR_ARG, "%s: file %d: scanlines outside the inflated buffer (whole dwords), or an offset that is no multiple of 4", fn, i);
        if (oo < 0 || (unsigned long long)oo > out_bytes || pixels > out_bytes - (unsigned long long)oo)
            return fail(ctx, AEJ_ERR_ARG, "%s: file %d: image outside the output", fn, i);
        f.raw_bytes = (long long)raw;
        f.in_off = io;
        f.out_off = oo;
        f.carry_off = (long long)carry;
        f.item = -1;
        carry += png_item_bytes(d);
        if (!d.interlace) continue;
        PngAdam7File w{};                                // the passes' images in the workspace, then the interleave into `out`
        w.out_off = oo;
        w.img_off = (long long)image;
        w.W = d.width;
        w.H = d.height;
        w.oc = f.oc;
        w.file = i;
        w.item = 8 * (int)woven.size();
        f.out_off = w.img_off;
        f.item = w.item;
        image += png_pass_image_bytes(d, f.oc);
        woven.push_back(w);
    }
    AEJ_TRY(check_workspace(ctx, image, workspace_bytes));
    AEJ_TRY(bind_device(ctx));
    for (int first = 0; first < n; first += kPngGroup) {
        PngGroup grp{};
        const int count = std::min(kPngGroup, n - first);
        std::copy(files.begin() + first, files.begin() + first + count, grp.f);
        launch_png_unfilter(ctx->stream, grp, first, count, inflated, reinterpret_cast<const long long *>(inflate_out_bytes), inflate_status,
                            palettes, out, static_cast<unsigned char *>(workspace), status);
        AEJ_HIP_CHECK(hipGetLastError());
    }
    const int n_woven = (int)woven.size();
    for (int first = 0; first < n_woven; first += kPngGroup) {
        PngAdam7Group grp{};
        const int count = std::min(kPngGroup, n_woven - first);
        int max_height = 0;
        for (int k = 0; k < count; k++) {
            grp.f[k] = woven[first + k];
            max_height = std::max(max_height, grp.f[k].H);
        }
        launch_png_adam7_interleave(ctx->stream, grp, count, max_height, static_cast<const unsigned char *>(workspace), out, status);
        AEJ_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

namespace {
constexpr int kPngEncMaxRowBytes = 1 << 24;      // a row's cost sum (at most 128 per byte) stays inside an int
bool png_enc_shape_ok(long long height, long long row_bytes, long long bpp)
{
    return height >= 1 && height <= kPngMaxSide && bpp >= 1 && bpp <= 4 && row_bytes >= bpp && row_bytes <= kPngEncMaxRowBytes && row_bytes % bpp == 0;
}
}  // namespace

extern "C" uint64_t aej_png_filter_bytes(int height, int row_bytes, int bpp)
{
    return png_enc_shape_ok(height, row_bytes, bpp) ? (uint64_t)height * (1ull + (uint64_t)row_bytes) : 0;
}

extern "C" int aej_png_filter_batch(aej_ctx *ctx, const int64_t *descs_host, int n, int optimize, uint8_t *out, uint64_t out_bytes)
{
    const char *fn = __func__;
    AEJ_TRY(enter(ctx, fn));
    if (n < 1 || !descs_host) return fail(ctx, AEJ_ERR_ARG, "%s: no images", fn);
    if (!out) return null_buffer(ctx, fn);
    if (reinterpret_cast<uintptr_t>(out) & 3) return fail(ctx, AEJ_ERR_ARG, "%s: out must be 4-byte aligned", fn);
    for (int i = 0; i < n; i++) {
        const int64_t *d = descs_host + 5 * (int64_t)i;      // source pointer, height, row bytes, bytes per pixel, offset in out
        if (!d[0]) return fail(ctx, AEJ_ERR_ARG, "%s: image %d: NULL source", fn, i);
        if (!png_enc_shape_ok(d[1], d[2], d[3]))
            return fail(ctx, AEJ_ERR_ARG, "%s: image %d: height %lld, row bytes %lld, bytes per pixel %lld (1 .. 2^24 rows of 1 .. 2^24 bytes, whole pixels of 1 .. 4 bytes)",
                        fn, i, (long long)d[1], (long long)d[2], (long long)d[3]);
        const unsigned long long need = (unsigned long long)d[1] * (1ull + (unsigned long long)d[2]);
        if (d[4] < 0 || (unsigned long long)d[4] > out_bytes || need > out_bytes - (unsigned long long)d[4])
            return fail(ctx, AEJ_ERR_ARG, "%s: image %d: scanlines outside the output", fn, i);
    }
    AEJ_TRY(bind_device(ctx));
    for (int first = 0; first < n;) {
        PngEncGroup grp{};
        int count = 0;
        long long rows = 0;
        for (; count < kPngGroup && first + count < n; count++) {
            const int64_t *d = descs_host + 5 * (int64_t)(first + count);
            if (rows + d[1] > INT32_MAX) break;              // (count >= 1: a height is at most 2^24)
            PngEncImage &f = grp.f[count];
            f.src = reinterpret_cast<const unsigned char *>(static_cast<uintptr_t>(d[0]));
            f.H = (int)d[1];
            f.rb = (int)d[2];
            f.bpp = (int)d[3];
            f.dst_off = d[4];
            f.row0 = (int)rows;
            rows += d[1];
        }
        launch_png_filter(ctx->stream, grp, count, (int)rows, optimize ? 1 : 0, out);
        AEJ_HIP_CHECK(hipGetLastError());
        first += count;
    }
    return 0;
}
