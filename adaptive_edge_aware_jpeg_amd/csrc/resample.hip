// resample.hip -- Pillow's 8-bit resampling on the device (aej_resample_*): Image.reduce's integer cell mean and Image.resize's two
// fixed-point convolution passes (box, bilinear, hamming, bicubic, lanczos), bit for bit, over many packed [h][w][3] (RGB) and [h][w]
// (mode "L") images of different sizes in one call.  The filters are evaluated on the HOST only, in double (rs_taps below: the arithmetic of Pillow's
// coefficient precompute, compiled without FP contraction); the device holds int32 taps and an int32 accumulator.
//
// One call is at most three launches per channel count present (the kernels are templated on it: a call of RGB images alone is three, a
// mixed one six), each one grid over every image of that channel count that needs the stage (a per-image entry, a prefix sum of
// workgroups, a binary search by blockIdx.x, as jpegdec.hip's k_jd_scaled): k_rs_reduce -> k_rs_horizontal -> k_rs_vertical.  The
// last stage an image needs writes its destination, the ones before it write the workspace; an image that needs none is copied by
// the vertical pass under identity taps.  The horizontal pass only covers the source rows the vertical taps touch.
#include <math.h>
#include <string.h>

#include <vector>

#include "aej_ctx.h"

#pragma clang fp contract(off)

namespace aej {

// ---- host: filters and taps ---------------------------------------------------------------------------------------------------------------
static double rs_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

static double rs_filter(int f, double x)
{
    switch (f) {
    case AEJ_RESAMPLE_BOX: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case AEJ_RESAMPLE_BILINEAR:
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    case AEJ_RESAMPLE_HAMMING:
        if (x < 0.0) x = -x;
        if (x == 0.0) return 1.0;
        if (x >= 1.0) return 0.0;
        x = x * M_PI;
        return sin(x) / x * (0.54 + 0.46 * cos(x));
    case AEJ_RESAMPLE_BICUBIC: {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    default: return -3.0 <= x && x < 3.0 ? rs_sinc(x) * rs_sinc(x / 3) : 0.0;      // AEJ_RESAMPLE_LANCZOS
    }
}

double rs_support(int f)
{
    return f == AEJ_RESAMPLE_BOX ? 0.5 : f == AEJ_RESAMPLE_BILINEAR || f == AEJ_RESAMPLE_HAMMING ? 1.0 : f == AEJ_RESAMPLE_BICUBIC ? 2.0
         : f == AEJ_RESAMPLE_LANCZOS ? 3.0 : 0.0;      // 0: not a filter
}

// the box edges are float32 and their difference is taken in float32: Pillow's C entry takes the box as four floats
static double rs_scale(float in0, float in1, int out_size) { return (double)(in1 - in0) / out_size; }

int rs_ksize(float in0, float in1, int out_size, int f)
{
    const double scale = rs_scale(in0, in1, out_size), support = rs_support(f) * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

// the window of output index xx, the one place this arithmetic lives: -> its centre; *xmin the first source index, *cnt the tap count
static double rs_window(int in_size, float in0, double scale, double support, int xx, int *xmin, int *cnt)
{
    const double center = in0 + (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in_size) hi = in_size;
    *xmin = lo;
    *cnt = hi - lo < 0 ? 0 : hi - lo;
    return center;
}

void rs_bounds_of_row(int in_size, float in0, float in1, int out_size, int f, int xx, int *bounds)
{
    const double scale = rs_scale(in0, in1, out_size), support = rs_support(f) * (scale < 1.0 ? 1.0 : scale);
    rs_window(in_size, in0, scale, support, xx, &bounds[0], &bounds[1]);
}

// bounds [out_size][2]: first source index, tap count; taps [out_size][ksize], zero beyond the count
void rs_taps(int in_size, float in0, float in1, int out_size, int f, int ksize, int *bounds, int *taps)
{
    const double scale = rs_scale(in0, in1, out_size), filterscale = scale < 1.0 ? 1.0 : scale, support = rs_support(f) * filterscale;
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out_size; xx++) {
        int xmin, xmax;
        const double center = rs_window(in_size, in0, scale, support, xx, &xmin, &xmax);
        if (xmax > ksize) xmax = ksize;              // (never: ksize is Pillow's own bound on the count)
        double ww = 0.0;
        for (int x = 0; x < xmax; x++) {
            k[x] = rs_filter(f, (x + xmin - center + 0.5) / filterscale);
            ww += k[x];
        }
        int *t = taps + (long long)xx * ksize;
        for (int x = 0; x < ksize; x++) {
            if (x >= xmax) { t[x] = 0; continue; }
            const double v = ww != 0.0 ? k[x] / ww : k[x];
            t[x] = v < 0 ? (int)(-0.5 + v * (1 << kRsBits)) : (int)(0.5 + v * (1 << kRsBits));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned char rs_clip(int acc)
{
    return (unsigned char)min(max(acc >> kRsBits, 0), 255);      // an arithmetic shift, as Pillow's clip8
}

// Image.reduce: thread = one output pixel, the mean of its fx x fy cell clipped at the box's right and bottom edges.
// Bounds: x < out_w = ceil(bw / fx) and y < out_h = ceil(bh / fy), so the cell holds at least one pixel and stays inside the box.
template <int kC>
__global__ __launch_bounds__(kRsThreads) void k_rs_reduce(const RsReduce *__restrict__ entries, int n)
{
    const RsReduce &e = tile_entry(entries, n);
    const long long p = ((long long)blockIdx.x - e.tile_base) * kRsThreads + threadIdx.x;
    if (p >= (long long)e.out_w * e.out_h) return;
    const int y = (int)(p / e.out_w), x = (int)(p - (long long)y * e.out_w);
    const int x0 = x * e.fx, x1 = min(x0 + e.fx, e.bw), y0 = y * e.fy, y1 = min(y0 + e.fy, e.bh);
    unsigned s0 = 0, s1 = 0, s2 = 0;                  // (kC == 1: s1 and s2 stay out of it)
    for (int r = y0; r < y1; r++) {
        const unsigned char *s = e.in + ((long long)r * e.in_w + x0) * kC;
        for (int c = x0; c < x1; c++, s += kC) {
            s0 += s[0];
            if (kC == 3) { s1 += s[1]; s2 += s[2]; }
        }
    }
    const unsigned cnt = (unsigned)(x1 - x0) * (unsigned)(y1 - y0), mul = (unsigned)((1ull << 32) / (256ull * cnt)), amend = cnt / 2;
    unsigned char *o = e.out + p * kC;
    o[0] = (unsigned char)(((s0 + amend) * mul) >> 24);
    if (kC == 3) {
        o[1] = (unsigned char)(((s1 + amend) * mul) >> 24);
        o[2] = (unsigned char)(((s2 + amend) * mul) >> 24);
    }
}

// The horizontal pass: thread = one output pixel of a [out_h][out_w] image whose row y is input row y (e.in already points at the first
// row the vertical taps touch).  taps are transposed, [ksize][out_w], so that a wave reads them as it reads its pixels: side by side.
// Bounds: xmin >= 0 and xmin + cnt <= in_w by rs_taps.
template <int kC>
__global__ __launch_bounds__(kRsThreads) void k_rs_horizontal(const RsConv *__restrict__ entries, int n)
{
    const RsConv &e = tile_entry(entries, n);
    const long long p = ((long long)blockIdx.x - e.tile_base) * kRsThreads + threadIdx.x;
    if (p >= (long long)e.out_w * e.out_h) return;
    const int y = (int)(p / e.out_w), xx = (int)(p - (long long)y * e.out_w);
    const int xmin = e.bounds[2 * xx], cnt = e.bounds[2 * xx + 1];
    const unsigned char *s = e.in + ((long long)y * e.in_w + xmin) * kC;
    const int *t = e.taps + xx;
    int a0 = 1 << (kRsBits - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < cnt; k++, s += kC, t += e.out_w) {
        const int w = *t;
        a0 += s[0] * w;
        if (kC == 3) { a1 += s[1] * w; a2 += s[2] * w; }
    }
    unsigned char *o = e.out + p * kC;
    o[0] = rs_clip(a0);
    if (kC == 3) { o[1] = rs_clip(a1); o[2] = rs_clip(a2); }
}

// The vertical pass: thread = one output pixel; the taps of its row, [out_h][ksize], are the same for a whole row of threads.
// e.shift is the input's first row in the coordinates of the bounds (the horizontal pass left out the rows above it).
// Bounds: shift <= ymin and ymin + cnt - shift <= the input's rows by rs_taps and the host's choice of shift.
template <int kC>
__global__ __launch_bounds__(kRsThreads) void k_rs_vertical(const RsConv *__restrict__ entries, int n)
{
    const RsConv &e = tile_entry(entries, n);
    const long long p = ((long long)blockIdx.x - e.tile_base) * kRsThreads + threadIdx.x;
    if (p >= (long long)e.out_w * e.out_h) return;
    const int yy = (int)(p / e.out_w), x = (int)(p - (long long)yy * e.out_w);
    const int ymin = e.bounds[2 * yy] - e.shift, cnt = e.bounds[2 * yy + 1];
    const long long pitch = (long long)e.in_w * kC;
    const unsigned char *s = e.in + ymin * pitch + (long long)x * kC;
    const int *t = e.taps + (long long)yy * e.ksize;
    int a0 = 1 << (kRsBits - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < cnt; k++, s += pitch) {
        const int w = t[k];
        a0 += s[0] * w;
        if (kC == 3) { a1 += s[1] * w; a2 += s[2] * w; }
    }
    unsigned char *o = e.out + p * kC;
    o[0] = rs_clip(a0);
    if (kC == 3) { o[1] = rs_clip(a1); o[2] = rs_clip(a2); }
}

// ---- host: the plan of a call ----------------------------------------------------------------------------------------------------------------
static long long rs_tiles(long long px) { return (px + kRsThreads - 1) / kRsThreads; }

const char *rs_check(const aej_resample_desc &d, int *code)
{
    *code = AEJ_ERR_ARG;
    if (rs_support(d.filter) == 0.0) return "unknown filter (1 lanczos, 2 bilinear, 3 bicubic, 4 box, 5 hamming)";
    if (d.src_w < 1 || d.src_h < 1 || d.dst_w < 1 || d.dst_h < 1 || d.src_w > 65535 || d.src_h > 65535 || d.dst_w > 65535 || d.dst_h > 65535)
        return "a size below 1 or above 65535";
    if (d.src_offset < 0 || d.dst_offset < 0) return "a negative offset";
    if (d.reduce_x < 1 || d.reduce_y < 1 || (long long)d.reduce_x * d.reduce_y > (1 << 24)) return "reduce factors below 1 or a cell above 2^24 pixels";
    int w = d.src_w, h = d.src_h;
    if (d.reduce_x > 1 || d.reduce_y > 1) {
        const int *r = d.reduce_box;
        if (r[0] < 0 || r[1] < 0 || r[2] > w || r[3] > h || r[2] <= r[0] || r[3] <= r[1]) return "an empty reduce box or one outside the image";
        w = (r[2] - r[0] + d.reduce_x - 1) / d.reduce_x;
        h = (r[3] - r[1] + d.reduce_y - 1) / d.reduce_y;
    }
    const float *b = d.box;
    if (!(b[0] >= 0 && b[1] >= 0 && b[2] <= (float)w && b[3] <= (float)h)) return "a box outside the image";      // (also refuses NaN)
    if (!(b[2] - b[0] > 0 && b[3] - b[1] > 0)) return "an empty box";
    if (h > w * 100LL && d.dst_h < h) {
        *code = AEJ_ERR_UNSUPPORTED;
        return "an image more than 100 times as tall as wide made shorter (Pillow resizes it vertically first: not built)";
    }
    return nullptr;
}

// the table of one (axis, in_size, in0, in1, out_size, filter), built once per call: images of one size share it
struct RsTableKey {
    int axis, in_size, out_size, filter; float in0, in1;
    bool operator==(const RsTableKey &o) const
    {
        return axis == o.axis && in_size == o.in_size && out_size == o.out_size && filter == o.filter && in0 == o.in0 && in1 == o.in1;
    }
};

// The lookup is a linear scan of the call's tables, so a call whose images all differ in size costs O(images^2) comparisons on the
// host: nothing next to building the tables at the batch sizes in use (hundreds); a hash on the key is the remedy should that change.
// -> the table's first int in plan.ints: bounds [out][2], then the taps ([out][ksize]; axis 1: transposed, [ksize][out])
static long long rs_table(RsPlan &plan, std::vector<RsTableKey> &keys, std::vector<long long> &where, const RsTableKey &key, int ksize, bool identity,
                          bool fill)
{
    for (size_t i = 0; i < keys.size(); i++)
        if (keys[i] == key) return where[i];
    const long long at = plan.n_ints, n = (long long)key.out_size * (2 + ksize);
    plan.n_ints += n;
    keys.push_back(key);
    where.push_back(at);
    if (!fill) return at;
    plan.ints.resize(plan.n_ints);
    int *bounds = plan.ints.data() + at, *taps = bounds + 2LL * key.out_size;
    if (identity) {
        for (int i = 0; i < key.out_size; i++) { bounds[2 * i] = i; bounds[2 * i + 1] = 1; taps[i] = 1 << kRsBits; }
    } else if (key.axis == 0) {
        rs_taps(key.in_size, key.in0, key.in1, key.out_size, key.filter, ksize, bounds, taps);
    } else {
        std::vector<int> rows((size_t)key.out_size * ksize);
        rs_taps(key.in_size, key.in0, key.in1, key.out_size, key.filter, ksize, bounds, rows.data());
        for (int i = 0; i < key.out_size; i++)
            for (int k = 0; k < ksize; k++) taps[(long long)k * key.out_size + i] = rows[(size_t)i * ksize + k];
    }
    return at;
}

// fill = false: sizes only (aej_resample_workspace_bytes); the bounds of the vertical tables are needed either way (they size the
// horizontal pass), so those are computed on the side.  channels (may be NULL: every image 3): 3 or 1 per image, the bytes of a pixel;
// the images of either count form launches of their own (RsPlan::count, ::tiles).  -> -1, or the first descriptor refused (*why, *code)
// windows (may be NULL: none; the _win entries): [n][4] x0, y0, vw, vh -- the stored source of image i, src_w x src_h, is the rectangle
// [y0, y0 + src_h) x [x0, x0 + src_w) of a virtual image vw x vh in whose coordinates box and reduce_box are.  Everything is planned
// from the virtual size -- the tables are those of the whole image, rs_taps never sees a shifted origin -- and only the first stage's
// base pointer (RsImage::win_shift, which may point before the stored bytes: no byte outside them is read) and pitch move.  Refused
// here, on the host: a window outside its virtual image, and a tap with a non-zero count or a reduce box that reaches outside the
// stored rectangle.
static bool rs_axis_inside(int in_size, float in0, float in1, int out_size, int f, int lo, int hi)
{
    for (int xx = 0; xx < out_size; xx++) {
        int b[2];
        rs_bounds_of_row(in_size, in0, in1, out_size, f, xx, b);
        if (b[1] > 0 && (b[0] < lo || b[0] + b[1] > hi)) return false;
    }
    return true;
}

int resample_plan(const aej_resample_desc *descs, int n, bool fill, RsPlan &plan, const char **why, int *code, const int *channels, const int *windows)
{
    plan = RsPlan{};
    std::vector<RsTableKey> keys;
    std::vector<long long> where;
    for (int i = 0; i < n; i++) {
        aej_resample_desc d = descs[i];
        const int sw = d.src_w, sh = d.src_h;        // the stored rectangle: its pitch and rows
        int wx0 = 0, wy0 = 0;
        if (windows) {
            const int *q = windows + 4 * i;
            *code = AEJ_ERR_ARG;
            if (sw < 1 || sh < 1 || q[0] < 0 || q[1] < 0 || q[2] < 1 || q[3] < 1 || q[2] > 65535 || q[3] > 65535 || (long long)q[0] + sw > q[2] ||
                (long long)q[1] + sh > q[3]) {
                *why = "a window (x0, y0, vw, vh) that does not hold the stored src_w x src_h rectangle";
                return i;
            }
            wx0 = q[0]; wy0 = q[1]; d.src_w = q[2]; d.src_h = q[3];      // planned as the whole virtual image
        }
        if ((*why = rs_check(d, code)) != nullptr) return i;
        const int ch = channels ? channels[i] : 3;
        if (ch != 1 && ch != 3) { *why = "a channel count other than 1 or 3"; *code = AEJ_ERR_ARG; return i; }
        RsImage im{};
        im.ch = ch;
        long long *tiles = plan.tiles[ch == 1];
        int w = d.src_w, h = d.src_h;
        im.reduce = d.reduce_x > 1 || d.reduce_y > 1;
        if (im.reduce) {
            const int *r = d.reduce_box;
            RsReduce &e = im.r;
            e.bw = r[2] - r[0]; e.bh = r[3] - r[1]; e.fx = d.reduce_x; e.fy = d.reduce_y; e.in_w = sw;
            if (windows && (r[0] < wx0 || r[1] < wy0 || r[2] > wx0 + sw || r[3] > wy0 + sh)) {
                *why = "a reduce box that reaches outside the stored window"; *code = AEJ_ERR_ARG;
                return i;
            }
            e.out_w = w = (e.bw + e.fx - 1) / e.fx;
            e.out_h = h = (e.bh + e.fy - 1) / e.fy;
            im.r_src = d.src_offset + ((long long)(r[1] - wy0) * sw + (r[0] - wx0)) * ch;
            e.tile_base = tiles[0];
            tiles[0] += rs_tiles((long long)w * h);
            im.tmp_a = plan.tmp_bytes;
            plan.tmp_bytes += align_up((long long)w * h * ch, 256);
        }
        const float *b = d.box;
        im.horizontal = d.dst_w != w || b[0] != 0 || b[2] != (float)d.dst_w;
        im.vertical = d.dst_h != h || b[1] != 0 || b[3] != (float)d.dst_h;
        const bool copy = !im.reduce && !im.horizontal && !im.vertical;
        int first = 0, last = h;
        if (windows && !im.reduce) {                  // the first stage reads the stored rectangle: every tap inside it
            const bool cols = im.horizontal ? rs_axis_inside(w, b[0], b[2], d.dst_w, d.filter, wx0, wx0 + sw) : wx0 == 0 && sw == w;
            const bool rows = im.vertical ? rs_axis_inside(h, b[1], b[3], d.dst_h, d.filter, wy0, wy0 + sh) : wy0 == 0 && sh == h;
            if (!cols || !rows) {
                *why = "a tap that reaches outside the stored window"; *code = AEJ_ERR_ARG;
                return i;
            }
        }
        if (im.vertical || copy) {
            RsConv &e = im.v;
            e.ksize = copy ? 1 : rs_ksize(b[1], b[3], d.dst_h, d.filter);
            const RsTableKey key{0, h, d.dst_h, copy ? 0 : d.filter, copy ? 0.f : b[1], copy ? 0.f : b[3]};
            im.v_table = rs_table(plan, keys, where, key, e.ksize, copy, fill);
            if (im.horizontal) {                     // the rows the vertical taps touch: those of the first and of the last output row
                int b0[2], b1[2];
                rs_bounds_of_row(h, b[1], b[3], d.dst_h, d.filter, 0, b0);
                rs_bounds_of_row(h, b[1], b[3], d.dst_h, d.filter, d.dst_h - 1, b1);
                first = b0[0];
                last = b1[0] + b1[1];
            }
            e.shift = first;
            e.in_w = e.out_w = d.dst_w; e.out_h = d.dst_h;
            if (windows && !im.reduce && !im.horizontal) e.in_w = sw;      // reads the stored rectangle itself
            e.tile_base = tiles[2];
            tiles[2] += rs_tiles((long long)e.out_w * e.out_h);
        }
        if (im.horizontal) {
            RsConv &e = im.h;
            e.ksize = rs_ksize(b[0], b[2], d.dst_w, d.filter);
            const RsTableKey key{1, w, d.dst_w, d.filter, b[0], b[2]};
            im.h_table = rs_table(plan, keys, where, key, e.ksize, false, fill);
            e.in_w = windows && !im.reduce ? sw : w; e.out_w = d.dst_w; e.out_h = last - first; e.shift = first;
            e.tile_base = tiles[1];
            tiles[1] += rs_tiles((long long)e.out_w * e.out_h);
            if (im.vertical) {
                im.tmp_b = plan.tmp_bytes;
                plan.tmp_bytes += align_up((long long)e.out_w * e.out_h * ch, 256);
            }
        }
        im.win_shift = windows && !im.reduce ? -((long long)wy0 * sw + wx0) * ch : 0;
        plan.spans.reads.push_back({ i, d.src_offset, (long long)sw * sh * ch });
        plan.spans.writes.push_back({ i, d.dst_offset, (long long)d.dst_w * d.dst_h * ch });
        int *count = plan.count[ch == 1];
        count[0] += im.reduce; count[1] += im.horizontal; count[2] += im.vertical || copy;
        plan.images.push_back(im);
    }
    return -1;
}

// the entries of a call: reduce (RGB images, then one-channel ones), horizontal (likewise), vertical (likewise)
static long long rs_entry_bytes(const RsPlan &p)
{
    return align_up(sizeof(RsReduce) * (p.count[0][0] + p.count[1][0]) +
                    sizeof(RsConv) * (p.count[0][1] + p.count[1][1] + p.count[0][2] + p.count[1][2]), 16);
}

static long long rs_blob_bytes(const RsPlan &p) { return rs_entry_bytes(p) + 4 * p.n_ints; }

unsigned long long resample_carve(void *base, const RsPlan &plan, RsBufs &w)
{
    Carver c(base);
    w.blob = c.take<unsigned char>(rs_blob_bytes(plan));
    w.tmp = c.take<unsigned char>(plan.tmp_bytes);
    return c.bytes();
}

// the upload of a call: the entries of the three stages with their device pointers, then the tables
void resample_blob(const RsPlan &plan, const RsBufs &w, const unsigned char *src, unsigned char *dst, std::vector<unsigned char> &blob)
{
    blob.assign(rs_blob_bytes(plan), 0);
    const long long entries = rs_entry_bytes(plan);
    RsReduce *rr[2];
    RsConv *hh[2], *vv[2];
    rr[0] = (RsReduce *)blob.data(); rr[1] = rr[0] + plan.count[0][0];
    hh[0] = (RsConv *)(rr[1] + plan.count[1][0]); hh[1] = hh[0] + plan.count[0][1];
    vv[0] = hh[1] + plan.count[1][1]; vv[1] = vv[0] + plan.count[0][2];
    const int *ints = (const int *)(w.blob + entries);
    if (plan.n_ints) memcpy(blob.data() + entries, plan.ints.data(), 4 * plan.n_ints);
    for (size_t i = 0; i < plan.images.size(); i++) {
        const RsImage &im = plan.images[i];
        const unsigned char *in = src + plan.spans.reads[i].offset + im.win_shift;      // pixel (0, 0) of the virtual image, were it stored
        unsigned char *out = dst + plan.spans.writes[i].offset;
        const bool copy = !im.reduce && !im.horizontal && !im.vertical;
        RsReduce *&r = rr[im.ch == 1];
        RsConv *&h = hh[im.ch == 1], *&v = vv[im.ch == 1];
        if (im.reduce) {
            *r = im.r;
            r->in = src + im.r_src;
            r->out = im.horizontal || im.vertical ? w.tmp + im.tmp_a : out;
            in = r->out;
            r++;
        }
        if (im.horizontal) {
            *h = im.h;
            h->in = in + (long long)im.h.shift * im.h.in_w * im.ch;
            h->out = im.vertical ? w.tmp + im.tmp_b : out;
            h->bounds = ints + im.h_table;
            h->taps = h->bounds + 2LL * im.h.out_w;
            in = h->out;
            h++;
        }
        if (im.vertical || copy) {
            *v = im.v;
            v->in = in;
            v->out = out;
            v->bounds = ints + im.v_table;
            v->taps = v->bounds + 2LL * im.v.out_h;
            v++;
        }
    }
}

hipError_t launch_resample(hipStream_t st, const RsPlan &plan, const RsBufs &w, const void *blob_host, unsigned long long blob_bytes)
{
    hipError_t e = hipMemcpyAsync(w.blob, blob_host, blob_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    const int (&c)[2][3] = plan.count;
    const long long (&tl)[2][3] = plan.tiles;
    const RsReduce *r3 = (const RsReduce *)w.blob, *r1 = r3 + c[0][0];
    const RsConv *h3 = (const RsConv *)(r1 + c[1][0]), *h1 = h3 + c[0][1], *v3 = h1 + c[1][1], *v1 = v3 + c[0][2];
    // stage by stage: an image's stages follow each other on the stream, and images of different channel counts share nothing
    if (c[0][0]) hipLaunchKernelGGL(k_rs_reduce<3>, dim3((unsigned)tl[0][0]), dim3(kRsThreads), 0, st, r3, c[0][0]);
    if (c[1][0]) hipLaunchKernelGGL(k_rs_reduce<1>, dim3((unsigned)tl[1][0]), dim3(kRsThreads), 0, st, r1, c[1][0]);
    if (c[0][1]) hipLaunchKernelGGL(k_rs_horizontal<3>, dim3((unsigned)tl[0][1]), dim3(kRsThreads), 0, st, h3, c[0][1]);
    if (c[1][1]) hipLaunchKernelGGL(k_rs_horizontal<1>, dim3((unsigned)tl[1][1]), dim3(kRsThreads), 0, st, h1, c[1][1]);
    if (c[0][2]) hipLaunchKernelGGL(k_rs_vertical<3>, dim3((unsigned)tl[0][2]), dim3(kRsThreads), 0, st, v3, c[0][2]);
    if (c[1][2]) hipLaunchKernelGGL(k_rs_vertical<1>, dim3((unsigned)tl[1][2]), dim3(kRsThreads), 0, st, v1, c[1][2]);
    return hipGetLastError();
}

}  // namespace aej
