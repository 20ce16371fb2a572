// convert.hip -- Pillow's Image.convert between L, LA, RGB, RGBA, YCbCr, HSV and CMYK, convert(mode, matrix), hue adjustment and
// ImageOps.colorize on the device (aej_convert_*), bit for bit, over many packed 8-bit images of different sizes and conversions in one
// call.  include/aej.h has the arithmetic.
//
//   k_convert<CIN, COUT>   reads each source byte once, runs the entry's step program per pixel in registers -- one or two converters of
//                          Image.convert (the route through the base mode is never written anywhere), or a matrix, a hue shift between
//                          RGB -> HSV and HSV -> RGB, or a colorize table -- and writes each output byte once
// A lane takes 16 / 8 / 4 / 4 adjacent pixels of 1 / 2 / 3 / 4 input channels by one vector access at whatever address the packed image
// has, and the last pixels of an image byte by byte, as k_adjust_apply.  A launch is one grid over every image of one (CIN, COUT) pair (a
// per-image entry, a prefix sum of chunks, a binary search by chunk); the grid is capped at kCvMaxGrid and the workgroups stride.
// The twelve 256-entry tables of the YCbCr converters are compile-time constants staged in LDS once per workgroup of a launch that has
// an entry reading them; a colorize table is staged per chunk.  Bounds: a lane touches pixel q only if q < npix; a table index is
// masked to 8 bits.
#include <math.h>
#include <string.h>

#include <vector>

#include "aej_ctx.h"

#pragma clang fp contract(off)

namespace aej {

template <int kC> struct CvLane { static constexpr int pix = kC == 1 ? 16 : kC == 2 ? 8 : 4; };

// T(coef)[i] = (int)(coef i 64 + 0.5) and U(coef)[i] = (int)(coef (i - 128) 64 + 0.5), float64, the cast truncating
enum { kCvYr = 0, kCvYg, kCvYb, kCvCbR, kCvCbG, kCvHalf, kCvCrG, kCvCrB, kCvRCr, kCvGCb, kCvGCr, kCvBCb, kCvTabs };
struct CvYcc { short t[kCvTabs][256]; };
constexpr CvYcc cv_make_ycc()
{
    constexpr double coef[kCvTabs] = { .299, .587, .114, -.16874, -.33126, .5, -.41869, -.08131, 1.402, -.34414, -.71414, 1.772 };
    CvYcc y = {};
    for (int k = 0; k < kCvTabs; k++)
        for (int i = 0; i < 256; i++) y.t[k][i] = (short)(int)(coef[k] * (k >= kCvRCr ? i - 128 : i) * 64 + 0.5);
    return y;
}
__device__ const CvYcc kCvYccTables = cv_make_ycc();

__device__ __forceinline__ int cv_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
__device__ __forceinline__ int cv_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ __forceinline__ void cv_rgb_to_hsv(int r, int g, int b, int &H, int &S, int &V)
{
    const int mx = max(max(r, g), b), mn = min(min(r, g), b);
    V = mx;
    H = S = 0;
    if (mx == mn) return;
    const float cr = (float)(mx - mn);
    const float s = __fdiv_rn(cr, (float)mx);
    const float rc = __fdiv_rn((float)(mx - r), cr), gc = __fdiv_rn((float)(mx - g), cr), bc = __fdiv_rn((float)(mx - b), cr);
    double hd;
    if (r == mx) hd = __dsub_rn((double)bc, (double)gc);
    else if (g == mx) hd = __dsub_rn(__dadd_rn(2.0, (double)rc), (double)bc);
    else hd = __dsub_rn(__dadd_rn(4.0, (double)gc), (double)rc);
    float h = (float)hd;
    double x = __dadd_rn(__ddiv_rn((double)h, 6.0), 1.0);      // in (0.83, 1.84): fmod(x, 1.0) is x - 1 at and above 1, exactly
    if (x >= 1.0) x = __dsub_rn(x, 1.0);
    h = (float)x;
    H = cv_clip8((int)__dmul_rn((double)h, 255.0));
    S = cv_clip8((int)__dmul_rn((double)s, 255.0));
}

__device__ __forceinline__ void cv_hsv_to_rgb(int h, int s, int v, int &r, int &g, int &b)
{
    r = g = b = v;
    if (s == 0) return;
    const double x = __ddiv_rn(__dmul_rn((double)h, 6.0), 255.0);
    const double fl = floor(x);
    const double f = (double)(float)__dsub_rn(x, fl);
    const double fs = (double)(float)__ddiv_rn((double)s, 255.0);
    const double vv = (double)v;
    const int p = cv_clip8((int)round(__dmul_rn(vv, __dsub_rn(1.0, fs))));
    const int q = cv_clip8((int)round(__dmul_rn(vv, __dsub_rn(1.0, __dmul_rn(fs, f)))));
    const int t = cv_clip8((int)round(__dmul_rn(vv, __dsub_rn(1.0, __dmul_rn(fs, __dsub_rn(1.0, f))))));
    switch ((int)fl % 6) {                                    // h 6 / 255 is in [0, 6]
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
    }
}

// one converter of Image.convert on one pixel, in place: px holds the bands of `from`, then those of `to`
__device__ __forceinline__ void cv_step(int from, int to, int (&px)[4], const short (*ycc)[256])
{
    if (from == to) return;
    const int alpha = from == AEJ_MODE_LA ? px[1] : from == AEJ_MODE_RGBA ? px[3] : 255;
    const bool grey = from == AEJ_MODE_L || from == AEJ_MODE_LA || (from == AEJ_MODE_YCBCR && (to == AEJ_MODE_L || to == AEJ_MODE_LA));
    int r = px[0], g = px[1], b = px[2];
    if (grey) {
        g = b = r;
    } else if (from == AEJ_MODE_CMYK) {
        const int nk = 255 - px[3];
        int o[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int t = px[c] * nk + 128;
            o[c] = cv_clip8(nk - (((t >> 8) + t) >> 8));
        }
        r = o[0]; g = o[1]; b = o[2];
    } else if (from == AEJ_MODE_YCBCR) {
        const int y = px[0], cb = px[1] & 255, cr = px[2] & 255;
        r = cv_clip8(y + ((int)ycc[kCvRCr][cr] >> 6));
        g = cv_clip8(y + (((int)ycc[kCvGCb][cb] + (int)ycc[kCvGCr][cr]) >> 6));
        b = cv_clip8(y + ((int)ycc[kCvBCb][cb] >> 6));
    } else if (from == AEJ_MODE_HSV) {
        cv_hsv_to_rgb(px[0], px[1], px[2], r, g, b);
    }
    int na = 0;                                               // the colour bands of `to`
    if (to == AEJ_MODE_L || to == AEJ_MODE_LA) {
        px[0] = grey ? r : cv_luma(r, g, b);
        na = 1;
    } else if (to == AEJ_MODE_RGB || to == AEJ_MODE_RGBA) {
        px[0] = r; px[1] = g; px[2] = b;
        na = 3;
    } else if (to == AEJ_MODE_YCBCR) {
        if (grey) {
            px[0] = r; px[1] = 128; px[2] = 128;
        } else {
            r &= 255; g &= 255; b &= 255;
            px[0] = ((int)ycc[kCvYr][r] + (int)ycc[kCvYg][g] + (int)ycc[kCvYb][b]) >> 6;
            px[1] = cv_clip8((((int)ycc[kCvCbR][r] + (int)ycc[kCvCbG][g] + (int)ycc[kCvHalf][b]) >> 6) + 128);
            px[2] = cv_clip8((((int)ycc[kCvHalf][r] + (int)ycc[kCvCrG][g] + (int)ycc[kCvCrB][b]) >> 6) + 128);
        }
    } else if (to == AEJ_MODE_HSV) {
        if (grey) {
            px[0] = 0; px[1] = 0; px[2] = r;
        } else {
            cv_rgb_to_hsv(r, g, b, px[0], px[1], px[2]);
        }
    } else {                                                  // AEJ_MODE_CMYK
        if (grey) {
            px[0] = 0; px[1] = 0; px[2] = 0; px[3] = 255 - r;
        } else {
            px[0] = 255 - r; px[1] = 255 - g; px[2] = 255 - b; px[3] = 0;
        }
    }
    if (to == AEJ_MODE_LA || to == AEJ_MODE_RGBA) px[na] = alpha;
}

// convert(mode, matrix)'s band: float32, left to right, the products and the sums rounded one by one
__device__ __forceinline__ int cv_matrix_row(const float *m, float r, float g, float b)
{
    float v = __fadd_rn(__fmul_rn(m[0], r), __fmul_rn(m[1], g));
    v = __fadd_rn(v, __fmul_rn(m[2], b));
    v = __fadd_rn(__fadd_rn(v, m[3]), 0.5f);
    return v <= 0.f ? 0 : v >= 255.f ? 255 : (int)v;
}

// the entry's program on one pixel: px holds kIn bands, then the output's
__device__ __forceinline__ void cv_run(const CvEntry &e, const short (*ycc)[256], const unsigned char *tab, int (&px)[4])
{
    if (e.kind == AEJ_CONVERT_MODE) {
        cv_step(e.from[0], e.to[0], px, ycc);
        if (e.n_steps > 1) cv_step(e.from[1], e.to[1], px, ycc);
    } else if (e.kind == AEJ_CONVERT_HUE) {                   // (alpha, if there is one, stays in px[3])
        int h, s, v;
        cv_rgb_to_hsv(px[0], px[1], px[2], h, s, v);
        cv_hsv_to_rgb((h + e.hue) & 255, s, v, px[0], px[1], px[2]);
    } else if (e.kind == AEJ_CONVERT_MATRIX) {
        const float r = (float)px[0], g = (float)px[1], b = (float)px[2];
        px[0] = cv_matrix_row(e.m, r, g, b);
        if (e.to[0] == AEJ_MODE_RGB) {
            px[1] = cv_matrix_row(e.m + 4, r, g, b);
            px[2] = cv_matrix_row(e.m + 8, r, g, b);
        }
    } else {                                                  // AEJ_CONVERT_TABLE
        const int l = px[0] & 255;
        px[0] = (int)tab[l]; px[1] = (int)tab[256 + l]; px[2] = (int)tab[512 + l];
    }
}

template <int kIn, int kOut>
__global__ __launch_bounds__(kCvThreads) void k_convert(const CvEntry *__restrict__ entries, int n, long long chunks, int any_ycc)
{
    constexpr int kP = CvLane<kIn>::pix;
    __shared__ short ycc[kCvTabs][256];
    __shared__ __align__(16) unsigned char tab[AEJ_CONVERT_TABLE_BYTES];
    if (any_ycc) {
        for (int i = threadIdx.x; i < kCvTabs * 256; i += kCvThreads) (&ycc[0][0])[i] = (&kCvYccTables.t[0][0])[i];
        __syncthreads();
    }
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const CvEntry &e = chunk_entry(entries, n, chunk);
        const bool staged = e.kind == AEJ_CONVERT_TABLE;     // (uniform over the workgroup: one entry per chunk)
        if (staged) {
            for (int i = threadIdx.x; i < AEJ_CONVERT_TABLE_BYTES / 4; i += kCvThreads) ((unsigned *)tab)[i] = ((const unsigned *)e.table)[i];
            __syncthreads();
        }
        const long long p0 = (chunk - e.chunk_base) * kCvChunk;
        for (int j = 0; j < kCvChunk / (kCvThreads * kP); j++) {
            const long long q = p0 + ((long long)j * kCvThreads + threadIdx.x) * kP;
            if (q >= e.npix) continue;
            const bool whole = q + kP <= e.npix;
            const unsigned char *in = e.in + q * kIn;
            unsigned char *o = e.out + q * kOut;
            unsigned wi[kP * kIn / 4], wo[kP * kOut / 4] = {};
            if (whole) __builtin_memcpy(wi, in, kP * kIn);
#pragma unroll
            for (int i = 0; i < kP; i++) {
                int px[4] = { 0, 0, 0, 0 };
                if (whole) {
#pragma unroll
                    for (int b = 0; b < kIn; b++) {
                        const int at = i * kIn + b;
                        px[b] = (int)((wi[at >> 2] >> (8 * (at & 3))) & 255u);
                    }
                } else {
                    if (q + i >= e.npix) break;
#pragma unroll
                    for (int b = 0; b < kIn; b++) px[b] = (int)in[i * kIn + b];
                }
                cv_run(e, ycc, tab, px);
                if (whole) {
#pragma unroll
                    for (int b = 0; b < kOut; b++) {
                        const int at = i * kOut + b;
                        wo[at >> 2] |= (unsigned)(px[b] & 255) << (8 * (at & 3));
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < kOut; b++) o[i * kOut + b] = (unsigned char)px[b];
                }
            }
            if (whole) __builtin_memcpy(o, wo, kP * kOut);
        }
        if (staged) __syncthreads();                          // the next chunk's table replaces this one
    }
}

// ---- host: the route of one descriptor, and the plan of a call ------------------------------------------------------------------------
static const int kCvBands[7] = { 1, 2, 3, 4, 3, 3, 4 };
static const int kCvBase[7] = { AEJ_MODE_L, AEJ_MODE_L, AEJ_MODE_RGB, AEJ_MODE_RGB, AEJ_MODE_RGB, AEJ_MODE_RGB, AEJ_MODE_RGB };

// whether Image.convert has a converter from one mode to another (a mode to itself is a copy)
static bool cv_direct(int from, int to)
{
    if (from == to || from <= AEJ_MODE_RGBA) return true;
    if (from == AEJ_MODE_YCBCR) return to == AEJ_MODE_L || to == AEJ_MODE_LA || to == AEJ_MODE_RGB;
    if (from == AEJ_MODE_HSV) return to == AEJ_MODE_RGB;
    return to == AEJ_MODE_RGB || to == AEJ_MODE_RGBA || to == AEJ_MODE_HSV;      // AEJ_MODE_CMYK
}

int convert_resolve(const aej_convert_desc &d, int n_tables, aej_convert_plan &p, const char **why)
{
    memset(&p, 0, sizeof p);
    if (d.width < 1 || d.height < 1 || d.width > kCvMaxSide || d.height > kCvMaxSide) { *why = "sizes from 1 to 32767 a side"; return AEJ_ERR_ARG; }
    if (d.channels < 1 || d.channels > 4) { *why = "1 to 4 channels"; return AEJ_ERR_ARG; }
    if (d.src_offset < 0 || d.dst_offset < 0) { *why = "negative offset"; return AEJ_ERR_ARG; }
    const int s = d.source_mode, t = d.target_mode;
    if (s < 0 || s > AEJ_MODE_CMYK || t < 0 || t > AEJ_MODE_CMYK) { *why = "unknown mode"; return AEJ_ERR_ARG; }
    if (kCvBands[s] != d.channels) { *why = "a source mode whose bands are not the image's channels"; return AEJ_ERR_ARG; }
    p.out_channels = kCvBands[t];
    p.n_steps = 1;
    p.step_from[0] = s;
    p.step_to[0] = t;
    switch (d.kind) {
    case AEJ_CONVERT_MODE:
        if (!cv_direct(s, t)) {
            p.n_steps = 2;
            p.step_to[0] = p.step_from[1] = kCvBase[s];
            p.step_to[1] = t;
        }
        break;
    case AEJ_CONVERT_MATRIX:
        if (s != AEJ_MODE_RGB || (t != AEJ_MODE_L && t != AEJ_MODE_RGB)) { *why = "a matrix takes an RGB source and the target L or RGB"; return AEJ_ERR_ARG; }
        for (int k = 0; k < (t == AEJ_MODE_L ? 4 : 12); k++)
            if (!isfinite(d.matrix[k])) { *why = "a matrix entry that is not finite"; return AEJ_ERR_ARG; }
        break;
    case AEJ_CONVERT_HUE:
        if ((s != AEJ_MODE_RGB && s != AEJ_MODE_RGBA) || t != s) { *why = "a hue shift takes RGB or RGBA and leaves the same"; return AEJ_ERR_ARG; }
        if (d.hue_shift < 0 || d.hue_shift > 255) { *why = "a hue shift outside 0 .. 255"; return AEJ_ERR_ARG; }
        p.n_steps = 2;
        p.step_from[0] = AEJ_MODE_RGB; p.step_to[0] = AEJ_MODE_HSV;
        p.step_from[1] = AEJ_MODE_HSV; p.step_to[1] = AEJ_MODE_RGB;
        break;
    case AEJ_CONVERT_TABLE:
        if (s != AEJ_MODE_L || t != AEJ_MODE_RGB) { *why = "a colorize table takes L and leaves RGB"; return AEJ_ERR_ARG; }
        if (n_tables >= 0 && (d.table < 0 || d.table >= n_tables)) { *why = "a table number outside the tables"; return AEJ_ERR_ARG; }
        break;
    default:
        *why = "unknown kind";
        return AEJ_ERR_ARG;
    }
    return 0;
}

static bool cv_reads_ycc(int from, int to)
{
    return from != to && ((from == AEJ_MODE_YCBCR && to != AEJ_MODE_L && to != AEJ_MODE_LA) || (to == AEJ_MODE_YCBCR && from >= AEJ_MODE_RGB));
}

// -> 0, or the error code with *bad the image and *why the reason.  workspace NULL: everything but the device pointers, and plan.bytes.
int convert_plan(const aej_convert_desc *descs, int n, const unsigned char *tables_host, int n_tables, void *workspace,
                 const unsigned char *src, unsigned char *dst, CvPlan &plan, int *bad, const char **why)
{
    plan = CvPlan();
    std::vector<aej_convert_plan> cp(n);
    for (int i = 0; i < n; i++) {
        *bad = i;
        const int code = convert_resolve(descs[i], n_tables, cp[i], why);
        if (code) return code;
        const long long npix = (long long)descs[i].width * descs[i].height;
        plan.spans.reads.push_back({ i, descs[i].src_offset, npix * descs[i].channels });
        plan.spans.writes.push_back({ i, descs[i].dst_offset, npix * cp[i].out_channels });
    }
    *bad = -1;
    Carver cv(workspace);
    plan.entries_dev = cv.take<unsigned char>((long long)n * (long long)sizeof(CvEntry));
    int used_tables = 0;                                      // the tables the descriptors name: what the size query, which sees no tables, can count too
    for (int i = 0; i < n; i++)
        if (descs[i].kind == AEJ_CONVERT_TABLE) used_tables = std::max(used_tables, descs[i].table + 1);
    plan.tables_dev = cv.take<unsigned char>((long long)used_tables * AEJ_CONVERT_TABLE_BYTES);
    if (tables_host && used_tables > 0) plan.tables.assign(tables_host, tables_host + (size_t)used_tables * AEJ_CONVERT_TABLE_BYTES);
    for (int cin = 1; cin <= 4; cin++)
        for (int cout = 1; cout <= 4; cout++) {
            CvLaunch l = { cin, cout, (int)plan.entries.size(), 0, 0 };
            for (int i = 0; i < n; i++) {
                const aej_convert_desc &d = descs[i];
                if (d.channels != cin || cp[i].out_channels != cout) continue;
                CvEntry e;
                memset(&e, 0, sizeof e);
                e.in = src ? src + d.src_offset : nullptr;
                e.out = dst ? dst + d.dst_offset : nullptr;
                e.table = d.kind == AEJ_CONVERT_TABLE && plan.tables_dev ? plan.tables_dev + (long long)d.table * AEJ_CONVERT_TABLE_BYTES : nullptr;
                e.npix = (long long)d.width * d.height;
                e.kind = d.kind;
                e.n_steps = cp[i].n_steps;
                e.hue = d.hue_shift & 255;
                for (int k = 0; k < 2; k++) { e.from[k] = cp[i].step_from[k]; e.to[k] = cp[i].step_to[k]; }
                if (d.kind == AEJ_CONVERT_MODE)
                    for (int k = 0; k < e.n_steps; k++) e.ycc |= cv_reads_ycc(e.from[k], e.to[k]) ? 1 : 0;
                memcpy(e.m, d.matrix, sizeof e.m);
                e.chunk_base = l.chunks;
                l.chunks += (e.npix + kCvChunk - 1) / kCvChunk;
                plan.entries.push_back(e);
            }
            l.count = (int)plan.entries.size() - l.first;
            if (l.count) plan.launches.push_back(l);
        }
    plan.bytes = cv.bytes();
    return 0;
}

template <int kIn, int kOut>
static void cv_launch(hipStream_t st, const CvLaunch &l, const CvEntry *entries, int any_ycc)
{
    const dim3 grid((unsigned)std::min<long long>(l.chunks, kCvMaxGrid)), block(kCvThreads);
    hipLaunchKernelGGL((k_convert<kIn, kOut>), grid, block, 0, st, entries, l.count, l.chunks, any_ycc);
}

template <int kIn>
static void cv_launch_in(hipStream_t st, const CvLaunch &l, const CvEntry *entries, int any_ycc)
{
    if (l.cout == 1) cv_launch<kIn, 1>(st, l, entries, any_ycc);
    if (l.cout == 2) cv_launch<kIn, 2>(st, l, entries, any_ycc);
    if (l.cout == 3) cv_launch<kIn, 3>(st, l, entries, any_ycc);
    if (l.cout == 4) cv_launch<kIn, 4>(st, l, entries, any_ycc);
}

// everything of a call on one stream: the uploads, then one launch per pair of channel counts.  The caller waits.
hipError_t launch_convert(hipStream_t st, const CvPlan &plan)
{
    hipError_t e = hipMemcpyAsync(plan.entries_dev, plan.entries.data(), plan.entries.size() * sizeof(CvEntry), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if (!plan.tables.empty()) {
        e = hipMemcpyAsync(plan.tables_dev, plan.tables.data(), plan.tables.size(), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    for (const CvLaunch &l : plan.launches) {
        const CvEntry *entries = (const CvEntry *)plan.entries_dev + l.first;
        int any_ycc = 0;
        for (int k = 0; k < l.count; k++) any_ycc |= plan.entries[l.first + k].ycc;
        if (l.cin == 1) cv_launch_in<1>(st, l, entries, any_ycc);
        if (l.cin == 2) cv_launch_in<2>(st, l, entries, any_ycc);
        if (l.cin == 3) cv_launch_in<3>(st, l, entries, any_ycc);
        if (l.cin == 4) cv_launch_in<4>(st, l, entries, any_ycc);
    }
    return hipGetLastError();
}

}  // namespace aej
