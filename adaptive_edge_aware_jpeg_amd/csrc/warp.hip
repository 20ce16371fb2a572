// warp.hip -- Pillow's Image.transform (AFFINE, PERSPECTIVE, QUAD under NEAREST, BILINEAR, BICUBIC) and Image.transpose on the device
// (aej_warp_*), bit for bit, over many packed 8-bit images of 1 to 4 channels, of different sizes, paths and filters, in one call.
// include/aej.h has the arithmetic: IEEE float64, one rounded operation at a time, in Pillow's order.
//
//   k_warp<C, FILTER, PATH>   a gather: one lane per output pixel, all its channels; a workgroup owns a compact 32 x 8 output tile, so
//                             that the source footprint of a rotated tile is a small parallelogram that stays in cache (a 256 x 1
//                             strip would walk a 256-row column of the source under a 90 degree matrix).  Alpha is premultiplied as a
//                             sample is loaded and un-premultiplied as the pixel is stored: no extra pass, no extra buffer.
//   k_flip<C>                 FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, ROTATE_180: a mirrored copy, a lane writes 4 adjacent bytes of a row
//   k_transpose<C>            the five methods that swap the axes: a 32 x 32 tile through LDS, rows read and rows written
// A launch is one grid over every image that needs it (a per-image entry, a prefix sum of workgroups, a binary search by blockIdx.x,
// as window.hip's).  Bounds: every source column and row is clamped to the image or tested against it before it is read, a table
// entry is range-tested, and only lanes with an in-image output pixel load or store.
#include <math.h>
#include <string.h>

#include <vector>

#include "aej_ctx.h"

#pragma clang fp contract(off)

namespace aej {

// nb (1 .. 4) bytes at any address, as the low bytes of a word
__device__ __forceinline__ unsigned wp_load4(const unsigned char *p, int nb)
{
    unsigned v = 0;
    if (nb == 4) {
        __builtin_memcpy(&v, p, 4);
    } else {
        for (int b = 0; b < nb; b++) v |= (unsigned)p[b] << (8 * b);
    }
    return v;
}

__device__ __forceinline__ void wp_store4(unsigned char *p, int nb, unsigned v)
{
    if (nb == 4) {
        __builtin_memcpy(p, &v, 4);
    } else {
        for (int b = 0; b < nb; b++) p[b] = (unsigned char)(v >> (8 * b));
    }
}

// the pixel at (x, y), both inside the image, as kC ints; premultiplied by its last channel if asked
template <int kC>
__device__ __forceinline__ void wp_pixel(const WpEntry &e, int x, int y, bool premul, int *p)
{
    const unsigned char *s = e.in + ((long long)y * e.sw + x) * kC;
    if (kC == 4) {
        const unsigned v = wp_load4(s, 4);
        for (int c = 0; c < 4; c++) p[c] = (int)((v >> (8 * c)) & 255u);
    } else {
        for (int c = 0; c < kC; c++) p[c] = s[c];
    }
    if ((kC == 2 || kC == 4) && premul) {
        for (int c = 0; c < kC - 1; c++) {
            const int t = p[c] * p[kC - 1] + 128;
            p[c] = ((t >> 8) + t) >> 8;
        }
    }
}

template <int kPath>
__device__ __forceinline__ void wp_coords(const double *a, int x, int y, double &xx, double &yy)
{
    const double xin = x + 0.5, yin = y + 0.5;
    if (kPath == AEJ_WARP_QUAD) {
        xx = a[0] + a[1] * xin + a[2] * yin + a[3] * xin * yin;
        yy = a[4] + a[5] * xin + a[6] * yin + a[7] * xin * yin;
    } else {
        xx = a[0] * xin + a[1] * yin + a[2];
        yy = a[3] * xin + a[4] * yin + a[5];
        if (kPath == AEJ_WARP_PERSPECTIVE) {
            const double den = a[6] * xin + a[7] * yin + 1.0;
            xx = xx / den;
            yy = yy / den;
        }
    }
}

__device__ __forceinline__ double wp_cubic(double v1, double v2, double v3, double v4, double d)
{
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2.0 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

__device__ __forceinline__ int wp_clamp(int v, int hi) { return min(max(v, 0), hi); }

// one source row of the interpolation: kF == BILINEAR: v = p[x0] + (p[x1] - p[x0]) dx; BICUBIC: cub over columns x0 .. x0 + 3
template <int kC, int kF>
__device__ __forceinline__ void wp_row(const WpEntry &e, int x0, int y, double dx, bool premul, double *v)
{
    constexpr int kTaps = kF == AEJ_WARP_BILINEAR ? 2 : 4;
    int p[kTaps][kC];
    for (int k = 0; k < kTaps; k++) wp_pixel<kC>(e, wp_clamp(x0 + k, e.sw - 1), y, premul, p[k]);
    for (int c = 0; c < kC; c++) {
        if (kF == AEJ_WARP_BILINEAR)
            v[c] = (double)p[0][c] + (double)(p[1][c] - p[0][c]) * dx;
        else
            v[c] = wp_cubic((double)p[0][c], (double)p[1][c], (double)p[2][c], (double)p[3][c], dx);
    }
}

template <int kC, int kF, int kPath>
__global__ __launch_bounds__(kWpThreads) void k_warp(const WpEntry *__restrict__ entries, int n)
{
    const WpEntry &e = tile_entry(entries, n);
    const int tiles_x = (e.dw + kWpTileW - 1) / kWpTileW, local = (int)((long long)blockIdx.x - e.tile_base);
    const int x = (local % tiles_x) * kWpTileW + (int)(threadIdx.x % kWpTileW);
    const int y = (local / tiles_x) * kWpTileH + (int)(threadIdx.x / kWpTileW);
    if (x >= e.dw || y >= e.dh) return;
    const bool premul = (kC == 2 || kC == 4) && kF != AEJ_WARP_NEAREST && e.premul;
    int px[kC];
    bool inside;
    if (kF == AEJ_WARP_NEAREST) {
        long long xi, yi;
        if (kPath == AEJ_WARP_TABLES) {
            xi = e.tab[x];
            yi = e.tab[e.dw + y];
        } else if (kPath == AEJ_WARP_FIXED) {
            xi = (e.fx[2] + (long long)x * e.fx[0] + (long long)y * e.fx[1]) >> 16;
            yi = (e.fx[5] + (long long)x * e.fx[3] + (long long)y * e.fx[4]) >> 16;
        } else {
            double xx, yy;
            wp_coords<kPath>(e.a, x, y, xx, yy);
            const bool ok = xx >= 0.0 && xx < (double)e.sw && yy >= 0.0 && yy < (double)e.sh;      // false for a NaN
            xi = ok ? (long long)xx : -1;
            yi = ok ? (long long)yy : -1;
        }
        inside = xi >= 0 && xi < e.sw && yi >= 0 && yi < e.sh;
        if (inside) wp_pixel<kC>(e, (int)xi, (int)yi, false, px);
    } else {
        double xx, yy;
        wp_coords<kPath>(e.a, x, y, xx, yy);
        inside = xx >= 0.0 && xx < (double)e.sw && yy >= 0.0 && yy < (double)e.sh;      // false for a NaN
        if (inside) {
            xx -= 0.5;
            yy -= 0.5;
            int sx = (int)floor(xx), sy = (int)floor(yy);
            const double dx = xx - sx, dy = yy - sy;
            double v[kC];
            if (kF == AEJ_WARP_BILINEAR) {
                double v1[kC], v2[kC];
                wp_row<kC, kF>(e, sx, wp_clamp(sy, e.sh - 1), dx, premul, v1);
                if (sy + 1 >= 0 && sy + 1 < e.sh) {
                    wp_row<kC, kF>(e, sx, sy + 1, dx, premul, v2);
                } else {
                    for (int c = 0; c < kC; c++) v2[c] = v1[c];
                }
                for (int c = 0; c < kC; c++) {
                    v[c] = v1[c] + (v2[c] - v1[c]) * dy;
                    px[c] = (int)v[c];
                }
            } else {
                sx -= 1;
                sy -= 1;
                double r[4][kC];
                wp_row<kC, kF>(e, sx, wp_clamp(sy, e.sh - 1), dx, premul, r[0]);
                for (int k = 1; k < 4; k++) {
                    if (sy + k >= 0 && sy + k < e.sh) {
                        wp_row<kC, kF>(e, sx, sy + k, dx, premul, r[k]);
                    } else {
                        for (int c = 0; c < kC; c++) r[k][c] = r[k - 1][c];
                    }
                }
                for (int c = 0; c < kC; c++) {
                    v[c] = wp_cubic(r[0][c], r[1][c], r[2][c], r[3][c], dy);
                    px[c] = v[c] <= 0.0 ? 0 : v[c] >= 255.0 ? 255 : (int)v[c];
                }
            }
        }
    }
    if (!inside) {
        for (int c = 0; c < kC; c++) px[c] = e.fill[c];
    }
    if (premul) {
        const int alpha = px[kC - 1];
        if (alpha != 0 && alpha != 255) {
            for (int c = 0; c < kC - 1; c++) px[c] = min(255, (255 * px[c]) / alpha);
        }
    }
    unsigned char *o = e.out + ((long long)y * e.dw + x) * kC;
    if (kC == 4) {
        wp_store4(o, 4, (unsigned)px[0] | ((unsigned)px[1] << 8) | ((unsigned)px[2] << 16) | ((unsigned)px[3] << 24));
    } else {
        for (int c = 0; c < kC; c++) o[c] = (unsigned char)px[c];
    }
}

// ---- transpose ---------------------------------------------------------------------------------------------------------------------
// FLIP_LEFT_RIGHT (0), FLIP_TOP_BOTTOM (1), ROTATE_180 (3): the output has the source's size.  A workgroup owns kWpFlipBytes bytes of
// kWpFlipRows output rows; a lane gathers the 4 bytes of its dword from the mirrored pixels and stores them at once.
template <int kC>
__global__ __launch_bounds__(kWpThreads) void k_flip(const WpEntry *__restrict__ entries, int n)
{
    const WpEntry &e = tile_entry(entries, n);
    const int rb = e.dw * kC, tiles_x = (rb + kWpFlipBytes - 1) / kWpFlipBytes, local = (int)((long long)blockIdx.x - e.tile_base);
    const int b0 = (local % tiles_x) * kWpFlipBytes + (int)threadIdx.x * 4, y0 = (local / tiles_x) * kWpFlipRows;
    if (b0 >= rb) return;
    const int nb = min(4, rb - b0);
    const bool mx = e.method != 1, my = e.method != 0;
    for (int r = 0; r < kWpFlipRows && y0 + r < e.dh; r++) {
        const int y = y0 + r;
        const unsigned char *srow = e.in + (long long)(my ? e.dh - 1 - y : y) * rb;
        unsigned v = 0;
        if (!mx) {
            v = wp_load4(srow + b0, nb);
        } else {
            for (int b = 0; b < nb; b++) {
                const int o = b0 + b, p = o / kC, c = o - p * kC;
                v |= (unsigned)srow[(e.dw - 1 - p) * kC + c] << (8 * b);
            }
        }
        wp_store4(e.out + (long long)y * rb + b0, nb, v);
    }
}

// ROTATE_90 (2), ROTATE_270 (4), TRANSPOSE (5), TRANSVERSE (6): out(y, x) = in(row fx ? sh - 1 - x : x, column fy ? sw - 1 - y : y) with
// dw == sh and dh == sw.  The tw x th output tile at (X0, Y0) reads the th x tw source block at row r0, column c0: staged by rows,
// written by rows.  The LDS pitch is an odd number of dwords, so a column of the block meets every bank once.
template <int kC>
__global__ __launch_bounds__(kWpThreads) void k_transpose(const WpEntry *__restrict__ entries, int n)
{
    constexpr int kPitch = kWpSwapTile * kC + 4;
    __shared__ unsigned char lds[kWpSwapTile * kPitch];
    const WpEntry &e = tile_entry(entries, n);
    const int tiles_x = (e.dw + kWpSwapTile - 1) / kWpSwapTile, local = (int)((long long)blockIdx.x - e.tile_base);
    const int X0 = (local % tiles_x) * kWpSwapTile, Y0 = (local / tiles_x) * kWpSwapTile;
    const int tw = min(kWpSwapTile, e.dw - X0), th = min(kWpSwapTile, e.dh - Y0);
    const bool fx = e.method == 4 || e.method == 6, fy = e.method == 2 || e.method == 6;
    const int r0 = fx ? e.sh - X0 - tw : X0, c0 = fy ? e.sw - Y0 - th : Y0;
    const int nbi = th * kC;                  // bytes of a source row of the block
    for (int it = threadIdx.x; it < tw * nbi; it += kWpThreads) {
        const int row = it / nbi, b = it - row * nbi;
        lds[row * kPitch + b] = e.in[((long long)(r0 + row) * e.sw + c0) * kC + b];
    }
    __syncthreads();
    const int nbo = tw * kC;                  // bytes of an output row of the tile
    for (int it = threadIdx.x; it < th * nbo; it += kWpThreads) {
        const int oy = it / nbo, b = it - oy * nbo, ox = b / kC, c = b - ox * kC;
        const int lr = fx ? tw - 1 - ox : ox, lc = fy ? th - 1 - oy : oy;
        e.out[((long long)(Y0 + oy) * e.dw + X0) * kC + b] = lds[lr * kPitch + lc * kC + c];
    }
}

// ---- host: the plan of an image and of a call ---------------------------------------------------------------------------------------
static bool wp_fix(double v, long long &out)
{
    const double f = floor(v * 65536.0 + 0.5);
    if (!(fabs(f) < 2147483648.0)) return false;
    out = (long long)f;
    return true;
}

static bool wp_guard(const double *a, int x, int y)
{
    return fabs(x * a[0] + y * a[1] + a[2]) < 32768.0 && fabs(x * a[3] + y * a[4] + a[5]) < 32768.0;
}

static void wp_table(double step, double offset, int n, std::vector<int> &tab)
{
    double o = offset + step * 0.5;
    for (int i = 0; i < n; i++) {
        tab.push_back(o >= 0.0 && o < 2147483648.0 ? (int)o : -1);      // Pillow's COORD; beyond an int the entry is outside as well
        o += step;
    }
}

// what the library makes of one descriptor: -> 0, or the error code with *why the reason.  tables (may be NULL): the two tables of an
// AEJ_WARP_TABLES image are appended.
int warp_resolve(const aej_warp_desc &d, aej_warp_plan &p, std::vector<int> *tables, const char **why)
{
    memset(&p, 0, sizeof p);
    if (d.src_w < 1 || d.src_h < 1 || d.dst_w < 1 || d.dst_h < 1 || d.src_w > kWpMaxSide || d.src_h > kWpMaxSide || d.dst_w > kWpMaxSide || d.dst_h > kWpMaxSide) {
        *why = "sizes from 1 to 32767 a side";
        return AEJ_ERR_ARG;
    }
    if (d.channels < 1 || d.channels > 4) { *why = "1 to 4 channels"; return AEJ_ERR_ARG; }
    if (d.src_offset < 0 || d.dst_offset < 0) { *why = "negative offset"; return AEJ_ERR_ARG; }
    p.path = d.path;
    if (d.path == AEJ_WARP_TRANSPOSE) {
        if (d.method < 0 || d.method > 6) { *why = "unknown transpose method"; return AEJ_ERR_ARG; }
        const bool swap = d.method == 2 || d.method >= 4;
        if (d.dst_w != (swap ? d.src_h : d.src_w) || d.dst_h != (swap ? d.src_w : d.src_h)) { *why = "the output size is not the transposed source's"; return AEJ_ERR_ARG; }
        return 0;
    }
    if (d.path != AEJ_WARP_AFFINE && d.path != AEJ_WARP_PERSPECTIVE && d.path != AEJ_WARP_QUAD) { *why = "unknown path"; return AEJ_ERR_ARG; }
    if (d.filter != AEJ_WARP_NEAREST && d.filter != AEJ_WARP_BILINEAR && d.filter != AEJ_WARP_BICUBIC) { *why = "unknown filter"; return AEJ_ERR_ARG; }
    for (int k = 0; k < (d.path == AEJ_WARP_AFFINE ? 6 : 8); k++)
        if (!isfinite(d.coef[k])) { *why = "a coefficient that is not finite"; return AEJ_ERR_ARG; }
    p.premultiply = (d.channels == 2 || d.channels == 4) && d.filter != AEJ_WARP_NEAREST && d.premultiply != 0;
    if (d.path != AEJ_WARP_AFFINE || d.filter != AEJ_WARP_NEAREST) return 0;
    const double *a = d.coef;
    if (a[1] == 0 && a[3] == 0) {
        p.path = AEJ_WARP_TABLES;
        if (tables) {
            wp_table(a[0], a[2], d.dst_w, *tables);
            wp_table(a[4], a[5], d.dst_h, *tables);
        }
        return 0;
    }
    p.path = AEJ_WARP_FIXED;
    long long A[6];
    const bool fits = wp_guard(a, 0, 0) && wp_guard(a, d.dst_w, d.dst_h) && wp_guard(a, 0, d.dst_h) && wp_guard(a, d.dst_w, 0) &&
                      wp_fix(a[0], A[0]) && wp_fix(a[1], A[1]) && wp_fix(a[2] + a[0] * 0.5 + a[1] * 0.5, A[2]) &&
                      wp_fix(a[3], A[3]) && wp_fix(a[4], A[4]) && wp_fix(a[5] + a[3] * 0.5 + a[4] * 0.5, A[5]);
    if (!fits) { *why = "an affine transform under NEAREST beyond 16.16 fixed point (a coordinate of 32768 or more at a corner) is not built"; return AEJ_ERR_UNSUPPORTED; }
    for (int k = 0; k < 6; k++) p.fixed[k] = A[k];
    return 0;
}

static long long wp_tiles(const WpLaunch &l, const WpEntry &e)
{
    if (l.kernel == 1) return (long long)(((long long)e.dw * l.ch + kWpFlipBytes - 1) / kWpFlipBytes) * ((e.dh + kWpFlipRows - 1) / kWpFlipRows);
    if (l.kernel == 2) return (long long)((e.dw + kWpSwapTile - 1) / kWpSwapTile) * ((e.dh + kWpSwapTile - 1) / kWpSwapTile);
    return (long long)((e.dw + kWpTileW - 1) / kWpTileW) * ((e.dh + kWpTileH - 1) / kWpTileH);
}

// -> 0, or the error code with *bad the image and *why the reason
int warp_plan(const aej_warp_desc *descs, int n, WpPlan &plan, int *bad, const char **why)
{
    struct Key { int kernel, ch, filter, path; };
    std::vector<WpEntry> image(n);
    std::vector<Key> key(n);
    plan = WpPlan();
    for (int i = 0; i < n; i++) {
        const aej_warp_desc &d = descs[i];
        WpEntry &e = image[i];
        memset(&e, 0, sizeof e);
        *bad = i;
        aej_warp_plan p;
        e.tab_at = (int)plan.tables.size();
        const int code = warp_resolve(d, p, &plan.tables, why);
        if (code) return code;
        if (p.path != AEJ_WARP_TABLES) e.tab_at = -1;
        e.sw = d.src_w; e.sh = d.src_h; e.dw = d.dst_w; e.dh = d.dst_h;
        e.method = d.method;
        e.premul = p.premultiply;
        memcpy(e.fill, d.fill, 4);
        memcpy(e.a, d.coef, sizeof e.a);
        for (int k = 0; k < 6; k++) e.fx[k] = p.fixed[k];
        if (p.path == AEJ_WARP_TRANSPOSE)
            key[i] = { (d.method == 0 || d.method == 1 || d.method == 3) ? 1 : 2, d.channels, 0, 0 };
        else
            key[i] = { 0, d.channels, d.filter, p.path };
        plan.spans.reads.push_back({ i, d.src_offset, (long long)d.src_w * d.src_h * d.channels });
        plan.spans.writes.push_back({ i, d.dst_offset, (long long)d.dst_w * d.dst_h * d.channels });
    }
    *bad = -1;
    std::vector<char> done(n, 0);
    for (int i = 0; i < n; i++) {
        if (done[i]) continue;
        const Key k = key[i];
        WpLaunch l = { k.kernel, k.ch, k.filter, k.path, (int)plan.entries.size(), 0, 0 };
        for (int j = i; j < n; j++) {
            if (done[j] || key[j].kernel != k.kernel || key[j].ch != k.ch || key[j].filter != k.filter || key[j].path != k.path) continue;
            done[j] = 1;
            WpEntry e = image[j];
            e.tile_base = l.tiles;
            l.tiles += wp_tiles(l, e);
            plan.entries.push_back(e);
            plan.image.push_back(j);
        }
        l.count = (int)plan.entries.size() - l.first;
        if (l.tiles > 0x7fffffffLL) { *why = "more than 2^31 workgroups in one launch"; return AEJ_ERR_UNSUPPORTED; }
        plan.launches.push_back(l);
    }
    return 0;
}

// the upload of a call: the entries of every launch with their device pointers
void warp_blob(const WpPlan &plan, const unsigned char *src, unsigned char *dst, const int *tables_dev, std::vector<WpEntry> &blob)
{
    blob = plan.entries;
    for (size_t k = 0; k < blob.size(); k++) {
        blob[k].in = src + plan.spans.reads[plan.image[k]].offset;
        blob[k].out = dst + plan.spans.writes[plan.image[k]].offset;
        blob[k].tab = blob[k].tab_at >= 0 ? tables_dev + blob[k].tab_at : nullptr;
    }
}

template <int kC, int kF>
static void wp_launch_filter(hipStream_t st, const WpLaunch &l, const WpEntry *entries)
{
    const dim3 grid((unsigned)l.tiles), block(kWpThreads);
    if constexpr (kF == AEJ_WARP_NEAREST) {
        if (l.path == AEJ_WARP_TABLES) hipLaunchKernelGGL((k_warp<kC, AEJ_WARP_NEAREST, AEJ_WARP_TABLES>), grid, block, 0, st, entries, l.count);
        if (l.path == AEJ_WARP_FIXED) hipLaunchKernelGGL((k_warp<kC, AEJ_WARP_NEAREST, AEJ_WARP_FIXED>), grid, block, 0, st, entries, l.count);
    }
    if constexpr (kF != AEJ_WARP_NEAREST)
        if (l.path == AEJ_WARP_AFFINE) hipLaunchKernelGGL((k_warp<kC, kF, AEJ_WARP_AFFINE>), grid, block, 0, st, entries, l.count);
    if (l.path == AEJ_WARP_PERSPECTIVE) hipLaunchKernelGGL((k_warp<kC, kF, AEJ_WARP_PERSPECTIVE>), grid, block, 0, st, entries, l.count);
    if (l.path == AEJ_WARP_QUAD) hipLaunchKernelGGL((k_warp<kC, kF, AEJ_WARP_QUAD>), grid, block, 0, st, entries, l.count);
}

template <int kC>
static void wp_launch(hipStream_t st, const WpLaunch &l, const WpEntry *entries)
{
    const dim3 grid((unsigned)l.tiles), block(kWpThreads);
    if (l.kernel == 1) hipLaunchKernelGGL(k_flip<kC>, grid, block, 0, st, entries, l.count);
    if (l.kernel == 2) hipLaunchKernelGGL(k_transpose<kC>, grid, block, 0, st, entries, l.count);
    if (l.kernel != 0) return;
    if (l.filter == AEJ_WARP_NEAREST) wp_launch_filter<kC, AEJ_WARP_NEAREST>(st, l, entries);
    if (l.filter == AEJ_WARP_BILINEAR) wp_launch_filter<kC, AEJ_WARP_BILINEAR>(st, l, entries);
    if (l.filter == AEJ_WARP_BICUBIC) wp_launch_filter<kC, AEJ_WARP_BICUBIC>(st, l, entries);
}

hipError_t launch_warp(hipStream_t st, const WpPlan &plan, unsigned char *blob_dev, const WpEntry *blob_host, int *tables_dev)
{
    hipError_t e = hipMemcpyAsync(blob_dev, blob_host, plan.entries.size() * sizeof(WpEntry), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if (!plan.tables.empty()) {
        e = hipMemcpyAsync(tables_dev, plan.tables.data(), plan.tables.size() * sizeof(int), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    for (const WpLaunch &l : plan.launches) {
        const WpEntry *entries = (const WpEntry *)blob_dev + l.first;
        if (l.ch == 1) wp_launch<1>(st, l, entries);
        if (l.ch == 2) wp_launch<2>(st, l, entries);
        if (l.ch == 3) wp_launch<3>(st, l, entries);
        if (l.ch == 4) wp_launch<4>(st, l, entries);
    }
    return hipGetLastError();
}

}  // namespace aej
