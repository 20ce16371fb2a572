// filter.hip -- Pillow's BoxBlur, GaussianBlur and UnsharpMask on the device (aej_filter_*), bit for bit, over many packed 8-bit images
// of 1 to 4 channels, of different sizes and filters, in one call.  The three filters are one family (include/aej.h has the
// arithmetic): `passes` runs of one extended box blur per axis, each rounded to uint8, then the integer unsharp epilogue.  Sums are
// uint32 and order-free, so the kernels may add in any order; what they must keep is WHERE a pass reads: pass k reads pass k - 1 at
// in-image positions clamped to the image, never at a replicated extension of it.
//
// Two paths, both exact:
//   k_filter_tile<C>   one workgroup = one 64 x 32 output tile and its halo of passes * (r + 1) per axis in LDS, clamped only at the
//                      image border; every pass runs between two byte buffers in LDS, each over the range the later passes still
//                      need, and the epilogue reads the original tile kept beside them.  One read and one write of the image.
//   k_filter_rows<C>   one pass along rows for any r: a workgroup per (row, span of 512 pixels), a prefix sum of the span and its halo.
//   k_filter_cols      one pass along columns of the image taken as [h][w * channels] bytes: a lane owns 4 adjacent byte columns and
//                      walks a band of 128 rows down with running sums.  The last pass of an image applies the epilogue.
// A launch is one grid over every image that needs it (a per-image entry, a prefix sum of workgroups, a binary search by blockIdx.x,
// as resample.hip's).  Bounds: every source index is clamped to [0, N - 1] of its line before it is used, and a lane that owns fewer
// than 4 bytes at the end of a row reads and writes them one by one.
#include <math.h>
#include <string.h>

#include <vector>

#include "aej_ctx.h"

#pragma clang fp contract(off)

namespace aej {

// ---- host: the box radius of a Gaussian and the weights of a box radius (Pillow's BoxBlur.c, in its float32 steps) ----------------------
static float ft_gaussian_box(float radius)
{
    const int passes = 3;
    float sigma2 = radius * radius / passes;
    float L = (float)sqrt(12.0 * sigma2 + 1.0);
    float l = (float)floor((L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    return l + a;
}

int filter_weights(int kind, float xradius, float yradius, aej_filter_plan &p)
{
    memset(&p, 0, sizeof p);
    if (kind != AEJ_FILTER_BOX && kind != AEJ_FILTER_GAUSSIAN && kind != AEJ_FILTER_UNSHARP) return AEJ_ERR_ARG;
    if (!isfinite(xradius) || !isfinite(yradius) || xradius < 0 || yradius < 0) return AEJ_ERR_ARG;
    p.passes = kind == AEJ_FILTER_BOX ? 1 : 3;
    const float radius[2] = { xradius, yradius };
    for (int a = 0; a < 2; a++) {
        const float fr = kind == AEJ_FILTER_BOX ? radius[a] : ft_gaussian_box(radius[a]);
        if (!(fr < (float)(kFtMaxRadius + 1))) return AEJ_ERR_UNSUPPORTED;      // (a radius whose square overflows lands here too)
        p.box[a] = fr;
        p.r[a] = (int)fr;
        p.ww[a] = (uint32_t)((float)(1 << 24) / (fr * 2 + 1));
        p.fw[a] = ((uint32_t)(1 << 24) - (uint32_t)(p.r[a] * 2 + 1) * p.ww[a]) / 2;
    }
    return 0;
}

// ---- device: what the three kernels share ---------------------------------------------------------------------------------------------------
// Every factor is below 2^24 -- acc <= 255 * 2049, far <= 510, fw < 2^23, and ww < 2^24 for every radius but one so small that
// 2^24 / (2 fr + 1) rounds to 2^24, which filter_plan replaces (see kFtUnitWeight) --, so the products are the full-rate 24-bit ones.
__device__ __forceinline__ unsigned ft_box(unsigned acc, unsigned far, unsigned ww, unsigned fw)
{
    return (__umul24(acc, ww) + __umul24(far, fw) + (1u << 23)) >> 24;
}

__device__ __forceinline__ unsigned ft_unsharp(unsigned in, unsigned blur, int percent, int threshold)
{
    const int diff = (int)in - (int)blur;
    if (abs(diff) <= threshold) return in;
    return (unsigned)min(max((int)in + diff * percent / 100, 0), 255);
}

__device__ __forceinline__ unsigned ft_unsharp4(unsigned in, unsigned blur, int percent, int threshold)
{
    unsigned v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) v |= ft_unsharp((in >> (8 * b)) & 255u, (blur >> (8 * b)) & 255u, percent, threshold) << (8 * b);
    return v;
}

// nb (1 .. 4) bytes at any address, as the low bytes of a word; the address of a row of a packed image has no alignment
__device__ __forceinline__ unsigned ft_load4(const unsigned char *p, int nb)
{
    unsigned v = 0;
    if (nb == 4) {
        __builtin_memcpy(&v, p, 4);
    } else {
        for (int b = 0; b < nb; b++) v |= (unsigned)p[b] << (8 * b);
    }
    return v;
}

__device__ __forceinline__ void ft_store4(unsigned char *p, int nb, unsigned v)
{
    if (nb == 4) {
        __builtin_memcpy(p, &v, 4);
    } else {
        for (int b = 0; b < nb; b++) p[b] = (unsigned char)(v >> (8 * b));
    }
}

// ---- the fused tile kernel --------------------------------------------------------------------------------------------------------------------
// LDS: two buffers of RH rows of `pitch` bytes -- the tile and its halo, RW = 64 + 2 hx pixels by RH = 32 + 2 hy rows, behind `pad`
// bytes that put the tile's first byte on a dword --, then (unsharp only) the original tile.  Region positions outside the image are
// never written and never read: a pass clamps its indices to the region's part of the image [cx_lo, cx_hi] x [cy_lo, cy_hi].  Pass k of
// an axis computes the positions k * (r + 1) inside the region's border (and inside the image), which is what pass k + 1 reads for its
// own range; after the last one that is the tile.  The vertical passes only run on the tile's columns.
__host__ __device__ inline int ft_tile_pad(int hx, int ch) { return (4 - (hx * ch) % 4) % 4; }
__host__ __device__ inline int ft_tile_pitch(int hx, int ch) { return (ft_tile_pad(hx, ch) + (kFtTileW + 2 * hx) * ch + 3) & ~3; }

template <int kC>
__global__ __launch_bounds__(kFtThreads) void k_filter_tile(const FtEntry *__restrict__ entries, int n)
{
    extern __shared__ __align__(16) unsigned char ft_lds[];
    const FtEntry &e = tile_entry(entries, n);
    const int tiles_x = (e.w + kFtTileW - 1) / kFtTileW, local = (int)((long long)blockIdx.x - e.tile_base);
    const int X0 = (local % tiles_x) * kFtTileW, Y0 = (local / tiles_x) * kFtTileH;
    const int hx = e.hx, hy = e.hy, RW = kFtTileW + 2 * hx, RH = kFtTileH + 2 * hy;
    const int pad = ft_tile_pad(hx, kC), pitch = ft_tile_pitch(hx, kC);
    unsigned char *cur = ft_lds, *oth = cur + RH * pitch, *O = oth + RH * pitch;
    const int cx_lo = max(0, hx - X0), cx_hi = min(RW - 1, e.w - 1 - (X0 - hx));
    const int cy_lo = max(0, hy - Y0), cy_hi = min(RH - 1, e.h - 1 - (Y0 - hy));
    const int nrows = cy_hi - cy_lo + 1;
    const int tile_off = pad + hx * kC;               // of the tile's first byte in a region row: a multiple of 4
    constexpr int kND = kFtTileW * kC / 4;            // dwords of a tile row

    {   // the region's part of the image: a lane loads 4 bytes of a row
        const int nb_row = (cx_hi - cx_lo + 1) * kC, ndw = (nb_row + 3) >> 2;
        for (int it = threadIdx.x; it < nrows * ndw; it += kFtThreads) {
            const int row = it / ndw, d = it - row * ndw, ly = cy_lo + row, nb = min(4, nb_row - 4 * d);
            const unsigned v = ft_load4(e.in + ((long long)(Y0 - hy + ly) * e.w + (X0 - hx + cx_lo)) * kC + 4 * d, nb);
            unsigned char *s = cur + ly * pitch + pad + cx_lo * kC + 4 * d;
            for (int b = 0; b < nb; b++) s[b] = (unsigned char)(v >> (8 * b));
        }
    }
    __syncthreads();
    if (e.orig) {
        const int rows = min(kFtTileH, cy_hi + 1 - hy);
        for (int it = threadIdx.x; it < rows * kND; it += kFtThreads) {
            const int row = it / kND, d = it - row * kND;
            *(unsigned *)(O + row * (kFtTileW * kC) + 4 * d) = *(const unsigned *)(cur + (hy + row) * pitch + tile_off + 4 * d);
        }
        __syncthreads();
    }

    for (int k = 1; k <= e.nx; k++) {                 // horizontal: a lane slides one channel's window over kFtSeg pixels of a row
        const int r = e.rx, a = max(k * (r + 1), cx_lo), b = min(RW - k * (r + 1), cx_hi + 1);
        const int nseg = (b - a + kFtSeg - 1) / kFtSeg;
        for (int it = threadIdx.x; it < nrows * nseg * kC; it += kFtThreads) {
            const int c = it % kC, t = it / kC, seg = t % nseg, ly = cy_lo + t / nseg;
            const unsigned char *line = cur + ly * pitch + pad + c;
            unsigned char *out = oth + ly * pitch + pad + c;
            const int xa = a + seg * kFtSeg, xb = min(xa + kFtSeg, b);
            unsigned acc = 0;
            for (int j = -r; j <= r; j++) acc += line[min(max(xa + j, cx_lo), cx_hi) * kC];
            unsigned prev = line[min(max(xa - r - 1, cx_lo), cx_hi) * kC];
            for (int x = xa; x < xb; x++) {
                const unsigned next = line[min(x + r + 1, cx_hi) * kC], drop = line[max(x - r, cx_lo) * kC];
                out[x * kC] = (unsigned char)ft_box(acc, prev + next, e.wwx, e.fwx);
                acc += next - drop;
                prev = drop;
            }
        }
        __syncthreads();
        unsigned char *t = cur; cur = oth; oth = t;
    }

    for (int k = 1; k <= e.ny; k++) {                 // vertical: a lane owns a dword of the tile's columns and slides down kFtSeg rows
        const int r = e.ry, a = max(k * (r + 1), cy_lo), b = min(RH - k * (r + 1), cy_hi + 1);
        const int nseg = (b - a + kFtSeg - 1) / kFtSeg;
        for (int it = threadIdx.x; it < nseg * kND; it += kFtThreads) {
            const int d = it % kND, seg = it / kND;
            const unsigned char *col = cur + tile_off + 4 * d;
            unsigned char *out = oth + tile_off + 4 * d;
            const int ya = a + seg * kFtSeg, yb = min(ya + kFtSeg, b);
            unsigned acc[4] = { 0, 0, 0, 0 };
            for (int j = -r; j <= r; j++) {
                const unsigned v = *(const unsigned *)(col + min(max(ya + j, cy_lo), cy_hi) * pitch);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] += (v >> (8 * q)) & 255u;
            }
            unsigned prev = *(const unsigned *)(col + min(max(ya - r - 1, cy_lo), cy_hi) * pitch);
            for (int y = ya; y < yb; y++) {
                const unsigned next = *(const unsigned *)(col + min(y + r + 1, cy_hi) * pitch);
                const unsigned drop = *(const unsigned *)(col + max(y - r, cy_lo) * pitch);
                unsigned v = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const unsigned pq = (prev >> (8 * q)) & 255u, nq = (next >> (8 * q)) & 255u, dq = (drop >> (8 * q)) & 255u;
                    v |= ft_box(acc[q], pq + nq, e.wwy, e.fwy) << (8 * q);
                    acc[q] += nq - dq;
                }
                *(unsigned *)(out + y * pitch) = v;
                prev = drop;
            }
        }
        __syncthreads();
        unsigned char *t = cur; cur = oth; oth = t;
    }

    {   // the tile: a lane stores 4 bytes of a row
        const int rows = min(kFtTileH, cy_hi + 1 - hy), nb_row = min(kFtTileW, e.w - X0) * kC, ndw = (nb_row + 3) >> 2;
        for (int it = threadIdx.x; it < rows * ndw; it += kFtThreads) {
            const int row = it / ndw, d = it - row * ndw;
            unsigned v = *(const unsigned *)(cur + (hy + row) * pitch + tile_off + 4 * d);
            if (e.orig) v = ft_unsharp4(*(const unsigned *)(O + row * (kFtTileW * kC) + 4 * d), v, e.percent, e.threshold);
            ft_store4(e.out + ((long long)(Y0 + row) * e.w + X0) * kC + 4 * d, min(4, nb_row - 4 * d), v);
        }
    }
}

// ---- the pass kernels ---------------------------------------------------------------------------------------------------------------------------
// One horizontal pass.  Workgroup = one row and a span of at most kFtRowSpan pixels from x0.  LDS, in uint32: per channel the T = span
// + 2 r + 2 samples at x0 - r - 1 .. x0 + span + r (clamped to the row), turned into prefix sums in two levels -- every lane sums its own
// run of L samples in place, then the kFtPassThreads run totals are scanned -- so that P(j), the sum of samples 0 .. j, is the in-run
// sum plus the total of the runs before it.  Output o of the span then needs P at o - 1, o, o + 2 r + 1 and o + 2 r + 2.
template <int kC>
__global__ __launch_bounds__(kFtPassThreads) void k_filter_rows(const FtEntry *__restrict__ entries, int n)
{
    extern __shared__ __align__(16) unsigned char ft_lds[];
    const FtEntry &e = tile_entry(entries, n);
    const int spans = (e.w + kFtRowSpan - 1) / kFtRowSpan;
    const long long local = (long long)blockIdx.x - e.tile_base;
    const int y = (int)(local / spans), x0 = (int)(local - (long long)y * spans) * kFtRowSpan;
    const int span = min(kFtRowSpan, e.w - x0), r = e.rx, T = span + 2 * r + 2, L = (T + kFtPassThreads - 1) / kFtPassThreads;
    unsigned *S = (unsigned *)ft_lds, *part = S + kC * T;      // [kC][T], [kC][kFtPassThreads]
    const long long row = (long long)y * e.w * kC;
    const unsigned char *in = e.in + row;
    const int tid = threadIdx.x;

    for (int b = tid; b < T * kC; b += kFtPassThreads) {
        const int j = b / kC, c = b - j * kC, x = min(max(x0 - r - 1 + j, 0), e.w - 1);
        S[c * T + j] = in[x * kC + c];
    }
    __syncthreads();
    {
        const int j0 = min(tid * L, T), j1 = min(j0 + L, T);
#pragma unroll
        for (int c = 0; c < kC; c++) {
            unsigned sum = 0;
            for (int j = j0; j < j1; j++) {
                sum += S[c * T + j];
                S[c * T + j] = sum;
            }
            part[c * kFtPassThreads + tid] = sum;
        }
    }
    __syncthreads();
    for (int off = 1; off < kFtPassThreads; off <<= 1) {      // an inclusive scan of the run totals, every channel at once
        unsigned v[kC];
#pragma unroll
        for (int c = 0; c < kC; c++) v[c] = tid >= off ? part[c * kFtPassThreads + tid - off] : 0u;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < kC; c++) part[c * kFtPassThreads + tid] += v[c];
        __syncthreads();
    }
    auto P = [&](int c, int j) -> unsigned {          // j >= -1
        if (j < 0) return 0u;
        const int q = j / L;
        return S[c * T + j] + (q ? part[c * kFtPassThreads + q - 1] : 0u);
    };
    unsigned char *out = e.out + row;
    const unsigned char *orig = e.orig ? e.orig + row : nullptr;
    for (int b = tid; b < span * kC; b += kFtPassThreads) {
        const int o = b / kC, c = b - o * kC;
        const unsigned p0 = P(c, o - 1), p1 = P(c, o), p2 = P(c, o + 2 * r + 1), p3 = P(c, o + 2 * r + 2);
        unsigned v = ft_box(p2 - p1, (p1 - p0) + (p3 - p2), e.wwx, e.fwx);
        const int at = (x0 + o) * kC + c;
        if (orig) v = ft_unsharp(orig[at], v, e.percent, e.threshold);
        out[at] = (unsigned char)v;
    }
}

// One vertical pass over an image taken as [h][w] bytes (w = pixels * channels): workgroup = kFtColBytes byte columns and a band of at
// most kFtColBand rows, lane = 4 adjacent byte columns (fewer at the end of a row) with a running sum each.  The window of the band's
// first row is summed over the rows it really covers, the clamped ones counted, not read.
__global__ __launch_bounds__(kFtPassThreads) void k_filter_cols(const FtEntry *__restrict__ entries, int n)
{
    const FtEntry &e = tile_entry(entries, n);
    const int groups = (e.w + kFtColBytes - 1) / kFtColBytes;
    const long long local = (long long)blockIdx.x - e.tile_base;
    const int band = (int)(local / groups), b0 = ((int)(local - (long long)band * groups) * kFtPassThreads + (int)threadIdx.x) * 4;
    if (b0 >= e.w) return;
    const int nb = min(4, e.w - b0), r = e.ry, h = e.h;
    const int y0 = band * kFtColBand, y1 = min(y0 + kFtColBand, h);
    const unsigned char *in = e.in + b0;
    auto ld = [&](int y) -> unsigned { return ft_load4(in + (long long)min(max(y, 0), h - 1) * e.w, nb); };
    unsigned acc[4] = { 0, 0, 0, 0 };
    {
        const unsigned below = (unsigned)max(0, r - y0), above = (unsigned)max(0, y0 + r - (h - 1));      // window rows before row 0, after row h - 1
        const unsigned first = ld(0), last = ld(h - 1);
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = below * ((first >> (8 * q)) & 255u) + above * ((last >> (8 * q)) & 255u);
        for (int y = max(y0 - r, 0); y <= min(y0 + r, h - 1); y++) {
            const unsigned v = ld(y);
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] += (v >> (8 * q)) & 255u;
        }
    }
    unsigned prev = ld(y0 - r - 1);
    for (int y = y0; y < y1; y++) {
        const unsigned next = ld(y + r + 1), drop = ld(y - r);
        unsigned v = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned pq = (prev >> (8 * q)) & 255u, nq = (next >> (8 * q)) & 255u, dq = (drop >> (8 * q)) & 255u;
            v |= ft_box(acc[q], pq + nq, e.wwy, e.fwy) << (8 * q);
            acc[q] += nq - dq;
        }
        const long long at = (long long)y * e.w + b0;
        if (e.orig) v = ft_unsharp4(ft_load4(e.orig + at, nb), v, e.percent, e.threshold);
        ft_store4(e.out + at, nb, v);
        prev = drop;
    }
}

// ---- host: the plan of a call -------------------------------------------------------------------------------------------------------------------
// A pass whose ww is 2^24 has r = 0 and fw = 0 and copies: (p 2^24 + 2^23) >> 24 = p.  (p (2^24 - 1) + 2^23) >> 24 is p as well for
// p <= 255, and that factor fits the 24-bit multiply of ft_box.
constexpr unsigned kFtUnitWeight = (1u << 24) - 1;

static unsigned ft_tile_lds(const FtEntry &e, int ch, bool unsharp)
{
    return 2u * (unsigned)((kFtTileH + 2 * e.hy) * ft_tile_pitch(e.hx, ch)) + (unsharp ? (unsigned)(kFtTileH * kFtTileW * ch) : 0u);
}

// -> 0, or the error code with *bad the image and *why the reason.  Launch order: the fused tiles, then horizontal pass 0, 1, 2 and
// vertical pass 0, 1, 2 of the images on the pass path, so that an image's passes follow each other on the stream.
int filter_plan(const aej_filter_desc *descs, int n, int path, FtPlan &plan, int *bad, const char **why)
{
    struct Image { aej_filter_plan p; bool fused, unsharp; int nx, ny, stages; long long tmp; };
    std::vector<Image> images(n);
    plan = FtPlan();
    *bad = -1;
    if (path != AEJ_FILTER_AUTO && path != AEJ_FILTER_FUSED && path != AEJ_FILTER_PASSES) { *why = "unknown path"; return AEJ_ERR_ARG; }
    for (int i = 0; i < n; i++) {
        const aej_filter_desc &d = descs[i];
        Image &im = images[i];
        *bad = i;
        if (d.width < 1 || d.height < 1 || d.width > 65535 || d.height > 65535) { *why = "sizes from 1 to 65535 a side"; return AEJ_ERR_ARG; }
        if (d.channels < 1 || d.channels > 4) { *why = "1 to 4 channels"; return AEJ_ERR_ARG; }
        if (d.src_offset < 0 || d.dst_offset < 0) { *why = "negative offset"; return AEJ_ERR_ARG; }
        const int rc = filter_weights(d.kind, d.xradius, d.yradius, im.p);
        if (rc == AEJ_ERR_UNSUPPORTED) { *why = "box radius above 1024"; return rc; }
        if (rc) { *why = "unknown filter kind, or a radius that is negative or not finite"; return rc; }
        im.unsharp = d.kind == AEJ_FILTER_UNSHARP;
        if (im.unsharp && (d.percent > 1000000 || d.percent < -1000000)) { *why = "|percent| above 1000000"; return AEJ_ERR_UNSUPPORTED; }
        im.nx = im.p.box[0] != 0 ? im.p.passes : 0;
        im.ny = im.p.box[1] != 0 ? im.p.passes : 0;
        const int hx = im.nx * (im.p.r[0] + 1), hy = im.ny * (im.p.r[1] + 1);
        const bool fits = hx <= kFtHalo && hy <= kFtHalo;
        if (path == AEJ_FILTER_FUSED && !fits) { *why = "filter beyond the fused kernel's halo"; return AEJ_ERR_ARG; }
        im.fused = path != AEJ_FILTER_PASSES && fits;
        im.stages = std::max(1, im.nx + im.ny);      // (no pass at all: one identity pass copies)
        const long long bytes = (long long)d.width * d.height * d.channels;
        plan.spans.reads.push_back({ i, d.src_offset, bytes });
        plan.spans.writes.push_back({ i, d.dst_offset, bytes });
        im.tmp = plan.tmp_bytes;
        if (!im.fused) plan.tmp_bytes += align_up(bytes, 256) * std::min(2, im.stages - 1);
    }
    *bad = -1;
    auto entry = [&](int i) {
        const aej_filter_desc &d = descs[i];
        const Image &im = images[i];
        FtStage s;
        memset(&s, 0, sizeof s);
        s.e.w = d.width; s.e.h = d.height;
        s.e.rx = im.p.r[0]; s.e.wwx = im.p.ww[0]; s.e.fwx = im.p.fw[0];
        s.e.ry = im.p.r[1]; s.e.wwy = im.p.ww[1]; s.e.fwy = im.p.fw[1];
        if (s.e.wwx >> 24) s.e.wwx = kFtUnitWeight;
        if (s.e.wwy >> 24) s.e.wwy = kFtUnitWeight;
        s.e.percent = d.percent; s.e.threshold = d.threshold;
        s.in_off = d.src_offset; s.out_off = d.dst_offset; s.out_base = 1;
        s.orig_off = im.unsharp ? d.src_offset : -1;
        return s;
    };
    auto close = [&](FtLaunch &l) {
        l.count = (int)plan.stages.size() - l.first;
        if (l.count) plan.launches.push_back(l);
    };
    for (int ch = 1; ch <= 4; ch++) {
        FtLaunch l = { 0, ch, (int)plan.stages.size(), 0, 0, 0 };
        for (int i = 0; i < n; i++) {
            if (!images[i].fused || descs[i].channels != ch) continue;
            FtStage s = entry(i);
            s.e.nx = images[i].nx; s.e.ny = images[i].ny;
            s.e.hx = s.e.nx * (s.e.rx + 1); s.e.hy = s.e.ny * (s.e.ry + 1);
            s.e.tile_base = l.tiles;
            l.tiles += (long long)((s.e.w + kFtTileW - 1) / kFtTileW) * ((s.e.h + kFtTileH - 1) / kFtTileH);
            l.lds = std::max(l.lds, ft_tile_lds(s.e, ch, images[i].unsharp));
            plan.stages.push_back(s);
        }
        close(l);
    }
    // stage s of an image reads the source (s = 0) or buffer (s - 1) & 1 and writes the destination (the last) or buffer s & 1
    auto route = [&](FtStage &s, int i, int stage) {
        const Image &im = images[i];
        const long long buf = align_up(plan.spans.writes[i].bytes, 256);
        if (stage > 0) { s.in_base = 2; s.in_off = im.tmp + ((stage - 1) & 1) * buf; }
        if (stage < im.stages - 1) { s.out_base = 2; s.out_off = im.tmp + (stage & 1) * buf; s.orig_off = -1; }
    };
    for (int k = 0; k < 3; k++)
        for (int ch = 1; ch <= 4; ch++) {
            FtLaunch l = { 1, ch, (int)plan.stages.size(), 0, 0, 0 };
            for (int i = 0; i < n; i++) {
                if (images[i].fused || descs[i].channels != ch || images[i].nx <= k) continue;
                FtStage s = entry(i);
                route(s, i, k);
                s.e.tile_base = l.tiles;
                l.tiles += (long long)s.e.h * ((s.e.w + kFtRowSpan - 1) / kFtRowSpan);
                l.lds = std::max(l.lds, 4u * (unsigned)ch * (unsigned)(std::min(s.e.w, kFtRowSpan) + 2 * s.e.rx + 2 + kFtPassThreads));
                plan.stages.push_back(s);
            }
            close(l);
        }
    for (int k = 0; k < 3; k++) {
        FtLaunch l = { 2, 0, (int)plan.stages.size(), 0, 0, 0 };
        for (int i = 0; i < n; i++) {
            const Image &im = images[i];
            const bool copy = im.nx + im.ny == 0 && k == 0;
            if (im.fused || (im.ny <= k && !copy)) continue;
            FtStage s = entry(i);
            route(s, i, copy ? 0 : im.nx + k);
            if (copy) { s.e.ry = 0; s.e.wwy = kFtUnitWeight; s.e.fwy = 0; }
            s.e.w *= descs[i].channels;
            s.e.tile_base = l.tiles;
            l.tiles += (long long)((s.e.w + kFtColBytes - 1) / kFtColBytes) * ((s.e.h + kFtColBand - 1) / kFtColBand);
            plan.stages.push_back(s);
        }
        close(l);
    }
    for (const FtLaunch &l : plan.launches)
        if (l.tiles > 0x7fffffffLL) { *why = "more than 2^31 workgroups in one launch"; return AEJ_ERR_UNSUPPORTED; }
    return 0;
}

unsigned long long filter_carve(void *base, const FtPlan &plan, FtBufs &w)
{
    Carver c(base);
    w.blob = c.take<unsigned char>((long long)(plan.stages.size() * sizeof(FtEntry)));
    w.tmp = c.take<unsigned char>(plan.tmp_bytes);
    return c.bytes();
}

// the upload of a call: the entries of every launch with their device pointers
void filter_blob(const FtPlan &plan, const FtBufs &w, const unsigned char *src, unsigned char *dst, std::vector<FtEntry> &blob)
{
    blob.clear();
    for (const FtStage &s : plan.stages) {
        FtEntry e = s.e;
        e.in = (s.in_base == 2 ? w.tmp : src) + s.in_off;
        e.out = (s.out_base == 2 ? w.tmp : dst) + s.out_off;
        e.orig = s.orig_off >= 0 ? src + s.orig_off : nullptr;
        blob.push_back(e);
    }
}

hipError_t launch_filter(hipStream_t st, const FtPlan &plan, const FtBufs &w, const FtEntry *blob_host)
{
    hipError_t e = hipMemcpyAsync(w.blob, blob_host, plan.stages.size() * sizeof(FtEntry), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    for (const FtLaunch &l : plan.launches) {
        const FtEntry *entries = (const FtEntry *)w.blob + l.first;
        const dim3 grid((unsigned)l.tiles);
        if (l.kernel == 0) {
            if (l.ch == 1) hipLaunchKernelGGL(k_filter_tile<1>, grid, dim3(kFtThreads), l.lds, st, entries, l.count);
            if (l.ch == 2) hipLaunchKernelGGL(k_filter_tile<2>, grid, dim3(kFtThreads), l.lds, st, entries, l.count);
            if (l.ch == 3) hipLaunchKernelGGL(k_filter_tile<3>, grid, dim3(kFtThreads), l.lds, st, entries, l.count);
            if (l.ch == 4) hipLaunchKernelGGL(k_filter_tile<4>, grid, dim3(kFtThreads), l.lds, st, entries, l.count);
        } else if (l.kernel == 1) {
            if (l.ch == 1) hipLaunchKernelGGL(k_filter_rows<1>, grid, dim3(kFtPassThreads), l.lds, st, entries, l.count);
            if (l.ch == 2) hipLaunchKernelGGL(k_filter_rows<2>, grid, dim3(kFtPassThreads), l.lds, st, entries, l.count);
            if (l.ch == 3) hipLaunchKernelGGL(k_filter_rows<3>, grid, dim3(kFtPassThreads), l.lds, st, entries, l.count);
            if (l.ch == 4) hipLaunchKernelGGL(k_filter_rows<4>, grid, dim3(kFtPassThreads), l.lds, st, entries, l.count);
        } else {
            hipLaunchKernelGGL(k_filter_cols, grid, dim3(kFtPassThreads), 0, st, entries, l.count);
        }
    }
    return hipGetLastError();
}

}  // namespace aej
