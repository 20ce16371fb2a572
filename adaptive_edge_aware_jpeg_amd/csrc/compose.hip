// compose.hip -- Pillow's two-image operations on the device (aej_compose_*), bit for bit: Image.paste with every mask Pillow takes,
// Image.alpha_composite, Image.blend, Image.composite (a masked paste) and ImageChops, over many packed 8-bit elements of 1 to 4
// channels, of different sizes, channel counts, offsets and kinds, in one call.  include/aej.h has the arithmetic.
//
//   k_compose<C>   a workgroup takes a chunk of kCpChunk pixels of one OUTPUT image of C channels; a lane takes k_adjust_apply's group of
//                  16 / 8 / 4 / 4 adjacent pixels (16 bytes, 12 for RGB).  The element -- and with it the kind, the op and the mask kind
//                  -- is the same for the whole workgroup, so every dispatch below is a scalar branch.  A group that lies in one row
//                  and wholly outside the region copies the base: one vector load, one vector store.  A group in one row and wholly
//                  inside reads its overlay (and an L mask) pixels, which are adjacent too, with one vector access each at whatever
//                  address the offset leaves them -- the hardware splits a misaligned one.  Every other group -- one that straddles
//                  the region's left or right edge, the end of a row or the end of the image -- takes its pixels one by one, each with
//                  its own place and its own inside test; there is no byte loop over a row.
// An overlay shared by many elements is read through the caches; nothing is staged in LDS.  A launch is one grid over every element
// of one channel count (a per-element entry, a prefix sum of chunks, a binary search by chunk, as adjust.hip's); the grid is capped at
// kCpMaxGrid and the workgroups stride.  Bounds: a lane touches output pixel q only if q < npix, and overlay or mask pixel
// (x - ox, y - oy) only if (x, y) is in the region, which the host has clipped to the overlay's own rectangle.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "aej_ctx.h"

#pragma clang fp contract(off)

namespace aej {

template <int kC> struct CpLane { static constexpr int pix = kC == 1 ? 16 : kC == 2 ? 8 : 4; };

// kBytes adjacent bytes by one vector access
template <int kBytes> struct CpWords {
    unsigned w[kBytes / 4];
    __device__ __forceinline__ int at(int k) const { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }
};
template <int kBytes> __device__ __forceinline__ CpWords<kBytes> cp_load(const unsigned char *p)
{
    CpWords<kBytes> r;
    __builtin_memcpy(r.w, p, kBytes);
    return r;
}

__device__ __forceinline__ int cp_div255(int t) { return ((t >> 8) + t) >> 8; }

__device__ __forceinline__ int cp_chop(int op, int a, int b, float scale, float offset)
{
    int t;
    switch (op) {
    case AEJ_CHOP_ADD: t = (int)__fadd_rn(__fdiv_rn((float)(a + b), scale), offset); break;
    case AEJ_CHOP_SUBTRACT: t = (int)__fadd_rn(__fdiv_rn((float)(a - b), scale), offset); break;
    case AEJ_CHOP_MULTIPLY: t = a * b / 255; break;
    case AEJ_CHOP_SCREEN: t = 255 - (255 - a) * (255 - b) / 255; break;
    case AEJ_CHOP_LIGHTER: t = a > b ? a : b; break;
    case AEJ_CHOP_DARKER: t = a < b ? a : b; break;
    case AEJ_CHOP_DIFFERENCE: t = a > b ? a - b : b - a; break;
    case AEJ_CHOP_ADD_MODULO: return (a + b) & 255;
    case AEJ_CHOP_SUBTRACT_MODULO: return (a - b) & 255;
    case AEJ_CHOP_HARD_LIGHT: return (b < 128 ? a * b / 127 : 255 - (255 - b) * (255 - a) / 127) & 255;
    case AEJ_CHOP_OVERLAY: return (a < 128 ? a * b / 127 : 255 - (255 - a) * (255 - b) / 127) & 255;
    default: return (((255 - a) * (a * b)) / 65536 + (a * (255 - (255 - a) * (255 - b) / 255)) / 255) & 255;      // AEJ_CHOP_SOFT_LIGHT
    }
    return t <= 0 ? 0 : t >= 255 ? 255 : t;
}

// one pixel inside the region: d the base's, s the overlay's bands (the overlay's extra last band already dropped), m the mask's sample
template <int kC>
__device__ __forceinline__ void cp_pixel(const CpEntry &e, const int (&d)[kC], const int (&s)[kC], int m, int (&r)[kC])
{
    if (e.kind == AEJ_COMPOSE_PASTE) {
        if (e.mkind == AEJ_COMPOSE_MASK_NONE) {
#pragma unroll
            for (int b = 0; b < kC; b++) r[b] = s[b];
        } else if (e.mkind == AEJ_COMPOSE_MASK_BIT) {
#pragma unroll
            for (int b = 0; b < kC; b++) r[b] = m ? s[b] : d[b];
        } else {
            // Pillow's fill of a COLOUR through an L mask into an image with alpha: where the base is transparent and the mask is not 0,
            // the colour bands take the colour whole
            const bool fill = (kC == 2 || kC == 4) && !e.over && e.mkind == AEJ_COMPOSE_MASK_BYTE && e.mc == 1 && m != 0 && d[kC - 1] == 0;
#pragma unroll
            for (int b = 0; b < kC; b++) {
                const int mb = fill && b < kC - 1 ? 255 : m;
                r[b] = cp_div255(d[b] * (255 - mb) + s[b] * mb + 128);
            }
        }
    } else if (e.kind == AEJ_COMPOSE_ALPHA) {
        if constexpr (kC == 2 || kC == 4) {
            const unsigned sa = (unsigned)s[kC - 1], da = (unsigned)d[kC - 1];
            const unsigned outa = sa * 255u + da * (255u - sa);
            const int c1 = (int)((sa * 255u * 255u * 128u) / (outa ? outa : 1u));      // (outa is 0 only where sa is: those lanes keep d below)
            const int c2 = 255 * 128 - c1;
#pragma unroll
            for (int b = 0; b < kC - 1; b++) r[b] = sa ? cp_div255(s[b] * c1 + d[b] * c2 + (0x80 << 7)) >> 7 : d[b];
            r[kC - 1] = sa ? cp_div255((int)outa + 0x80) : d[kC - 1];
        } else {
#pragma unroll
            for (int b = 0; b < kC; b++) r[b] = d[b];
        }
    } else if (e.kind == AEJ_COMPOSE_BLEND) {
        const float a = e.alpha;
        const bool inside = a >= 0.f && a <= 1.f;
#pragma unroll
        for (int b = 0; b < kC; b++) r[b] = ad_blend(d[b], s[b], a, inside);
    } else {
#pragma unroll
        for (int b = 0; b < kC; b++) r[b] = cp_chop(e.op, d[b], s[b], e.scale, e.offset);
    }
}

// the overlay's and the mask's samples of kP adjacent pixels from pixel `at` of the overlay's own raster on, by vector accesses
template <int kC, int kOC, int kP>
__device__ __forceinline__ void cp_over_group(const CpEntry &e, long long at, int (&s)[kP][kC], int (&m)[kP])
{
    const CpWords<kP * kOC> w = cp_load<kP * kOC>(e.over + at * kOC);
#pragma unroll
    for (int i = 0; i < kP; i++) {
#pragma unroll
        for (int b = 0; b < kC; b++) s[i][b] = w.at(i * kOC + b);
        m[i] = w.at(i * kOC + kOC - 1);                        // AEJ_COMPOSE_MASK_OVERLAY's sample; any other kind replaces it
    }
}

template <int kC>
__global__ __launch_bounds__(kCpThreads) void k_compose(const CpEntry *__restrict__ entries, int n, long long chunks)
{
    constexpr int kP = CpLane<kC>::pix;
    constexpr int kWide = kC == 1 || kC == 3 ? kC + 1 : kC;    // the overlay with one band more: 2 over 1, 4 over 3
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const CpEntry &e = chunk_entry(entries, n, chunk);
        const int p0 = (int)(chunk - e.chunk_base) * kCpChunk;
        const bool masked = e.mkind == AEJ_COMPOSE_MASK_BIT || e.mkind == AEJ_COMPOSE_MASK_BYTE;
        for (int j = 0; j < kCpChunk / (kCpThreads * kP); j++) {
            const int q = p0 + (j * kCpThreads + (int)threadIdx.x) * kP;
            if (q >= e.npix) continue;
            const bool whole = q + kP <= e.npix;
            const int y = q / e.W, x = q - y * e.W;
            const bool row = whole && x + kP <= e.W;           // the group lies in one row of the output
            const bool rows_in = y >= e.ry0 && y < e.ry1;
            const bool all_in = row && rows_in && x >= e.rx0 && x + kP <= e.rx1;
            const bool all_out = row && (!rows_in || x + kP <= e.rx0 || x >= e.rx1);
            int d[kP][kC], s[kP][kC] = {}, m[kP] = {};
            bool in[kP];
            // ---- the base
            if ((whole && e.bw == e.W) || row) {
                const long long at = e.bw == e.W ? (long long)q : (long long)y * e.bw + x;
                const CpWords<kP * kC> w = cp_load<kP * kC>(e.base + at * kC);
#pragma unroll
                for (int i = 0; i < kP; i++)
#pragma unroll
                    for (int b = 0; b < kC; b++) d[i][b] = w.at(i * kC + b);
            } else {
                int xi = x, yi = y;
#pragma unroll
                for (int i = 0; i < kP; i++) {
                    const bool valid = q + i < e.npix;
                    const long long at = (long long)yi * e.bw + xi;
#pragma unroll
                    for (int b = 0; b < kC; b++) d[i][b] = valid ? (int)e.base[at * kC + b] : 0;
                    if (++xi == e.W) { xi = 0; yi++; }
                }
            }
            unsigned char *o = e.out + (long long)q * kC;
            if (!all_out) {
                // ---- the overlay and the mask
                if (all_in) {
                    const long long at = (long long)(y - e.oy) * e.ow + (x - e.ox);
                    if (!e.over) {
#pragma unroll
                        for (int i = 0; i < kP; i++)
#pragma unroll
                            for (int b = 0; b < kC; b++) s[i][b] = (int)e.colour[b];
                    } else if (e.oc == kC) {
                        cp_over_group<kC, kC, kP>(e, at, s, m);
                    } else {
                        cp_over_group<kC, kWide, kP>(e, at, s, m);
                    }
                    if (masked) {
                        if (e.mc == 1) {
                            const CpWords<kP> w = cp_load<kP>(e.mask + at);
#pragma unroll
                            for (int i = 0; i < kP; i++) m[i] = w.at(i);
                        } else {
#pragma unroll
                            for (int i = 0; i < kP; i++) m[i] = (int)e.mask[(at + i) * e.mc + e.mc - 1];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < kP; i++) in[i] = true;
                } else {
                    int xi = x, yi = y;
#pragma unroll
                    for (int i = 0; i < kP; i++) {
                        in[i] = q + i < e.npix && xi >= e.rx0 && xi < e.rx1 && yi >= e.ry0 && yi < e.ry1;
                        if (in[i]) {
                            const long long at = (long long)(yi - e.oy) * e.ow + (xi - e.ox);
#pragma unroll
                            for (int b = 0; b < kC; b++) s[i][b] = e.over ? (int)e.over[at * e.oc + b] : (int)e.colour[b];
                            if (e.mkind == AEJ_COMPOSE_MASK_OVERLAY) m[i] = (int)e.over[at * e.oc + e.oc - 1];
                            if (masked) m[i] = (int)e.mask[at * e.mc + e.mc - 1];
                        }
                        if (++xi == e.W) { xi = 0; yi++; }
                    }
                }
#pragma unroll
                for (int i = 0; i < kP; i++) {
                    int r[kC];
                    cp_pixel<kC>(e, d[i], s[i], m[i], r);
#pragma unroll
                    for (int b = 0; b < kC; b++) d[i][b] = in[i] ? r[b] : d[i][b];
                }
            }
            // ---- the output
            if (whole) {
                unsigned w[kP * kC / 4] = {};
#pragma unroll
                for (int i = 0; i < kP; i++)
#pragma unroll
                    for (int b = 0; b < kC; b++) {
                        const int at = i * kC + b;
                        w[at >> 2] |= (unsigned)(d[i][b] & 255) << (8 * (at & 3));
                    }
                __builtin_memcpy(o, w, kP * kC);
            } else {
#pragma unroll
                for (int i = 0; i < kP; i++)
#pragma unroll
                    for (int b = 0; b < kC; b++)
                        if (q + i < e.npix) o[i * kC + b] = (unsigned char)d[i][b];
            }
        }
    }
}

// ---- host: what one descriptor becomes, and the plan of a call ----------------------------------------------------------------------
static bool cp_side(int v) { return v >= 1 && v <= kCpMaxSide; }

int compose_resolve(const aej_compose_desc &d, aej_compose_plan &p, const char **why)
{
    memset(&p, 0, sizeof p);
    if (!cp_side(d.width) || !cp_side(d.height)) { *why = "sizes from 1 to 32767 a side"; return AEJ_ERR_ARG; }
    if (d.channels < 1 || d.channels > 4) { *why = "1 to 4 channels"; return AEJ_ERR_ARG; }
    if (d.base_offset < 0 || d.over_offset < 0 || d.mask_offset < 0 || d.dst_offset < 0) { *why = "negative offset"; return AEJ_ERR_ARG; }
    if (!cp_side(d.over_width) || !cp_side(d.over_height)) { *why = "overlay sizes from 1 to 32767 a side"; return AEJ_ERR_ARG; }
    const int C = d.channels, oc = d.over_channels, mk = d.mask_kind;
    if (mk < AEJ_COMPOSE_MASK_NONE || mk > AEJ_COMPOSE_MASK_OVERLAY) { *why = "unknown mask kind"; return AEJ_ERR_ARG; }
    if (d.kind == AEJ_COMPOSE_PASTE) {
        if (!(oc == 0 || oc == C || (C == 3 && oc == 4) || (C == 1 && oc == 2))) { *why = "a pair of channel counts that is not built"; return AEJ_ERR_ARG; }
        if (mk == AEJ_COMPOSE_MASK_OVERLAY && oc != 2 && oc != 4) { *why = "the overlay as its own mask needs 2 or 4 channels"; return AEJ_ERR_ARG; }
        if (mk == AEJ_COMPOSE_MASK_BIT || mk == AEJ_COMPOSE_MASK_BYTE) {
            const int mc = d.mask_channels;
            if (mk == AEJ_COMPOSE_MASK_BIT ? mc != 1 : (mc != 1 && mc != 2 && mc != 4)) { *why = "a mask of 1, 2 or 4 channels (a bit mask: 1)"; return AEJ_ERR_ARG; }
            if (oc == 0 && mc == 2) { *why = "a colour through a 2-channel mask (Pillow: bad transparency mask)"; return AEJ_ERR_ARG; }
            if (d.mask_width != d.over_width || d.mask_height != d.over_height) { *why = "a mask whose size is not the overlay's"; return AEJ_ERR_ARG; }
        }
    } else if (d.kind == AEJ_COMPOSE_ALPHA || d.kind == AEJ_COMPOSE_BLEND || d.kind == AEJ_COMPOSE_CHOP) {
        if (oc != C) { *why = "a pair of channel counts that is not built"; return AEJ_ERR_ARG; }
        if (mk != AEJ_COMPOSE_MASK_NONE) { *why = "a mask where only a paste takes one"; return AEJ_ERR_ARG; }
        if (d.kind == AEJ_COMPOSE_ALPHA && C != 2 && C != 4) { *why = "an alpha composite of images without alpha"; return AEJ_ERR_ARG; }
        if (d.kind != AEJ_COMPOSE_ALPHA && (d.x != 0 || d.y != 0)) { *why = "an offset where only a paste and an alpha composite take one"; return AEJ_ERR_ARG; }
        if (d.kind == AEJ_COMPOSE_BLEND) {
            if (d.over_width != d.width || d.over_height != d.height) { *why = "a blend of images of different sizes"; return AEJ_ERR_ARG; }
            if (!isfinite(d.alpha)) { *why = "an alpha that is not finite"; return AEJ_ERR_ARG; }
        }
        if (d.kind == AEJ_COMPOSE_CHOP) {
            if (d.op < AEJ_CHOP_ADD || d.op > AEJ_CHOP_OVERLAY) { *why = "unknown op"; return AEJ_ERR_ARG; }
            if ((d.op == AEJ_CHOP_ADD || d.op == AEJ_CHOP_SUBTRACT) && (!isfinite(d.scale) || !isfinite(d.offset) || d.scale == 0.f)) {
                *why = "a scale or offset that is not finite, or a scale of 0";
                return AEJ_ERR_ARG;
            }
        }
    } else {
        *why = "unknown kind";
        return AEJ_ERR_ARG;
    }
    if (d.box[0] > d.box[2] || d.box[1] > d.box[3]) { *why = "a box whose right or bottom lies before its left or top"; return AEJ_ERR_ARG; }
    const bool chop = d.kind == AEJ_COMPOSE_CHOP;
    p.out_width = chop ? std::min(d.width, d.over_width) : d.width;
    p.out_height = chop ? std::min(d.height, d.over_height) : d.height;
    p.out_channels = C;
    const long long x0 = std::max<long long>(0, (long long)d.x + std::max(d.box[0], 0)), x1 = std::min<long long>(p.out_width, (long long)d.x + std::min(d.box[2], d.over_width));
    const long long y0 = std::max<long long>(0, (long long)d.y + std::max(d.box[1], 0)), y1 = std::min<long long>(p.out_height, (long long)d.y + std::min(d.box[3], d.over_height));
    if (x0 < x1 && y0 < y1) {
        p.region[0] = (int)x0; p.region[1] = (int)y0; p.region[2] = (int)x1; p.region[3] = (int)y1;
        p.reads_overlay = oc > 0;
        p.reads_mask = mk == AEJ_COMPOSE_MASK_BIT || mk == AEJ_COMPOSE_MASK_BYTE;
    }
    return 0;
}

// -> 0, or the error code with *bad the element and *why the reason.  workspace NULL: everything but the device pointers, and plan.bytes.
int compose_plan(const aej_compose_desc *descs, int n, void *workspace, const unsigned char *src, unsigned char *dst, CpPlan &plan, int *bad,
                 const char **why)
{
    plan = CpPlan();
    std::vector<aej_compose_plan> cp(n);
    for (int i = 0; i < n; i++) {
        *bad = i;
        const int code = compose_resolve(descs[i], cp[i], why);
        if (code) return code;
        const aej_compose_desc &d = descs[i];
        const bool masked = d.mask_kind == AEJ_COMPOSE_MASK_BIT || d.mask_kind == AEJ_COMPOSE_MASK_BYTE;
        plan.spans.writes.push_back({ i, d.dst_offset, (long long)cp[i].out_width * cp[i].out_height * d.channels });
        plan.spans.reads.push_back({ i, d.base_offset, (long long)d.width * d.height * d.channels });
        if (d.over_channels > 0) plan.spans.reads.push_back({ i, d.over_offset, (long long)d.over_width * d.over_height * d.over_channels });
        if (masked) plan.spans.reads.push_back({ i, d.mask_offset, (long long)d.mask_width * d.mask_height * d.mask_channels });
    }
    *bad = -1;
    Carver cv(workspace);
    plan.entries_dev = cv.take<unsigned char>((long long)n * (long long)sizeof(CpEntry));
    for (int c = 1; c <= 4; c++) {
        CpLaunch l = { c, (int)plan.entries.size(), 0, 0 };
        for (int i = 0; i < n; i++) {
            const aej_compose_desc &d = descs[i];
            if (d.channels != c) continue;
            const bool masked = d.mask_kind == AEJ_COMPOSE_MASK_BIT || d.mask_kind == AEJ_COMPOSE_MASK_BYTE;
            CpEntry e;
            memset(&e, 0, sizeof e);
            e.base = src ? src + d.base_offset : nullptr;
            e.over = src && d.over_channels > 0 ? src + d.over_offset : nullptr;
            e.mask = src && masked ? src + d.mask_offset : nullptr;
            e.out = dst ? dst + d.dst_offset : nullptr;
            e.W = cp[i].out_width; e.npix = e.W * cp[i].out_height; e.bw = d.width;
            e.ox = d.x; e.oy = d.y; e.ow = d.over_width;
            e.rx0 = cp[i].region[0]; e.ry0 = cp[i].region[1]; e.rx1 = cp[i].region[2]; e.ry1 = cp[i].region[3];
            e.kind = d.kind; e.op = d.op; e.mkind = d.mask_kind; e.oc = d.over_channels; e.mc = masked ? d.mask_channels : 1;
            e.alpha = d.alpha; e.scale = d.scale; e.offset = d.offset;
            memcpy(e.colour, d.colour, 4);
            e.chunk_base = l.chunks;
            l.chunks += ((long long)e.npix + kCpChunk - 1) / kCpChunk;
            plan.entries.push_back(e);
        }
        l.count = (int)plan.entries.size() - l.first;
        if (l.count) plan.launches.push_back(l);
    }
    plan.bytes = cv.bytes();
    return 0;
}

// everything of a call on one stream: the upload and one launch per channel count.  The caller waits.
hipError_t launch_compose(hipStream_t st, const CpPlan &plan)
{
    hipError_t err = hipMemcpyAsync(plan.entries_dev, plan.entries.data(), plan.entries.size() * sizeof(CpEntry), hipMemcpyHostToDevice, st);
    if (err != hipSuccess) return err;
    for (const CpLaunch &l : plan.launches) {
        const CpEntry *entries = (const CpEntry *)plan.entries_dev + l.first;
        const dim3 grid((unsigned)std::min<long long>(l.chunks, kCpMaxGrid)), block(kCpThreads);
        if (l.channels == 1) hipLaunchKernelGGL(k_compose<1>, grid, block, 0, st, entries, l.count, l.chunks);
        if (l.channels == 2) hipLaunchKernelGGL(k_compose<2>, grid, block, 0, st, entries, l.count, l.chunks);
        if (l.channels == 3) hipLaunchKernelGGL(k_compose<3>, grid, block, 0, st, entries, l.count, l.chunks);
        if (l.channels == 4) hipLaunchKernelGGL(k_compose<4>, grid, block, 0, st, entries, l.count, l.chunks);
    }
    return hipGetLastError();
}

}  // namespace aej
