// jfif_transform_core.h -- the lossless geometric transforms of a JPEG file's quantised coefficients (jpegtran's transupp.c restated):
// the output frame of a (source frame, transform, trim), output block -> source block, output natural index -> source natural index
// and sign, and which output blocks are dummies.  Host + device, so that aej_jfif_transform_coefs_host runs the code k_jt_transform
// (jfiftrans.hip) runs.
//
// Every transform is (T, MX, MY): with in' = T ? transposed source : source and (H', W') the output size,
//     out[y][x] = in'[MY ? H' - 1 - y : y][MX ? W' - 1 - x : x]
// none (0,0,0)  flip_h (0,1,0)  flip_v (0,0,1)  transpose (1,0,0)  transverse (1,1,1)  rot90 (1,1,0)  rot180 (0,1,1)  rot270 (1,0,1)
// (rot90 = transpose then flip_h, rot270 = flip_h then transpose, transverse = transpose then rot180; rotations are clockwise).
// On coefficients c(v, u), natural index 8 v + u: T reads c(u, v), MX multiplies by (-1)^u, MY by (-1)^v; on blocks: T swaps (by, bx),
// MX / MY reverse the block columns / rows of every component.  T swaps width and height and the luma sampling factors.  A mirrored
// OUTPUT axis must be a whole number of output MCUs (its reversal is then one of whole blocks for every component): jx_geom refuses
// the file (trim 0: jpegtran -perfect) or drops the partial MCUs at the right / bottom edge of that axis first (trim 1: -trim).
//
// Blocks are addressed in MCU order: MCU after MCU in raster order, inside an MCU the hs x vs luma blocks in raster order, then Cb, Cr.
// A luma block beyond the component's ceil(w / 8) x ceil(h / 8) real blocks is a dummy: it only fills out an edge MCU, and is written as
// libjpeg writes it (jctrans.c): AC zero, DC that of the block before it in the MCU.  The first block of an MCU and its chroma blocks are
// always real, so the walk back ends, and a real output block always maps to a real source block.
//
// A one-component (grey) file (JxGeom::nc = 1) is sampled 1 x 1 whatever its frame header says, its MCU is its one block and it has no
// dummies: the same mapping with hs = vs = 1 and no chroma blocks, so every transform is allowed and a mirrored axis is a multiple of 8.
//
// The cut (jpegtran -crop and -grayscale; k_jt_cut): a crop box (left, upper, right, lower), in the coordinates of the image after the
// transform and its trim, keeps [U, lower) x [L, right) of it, (L, U) being the box's corner moved up and left to the output's MCU grid:
// the output's MCU (mx, my) is MCU (mx + cx, my + cy) of the uncropped transform, whose own grid (tmcux, tmcuy) is what a mirror turns
// about.  The new right and bottom edges may cut through an MCU: dummy blocks as above.  A chroma drop writes a three-component source as
// a one-component file: snc = 3, nc = 1, the output sampled 1 x 1 as a grey file is, its blocks the source's REAL luma blocks, found in the
// source's three-component MCU order.  Every real output block is a real source block still: it lies left of `right` and above `lower`,
// which lie inside the (trimmed) transform, whose real blocks are real source blocks.
#pragma once
#include <stdint.h>

#ifndef AEJ_HD
#define AEJ_HD __host__ __device__
#endif

namespace aej {

enum { kJxNone = 0, kJxFlipH = 1, kJxFlipV = 2, kJxTranspose = 3, kJxTransverse = 4, kJxRot90 = 5, kJxRot180 = 6, kJxRot270 = 7 };      // jpegtran's JXFORM order
enum { kJxOk = 0, kJxNotPerfect = 1, kJxTrimsToZero = 2, kJxLayout = 3, kJxBadArg = 4, kJxCropRange = 5 };

struct JxGeom {                        // one file's transform (host-computed by jx_geom; the kernel reads nothing else)
    int xf, t, mx, my;                 // the code and its (T, MX, MY)
    int sW, sH, shs, svs, smcux, smcuy;      // source frame: size, luma sampling factors, MCU grid
    int oW, oH, ohs, ovs, omcux, omcuy;      // output frame
    int n_src, n_out;                  // blocks of the two MCU grids, dummies included
    int nc;                            // components of the output: 3, or 1
    // the cut (appended: what k_jt_transform reads keeps its place).  Without one: snc = nc, tmcu* = omcu*, cx = cy = cut = 0
    int snc;                           // components of the source: nc, or 3 over nc = 1 (a chroma drop)
    int tmcux, tmcuy;                  // MCU grid of the whole (trimmed) transform, in the output's MCUs: the grid a mirror turns about
    int cx, cy;                        // the output's first MCU in that grid (the crop's aligned corner)
    int cut;                           // a crop that is not the whole image, or a chroma drop: the mapping is run even for kJxNone
};

AEJ_HD inline bool jx_transposes(int xf) { return xf == kJxTranspose || xf == kJxTransverse || xf == kJxRot90 || xf == kJxRot270; }
AEJ_HD inline bool jx_mirrors_x(int xf) { return xf == kJxFlipH || xf == kJxTransverse || xf == kJxRot90 || xf == kJxRot180; }      // of the output
AEJ_HD inline bool jx_mirrors_y(int xf) { return xf == kJxFlipV || xf == kJxTransverse || xf == kJxRot180 || xf == kJxRot270; }

// -> kJxOk and g, or why not.  Sampling: 1x1, 2x1 or 2x2 luma over 1x1 chroma; a transposed 2x1 would be 1x2 (4:4:0): kJxLayout.
// allow440: 1x2 is a source layout too (it transposes to 2x1), and a transposed 2x1 is written as 1x2.
// box (NULL, or left, upper, right, lower; right == 0: none): the crop, in the trimmed transform's coordinates; 0 <= left < right <= its
// width and 0 <= upper < lower <= its height, or kJxCropRange -- nothing is clamped.  drop: a three-component source is written as a
// one-component file (a one-component source is that already), so that the MCU of every rule here is 8 x 8 and no layout is refused.
AEJ_HD inline int jx_geom(int H, int W, int hs, int vs, int xf, int trim, JxGeom &g, int nc = 3, bool allow440 = false, const int *box = nullptr,
                          bool drop = false)
{
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || xf < 0 || xf > 7 || (nc != 1 && nc != 3)) return kJxBadArg;
    if (nc == 1) hs = vs = 1;                                // the source's sampling factors mean nothing for one component
    g.snc = nc; g.nc = drop ? 1 : nc;
    if (!((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)) || (allow440 && hs == 1 && vs == 2))) return kJxBadArg;
    g.xf = xf; g.t = jx_transposes(xf); g.mx = jx_mirrors_x(xf); g.my = jx_mirrors_y(xf);
    if (g.t && hs != vs && !allow440 && g.nc == 3) return kJxLayout;
    g.sW = W; g.sH = H; g.shs = hs; g.svs = vs;
    g.smcux = (W + 8 * hs - 1) / (8 * hs); g.smcuy = (H + 8 * vs - 1) / (8 * vs);
    g.oW = g.t ? H : W; g.oH = g.t ? W : H; g.ohs = g.t ? vs : hs; g.ovs = g.t ? hs : vs;
    if (g.nc == 1) g.ohs = g.ovs = 1;
    const int mw = 8 * g.ohs, mh = 8 * g.ovs;
    if ((g.mx && g.oW % mw) || (g.my && g.oH % mh)) {
        if (!trim) return kJxNotPerfect;
        if (g.mx) g.oW = g.oW / mw * mw;
        if (g.my) g.oH = g.oH / mh * mh;
        if (g.oW < 1 || g.oH < 1) return kJxTrimsToZero;
    }
    g.tmcux = (g.oW + mw - 1) / mw; g.tmcuy = (g.oH + mh - 1) / mh;
    g.cx = g.cy = 0; g.cut = g.snc != g.nc;
    if (box && box[2] != 0) {
        if (box[0] < 0 || box[0] >= box[2] || box[2] > g.oW || box[1] < 0 || box[1] >= box[3] || box[3] > g.oH) return kJxCropRange;
        g.cx = box[0] / mw; g.cy = box[1] / mh;
        g.cut |= g.cx != 0 || g.cy != 0 || box[2] != g.oW || box[3] != g.oH;      // the whole image: no crop
        g.oW = box[2] - g.cx * mw; g.oH = box[3] - g.cy * mh;
    }
    g.omcux = (g.oW + mw - 1) / mw; g.omcuy = (g.oH + mh - 1) / mh;
    g.n_src = (hs * vs + nc - 1) * g.smcux * g.smcuy;        // <= 3 * 8192 * 8192: an int holds it
    g.n_out = (g.ohs * g.ovs + g.nc - 1) * g.omcux * g.omcuy;
    return kJxOk;
}

// Output block ob (in [0, n_out)) -> the source block its coefficients come from, in [0, n_src).  *dummy: ob is a dummy block; the
// block returned is then the source of the real block whose DC it repeats.  With the transform kJxNone this is the identity for the
// real blocks (the transcoder proper, which carries a source's dummy blocks as they are, does not come here).  cut (a constant at every
// call): g may hold a crop or a chroma drop (k_jt_cut); without it the fields of the cut are not read, and the code is what it was.
AEJ_HD inline int jx_source_block(const JxGeom &g, int ob, bool *dummy, bool cut = false)
{
    const int nl = g.ohs * g.ovs, bpm = nl + g.nc - 1, mcu = ob / bpm;
    int k = ob - mcu * bpm;
    const int my = mcu / g.omcux, mx = mcu - my * g.omcux;
    int by = my, bx = mx, ch = 1, cv = 1;                    // block coordinates in the component; its sampling factors
    *dummy = false;
    if (k < nl) {
        ch = g.ohs; cv = g.ovs;
        const int rbx = (g.oW + 7) >> 3, rby = (g.oH + 7) >> 3;      // real luma blocks
        for (;; k--) {
            const int ky = k / ch;
            by = my * cv + ky; bx = mx * ch + (k - ky * ch);
            if (bx < rbx && by < rby) break;                 // k == 0 always is
            *dummy = true;
        }
    }
    if (cut) { bx += g.cx * ch; by += g.cy * cv; }           // the block in the whole transform
    if (g.mx) bx = (cut ? g.tmcux : g.omcux) * ch - 1 - bx;  // in': the mirrored axes are whole MCUs
    if (g.my) by = (cut ? g.tmcuy : g.omcuy) * cv - 1 - by;
    const int sby = g.t ? bx : by, sbx = g.t ? by : bx;      // source block; the component's source sampling factors are (cv, ch) then
    int sh = g.t ? cv : ch, sv = g.t ? ch : cv;
    if (cut && k < nl) { sh = g.shs; sv = g.svs; }           // (after a chroma drop the output's factors are not the source's transposed)
    const int smy = sby / sv, smx = sbx / sh;
    const int sk = k < nl ? (sby - smy * sv) * sh + (sbx - smx * sh) : g.shs * g.svs + (k - nl);
    return (smy * g.smcux + smx) * (g.shs * g.svs + (cut ? g.snc : g.nc) - 1) + sk;
}

// Output natural index n = 8 v + u -> source natural index; *negate: the coefficient changes sign.
AEJ_HD inline int jx_source_index(const JxGeom &g, int n, bool *negate)
{
    const int v = n >> 3, u = n & 7;
    *negate = ((g.mx & u) ^ (g.my & v)) & 1;
    return g.t ? 8 * u + v : n;
}

}  // namespace aej
