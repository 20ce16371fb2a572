// jfif_many_core.h -- the index mapping of the ragged JPEG encoder front end (jfifmany.hip): image size -> MCU grid -> block -> the
// pixel rectangle its samples come from, and which blocks are dummies; then one row of a block's level-shifted samples and the
// quantised block itself, over the arithmetic of jfif_arith.h.  Host + device, so that aej_jfif_many_coefs_host runs the code
// k_jm_coefs runs.
//
// Blocks are addressed in MCU order: MCU after MCU in raster order, inside an MCU the hs x vs luma blocks in raster order, then Cb, Cr.
// A luma block beyond the ceil(W / 8) x ceil(H / 8) real ones is a dummy: it only fills out an edge MCU, and libjpeg writes it with AC
// zero and the DC of the block before it in the MCU.  The first block of an MCU is always real, so the walk back ends.
// A grey image (JmGeom::nc = 1) is packed uint8 [H][W]: its one component is sampled 1 x 1, its blocks are the ceil(W / 8) x ceil(H / 8)
// real ones in raster order (an MCU is one block, none is a dummy), and the sample itself is Y: no colour conversion, no down-sampling.
// Bounds: every pixel jm_row reads has its row clamped to [0, H) and its column to [0, W), so it lies inside the image's 3 H W (grey: H W)
// bytes.
#pragma once
#include <stdint.h>
#include "aej_common.h"
#include "jfif_arith.h"

namespace aej {

struct JmGeom {                        // one image (host-computed by jm_geom; the kernel reads nothing else about its shape)
    int W, H, hs, vs;                  // size; luma sampling factors (chroma is 1 x 1)
    int mcux, mcuy, ybx, yby;          // MCU grid; real luma blocks per row / column
    int n_blocks, nc;                  // (hs vs + 2) mcux mcuy, dummies included (at most 3 * 8192 * 8192: an int holds it); components: 3, or 1
};
struct JmBlock {
    int comp;                          // 0 Y, 1 Cb, 2 Cr
    int bx, by;                        // the block of the component's grid whose samples are transformed: for a dummy, the real block whose DC it takes
    bool dummy;
};

// ss: Pillow's subsampling code (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)
AEJ_HD inline bool jm_geom(int H, int W, int ss, JmGeom &g, int nc = 3)
{
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || ss < 0 || ss > 2 || (nc != 1 && nc != 3)) return false;
    if (nc == 1) ss = 0;                                     // one component is sampled 1 x 1 whatever the call's subsampling
    g.W = W; g.H = H; g.hs = ss == 0 ? 1 : 2; g.vs = ss == 2 ? 2 : 1;
    g.mcux = (W + 8 * g.hs - 1) / (8 * g.hs); g.mcuy = (H + 8 * g.vs - 1) / (8 * g.vs);
    g.ybx = (W + 7) / 8; g.yby = (H + 7) / 8;
    g.n_blocks = (g.hs * g.vs + nc - 1) * g.mcux * g.mcuy;
    g.nc = nc;
    return true;
}

AEJ_HD inline JmBlock jm_block(const JmGeom &g, int b)      // b in [0, g.n_blocks)
{
    JmBlock r;
    r.dummy = false;
    if (g.nc == 1) { r.comp = 0; r.by = b / g.ybx; r.bx = b % g.ybx; return r; }
    const int nl = g.hs * g.vs, m = b / (nl + 2), my = m / g.mcux, mx = m % g.mcux;
    int k = b % (nl + 2);
    if (k >= nl) { r.comp = k - nl + 1; r.bx = mx; r.by = my; return r; }
    r.comp = 0;
    while (k > 0 && !(g.vs * my + k / g.hs < g.yby && g.hs * mx + k % g.hs < g.ybx)) { k--; r.dummy = true; }
    r.by = g.vs * my + k / g.hs; r.bx = g.hs * mx + k % g.hs;
    return r;
}

AEJ_HD __forceinline__ int jm_min(int a, int b) { return a < b ? a : b; }

// row r (0..7) of block b's samples minus 128: colour conversion, right and bottom edge replication, chroma down-sampling
AEJ_HD inline void jm_row(const unsigned char *img, const JmGeom &g, const JmBlock &b, int r, long long *d)
{
    const int W = g.W, H = g.H, comp = b.comp - 1;
    if (g.nc == 1) {                                         // grey: the sample is Y
        const unsigned char *row = img + (long long)jm_min(b.by * 8 + r, H - 1) * W;
        for (int c = 0; c < 8; c++) d[c] = row[jm_min(b.bx * 8 + c, W - 1)] - 128;
    } else if (b.comp == 0 || g.hs == 1) {                          // full-size plane: luma, or 4:4:4 chroma
        const unsigned char *row = img + (long long)jm_min(b.by * 8 + r, H - 1) * W * 3;
        for (int c = 0; c < 8; c++) {
            const unsigned char *p = row + jm_min(b.bx * 8 + c, W - 1) * 3;
            d[c] = (b.comp == 0 ? jf_y(p) : jf_c(p, comp)) - 128;
        }
    } else if (g.vs == 1) {                                  // 4:2:2
        const unsigned char *r0 = img + (long long)jm_min(b.by * 8 + r, H - 1) * W * 3;
        for (int c = 0; c < 8; c++) {
            const int cx = b.bx * 8 + c;
            d[c] = jf_h2v1(r0, jm_min(2 * cx, W - 1) * 3, jm_min(2 * cx + 1, W - 1) * 3, comp, cx) - 128;
        }
    } else {                                                 // 4:2:0
        const int cy = jm_min(b.by * 8 + r, (H + 1) / 2 - 1);
        const unsigned char *r0 = img + (long long)(2 * cy) * W * 3, *r1 = img + (long long)jm_min(2 * cy + 1, H - 1) * W * 3;
        for (int c = 0; c < 8; c++) {
            const int cx = b.bx * 8 + c;
            d[c] = jf_h2v2(r0, r1, jm_min(2 * cx, W - 1) * 3, jm_min(2 * cx + 1, W - 1) * 3, comp, cx) - 128;
        }
    }
}

// the coefficient at natural index n of block blk from the FDCT output c, as it is stored at zigzag position z under the quantiser
// qt (the component's table in zigzag order): a dummy keeps the DC alone
AEJ_HD __forceinline__ short jm_store(const JmBlock &blk, int n, long long c, int qt) { return blk.dummy && n != 0 ? (short)0 : (short)jf_quant((int)c, qt); }

// One whole block on one thread (the host entry): out[64] in zigzag order.  qt: [2][64] luma, chroma in zigzag order
AEJ_HD inline void jm_block_coefs(const unsigned char *img, const JmGeom &g, int b, const unsigned short *qt, short *out)
{
    const JmBlock blk = jm_block(g, b);
    long long d[64];
    for (int r = 0; r < 8; r++) {
        jm_row(img, g, blk, r, d + r * 8);
        jf_fdct8<true>(d + r * 8, 1);
    }
    for (int c = 0; c < 8; c++) jf_fdct8<false>(d + c, 8);
    for (int z = 0; z < 64; z++) {
        const int n = kZigzag8.natural[z];
        out[z] = jm_store(blk, n, d[n], qt[(blk.comp > 0) * 64 + z]);
    }
}

}  // namespace aej
