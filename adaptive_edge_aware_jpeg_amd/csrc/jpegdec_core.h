// jpegdec_core.h -- the per-thread work of jpegdec.hip's stages (aej_jpegdec_*), written as host + device functions so that the same
// decode can be stepped through on the CPU.  Everything here is bounded by the sizes it is given: the Huffman loop by its stop bit,
// every read by the file's clean stream (whose allocation carries 8 bytes of slack past the last byte a stop bit can reach).
#pragma once
#include <stdint.h>

#include "../../include/aej.h"
#include "aej_common.h"
#include "jfif_stream_core.h"

namespace aej {

constexpr int kJdChunk = 64;           // bytes per un-stuffing chunk
constexpr int kJdSyncBatch = 4;        // sync rounds launched between two read-backs of the "changed" word
constexpr int kJdLuma = 4;             // added to log2 of a file's scale: the luma plane alone, [oh][ow] (JdFile::shift)
constexpr int kJdBox = 8;              // added to a file's shift: only a box of it is reconstructed (k_jd_sbox; JdFile::box, ::win)
constexpr int kJdAdobe = 16;           // a four-component or RGB-coded file (aej_jpeg_adobe::colour): k_jd_idct<true> and k_jd_adobe alone reconstruct it
constexpr int kJdCmyk = 32;            // with kJdAdobe: the image leaves with four channels (Pillow's mode "CMYK"), not as RGB
constexpr int kJdAdobePx = 4;          // pixels one thread of k_jd_adobe reconstructs: 12 or 16 output bytes, whole dwords
constexpr int kJdBoxW = 128, kJdBoxH = 32;      // pixels of one tile of k_jd_sbox: a whole number of MCUs of every layout at every scale
constexpr int kJdSbox = 64;            // with kJdBox, on a file decoded at scale 2, 4 or 8: the box is in pixels of the scaled image

// per-file layout of one aej_jpegdec_batch (host-computed, uploaded with the descriptors)
struct JdFile {
    long long scan_off, scan_len;      // stuffed scan bytes in the caller's buffer
    long long clean_off;               // byte offset of the file's un-stuffed stream in the clean buffer (4-byte aligned)
    long long chunk_base, n_chunks;    // un-stuffing chunks
    long long seg_base;                // first restart segment (global index)
    long long slot_base, n_slots;      // subsequence slots (an upper bound: every segment's slots start at seg + start_bit / S)
    long long blk_base, n_blocks;      // coefficient blocks, MCU order
    long long plane_off;               // byte offset of the sample planes
    int pw0, ph0, pw1, ph1;            // luma and chroma plane shapes (whole MCUs)
    long long px_base;                 // first output pixel of the call's pixel range (a scaled file has none: k_jd_rgb never meets it)
    long long out_off;                 // byte offset of the RGB output
    int shift;                         // log2 of the decode scale: 0 full size (k_jd_idct, k_jd_rgb), 1..3 scale 2, 4, 8 (k_jd_scaled);
                                       // kJdLuma + 0..3: luma only at that scale (k_jd_luma; non-zero, so k_jd_idct leaves the file alone)
    int ow, oh;                        // output shape: ceil(width / scale), ceil(height / scale)
    long long grp_base[3];             // [shift - 1]: first workgroup of the file in k_jd_scaled<shift>'s grid (kJdRun MCUs of one MCU row each)
    long long grp440_base[3];          // the same in k_jd_scaled_h1v2<shift>'s grid, where the three-component 1 x 2 (4:4:0) files go
    long long grpl_base[4];            // [log2 scale]: the same in k_jd_luma's grid, where the luma-only files of every layout go
    int box[4];                        // a boxed file (shift & kJdBox): left, top, right, bottom in pixels of the image; ow, oh are the box's
    int win[4];                        // its MCU window mx0, my0, mx1, my1 (jd_sbox_window): the MCUs whose blocks the box's pixels read
    int row0;                          // first MCU row whose coefficients are stored (win[1] for a baseline file, 0 for a progressive
                                       // one): block b of MCU (my, mx) is blk_base + ((my - row0) * mcux + mx) * blocks_per_mcu + b
    long long grpa_base;               // first workgroup of the file in k_jd_adobe's grid (shift & kJdAdobe)
    long long grps_base[4];            // [log2 scale]: first workgroup of the file in k_jd_sbox<log2 scale>'s grid (shift & kJdBox; one tile of
                                       // kJdBoxW x kJdBoxH pixels each): box and win are in pixels and MCUs of the image at that scale, ow, oh the box's
    int pw3, ph3;                      // such a file's fourth plane (whole MCUs; behind the three others), 0 x 0 for three components
    int uniform;                       // a baseline file of three or four components that all decode under one DC and one AC table (what
                                       // libjpeg writes for CMYK and RGB, and what optimised tables of a flat YCbCr picture can be): its bits
                                       // say nothing about the block slot, which the kFour kernels -- run for every call with such a file --
                                       // take from the block counts instead of the predecessor's state (k_jd_sync4, k_jd_fix4, k_jd_write4)
};

// one restart segment: written by the un-stuffing scatter (start) and k_jd_segments (the rest)
struct JdSeg {
    long long start, nbytes;           // in the clean stream of its file
    long long slot_base;               // first slot, relative to the file's slot_base
    int n_sub;                         // subsequences (>= 1)
    int first_mcu, n_mcu;
};

struct JdSlots {
    unsigned long long *state, *used;     // exit state; the entry state it was decoded from
    int *cnt;                             // [slot][4]: blocks started, DC sums of components 0..2 (a kFour call: [slot][5], components 0..3)
    unsigned char *first;                 // the slot starts a segment
    long long *blk_pre;                   // exclusive prefix of blocks started within the segment
    int *dc_pre;                          // [slot][3] (a kFour call: [slot][4])
};

// decoder state at a symbol boundary, packed in one 64-bit word (so that a successor reads it whole):
// bits 0..5 zigzag index, 6..8 block slot in the MCU, 9 "no state" (the decode that would produce it stopped on an error), 10.. bit offset
// kFour (a call with a four-component file, whose MCU has up to 10 blocks): the block slot takes bits 6..9, the others move up one
template <bool kFour = false>
AEJ_HD inline unsigned long long jd_pack(long long pos, int k, int z, int err)
{
    constexpr int kb = kFour ? 4 : 3;
    return ((unsigned long long)pos << (7 + kb)) | ((unsigned long long)(err & 1) << (6 + kb)) | ((unsigned long long)(k & ((1 << kb) - 1)) << 6) |
           (unsigned long long)(z & 63);
}
template <bool kFour = false> AEJ_HD inline long long jd_pos(unsigned long long s) { return (long long)(s >> (kFour ? 11 : 10)); }
template <bool kFour = false> AEJ_HD inline int jd_k(unsigned long long s) { return (int)((s >> 6) & (kFour ? 15 : 7)); }
AEJ_HD inline int jd_z(unsigned long long s) { return (int)(s & 63); }
template <bool kFour = false> AEJ_HD inline int jd_err(unsigned long long s) { return (int)((s >> (kFour ? 10 : 9)) & 1); }

// big-endian bit window over a 4-byte-aligned byte stream
struct JdBits {
    const unsigned *w;
    long long cw;
    unsigned a, b;
    AEJ_HD explicit JdBits(const unsigned char *base) : w(reinterpret_cast<const unsigned *>(base)), cw(-2), a(0), b(0) {}      // -2: the first peek loads both words
    AEJ_HD inline unsigned peek32(long long pos)       // the 32 bits from bit `pos` on
    {
        const long long wi = pos >> 5;
        if (wi != cw) {
            if (wi == cw + 1) { a = b; b = js_bswap(w[wi + 1]); }
            else { a = js_bswap(w[wi]); b = js_bswap(w[wi + 1]); }
            cw = wi;
        }
        const int sh = (int)(pos & 31);
        return sh ? (a << sh) | (b >> (32 - sh)) : a;
    }
};

// The "& 255" below is defensive only and no test can tell it from its absence: a code that no entry of the 9-bit table matches and that is
// <= maxcode[l] is, by the canonical order of the codes, one of length l's own, so valoff[l] + code is its index in vals, 0 .. 255.
AEJ_HD inline bool jd_huff(const aej_jpegdec_huff &h, unsigned win, int &len, int &sym)
{
    const unsigned e = h.lut[win >> 23];
    if (e) { len = (int)(e >> 8); sym = (int)(e & 255); return true; }
    for (int l = 10; l <= 16; l++) {
        const int code = (int)(win >> (32 - l));
        if (code <= h.maxcode[l]) { len = l; sym = h.vals[(h.valoff[l] + code) & 255]; return true; }
    }
    return false;
}

// natural index of zigzag position z (z < 64)
AEJ_HD inline int jd_natural(int z) { return kZigzag8.natural[z]; }

AEJ_HD inline int jd_comp(const aej_jpegdec_desc &d, int k) { return d.ncomp == 1 ? 0 : (k < d.hs * d.vs ? 0 : k - d.hs * d.vs + 1); }

// the same in a kFour call, for every file of it: component 3's blocks follow the MCU's others (one component: hs = vs = 1, k = 0)
AEJ_HD inline int jd_comp4(const aej_jpegdec_desc &d, int k) { const int n0 = d.hs * d.vs; return k < n0 ? 0 : k - n0 < 2 ? k - n0 + 1 : 3; }

enum { kJdRunStop = 0, kJdRunOutOfBits = 1, kJdRunBadCode = 2, kJdRunPast63 = 3, kJdRunBadDc = 4, kJdRunDone = 5 };

// One Huffman symbol from the 32-bit window at a position that has `avail` (>= 1) bits left in its restart segment.  The window's bits
// from `avail` on are whatever follows the segment in memory -- the next segment, or bytes nobody wrote -- and must decide nothing: a code
// of at most `avail` bits is found whatever they hold (the table is a prefix code, shorter lengths are tried first); everything else --
// a match longer than `avail`, or no match while fewer than 16 bits are left -- is a segment that ends inside a code.  Without this rule a
// truncated file was "truncated scan" or "bad Huffman code" (or "DC category above 11") depending on the bytes behind its data.
AEJ_HD inline int jd_symbol(const aej_jpegdec_huff &h, unsigned win, long long avail, int &len, int &sym)
{
    if (!jd_huff(h, win, len, sym)) return avail < 16 ? kJdRunOutOfBits : kJdRunBadCode;
    return len > avail ? kJdRunOutOfBits : kJdRunStop;
}

// Decode symbols from state (pos, k, z) while pos < stop; no symbol may end past seg_end.  Counts the blocks started and sums their
// DC differences per component.  kWrite: also stores the coefficients (natural order) of blocks [0, seg_blocks) of the segment into
// coef (its block 0), with DC predictors pred[], `next` being the index of the next block to start; stops once every block is done.
// kWin (a boxed file): only blocks [win_lo, seg_blocks) of the segment are stored -- seg_blocks being where the file's coefficient window
// ends in the segment -- while the DC predictions are still tracked through the blocks before win_lo; kJdRunDone once block
// seg_blocks - 1 is complete.  coef + b * 64 is only formed for win_lo <= b < seg_blocks.
// dc and pred have one entry per component the call can meet: three, or with kFour (a call with a four-component file) four, and
// component 3 then decodes under x's tables (x: the file's
// aej_jpeg_adobe, only read for a block of component 3).
template <bool kWrite, bool kWin = false, bool kFour = false>
AEJ_HD inline int jd_run(const aej_jpegdec_desc &d, JdBits &br, long long &pos, int &k, int &z, long long stop, long long seg_end,
                         int &nstart, int *dc, short *coef, long long &next, long long seg_blocks, int *pred, long long win_lo = 0,
                         const aej_jpeg_adobe *x = nullptr)
{
    const int bpm = d.blocks_per_mcu;
    while (pos < stop) {
        if (kWrite && z == 0 && next >= seg_blocks) return kJdRunDone;
        const int c = kFour ? jd_comp4(d, k) : jd_comp(d, k);
        const aej_jpegdec_huff &h = kFour && c == 3 ? (z == 0 ? x->dc3 : x->ac3) : z == 0 ? d.dc[c] : d.ac[c];
        const unsigned win = br.peek32(pos);
        int len, sym;
        const int rc = jd_symbol(h, win, seg_end - pos, len, sym);
        if (rc != kJdRunStop) return rc;
        const int sz = z == 0 ? sym : (sym & 15);
        if (z == 0 && sym > 11) return kJdRunBadDc;
        if (pos + len + sz > seg_end) return kJdRunOutOfBits;
        int v = 0;
        if (sz) {
            const unsigned bits = (win << len) >> (32 - sz);
            v = bits < (1u << (sz - 1)) ? (int)bits - (1 << sz) + 1 : (int)bits;
        }
        pos += len + sz;
        if (z == 0) {
            nstart++;
            dc[c] += v;
            if (kWrite) {
                pred[c] += v;
                if (!kWin || next >= win_lo) coef[next * 64] = (short)pred[c];
                next++;
            }
            z = 1;
        } else {
            const int r = sym >> 4;
            if (sz) {
                if (z + r > 63) return kJdRunPast63;
                z += r;
                if (kWrite) {
                    const long long cur = next - 1;
                    if (cur >= (kWin ? win_lo : 0) && cur < seg_blocks) coef[cur * 64 + jd_natural(z)] = (short)v;
                }
                z++;
            } else if (r == 15) {
                if (z + 16 > 64) return kJdRunPast63;
                z += 16;
            } else {
                z = 64;
            }
        }
        if (z >= 64) {
            z = 0;
            k = k + 1 == bpm ? 0 : k + 1;
        }
    }
    return kJdRunStop;
}

// ---- reconstruction arithmetic (libjpeg-turbo's islow IDCT, range limit, fancy up-sampling, YCbCr -> RGB) ----------------------------
AEJ_HD inline long long jd_descale(long long x, int n) { return (x + (1LL << (n - 1))) >> n; }

template <bool kPass1>
AEJ_HD inline void jd_idct8(long long *d, int s)
{
    const int n = kPass1 ? 11 : 18;
    long long z2 = d[2 * s], z3 = d[6 * s], z1 = (z2 + z3) * 4433;
    long long t2 = z1 - z3 * 15137, t3 = z1 + z2 * 6270;
    long long t0 = (d[0] + d[4 * s]) * 8192, t1 = (d[0] - d[4 * s]) * 8192;
    long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7 * s]; t1 = d[5 * s]; t2 = d[3 * s]; t3 = d[s];
    z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
    long long z4 = t1 + t3, z5 = (z3 + z4) * 9633;
    t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    d[0] = jd_descale(t10 + t3, n); d[7 * s] = jd_descale(t10 - t3, n);
    d[s] = jd_descale(t11 + t2, n); d[6 * s] = jd_descale(t11 - t2, n);
    d[2 * s] = jd_descale(t12 + t1, n); d[5 * s] = jd_descale(t12 - t1, n);
    d[3 * s] = jd_descale(t13 + t0, n); d[4 * s] = jd_descale(t13 - t0, n);
}

// libjpeg's masked range-limit table (the C code's: jidctint.c after prepare_range_limit_table), which wraps modulo 1024.  Pillow runs
// libjpeg-turbo's SIMD inverse DCT, which saturates instead; the two agree while x stays in [-512, 511], which every block of real
// 8-bit samples does (the JPEG decode section, has the measured boundary).  Outside it this follows the C code, not Pillow.
AEJ_HD inline unsigned char jd_range_limit(long long x)
{
    const int m = (int)(x & 1023);
    return (unsigned char)(m < 128 ? m + 128 : m < 512 ? 255 : m < 896 ? 0 : m - 896);
}

// one block: coefficients (natural order) times the quantisers -> 8 x 8 samples at dst (row stride `stride`)
AEJ_HD inline __attribute__((always_inline)) void jd_idct_block(const short *c, const uint16_t *qt, unsigned char *dst, long long stride)
{
    long long d[64];
    for (int j = 0; j < 64; j++) d[j] = (long long)c[j] * qt[j];
    for (int col = 0; col < 8; col++) jd_idct8<true>(d + col, 8);
    for (int r = 0; r < 8; r++) jd_idct8<false>(d + r * 8, 1);
    for (int r = 0; r < 8; r++)
        for (int cc = 0; cc < 8; cc++) dst[r * stride + cc] = jd_range_limit(d[r * 8 + cc]);
}

// ---- reduced-size reconstruction (scale 2, 4, 8: libjpeg-turbo's jidctred.c, as Pillow's draft() selects it) ------------------------
// The two passes differ in width.  Pass 1 multiplies coefficient * quantiser products (|d| < 2^31) by constants whose absolute values
// sum to less than 2^17, so its sums need up to 48 bits: 64-bit arithmetic.  Of a pass-2 result only (x >> k) & 1023 with k <= 20
// survives jd_range_limit, i.e. the sum modulo 2^30.  The sum is an integer-linear form of the pass-1 results, so it is right modulo
// 2^32 when those are kept modulo 2^32 and the arithmetic wraps: pass 1 stores the low 32 bits, pass 2 runs in uint32.
AEJ_HD inline unsigned jd_descale_lo(long long x, int n) { return (unsigned)((x + (1LL << (n - 1))) >> n); }
AEJ_HD inline unsigned char jd_limit_u32(unsigned sum, int n) { return jd_range_limit((long long)((sum + (1u << (n - 1))) >> n)); }

// 4 x 4 samples of one block: row 4 and column 4 of the coefficients are never read
AEJ_HD inline void jd_idct4_block(const short *c, const uint16_t *qt, unsigned char *dst, long long stride)
{
    unsigned w[4][7];                                 // pass 1: columns 0..3, 5..7 (index 4..6)
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const int col = i < 4 ? i : i + 1;
        long long d[8];
#pragma unroll
        for (int r = 0; r < 8; r++) d[r] = r == 4 ? 0 : (long long)((int)c[r * 8 + col] * (int)qt[r * 8 + col]);
        const long long t0 = d[0] * 16384, t2 = d[2] * 15137 - d[6] * 6270, t10 = t0 + t2, t12 = t0 - t2;
        const long long o0 = -d[7] * 1730 + d[5] * 11893 - d[3] * 17799 + d[1] * 8697;
        const long long o2 = -d[7] * 4176 - d[5] * 4926 + d[3] * 7373 + d[1] * 20995;
        w[0][i] = jd_descale_lo(t10 + o2, 12); w[1][i] = jd_descale_lo(t12 + o0, 12);
        w[2][i] = jd_descale_lo(t12 - o0, 12); w[3][i] = jd_descale_lo(t10 - o2, 12);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {                     // pass 2: w[r][4..6] are columns 5..7
        const unsigned t0 = w[r][0] * 16384u, t2 = w[r][2] * 15137u - w[r][5] * 6270u, t10 = t0 + t2, t12 = t0 - t2;
        const unsigned o0 = w[r][4] * 11893u - w[r][6] * 1730u - w[r][3] * 17799u + w[r][1] * 8697u;
        const unsigned o2 = w[r][3] * 7373u - w[r][6] * 4176u - w[r][4] * 4926u + w[r][1] * 20995u;
        unsigned char *o = dst + r * stride;
        o[0] = jd_limit_u32(t10 + o2, 19); o[1] = jd_limit_u32(t12 + o0, 19);
        o[2] = jd_limit_u32(t12 - o0, 19); o[3] = jd_limit_u32(t10 - o2, 19);
    }
}

// 2 x 2 samples of one block: only rows and columns 0, 1, 3, 5, 7 are read
AEJ_HD inline void jd_idct2_block(const short *c, const uint16_t *qt, unsigned char *dst, long long stride)
{
    unsigned w[2][5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const int col = i < 2 ? i : 2 * i - 1;        // 0, 1, 3, 5, 7
        long long d[5];
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const int k = (j < 2 ? j : 2 * j - 1) * 8 + col;
            d[j] = (long long)((int)c[k] * (int)qt[k]);
        }
        const long long t10 = d[0] * 32768, t0 = -d[4] * 5906 + d[3] * 6967 - d[2] * 10426 + d[1] * 29692;
        w[0][i] = jd_descale_lo(t10 + t0, 13); w[1][i] = jd_descale_lo(t10 - t0, 13);
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const unsigned t10 = w[r][0] * 32768u, t0 = w[r][3] * 6967u - w[r][4] * 5906u - w[r][2] * 10426u + w[r][1] * 29692u;
        dst[r * stride] = jd_limit_u32(t10 + t0, 20);
        dst[r * stride + 1] = jd_limit_u32(t10 - t0, 20);
    }
}

// The 8 x 8 block behind a call.  jd_idct_block itself is always inlined, so that k_jd_idct compiles as it did when that was its
// only caller; inlined into k_jd_scaled<1> beside the 4 x 4 one it costs that kernel half its occupancy (measured on 64 4K 4:2:0
// files: 2.6 ms against 1.25 ms through this call).
AEJ_HD __attribute__((noinline)) inline void jd_idct_block_call(const short *c, const uint16_t *qt, unsigned char *dst, long long stride)
{
    jd_idct_block(c, qt, dst, stride);
}

// one block at IDCT size n (1, 2, 4 or 8): n x n samples at dst
AEJ_HD inline void jd_idct_sized(const short *c, const uint16_t *qt, int n, unsigned char *dst, long long stride)
{
    if (n == 8) jd_idct_block_call(c, qt, dst, stride);
    else if (n == 4) jd_idct4_block(c, qt, dst, stride);
    else if (n == 2) jd_idct2_block(c, qt, dst, stride);
    else dst[0] = jd_range_limit(jd_descale((long long)((int)c[0] * (int)qt[0]), 3));
}

// the IDCT size of a chroma component when luma is reconstructed at m = 8 / scale samples per block (libjpeg's
// jpeg_calc_output_dimensions with chroma sampled 1 x 1): 2m where the luma factors are 2 x 2 -- the chroma then comes out at luma
// resolution and is not up-sampled -- and m otherwise
AEJ_HD inline int jd_chroma_idct_size(int hs, int vs, int m)
{
    int n = m;
    while (n < 8 && (hs * m) % (n * 2) == 0 && (vs * m) % (n * 2) == 0) n *= 2;
    return n;
}

// ---- chroma up-sampling: libjpeg's rule, stated here once ----------------------------------------------------------------------------------
// A chroma component comes out of its IDCT (jd_chroma_idct_size) at 1 / uh of the output's width and 1 / uv of its height, uh and uv in
// 1, 2, and jdsample.c brings it to the output's size.  Along an axis with factor 1 the pixel reads the sample at its own place.  Along
// one with factor 2, pixel x reads sample x >> 1, and
//   plain replication   nothing else: beside a 1 x 1 IDCT (scale 8; `fancy` false -- jdmaster.c's use_merged_upsample / do_fancy test on
//                       the IDCT size), and in both directions where a column is up-sampled over a plane at most two samples wide;
//   "fancy"             3/4 of it and 1/4 of the neighbour the pixel lies nearer to -- x >> 1 - 1 for an even x, x >> 1 + 1 for an odd
//                       one -- with bias 1 (even) or 2 (odd) before >> 2: h2v1 along a row, h1v2 down a column.  h2v2 runs the vertical
//                       filter unrounded on both columns first (3 * near row + far row), then the horizontal one on those sums with bias
//                       8 (even) or 7 (odd) before >> 4.
// At the plane's edges the missing neighbour is the edge sample itself: (3 s + s + 1) >> 2 = (3 s + s + 2) >> 2 = s, which libjpeg writes
// as special cases of the first and last column (h2v1, h2v2: s, (4 cs + 8) >> 4, (4 cs + 7) >> 4) and as the edge row standing in for
// rows -1 and hc (h1v2, h2v2).  jd_up_far is that clamped neighbour, over the plane's REAL samples.

// the neighbour sample that output coordinate x of an axis up-sampled by 2 reads beside sample x >> 1, of n real samples
AEJ_HD inline int jd_up_far(int x, int n) { const int j = x >> 1; return (x & 1) ? (j + 1 < n ? j + 1 : n - 1) : (j > 0 ? j - 1 : 0); }

// What is still to up-sample after the chroma IDCT of a file decoded at scale 1 << shift: m = 8 >> shift luma samples per block side, the
// chroma IDCT size nc, the factors uh, uv that remain (2 x 2 luma at a scale: the chroma comes out of a 2m IDCT at luma resolution), fancy,
// and the real sample counts wc x hc of the chroma plane at that scale.  hs, vs: the luma factors, 1 x 1 for a file without chroma.
struct JdUp { int m, nc, uh, uv; bool fancy; int wc, hc; };
AEJ_HD inline JdUp jd_up_plan(int width, int height, int hs, int vs, int shift)
{
    JdUp u;
    u.m = 8 >> shift;
    u.nc = jd_chroma_idct_size(hs, vs, u.m);
    u.uh = hs * u.m / u.nc; u.uv = vs * u.m / u.nc;
    u.fancy = u.nc > 1;
    u.wc = (((width + (1 << shift) - 1) >> shift) + u.uh - 1) / u.uh;
    u.hc = (((height + (1 << shift) - 1) >> shift) + u.uv - 1) / u.uv;
    return u;
}
// plain replication in both directions?
AEJ_HD inline bool jd_up_replicates(int uh, bool fancy, int wc) { return !fancy || (uh == 2 && wc <= 2); }

// The chroma sample of output pixel (y, x), from a plane or a part of one with row stride W in which the file's sample (row, column) is
// p[row * W + column - off] (off: the index the part's first sample would have in the whole plane; 0 for a whole plane).  uh, uv, fancy,
// wc, hc as above; uh = uv = 2 without fancy does not occur.  Index arithmetic, not row pointers: a row's first samples may lie before
// the part.  Only the neighbour that the pixel's parity selects is read, a row clamped to the FILE's plane and a column not at all at
// the FILE's edges: the other one may lie outside the part (the boxed kernel and the halos of the scaled kernels hold exactly what
// jd_up_span says).  How the tests are spelt decides registers in k_jd_rgb: `fancy` first, on its own.
AEJ_HD inline int jd_up_chroma(const unsigned char *p, long long W, long long off, int uh, int uv, bool fancy, int wc, int hc, int y, int x)
{
    if (!fancy) return p[(uv == 2 ? y >> 1 : y) * W + (uh == 2 ? x >> 1 : x) - off];
    if (uh == 1) {
        if (uv == 1) return p[y * W + x - off];
        return (3 * p[(y >> 1) * W + x - off] + p[jd_up_far(y, hc) * W + x - off] + 1 + (y & 1)) >> 2;    // h1v2
    }
    const int j = x >> 1;
    if (wc <= 2) return p[(uv == 2 ? y >> 1 : y) * W + j - off];
    const int odd = x & 1, jn = odd ? j + 1 : j - 1;  // the nearer neighbour column
    const bool edge = odd ? j == wc - 1 : j == 0;     // it does not exist: the sample stands in for it, and it is not read
    if (uv == 1) {                                                                                        // h2v1
        const long long r0 = y * W - off;
        return edge ? p[r0 + j] : (3 * p[r0 + j] + p[r0 + jn] + 1 + odd) >> 2;
    }
    const long long r0 = (y >> 1) * W - off, r1 = jd_up_far(y, hc) * W - off;                             // h2v2
    const int cs = 3 * p[r0 + j] + p[r1 + j];
    return (3 * cs + (edge ? cs : 3 * p[r0 + jn] + p[r1 + jn]) + 8 - odd) >> 4;
}

// full size, a whole plane of wc x hc real samples (row stride `stride`); hs, vs: the luma sampling factors
AEJ_HD inline int jd_chroma(const unsigned char *p, long long stride, int hs, int vs, int wc, int hc, int y, int x)
{
    return jd_up_chroma(p, stride, 0, hs, vs, true, wc, hc, y, x);
}

// the samples s0..s1 that output coordinates a..b of one axis read (factor u, n real samples): the indices are monotonic in the
// coordinate, so the two ends decide
AEJ_HD inline void jd_up_span(int a, int b, int u, bool rep, int n, int &s0, int &s1)
{
    s0 = a; s1 = b;
    if (u != 2) return;
    s0 = a >> 1; s1 = b >> 1;
    if (rep) return;
    if (jd_up_far(a, n) < s0) s0 = jd_up_far(a, n);
    if (jd_up_far(b, n) > s1) s1 = jd_up_far(b, n);
}

// The MCU window of a box (l, t, r, b; 0 <= l < r, 0 <= t < b) in pixels of the image scaled by 1 << shift (0: full size), ceil(width >>
// shift) by ceil(height >> shift): win = mx0, my0, mx1, my1, the bounding rectangle of the MCUs that hold the luma samples of the box's
// pixels -- an MCU covers hs * m x vs * m of them -- and, unless luma_only or the file has one component, the chroma samples jd_up_chroma
// reads for them under the file's jd_up_plan (jd_up_span; chroma sample (i, j) lies in MCU (i / nc, j / nc)).  Exact.
AEJ_HD inline void jd_sbox_window(int width, int height, int hs, int vs, int ncomp, bool luma_only, int shift, const int *box, int *win)
{
    if (ncomp != 3) hs = vs = 1;
    const JdUp u = jd_up_plan(width, height, hs, vs, shift);
    const int l = box[0], t = box[1], r = box[2], b = box[3];
    win[0] = l / (hs * u.m); win[2] = (r - 1) / (hs * u.m) + 1;      // the luma samples: the pixels themselves
    win[1] = t / (vs * u.m); win[3] = (b - 1) / (vs * u.m) + 1;
    if (ncomp != 3 || luma_only) return;
    const bool rep = jd_up_replicates(u.uh, u.fancy, u.wc);
    int j0, j1, i0, i1;
    jd_up_span(l, r - 1, u.uh, rep, u.wc, j0, j1);
    jd_up_span(t, b - 1, u.uv, rep, u.hc, i0, i1);
    if (j0 / u.nc < win[0]) win[0] = j0 / u.nc;
    if (j1 / u.nc + 1 > win[2]) win[2] = j1 / u.nc + 1;
    if (i0 / u.nc < win[1]) win[1] = i0 / u.nc;
    if (i1 / u.nc + 1 > win[3]) win[3] = i1 / u.nc + 1;
}

AEJ_HD inline void jd_rgb(int Y, int cb, int cr, unsigned char *o)
{
    cb -= 128; cr -= 128;
    const int R = Y + ((91881 * cr + 32768) >> 16);
    const int G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    const int B = Y + ((116130 * cb + 32768) >> 16);
    o[0] = (unsigned char)(R < 0 ? 0 : R > 255 ? 255 : R);
    o[1] = (unsigned char)(G < 0 ? 0 : G > 255 ? 255 : G);
    o[2] = (unsigned char)(B < 0 ? 0 : B > 255 ? 255 : B);
}

// ---- the colour models that are not YCbCr (aej_jpeg_adobe::colour), per pixel, as Pillow returns them -------------------------------------
// s: the pixel's four samples after up-sampling -> Pillow's mode "CMYK" pixel.  CMYK: Pillow unpacks every four-component file as
// "CMYK;I", 255 - sample.  YCCK: libjpeg's ycck_cmyk_convert (255 - R, 255 - G, 255 - B of its YCbCr -> RGB, K as it is) and then that
// inversion: R, G, B and 255 - K.
AEJ_HD inline void jd_cmyk_pixel(const int *s, unsigned char *o)
{
    for (int c = 0; c < 4; c++) o[c] = (unsigned char)(255 - s[c]);
}
AEJ_HD inline void jd_ycck_pixel(const int *s, unsigned char *o)
{
    jd_rgb(s[0], s[1], s[2], o);
    o[3] = (unsigned char)(255 - s[3]);
}
// Pillow's MULDIV255 and its cmyk2rgb (Convert.c): a mode "CMYK" pixel -> RGB, in integers
AEJ_HD inline int jd_muldiv255(int a, int b) { const int t = a * b + 128; return ((t >> 8) + t) >> 8; }
AEJ_HD inline void jd_cmyk_rgb(const unsigned char *cmyk, unsigned char *o)
{
    const int nk = 255 - cmyk[3];
    for (int c = 0; c < 3; c++) {
        const int v = nk - jd_muldiv255(cmyk[c], nk);
        o[c] = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
}
// one pixel of a file with colour AEJ_JPEG_RGB / _CMYK / _YCCK from its samples s[0..3] (three components: s[3] unused): o gets 4
// channels when cmyk_out (four-component files alone), else 3
AEJ_HD inline void jd_adobe_pixel(int colour, bool cmyk_out, const int *s, unsigned char *o)
{
    if (colour == AEJ_JPEG_RGB) { o[0] = (unsigned char)s[0]; o[1] = (unsigned char)s[1]; o[2] = (unsigned char)s[2]; return; }
    unsigned char p[4];
    if (colour == AEJ_JPEG_YCCK) jd_ycck_pixel(s, p); else jd_cmyk_pixel(s, p);
    if (cmyk_out) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3]; }
    else jd_cmyk_rgb(p, o);
}

// un-stuffing: what byte p of a scan is (the neighbours decide: a run of 0xFF followed by 0x00 is one data 0xFF)
enum { kJdByteData = 0, kJdByteSkip = 1, kJdByteRst = 2, kJdByteEnd = 3 };
AEJ_HD inline int jd_byte_class(const unsigned char *s, long long n, long long p)
{
    const int b = s[p];
    if (b == 0xFF) return (p + 1 < n && s[p + 1] == 0x00) ? kJdByteData : kJdByteSkip;
    if (p > 0 && s[p - 1] == 0xFF) {
        if (b == 0x00) return kJdByteSkip;
        if (b >= 0xD0 && b <= 0xD7) return kJdByteRst;
        return kJdByteEnd;
    }
    return kJdByteData;
}

}  // namespace aej
