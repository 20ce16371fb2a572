// jfif.hip -- baseline JPEG as Pillow writes it with libjpeg-turbo (quality q, subsampling 4:2:0 / 4:2:2 / 4:4:4, the Annex K Huffman
// tables or with optimize=True the file's own, islow DCT; restart markers in the entropy chains, below) and the pixels Pillow's decoder returns for it (aej_jfif_*,
// include/aej.h).  The arithmetic restates libjpeg's published integer algorithm; tests/jfif_reference.py and
// tests/jfif_options_reference.py are the same algorithm in numpy and tests/test_gpu_jfif*.py pin both to Pillow's files byte for byte.
//
// Every kernel that walks blocks is a template over the luma sampling factors <HS, VS> (2 x 2, 2 x 1, 1 x 1; the entropy stages also
// <1, 2>, the 4:4:0 layout the transcoder and the transforms write): an MCU holds HS * VS luma blocks in raster order, then Cb, then Cr.  The entropy stages that walk blocks (k_jfif_hist, k_jfif_count, k_jfif_emit) also take the
// component count NC (3, or 1): a one-component (grey) file is <1, 1, 1>, its scan is not interleaved, so its MCU is one block, the blocks
// are the component's ceil(W / 8) x ceil(H / 8) in raster order and none is a dummy; it uses the luma tables (slots 0 and 1) alone, and
// k_jfif_tables / k_jfif_annexk leave the chroma slots of such a segment untouched (JfifGeom::ncomp).  Colour, DCT, quantisation and
// reconstruction (k_jfif_fdct, k_jfif_quant, k_jfif_idct, k_jfif_rgb) are three-component only: grey coefficients come from
// jfifmany.hip or jfiftrans.hip.
// Stages (one launch each, every quality of a call in the same launch after the first):
//   k_jfif_fdct     one thread per 8 x 8 block of one image: colour, edge padding, chroma down-sampling, islow FDCT -> int32 (zigzag order)
//   k_jfif_quant    one thread per (quality, image, block): quantise, resolve dummy blocks, count the block's Huffman bits (Annex K)
//   optimize only, between k_jfif_quant and the scan:
//   k_jfif_hist     one thread per block: the symbols the emitter will write, counted per wave in LDS, then one add per non-zero bin
//   k_jfif_tables   one workgroup per (quality, image), one wave per table: jh_build (jfif_huff_core.h), the codes, the file's markers
//   k_jfif_count    one thread per block: its bits under the file's own tables
//   k_js_scan       one workgroup per (quality, image): exclusive prefix sums of per-block bit counts (and later of per-chunk 0xFF
//                   counts), n + 1 entries whose last is the total -- jfif_stream_core.h, shared with jfifprog.hip
//   k_js_scan       restarts only (JfifGeom::R, jfif_restart_core.h): the byte starts of the restart intervals -- the same kernel over the
//                   intervals' byte lengths, ceil(bits / 8) each, read off the bit prefix sums (JfIntervalBytes)
//   k_jfif_emit     one thread per block: its code string at its bit offset, boundary words by atomicOr; the last block pads with 1-bits
//                   (with restarts: the offset is 8 x its interval's byte start + its bits inside the interval, the last block of every
//                   interval pads, and a block whose predecessor lies in an earlier interval predicts its DC from 0 -- as k_jfif_hist
//                   and k_jfif_count do)
//   k_jfif_ffcount  one thread per 64-byte chunk of a stream: its 0xFF bytes
//   k_jfif_layout   one thread: file lengths (markers + stuffed data + EOI) and their offsets in the packed output
//   k_jfif_scatter  one thread per chunk: the chunk with a 0x00 after every 0xFF at its final place; chunk 0 also writes markers and EOI;
//                   with restarts the chunk moves by 2 bytes per RSTn before it and writes those that fall inside it (jr_stuff_copy)
//   k_jfif_idct     one thread per (quality, image, real block): dequantise (its own load: zigzag order, int quantisers), then the
//                   decoder's islow IDCT pass and masked range limit (jd_idct8, jd_range_limit) -> uint8 sample planes
//   k_jfif_rgb      one thread per output pixel: h2v2 / h2v1 fancy up-sampling (plain replication when the chroma is <= 2 wide, as
//                   libjpeg-turbo does; none at 4:4:4) and the fixed-point YCbCr -> RGB -- jd_chroma, jd_rgb of jpegdec_core.h
// What a block gives the scan is written once, in jfif_prog_core.h: je_block_seq (the DC difference, the run-length walk of Annex F.1.2
// with its ZRL and EOB symbols) into a sink -- a histogram (k_jfif_hist), a bit count (k_jfif_quant, whose coefficient source quantises
// as the walk reads; k_jfif_count) or the bit writer (k_jfif_emit) -- and je_dc_pred, the DC predictor with its restart rule.  A block's
// place in its restart interval and the stuffing copy with markers are jfif_restart_core.h's (jr_place, jr_stuff_chunk), shared with
// jfifprog.hip.  jfif_seq_scan_host (aej_test_jfif_seq_scan_host) steps through all of these on the CPU.
// The bit writer (JeBits), magnitude category, predecessor block, 0xFF counting / stuffing loops and the prefix-sum kernel are
// jfif_stream_core.h's, the zigzag tables aej_common.h's (kZigzag8, k_zigzag8): one copy for every coder and decoder.
// Bounds: every index derives from JfifGeom; a stream's words stay inside its stride (the per-block bound kJfifBlockWords holds for every
// input: DC <= 22 bits, 63 AC <= 26 bits each; kJfifBlockWordsOpt with a file's own tables: DC <= 27, AC <= 26) and every store into
// a stream checks that stride; k_jfif_scatter writes a file only if it ends inside the caller's capacity.
#include "aej_common.h"
#include "aej_ctx.h"
#include "aej_launch.h"
#include "jfif_arith.h"
#include "jfif_huff_core.h"
#include "jfif_prog_core.h"
#include "jfif_restart_core.h"
#include "jfif_stream_core.h"
#include "jpegdec_core.h"

#include <vector>

namespace aej {

constexpr int kJfThreads = 256;
constexpr int kJfChunk = 64;           // bytes per stuffing chunk

// Annex K.3 Huffman codes, (code << 8) | length, indexed by symbol (0 = symbol not in the table)
// dc_luma: (code << 8) | length
__constant__ unsigned k_dc_luma[16] = {
    2, 515, 771, 1027, 1283, 1539, 3588, 7685, 15878, 32263, 65032, 130569, 0, 0, 0, 0};
// dc_chroma: (code << 8) | length
__constant__ unsigned k_dc_chroma[16] = {
    2, 258, 514, 1539, 3588, 7685, 15878, 32263, 65032, 130569, 261642, 523787, 0, 0, 0, 0};
// ac_luma: (code << 8) | length
__constant__ unsigned k_ac_luma[256] = {
    2564, 2, 258, 1027, 2820, 6661, 30727, 63496, 259594, 16744976, 16745232, 0, 0, 0, 0, 0,
    0, 3076, 6917, 30983, 128521, 521739, 16745488, 16745744, 16746000, 16746256, 16746512, 0, 0, 0, 0, 0,
    0, 7173, 63752, 259850, 1045516, 16746768, 16747024, 16747280, 16747536, 16747792, 16748048, 0, 0, 0, 0, 0,
    0, 14854, 128777, 1045772, 16748304, 16748560, 16748816, 16749072, 16749328, 16749584, 16749840, 0, 0, 0, 0, 0,
    0, 15110, 260106, 16750096, 16750352, 16750608, 16750864, 16751120, 16751376, 16751632, 16751888, 0, 0, 0, 0, 0,
    0, 31239, 521995, 16752144, 16752400, 16752656, 16752912, 16753168, 16753424, 16753680, 16753936, 0, 0, 0, 0, 0,
    0, 31495, 1046028, 16754192, 16754448, 16754704, 16754960, 16755216, 16755472, 16755728, 16755984, 0, 0, 0, 0, 0,
    0, 64008, 1046284, 16756240, 16756496, 16756752, 16757008, 16757264, 16757520, 16757776, 16758032, 0, 0, 0, 0, 0,
    0, 129033, 8372239, 16758288, 16758544, 16758800, 16759056, 16759312, 16759568, 16759824, 16760080, 0, 0, 0, 0, 0,
    0, 129289, 16760336, 16760592, 16760848, 16761104, 16761360, 16761616, 16761872, 16762128, 16762384, 0, 0, 0, 0, 0,
    0, 129545, 16762640, 16762896, 16763152, 16763408, 16763664, 16763920, 16764176, 16764432, 16764688, 0, 0, 0, 0, 0,
    0, 260362, 16764944, 16765200, 16765456, 16765712, 16765968, 16766224, 16766480, 16766736, 16766992, 0, 0, 0, 0, 0,
    0, 260618, 16767248, 16767504, 16767760, 16768016, 16768272, 16768528, 16768784, 16769040, 16769296, 0, 0, 0, 0, 0,
    0, 522251, 16769552, 16769808, 16770064, 16770320, 16770576, 16770832, 16771088, 16771344, 16771600, 0, 0, 0, 0, 0,
    0, 16771856, 16772112, 16772368, 16772624, 16772880, 16773136, 16773392, 16773648, 16773904, 16774160, 0, 0, 0, 0, 0,
    522507, 16774416, 16774672, 16774928, 16775184, 16775440, 16775696, 16775952, 16776208, 16776464, 16776720, 0, 0, 0, 0, 0};
// ac_chroma: (code << 8) | length
__constant__ unsigned k_ac_chroma[256] = {
    2, 258, 1027, 2564, 6149, 6405, 14342, 30727, 128009, 259594, 1045516, 0, 0, 0, 0, 0,
    0, 2820, 14598, 62984, 128265, 521739, 1045772, 16746512, 16746768, 16747024, 16747280, 0, 0, 0, 0, 0,
    0, 6661, 63240, 259850, 1046028, 8372751, 16747536, 16747792, 16748048, 16748304, 16748560, 0, 0, 0, 0, 0,
    0, 6917, 63496, 260106, 1046284, 16748816, 16749072, 16749328, 16749584, 16749840, 16750096, 0, 0, 0, 0, 0,
    0, 14854, 128521, 16750352, 16750608, 16750864, 16751120, 16751376, 16751632, 16751888, 16752144, 0, 0, 0, 0, 0,
    0, 15110, 260362, 16752400, 16752656, 16752912, 16753168, 16753424, 16753680, 16753936, 16754192, 0, 0, 0, 0, 0,
    0, 30983, 521995, 16754448, 16754704, 16754960, 16755216, 16755472, 16755728, 16755984, 16756240, 0, 0, 0, 0, 0,
    0, 31239, 522251, 16756496, 16756752, 16757008, 16757264, 16757520, 16757776, 16758032, 16758288, 0, 0, 0, 0, 0,
    0, 63752, 16758544, 16758800, 16759056, 16759312, 16759568, 16759824, 16760080, 16760336, 16760592, 0, 0, 0, 0, 0,
    0, 128777, 16760848, 16761104, 16761360, 16761616, 16761872, 16762128, 16762384, 16762640, 16762896, 0, 0, 0, 0, 0,
    0, 129033, 16763152, 16763408, 16763664, 16763920, 16764176, 16764432, 16764688, 16764944, 16765200, 0, 0, 0, 0, 0,
    0, 129289, 16765456, 16765712, 16765968, 16766224, 16766480, 16766736, 16766992, 16767248, 16767504, 0, 0, 0, 0, 0,
    0, 129545, 16767760, 16768016, 16768272, 16768528, 16768784, 16769040, 16769296, 16769552, 16769808, 0, 0, 0, 0, 0,
    0, 522507, 16770064, 16770320, 16770576, 16770832, 16771088, 16771344, 16771600, 16771856, 16772112, 0, 0, 0, 0, 0,
    0, 4186126, 16772368, 16772624, 16772880, 16773136, 16773392, 16773648, 16773904, 16774160, 16774416, 0, 0, 0, 0, 0,
    260618, 8373007, 16774672, 16774928, 16775184, 16775440, 16775696, 16775952, 16776208, 16776464, 16776720, 0, 0, 0, 0, 0};

// ---- arithmetic shared by the stages ----------------------------------------------------------------------------------------------
// jf_y, jf_c, jf_h2v1, jf_h2v2, jf_descale, jf_fdct8, jf_quant: jfif_arith.h (shared with jfifmany.hip); js_nbits, js_prev, JeBits,
// js_stuff_*, k_js_scan: jfif_stream_core.h, je_block_seq, je_dc_pred and the sinks: jfif_prog_core.h (shared with jfifprog.hip); jd_idct8, jd_range_limit, jd_chroma, jd_rgb: jpegdec_core.h

// MCU geometry: block k (0 .. HS * VS - 1 luma in raster order, then Cb, Cr) of MCU m; luma blocks outside ceil(H/8) x ceil(W/8) are
// dummies (right edge when HS = 2, bottom edge when VS = 2)
template <int HS, int VS>
__device__ __forceinline__ bool jf_real(const JfifGeom &g, long long m, int k)
{
    if (k >= HS * VS) return true;
    const int my = (int)(m / g.mcux), mx = (int)(m % g.mcux);
    return VS * my + k / HS < g.yby && HS * mx + k % HS < g.ybx;
}
// quantised DC of block k of MCU m under the quality's tables: a dummy takes the DC of the block before it in the MCU (block 0 is real)
template <int HS, int VS>
__device__ __forceinline__ int jf_qdc(const JfifGeom &g, const int *dct_img, const JfifParams &p, long long m, int k)
{
    while (!jf_real<HS, VS>(g, m, k)) k--;
    return jf_quant(dct_img[(m * (HS * VS + 2) + k) * 64], p.qt[k >= HS * VS][0]);
}
// ---- encode ------------------------------------------------------------------------------------------------------------------------
template <int HS, int VS>
__global__ __launch_bounds__(kJfThreads) void k_jfif_fdct(JfifGeom g, const unsigned char *__restrict__ rgb, int *__restrict__ dct)
{
    constexpr int NL = HS * VS, BPM = NL + 2;
    const long long idx = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    if (idx >= (long long)g.B * g.nblk) return;
    const int b = (int)(idx / g.nblk);
    const long long blk = idx % g.nblk, m = blk / BPM;
    const int k = (int)(blk % BPM), my = (int)(m / g.mcux), mx = (int)(m % g.mcux);
    const unsigned char *img = rgb + (long long)b * g.H * g.W * 3;
    long long d[64];
    if (k < NL) {
        const int by = VS * my + k / HS, bx = HS * mx + k % HS;
        if (by >= g.yby || bx >= g.ybx) return;          // dummy: never read
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int py = min(by * 8 + r, g.H - 1);
#pragma unroll
            for (int c = 0; c < 8; c++) d[r * 8 + c] = jf_y(img + ((long long)py * g.W + min(bx * 8 + c, g.W - 1)) * 3) - 128;
        }
    } else if (HS == 1) {                                    // 4:4:4: full-size chroma, edges replicated
        const int comp = k - NL;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int py = min(my * 8 + r, g.H - 1);
#pragma unroll
            for (int c = 0; c < 8; c++) d[r * 8 + c] = jf_c(img + ((long long)py * g.W + min(mx * 8 + c, g.W - 1)) * 3, comp) - 128;
        }
    } else if (VS == 1) {                                    // 4:2:2: h2v1_downsample, bias 0, 1, 0, 1, ... from column 0
        const int comp = k - NL;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const unsigned char *r0 = img + (long long)min(my * 8 + r, g.H - 1) * g.W * 3;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int cx = mx * 8 + c, x0 = min(2 * cx, g.W - 1) * 3, x1 = min(2 * cx + 1, g.W - 1) * 3;
                d[r * 8 + c] = jf_h2v1(r0, x0, x1, comp, cx) - 128;
            }
        }
    } else {                                                 // 4:2:0: h2v2_downsample
        const int comp = k - NL, hc = (g.H + 1) / 2;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int cy = min(my * 8 + r, hc - 1), y0 = 2 * cy, y1 = min(2 * cy + 1, g.H - 1);
            const unsigned char *r0 = img + (long long)y0 * g.W * 3, *r1 = img + (long long)y1 * g.W * 3;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int cx = mx * 8 + c, x0 = min(2 * cx, g.W - 1) * 3, x1 = min(2 * cx + 1, g.W - 1) * 3;
                d[r * 8 + c] = jf_h2v2(r0, r1, x0, x1, comp, cx) - 128;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; r++) jf_fdct8<true>(d + r * 8, 1);
#pragma unroll
    for (int c = 0; c < 8; c++) jf_fdct8<false>(d + c, 8);
    int *o = dct + idx * 64;
#pragma unroll
    for (int i = 0; i < 64; i++) o[i] = (int)d[i];
}

struct JfCodes { const unsigned *dc, *ac; };
__device__ __forceinline__ JfCodes jf_codes(bool chroma) { return chroma ? JfCodes{ k_dc_chroma, k_ac_chroma } : JfCodes{ k_dc_luma, k_ac_luma }; }
// a file's own tables: [seg][DC luma, AC luma, DC chroma, AC chroma][256]
__device__ __forceinline__ JfCodes jf_file_codes(const unsigned *codes, long long seg, bool chroma)
{
    const unsigned *t = codes + (seg * 4 + (chroma ? 2 : 0)) * 256;
    return JfCodes{ t, t + 256 };
}

// k_jfif_quant's coefficient sources for je_block_seq, which reads every index once, in increasing order: JfQuantSrc quantises
// coefficient i of the block d (FDCT output, natural order) with qt[i] as it is read and stores it to o[i]; a dummy block has no AC
struct JfQuantSrc {
    const int *d, *qt;
    short *o;
    __device__ __forceinline__ int operator[](int i) const
    {
        const int v = jf_quant(d[k_zigzag8.natural[i]], qt[i]);
        o[i] = (short)v;
        return v;
    }
};
struct JfNoAc {
    __device__ __forceinline__ int operator[](int) const { return 0; }
};

// (a) quantise every block of every (quality, image) and count its Huffman bits
template <int HS, int VS>
__global__ __launch_bounds__(kJfThreads) void k_jfif_quant(JfifGeom g, const JfifParams *__restrict__ par, const int *__restrict__ dct,
                                                           short *__restrict__ coef, int *__restrict__ lens)
{
    constexpr int NL = HS * VS, BPM = NL + 2;
    const long long idx = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    if (idx >= (long long)g.nq * g.B * g.nblk) return;
    const long long seg = idx / g.nblk, blk = idx % g.nblk, m = blk / BPM;
    const int k = (int)(blk % BPM), b = (int)(seg % g.B);
    const JfifParams &p = par[seg / g.B];
    const int *qt = p.qt[k >= NL];
    const int *img = dct + (long long)b * g.nblk * 64;
    const JfCodes hc = jf_codes(k >= NL);
    short *o = coef + idx * 64;
    const int dc = jf_qdc<HS, VS>(g, img, p, m, k);
    const long long pb = js_prev(NL, BPM, m, k);
    const int pred = pb < 0 ? 0 : jf_qdc<HS, VS>(g, img, p, pb / BPM, (int)(pb % BPM));      // (this chain has no restart intervals)
    JeLen sink{ nullptr, 0 };
    o[0] = (short)dc;
    if (!jf_real<HS, VS>(g, m, k)) {
        for (int i = 1; i < 64; i++) o[i] = 0;
        je_block_seq(dc, pred, JfNoAc{}, hc.dc, hc.ac, sink);
        lens[idx] = sink.total;
        return;
    }
    je_block_seq(dc, pred, JfQuantSrc{ img + blk * 64, qt, o }, hc.dc, hc.ac, sink);
    lens[idx] = sink.total;
}

// ---- optimize: the file's own Huffman tables -----------------------------------------------------------------------------------------
// (a1) the symbols k_jfif_emit will write for every block, dummies included (je_block_seq into a histogram).
// grid (blocks of one segment, segment); counts are private to a wave in LDS, then one 64-bit add per non-zero bin.
template <int HS, int VS, int NC>
__global__ __launch_bounds__(kJfThreads) void k_jfif_hist(JfifGeom g, const short *__restrict__ coef, unsigned long long *__restrict__ hist)
{
    constexpr int NL = HS * VS, BPM = NL + NC - 1, kWaves = kJfThreads / 64, kTables = NC == 1 ? 2 : 4;
    __shared__ unsigned cnt[kWaves][4][kJhSymbols];
    for (int i = threadIdx.x; i < kWaves * 4 * kJhSymbols; i += kJfThreads) (&cnt[0][0][0])[i] = 0;
    __syncthreads();
    const long long seg = blockIdx.y, blk = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    if (blk < g.nblk) {
        const long long m = blk / BPM;
        const int k = (int)(blk % BPM);
        unsigned(*h)[kJhSymbols] = cnt[threadIdx.x / 64] + (k >= NL ? 2 : 0);      // [0] DC, [1] AC of the block's component class
        const short *base = coef + seg * g.nblk * 64, *c = base + blk * 64;
        JeHist<unsigned> sink{ nullptr };
        je_block_seq(c[0], je_dc_pred(base, NL, BPM, m, k, g.R), c, h[0], h[1], sink);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTables * kJhSymbols; i += kJfThreads) {
        unsigned n = 0;
        for (int w = 0; w < kWaves; w++) n += (&cnt[w][0][0])[i];
        if (n) atomicAdd(hist + seg * 4 * kJhSymbols + i, (unsigned long long)n);
    }
}

// (a2) one workgroup per (quality, image), one wave per table (DC luma, AC luma, DC chroma, AC chroma): the table (jh_build, serial on
// the wave's first lane with its work arrays in LDS), its codes, and the file's markers: those of its quality with these four DHTs.
// A one-component file has the two luma tables alone: the chroma waves only keep the barriers, and the SOS it ends with is shorter
__global__ __launch_bounds__(kJfThreads) void k_jfif_tables(JfifGeom g, const JfifParams *__restrict__ par, const unsigned long long *__restrict__ hist,
                                                            unsigned *__restrict__ codes, unsigned char *__restrict__ fhdr, int *__restrict__ fhdr_len)
{
    static_assert(kJfThreads == 4 * 64, "one wave per table");
    __shared__ JhWork work[4];
    __shared__ unsigned char bits[4][16], vals[4][256];
    __shared__ int nsym[4];
    const long long seg = blockIdx.x;
    const int t = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ntab = g.ncomp == 1 ? 2 : 4, sos = jfif_sos_bytes(g.ncomp == 1 ? 1 : 3), dri = g.R ? kJrDriBytes : 0;      // the DRI: between the DHTs and the SOS
    const bool mine = t < ntab;                              // uniform over the wave
    unsigned *tc = codes + (seg * 4 + t) * 256;
    for (int i = lane; mine && i < 256; i += 64) {
        work[t].freq[i] = (long long)hist[(seg * 4 + t) * kJhSymbols + i];
        tc[i] = 0;
    }
    __syncthreads();
    if (mine && lane == 0) nsym[t] = jh_build(work[t], bits[t], vals[t]);
    __syncthreads();
    if (mine && lane == 0) jh_codes(bits[t], vals[t], tc);
    const JfifParams &p = par[seg / g.B];
    unsigned char *o = fhdr + seg * kJfifHdrMax;
    for (int i = threadIdx.x; i < p.dht_off; i += kJfThreads) o[i] = p.hdr[i];
    int off = p.dht_off, end = p.dht_off;
    for (int u = 0; u < ntab; u++) {
        if (u < t) off += 5 + 16 + nsym[u];
        end += 5 + 16 + nsym[u];
    }
    if (end + dri + sos <= kJfifHdrMax) {                    // always: at most 12 DC and 162 AC symbols, the Annex K sizes
        if (mine) {
            const int n = nsym[t];
            if (lane == 0) {
                o[off] = 0xFF; o[off + 1] = 0xC4; o[off + 2] = (unsigned char)((19 + n) >> 8); o[off + 3] = (unsigned char)((19 + n) & 255);
                o[off + 4] = (unsigned char)(((t & 1) << 4) | (t >> 1));
            }
            for (int i = lane; i < 16 + n; i += 64) o[off + 5 + i] = i < 16 ? bits[t][i] : vals[t][i - 16];
        }
        if (dri && threadIdx.x == 0) jr_dri(o + end, g.R);
        if (threadIdx.x < sos) o[end + dri + threadIdx.x] = p.hdr[p.hdr_len - sos + threadIdx.x];      // SOS
    }
    if (threadIdx.x == 0) fhdr_len[seg] = end + dri + sos <= kJfifHdrMax ? end + dri + sos : 0;
}

// in the place of (a1) and (a2) for files that carry the Annex K tables but run the table-driven stages (launch_jfif_entropy_annexk):
// one workgroup per (quality, image), thread i symbol i of the four tables; the file's markers are those of its quality, whole
__global__ __launch_bounds__(kJfThreads) void k_jfif_annexk(JfifGeom g, const JfifParams *__restrict__ par, unsigned *__restrict__ codes,
                                                            unsigned char *__restrict__ fhdr, int *__restrict__ fhdr_len)
{
    static_assert(kJfThreads == 256, "one thread per symbol");
    const long long seg = blockIdx.x;
    const int i = threadIdx.x;
    unsigned *tc = codes + seg * 4 * 256;
    tc[i] = i < 16 ? k_dc_luma[i] : 0;
    tc[256 + i] = k_ac_luma[i];
    if (g.ncomp != 1) {                                      // a one-component file has no chroma slots to fill
        tc[512 + i] = i < 16 ? k_dc_chroma[i] : 0;
        tc[768 + i] = k_ac_chroma[i];
    }
    const JfifParams &p = par[seg / g.B];
    const int n = min(max(p.hdr_len, 0), kJfifHdrMax);
    for (int j = i; j < n; j += kJfThreads) fhdr[seg * kJfifHdrMax + j] = p.hdr[j];
    if (i == 0) fhdr_len[seg] = n;
}

// (a3) every block's bits under its file's tables (k_jfif_quant counted them with the Annex K lengths)
template <int HS, int VS, int NC>
__global__ __launch_bounds__(kJfThreads) void k_jfif_count(JfifGeom g, const short *__restrict__ coef, const unsigned *__restrict__ codes,
                                                           int *__restrict__ lens)
{
    constexpr int NL = HS * VS, BPM = NL + NC - 1;
    const long long idx = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    if (idx >= (long long)g.nq * g.B * g.nblk) return;
    const long long seg = idx / g.nblk, blk = idx % g.nblk, m = blk / BPM;
    const int k = (int)(blk % BPM);
    const JfCodes hc = jf_file_codes(codes, seg, k >= NL);
    const short *base = coef + seg * g.nblk * 64, *c = base + blk * 64;
    JeLen sink{ nullptr, 0 };
    je_block_seq(c[0], je_dc_pred(base, NL, BPM, m, k, g.R), c, hc.dc, hc.ac, sink);
    lens[idx] = sink.total;
}

// (b) k_js_scan (jfif_stream_core.h): a segment's n + 1 prefix sums of its blocks' bits (boff) and later of its chunks' 0xFF counts (ffpre)
// the bits of segment seg: the last entry of its prefix sums
__device__ __forceinline__ long long jf_bits(const JfifGeom &g, const unsigned long long *boff, long long seg)
{
    return (long long)boff[seg * (g.nblk + 1) + g.nblk];
}

// the bytes of segment seg's unstuffed stream: its bits rounded up, or with restarts the sum of its byte-aligned intervals
__device__ __forceinline__ long long jf_bytes(const JfifGeom &g, const unsigned long long *boff, const unsigned long long *ivoff, long long seg)
{
    return g.R ? (long long)ivoff[seg * (g.niv + 1) + g.niv] : (jf_bits(g, boff, seg) + 7) >> 3;
}
// restarts: k_js_scan's input for the intervals' starts -- interval i of the launch, its blocks' bits (from boff) rounded up to bytes
struct JfIntervalBytes {
    const unsigned long long *boff;
    long long nblk, niv, per;              // blocks per segment, intervals per segment, blocks per interval (R x blocks per MCU)
    __device__ __forceinline__ unsigned long long operator()(long long i) const
    {
        const unsigned long long *b = boff + (i / niv) * (nblk + 1);
        const long long lo = (i % niv) * per, hi = min(lo + per, nblk);
        return (b[hi] - b[lo] + 7) >> 3;
    }
};

__global__ __launch_bounds__(kJfThreads) void k_jfif_zero(JfifGeom g, const unsigned long long *__restrict__ boff,
                                                          const unsigned long long *__restrict__ ivoff, unsigned *__restrict__ stream)
{
    const long long seg = blockIdx.y, i = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    if (i < min(g.stream_words, (jf_bytes(g, boff, ivoff, seg) + 3) >> 2)) stream[seg * g.stream_words + i] = 0;
}

// (c) every block's code string at its bit offset
// kOpt: the codes are the file's own (k_jfif_tables) instead of the Annex K constants
template <int HS, int VS, bool kOpt, int NC>
__global__ __launch_bounds__(kJfThreads) void k_jfif_emit(JfifGeom g, const short *__restrict__ coef, const unsigned long long *__restrict__ boff,
                                                          const unsigned long long *__restrict__ ivoff, const unsigned *__restrict__ codes,
                                                          unsigned *__restrict__ stream)
{
    constexpr int NL = HS * VS, BPM = NL + NC - 1;
    const long long idx = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    if (idx >= (long long)g.nq * g.B * g.nblk) return;
    const long long seg = idx / g.nblk, blk = idx % g.nblk, m = blk / BPM;
    const int k = (int)(blk % BPM);
    const JfCodes hc = kOpt ? jf_file_codes(codes, seg, k >= NL) : jf_codes(k >= NL);
    const short *base = coef + seg * g.nblk * 64, *c = base + blk * 64;
    const unsigned long long *b = boff + seg * (g.nblk + 1);                                    // n + 1 entries per segment
    const int dc = c[0], pred = je_dc_pred(base, NL, BPM, m, k, g.R);                           // (loaded beside the offsets, not behind them)
    JrPlace at{ (long long)b[blk], 0, blk == g.nblk - 1 };
    if (g.R) at = jr_place(blk, (long long)g.R * BPM, g.nblk, b, ivoff + seg * (g.niv + 1));   // uniform: inside its byte-aligned interval
    else if (at.last) at.total = jf_bits(g, boff, seg);
    JeEmit sink{ nullptr, JeBits(stream + seg * g.stream_words, at.pos, g.stream_words) };
    je_block_seq(dc, pred, c, hc.dc, hc.ac, sink);
    if (at.last) sink.bw.pad_ones(at.total);                 // the last byte (of every restart interval) is padded with 1-bits
    sink.bw.finish();
}

// 0xFF bytes per 64-byte chunk of each stream's data
__global__ __launch_bounds__(kJfThreads) void k_jfif_ffcount(JfifGeom g, const unsigned long long *__restrict__ boff,
                                                             const unsigned long long *__restrict__ ivoff, const unsigned *__restrict__ stream,
                                                             int *__restrict__ cnt)
{
    const long long idx = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    if (idx >= (long long)g.nq * g.B * g.n_chunks) return;
    const long long seg = idx / g.n_chunks, ch = idx % g.n_chunks, nbytes = min(g.stream_words * 4, jf_bytes(g, boff, ivoff, seg));
    const long long lo = ch * kJfChunk, hi = min(nbytes, lo + kJfChunk);
    const unsigned char *src = reinterpret_cast<const unsigned char *>(stream + seg * g.stream_words);
    cnt[idx] = js_stuff_count(src, lo, hi);
}

// file lengths (markers + stuffed data + EOI) and their offsets in the packed output, segments in (quality, image) order
// (with per-file tables the markers of file seg are fhdr[seg], fhdr_len[seg] bytes; otherwise those of its quality)
__global__ void k_jfif_layout(JfifGeom g, const JfifParams *__restrict__ par, const int *__restrict__ fhdr_len,
                              const unsigned long long *__restrict__ boff, const unsigned long long *__restrict__ ivoff,
                              const unsigned long long *__restrict__ ffpre, long long *__restrict__ lengths, long long *__restrict__ offsets,
                              long long *__restrict__ total)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long off = 0;
    for (long long seg = 0; seg < (long long)g.nq * g.B; seg++) {
        const long long len = (g.opt ? fhdr_len[seg] : par[seg / g.B].hdr_len) + jf_bytes(g, boff, ivoff, seg) +
                              (long long)ffpre[seg * (g.n_chunks + 1) + g.n_chunks] + (g.R ? 2 * (g.niv - 1) : 0) + 2;      // an RSTn before every interval but the first
        lengths[seg] = len;
        offsets[seg] = off;
        off += len;
    }
    *total = off;
}

__global__ __launch_bounds__(kJfThreads) void k_jfif_scatter(JfifGeom g, const JfifParams *__restrict__ par,
                                                             const unsigned char *__restrict__ fhdr, const int *__restrict__ fhdr_len,
                                                             const unsigned long long *__restrict__ boff, const unsigned long long *__restrict__ ivoff,
                                                             const unsigned *__restrict__ stream, const unsigned long long *__restrict__ ffpre,
                                                             const long long *__restrict__ lengths, const long long *__restrict__ offsets,
                                                             unsigned char *__restrict__ out, unsigned long long cap)
{
    const long long idx = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    if (idx >= (long long)g.nq * g.B * g.n_chunks) return;
    const long long seg = idx / g.n_chunks, ch = idx % g.n_chunks;
    const long long off = offsets[seg], len = lengths[seg];
    if (off < 0 || len < 0 || (unsigned long long)(off + len) > cap) return;
    const unsigned char *hdr = g.opt ? fhdr + seg * kJfifHdrMax : par[seg / g.B].hdr;
    const int hdr_len = g.opt ? fhdr_len[seg] : par[seg / g.B].hdr_len;
    unsigned char *file = out + off;
    if (ch == 0) {
        for (int i = 0; i < hdr_len; i++) file[i] = hdr[i];
        file[len - 2] = 0xFF;
        file[len - 1] = 0xD9;
    }
    const long long nbytes = min(g.stream_words * 4, jf_bytes(g, boff, ivoff, seg)), lo = ch * kJfChunk, hi = min(nbytes, lo + kJfChunk);
    const unsigned char *src = reinterpret_cast<const unsigned char *>(stream + seg * g.stream_words);
    if (lo >= hi) return;
    unsigned char *dst = file + hdr_len + lo + (long long)ffpre[idx + seg];                         // n + 1 entries per segment
    // uniform: with restarts the markers before this chunk shift it, those inside it are written here
    jr_stuff_chunk(dst, src, lo, hi, g.R ? ivoff + seg * (g.niv + 1) : nullptr, g.R ? g.niv : 0);
}

// ---- reconstruction ----------------------------------------------------------------------------------------------------------------
template <int HS, int VS>
__global__ __launch_bounds__(kJfThreads) void k_jfif_idct(JfifGeom g, const JfifParams *__restrict__ par, const short *__restrict__ coef,
                                                          unsigned char *__restrict__ planes)
{
    constexpr int NL = HS * VS, BPM = NL + 2;
    const long long idx = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    if (idx >= (long long)g.nq * g.B * g.nblk) return;
    const long long seg = idx / g.nblk, blk = idx % g.nblk, m = blk / BPM;
    const int k = (int)(blk % BPM), my = (int)(m / g.mcux), mx = (int)(m % g.mcux);
    if (!jf_real<HS, VS>(g, m, k)) return;
    const int *qt = par[seg / g.B].qt[k >= NL];
    const short *c = coef + idx * 64;
    long long d[64];
#pragma unroll
    for (int j = 0; j < 64; j++) d[j] = c[kZigzag8.position[j]] * qt[kZigzag8.position[j]];      // natural order (j constant after unrolling)
#pragma unroll
    for (int col = 0; col < 8; col++) jd_idct8<true>(d + col, 8);
#pragma unroll
    for (int r = 0; r < 8; r++) jd_idct8<false>(d + r * 8, 1);
    unsigned char *pl = planes + seg * g.plane_bytes;
    int stride, y0, x0;
    if (k < NL) {
        stride = g.yw; y0 = (VS * my + k / HS) * 8; x0 = (HS * mx + k % HS) * 8;
    } else {
        pl += (long long)g.yh * g.yw + (long long)(k - NL) * g.ch * g.cw;
        stride = g.cw; y0 = my * 8; x0 = mx * 8;
    }
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
        for (int cc = 0; cc < 8; cc++) pl[(long long)(y0 + r) * stride + x0 + cc] = jd_range_limit(d[r * 8 + cc]);
}

// chroma of output pixel (y, x): jd_chroma (jpegdec_core.h) over the real ceil(H / VS) x ceil(W / HS) samples -- h2v2 / h2v1 fancy
// up-sampling, replication when that is at most 2 wide, the sample itself at 4:4:4
template <int HS, int VS>
__global__ __launch_bounds__(kJfThreads) void k_jfif_rgb(JfifGeom g, const unsigned char *__restrict__ planes, unsigned char *__restrict__ out)
{
    const long long idx = (long long)blockIdx.x * kJfThreads + threadIdx.x;
    const long long px = (long long)g.H * g.W;
    if (idx >= (long long)g.nq * g.B * px) return;
    const long long seg = idx / px, r = idx % px;
    const int y = (int)(r / g.W), x = (int)(r % g.W);
    const unsigned char *pl = planes + seg * g.plane_bytes;
    const int Y = pl[(long long)y * g.yw + x];
    const unsigned char *cbp = pl + (long long)g.yh * g.yw, *crp = cbp + (long long)g.ch * g.cw;
    const int wc = (g.W + HS - 1) / HS, hc = (g.H + VS - 1) / VS;
    jd_rgb(Y, jd_chroma(cbp, g.cw, HS, VS, wc, hc, y, x), jd_chroma(crp, g.cw, HS, VS, wc, hc, y, x), out + idx * 3);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// Annex K.3 tables as DHT carries them: BITS[1..16] then HUFFVAL (host side, for the markers)
static const unsigned char kDht_dc_luma[28] = {
    0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const unsigned char kDht_ac_luma[178] = {
    0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125, 1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6,
    19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22,
    23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85,
    86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137,
    138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
    194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234,
    241, 242, 243, 244, 245, 246, 247, 248, 249, 250};
static const unsigned char kDht_dc_chroma[28] = {
    0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const unsigned char kDht_ac_chroma[178] = {
    0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119, 0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65,
    81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52,
    225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84,
    85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135,
    136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184,
    185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233,
    234, 242, 243, 244, 245, 246, 247, 248, 249, 250};
static const unsigned char kLumaBase[64] = { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 };
static const unsigned char kChromaBase[64] = { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 };

bool jfif_geom(int B, int H, int W, int nq, JfifGeom &g, int ss, int opt, int ncomp)
{
    if (ncomp == 1) ss = 0;                                  // one component is sampled 1 x 1
    if (ss < 0 || ss > 2) return false;
    return jfif_geom_sampled(B, H, W, nq, g, ss == 0 ? 1 : 2, ss == 2 ? 2 : 1, opt, ncomp);
}

bool jfif_geom_sampled(int B, int H, int W, int nq, JfifGeom &g, int hs, int vs, int opt, int ncomp)
{
    if (B < 1 || nq < 1 || H < 1 || W < 1 || H > 65535 || W > 65535 || (long long)B * nq > 65535) return false;      // segments index grid.y
    if (ncomp != 1 && ncomp != 3) return false;
    if (ncomp == 1) hs = vs = 1;
    if (!((hs == 1 || hs == 2) && (vs == 1 || vs == 2))) return false;
    g.B = B; g.H = H; g.W = W; g.nq = nq;
    g.hs = hs; g.vs = vs; g.opt = opt ? 1 : 0; g.ncomp = ncomp;
    g.mcux = (W + 8 * g.hs - 1) / (8 * g.hs); g.mcuy = (H + 8 * g.vs - 1) / (8 * g.vs);
    g.ybx = (W + 7) / 8; g.yby = (H + 7) / 8;
    g.yw = 8 * g.hs * g.mcux; g.yh = 8 * g.vs * g.mcuy;   // luma planes cover every MCU (dummy blocks are never written)
    g.cw = 8 * g.mcux; g.ch = 8 * g.mcuy;
    g.n_mcu = (long long)g.mcux * g.mcuy;
    g.nblk = (g.hs * g.vs + ncomp - 1) * g.n_mcu;
    g.stream_words = (g.nblk * (g.opt ? kJfifBlockWordsOpt : kJfifBlockWords) + 2 + 15) / 16 * 16;
    // With restarts (jfif_geom_restart) every interval is padded to a byte: up to 7 bits for each of at most nblk intervals.  A block
    // under a file's own tables has 53 x 32 - 1665 = 31 bits to spare, so nblk x 53 words still hold sum(bits) + 7 x intervals; under
    // the Annex K bound the spare is 52 x 32 - 1660 = 4 bits, which is why an interval requires opt.
    g.R = 0; g.rst_pad_ = 0; g.niv = 0;
    g.n_chunks = g.stream_words * 4 / kJfChunk;
    g.plane_bytes = ((long long)g.yh * g.yw + 2LL * g.ch * g.cw + 255) / 256 * 256;
    return true;
}

bool jfif_geom_restart(JfifGeom &g, int blocks, int rows)
{
    if (blocks < 0 || blocks > kJrMaxInterval || rows < 0 || rows > kJrMaxInterval) return false;
    g.R = jr_interval(blocks, rows, g.mcux);                 // one component: mcux is its blocks per row
    g.niv = g.R ? jr_count(g.n_mcu, g.R) : 0;
    return g.R == 0 || g.opt != 0;
}

unsigned long long jfif_carve(void *base, const JfifGeom &g, JfifBufs &w)
{
    Carver c(base);
    const long long segs = (long long)g.nq * g.B;
    w.par = c.take<JfifParams>(g.nq);
    w.dct = c.take<int>((long long)g.B * g.nblk * 64);
    w.coef = c.take<short>(segs * g.nblk * 64);
    w.lens = c.take<int>(segs * g.nblk);
    w.boff = c.take<unsigned long long>(segs * (g.nblk + 1));
    w.stream = c.take<unsigned>(segs * g.stream_words);
    w.ffcnt = c.take<int>(segs * g.n_chunks);
    w.ffpre = c.take<unsigned long long>(segs * (g.n_chunks + 1));
    w.total = c.take<long long>(1);
    w.planes = c.take<unsigned char>(segs * g.plane_bytes);
    w.hist = nullptr; w.codes = nullptr; w.fhdr = nullptr; w.fhdr_len = nullptr; w.ivoff = nullptr;
    if (g.opt) {
        w.hist = c.take<unsigned long long>(segs * 4 * kJhSymbols);
        w.codes = c.take<unsigned>(segs * 4 * 256);
        w.fhdr = c.take<unsigned char>(segs * kJfifHdrMax);
        w.fhdr_len = c.take<int>(segs);
    }
    return c.bytes();
}

// the transcoder's workspace of one group of files (jfiftrans.hip): jfif_carve without what colour, DCT and reconstruction use -- the
// markers, the coefficients and every buffer of the optimised entropy stages.  Kept beside jfif_carve so that the two lists stay one.
unsigned long long jfif_carve_coded(Carver &c, const JfifGeom &g, JfifBufs &w)
{
    const long long segs = (long long)g.nq * g.B;
    w = JfifBufs{};
    w.par = c.take<JfifParams>(g.nq);
    w.coef = c.take<short>(segs * g.nblk * 64);
    w.lens = c.take<int>(segs * g.nblk);
    w.boff = c.take<unsigned long long>(segs * (g.nblk + 1));
    w.stream = c.take<unsigned>(segs * g.stream_words);
    w.ffcnt = c.take<int>(segs * g.n_chunks);
    w.ffpre = c.take<unsigned long long>(segs * (g.n_chunks + 1));
    w.total = c.take<long long>(1);
    w.hist = c.take<unsigned long long>(segs * 4 * kJhSymbols);
    w.codes = c.take<unsigned>(segs * 4 * 256);
    w.fhdr = c.take<unsigned char>(segs * kJfifHdrMax);
    w.fhdr_len = c.take<int>(segs);
    if (g.R) w.ivoff = c.take<unsigned long long>(segs * (g.niv + 1));
    return c.bytes();
}

int jfif_huffman_host(const long long *counts, unsigned char *bits, unsigned char *huffval)
{
    JhWork w;
    bool any = false;
    for (int i = 0; i < 256; i++) {
        if (counts[i] < 0) return -1;
        any |= counts[i] > 0;
        w.freq[i] = counts[i];
    }
    if (!any || counts[256] < 0) return -1;
    return jh_build(w, bits, huffval);
}

// the testing entry aej_test_jfif_seq_scan_host: the baseline scan of n_mcu MCUs of given coefficients, by the text the kernels run --
// je_block_seq and je_dc_pred into the three sinks, jh_build / jh_codes, jr_place, JeBits::pad_ones, jr_stuff_chunk -- stage after stage
// as jf_entropy launches them
int jfif_seq_scan_host(const short *coefs, long long n_mcu, int hs, int vs, int ncomp, int R, int optimize, long long *hist, unsigned char *out,
                       unsigned long long cap, unsigned long long *out_len)
{
    if (!coefs || !hist || !out || !out_len || n_mcu < 1 || n_mcu > (1LL << 20) || (ncomp != 1 && ncomp != 3) || (optimize != 0 && optimize != 1)) return AEJ_ERR_ARG;
    if (ncomp == 1) hs = vs = 1;
    if (!((hs == 1 || hs == 2) && (vs == 1 || vs == 2)) || R < 0 || R > kJrMaxInterval || (R > 0 && !optimize)) return AEJ_ERR_ARG;
    const int NL = hs * vs, BPM = NL + ncomp - 1, ntab = ncomp == 1 ? 2 : 4;
    const long long n = n_mcu * BPM;
    for (long long i = 0; i < n * 64; i++)
        if (coefs[i] > kJeMaxCoef || coefs[i] < -kJeMaxCoef) return AEJ_ERR_ARG;
    std::vector<unsigned> codes(4 * 256, 0);
    // block i as the kernels code it, under tables of `stride` entries each: DC luma, AC luma, DC chroma, AC chroma
    auto block = [&](long long i, auto *tabs, int stride, auto &sink) {
        const int k = (int)(i % BPM);
        const short *c = coefs + i * 64;
        tabs += (k >= NL ? 2 : 0) * stride;
        je_block_seq(c[0], je_dc_pred(coefs, NL, BPM, i / BPM, k, R), c, tabs, tabs + stride, sink);
    };
    // k_jfif_hist
    for (int i = 0; i < 4 * kJhSymbols; i++) hist[i] = 0;
    for (long long i = 0; i < n; i++) {
        JeHist<unsigned long long> sink{ nullptr };
        block(i, reinterpret_cast<unsigned long long *>(hist), kJhSymbols, sink);      // (the counts are not negative)
    }
    // k_jfif_tables, or the Annex K tables
    const unsigned char *annexk[4] = { kDht_dc_luma, kDht_ac_luma, kDht_dc_chroma, kDht_ac_chroma };
    for (int t = 0; t < ntab; t++) {
        unsigned char bits[16], vals[256];
        if (optimize) {
            JhWork w;
            for (int i = 0; i < 256; i++) w.freq[i] = hist[t * kJhSymbols + i];
            jh_build(w, bits, vals);
        }
        jh_codes(optimize ? bits : annexk[t], optimize ? vals : annexk[t] + 16, codes.data() + t * 256);
    }
    // k_jfif_count, k_js_scan (bits, then the intervals' bytes)
    std::vector<unsigned long long> P(n + 1, 0), starts;
    for (long long i = 0; i < n; i++) {
        JeLen sink{ nullptr, 0 };
        block(i, codes.data(), 256, sink);
        P[i + 1] = P[i] + sink.total;
    }
    const long long per = (long long)R * BPM, niv = R ? jr_count(n_mcu, R) : 0;
    starts.assign(niv + 1, 0);
    for (long long v = 0; v < niv; v++) starts[v + 1] = starts[v] + ((P[std::min((v + 1) * per, n)] - P[v * per] + 7) >> 3);
    const long long nbytes = R ? (long long)starts[niv] : (long long)((P[n] + 7) >> 3), limit = (nbytes + 3) / 4 + 1;
    // k_jfif_emit
    std::vector<unsigned> words(limit, 0);
    for (long long i = 0; i < n; i++) {
        JrPlace at{ (long long)P[i], (long long)P[n], i == n - 1 };
        if (R) at = jr_place(i, per, n, P.data(), starts.data());
        JeEmit sink{ nullptr, JeBits(words.data(), at.pos, limit) };
        block(i, codes.data(), 256, sink);
        if (at.last) sink.bw.pad_ones(at.total);
        sink.bw.finish();
    }
    // k_jfif_ffcount, k_jfif_layout, k_jfif_scatter
    const unsigned char *src = reinterpret_cast<const unsigned char *>(words.data());
    const unsigned long long o = (unsigned long long)(nbytes + js_stuff_count(src, 0, nbytes) + (R ? 2 * (niv - 1) : 0));
    *out_len = o;
    if (o > cap) return AEJ_ERR_CAPACITY;
    jr_stuff_chunk(out, src, 0, nbytes, starts.data(), niv);
    return 0;
}

void jfif_quant_tables(int q, int luma[64], int chroma[64])
{
    q = q < 1 ? 1 : q > 100 ? 100 : q;
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 64; i++) {
        luma[i] = std::min(255, std::max(1, (kLumaBase[i] * scale + 50) / 100));
        chroma[i] = std::min(255, std::max(1, (kChromaBase[i] * scale + 50) / 100));
    }
}

void jfif_params_host(int q, int H, int W, JfifParams &p, int ss, int ncomp, int R)
{
    const int nt = ncomp == 1 ? 1 : 2;                       // a grey file: the luma quantiser and the two luma Huffman tables alone
    int t[2][64];
    jfif_quant_tables(q, t[0], t[1]);
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < 64; i++) p.qt[c][i] = t[c][kZigzag8.natural[i]];
    unsigned char *o = p.hdr;
    int n = 0;
    auto put = [&](std::initializer_list<int> v) { for (int x : v) o[n++] = (unsigned char)x; };
    auto seg = [&](int marker, int len) { put({ 0xFF, marker, (len + 2) >> 8, (len + 2) & 255 }); };
    put({ 0xFF, 0xD8 });
    seg(0xE0, 14);                                                        // JFIF 1.01, no units, 1:1 density, no thumbnail
    put({ 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 });
    for (int c = 0; c < nt; c++) {
        seg(0xDB, 65);
        put({ c });
        for (int i = 0; i < 64; i++) o[n++] = (unsigned char)p.qt[c][i];
    }
    seg(0xC0, jfif_sof_bytes(ncomp == 1 ? 1 : 3) - 4);
    if (ncomp == 1) put({ 8, H >> 8, H & 255, W >> 8, W & 255, 1, 1, 0x11, 0 });
    else put({ 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, ss == 0 ? 0x11 : ss == 1 ? 0x21 : ss == 2 ? 0x22 : 0x12, 0, 2, 0x11, 1, 3, 0x11, 1 });      // 3: 4:4:0
    p.dht_off = n;
    const struct { int id; const unsigned char *t; int len; } dht[4] = {
        { 0x00, kDht_dc_luma, (int)sizeof kDht_dc_luma }, { 0x10, kDht_ac_luma, (int)sizeof kDht_ac_luma },
        { 0x01, kDht_dc_chroma, (int)sizeof kDht_dc_chroma }, { 0x11, kDht_ac_chroma, (int)sizeof kDht_ac_chroma } };
    for (int t = 0; t < 2 * nt; t++) {
        const auto &d = dht[t];
        seg(0xC4, 1 + d.len);
        put({ d.id });
        for (int i = 0; i < d.len; i++) o[n++] = d.t[i];
    }
    if (R > 0) {                                             // libjpeg writes the DRI in the scan header, after the tables
        jr_dri(o + n, R);
        n += kJrDriBytes;
    }
    seg(0xDA, jfif_sos_bytes(ncomp == 1 ? 1 : 3) - 4);
    if (ncomp == 1) put({ 1, 1, 0x00, 0, 63, 0 });
    else put({ 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0 });
    p.hdr_len = n;
}

static unsigned jf_blocks(long long n) { return (unsigned)((n + kJfThreads - 1) / kJfThreads); }

// the kernels' template arguments of a geometry: f(JfShape<HS, VS, NC>{}) for g's sampling factors and component count
template <int HS, int VS, int NC>
struct JfShape { static constexpr int hs = HS, vs = VS, nc = NC; };
template <class F>
static hipError_t jf_dispatch(const JfifGeom &g, F f)
{
    if (g.ncomp == 1) return f(JfShape<1, 1, 1>{});
    if (g.hs == 1 && g.vs == 2) return hipErrorInvalidValue;      // 4:4:0 has entropy chains alone (jf_dispatch_coded)
    if (g.hs == 1) return f(JfShape<1, 1, 3>{});
    if (g.vs == 1) return f(JfShape<2, 1, 3>{});
    return f(JfShape<2, 2, 3>{});
}
// the same for the entropy chains, which also take 4:4:0 (two luma blocks stacked in the MCU: the transcoder's and the transforms' outputs)
template <class F>
static hipError_t jf_dispatch_coded(const JfifGeom &g, F f)
{
    if (g.ncomp == 3 && g.hs == 1 && g.vs == 2) return f(JfShape<1, 2, 3>{});
    return jf_dispatch(g, f);
}

// the stages from w.coef to the file lengths and offsets (k_jfif_quant has left the Annex K bit counts in w.lens)
// annexk (requires g.opt): the table-driven stages under the Annex K tables -- k_jfif_annexk in the place of histogram and tables
template <int HS, int VS, int NC>
static hipError_t jf_entropy(hipStream_t st, const JfifGeom &g, const JfifBufs &w, long long *lengths, long long *offsets, bool annexk)
{
    const long long segs = (long long)g.nq * g.B, nb = segs * g.nblk, nc = segs * g.n_chunks;
    const dim3 th(kJfThreads), per_seg((unsigned)segs), scan_th(kJsScanThreads);
    if (annexk && !g.opt) return hipErrorInvalidValue;
    if (annexk) {
        hipLaunchKernelGGL(k_jfif_annexk, per_seg, th, 0, st, g, w.par, w.codes, w.fhdr, w.fhdr_len);
    } else if (g.opt) {
        const hipError_t e = hipMemsetAsync(w.hist, 0, (size_t)segs * 4 * kJhSymbols * 8, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_jfif_hist<HS, VS, NC>), dim3(jf_blocks(g.nblk), (unsigned)segs), th, 0, st, g, w.coef, w.hist);
        hipLaunchKernelGGL(k_jfif_tables, per_seg, th, 0, st, g, w.par, w.hist, w.codes, w.fhdr, w.fhdr_len);
    }
    if (g.opt) hipLaunchKernelGGL((k_jfif_count<HS, VS, NC>), dim3(jf_blocks(nb)), th, 0, st, g, w.coef, w.codes, w.lens);
    hipLaunchKernelGGL(k_js_scan<JsInts>, per_seg, scan_th, 0, st, JsInts{ w.lens }, g.nblk, w.boff);
    if (g.R) {                                               // the byte starts of the restart intervals: a second prefix sum, over their byte lengths
        if (!g.opt || !w.ivoff) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_js_scan<JfIntervalBytes>, per_seg, scan_th, 0, st, JfIntervalBytes{ w.boff, g.nblk, g.niv, (long long)g.R * (HS * VS + NC - 1) },
                           g.niv, w.ivoff);
    }
    hipLaunchKernelGGL(k_jfif_zero, dim3(jf_blocks(g.stream_words), (unsigned)segs), th, 0, st, g, w.boff, w.ivoff, w.stream);
    if (g.opt) hipLaunchKernelGGL((k_jfif_emit<HS, VS, true, NC>), dim3(jf_blocks(nb)), th, 0, st, g, w.coef, w.boff, w.ivoff, w.codes, w.stream);
    else hipLaunchKernelGGL((k_jfif_emit<HS, VS, false, NC>), dim3(jf_blocks(nb)), th, 0, st, g, w.coef, w.boff, w.ivoff, w.codes, w.stream);
    hipLaunchKernelGGL(k_jfif_ffcount, dim3(jf_blocks(nc)), th, 0, st, g, w.boff, w.ivoff, w.stream, w.ffcnt);
    hipLaunchKernelGGL(k_js_scan<JsInts>, per_seg, scan_th, 0, st, JsInts{ w.ffcnt }, g.n_chunks, w.ffpre);
    hipLaunchKernelGGL(k_jfif_layout, dim3(1), dim3(1), 0, st, g, w.par, w.fhdr_len, w.boff, w.ivoff, w.ffpre, lengths, offsets, w.total);
    return hipGetLastError();
}

// the transcoder's cut (jfiftrans.hip): given coefficients in w.coef and the files' markers in w.par (uploaded by the caller), the
// entropy stages up to the lengths, and the scatter as a launch of its own once the caller has placed the files
hipError_t launch_jfif_entropy(hipStream_t st, const JfifGeom &g, const JfifBufs &w, long long *lengths, long long *offsets)
{
    return jf_dispatch_coded(g, [&](auto s) { return jf_entropy<s.hs, s.vs, s.nc>(st, g, w, lengths, offsets, false); });
}

hipError_t launch_jfif_entropy_annexk(hipStream_t st, const JfifGeom &g, const JfifBufs &w, long long *lengths, long long *offsets)
{
    return jf_dispatch_coded(g, [&](auto s) { return jf_entropy<s.hs, s.vs, s.nc>(st, g, w, lengths, offsets, true); });
}

hipError_t launch_jfif_scatter(hipStream_t st, const JfifGeom &g, const JfifBufs &w, const long long *lengths, const long long *offsets,
                               unsigned char *out, unsigned long long cap)
{
    hipLaunchKernelGGL(k_jfif_scatter, dim3(jf_blocks((long long)g.nq * g.B * g.n_chunks)), dim3(kJfThreads), 0, st, g, w.par, w.fhdr, w.fhdr_len,
                       w.boff, w.ivoff, w.stream, w.ffpre, lengths, offsets, out, cap);
    return hipGetLastError();
}

hipError_t launch_jfif_coefs(hipStream_t st, const JfifGeom &g, const JfifBufs &w, const JfifParams *par_host, const unsigned char *rgb)
{
    if (g.ncomp != 3) return hipErrorInvalidValue;           // colour, FDCT and quantisation are three-component
    const hipError_t e = hipMemcpyAsync(w.par, par_host, sizeof(JfifParams) * g.nq, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    return jf_dispatch(g, [&](auto s) {
        const long long nb = (long long)g.B * g.nblk;
        hipLaunchKernelGGL((k_jfif_fdct<s.hs, s.vs>), dim3(jf_blocks(nb)), dim3(kJfThreads), 0, st, g, rgb, w.dct);
        hipLaunchKernelGGL((k_jfif_quant<s.hs, s.vs>), dim3(jf_blocks(g.nq * nb)), dim3(kJfThreads), 0, st, g, w.par, w.dct, w.coef, w.lens);
        return hipGetLastError();
    });
}

hipError_t launch_jfif_encode(hipStream_t st, const JfifGeom &g, const JfifBufs &w, const JfifParams *par_host, const unsigned char *rgb,
                              unsigned char *out, unsigned long long cap, long long *lengths, long long *offsets)
{
    if (g.ncomp != 3) return hipErrorInvalidValue;           // the same-size encoder is three-component
    hipError_t e = launch_jfif_coefs(st, g, w, par_host, rgb);
    if (e == hipSuccess) e = launch_jfif_entropy(st, g, w, lengths, offsets);
    if (e == hipSuccess && out) e = launch_jfif_scatter(st, g, w, lengths, offsets, out, cap);
    return e;
}

hipError_t launch_jfif_recon(hipStream_t st, const JfifGeom &g, const JfifBufs &w, unsigned char *rgb_out)
{
    if (g.ncomp != 3) return hipErrorInvalidValue;
    return jf_dispatch(g, [&](auto s) {
        const long long segs = (long long)g.nq * g.B;
        hipLaunchKernelGGL((k_jfif_idct<s.hs, s.vs>), dim3(jf_blocks(segs * g.nblk)), dim3(kJfThreads), 0, st, g, w.par, w.coef, w.planes);
        hipLaunchKernelGGL((k_jfif_rgb<s.hs, s.vs>), dim3(jf_blocks(segs * g.H * g.W)), dim3(kJfThreads), 0, st, g, w.planes, rgb_out);
        return hipGetLastError();
    });
}

}  // namespace aej
