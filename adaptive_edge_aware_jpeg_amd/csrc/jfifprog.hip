// jfifprog.hip -- the progressive file Pillow writes with save(..., "JPEG", quality=q, subsampling=s, progressive=True): libjpeg's
// jpeg_simple_progression of ten scans, every scan Huffman-coded under its own optimal table (aej_jfif_*_prog, include/aej.h).  Colour,
// down-sampling, FDCT and quantisation are jfif.hip's (launch_jfif_coefs); this file codes the quantised coefficients.  The rules of
// the coder -- what one block emits, how end-of-band runs and deferred correction bits partition a scan -- are jfif_prog_core.h; the
// bit writer, byte stuffing, predecessor block and prefix-sum kernel are jfif_stream_core.h, which the baseline coder shares;
// tests/jfif_progressive_reference.py is libjpeg's serial state machine in Python and tests/test_*jfif_progressive*.py pin both to
// Pillow's files byte for byte.  A one-component (grey) file takes libjpeg's six-scan script and one DC table (JfpGeom::nchroma = 0, as the
// testing entry's plain list): its DC scans walk the component's blocks in raster order, which is its MCU order, so every kernel below
// runs it unchanged -- jfifprog_geom alone knows about it.
//
// An item is one block of one scan; a file has T of them, scan after scan (interleaved scans walk the MCU-padded blocks in MCU order,
// single-component scans the component's own blocks in raster order).  Stages (one launch each for every file of a call):
//   k_jfp_facts    one thread per item of an AC scan: does the block emit, does it leave zeros or correction bits pending, how many
//   k_js_scan      one workgroup per file: exclusive prefix sums of the packed (break, pending bits) values (je_pack; JfpPacked) --
//                  the segmented prefix-sum kernel of jfif_stream_core.h, which jfif.hip runs too
//   k_jfp_cuts     one thread per chain start: the pieces of its chain, one binary search (je_piece_end) per piece; the opener of a
//                  piece gets the piece's length.  The longest serial walk is the number of pieces of one chain: a piece spans 0x7FFF
//                  blocks unless more than 937 bits are deferred, and then at least 15 (a block defers at most 63)
//   k_jfp_hist     one thread per item: the symbols it writes (its own, and the EOBn of the piece it opens), counted per wave in LDS
//   k_jfp_tables   one workgroup per file, one wave per table (two DC, eight AC): jh_build, the codes, the DHT / SOS markers per scan
//   k_jfp_count    one thread per item: its bits under the file's codes (the scan's table staged in LDS, as in k_jfp_emit)
//   k_js_scan      bit offsets (JsInts)
//   k_jfp_zero     the words the scans will use
//   k_js_scan      restarts only (JfpScan::R, jfif_restart_core.h): the byte starts of every scan's restart intervals (JfpIntervalBytes)
//   k_jfp_emit     one thread per item: own symbols, EOBn, deferred bits at the item's bit offset; the last item of a scan pads
// Restart markers: every scan has its own interval (jfp_restarts); the first item of an interval is the first item of a scan -- it breaks
// the end-of-band chain (k_jfp_facts), its DC predictor is 0 -- every interval is byte-aligned and padded in the scan's stream, and
// k_jfp_scatter inserts the RSTn markers while it stuffs; k_jfp_tables writes a DRI before the SOS of a scan whose interval changed.
//   k_jfp_ffcount, k_js_scan, k_jfp_layout, k_jfp_scatter: 0xFF stuffing per 64-byte chunk of every scan's stream (js_stuff_count,
//                  js_stuff_copy) and the file SOI .. SOF2, then per scan [DHT] SOS data, then EOI
// Bounds: an item's index derives from JfpGeom; a scan's words stay inside its wcap (je_block_bound per block) and every store into a
// stream checks it; k_jfp_scatter writes a file only if it ends inside the caller's capacity.
#include "aej_common.h"
#include "aej_ctx.h"
#include "aej_launch.h"
#include "jfif_huff_core.h"
#include "jfif_prog_core.h"
#include "jfif_restart_core.h"
#include "jfif_stream_core.h"

#include <vector>

namespace aej {

constexpr int kJfpThreads = 256;
constexpr int kJfpChunk = 64;          // bytes per stuffing chunk
constexpr int kJfpMaxTables = 10;
constexpr unsigned short kFlagE = 1, kFlagJoins = 2, kFlagFirst = 256, kFlagAc = 512;      // bits 2..7: pending correction bits

// ---- geometry ------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline long long jfp_coef_block(const JfpGeom &g, const JfpScan &s, long long i)      // item i of scan s -> block of the file
{
    if (s.comp < 0) return i;
    const int NL = g.hs * g.vs, BPM = NL + g.nchroma;
    if (s.comp > 0) return i * BPM + NL + s.comp - 1;
    const long long by = i / g.ybx, bx = i % g.ybx;
    return ((by / g.vs) * g.mcux + bx / g.hs) * BPM + (by % g.vs) * g.hs + bx % g.hs;
}
// DC first scans (interleaved): the predictor of item i (je_dc_pred) and whether i is chroma
__device__ __forceinline__ int jfp_dc_pred(const JfpGeom &g, const JfpScan &s, const short *base, long long i, bool *chroma)
{
    const int NL = g.hs * g.vs, BPM = NL + g.nchroma, k = (int)(i % BPM);
    *chroma = k >= NL;
    return je_dc_pred(base, NL, BPM, i / BPM, k, s.R);
}
// the value of item idx in the partition's prefix sums (je_pack), from the flags k_jfp_facts left
__device__ __forceinline__ unsigned long long jfp_value(const unsigned short *flags, long long idx)
{
    const unsigned f = flags[idx];
    if (!(f & kFlagAc)) return 0;
    const bool first = (f & kFlagFirst) != 0;
    return je_pack(first, (f & kFlagE) != 0, first ? false : (flags[idx - 1] & kFlagJoins) != 0, (int)((f >> 2) & 63));
}
__device__ __forceinline__ long long jfp_scan_bits(const JfpGeom &g, const unsigned long long *pre, long long seg, const JfpScan &s)
{
    const unsigned long long *p = pre + seg * (g.T + 1) + s.ioff;
    return (long long)(p[s.n] - p[0]);
}
// the bytes of scan s of file seg in its unstuffed stream: its bits rounded up, or with restarts the sum of its byte-aligned intervals
__device__ __forceinline__ long long jfp_scan_bytes(const JfpGeom &g, const unsigned long long *pre, const unsigned long long *ivpre, long long seg,
                                                    const JfpScan &s)
{
    if (g.NIV) {
        const unsigned long long *v = ivpre + seg * (g.NIV + 1) + s.ivoff;
        return (long long)(v[s.niv] - v[0]);
    }
    return (jfp_scan_bits(g, pre, seg, s) + 7) >> 3;
}
__device__ __forceinline__ int jfp_chunk_scan(const JfpGeom &g, long long ch)      // the scan whose stream holds chunk ch
{
    int s = 0;
    while (s + 1 < g.nscan && ch >= g.sc[s + 1].coff) s++;
    return s;
}

// ---- stages --------------------------------------------------------------------------------------------------------------------------
// grid of the per-item kernels: (blocks of the longest scan, scan, file)
__global__ __launch_bounds__(kJfpThreads) void k_jfp_facts(JfpGeom g, const short *__restrict__ coef, unsigned short *__restrict__ flags)
{
    const JfpScan s = g.sc[blockIdx.y];
    const long long i = (long long)blockIdx.x * kJfpThreads + threadIdx.x, seg = blockIdx.z;
    if (i >= s.n) return;
    unsigned f = 0;
    if (s.Ss > 0) {
        const short *c = coef + (seg * g.nblk + jfp_coef_block(g, s, i)) * 64;
        JeNull nul;
        const JeBlock b = s.Ah ? je_ac_refine(c, s.Ss, s.Se, s.Al, nul) : je_ac_first(c, s.Ss, s.Se, s.Al, nul);
        f = kFlagAc | (b.e ? kFlagE : 0) | (b.r > 0 || b.br > 0 ? kFlagJoins : 0) | ((unsigned)b.br << 2) |
            (i == 0 || (s.R && i % s.per == 0) ? kFlagFirst : 0);      // the first item of a restart interval is the first of a scan: it breaks the chain
    }
    flags[seg * g.T + s.ioff + i] = (unsigned short)f;
}

// k_js_scan's input for the partition: jfp_value of the flags
struct JfpPacked {
    const unsigned short *flags;
    __device__ __forceinline__ unsigned long long operator()(long long i) const { return jfp_value(flags, i); }
};

__global__ __launch_bounds__(kJfpThreads) void k_jfp_cuts(JfpGeom g, const unsigned short *__restrict__ flags,
                                                          const unsigned long long *__restrict__ pre, int *__restrict__ plen, int *__restrict__ cuts)
{
    const JfpScan s = g.sc[blockIdx.y];
    const long long i = (long long)blockIdx.x * kJfpThreads + threadIdx.x, seg = blockIdx.z;
    if (i >= s.n || s.Ss == 0) return;
    const long long idx = seg * g.T + s.ioff + i;
    if (!(flags[idx] & kFlagJoins) || !(jfp_value(flags, idx) >> kJeBrShift)) return;      // not the start of a chain
    const unsigned long long *P = pre + seg * (g.T + 1) + s.ioff;
    const long long ce = je_chain_end(P, i, s.n);
    for (long long p = i; p < ce;) {
        int why;
        const long long q = je_piece_end(P, p, ce, &why);
        plen[idx - i + p] = (int)(q - p);
        if (why) atomicAdd(cuts + (seg * g.nscan + blockIdx.y) * 2 + why - 1, 1);
        p = q;
    }
}

__global__ __launch_bounds__(kJfpThreads) void k_jfp_hist(JfpGeom g, const short *__restrict__ coef, const int *__restrict__ plen,
                                                          unsigned long long *__restrict__ hist)
{
    constexpr int kWaves = kJfpThreads / 64;
    __shared__ unsigned cnt[kWaves][2][kJhSymbols];
    const JfpScan s = g.sc[blockIdx.y];
    if (s.Ss == 0 && s.Ah) return;                           // a DC refinement scan writes raw bits alone (uniform over the workgroup)
    for (int i = threadIdx.x; i < kWaves * 2 * kJhSymbols; i += kJfpThreads) (&cnt[0][0][0])[i] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * kJfpThreads + threadIdx.x, seg = blockIdx.z;
    if (i < s.n) {
        const short *base = coef + seg * g.nblk * 64;
        if (s.Ss == 0) {
            bool chroma;
            const int pred = jfp_dc_pred(g, s, base, i, &chroma);
            JeHist<unsigned> sink{ cnt[threadIdx.x / 64][chroma ? 1 : 0] };
            je_dc_first(base[i * 64], pred, s.Al, sink);
        } else {
            JeHist<unsigned> sink{ cnt[threadIdx.x / 64][0] };
            const short *c = base + jfp_coef_block(g, s, i) * 64;
            if (s.Ah) je_ac_refine(c, s.Ss, s.Se, s.Al, sink); else je_ac_first(c, s.Ss, s.Se, s.Al, sink);
            const int run = plen[seg * g.T + s.ioff + i];
            if (run > 0) je_eobrun(run, sink);
        }
    }
    __syncthreads();
    const int nt = s.Ss == 0 && g.nchroma > 0 ? 2 : 1;
    for (int j = threadIdx.x; j < nt * kJhSymbols; j += kJfpThreads) {
        unsigned n = 0;
        for (int w = 0; w < kWaves; w++) n += (&cnt[w][0][0])[j];
        if (n) atomicAdd(hist + (seg * g.ntab + s.tbl) * kJhSymbols + j, (unsigned long long)n);
    }
}

// one workgroup per file, one wave per table: the table (jh_build, serial on the wave's first lane with its work arrays in LDS) and
// its codes; then one wave per scan: the markers before the scan's data -- the DHT of the tables it is the first to use, and its SOS
__global__ __launch_bounds__(kJfpMaxTables * 64) void k_jfp_tables(JfpGeom g, const unsigned long long *__restrict__ hist, unsigned *__restrict__ codes,
                                                                   unsigned char *__restrict__ fhdr, int *__restrict__ fhdr_len)
{
    __shared__ JhWork work[kJfpMaxTables];
    __shared__ unsigned char bits[kJfpMaxTables][16], vals[kJfpMaxTables][256];
    __shared__ int nsym[kJfpMaxTables];
    const long long seg = blockIdx.x;
    const int t = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    if (t < g.ntab) {
        unsigned *tc = codes + (seg * g.ntab + t) * 256;
        for (int i = lane; i < 256; i += 64) {
            work[t].freq[i] = (long long)hist[(seg * g.ntab + t) * kJhSymbols + i];
            tc[i] = 0;
        }
    }
    __syncthreads();
    if (t < g.ntab && lane == 0) {
        nsym[t] = jh_build(work[t], bits[t], vals[t]);
        jh_codes(bits[t], vals[t], codes + (seg * g.ntab + t) * 256);
    }
    __syncthreads();
    for (int si = t; si < g.nscan; si += nwaves) {
        const JfpScan &s = g.sc[si];
        unsigned char *o = fhdr + (seg * g.nscan + si) * kJfpPiece;
        int off = 0;
        const int ntables = g.raw ? 0 : s.Ss > 0 ? 1 : s.Ah ? 0 : 1 + (g.nchroma > 0);
        for (int u = 0; u < ntables; u++) {
            const int tb = s.tbl + u, n = nsym[tb];
            if (off + 5 + 16 + n + kJrDriBytes + 14 > kJfpPiece) break;      // never: a DC table holds at most 17 symbols, an AC table 256
            if (lane == 0) {
                o[off] = 0xFF; o[off + 1] = 0xC4; o[off + 2] = (unsigned char)((19 + n) >> 8); o[off + 3] = (unsigned char)((19 + n) & 255);
                o[off + 4] = (unsigned char)(s.Ss == 0 ? u : 0x10 | (s.comp > 0 ? 1 : 0));
            }
            for (int i = lane; i < 16 + n; i += 64) o[off + 5 + i] = i < 16 ? bits[tb][i] : vals[tb][i - 16];
            off += 5 + 16 + n;
        }
        if (!g.raw) {
            const int nc = s.Ss == 0 ? 1 + g.nchroma : 1;
            if (s.dri) {                                     // the scan's interval differs from the one before: a DRI after its tables
                if (lane == 0) jr_dri(o + off, s.R);
                off += kJrDriBytes;
            }
            if (lane == 0) {
                unsigned char *q = o + off;
                q[0] = 0xFF; q[1] = 0xDA; q[2] = 0; q[3] = (unsigned char)(6 + 2 * nc); q[4] = (unsigned char)nc;
                for (int c = 0; c < nc; c++) {               // libjpeg zeroes the selector of a table the scan does not use
                    q[5 + 2 * c] = (unsigned char)(s.Ss == 0 ? c + 1 : (s.comp < 0 ? 0 : s.comp) + 1);
                    q[6 + 2 * c] = (unsigned char)(s.Ss == 0 ? (s.Ah || c == 0 ? 0 : 0x10) : (s.comp > 0 ? 1 : 0));
                }
                q[5 + 2 * nc] = (unsigned char)s.Ss; q[6 + 2 * nc] = (unsigned char)s.Se; q[7 + 2 * nc] = (unsigned char)((s.Ah << 4) | s.Al);
            }
            off += 8 + 2 * nc;
        }
        if (lane == 0) fhdr_len[seg * g.nscan + si] = off;
    }
}

// the tables of scan s of file seg into LDS: one table, or the two DC tables of the first scan ([2][256], (code << 8) | length).  Every
// thread of the workgroup calls it (it holds the barrier).
__device__ __forceinline__ void jfp_stage_codes(const JfpGeom &g, const JfpScan &s, long long seg, const unsigned *__restrict__ codes, unsigned *lds)
{
    const int n = s.Ss == 0 ? (s.Ah ? 0 : g.nchroma > 0 ? 512 : 256) : 256;
    const unsigned *src = codes + (seg * g.ntab + s.tbl) * 256;
    for (int j = threadIdx.x; j < n; j += kJfpThreads) lds[j] = src[j];
    __syncthreads();
}

// item i of scan s into a sink that reads the scan's codes (the LDS copy): own symbols, the EOBn of the piece it opens, its deferred bits
template <class Sink>
__device__ __forceinline__ void jfp_item(const JfpGeom &g, const JfpScan &s, long long seg, long long i, const short *coef, const int *plen,
                                         const unsigned *codes, Sink &sink)
{
    const short *base = coef + seg * g.nblk * 64;
    if (s.Ss == 0) {
        if (s.Ah) {
            je_dc_refine(base[i * 64], s.Al, sink);
        } else {
            bool chroma;
            const int pred = jfp_dc_pred(g, s, base, i, &chroma);
            sink.codes = codes + (chroma ? 256 : 0);
            je_dc_first(base[i * 64], pred, s.Al, sink);
        }
        return;
    }
    sink.codes = codes;
    const short *c = base + jfp_coef_block(g, s, i) * 64;
    const JeBlock b = s.Ah ? je_ac_refine(c, s.Ss, s.Se, s.Al, sink) : je_ac_first(c, s.Ss, s.Se, s.Al, sink);
    const int run = plen[seg * g.T + s.ioff + i];
    if (run > 0) je_eobrun(run, sink);
    sink.many(b.brbits, b.br);
}

__global__ __launch_bounds__(kJfpThreads) void k_jfp_count(JfpGeom g, const short *__restrict__ coef, const int *__restrict__ plen,
                                                           const unsigned *__restrict__ codes, int *__restrict__ lens)
{
    __shared__ unsigned lc[512];
    const JfpScan s = g.sc[blockIdx.y];
    const long long i = (long long)blockIdx.x * kJfpThreads + threadIdx.x, seg = blockIdx.z;
    if ((long long)blockIdx.x * kJfpThreads >= s.n) return;  // uniform over the workgroup
    jfp_stage_codes(g, s, seg, codes, lc);
    if (i >= s.n) return;
    JeLen sink{ nullptr, 0 };
    jfp_item(g, s, seg, i, coef, plen, lc, sink);
    lens[seg * g.T + s.ioff + i] = sink.total;
}

// every item's code string at its bit offset, boundary words by atomicOr
__global__ __launch_bounds__(kJfpThreads) void k_jfp_emit(JfpGeom g, const short *__restrict__ coef, const int *__restrict__ plen,
                                                          const unsigned *__restrict__ codes, const unsigned long long *__restrict__ pre,
                                                          const unsigned long long *__restrict__ ivpre, unsigned *__restrict__ stream)
{
    __shared__ unsigned lc[512];
    const JfpScan s = g.sc[blockIdx.y];
    const long long i = (long long)blockIdx.x * kJfpThreads + threadIdx.x, seg = blockIdx.z;
    if ((long long)blockIdx.x * kJfpThreads >= s.n) return;  // uniform over the workgroup
    jfp_stage_codes(g, s, seg, codes, lc);
    if (i >= s.n) return;
    const unsigned long long *p = pre + seg * (g.T + 1) + s.ioff;
    JrPlace at{ (long long)(p[i] - p[0]), (long long)(p[s.n] - p[0]), i == s.n - 1 };
    if (s.R) at = jr_place(i, s.per, s.n, p, ivpre + seg * (g.NIV + 1) + s.ivoff);      // uniform: inside its byte-aligned restart interval
    JeEmit sink{ nullptr, JeBits(stream + seg * g.stream_words + s.woff, at.pos, s.wcap) };
    jfp_item(g, s, seg, i, coef, plen, lc, sink);
    if (at.last) sink.bw.pad_ones(at.total);                 // the last byte of the scan (of every restart interval) is padded with 1-bits
    sink.bw.finish();
}

// grid of the per-chunk kernels: (chunks of a file, file)
__global__ __launch_bounds__(kJfpThreads) void k_jfp_zero(JfpGeom g, const unsigned long long *__restrict__ pre,
                                                         const unsigned long long *__restrict__ ivpre, unsigned *__restrict__ stream)
{
    const long long seg = blockIdx.y, ch = (long long)blockIdx.x * kJfpThreads + threadIdx.x;
    if (ch >= g.n_chunks) return;
    const JfpScan &s = g.sc[jfp_chunk_scan(g, ch)];
    const long long used = min(s.wcap, (jfp_scan_bytes(g, pre, ivpre, seg, s) + 3) >> 2), lo = (ch - s.coff) * (kJfpChunk / 4);
    unsigned *w = stream + seg * g.stream_words + s.woff;
    for (long long j = lo; j < min(used, lo + kJfpChunk / 4); j++) w[j] = 0;
}

__global__ __launch_bounds__(kJfpThreads) void k_jfp_ffcount(JfpGeom g, const unsigned long long *__restrict__ pre,
                                                             const unsigned long long *__restrict__ ivpre, const unsigned *__restrict__ stream,
                                                             int *__restrict__ cnt)
{
    const long long seg = blockIdx.y, ch = (long long)blockIdx.x * kJfpThreads + threadIdx.x;
    if (ch >= g.n_chunks) return;
    const JfpScan &s = g.sc[jfp_chunk_scan(g, ch)];
    const long long nbytes = min(s.wcap * 4, jfp_scan_bytes(g, pre, ivpre, seg, s));
    const long long lo = (ch - s.coff) * kJfpChunk, hi = min(nbytes, lo + kJfpChunk);
    const unsigned char *src = reinterpret_cast<const unsigned char *>(stream + seg * g.stream_words + s.woff);
    cnt[seg * g.n_chunks + ch] = js_stuff_count(src, lo, hi);
}

// the bytes of file seg before the markers of scan si (si == nscan: before EOI)
__device__ __forceinline__ long long jfp_file_pos(const JfpGeom &g, const JfifParams *par, const int *fhdr_len, const unsigned long long *pre,
                                                  const unsigned long long *ivpre, const unsigned long long *ffpre, long long seg, int si)
{
    long long pos = g.raw ? 0 : par[seg / g.B].dht_off;
    const unsigned long long *ff = ffpre + seg * (g.n_chunks + 1);
    for (int u = 0; u < si; u++) {
        const JfpScan &s = g.sc[u];
        const long long last = u + 1 < g.nscan ? g.sc[u + 1].coff : g.n_chunks;
        pos += fhdr_len[seg * g.nscan + u] + jfp_scan_bytes(g, pre, ivpre, seg, s) + (long long)(ff[last] - ff[s.coff]) +
               (g.NIV ? 2 * (s.niv - 1) : 0);                // an RSTn before every interval but the first
    }
    return pos;
}

__global__ __launch_bounds__(kJfpThreads) void k_jfp_layout(JfpGeom g, const JfifParams *__restrict__ par, const int *__restrict__ fhdr_len,
                                                            const unsigned long long *__restrict__ pre, const unsigned long long *__restrict__ ivpre,
                                                            const unsigned long long *__restrict__ ffpre, long long *__restrict__ lengths,
                                                            long long *__restrict__ offsets, long long *__restrict__ total)
{
    // every thread sizes its share of the files, thread 0 lays them out in (quality, image) order
    for (long long seg = threadIdx.x; seg < g.segs; seg += kJfpThreads)
        lengths[seg] = jfp_file_pos(g, par, fhdr_len, pre, ivpre, ffpre, seg, g.nscan) + (g.raw ? 0 : 2);
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long off = 0;
    for (long long seg = 0; seg < g.segs; seg++) {
        offsets[seg] = off;
        off += lengths[seg];
    }
    *total = off;
}

__global__ __launch_bounds__(kJfpThreads) void k_jfp_scatter(JfpGeom g, const JfifParams *__restrict__ par, const unsigned char *__restrict__ fhdr,
                                                             const int *__restrict__ fhdr_len, const unsigned long long *__restrict__ pre,
                                                             const unsigned long long *__restrict__ ivpre, const unsigned *__restrict__ stream,
                                                             const unsigned long long *__restrict__ ffpre,
                                                             const long long *__restrict__ lengths, const long long *__restrict__ offsets,
                                                             unsigned char *__restrict__ out, unsigned long long cap)
{
    const long long seg = blockIdx.y, ch = (long long)blockIdx.x * kJfpThreads + threadIdx.x;
    if (ch >= g.n_chunks) return;
    const long long off = offsets[seg], len = lengths[seg];
    if (off < 0 || len < 0 || (unsigned long long)(off + len) > cap) return;
    const int si = jfp_chunk_scan(g, ch);
    const JfpScan &s = g.sc[si];
    const long long nbytes = min(s.wcap * 4, jfp_scan_bytes(g, pre, ivpre, seg, s));
    const long long lo = (ch - s.coff) * kJfpChunk, hi = min(nbytes, lo + kJfpChunk);
    if (lo > 0 && lo >= hi) return;
    unsigned char *file = out + off;
    const int hl = fhdr_len[seg * g.nscan + si];
    const long long at = jfp_file_pos(g, par, fhdr_len, pre, ivpre, ffpre, seg, si);
    if (lo == 0) {                                           // the scan's first chunk also writes the markers before it
        const unsigned char *h = fhdr + (seg * g.nscan + si) * kJfpPiece;
        for (int j = 0; j < hl; j++) file[at + j] = h[j];
        if (si == 0 && !g.raw) {
            const JfifParams &p = par[seg / g.B];
            for (int j = 0; j < p.dht_off; j++) file[j] = p.hdr[j];
            file[len - 2] = 0xFF;
            file[len - 1] = 0xD9;
        }
    }
    const unsigned long long *ff = ffpre + seg * (g.n_chunks + 1);
    const unsigned char *src = reinterpret_cast<const unsigned char *>(stream + seg * g.stream_words + s.woff);
    unsigned char *dst = file + at + hl + lo + (long long)(ff[ch] - ff[s.coff]);
    // uniform: with restarts the markers before this chunk shift it, those inside it are written here
    jr_stuff_chunk(dst, src, lo, hi, s.R ? ivpre + seg * (g.NIV + 1) + s.ivoff : nullptr, s.R ? s.niv : 0);
}

// restarts: k_js_scan's input for the intervals' starts -- interval i of the launch (file after file, scan after scan inside a file),
// its items' bits (from the bit prefix sums) rounded up to bytes
struct JfpIntervalBytes {
    const unsigned long long *pre;
    JfpGeom g;
    __device__ __forceinline__ unsigned long long operator()(long long i) const
    {
        const long long seg = i / g.NIV, j = i % g.NIV;
        int si = 0;
        while (si + 1 < g.nscan && j >= g.sc[si + 1].ivoff) si++;
        const JfpScan &s = g.sc[si];
        const unsigned long long *p = pre + seg * (g.T + 1) + s.ioff;
        const long long lo = (j - s.ivoff) * s.per, hi = min(lo + s.per, s.n);
        return (p[hi] - p[lo] + 7) >> 3;
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static void jfp_finish_geom(JfpGeom &p)
{
    long long ioff = 0, woff = 0, ivoff = 0;
    p.nmax = 0;
    for (int i = 0; i < p.nscan; i++) {
        JfpScan &s = p.sc[i];
        s.ioff = ioff;
        s.woff = woff;
        s.coff = woff / (kJfpChunk / 4);
        s.niv = s.R ? jr_count(s.n, (int)s.per) : 0;         // (per <= 6 x 65535)
        s.ivoff = ivoff;
        ivoff += s.niv;
        // je_block_bound is exact for some scans (a DC refinement item is one bit), so the 1-bits that pad every restart interval to a
        // byte, up to 7 per interval, are counted on their own
        s.wcap = ((s.n * je_block_bound(s.Ss, s.Se, s.Ah) + 7 * s.niv + 31) / 32 + 2 + 15) / 16 * 16;
        ioff += s.n;
        woff += s.wcap;
        p.nmax = std::max(p.nmax, s.n);
    }
    p.T = ioff;
    p.NIV = ivoff;
    p.stream_words = woff;
    p.n_chunks = woff / (kJfpChunk / 4);
}

// the restart interval of every scan of the script: its own MCUs per row (an interleaved scan mcux, a single-component scan the
// component's blocks per row), a DRI where it differs from the last one written (0 before the first scan)
static void jfp_restarts(const JfifGeom &g, JfpGeom &p, int blocks, int rows)
{
    int written = 0;
    for (int i = 0; i < p.nscan; i++) {
        JfpScan &s = p.sc[i];
        const bool inter = s.comp < 0;
        s.R = jr_interval(blocks, rows, inter || s.comp > 0 ? g.mcux : g.ybx);
        s.per = (long long)s.R * (inter ? p.hs * p.vs + p.nchroma : 1);
        s.dri = s.R != written;
        written = s.R;
    }
}

bool jfifprog_geom(const JfifGeom &g, JfpGeom &p, int blocks, int rows)
{
    if ((long long)g.nq * g.B > 65535) return false;         // files index grid.z
    if (blocks < 0 || blocks > kJrMaxInterval || rows < 0 || rows > kJrMaxInterval) return false;
    p = JfpGeom{};
    p.segs = g.nq * g.B; p.B = g.B; p.hs = g.hs; p.vs = g.vs; p.nchroma = 2; p.mcux = g.mcux; p.ybx = g.ybx;
    p.nscan = kJfpMaxScans; p.ntab = kJfpMaxTables; p.raw = 0; p.nblk = g.nblk;
    if (g.ncomp == 1) {                                      // slot 0 the DC table, 1 .. 4 one per AC scan; every scan walks the nblk real blocks
        static const int grey[6][6] = { { -1, 0, 0, 0, 1, 0 }, { 0, 1, 5, 0, 2, 1 }, { 0, 6, 63, 0, 2, 2 }, { 0, 1, 63, 2, 1, 3 }, { -1, 0, 0, 1, 0, 0 },
                                        { 0, 1, 63, 1, 0, 4 } };
        p.nchroma = 0; p.nscan = 6; p.ntab = 5;
        for (int i = 0; i < p.nscan; i++) {
            JfpScan &s = p.sc[i];
            s.comp = grey[i][0]; s.Ss = grey[i][1]; s.Se = grey[i][2]; s.Ah = grey[i][3]; s.Al = grey[i][4]; s.tbl = grey[i][5];
            s.n = g.nblk;
        }
        jfp_restarts(g, p, blocks, rows);
        jfp_finish_geom(p);
        return true;
    }
    // jpeg_simple_progression: { component, Ss, Se, Ah, Al, first table slot }; slots 0 / 1 the DC tables, 2 .. 9 one per AC scan
    static const int script[kJfpMaxScans][6] = { { -1, 0, 0, 0, 1, 0 }, { 0, 1, 5, 0, 2, 2 }, { 2, 1, 63, 0, 1, 3 }, { 1, 1, 63, 0, 1, 4 },
                                                 { 0, 6, 63, 0, 2, 5 }, { 0, 1, 63, 2, 1, 6 }, { -1, 0, 0, 1, 0, 0 }, { 2, 1, 63, 1, 0, 7 },
                                                 { 1, 1, 63, 1, 0, 8 }, { 0, 1, 63, 1, 0, 9 } };
    for (int i = 0; i < kJfpMaxScans; i++) {
        JfpScan &s = p.sc[i];
        s.comp = script[i][0]; s.Ss = script[i][1]; s.Se = script[i][2]; s.Ah = script[i][3]; s.Al = script[i][4]; s.tbl = script[i][5];
        s.n = s.comp < 0 ? g.nblk : s.comp == 0 ? (long long)g.ybx * g.yby : g.n_mcu;
    }
    jfp_restarts(g, p, blocks, rows);
    jfp_finish_geom(p);
    return true;
}

static void jfp_carve(Carver &c, const JfpGeom &p, JfpBufs &pw)
{
    const long long segs = p.segs;
    pw.flags = c.take<unsigned short>(segs * p.T);
    pw.pre = c.take<unsigned long long>(segs * (p.T + 1));
    pw.plen = c.take<int>(segs * p.T);
    pw.lens = c.take<int>(segs * p.T);
    pw.stream = c.take<unsigned>(segs * p.stream_words);
    pw.ffcnt = c.take<int>(segs * p.n_chunks);
    pw.ffpre = c.take<unsigned long long>(segs * (p.n_chunks + 1));
    pw.hist = c.take<unsigned long long>(segs * p.ntab * kJhSymbols);
    pw.codes = c.take<unsigned>(segs * p.ntab * 256);
    pw.fhdr = c.take<unsigned char>(segs * p.nscan * kJfpPiece);
    pw.fhdr_len = c.take<int>(segs * p.nscan);
    pw.cuts = c.take<int>(segs * p.nscan * 2);
    pw.total = c.take<long long>(1);
    pw.ivpre = p.NIV ? c.take<unsigned long long>(segs * (p.NIV + 1)) : nullptr;
}

// the workspace: what colour .. quantisation and the reconstruction use of JfifBufs (the baseline coder's buffers are not carved;
// k_jfif_quant's Annex K bit counts land in pw.lens, which holds T >= nblk entries per file), then JfpBufs
unsigned long long jfifprog_carve(void *base, const JfifGeom &g, const JfpGeom &p, JfifBufs &w, JfpBufs &pw)
{
    Carver c(base);
    const long long segs = (long long)g.nq * g.B;
    w = JfifBufs{};
    w.par = c.take<JfifParams>(g.nq);
    w.dct = c.take<int>((long long)g.B * g.nblk * 64);
    w.coef = c.take<short>(segs * g.nblk * 64);
    w.planes = c.take<unsigned char>(segs * g.plane_bytes);
    jfp_carve(c, p, pw);
    w.lens = pw.lens;
    w.total = pw.total;
    return c.bytes();
}

// the transcoder's workspace of one group of files: their markers and coefficients, then JfpBufs (no colour, DCT or sample planes)
unsigned long long jfifprog_carve_coded(Carver &c, const JfifGeom &g, const JfpGeom &p, JfifBufs &w, JfpBufs &pw)
{
    w = JfifBufs{};
    w.par = c.take<JfifParams>(g.nq);
    w.coef = c.take<short>((long long)g.nq * g.B * g.nblk * 64);
    jfp_carve(c, p, pw);
    w.lens = pw.lens;
    w.total = pw.total;
    return c.bytes();
}

static unsigned jfp_blocks(long long n) { return (unsigned)((n + kJfpThreads - 1) / kJfpThreads); }

// every stage after quantisation
static hipError_t jfp_entropy(hipStream_t st, const JfpGeom &p, const JfpBufs &pw, const short *coef, const JfifParams *par, unsigned char *out,
                              unsigned long long cap, long long *lengths, long long *offsets)
{
    const unsigned segs = (unsigned)p.segs;
    const dim3 items(jfp_blocks(p.nmax), (unsigned)p.nscan, segs), chunks(jfp_blocks(p.n_chunks), segs), th(kJfpThreads);
    hipError_t e = hipMemsetAsync(pw.plen, 0, (size_t)p.segs * p.T * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(pw.hist, 0, (size_t)p.segs * p.ntab * kJhSymbols * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(pw.cuts, 0, (size_t)p.segs * p.nscan * 2 * 4, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_jfp_facts, items, th, 0, st, p, coef, pw.flags);
    hipLaunchKernelGGL(k_js_scan<JfpPacked>, dim3(segs), dim3(kJsScanThreads), 0, st, JfpPacked{ pw.flags }, p.T, pw.pre);
    hipLaunchKernelGGL(k_jfp_cuts, items, th, 0, st, p, pw.flags, pw.pre, pw.plen, pw.cuts);
    hipLaunchKernelGGL(k_jfp_hist, items, th, 0, st, p, coef, pw.plen, pw.hist);
    hipLaunchKernelGGL(k_jfp_tables, dim3(segs), dim3(64 * p.ntab), 0, st, p, pw.hist, pw.codes, pw.fhdr, pw.fhdr_len);
    hipLaunchKernelGGL(k_jfp_count, items, th, 0, st, p, coef, pw.plen, pw.codes, pw.lens);
    hipLaunchKernelGGL(k_js_scan<JsInts>, dim3(segs), dim3(kJsScanThreads), 0, st, JsInts{ pw.lens }, p.T, pw.pre);
    if (p.NIV) {                                             // the byte starts of the restart intervals: a second prefix sum, over their byte lengths
        if (!pw.ivpre) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_js_scan<JfpIntervalBytes>, dim3(segs), dim3(kJsScanThreads), 0, st, JfpIntervalBytes{ pw.pre, p }, p.NIV, pw.ivpre);
    }
    hipLaunchKernelGGL(k_jfp_zero, chunks, th, 0, st, p, pw.pre, pw.ivpre, pw.stream);
    hipLaunchKernelGGL(k_jfp_emit, items, th, 0, st, p, coef, pw.plen, pw.codes, pw.pre, pw.ivpre, pw.stream);
    hipLaunchKernelGGL(k_jfp_ffcount, chunks, th, 0, st, p, pw.pre, pw.ivpre, pw.stream, pw.ffcnt);
    hipLaunchKernelGGL(k_js_scan<JsInts>, dim3(segs), dim3(kJsScanThreads), 0, st, JsInts{ pw.ffcnt }, p.n_chunks, pw.ffpre);
    hipLaunchKernelGGL(k_jfp_layout, dim3(1), th, 0, st, p, par, pw.fhdr_len, pw.pre, pw.ivpre, pw.ffpre, lengths, offsets, pw.total);
    return out ? launch_jfifprog_scatter(st, p, pw, par, lengths, offsets, out, cap) : hipGetLastError();
}

hipError_t launch_jfifprog_scatter(hipStream_t st, const JfpGeom &p, const JfpBufs &pw, const JfifParams *par, const long long *lengths,
                                   const long long *offsets, unsigned char *out, unsigned long long cap)
{
    hipLaunchKernelGGL(k_jfp_scatter, dim3(jfp_blocks(p.n_chunks), (unsigned)p.segs), dim3(kJfpThreads), 0, st, p, par, pw.fhdr, pw.fhdr_len, pw.pre,
                       pw.ivpre, pw.stream, pw.ffpre, lengths, offsets, out, cap);
    return hipGetLastError();
}

// the transcoder's cut (jfiftrans.hip): every stage after quantisation up to the lengths, from coefficients and markers (par, device)
// the caller has put in place
hipError_t launch_jfifprog_entropy(hipStream_t st, const JfpGeom &p, const JfpBufs &pw, const short *coef, const JfifParams *par, long long *lengths,
                                   long long *offsets)
{
    return jfp_entropy(st, p, pw, coef, par, nullptr, 0, lengths, offsets);
}

hipError_t launch_jfifprog_encode(hipStream_t st, const JfifGeom &g, const JfpGeom &p, const JfifBufs &w, const JfpBufs &pw,
                                  const JfifParams *par_host, const unsigned char *rgb, unsigned char *out, unsigned long long cap,
                                  long long *lengths, long long *offsets)
{
    const hipError_t e = launch_jfif_coefs(st, g, w, par_host, rgb);
    if (e != hipSuccess) return e;
    return jfp_entropy(st, p, pw, w.coef, w.par, out, cap, lengths, offsets);
}

// ---- the testing entries: one scan over given coefficients ----------------------------------------------------------------------------
static bool jfp_scan_args(const short *coefs, long long n, int Ss, int Se, int Ah, int Al)
{
    if (!coefs || n < 1 || n > (1LL << 24) || Ss < 0 || Se > 63 || Ss > Se || (Ss == 0) != (Se == 0) || Al < 0 || Al > 13 || Ah < 0 || Ah > 13) return false;
    if (Ah != 0 && Ah != Al + 1) return false;
    for (long long i = 0; i < n * 64; i++)
        if (coefs[i] > kJeMaxCoef || coefs[i] < -kJeMaxCoef) return false;
    return true;
}

int jfifprog_scan_host(const short *coefs, long long n, int Ss, int Se, int Ah, int Al, unsigned char *out, unsigned long long cap,
                       unsigned long long *out_len, long long *counts, long long *cuts)
{
    if (!jfp_scan_args(coefs, n, Ss, Se, Ah, Al) || !out_len || !counts || !cuts) return AEJ_ERR_ARG;
    for (int i = 0; i < kJhSymbols; i++) counts[i] = 0;
    cuts[0] = cuts[1] = 0;
    std::vector<int> plen(n, 0);
    JeHist<unsigned long long> cs{ reinterpret_cast<unsigned long long *>(counts) };      // (the counts are not negative)
    auto block = [&](long long i, auto &sink) {              // item i as the kernels code it
        const short *c = coefs + i * 64;
        if (Ss == 0) {
            if (Ah) je_dc_refine(c[0], Al, sink); else je_dc_first(c[0], i ? c[-64] : 0, Al, sink);
            return;
        }
        const JeBlock b = Ah ? je_ac_refine(c, Ss, Se, Al, sink) : je_ac_first(c, Ss, Se, Al, sink);
        if (plen[i] > 0) je_eobrun(plen[i], sink);
        sink.many(b.brbits, b.br);
    };
    if (Ss > 0) {                                            // facts, prefix sums, cuts
        std::vector<unsigned long long> P(n + 1, 0);
        std::vector<unsigned char> joins(n), emits(n);
        JeNull nul;
        for (long long i = 0; i < n; i++) {
            const JeBlock b = Ah ? je_ac_refine(coefs + i * 64, Ss, Se, Al, nul) : je_ac_first(coefs + i * 64, Ss, Se, Al, nul);
            joins[i] = b.r > 0 || b.br > 0;
            emits[i] = (unsigned char)b.e;
            P[i + 1] = P[i] + je_pack(i == 0, b.e != 0, i ? joins[i - 1] != 0 : false, b.br);
        }
        for (long long i = 0; i < n; i++) {
            if (!joins[i] || !((P[i + 1] - P[i]) >> kJeBrShift)) continue;
            const long long ce = je_chain_end(P.data(), i, n);
            for (long long p = i; p < ce;) {
                int why;
                const long long q = je_piece_end(P.data(), p, ce, &why);
                plen[p] = (int)(q - p);
                if (why) cuts[why - 1]++;
                p = q;
            }
        }
    }
    for (long long i = 0; i < n; i++) block(i, cs);
    unsigned codes[256] = { 0 };
    if (!(Ss == 0 && Ah)) {
        JhWork w;
        unsigned char bits[16], vals[256];
        for (int i = 0; i < 256; i++) w.freq[i] = counts[i];
        jh_build(w, bits, vals);
        jh_codes(bits, vals, codes);
    }
    std::vector<long long> pos(n + 1, 0);
    for (long long i = 0; i < n; i++) {
        JeLen len{ codes, 0 };
        block(i, len);
        pos[i + 1] = pos[i] + len.total;
    }
    const long long nbytes = (pos[n] + 7) >> 3, limit = (nbytes + 3) / 4 + 1;
    std::vector<unsigned> words(limit, 0);
    for (long long i = 0; i < n; i++) {
        JeEmit em{ codes, JeBits(words.data(), pos[i], limit) };
        block(i, em);
        if (i == n - 1) em.bw.pad_ones(pos[n]);
        em.bw.finish();
    }
    const unsigned char *src = reinterpret_cast<const unsigned char *>(words.data());
    const unsigned long long o = (unsigned long long)(nbytes + js_stuff_count(src, 0, nbytes));
    *out_len = o;
    if (o > cap || (o && !out)) return AEJ_ERR_CAPACITY;
    js_stuff_copy(out, src, 0, nbytes);
    return 0;
}

int jfifprog_scan_device(hipStream_t st, const short *coefs_host, long long n, int Ss, int Se, int Ah, int Al, unsigned char *out_host,
                         unsigned long long cap, unsigned long long *out_len, long long *counts, long long *cuts, hipError_t *err)
{
    *err = hipSuccess;
    if (!jfp_scan_args(coefs_host, n, Ss, Se, Ah, Al) || !out_len || !counts || !cuts) return AEJ_ERR_ARG;
    JfpGeom p{};
    p.segs = 1; p.B = 1; p.hs = p.vs = 1; p.nchroma = 0; p.mcux = 1; p.ybx = 1; p.nscan = 1; p.ntab = 1; p.raw = 1; p.nblk = n;
    p.sc[0] = JfpScan{ Ss, Se, Ah, Al, -1, 0, n, 0, 0, 0, 0 };
    jfp_finish_geom(p);
    JfpBufs pw;
    const unsigned long long out_cap = (unsigned long long)p.stream_words * 8;
    short *coef = nullptr;
    unsigned char *out = nullptr;
    long long *lengths = nullptr;
    auto carve = [&](void *b) {      // the coefficients, the output and its length / offset words, then JfpBufs
        Carver c(b);
        coef = c.take<short>(n * 64);
        out = c.take<unsigned char>((long long)out_cap);
        lengths = c.take<long long>(2);
        jfp_carve(c, p, pw);
        return c.bytes();
    };
    char *base = nullptr;
    hipError_t e = hipMalloc((void **)&base, carve(nullptr));
    if (e != hipSuccess) { *err = e; return AEJ_ERR_HIP; }
    carve(base);
    long long *offsets = lengths + 1;
    long long len = 0;
    int cut32[2] = { 0, 0 };
    std::vector<unsigned long long> hist(kJhSymbols);
    e = hipMemcpyAsync(coef, coefs_host, (size_t)n * 128, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = jfp_entropy(st, p, pw, coef, nullptr, out, out_cap, lengths, offsets);
    if (e == hipSuccess) e = hipMemcpyAsync(&len, lengths, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cut32, pw.cuts, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hist.data(), pw.hist, kJhSymbols * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    int rc = 0;
    if (e == hipSuccess) {
        *out_len = (unsigned long long)len;
        cuts[0] = cut32[0]; cuts[1] = cut32[1];
        for (int i = 0; i < kJhSymbols; i++) counts[i] = (long long)hist[i];
        if ((unsigned long long)len > cap || (len && !out_host)) rc = AEJ_ERR_CAPACITY;
        else if (len) e = hipMemcpy(out_host, out, (size_t)len, hipMemcpyDeviceToHost);
    }
    const hipError_t e2 = hipFree(base);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { *err = e; return AEJ_ERR_HIP; }
    return rc;
}

}  // namespace aej
