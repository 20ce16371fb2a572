// aej_launch.h -- host-side launch functions exported by the .hip translation units.
#pragma once
#include "aej_common.h"
#include "aej_spans.h"

namespace aej {

// DEVICE: index of the last of n entries with base(entry) <= t (entries sorted by base, entry 0 at or below every t asked for): how a
// workgroup, wave or lane of a grid laid over many images finds its own
template <class E, class T, class Base>
__device__ __forceinline__ int find_last(const E *f, int n, T t, Base base)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (base(f[mid]) <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// the same for the tile kernels: the entry whose workgroups (from its tile_base on) contain blockIdx.x.  (`Here` reads blockIdx.x
// in the comparison, where the loops this replaces read it: handing find_last its value instead changes the code the compiler emits
// for the kernels of filter.hip, window.hip and warp.hip -- EXPERIMENTS.md, "One binary search on the device")
template <class E>
__device__ __forceinline__ const E &tile_entry(const E *__restrict__ e, int n)
{
    struct Here { __device__ __forceinline__ operator long long() const { return (long long)blockIdx.x; } };
    return e[find_last(e, n, Here(), [](const E &x) { return x.tile_base; })];
}
// and for the chunk kernels: the entry whose chunks (from its chunk_base on) contain `chunk`
template <class E>
__device__ __forceinline__ const E &chunk_entry(const E *__restrict__ e, int n, long long chunk)
{
    return e[find_last(e, n, chunk, [](const E &x) { return x.chunk_base; })];
}

// color.hip
int launch_color_convert(hipStream_t st, int space, const float *rgb, float *out, long long n);
// whether the encode path may keep this geometry's normalised planes in 4 x 4 blocks (Geom::tiled): the strip kernel writes them, every DCT kernel reads both forms
bool color_planes_can_tile(const Geom &g, int space, bool in_u8, const Tuning &t);
int launch_color_planes(hipStream_t st, int space, const void *rgb, bool in_u8, const Geom &g, const float *mid, const float *scale,
                        float *raw, float *norm, unsigned char *u8, int *tile_hist, const Tuning &t);
// tables of cv.resize(INTER_AREA) for the chroma layers when the ratios are not exact 2x2 (device arrays)
struct AreaTabs {
    int mode;                  // 0: exact 2x2, 1: other integer ratios (isx, isy), 2: general tables
    int isx, isy;
    const int *xoff, *xsi, *yoff, *ysi;
    const float *xal, *yal;
};
int launch_color_planes_generic(hipStream_t st, int space, const void *rgb, bool in_u8, const Geom &g, const float *mid, const float *scale,
                                const AreaTabs &tabs, float *raw, float *norm, unsigned char *u8, int *tile_hist);
void launch_plane_u8(hipStream_t st, const float *plane, const Geom &g, unsigned char *u8, int *tile_hist);

// canny.hip
struct CannyBuffers {
    unsigned char *u8a;     // [B][pstride] scaled uint8 in; NMS / hysteresis map out
    unsigned char *u8b;     // [B][pstride] bilateral output
    int *tile_hist;         // [B][3][16][256]
    unsigned char *lut;     // [B][3][16][256]
    int *blur_hist;         // [B][3][256]
    int *thr;               // [B][3][2]
    unsigned long long *weak;    // [B][bpstride] NMS candidates (bit-plane)
    unsigned long long *strong;  // [B][bpstride] strong edges, grown by the hysteresis passes -> final edge map
    int *hflags;            // [2][B * tiles] "look at this tile again" / "queued" flags, one parity per launch of the hysteresis
    int *hlist;             // [hyst_ring_slots()] the work queue of the last launch: a ring of tile + 1 (0 = empty slot)
    int *pass_count;        // [kHystCounters] the queue's tail / head / done counters (canny.hip kQTail ...)
    const float *space_w;   // [13]
    const float *color_w;   // [256]
    // run-time hyper-parameters of EdgeDetection.canny (edge_detection.py:31-40; aej_set_canny_params)
    double low_q = 0.10 * 100, high_q = 0.30 * 100;     // np.percentile arguments
    double clip_limit = 0.75;                           // CLAHE clipLimit (<= 0: no clipping)
    int l2 = 1;                                         // cv.Canny L2gradient
    // optional stage dumps (stand-alone entry point only)
    unsigned char *dump_clahe, *dump_gauss;
};
constexpr int kHystCounters = 128;
long long hyst_tiles_per_image(const Geom &g);
int hyst_ring_slots(const Geom &g);
void launch_clahe_pad_hist(hipStream_t st, const Geom &g, const CannyBuffers &cb);
void launch_clahe_lut(hipStream_t st, const Geom &g, const CannyBuffers &cb);
void launch_clahe_blur(hipStream_t st, const Geom &g, const CannyBuffers &cb);
void launch_thresholds(hipStream_t st, const Geom &g, const CannyBuffers &cb);
void launch_sobel_nms(hipStream_t st, const Geom &g, const CannyBuffers &cb, const Tuning &t);
void launch_hysteresis(hipStream_t st, const Geom &g, const CannyBuffers &cb);      // pass over every tile + device-side drain of the work queue
void launch_zero(hipStream_t st, void *p16, size_t bytes_multiple_of_16);
void launch_bits_to_edge(hipStream_t st, const Geom &g, const unsigned long long *strong, unsigned char *edge01);
void launch_bits_to_map(hipStream_t st, const Geom &g, const unsigned long long *weak, const unsigned long long *strong, unsigned char *map);

// quadtree.hip
struct QtBuffers {
    unsigned char *pyr;     // [B][pyr_stride] (only levels >= 5 are used)
    const unsigned long long *edge_bits;   // [B][bpstride] final edge bit-plane
    int *chunk_cnt;         // [B][chunk_stride][kChunkInts]: counts, then exclusive offsets after the scan
    unsigned short *lane_code;   // [B][chunk_stride][64]: what the count pass found per lane (quadtree.hip pack_lane)
    int *leaves;            // out [B][leaf_stride][4]
    unsigned char *states;  // out [B][state_stride]
    long long *counts;      // out [B][3][4]
    LeafWork *work[kMaxSizes];   // per-size work lists (null when no DCT follows)
    int *work_count;        // [B*3][kMaxSizes] leaves per plane and size (written by the scan pass); null without DCT
    long long work_cap[kMaxSizes];
    int *overflow;          // [1] set to 1 when a capacity would be exceeded
};
void launch_qt_cells(hipStream_t st, const Geom &g, const QtGeom &q, const unsigned long long *edge_bits, const QtBuffers &qb);
void launch_pack_edge_bits(hipStream_t st, const Geom &g, const unsigned char *edge, unsigned long long *bits);
// The chunk-run kernel set (Tuning::qt_chunks; min block 4, at least 16 cells per root side): its count and emit grids cover the chunks
// whose origin lies inside the plane, a wave taking `run` consecutive ones of the sequence (image, layer, chunk row, chunk column).
struct QtRuns {
    int ncx0, ncx1, ncx2;   // chunk columns of layers 0 .. 2 that lie (partly) inside the plane
    int ncy0, ncy1, ncy2;   // chunk rows
    int nin0, nin1, nin2;   // ncx * ncy
    int per_image, total;   // in-plane chunks of one image / of the call
    int run;                // chunks per wave
};
bool qt_chunk_runs(const Geom &g, const QtGeom &q, const Tuning &t, QtRuns &r);      // false: the general kernels serve this call
bool qt_needs_upper(const Geom &g, const QtGeom &q);      // k_qt_upper runs, and QtBuffers::pyr has to be zero in front of it
// runs: what qt_chunk_runs() gave for this call, or null for the general kernels (decided once per call, by run_quadtree)
void launch_qt_count(hipStream_t st, const Geom &g, const QtGeom &q, const QtBuffers &qb, const QtRuns *runs);      // (the chunk-run count kernel clears qb.overflow)
void launch_qt_scan(hipStream_t st, const Geom &g, const QtGeom &q, const QtBuffers &qb, const QtRuns *runs);
void launch_qt_emit(hipStream_t st, const Geom &g, const QtGeom &q, const QtBuffers &qb, const QtRuns *runs);

// dct.hip
constexpr int kBigBlocks = 128;      // workgroups (and scratch slots of 256 KiB) of the 256 x 256 kernels
constexpr int kMaxBlock = 1024;      // largest block size with a kernel (the reference takes any power of two, jpeg.py:216-219; its GUI stops at 256)
// sizes >= 256 run one workgroup per leaf with the first product in a global scratch slot of S x S floats per workgroup
constexpr int big_blocks(int S) { return S <= 256 ? kBigBlocks : S == 512 ? 64 : 32; }
constexpr long long big_scratch_floats_for(int S) { return S >= 256 ? (long long)big_blocks(S) * S * S : 0; }
struct DctArgs {
    const float *norm;        // [B][pstride] normalised planes
    int *coeffs;              // out [B][coeff_stride]
    float *dct_f32;           // optional
    const LeafWork *work;     // work lists for this size (per-plane segments, see QtGeom)
    float *scratch;           // [big_blocks(S)][S * S] intermediate product of the kernels for S >= 256 (sized for the largest S), else null
    const int *work_count;    // [nplanes][kMaxSizes]
    int k;                    // size index
    int nplanes;
    const float *D;           // [s][s]
    const int *zzinv;         // [s*s]
    const int *qm[3];         // [s*s] per layer
    int crowded = 0;          // other kernels are expected beside this launch (sub-batches, calls in flight): prefer kernels that share a CU
};
int launch_dct(hipStream_t st, int size, const Geom &g, const QtGeom &q, const DctArgs &a, long long max_items, const Tuning &t);   // 0, or -1 when no kernel serves the request
// latency-sized calls: the sizes 4 .. 64 in one launch (args / max_items indexed by size index); 0 = launched, 1 = not a call for it
int launch_dct_multi(hipStream_t st, const Geom &g, const QtGeom &q, const DctArgs *args, const long long *max_items);
// builds a work list from a leaf table (stand-alone aej_dct_quant_zigzag)
void launch_work_from_leaves(hipStream_t st, const int *leaves, long long n, int bmin, int plane, LeafWork *const *work, int *work_count);


// decode.hip
struct IdctArgs {
    const int *coeffs;        // [B][coeff_stride] zigzag-ordered quantised coefficients
    float *planes;            // out [B][pstride] de-normalised layers
    const LeafWork *work;
    float *scratch;           // [big_blocks(S)][S * S] for the kernels of S >= 256, else null
    const int *work_count;    // [nplanes][kMaxSizes]
    int k, nplanes;
    const float *D;           // [s][s]
    const int *zz, *zzinv;    // zigzag order and its inverse
    const int *qm[3];
    float mid[3], scale[3];
};
void launch_work_from_tables(hipStream_t st, const Geom &g, const QtGeom &q, const int *leaves, const long long *counts, LeafWork *const *work,
                             int *work_count, int *bad /* [1], zeroed by the caller: set when the tables do not fit the plan */);
int launch_idct(hipStream_t st, int size, const Geom &g, const QtGeom &q, const IdctArgs &a, long long max_items);
int launch_color_inverse(hipStream_t st, int space, const float *in, float *out, long long n);
int launch_upsample_color(hipStream_t st, int space, const Geom &g, const float *planes, float *rgb);

// deflate.hip -- opt-in GPU entropy stage: the layers' int32 coefficients as zlib streams (jpeg.py:588-590, 659)
unsigned long long deflate_stream_bound(unsigned long long raw_bytes);
unsigned long long deflate_workspace_bytes(int batch, const long long *coeff_cap /* [3] */);
// LZ77 match search + parse of every stream: tokens into the workspace, symbol histogram (device [3][320], may be null)
void launch_deflate_parse(hipStream_t st, const int *coeffs, const long long *counts, int batch, long long coeff_stride, const long long *coeff_off,
                          const long long *coeff_cap, int *hist, void *workspace);
// the streams from the parse in the workspace (reuse_parse) or from a fresh one
void launch_deflate(hipStream_t st, const int *coeffs, const long long *counts, int batch, long long coeff_stride, const long long *coeff_off,
                    const long long *coeff_cap, const unsigned *tables /* [3][448] or null */, int reuse_parse, unsigned char *out,
                    unsigned long long stream_stride, long long *sizes, void *workspace);
// the same stage on byte streams of mixed lengths (aej_deflate_bytes_*: png_encode_many's filtered scanlines), one zlib stream per file
constexpr int kBzGroup = 32;           // files per launch: their table travels in the kernel's arguments
struct BzFile {
    long long in_off, n_bytes;         // the stream in `in`: in_off a multiple of 4, whole dwords readable
    long long out_off, out_cap;        // its slot in `out`: both multiples of 4
    int chunk0;                        // its first chunk among the call's: the sum of deflate_bytes_chunks() of the files before it
    int bpp, stride;                   // the distances always tried: a pixel and a scanline (1 + row bytes)
    int pad;
};
struct BzGroup { BzFile f[kBzGroup]; };
long long deflate_bytes_chunks(long long n_bytes);
unsigned long long deflate_bytes_workspace_bytes(long long chunks, int n);
void launch_deflate_bytes_parse(hipStream_t st, const unsigned char *in, const BzFile *files, int n, int *hist /* device [n][320] */, void *workspace);
void launch_deflate_bytes(hipStream_t st, const unsigned char *in, const BzFile *files, int n, const unsigned *tables /* device [n][448] or null */,
                          unsigned char *out, long long *sizes /* device [n] */, void *workspace);

// inflate.hip -- zlib streams (RFC 1950 / 1951), one wave per stream.  desc: device [n][4] int64 = in_off, in_len, out_off, out_cap (bytes)
void launch_inflate(hipStream_t st, const unsigned char *src, const long long *desc, int n, unsigned char *dst, long long dst_bytes,
                    long long *out_bytes, int *status);

// headers.hip -- quadtree headers of .ajpg layers -> leaf tables and counts in the plan layout
struct HdrGeom {
    int bmin, bmax;
    int h[3], w[3];
    int proot[3];                        // root of the position walk (QtGeom::root: 2 * largest_power_of_2(max(h, w)), jpeg.py:425)
    long long leaf_off[3], leaf_span[3], leaf_stride;
    long long coeff_span[3];
};
void launch_headers(hipStream_t st, const unsigned char *states, const long long *desc, const long long *inflated, int nlayers, const HdrGeom &g,
                    unsigned char *codes, int *leaves, long long *counts, int *status);

// requant.hip -- requantisation of stored DCT values (aej_requantise_batch).  bad: device word, zeroed by the caller; the check sets it (1 leaf
// tables, 2 quantisers) and k_requant then writes nothing
void launch_requant_check(hipStream_t st, const Geom &g, const QtGeom &q, const int *leaves, const long long *counts, const int *qmats,
                          long long qmat_words, int *bad);
int launch_requant(hipStream_t st, const Geom &g, const QtGeom &q, const float *dct, const int *leaves, const long long *counts, int n_sets,
                   const int *qmats, const int *const *zz, int *out, long long set_stride, int *bad, int blocks_per_plane);

// metrics.hip.  Every partial sum is written once (no atomics) to [B][stride] doubles and k_metric_final adds an image's in a fixed order, so
// each image's scores are independent of the batch around it and of scheduling.  Per image: [0, psnr_n) the squared differences of each
// k_metric_prep block; [grey_off, + grey_n) the grey SSIM map's ssim sums; [lvl_off[l], + 3 lvl_n[l]) MS-SSIM scale l's (cs for scales 0..3,
// ssim for 4), channel-major.  An SSIM map contributes one sum per (channel, kMetricBand-row band, 128-column strip): ssim_partials().
struct MetricParts {
    long long stride;
    int psnr_n;
    long long grey_off, grey_n;         // grey_n = 0: not computed
    long long lvl_off[5], lvl_n[5];     // lvl_n[l] per channel
};
int metric_prep_blocks(long long npx);
long long ssim_partials(int h, int w);     // per channel; 0 below 11 x 11
void launch_metric_prep(hipStream_t st, const float *a, const float *b, int B, long long npx, double *part, long long stride, unsigned char *ga,
                        unsigned char *gb);
void launch_metric_pool_grey(hipStream_t st, const unsigned char *ga, const unsigned char *gb, int B, int H, int W, int f, int hp, int wp, float *xa,
                             float *xb);
void launch_ssim_level(hipStream_t st, bool interleaved, const float *xa, const float *xb, int B, int C, int h, int w, const float *g11, double *part,
                       long long stride, long long off, bool want_ss, float *pool_a = nullptr, float *pool_b = nullptr);   // pool_*: scale 0 of even-sized images also writes scale 1
void launch_pool2_rgb(hipStream_t st, const float *ia, const float *ib, int B, int h, int w, int p, int h2, int w2, float *oa, float *ob);
void launch_pool2(hipStream_t st, bool interleaved, const float *in, int B, int C, int h, int w, int p, int h2, int w2, float *out);
void launch_metric_final(hipStream_t st, const double *part, const MetricParts &P, int B, long long npx, long long n_ssim, const long long *n_level, double *out);


// lpips.hip: LPIPS(net='alex') (aej_lpips_*, include/aej.h)
constexpr int kLpipsTaps = 5;
constexpr int kLpipsHeadPixels = 256;      // pixels of a tap whose distances one workgroup of the head sums into one float64 partial
struct LpipsLayer { int cin, cinp, cout, k, stride, pad; };
extern const LpipsLayer kLpipsLayers[kLpipsTaps];
struct LpipsGeom {
    int H, W;
    int h[kLpipsTaps], w[kLpipsTaps];      // conv l's output (= tap l)
    int ph[2], pw[2];                       // the two maxpools' outputs
    long long tap_off[kLpipsTaps];          // element offset of tap l inside one image's normalised features
    long long feat_elems;                   // normalised features per image
    long long x_elems, y_elems;             // per image: the two ping-pong activation buffers
    int nblk[kLpipsTaps], max_blk;          // head workgroups (float64 partials) per image and tap
};
bool lpips_geom(int H, int W, LpipsGeom &g);          // false below 31 x 31 (torch's second maxpool would have no output)
long long lpips_param_floats();                        // floats of the canonical parameter list aej_lpips_pack_weights_host reads
long long lpips_packed_floats(long long off[kLpipsTaps][3]);     // floats of the packed weights; off[l] = {conv weights, bias, lin}
void lpips_pack_host(const float *params, float *packed);
// feats_out != NULL: write the normalised taps (features mode); else score against the normalised taps feats_a into out[B] (float64)
void launch_lpips(hipStream_t st, const float *wpk, const float *img, int B, const LpipsGeom &g, float *X, float *Y, float *feats_out,
                  const float *feats_a, double *partial, double *out);


// jfif.hip: baseline JPEG as Pillow / libjpeg-turbo writes it, and its decode (aej_jfif_*)
constexpr int kJfifBlockWords = 52;    // 32-bit words that bound one block's Huffman codes (DC <= 22 bits, 63 AC <= 26 bits each)
constexpr int kJfifBlockWordsOpt = 53; // the same with a file's own tables, whose codes reach 16 bits: 27 + 63 x 26 = 1665 bits
constexpr int kJfifHdrMax = 1024;      // SOI .. SOS are 623 bytes with the Annex K tables and never longer with optimised ones; a DRI adds 6
struct JfifGeom {
    int B, H, W, nq;
    int mcux, mcuy, ybx, yby;          // MCUs; real luma blocks per row / column
    int yw, yh, cw, ch;                // reconstruction sample planes
    long long n_mcu, nblk;             // per image; nblk = (hs * vs + 2) * n_mcu, dummy luma blocks included (one component: n_mcu)
    long long stream_words, n_chunks;  // per (quality, image): unstuffed scan words, 64-byte stuffing chunks
    long long plane_bytes;             // per (quality, image): Y, Cb, Cr sample planes
    int hs, vs, opt, ncomp;            // luma sampling factors (2 x 2, 2 x 1, 1 x 1, 1 x 2; chroma is 1 x 1); Huffman tables per file;
                                       // components: 3, or 1 (grey: hs = vs = 1, an MCU is one block, no dummies; entropy chains only)
    int R, rst_pad_;                   // restart interval of the baseline scan in MCUs (jfif_geom_restart; 0: none, requires opt otherwise)
    long long niv;                     // its intervals, ceil(n_mcu / R) (0 without restarts)
};
struct JfifParams {                    // one quality: quantisers in zigzag order (luma, chroma) and the markers SOI .. SOS
    int qt[2][64];
    int hdr_len, dht_off, pad_[2];     // dht_off: where the first DHT segment starts (SOS follows the fourth; the second of a grey file)
    unsigned char hdr[kJfifHdrMax];
};
struct JfifBufs {
    JfifParams *par; int *dct; short *coef; int *lens; unsigned *stream; int *ffcnt; long long *total;
    unsigned long long *boff, *ffpre;  // [seg][nblk + 1], [seg][n_chunks + 1] prefix sums of the blocks' bits and the chunks' 0xFF counts; the last is the total
    unsigned char *planes;
    // per-file Huffman tables (opt only): symbol counts [seg][4][257], (code << 8) | length [seg][4][256], markers [seg][kJfifHdrMax]
    unsigned long long *hist; unsigned *codes; unsigned char *fhdr; int *fhdr_len;
    unsigned long long *ivoff;         // restarts only: [seg][niv + 1] byte starts of the intervals in the unstuffed stream; the last is its bytes
};
// ss: Pillow's subsampling code (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0); opt: optimise the Huffman tables per file; ncomp: 3, or 1 (ss is
// then not looked at)
bool jfif_geom(int B, int H, int W, int nq, JfifGeom &g, int ss = 2, int opt = 0, int ncomp = 3);
// the same from luma sampling factors: 1 x 1, 2 x 1, 2 x 2 and 1 x 2 (4:4:0, which no subsampling code names: the entropy chains of the
// transcoder and the transforms alone take it -- launch_jfif_coefs, _encode and _recon refuse such a geometry)
bool jfif_geom_sampled(int B, int H, int W, int nq, JfifGeom &g, int hs, int vs, int opt = 0, int ncomp = 3);
// after jfif_geom: the restart interval of Pillow's restart_marker_blocks / restart_marker_rows (jr_interval, jfif_restart_core.h).
// false: a value outside 0..65535, or an interval with opt = 0 (the Annex K per-block stream bound has no room for the padding)
bool jfif_geom_restart(JfifGeom &g, int blocks, int rows);
unsigned long long jfif_carve(void *base, const JfifGeom &g, JfifBufs &w);
void jfif_quant_tables(int q, int luma[64], int chroma[64]);
void jfif_params_host(int q, int H, int W, JfifParams &p, int ss = 2, int ncomp = 3, int R = 0);      // R > 0: a DRI before the SOS
constexpr int jfif_sof_bytes(int ncomp) { return 10 + 3 * ncomp; }      // a frame header, marker and length included
constexpr int jfif_sos_bytes(int ncomp) { return 8 + 2 * ncomp; }       // a scan header of every component
int jfif_huffman_host(const long long *counts, unsigned char *bits, unsigned char *huffval);
// the baseline scan of n_mcu MCUs of given coefficients (int16 [n_mcu * blocks per MCU][64], zigzag and MCU order) on the host: the
// symbol counts [4][257] in table order and the stuffed scan bytes with their RSTn markers.  -> 0, or AEJ_ERR_ARG / AEJ_ERR_CAPACITY
// (out_len is set)
int jfif_seq_scan_host(const short *coefs, long long n_mcu, int hs, int vs, int ncomp, int R, int optimize, long long *hist, unsigned char *out,
                       unsigned long long cap, unsigned long long *out_len);
hipError_t launch_jfif_encode(hipStream_t st, const JfifGeom &g, const JfifBufs &w, const JfifParams *par_host, const unsigned char *rgb,
                              unsigned char *out, unsigned long long cap, long long *lengths, long long *offsets);
hipError_t launch_jfif_recon(hipStream_t st, const JfifGeom &g, const JfifBufs &w, unsigned char *rgb_out);
// the stages before entropy coding alone: parameters up, colour / down-sampling / FDCT, quantisation -> w.coef (w.lens is scratch)
hipError_t launch_jfif_coefs(hipStream_t st, const JfifGeom &g, const JfifBufs &w, const JfifParams *par_host, const unsigned char *rgb);

// the entropy stages alone (optimised tables): from w.coef and the markers in w.par, both already on the device, to lengths / offsets;
// the scatter is a launch of its own, so that a caller can place the files of several such chains first (jfiftrans.hip)
struct Carver;
unsigned long long jfif_carve_coded(Carver &c, const JfifGeom &g, JfifBufs &w);      // requires g.opt
hipError_t launch_jfif_entropy(hipStream_t st, const JfifGeom &g, const JfifBufs &w, long long *lengths, long long *offsets);
// the same chain for files that carry the Annex K tables (Pillow's optimize=False): one kernel fills every segment's codes and markers
// (those of w.par, whole) in the place of the histogram and table stages
hipError_t launch_jfif_entropy_annexk(hipStream_t st, const JfifGeom &g, const JfifBufs &w, long long *lengths, long long *offsets);
hipError_t launch_jfif_scatter(hipStream_t st, const JfifGeom &g, const JfifBufs &w, const long long *lengths, const long long *offsets,
                               unsigned char *out, unsigned long long cap);

// jfifprog.hip: the progressive file Pillow writes with progressive=True from the same coefficients (aej_jfif_*_prog)
constexpr int kJfpMaxScans = 10;       // jpeg_simple_progression of a three-component file (six scans for one component)
constexpr int kJfpPiece = 582;         // bytes that bound the markers before one scan's data: two DHT of 5 + 16 + 256, a DRI of 6 and an SOS of 14
struct JfpScan {
    int Ss, Se, Ah, Al;
    int comp, tbl;                     // -1: every block in MCU order, else 0 Y / 1 Cb / 2 Cr in the component's raster order; first table slot
    long long n, ioff;                 // blocks, and the first of them among the file's items
    long long woff, wcap, coff;        // the scan's stream: first word, words, first 64-byte chunk
    int R, dri;                        // restart interval in MCUs of this scan (0: none); whether a DRI precedes its SOS (R differs from the scan before)
    long long per, niv, ivoff;         // restarts only: items per interval (R x blocks per MCU), intervals, the first of them among the file's
};
struct JfpGeom {
    int segs, hs, vs, nchroma;         // files (quality x image); luma sampling factors; chroma blocks per MCU (0: the testing entry's plain list)
    int mcux, ybx, nscan, ntab;
    int raw, B;                        // raw: no markers, the scan bytes alone (the testing entry); images per quality
    long long nblk, T, nmax;           // coefficient blocks per file; items per file (the sum of the scans' blocks); the longest scan
    long long stream_words, n_chunks;
    long long NIV;                     // restart intervals per file, the sum of the scans' (0: no restarts)
    JfpScan sc[kJfpMaxScans];
};
struct JfpBufs {
    unsigned short *flags;             // [seg][T] what each block leaves pending (k_jfp_facts)
    unsigned long long *pre;           // [seg][T + 1] prefix sums: of je_pack for the partition, afterwards of the bit counts
    int *plen, *lens;                  // [seg][T] blocks of the piece an item opens (0: opens none); bits of an item
    unsigned *stream; int *ffcnt; unsigned long long *ffpre;
    unsigned long long *hist; unsigned *codes; unsigned char *fhdr; int *fhdr_len, *cuts;
    long long *total;
    unsigned long long *ivpre;         // restarts only: [seg][NIV + 1] prefix sums of the intervals' bytes (each ceil(bits / 8)), scan after scan
};
// blocks, rows: Pillow's restart_marker_blocks / restart_marker_rows; every scan takes its own interval (jr_interval)
bool jfifprog_geom(const JfifGeom &g, JfpGeom &p, int blocks = 0, int rows = 0);
unsigned long long jfifprog_carve(void *base, const JfifGeom &g, const JfpGeom &p, JfifBufs &w, JfpBufs &pw);
hipError_t launch_jfifprog_encode(hipStream_t st, const JfifGeom &g, const JfpGeom &p, const JfifBufs &w, const JfpBufs &pw,
                                  const JfifParams *par_host, const unsigned char *rgb, unsigned char *out, unsigned long long cap,
                                  long long *lengths, long long *offsets);
unsigned long long jfifprog_carve_coded(Carver &c, const JfifGeom &g, const JfpGeom &p, JfifBufs &w, JfpBufs &pw);
hipError_t launch_jfifprog_entropy(hipStream_t st, const JfpGeom &p, const JfpBufs &pw, const short *coef, const JfifParams *par, long long *lengths,
                                   long long *offsets);
hipError_t launch_jfifprog_scatter(hipStream_t st, const JfpGeom &p, const JfpBufs &pw, const JfifParams *par, const long long *lengths,
                                   const long long *offsets, unsigned char *out, unsigned long long cap);
// one scan over n blocks of given coefficients (int16 [n][64], zigzag order): the padded, stuffed scan bytes, the counts of its
// symbols [257] and its cuts (by kJeMaxRun, by kJeMaxDeferred).  -> 0, or AEJ_ERR_ARG / AEJ_ERR_CAPACITY (out_len is set)
int jfifprog_scan_host(const short *coefs, long long n, int Ss, int Se, int Ah, int Al, unsigned char *out, unsigned long long cap,
                       unsigned long long *out_len, long long *counts, long long *cuts);
int jfifprog_scan_device(hipStream_t st, const short *coefs_host, long long n, int Ss, int Se, int Ah, int Al, unsigned char *out_host,
                         unsigned long long cap, unsigned long long *out_len, long long *counts, long long *cuts, hipError_t *err);

}  // namespace aej

// jpegdec.hip: baseline JPEG files decoded on the device (aej_jpegdec_*); jpegparse.hip: the marker walk of both decoders
#include <string>
#include <vector>
#include "jpegdec_core.h"

namespace aej {
struct JdBufSizes { long long chunks, segs, slots, blocks, clean, planes, px, grp[3], grp440[3], grpl[4], grpa, uniform, grps[4]; };      // totals over the files of one call (grp, grp440, grpl, grps: JdFile::grp_base, ::grp440_base, ::grpl_base, ::grps_base; grpa: ::grpa_base, the workgroups of k_jd_adobe -- non-zero exactly when the call has a four-component or RGB-coded file; uniform: the files with JdFile::uniform, three-component YCbCr ones included -- a call with one runs the kFour slot kernels too)
inline bool jpeg_any_box(const JdBufSizes &z) { return z.grps[0] > 0 || z.grps[1] > 0 || z.grps[2] > 0 || z.grps[3] > 0; }      // a call with a boxed file, at full size or at a scale: the <true> slot kernels, aej_jpegdec_box_stats
struct JdBufs {
    JdFile *files; aej_jpegdec_desc *descs; int *last_change;      // one upload: files, descriptors, the "last round that changed" word
    aej_jpeg_adobe *adobe;                                         // and, in a call that runs the kFour slot kernels (z.grpa > 0 or z.uniform > 0), room for the files' aej_jpeg_adobe (uploaded when z.grpa > 0; else NULL)
    int *cnt; long long *pre, *clean_len; JdSeg *segs; unsigned char *clean; JdSlots sl; short *coef; unsigned char *planes;
};
struct JdHuffSrc { bool defined = false; unsigned char bits[17] = {}; unsigned char vals[256] = {}; int count = 0; };      // one DHT table
bool jd_build_huff(const JdHuffSrc &s, aej_jpegdec_huff &h);                                                              // jpegparse.hip
// allow440 (both parsers): luma sampled 1 x 2 over 1 x 1 chroma is accepted beside 4:4:4, 4:2:2 and 4:2:0
// adobe (both parsers; not NULL: the _adobe entries): four-component and RGB-coded files are accepted too, *adobe says what the file is
int jpegdec_parse(const unsigned char *data, unsigned long long n, aej_jpegdec_desc &d, std::string &msg, bool allow440 = false,
                  aej_jpeg_adobe *adobe = nullptr);                                                                    // jpegparse.hip
// did one of the parsers write this frame?  D: aej_jpegdec_desc or aej_jpegprog_frame -- what the layouts below size buffers from
template <class D>
bool jpeg_frame_ok(const D &e)
{
    const bool color = e.ncomp == 3 && ((e.hs == 1 && (e.vs == 1 || e.vs == 2)) || (e.hs == 2 && (e.vs == 1 || e.vs == 2)));      // 1 x 2: the _440 parsers'
    if (!(color || (e.ncomp == 1 && e.hs == 1 && e.vs == 1))) return false;
    if (e.width < 1 || e.height < 1 || e.width > 65535 || e.height > 65535) return false;
    if (e.mcux != (e.width + 8 * e.hs - 1) / (8 * e.hs) || e.mcuy != (e.height + 8 * e.vs - 1) / (8 * e.vs)) return false;
    return e.blocks_per_mcu == (e.ncomp == 1 ? 1 : e.hs * e.vs + 2);
}
inline bool jpeg_adobe_new(const aej_jpeg_adobe *x) { return x && x->colour != AEJ_JPEG_YCBCR; }      // a file only the _adobe entries take
// the same with the file's aej_jpeg_adobe (NULL: none): a four-component frame is one the _adobe parsers wrote
template <class D>
bool jpeg_frame_ok(const D &e, const aej_jpeg_adobe *x)
{
    if (!x || x->colour == AEJ_JPEG_YCBCR) return jpeg_frame_ok(e);
    if (x->colour == AEJ_JPEG_RGB) return e.ncomp == 3 && jpeg_frame_ok(e);
    if ((x->colour != AEJ_JPEG_CMYK && x->colour != AEJ_JPEG_YCCK) || e.ncomp != 4) return false;
    if (!((e.hs == 1 || e.hs == 2) && (e.vs == 1 || e.vs == 2))) return false;
    if (!((x->h3 == e.hs && x->v3 == e.vs) || (x->h3 == 1 && x->v3 == 1))) return false;
    if (e.width < 1 || e.height < 1 || e.width > 65535 || e.height > 65535) return false;
    if (e.mcux != (e.width + 8 * e.hs - 1) / (8 * e.hs) || e.mcuy != (e.height + 8 * e.vs - 1) / (8 * e.vs)) return false;
    return e.blocks_per_mcu == e.hs * e.vs + 2 + x->h3 * x->v3;
}
bool jpegdec_descs_ok(const aej_jpegdec_desc *descs, int n, const aej_jpeg_adobe *adobe = nullptr);      // n >= 1 descriptors aej_jpegdec_parse_host wrote (adobe: [n] or NULL)
// one un-stuffing stream of len stuffed bytes and n_segments restart segments, subsequences of S bits: F's stream fields, z's totals
void jpeg_stream_layout(long long len, int n_segments, int S, JdFile &F, JdBufSizes &z);
// one file's coefficient blocks and, decoded at scale 1 << shift, its sample planes and pixels (shift 0) or its workgroups of the
// scaled kernel (1..3), or, with kJdLuma added to shift, its workgroups of the luma kernel (d's frame fields): F's reconstruction
// fields, z's totals
// box (NULL, or the whole image: none): left, top, right, bottom inside the image (jpeg_box_inside), full size only -- the file's
// workgroups of k_jd_sbox<0> and no sample planes; window_coef: only the coefficients of the window's MCU rows are stored (baseline files)
// kJdSbox in shift (the _sbox entries, scale 2, 4, 8): box is in pixels of the scaled image, inside it and not the whole of it -- the
// file's workgroups of k_jd_sbox<log2 scale>, the same coefficient window
// x (NULL: none): the file's aej_jpeg_adobe; with another colour than YCbCr the file gets kJdAdobe in its shift, four sample planes and
// its workgroups of k_jd_adobe (shift: 0, or kJdCmyk for four-channel output; the callers refuse a scale, luma or a box for such a file)
void jpeg_recon_layout(const aej_jpegdec_desc &d, int shift, JdFile &F, JdBufSizes &z, const int *box = nullptr, bool window_coef = true,
                       const aej_jpeg_adobe *x = nullptr);
template <class D>                     // D: aej_jpegdec_desc or aej_jpegprog_frame
bool jpeg_box_whole(const D &d, const int *box) { return !box || (box[0] == 0 && box[1] == 0 && box[2] == d.width && box[3] == d.height); }
template <class D>
bool jpeg_box_inside(const D &d, const int *box)
{
    return 0 <= box[0] && box[0] < box[2] && box[2] <= d.width && 0 <= box[1] && box[1] < box[3] && box[3] <= d.height;
}
inline int jpeg_scale_shift(int scale) { return scale == 1 ? 0 : scale == 2 ? 1 : scale == 4 ? 2 : scale == 8 ? 3 : -1; }      // -1: not a scale
// What the options of a decoder call resolve to (api_jpeg.hip: jd_resolve; {}: no options).  shifts: jpeg_recon_layout's shift of every
// file -- log2 of its scale, + kJdLuma for one that leaves as its luma plane, + kJdSbox, + kJdCmyk -- or empty for all at full size,
// RGB; boxes: NULL or [n][4], jpeg_recon_layout's box of every file; adobe: NULL or [n], its aej_jpeg_adobe
struct JdResolved { std::vector<int> shifts; const int *boxes = nullptr; const aej_jpeg_adobe *adobe = nullptr; };
void jpegdec_layout(const aej_jpegdec_desc *descs, int n, int S, std::vector<JdFile> &files, JdBufSizes &z, const JdResolved &r);
unsigned long long jpegdec_carve(void *base, int n, const JdBufSizes &z, JdBufs &w);
hipError_t launch_jpegdec_begin(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, const void *blob_host, unsigned long long blob_bytes,
                                const unsigned char *scans, int S, int *status);
hipError_t launch_jpegdec_unstuff(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, const unsigned char *scans, int S, int *status);
hipError_t launch_jpegdec_recon(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, unsigned char *out);
int jpegdec_coefs_host(const aej_jpegdec_desc &d, const unsigned char *file, unsigned long long nbytes, short *coef, unsigned long long coef_blocks);
hipError_t launch_jpegdec_sync(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, int S, int first_round, int rounds);
hipError_t launch_jpegdec_write(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, int S, int *status);      // finish without the reconstruction
hipError_t launch_jpegdec_finish(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, int S, unsigned char *out, int *status);

}  // namespace aej

// jpegprog.hip: progressive JPEG files decoded on the device (aej_jpegprog_*)
#include "jpegprog_core.h"

namespace aej {
struct JpLayout {                      // host-computed layout of one aej_jpegprog_batch; scans ordered by dependency level
    std::vector<JdFile> sfiles, ffiles;                // one un-stuffing stream per scan; one reconstruction entry per file
    std::vector<aej_jpegdec_desc> sdescs, fdescs;      // per scan: segments, unit counts, Huffman tables; per file: what k_jd_idct / k_jd_rgb read
    std::vector<JpScan> scans;
    std::vector<aej_jpeg_adobe> fadobe;                // per file, in a call with a four-component or RGB-coded file alone (fz.grpa > 0); else empty
    std::vector<int> src;                              // scans[t] is the caller's scan src[t]
    std::vector<JpItem> items;
    std::vector<long long> level_items;                // items of level l: [level_items[l], level_items[l + 1])
    JdBufSizes sz{}, fz{};                             // totals over the scans (chunks, segs, slots, clean) and the files (blocks, planes, px)
    int n_levels = 0;
};
struct JpBufs { void *blob; JdBufs s, f; JpScan *scans; JpItem *items; int *sstatus; };
// the units a progressive scan walks (x: the file's aej_jpeg_adobe or NULL -- component 3 sampled as component 0 has its block grid)
inline void jp_scan_units(const aej_jpegprog_frame &f, int ncomp, int comp0, int &ux, int &uy, const aej_jpeg_adobe *x = nullptr)
{
    const bool full3 = comp0 == 3 && x && x->h3 == f.hs && x->v3 == f.vs;
    if (ncomp > 1 || f.ncomp == 1 || (comp0 > 0 && !full3)) { ux = f.mcux; uy = f.mcuy; }      // chroma is sampled 1x1: its block grid is the MCU grid
    else { ux = (f.width + 7) / 8; uy = (f.height + 7) / 8; }
}
int jpegprog_parse(const unsigned char *data, unsigned long long n, aej_jpegprog_frame &f, std::vector<aej_jpegprog_scan> &scans,
                   std::string &msg, bool allow440 = false, aej_jpeg_adobe *adobe = nullptr);                          // jpegparse.hip
bool jpegprog_layout(const aej_jpegprog_frame *frames, const aej_jpegprog_scan *scans, int n, JpLayout &y, const JdResolved &r);
unsigned long long jpegprog_blob(const JpLayout &y, std::vector<unsigned char> *out);
unsigned long long jpegprog_carve(void *base, const JpLayout &y, JpBufs &w);
hipError_t launch_jpegprog_entropy(hipStream_t st, const JpLayout &y, const JpBufs &w, const void *blob_host, unsigned long long blob_bytes,
                                   const unsigned char *data, int n_levels, int *status);
hipError_t launch_jpegprog_recon(hipStream_t st, const JpLayout &y, const JpBufs &w, unsigned char *out);
int jpegprog_coefs_host(const aej_jpegprog_frame &frame, const aej_jpegprog_scan *scans, const unsigned char *file, unsigned long long nbytes,
                        int n_levels, short *coef, unsigned long long coef_blocks);

}  // namespace aej

// jfiftrans.hip: lossless transcode -- the decoders' coefficients entropy-coded again under optimal tables (aej_jfif_transcode_*),
// with a lossless flip / rotation / transposition on the way (aej_jfif_transform_*)
#include "jfif_transform_core.h"

namespace aej {
struct JtSource {                      // what the output's markers take from one parsed file
    int width, height, hs, vs, ncomp;  // ncomp: 3, or 1 (hs = vs = 1 whatever the file's frame header says: the parsers' rule)
    unsigned char comp_id[3], comp_tq[3];
    unsigned short qt[3][64];          // natural order
    int units, xdensity, ydensity;     // of the JFIF APP0
};
struct JtFile {                        // one file of a call (host-computed, uploaded): where the bridge reads and writes its blocks
    long long src_base, n_blocks;      // its first block among the call's OUTPUT blocks, files in the caller's order, and their number
    const short *src;                  // its coefficients as its decoder left them: natural order, the source's MCU order (JdFile::blk_base)
    short *dst;                        // its segment of its group's w.coef: zigzag order, the group's MCU order
    int status_index, out_pos;         // its word in the status array; its place in output order (group after group)
};
struct JtGroup {                       // the files of one OUTPUT (H, W, hs, vs, components): one entropy-encode chain, every file one "quality" of one image
    JfifGeom g; JfpGeom p; JfifBufs w; JfpBufs pw;
    std::vector<int> files;            // caller's indices, in segment order
    std::vector<JfifParams> par;       // their markers (kept until the upload has run)
    long long first;                   // its first file in output order
    bool foreign_ids;                  // a file's component ids are not 1, 2, 3 (one component: not 1)
};
struct JtPlan {
    bool prog = false;
    bool transform = false;            // a file has a transform other than kJxNone: k_jt_transform takes the place of k_jt_bridge
    bool cut = false;                  // a file has a crop or drops its chroma (JxGeom::cut): k_jt_cut takes the place of both
    bool annexk = false;               // baseline files under the Annex K Huffman tables, not their own (the ragged encoder without optimize)
    int rst_blocks = 0, rst_rows = 0;  // restart_marker_blocks / restart_marker_rows of the call (jfiftrans_close gives every group its interval)
    std::vector<JtFile> files;         // caller's order
    std::vector<JxGeom> geom;          // caller's order (transform only)
    std::vector<JtGroup> groups;
    long long n_blocks = 0;
    JtFile *d_files = nullptr;         // device: the table,
    JxGeom *d_geom = nullptr;          // the transforms beside it (transform only),
    long long *glen = nullptr, *goff = nullptr, *total = nullptr;      // lengths and offsets in output order, their sum
};
void jfiftrans_source(const aej_jpegdec_desc &d, JtSource &s);
void jfiftrans_source(const aej_jpegprog_frame &f, JtSource &s);
// the markers SOI .. SOF0 / SOF2 the transcoder writes for one source -> their length, or -1 when they do not fit
int jfiftrans_prefix_host(const JtSource &s, bool prog, unsigned char *out, int capacity);
// what the markers of the transformed file take: the output size, sampling and component count of g, the tables transposed with it
JtSource jfiftrans_transformed(const JtSource &s, const JxGeom &g);
// n_blocks[i]: blocks the decoder holds for file i (must equal the source's MCU-padded count).  xf (may be NULL: the transcoder):
// one transform code per file.  -> -1, or the first file that does not fit: *why (may be NULL) gets jx_geom's answer, kJxBadArg for
// descriptors that disagree.  boxes (may be NULL): 4 ints per file, jx_geom's crop box (right == 0: none); drop: jx_geom's chroma drop, for
// every file.
int jfiftrans_plan(const std::vector<JtSource> &src, const std::vector<long long> &n_blocks, bool prog, const int *xf, int trim, JtPlan &plan,
                   int *why, int rst_blocks = 0, int rst_rows = 0, bool allow440 = false, const int *boxes = nullptr, bool drop = false);
// the pieces of a plan, shared with the ragged encoder (jfifmany.hip).  Before them: plan.files sized, plan.prog set.
// the group of one output geometry, made on first use (NULL: a geometry jfif_geom refuses)
JtGroup *jfiftrans_group(JtPlan &plan, int H, int W, int hs, int vs, int ncomp = 3);
// file i, of n_out blocks, joins grp: its place among the call's blocks
void jfiftrans_add(JtPlan &plan, JtGroup &grp, int i, long long n_out);
// after the last file: every group's geometry with one "quality" per file, its place in output order, empty markers (JtGroup::par) for
// the caller to fill.  -> -1, or a file of a group that does not fit
int jfiftrans_close(JtPlan &plan);
// HOST: the transform of one file's coefficients, the code k_jt_transform runs.  src: [g.n_src][64] natural order, the source's MCU
// order; dst: [g.n_out][64] zigzag order, the output's MCU order
void jfiftrans_coefs_host(const JxGeom &g, const short *src, short *dst);
unsigned long long jfiftrans_carve(void *base, JtPlan &plan);
// bridge, one entropy chain per group, placement, scatter.  Before it: plan.files[i].src / status_index set by the caller.  status: the
// call's status words (the decoders' results in; out-of-range coefficients added); lengths / offsets: device, caller's order
hipError_t launch_jfiftrans(hipStream_t st, JtPlan &plan, int *status, unsigned char *out, unsigned long long cap, long long *lengths,
                            long long *offsets);
// its stages after the bridge: given every JtFile::dst filled and plan.d_files uploaded, one entropy chain per group, placement, scatter,
// finish.  status may be NULL (no file can have failed)
hipError_t launch_jfiftrans_chains(hipStream_t st, JtPlan &plan, const int *status, unsigned char *out, unsigned long long cap, long long *lengths,
                                   long long *offsets);

}  // namespace aej

// jfifmany.hip: the encoder for images of mixed sizes and qualities in one call (aej_jfif_many_*): a ragged front end, then the
// transcoder's chains
#include "jfif_many_core.h"

namespace aej {
struct JmImage {                       // one image of a call (host-computed, uploaded): all that k_jm_coefs reads about it
    long long blk_base;                // its first block among the call's blocks, images in the caller's order
    long long src_offset;              // its packed uint8 [H][W][3] (grey: [H][W]) in the source buffer
    short *dst;                        // its segment of its group's w.coef: n_blocks x 64, zigzag order, MCU order
    JmGeom g;
    unsigned short qt[2][64];          // its quality's quantisers (luma, chroma), zigzag order
};
struct JmPlan {
    JtPlan t;                          // groups, chains and placement: the transcoder's (JtFile::src unused, no status words)
    std::vector<JmImage> images;       // caller's order
    JmImage *d_images = nullptr;
    int hs = 2, vs = 2;                // the call's luma sampling factors (its colour images'; a grey image is 1 x 1 whatever they are)
};
// src_bytes < 0: the source buffer's size is not known yet (a workspace query).  -> -1, or the first image the call refuses and *why
int jfifmany_plan(const aej_jfif_many_desc *descs, int n, long long src_bytes, int ss, bool opt, bool prog, JmPlan &plan, const char **why,
                  int rst_blocks = 0, int rst_rows = 0);
unsigned long long jfifmany_carve(void *base, JmPlan &plan);
hipError_t launch_jfifmany(hipStream_t st, JmPlan &plan, const unsigned char *src, unsigned char *out, unsigned long long cap, long long *lengths,
                           long long *offsets);
// HOST: one image's quantised blocks, the code k_jm_coefs runs.  -> its block count (rgb and dst both NULL: a size query), -1 for
// arguments outside the encoder's
long long jfifmany_coefs_host(int W, int H, int quality, int ss, const unsigned char *rgb, short *dst, int ncomp = 3);

}  // namespace aej

// resample.hip: Pillow's reduce and two-pass resize of packed 8-bit RGB and one-channel images (aej_resample_*)
namespace aej {
constexpr int kRsBits = 22;            // Pillow's PRECISION_BITS for 8-bit images: taps are int(k * 2^22 +- 0.5)
constexpr int kRsThreads = 256;
struct RsReduce {                      // one image of k_rs_reduce (device pointers set by resample_blob)
    const unsigned char *in;           // the first pixel of the reduce box
    unsigned char *out;
    long long tile_base;               // its first workgroup
    int in_w;                          // pixels per input row
    int bw, bh, fx, fy, out_w, out_h;  // the box, the factors, ceil(box / factor)
};
struct RsConv {                        // one image of k_rs_horizontal / k_rs_vertical
    const unsigned char *in;
    unsigned char *out;
    const int *bounds, *taps;          // [out][2] first source index and count; horizontal [ksize][out_w], vertical [out_h][ksize]
    long long tile_base;
    int in_w, out_w, out_h, ksize;
    int shift;                         // the input's first row in the vertical bounds' coordinates
    int pad;
};
struct RsImage {                       // host: the stages of one image and where they read and write
    bool reduce, horizontal, vertical;
    int ch;                            // bytes per pixel: 3, or 1
    RsReduce r; RsConv h, v;
    long long r_src, tmp_a, tmp_b, h_table, v_table;
    long long win_shift;               // a windowed source without a reduce: bytes from its first stored pixel to pixel (0, 0) of the virtual image (<= 0)
};
struct RsPlan {
    std::vector<RsImage> images;
    Spans spans;                       // per image: its stored source rectangle, its output
    std::vector<int> ints;             // the tables (filled on request)
    long long n_ints = 0, tmp_bytes = 0, tiles[2][3] = {{0, 0, 0}, {0, 0, 0}};      // [0]: the three-channel images, [1]: the one-channel ones
    int count[2][3] = {{0, 0, 0}, {0, 0, 0}};      // images in the reduce / horizontal / vertical launch of either
};
struct RsBufs { unsigned char *blob, *tmp; };
double rs_support(int filter);         // 0: not a filter
int rs_ksize(float in0, float in1, int out_size, int filter);
void rs_taps(int in_size, float in0, float in1, int out_size, int filter, int ksize, int *bounds, int *taps);
void rs_bounds_of_row(int in_size, float in0, float in1, int out_size, int filter, int xx, int *bounds);
const char *rs_check(const aej_resample_desc &d, int *code);
int resample_plan(const aej_resample_desc *descs, int n, bool fill, RsPlan &plan, const char **why, int *code, const int *channels = nullptr,
                  const int *windows = nullptr);
unsigned long long resample_carve(void *base, const RsPlan &plan, RsBufs &w);
void resample_blob(const RsPlan &plan, const RsBufs &w, const unsigned char *src, unsigned char *dst, std::vector<unsigned char> &blob);
hipError_t launch_resample(hipStream_t st, const RsPlan &plan, const RsBufs &w, const void *blob_host, unsigned long long blob_bytes);

}  // namespace aej

// filter.hip: Pillow's BoxBlur / GaussianBlur / UnsharpMask on packed 8-bit images of 1 to 4 channels (aej_filter_*)
namespace aej {
constexpr int kFtThreads = 512;        // k_filter_tile: eight waves, two workgroups a CU at its largest tile
constexpr int kFtTileW = 64, kFtTileH = 32;      // output pixels of a fused tile
constexpr int kFtHalo = 16;            // the most passes * (r + 1) may be on an axis of the fused kernel: 4-channel tiles then take 56 KiB of LDS
constexpr int kFtSeg = 8;              // samples one lane slides its window over in the fused kernel
constexpr int kFtPassThreads = 256;    // k_filter_rows, k_filter_cols
constexpr int kFtRowSpan = 512;        // pixels of a row one k_filter_rows workgroup writes
constexpr int kFtColBand = 128;        // rows one k_filter_cols lane walks down
constexpr int kFtColBytes = 4 * kFtPassThreads;      // byte columns of a k_filter_cols workgroup: a lane owns 4
constexpr int kFtMaxRadius = 1024;
struct FtEntry {                       // one image of one launch (device pointers set by filter_blob)
    const unsigned char *in, *orig;    // orig: the unfiltered image where this launch applies the unsharp epilogue, else NULL
    unsigned char *out;
    long long tile_base;               // the first workgroup of this image in its launch
    int w, h;                          // k_filter_tile, k_filter_rows: pixels; k_filter_cols: w is the bytes of a row
    int nx, ny, hx, hy;                // k_filter_tile: passes per axis (0: none) and the halo passes * (r + 1)
    int rx, ry;                        // the rows kernel reads the x fields, the columns kernel the y fields
    unsigned wwx, fwx, wwy, fwy;
    int percent, threshold;
};
struct FtStage {                       // host: an entry and where its pointers come from (0 src, 1 dst, 2 the workspace's buffers)
    FtEntry e;
    int in_base, out_base;
    long long in_off, out_off, orig_off;      // orig_off < 0: no epilogue
};
struct FtLaunch { int kernel, ch, first, count; long long tiles; unsigned lds; };      // kernel: 0 tile, 1 rows, 2 columns
struct FtPlan {
    std::vector<FtStage> stages;       // launch by launch
    std::vector<FtLaunch> launches;
    Spans spans;                       // per image: its source, its output
    long long tmp_bytes = 0;
};
struct FtBufs { unsigned char *blob, *tmp; };
int filter_weights(int kind, float xradius, float yradius, aej_filter_plan &p);      // aej_filter_plan_host
int filter_plan(const aej_filter_desc *descs, int n, int path, FtPlan &plan, int *bad, const char **why);
unsigned long long filter_carve(void *base, const FtPlan &plan, FtBufs &w);
void filter_blob(const FtPlan &plan, const FtBufs &w, const unsigned char *src, unsigned char *dst, std::vector<FtEntry> &blob);
hipError_t launch_filter(hipStream_t st, const FtPlan &plan, const FtBufs &w, const FtEntry *blob_host);

}  // namespace aej

// window.hip: Pillow's Kernel, rank and mode filters on packed 8-bit images of 1 to 4 channels (aej_window_*)
namespace aej {
constexpr int kWnThreads = 512;        // eight waves: a lane produces 4 adjacent bytes of a tile row at a time
constexpr int kWnTileW = 64, kWnTileH = 32;      // output pixels of a tile
constexpr int kWnKernelHalo = 2, kWnRankHalo = 7, kWnModeHalo = 3;      // the largest r of each kind: a 4-channel rank-15 tile takes 14 KiB of LDS
struct WnEntry {                       // one image of one launch (device pointers set by window_blob)
    const unsigned char *in;
    unsigned char *out;
    long long tile_base;               // the first workgroup of this image in its launch
    int w, h;                          // pixels
    int r, rank;                       // the halo size / 2; the rank kernel's rank
    float ss0;                         // Kernel: offset + 0.5f
    float q[25];                       // Kernel: kernel[i] / scale
};
struct WnLaunch { int kind, ch, size, first, count; long long tiles; unsigned lds; };      // size: the Kernel's (3 or 5), else 0
struct WnPlan {
    std::vector<WnEntry> entries;      // launch by launch; in / out hold nothing yet
    std::vector<int> image;            // the image of each entry
    std::vector<WnLaunch> launches;
    Spans spans;                       // per image: its source, its output
};
int window_plan(const aej_window_desc *descs, int n, WnPlan &plan, int *bad, const char **why);
void window_blob(const WnPlan &plan, const unsigned char *src, unsigned char *dst, std::vector<WnEntry> &blob);
hipError_t launch_window(hipStream_t st, const WnPlan &plan, unsigned char *blob_dev, const WnEntry *blob_host);

}  // namespace aej

// lut3d.hip: Pillow's Color3DLUT on packed 8-bit images of 3 and 4 channels (aej_lut3d_*)
namespace aej {
constexpr int kLtThreads = 512;        // eight waves
constexpr int kLtRun = 4;              // adjacent pixels a lane takes at a time: 3 or 4 dwords in, 3 or 4 out
constexpr int kLtTile = 2 * kLtThreads * kLtRun;      // pixels of a workgroup
struct LtEntry {                       // one image of one launch (device pointers set by lut3d_blob)
    const unsigned char *in;
    unsigned char *out;
    const uint2 *table;                // its table, every entry four INT16 (a 3-channel entry padded)
    long long tile_base;               // the first workgroup of this image in its launch
    long long npix;
    unsigned scale[3];                 // (s_d - 1) / 255 in 18 fraction bits
    int s1, s12;                       // the steps of axis 2 and axis 3, in entries
    int entries;                       // s1 * s2 * s3
    int pad;
};
struct LtLaunch { int ci, tc, co, first, count; long long tiles; };
struct LtPlan {
    std::vector<LtEntry> entries;      // launch by launch; in / out / table hold nothing yet
    std::vector<int> image;            // the image of each entry
    std::vector<LtLaunch> launches;
    std::vector<long long> table_at;   // per table: its first entry in the padded upload; one more: the end
    std::vector<int> table_tc;         // per table: its channels (0: no image uses it)
    Spans spans;                       // per image: its source, its output
};
int lut3d_plan(const aej_lut3d_desc *descs, int n, const long long *table_offsets, int n_tables, LtPlan &plan, int *bad, const char **why);
int lut3d_prepare(const float *table, long long n, short *out);      // aej_lut3d_prepare_host
void lut3d_blob(const LtPlan &plan, const aej_lut3d_desc *descs, const short *tables_host, const long long *table_offsets, const unsigned char *src,
                unsigned char *dst, const uint2 *tables_dev, std::vector<LtEntry> &blob, std::vector<short> &padded);
hipError_t launch_lut3d(hipStream_t st, const LtPlan &plan, unsigned char *blob_dev, const LtEntry *blob_host, uint2 *tables_dev, const short *padded);

}  // namespace aej

// warp.hip: Pillow's Image.transform and Image.transpose on packed 8-bit images of 1 to 4 channels (aej_warp_*)
namespace aej {
constexpr int kWpThreads = 256;
constexpr int kWpTileW = 32, kWpTileH = 8;       // k_warp: output pixels of a workgroup, one per lane
constexpr int kWpFlipBytes = 1024, kWpFlipRows = 4;      // k_flip: bytes of an output row (4 per lane) and rows of a workgroup
constexpr int kWpSwapTile = 32;                  // k_transpose: a square tile of output pixels, staged in LDS
constexpr int kWpMaxSide = 32767;
struct WpEntry {                       // one image of one launch (device pointers set by warp_blob)
    const unsigned char *in;
    unsigned char *out;
    const int *tab;                    // AEJ_WARP_TABLES: xtab[dw], ytab[dh]
    long long tile_base;               // the first workgroup of this image in its launch
    long long fx[6];                   // AEJ_WARP_FIXED: A0 .. A5
    double a[8];
    int sw, sh, dw, dh;                // pixels
    int method;                        // AEJ_WARP_TRANSPOSE: Pillow's method
    int premul;
    unsigned char fill[4];
    int tab_at;                        // host: its tables in WpPlan::tables (ints), -1: none
};
struct WpLaunch { int kernel, ch, filter, path, first, count; long long tiles; };      // kernel: 0 k_warp, 1 k_flip, 2 k_transpose
struct WpPlan {
    std::vector<WpEntry> entries;      // launch by launch; in / out / tab hold nothing yet
    std::vector<int> image;            // the image of each entry
    std::vector<WpLaunch> launches;
    std::vector<int> tables;           // every AEJ_WARP_TABLES image's two tables
    Spans spans;                       // per image: its source, its output
};
int warp_resolve(const aej_warp_desc &d, aej_warp_plan &p, std::vector<int> *tables, const char **why);      // aej_warp_plan_host
int warp_plan(const aej_warp_desc *descs, int n, WpPlan &plan, int *bad, const char **why);
void warp_blob(const WpPlan &plan, const unsigned char *src, unsigned char *dst, const int *tables_dev, std::vector<WpEntry> &blob);
hipError_t launch_warp(hipStream_t st, const WpPlan &plan, unsigned char *blob_dev, const WpEntry *blob_host, int *tables_dev);

}  // namespace aej

// adjust.hip: Pillow's ImageEnhance, ImageOps point operations and Image.histogram on packed 8-bit images of 1 to 4 channels (aej_adjust_*)
namespace aej {
constexpr int kAdThreads = 256;
constexpr int kAdChunk = 4096;         // pixels of one image a workgroup takes at a time: in groups of 16 bytes a lane (12 for 3 channels)
constexpr int kAdMaxGrid = 16384;      // workgroups of a launch; the chunks beyond are reached by striding
constexpr int kAdMaxSide = 32767;
constexpr int kAdHistWords = 1024;     // counters of one histogram pass of one image: up to 4 bands x 256
constexpr int kAdWiden = -1;           // AdLutEntry::kind of aej_histogram_batch's widening
struct AdStep { int kind, slot; float factor; int pad; };
struct AdEntry {                       // one image of one histogram or apply launch
    const unsigned char *in;           // the segment's input, cin bytes a pixel
    const unsigned char *deg;          // filter(SMOOTH) of `in`: read when step 0 is AEJ_ADJUST_SHARPNESS
    unsigned char *out;                // apply: what the steps leave, 1 byte a pixel after a GRAYSCALE, else cin
    unsigned *hist;                    // histogram: `bins` counters of this pass
    const unsigned char *tables;       // the image's AEJ_ADJUST_MAX_OPS tables, one per op of its chain
    long long chunk_base;              // the first chunk of this image in its launch
    long long npix;
    int n_steps, luma, bins, pad;      // luma: the histogram is of L alone
    AdStep step[AEJ_ADJUST_MAX_OPS];
};
struct AdLutEntry {                    // one image of one table launch (k_adjust_luts)
    const unsigned *hist;
    unsigned char *table;              // the op's table; CONTRAST: byte 0 is the mean
    long long *wide;                   // kAdWiden: the int64 counts
    long long npix;
    int kind, bands, copies, pad;      // bands histograms -> bands tables, or one table written `copies` times (preserve_tone)
    double cutoff[2];
    unsigned ignore[8];
};
struct AdLaunch { int kernel, cin, gray, first, count, round; long long chunks; };      // kernel: 0 k_adjust_hist, 1 k_adjust_luts, 2 k_adjust_apply, 3 SMOOTH round
struct AdSmooth { WnPlan plan; std::vector<WnEntry> blob; unsigned char *blob_dev; };
struct AdPlan {
    std::vector<AdEntry> entries;      // launch by launch, device pointers set (null when only measured)
    std::vector<AdLutEntry> luts;
    std::vector<AdLaunch> launches;
    std::vector<AdSmooth> smooths;
    std::vector<unsigned char> tables; // per image AEJ_ADJUST_MAX_OPS tables, the AEJ_ADJUST_LUT ones filled
    Spans spans;                       // per image: its source, its output (in the output's own elements)
    unsigned char *entries_dev, *luts_dev, *tables_dev;
    unsigned *hists_dev;
    long long n_hists;
    unsigned long long bytes;          // the workspace
};
// Image.blend's sample (the enhancers of adjust.hip, AEJ_COMPOSE_BLEND of compose.hip): the product and the sum are rounded separately
__device__ __forceinline__ int ad_blend(int d, int s, float a, bool inside)
{
    const float t = __fadd_rn((float)d, __fmul_rn(a, (float)(s - d)));
    if (inside) return (int)t;
    return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}
int adjust_resolve(const aej_adjust_desc &d, int n_tables, aej_adjust_plan &p, const char **why);      // aej_adjust_plan_host
int adjust_plan(const aej_adjust_desc *descs, int n, const unsigned char *tables_host, int n_tables, bool histogram, void *workspace,
                const unsigned char *src, unsigned char *dst, AdPlan &plan, int *bad, const char **why);
hipError_t launch_adjust(hipStream_t st, const AdPlan &plan);

}  // namespace aej

// compose.hip: Pillow's paste, alpha_composite, blend, composite and ImageChops on packed 8-bit images of 1 to 4 channels (aej_compose_*)
namespace aej {
constexpr int kCpThreads = 256;
constexpr int kCpChunk = 4096;         // pixels of one output image a workgroup takes at a time, in k_adjust_apply's lane groups
constexpr int kCpMaxGrid = 16384;      // workgroups of a launch; the chunks beyond are reached by striding
constexpr int kCpMaxSide = 32767;
struct CpEntry {                       // one element of one launch
    const unsigned char *base;         // bw pixels a row, the output's channels a pixel
    const unsigned char *over;         // ow pixels a row, oc bytes a pixel; null: `colour`
    const unsigned char *mask;         // ow pixels a row, mc bytes a pixel; null unless mkind is AEJ_COMPOSE_MASK_BIT or _BYTE
    unsigned char *out;                // W x H pixels
    long long chunk_base;              // the first chunk of this element in its launch
    int npix, W, bw, pad;              // npix = W x the output's rows (below 2^30)
    int ox, oy, ow;                    // the overlay's pixel (0, 0) in the output, its row
    int rx0, ry0, rx1, ry1;            // the region, clipped: every pixel in it has an overlay (and mask) pixel
    int kind, op, mkind, oc, mc;
    float alpha, scale, offset;
    unsigned char colour[4];
};
struct CpLaunch { int channels, first, count; long long chunks; };
struct CpPlan {
    std::vector<CpEntry> entries;      // launch by launch, device pointers set (null when only measured)
    std::vector<CpLaunch> launches;
    Spans spans;                       // per element: every source it reads (base, overlay, mask), its output
    unsigned char *entries_dev;
    unsigned long long bytes;          // the workspace
};
int compose_resolve(const aej_compose_desc &d, aej_compose_plan &p, const char **why);      // aej_compose_plan_host
int compose_plan(const aej_compose_desc *descs, int n, void *workspace, const unsigned char *src, unsigned char *dst, CpPlan &plan, int *bad,
                 const char **why);
hipError_t launch_compose(hipStream_t st, const CpPlan &plan);

}  // namespace aej

// convert.hip: Pillow's Image.convert between its 8-bit modes, hue adjustment and ImageOps.colorize on packed 8-bit images (aej_convert_*)
namespace aej {
constexpr int kCvThreads = 256;
constexpr int kCvChunk = 4096;         // pixels of one image a workgroup takes at a time, in k_adjust_apply's lane groups
constexpr int kCvMaxGrid = 16384;      // workgroups of a launch; the chunks beyond are reached by striding
constexpr int kCvMaxSide = 32767;
struct CvEntry {                       // one image of one launch
    const unsigned char *in;           // cin bytes a pixel
    unsigned char *out;                // cout bytes a pixel
    const unsigned char *table;        // AEJ_CONVERT_TABLE: its 768 bytes
    long long chunk_base;              // the first chunk of this image in its launch
    long long npix;
    int kind, n_steps, hue, ycc;       // ycc: a step reads the YCbCr tables
    int from[2], to[2];                // AEJ_MODE_* of each step
    float m[12];
};
struct CvLaunch { int cin, cout, first, count; long long chunks; };
struct CvPlan {
    std::vector<CvEntry> entries;      // launch by launch, device pointers set (null when only measured)
    std::vector<CvLaunch> launches;
    std::vector<unsigned char> tables; // the call's tables, as tables_host has them
    Spans spans;                       // per image: its source, its output
    unsigned char *entries_dev, *tables_dev;
    unsigned long long bytes;          // the workspace
};
int convert_resolve(const aej_convert_desc &d, int n_tables, aej_convert_plan &p, const char **why);      // aej_convert_plan_host
int convert_plan(const aej_convert_desc *descs, int n, const unsigned char *tables_host, int n_tables, void *workspace,
                 const unsigned char *src, unsigned char *dst, CvPlan &plan, int *bad, const char **why);
hipError_t launch_convert(hipStream_t st, const CvPlan &plan);

}  // namespace aej

// png.hip: the scanline un-filter of PNG files and their expansion to the output layout (aej_png_unfilter_batch), one workgroup per work
// item: a non-interlaced file, or one non-empty Adam7 pass of an interlaced one (the kernel finds a pass's geometry from its file's)
namespace aej {

constexpr int kPngGroup = 64;          // files per launch: their table travels in the kernel's arguments, so nothing is uploaded
struct PngFile {
    long long in_off;                  // its filtered scanlines in `inflated`, at a multiple of 4: H x (1 + rb) bytes, or its passes back to back
    long long out_off;                 // its image in `out`; of an interlaced file its pass images in the workspace (PngAdam7File::img_off)
    long long carry_off;               // its carried scanline in the workspace (png_carry_bytes), a multiple of 256; an interlaced file's: one
                                       // per non-empty pass, back to back
    long long raw_bytes;               // the inflated size the file must have (of an interlaced file: all its passes)
    int W, H, rb;                      // pixels per row, rows, bytes per row without the filter byte
    int item;                          // -1, or for an interlaced file: the status word of its pass p is int item + p of the workspace
    unsigned char bpp;                 // the filters' distance to the byte "to the left": bytes per whole pixel (1 .. 8), 1 for the packed depths
    unsigned char depth, ct;           // bit depth (1, 2, 4, 8, 16), colour type (0, 2, 3, 4, 6)
    unsigned char oc;                  // bytes per pixel of the image written: 1 .. 4
};
struct PngGroup { PngFile f[kPngGroup]; };
long long png_carry_bytes(int rb, int bpp);
// files first .. first + count of the call (count <= kPngGroup); the per-file arrays are the whole call's
void launch_png_unfilter(hipStream_t st, const PngGroup &grp, int first, int count, const unsigned char *inflated, const long long *inflate_out_bytes,
                         const int *inflate_status, const unsigned char *palettes, unsigned char *out, unsigned char *workspace, int *status);

// Adam7 (PNG specification, section 8.2): pass p = 0 .. 6 holds the pixels (x0 + i dx, y0 + j dy) of the image
struct Adam7Pass { int x0, y0, sx, sy, w, h; };      // dx = 1 << sx, dy = 1 << sy; w x h pixels, either 0 for an empty pass
__host__ __device__ inline Adam7Pass adam7_pass(int W, int H, int p)
{
    Adam7Pass a;
    a.x0 = (0x0402010 >> (4 * (6 - p))) & 15;        // 0 4 0 2 0 1 0
    a.y0 = (0x0040201 >> (4 * (6 - p))) & 15;        // 0 0 4 0 2 0 1
    a.sx = (0x3322110 >> (4 * (6 - p))) & 15;        // 8 8 4 4 2 2 1
    a.sy = (0x3332211 >> (4 * (6 - p))) & 15;        // 8 8 8 4 4 2 2
    a.w = W > a.x0 ? (W - a.x0 + (1 << a.sx) - 1) >> a.sx : 0;
    a.h = H > a.y0 ? (H - a.y0 + (1 << a.sy) - 1) >> a.sy : 0;
    if (a.w == 0 || a.h == 0) a.w = a.h = 0;
    return a;
}
// the pass that holds pixel (x, y)
__host__ __device__ inline int adam7_pass_of(int x, int y)
{
    return y & 1 ? 6 : x & 1 ? 5 : y & 2 ? 4 : x & 2 ? 3 : y & 4 ? 2 : x & 4 ? 1 : 0;
}
// the interleave of the pass images of interlaced files into their images (png_adam7_interleave_kernel), kPngGroup files per launch
struct PngAdam7File {
    long long out_off;                 // its image in `out`
    long long img_off;                 // its pass images in the workspace, a multiple of 4: pass p behind pass p - 1, each w x h x oc rounded up to 4
    int W, H, oc;
    int file;                          // its status word in `status`: the largest of its passes'
    int item;                          // the status word of its pass p is int item + p of the workspace
};
struct PngAdam7Group { PngAdam7File f[kPngGroup]; };
void launch_png_adam7_interleave(hipStream_t st, const PngAdam7Group &grp, int count, int max_height, const unsigned char *workspace,
                                 unsigned char *out, int *status);
// the scanline filter of png_encode_many (aej_png_filter_batch): one wave per row, kPngGroup images per launch
struct PngEncImage {
    const unsigned char *src;          // H rows of rb bytes, contiguous (any alignment)
    long long dst_off;                 // its scanline stream in `out`: H x (1 + rb) bytes
    int rb, H;                         // bytes per row, rows
    int row0;                          // its first row among the launch's rows
    int bpp;                           // bytes per pixel: 1 .. 4
};
struct PngEncGroup { PngEncImage f[kPngGroup]; };
void launch_png_filter(hipStream_t st, const PngEncGroup &grp, int count, int rows, int optimize, unsigned char *out);

}  // namespace aej
