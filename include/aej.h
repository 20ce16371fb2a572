/*
 * aej.h -- C ABI of libaejpeg_hip.so: the MI355X (gfx950) implementation of the adaptive-JPEG
 * ENCODE hot path of fevzibabaoglu/adaptive-edge-aware-jpeg.
 *
 * The reference is pure Python and has no FFI; its boundary for this path is the Python API
 * (src/jpeg/jpeg.py:240-272 Jpeg.compress, src/jpeg/edge_detection.py:28 EdgeDetection.canny,
 * src/jpeg/quadtree.py:71 QuadTree, src/color/conversion.py:95 convert).  Each entry point below
 * names the reference interface it replaces; INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.  Citations are path:line under the reference checkout.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP) unless the name ends in _host;
 *   - every function returns 0 on success or a negative aej_status; aej_last_error() gives the text;
 *   - no exceptions cross the ABI; nothing here allocates device memory after aej_create()
 *     except aej_set_settings() (tables) -- the caller owns inputs, outputs and the workspace;
 *   - a context is bound to one HIP device and one stream and is NOT thread-safe (like the
 *     reference's stateful Jpeg object, jpeg.py:256-259); distinct contexts are independent;
 *   - work is enqueued on the context's stream; the blocking calls synchronise it once, at their end (aej_encode_batch_begin
 *     returns without waiting); nothing inside a call depends on a value read back from the device.
 */
#ifndef AEJ_H
#define AEJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AEJ_ABI_VERSION 3   /* 2: the hysteresis completes on the device -- the speculation entry points of version 1 are gone; aej_set_option.
                             * 3: the entropy stage keeps its parse in the workspace (aej_deflate_histogram / _batch signatures, table layout); aej_pack_u8_levels_host */

#if defined(__GNUC__)
#define AEJ_API __attribute__((visibility("default")))
#else
#define AEJ_API
#endif

typedef struct aej_ctx aej_ctx;

typedef enum aej_status {
    AEJ_OK = 0,
    AEJ_ERR_ARG = -1,        /* bad argument (ValueError on the Python side)          */
    AEJ_ERR_HIP = -2,        /* a HIP runtime call failed                             */
    AEJ_ERR_STATE = -3,      /* settings not set / plan mismatch                      */
    AEJ_ERR_CAPACITY = -4,   /* an output or the workspace is too small               */
    AEJ_ERR_UNSUPPORTED = -5 /* shape/ratio combination not built     */
} aej_status;

/* colour spaces: keys of JpegCompressionSettings.COLOR_SPACE_SETTINGS (jpeg.py:62-147) */
typedef enum aej_space {
    AEJ_YCBCR = 0, AEJ_YCOCG = 1, AEJ_YCOCG_R = 2, AEJ_OKLAB = 3, AEJ_ICTCP = 4, AEJ_ICACB = 5, AEJ_JZAZBZ = 6,
    AEJ_XYZ = 7 /* aej_color_convert / aej_color_convert_inverse only (conversion.py:63-68); not a codec space */
} aej_space;

#define AEJ_MAX_SIZES 8 /* a block-size range spans at most 8 powers of two between 2 and 1024 (the GUI offers 2..256, src/gui/main_frame.py:41-45;
                         Jpeg itself takes any power of two, jpeg.py:216-219) */

/* Shapes and capacities for one (batch, H, W) under the current settings.  Layer l of image b lives at
 * element offset  b*<x>_stride + <x>_off[l]  of the corresponding output array. */
typedef struct aej_plan {
    int32_t batch, H, W;
    int32_t layer_h[3], layer_w[3]; /* Jpeg._compute_downsampled_shapes, jpeg.py:676-686          */
    int32_t root_size[3];           /* QuadTree root size, quadtree.py:89-90                         */
    int64_t coeff_off[3], coeff_stride; /* int32 coefficients, capacity per layer = coeff_off[l+1]-coeff_off[l] */
    int64_t leaf_off[3], leaf_stride;   /* leaves, 4 x int32 each: x, y, size, coeff offset in layer  */
    int64_t state_off[3], state_stride; /* state symbols, one uint8 each: 0 leaf, 1 internal, 2 absent */
    uint64_t workspace_bytes;
} aej_plan;

/* ---- lifetime ------------------------------------------------------------------------------- */
AEJ_API int aej_abi_version(void);
AEJ_API aej_ctx *aej_create(int device, void *hip_stream /* hipStream_t or NULL = null stream */);
AEJ_API void aej_destroy(aej_ctx *ctx);
AEJ_API const char *aej_last_error(aej_ctx *ctx); /* host string owned by ctx (or a static one if ctx==NULL) */
AEJ_API int aej_synchronize(aej_ctx *ctx);
/* Re-binds the context to another stream of its device (the Python host follows torch's current stream with it, so
 * that the library's kernels are ordered behind whatever produced the caller's tensors); drains the stream it leaves. */
AEJ_API int aej_set_stream(aej_ctx *ctx, void *hip_stream);

/* Stage timing of aej_encode_batch: HIP events recorded on the context's stream around every stage of the
 * last call (measurement only; used by bench.py for the roofline figures). */
enum {
    AEJ_STAGE_CLEAR = 0, AEJ_STAGE_COLOR_PLANES, AEJ_STAGE_CLAHE_LUT, AEJ_STAGE_CLAHE_BLUR, AEJ_STAGE_THRESHOLDS,
    AEJ_STAGE_SOBEL_NMS, AEJ_STAGE_HYSTERESIS, AEJ_STAGE_QUADTREE, AEJ_STAGE_DCT_2, AEJ_STAGE_DCT_4, AEJ_STAGE_DCT_8,
    AEJ_STAGE_DCT_16, AEJ_STAGE_DCT_32, AEJ_STAGE_DCT_64, AEJ_STAGE_DCT_128, AEJ_STAGE_DCT_256, AEJ_STAGE_DCT_512, AEJ_STAGE_DCT_1024,
    AEJ_N_STAGES
};
/* Diagnostic.  The hysteresis of cv.Canny (edge_detection.py:85) is two launches whatever the image holds: a pass over every 64 x 64 tile,
 * then a device-side work queue of the tiles whose neighbourhood changed, drained to the fix-point by one persistent launch -- the host
 * guesses no pass count and reads nothing back.  out_host[2] = { whole-path calls since aej_create, tiles that went through that queue
 * in the last completed call }. */
AEJ_API int aej_get_hysteresis_stats(aej_ctx *ctx, int64_t *out_host);
/* Launch-latency path: aej_encode_batch can replay its whole launch sequence (about 20 kernel launches) as one
 * captured hipGraph, cached per (buffers, shape).  mode 0 = never (the default: on MI355X / ROCm 7.2 the replay of one 1080p encode measured 0.287 ms against 0.274 ms for
 * the eager launches), 1 = automatic (calls of at most 8 Mpx), 2 = whenever possible.  The graph runs on a private stream ordered behind the context's
 * stream; results are identical.  out_host[3] = { graph launches, graph captures, graphs cached }. */
AEJ_API int aej_set_graph_mode(aej_ctx *ctx, int mode);
/* Throughput path: aej_encode_batch cuts a large call into sub-batches (contiguous image ranges, the unit the reference's sweep
 * hands to one worker, metrics_computation.py:253) that run the whole chain on private streams, each one stage behind the previous,
 * so that the HBM-bound stages of one sub-batch (colour planes, DCT) run beside the issue-bound stages of another (blur, Sobel / NMS,
 * quadtree).  n = 0: automatic (the default: by call size -- 4 sub-batches from 384 Mpx / 16 images, 2 from 64 Mpx / 8 images -- when the
 * process runs with GPU_MAX_HW_QUEUES >= 8, so that every stream has a hardware queue of its own; with HIP's default of 4 queues: 2
 * sub-batches, and only while no other context has a call in flight), 1: never, 2..8: that many.
 * Outputs are identical; the call still returns with everything complete.  aej_encode_plan's workspace_bytes covers every split. */
AEJ_API int aej_set_sub_batches(aej_ctx *ctx, int n);
/* How many hardware queues the HIP runtime of this process maps its streams onto (GPU_MAX_HW_QUEUES as it was when the runtime
 * initialised; HIP's default is 4).  The library cannot see that value -- the environment may have been changed after the runtime
 * read it -- so the HOST states it: aej_create assumes 4 (the conservative schedule) and the Python package passes what it knows
 * (adaptive_edge_aware_jpeg_amd/_lib.py: the variable's value when the package was imported before the first HIP call, 4 otherwise).
 * aej_get_schedule_host: out_host[4] = { hardware queues assumed, sub-batches the automatic mode would use for (batch, H, W) right now,
 * 1 when fewer than 8 queues force the two-sub-batch schedule for a call the 4-sub-batch one would serve better, the queues the
 * sub-batch streams spread over: the first word times the stream-priority levels in use ("stream_priorities" below), the first word
 * itself when no stream gets a priority }.  aej_set_hw_queues refuses (AEJ_ERR_ARG) a count that "stream_priorities" = 2 would take
 * past 32 queues. */
AEJ_API int aej_set_hw_queues(aej_ctx *ctx, int n);
AEJ_API int aej_get_schedule_host(aej_ctx *ctx, int batch, int H, int W, int32_t *out_host);
/* Tuning and A / B options of one context.  The library reads NO environment variable: whatever changes which kernel or launch shape
 * serves a stage is said here, by the caller, per context (and reported back by aej_get_option).  Every option leaves the results
 * bit-identical; the defaults are the measured best on MI355X.  Unknown name or value outside the range: AEJ_ERR_ARG.
 *   name                    values             meaning
 *   "color_strip"           0 | 1 (default 1)  0: never the persistent strip colour kernel (the 128 x 16 kernel instead)
 *   "color_strip_rows"      0 | 16..64 (0)     strip height of that kernel; 0 = automatic
 *   "color_workgroups"      0..65536 (0)       workgroups of its persistent launch; 0 = automatic (256 for the matrix spaces)
 *   "planes_row_major"      0 | 1 (0)          1: normalised planes row-major in the workspace (default: 4 x 4 blocks where possible)
 *   "dct64_kernel"          0 | 1 | 4 (0)      64 x 64 DCT: 0 = by company (one wave per leaf alone, four beside other work), 1 / 4 force
 *   "dct_small_workgroups"  0..65536 (0)       cap on the grids of the 4 / 8 / 16 DCT kernels; 0 = automatic
 *   "sobel_lds"             0 | 1 (0)          1: the LDS-tiled Sobel / NMS kernel for every shape (default: register kernel when w % 4 == 0)
 *   "dct_multi"             0 | 1 (1)          1: calls of at most 8 Mpx run the DCTs of block sizes 4 .. 64 as ONE launch (latency), 0: one launch per size
 *   "sobel_xcd"             0 | 1 (1)          1: each XCD gets a contiguous range of the register Sobel kernel's tiles (0: round-robin)
 *   "qt_chunks"             0 | 1 (1)          1: with min block 4 the quadtree's count / emit kernels cover the in-plane chunks only, several per
 *                                              wave, and count from ballot masks (0: one wave per chunk of the Morton root square)
 *   "qt_chunk_run"          0..16 (0)          chunks per wave of those kernels; 0 = automatic (1 .. 16, sized for about 4096 waves per call)
 *   "qt_chunk_launches"     counter            quadtree stages the chunk-run kernels have served on this context (read it with
 *                                              aej_get_option; setting it, usually to 0, restarts the count)
 *   "sub_chain"             -1..3 (-1)         which stage of the previously enqueued part a part's colour stage waits for: 0 none, 1 colour,
 *                                              2 blur, 3 Sobel; -1 = 1
 *   "stream_priorities"     0 | 1 | 2 (1)      sub-batch streams created with stream priorities: the HIP runtime keeps one pool of hardware
 *                                              queues per priority level, each up to GPU_MAX_HW_QUEUES, so the sub-batch streams get queues
 *                                              beside the ones the caller's streams share.  0: never; 1: when the host states fewer than 8
 *                                              hardware queues (with 8 or more nothing changes); 2: always (A / B runs; refused when queues x
 *                                              levels would pass the 32 queues a process may hold).  Streams made under another value are
 *                                              replaced by the next split call.  The caller's stream and the graph stream are never touched.
 *   "stream_priority_pattern" 0..3 (3)         the levels dealt to those streams, process-wide in creation order: 0 normal / high,
 *                                              1 normal / low, 2 normal / high / low, 3 high / low (the measured best; a sub-batch at the
 *                                              normal level beside one at another ran slower than no priorities at all)
 *   "priority_streams"      counter            sub-batch streams this context holds that were created with a priority (read-only)
 *   "jpegdec_subseq_bits"   32..1048576 (2048) bits per subsequence of aej_jpegdec_batch's self-synchronising Huffman decode */
AEJ_API int aej_set_option(aej_ctx *ctx, const char *name, int64_t value);
AEJ_API int aej_get_option(aej_ctx *ctx, const char *name, int64_t *value_host);
/* The two halves of aej_encode_batch / aej_encode_batch_u8 (same arguments; rgb_is_u8 selects the ingest): _begin enqueues the whole
 * call and returns without waiting, _end waits for it and checks the device-side counters.  One call may
 * be in flight per context; until _end returns, the context's other entry points, the workspace and the output buffers must not be
 * used.  Two contexts on two streams, each with its own buffers, keep the GPU busy across calls: while one call drains (hysteresis
 * tail, DCT) the other's colour stage runs (bench.py times this pipeline; the strictly serial figure is reported beside it). */
AEJ_API int aej_encode_batch_begin(aej_ctx *ctx, const void *rgb, int rgb_is_u8, int batch, int H, int W, int32_t *coeffs, int32_t *leaves,
                                   uint8_t *states, int64_t *counts, float *dct_f32, void *workspace, uint64_t workspace_bytes);
AEJ_API int aej_encode_batch_end(aej_ctx *ctx);
AEJ_API int64_t aej_get_split_calls(aej_ctx *ctx);   /* calls since aej_create that ran as sub-batches */
AEJ_API int aej_get_graph_stats(aej_ctx *ctx, int64_t *out_host);
AEJ_API int aej_set_profiling(aej_ctx *ctx, int enable);
AEJ_API int aej_get_stage_ms(aej_ctx *ctx, float *ms_host /* [AEJ_N_STAGES] */);
AEJ_API const char *aej_stage_name(int stage);

/* ---- settings: JpegCompressionSettings + Jpeg.precompute_caches (jpeg.py:150-174, 216-238) ------
 * qmats_host: the integer quantisation matrices of Jpeg._get_quantization_matrix (jpeg.py:707-724),
 * built by the Python host, laid out [layer 0..2][size = bmin, 2*bmin, ..., bmax][size*size] int32.
 * Zigzag orders (jpeg.py:726-766) and DCT bases are derived inside the library. */
AEJ_API int aej_set_settings(aej_ctx *ctx, int space, int bmin, int bmax, const int32_t *qmats_host);

/* ---- whole path: Jpeg.compress up to and including the zigzag gather (jpeg.py:262-270, 579-588) --
 * Any image size up to 65535 pixels a side and 2^29 = 536870912 pixels in all (H x W of one image; AEJ_ERR_UNSUPPORTED above, from the
 * plan, the whole path, decode and every stage entry that takes an image or a plane; the reference has no limit of its own), at most
 * 1024 images a call.  aej_color_convert / _inverse take a pixel count, not an image, and are not bound by it. */
AEJ_API int aej_encode_plan(aej_ctx *ctx, int batch, int H, int W, aej_plan *plan_host);

/* rgb: [batch][H][W][3] float32 in [0,1] (Image.data, image.py:26-36).
 * coeffs / leaves / states: laid out as the plan says.  counts: [batch][3][4] int64 =
 * {n_coeffs, n_leaves, n_states, root_size}.  dct_f32 (optional, may be NULL): pre-quantisation
 * DCT values in raster order per leaf, same offsets as coeffs. */
AEJ_API int aej_encode_batch(aej_ctx *ctx, const float *rgb, int batch, int H, int W,
                     int32_t *coeffs, int32_t *leaves, uint8_t *states, int64_t *counts,
                     float *dct_f32, void *workspace, uint64_t workspace_bytes);

/* Same call for images that are still 8-bit: rgb_u8 is [batch][H][W][3] uint8 and the library forms
 * float32(v) / 255.0f itself (image.py:80, Image.load: `iio.imread(path).astype(np.float32) / 255.0`), so the
 * result is identical to aej_encode_batch on that float image while the input costs 3 B/px instead of 12. */
AEJ_API int aej_encode_batch_u8(aej_ctx *ctx, const uint8_t *rgb_u8, int batch, int H, int W,
                     int32_t *coeffs, int32_t *leaves, uint8_t *states, int64_t *counts,
                     float *dct_f32, void *workspace, uint64_t workspace_bytes);

/* ---- EvaluationMetrics(original, compressed).psnr() / .ssim() / .ms_ssim() (evaluation_metrics.py:50-89) for a batch
 * of image pairs.  img_a, img_b: [batch][H][W][3] float32 in [0,1].  out: device [batch][3] float64 = {psnr (dB), ssim of
 * the 8-bit grey images, ms_ssim}; entries not requested in `which` are NaN.  The metrics are piq 0.8.0's (requirements.txt:22)
 * with the reference's arguments; AEJ_ERR_ARG where piq raises ValueError (image smaller than the 11x11 window after
 * pooling, or smaller than 161x161 for MS-SSIM).  A pair's scores are bit-identical from call to call and whatever the batch
 * around it (fixed-order sums, no atomics).  lpips() is aej_lpips_batch below, with weights the caller supplies. */
enum { AEJ_METRIC_PSNR = 1, AEJ_METRIC_SSIM = 2, AEJ_METRIC_MS_SSIM = 4 };
AEJ_API uint64_t aej_metrics_workspace_bytes(int batch, int H, int W);
AEJ_API int aej_metrics_batch(aej_ctx *ctx, const float *img_a, const float *img_b, int batch, int H, int W, int which,
                      double *out, void *workspace, uint64_t workspace_bytes);

/* ---- EvaluationMetrics.lpips(): LPIPS(net='alex') of lpips 0.1.4 (evaluation_metrics.py:91-109) for a batch of image pairs --------
 * The ScalingLayer ((x*2 - 1 - shift) / scale), AlexNet's `features` trunk up to conv5's ReLU with a tap after each of its five ReLUs,
 * per tap and pixel d = sum_c lin[c] * (n0_c - n1_c)^2 of the channel-normalised features n = f / (sqrt(sum_c f_c^2) + 1e-10), the mean
 * of d over the tap's pixels, and the sum over the taps.  Convolutions and normalisation in float32; the spatial means are accumulated in
 * float64 in a fixed order without atomics, so a result is the same from run to run and element i of a batch equals a batch of one.
 * Images must be at least 31 x 31 (AEJ_ERR_ARG otherwise: torch's second maxpool raises below that).
 *
 * Weights: the caller lists the parameters in the canonical order -- conv1..conv5 each as weight [Cout][Cin][k][k] then bias [Cout]
 * (Cin, Cout, k = 3, 64, 11 / 64, 192, 5 / 192, 384, 3 / 384, 256, 3 / 256, 256, 3), then lin0..lin4 [Cout] -- aej_lpips_param_count()
 * floats, and aej_lpips_pack_weights_host turns them into aej_lpips_weights_bytes() bytes of host memory in the kernels' layout; the
 * caller copies that to the device and passes it as `weights` (it stays caller-owned).
 * aej_lpips_features: the normalised taps of a batch of images into feats (aej_lpips_features_bytes; per image the five taps NHWC float32,
 *   one image after the other) -- computed once, they stand for img_a in every later aej_lpips_batch with the same (H, W).
 * aej_lpips_batch: out[b] (device float64) = LPIPS(img_a[b] or the taps feats_a[b], img_b[b]).  Exactly one of img_a / feats_a is given;
 *   the two give bit-identical results.  img_*: [batch][H][W][3] float32 in [0, 1].
 * Workspace: aej_lpips_workspace_bytes(batch, H, W) for aej_lpips_features and for aej_lpips_batch with feats_a; with img_a
 *   aej_lpips_batch needs aej_lpips_features_bytes(batch, H, W) more (img_a's taps are kept there).  Both calls only enqueue work. */
AEJ_API uint64_t aej_lpips_weights_bytes(void);
AEJ_API int64_t aej_lpips_param_count(void);
AEJ_API int aej_lpips_pack_weights_host(const float *params, int64_t n_params, void *packed_host);
AEJ_API uint64_t aej_lpips_features_bytes(int batch, int H, int W);
AEJ_API uint64_t aej_lpips_workspace_bytes(int batch, int H, int W);
AEJ_API int aej_lpips_features(aej_ctx *ctx, const void *weights, const float *img, int batch, int H, int W, float *feats,
                               void *workspace, uint64_t workspace_bytes);
AEJ_API int aej_lpips_batch(aej_ctx *ctx, const void *weights, const float *img_a, const float *feats_a, const float *img_b, int batch,
                            int H, int W, double *out, void *workspace, uint64_t workspace_bytes);

/* ---- stage entry points (same kernels; used by the Python mirrors and the parity tests) -------- */

/* color.convert("sRGB", space, x)  (conversion.py:95-124): rgb [n][3] -> out [n][3], float32 */
AEJ_API int aej_color_convert(aej_ctx *ctx, int space, const float *rgb, float *out, int64_t n);

/* Jpeg._convert_color_space + _downsample (jpeg.py:262-267): raw (un-normalised) float32 planes,
 * planes[l] has layer_h[l]*layer_w[l] elements at offset plane_off[l]; total = plane_stride per image */
AEJ_API int aej_color_planes(aej_ctx *ctx, const float *rgb, int batch, int H, int W, float *planes_raw,
                     float *planes_norm, uint8_t *planes_u8);

/* EdgeDetection.canny(img2d) (edge_detection.py:28-86): plane float32 [H][W] -> edge uint8 {0,1}.
 * stages (optional): 5*H*W uint8 = scaled, CLAHE, Gaussian, bilateral, NMS map (0 weak,1 none,2 strong);
 * thresholds (optional): 2 int32 = the integer low/high passed to the NMS test. */
AEJ_API uint64_t aej_canny_workspace_bytes(int H, int W);
/* The keyword arguments of EdgeDetection.canny (edge_detection.py:31-40) that are run-time values of the kernels; they apply to
 * aej_canny and to the Canny stage of aej_encode_batch until changed (NULL = the reference's defaults 0.10, 0.30, 0.75, 75, 75,
 * true, which is what Jpeg._block_split uses, jpeg.py:376).  aperture_size = 3, clahe_tile_grid = (4, 4),
 * bilateral_diameter = 5 and gaussian_kernel = 3 are structural (stencil shapes) and not selectable. */
typedef struct aej_canny_params {
    double canny_low_ratio, canny_high_ratio;     /* np.percentile(blur, ratio * 100) */
    double clahe_clip_limit;                      /* cv.createCLAHE(clipLimit=...); <= 0 disables clipping */
    double bilateral_sigma_color, bilateral_sigma_space;
    int use_l2_gradient;                          /* cv.Canny(L2gradient=...) */
} aej_canny_params;
AEJ_API int aej_set_canny_params(aej_ctx *ctx, const aej_canny_params *params);
AEJ_API int aej_canny(aej_ctx *ctx, const float *plane, int H, int W, uint8_t *edge, uint8_t *stages,
              int32_t *thresholds, void *workspace, uint64_t workspace_bytes);

/* QuadTree(edge, max_size, min_size).get_leaves_and_states() (quadtree.py:71-165).
 * edge: uint8 [H][W], non-zero == edge.  leaves: [cap][4] int32 (x, y, size, coeff offset);
 * states: uint8 symbols; counts: 4 int64 = {n_coeffs, n_leaves, n_states, root_size}. */
AEJ_API uint64_t aej_quadtree_workspace_bytes(int H, int W, int min_size, int max_size);
AEJ_API int aej_quadtree_capacity(int H, int W, int min_size, int max_size, int64_t *leaf_cap, int64_t *state_cap,
                          int64_t *coeff_cap);
AEJ_API int aej_quadtree(aej_ctx *ctx, const uint8_t *edge, int H, int W, int min_size, int max_size,
                 int32_t *leaves, uint8_t *states, int64_t *counts, void *workspace, uint64_t workspace_bytes);

/* gather + reflect pad + DCT + quantise + zigzag (jpeg.py:393-404, 471, 499-502, 579-588) for the leaves
 * of one layer.  norm: normalised plane [H][W]; leaves: [n][4] as produced by aej_quadtree;
 * coeffs: sum(size^2) int32; dct_f32 optional. Uses the quantisation matrices of `layer` from the
 * current settings. */
AEJ_API int aej_dct_quant_zigzag(aej_ctx *ctx, const float *norm, int H, int W, int layer, const int32_t *leaves,
                         int64_t n_leaves, int32_t *coeffs, float *dct_f32);

/* ---- OPT-IN entropy stage on the GPU: every layer's coefficient array as a zlib stream ---------------------------
 * The container's per-layer streams are `zlib.compress(coeffs.tobytes(), level=9)` in the reference (jpeg.py:588-590) and are read back
 * with `zlib.decompress` (jpeg.py:659) -- which accepts ANY conforming zlib stream.  With the hot path on the GPU that host call is the
 * whole of Jpeg.compress end to end, so the library can write the streams itself (csrc/deflate.hip): ONE deflate block per stream, LZ77
 * matches found by an exact hash-chain search over 32 KiB chunks (window: the chunk), tokens chosen by dynamic programming over a static
 * cost model, coded with RFC 1951's fixed code or -- when `tables` is given, complete for the stream and smaller -- a dynamic code per
 * layer that the HOST builds from the token histogram (aej_deflate_build_tables).  The bytes differ from zlib level 9's (about 1.1 x larger
 * on natural images with the dynamic codes: zlib level 6's size); the decoded coefficients are identical.  Never the default.
 * coeffs / counts: aej_encode_batch's outputs (counts is the DEVICE array; a count outside its layer's capacity returns AEJ_ERR_ARG).
 * aej_deflate_histogram: match search + parse of every stream.  The tokens stay in `workspace`; hist = device [3][AEJ_DEFLATE_HIST_BINS]
 *   int32: per layer (summed over the batch) the occurrences of the 286 literal / length symbols, then of the 30 distance symbols.
 * aej_deflate_batch: tables = device [3][AEJ_DEFLATE_TABLE_WORDS] uint32 or NULL (fixed code everywhere).  reuse_parse != 0: the tokens
 *   aej_deflate_histogram left in this workspace for these very coeffs / counts are used (the usual sequence: histogram -> build tables ->
 *   batch); 0: the streams are parsed again first.  The stream of (image b, layer l) is written at streams + (3 b + l) * stream_stride
 *   (4-byte aligned, stride a multiple of 4), its length to sizes[3 b + l] (device int64).  aej_deflate_stream_bound(raw bytes) is always
 *   enough for stream_stride; a stream that does not fit returns AEJ_ERR_CAPACITY.  Both calls synchronise the context's stream. */
#define AEJ_DEFLATE_HIST_BINS 320
#define AEJ_DEFLATE_TABLE_WORDS 448
AEJ_API uint64_t aej_deflate_stream_bound(uint64_t raw_bytes);
AEJ_API uint64_t aej_deflate_workspace_bytes(aej_ctx *ctx, int batch, int H, int W);
AEJ_API int aej_deflate_histogram(aej_ctx *ctx, const int32_t *coeffs, const int64_t *counts, int batch, int H, int W, int32_t *hist, void *workspace,
                                  uint64_t workspace_bytes);
/* HOST-only helper (no context, no device work): the three layers' dynamic codes from the histograms above, copied to the host --
 * hist_host [3][AEJ_DEFLATE_HIST_BINS], tables_host [3][AEJ_DEFLATE_TABLE_WORDS].  Layout of a table: [0..285] literal / length symbols as
 * `bit-reversed code | nbits << 16`, [286..315] the distance symbols likewise, [316] number of block-header bits, [317..] those bits, LSB
 * first (BFINAL = 1, BTYPE = 10, HLIT / HDIST / HCLEN, the run-length coded code lengths).  tests/deflate_reference.py is the readable
 * restatement (tests compare the two word for word).  cover_all [3] or NULL (= all 1): 1 = every symbol gets a code (a table valid for
 * any data), 0 = only the symbols counted (shorter block headers; a stream that needs a missing code is written with the fixed code). */
AEJ_API int aej_deflate_build_tables(const int32_t *hist_host, const int32_t *cover_all, uint32_t *tables_host);
AEJ_API int aej_deflate_batch(aej_ctx *ctx, const int32_t *coeffs, const int64_t *counts, int batch, int H, int W, const uint32_t *tables, int reuse_parse,
                              uint8_t *streams, uint64_t stream_stride, int64_t *sizes, void *workspace, uint64_t workspace_bytes);

/* The same stage on BYTE streams of mixed lengths, one zlib stream per file (png_encode_many(entropy="gpu"): the filtered scanlines).
 * Matches start at any byte position, in chunks of 8192 positions with up to 24576 bytes of history; the distances always tried are
 * 1, bpp, 2 bpp, stride -+ bpp and up to 16 multiples of the stride, the rest comes from exact hash chains over the chunk and the 8192 bytes before it.  One deflate block
 * per stream: the file's dynamic code (aej_deflate_bytes_build_tables over its histogram) or the fixed code when that is smaller.
 * descs_host: [n][6] int64 = offset of the stream in `in` (a multiple of 4; whole dwords are read, so the length rounded up to 4 must
 *   lie inside in_bytes), its bytes (1 .. 2^40), bytes per pixel (1 .. 4), bytes per scanline (stride, 1 .. 2^26), offset and size of
 *   its slot in `out` (multiples of 4, at least 16 bytes; read by aej_deflate_bytes_batch only).
 * aej_deflate_bytes_workspace_bytes: 0 for lengths outside the range.  aej_deflate_bytes_histogram: parse; hist = device
 *   [n][AEJ_DEFLATE_HIST_BINS].  aej_deflate_bytes_build_tables (host only): tables_host [n][AEJ_DEFLATE_TABLE_WORDS] with codes for the
 *   symbols that occur.  aej_deflate_bytes_batch: tables = device [n][AEJ_DEFLATE_TABLE_WORDS] or NULL; reuse_parse as above; the
 *   stream of file i goes to its slot, its length to sizes[i] (device int64).  aej_deflate_stream_bound(bytes) is always enough for a
 *   slot; a stream that does not fit returns AEJ_ERR_CAPACITY and is not written.  `in`, `out` 4-byte, workspace 256-byte aligned.
 *   Both device calls synchronise the context's stream.  The same input gives the same bytes. */
AEJ_API uint64_t aej_deflate_bytes_workspace_bytes(const int64_t *descs_host, int n);
AEJ_API int aej_deflate_bytes_histogram(aej_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const int64_t *descs_host, int n, int32_t *hist, void *workspace,
                                        uint64_t workspace_bytes);
AEJ_API int aej_deflate_bytes_build_tables(const int32_t *hist_host, int n, uint32_t *tables_host);
AEJ_API int aej_deflate_bytes_batch(aej_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const int64_t *descs_host, int n, const uint32_t *tables, int reuse_parse,
                                    uint8_t *out, uint64_t out_bytes, int64_t *sizes, void *workspace, uint64_t workspace_bytes);

/* HOST-only helper (no context, no device work) for the 8-bit ingest of HOST images (src/image/image.py:80 makes every
 * loaded image `uint8.astype(float32) / 255.0`): if every one of the n float32 values at rgb_host is bit for bit float32(k) / 255.0f for
 * some k in 0..255, the levels k are written to u8_host and 1 is returned -- the caller then uploads 3 B per pixel instead of 12 and
 * calls aej_encode_batch_u8, whose outputs are identical; otherwise 0 (u8_host is then undefined; the pass stops at the first block that
 * holds another value).  `threads` host threads share the pass (clamped to 1..64). */
AEJ_API int aej_pack_u8_levels_host(const float *rgb_host, int64_t n, uint8_t *u8_host, int threads);

/* ---- decode path: Jpeg.decompress after the host-side entropy decode (jpeg.py:285-296) ------
 * coeffs / leaves / counts use the layout of aej_encode_batch's outputs (so an encoded batch can be decoded in
 * place); counts is a DEVICE array [batch][3][4], only n_leaves is read.  rgb_out: [batch][H][W][3] float32 in [0,1]
 * (Jpeg._dequantize, _apply_inverse_dct, _block_merge, _upsample, _convert_color_space_inverse).
 * The leaf tables must tile every layer (aej_encode_batch's output does; Jpeg.decompress checks a parsed stream on the host
 * with aej_leaf_positions_host): a table that does not fit the plan -- n_leaves beyond the layer's capacity, a size outside
 * the settings' block range, an origin outside the layer, a coefficient offset outside the layer's span, more leaves of one size
 * than can exist -- returns AEJ_ERR_ARG instead of touching memory it
 * does not own; pixels no leaf covers are left undefined (the reference starts from np.zeros, jpeg.py:421). */
AEJ_API uint64_t aej_decode_workspace_bytes(aej_ctx *ctx, int batch, int H, int W);
AEJ_API int aej_decode_batch(aej_ctx *ctx, const int32_t *coeffs, const int32_t *leaves, const int64_t *counts, int batch, int H,
                             int W, float *rgb_out, void *workspace, uint64_t workspace_bytes);
/* aej_decode_batch with the dequantisation tables taken from a device buffer instead of the context: qmats_dev is ONE set laid out as
 * aej_set_settings' qmats_host ([layer 0..2][size = bmin .. bmax][size*size] int32, raster order, no padding) for the block range the
 * context is bound to; colour space, block range, zigzag orders and DCT bases stay the context's.  Same preconditions, checks and
 * completion as aej_decode_batch (it waits for its one check word); the quantisers are used as given. */
AEJ_API int aej_decode_batch_tables(aej_ctx *ctx, const int32_t *coeffs, const int32_t *leaves, const int64_t *counts, int batch, int H, int W,
                                    const int32_t *qmats_dev, float *rgb_out, void *workspace, uint64_t workspace_bytes);

/* ---- requantisation for rate-distortion sweeps: Jpeg.compress under other quality ranges without colour, Canny, quadtree or DCT work ----
 * The quality range only enters the encode through the quantisation matrices (jpeg.py:356-404, 485-506, 688-705), so the coefficients
 * for any other set of matrices follow from the pre-quantisation DCT values of an encode: coefficient i of a leaf of size s is
 * rint(double(Y[zz_s[i]]) / double(Q[zz_s[i]])) -- the very quantiser of the DCT epilogues, bit for bit what aej_encode_batch writes
 * when the context is bound to that set.
 * Preconditions: the context is bound (aej_set_settings) to the colour space and block range that produced the leaves; dct_f32, leaves
 * and counts are aej_encode_batch's outputs for (batch, H, W) (dct_f32 requested from it; counts is the DEVICE array).
 * qmats_dev: device [n_sets][layer 0..2][size = bmin .. bmax][size*size] int32, each set laid out as aej_set_settings' qmats_host.
 * Set j is written at coeffs_out + j * set_stride_elems in aej_encode_batch's coefficient layout (a drop-in `coeffs` for
 * aej_decode_batch, aej_deflate_* and the container); entries beyond a layer's n_coeffs are left untouched.  set_stride_elems must be
 * at least batch * coeff_stride when n_sets > 1 (16-byte aligned sets write with 16-byte stores).
 * A leaf table that does not fit the plan (n_leaves over capacity, a size outside the bound block range, an origin outside the layer, a
 * coefficient offset outside the layer's span) or a quantiser < 1 returns AEJ_ERR_ARG and nothing is written.  The call enqueues a check
 * and the requantisation on the context's stream and waits only for the check word. */
AEJ_API int aej_requantise_batch(aej_ctx *ctx, const float *dct_f32, const int32_t *leaves, const int64_t *counts, int batch, int H, int W,
                                 int n_sets, const int32_t *qmats_dev, int32_t *coeffs_out, uint64_t set_stride_elems);
/* color.convert(space, "sRGB", x) (conversion.py:122-124): in [n][3] -> sRGB [n][3], float32 */
AEJ_API int aej_color_convert_inverse(aej_ctx *ctx, int space, const float *in, float *out_rgb, int64_t n);
/* HOST helper (no device): leaf positions from leaf sizes, the walk of Jpeg._block_merge (jpeg.py:424-448).
 * sizes_host [n] -> xy_host [n][2]; returns the number of leaves placed (== n for a well-formed stream), or -2 when the n
 * leaves leave a part of the layer uncovered. */
AEJ_API int64_t aej_leaf_positions_host(const int32_t *sizes_host, int64_t n, int root, int H, int W, int32_t *xy_host);

/* ---- .ajpg containers decoded on the device (Jpeg.decompress_many): the entropy decode and the quadtree headers ------------------
 * Both calls only enqueue work on the context's stream (no synchronisation, no read-back); their per-stream / per-layer status arrays
 * stay on the device for the caller.  The inflate needs no workspace (its state lives in LDS).
 *
 * aej_inflate_batch: n zlib streams (RFC 1950 / 1951: stored, fixed and dynamic blocks, Adler-32 checked, bytes after the trailer ignored),
 *   one wave per stream.  streams: device [n][4] int64 = { input offset in src (bytes, a multiple of 4), input length, output offset in dst
 *   (bytes, a multiple of 4), output capacity (bytes) }; src and dst must be 4-byte aligned.  A stream writes only inside
 *   [out_off, out_off + cap), which must lie inside dst_bytes.  out_bytes[i] (device int64): bytes decoded; status[i] (device int32):
 *   AEJ_INFLATE_*.  A bad stream leaves the others alone. */
enum {
    AEJ_INFLATE_OK = 0, AEJ_INFLATE_BAD_HEADER = 1 /* CM, CINFO, FCHECK or FDICT */, AEJ_INFLATE_BAD_BLOCK_TYPE = 2,
    AEJ_INFLATE_BAD_CODE_LENGTHS = 3 /* over-subscribed / incomplete code, bad repeat, too many symbols */,
    AEJ_INFLATE_BAD_SYMBOL = 4 /* a code that is not in the table, literal / length 286-287, distance 30-31 */,
    AEJ_INFLATE_DISTANCE_TOO_FAR = 5, AEJ_INFLATE_STORED_LENGTH = 6 /* LEN != ~NLEN */, AEJ_INFLATE_TRUNCATED = 7,
    AEJ_INFLATE_OVER_CAPACITY = 8, AEJ_INFLATE_ADLER = 9, AEJ_INFLATE_BAD_ARG = 10 /* descriptor outside dst or misaligned */
};
AEJ_API int aej_inflate_batch(aej_ctx *ctx, const uint8_t *src, const int64_t *streams, int n, uint8_t *dst, uint64_t dst_bytes,
                              int64_t *out_bytes, int32_t *status);
/* aej_decode_headers: the quadtree header of every layer of a batch (the walks of Jpeg._decode_leaf_sizes and aej_leaf_positions_host, with
 *   every check Jpeg.decompress makes) into the tables aej_decode_batch reads.  layers: device [batch * 3][3] int64 = { offset of the layer's
 *   packed 2-bit state symbols in `states` (the container's packing: first symbol in the top bits of a byte), number of symbols, the root
 *   size the container stores }.  inflated_bytes: device [batch * 3] int64, the size of each layer's decoded coefficient stream.  leaves /
 *   counts: aej_encode_batch's layout (counts[b][l] = { n_coeffs, n_leaves, n_states, root }; a layer in error gets n_coeffs = n_leaves = 0).
 *   status: device [batch * 3] int32, AEJ_HEADER_*.  leaves and workspace 16-byte aligned. */
enum {
    AEJ_HEADER_OK = 0, AEJ_HEADER_TOO_MANY_LEAVES = 1, AEJ_HEADER_BAD_SIZE = 2 /* leaf size outside the settings' block range */,
    AEJ_HEADER_NO_TILING = 3, AEJ_HEADER_COEFF_COUNT = 4 /* inflated bytes != 4 * sum(size^2) */, AEJ_HEADER_BAD_ARG = 5
};
AEJ_API uint64_t aej_decode_headers_workspace_bytes(aej_ctx *ctx, int batch, int H, int W);
AEJ_API int aej_decode_headers(aej_ctx *ctx, const uint8_t *states, const int64_t *layers, const int64_t *inflated_bytes, int batch, int H, int W,
                               int32_t *leaves, int64_t *counts, int32_t *status, void *workspace, uint64_t workspace_bytes);

/* ---- baseline JPEG (the standard-JPEG side of a rate-distortion study) --------------------------------------------------------------
 * Byte-identical to PIL.Image.fromarray(x).save(buf, "JPEG", quality=q) with libjpeg-turbo: JFIF 1.01 (no units, 1:1), 4:2:0, baseline,
 * Annex K quantisation (Pillow's quality scaling, clamped to 1..255) and Huffman tables, islow DCT, no restart markers (the ragged
 * encoder and the transcoder write them: the _rst entries further down).
 * aej_jfif_headers_host: the markers SOI .. SOS of one (quality, H, W) file into out_host; returns their length (623), AEJ_ERR_ARG for a
 *   quality outside 1..100 or H, W outside 1..65535, AEJ_ERR_CAPACITY when capacity is smaller.
 * aej_jfif_encode_batch: rgb is device uint8 [batch][H][W][3]; colour, down-sampling and DCT run once per image, then every one of the
 *   n_q qualities.  File (j, b) -- quality qualities_host[j], image b -- is written at out + offsets[j * batch + b] with length
 *   lengths[j * batch + b] (device int64 [n_q * batch], n_q * batch <= 65535, files packed in that order); *total_host gets their sum.  out may be NULL (sizes
 *   only); if the files do not fit out_capacity nothing is written to out and AEJ_ERR_CAPACITY is returned with *total_host set.  The
 *   call waits for that one word.  Workspace: aej_jfif_workspace_bytes(batch, H, W, n_q) bytes, 256-byte aligned.
 * aej_jfif_recon_batch: the pixels libjpeg-turbo's decoder (islow IDCT, h2v2 fancy up-sampling -- plain replication when the chroma is at
 *   most 2 samples wide) returns for those files, from the quantised coefficients the preceding aej_jfif_encode_batch of the same
 *   (batch, H, W, n_q) left in `workspace`: rgb_out is device uint8 [n_q][batch][H][W][3].  Only enqueues work. */
AEJ_API uint64_t aej_jfif_workspace_bytes(int batch, int H, int W, int n_q);
AEJ_API int aej_jfif_headers_host(int quality, int H, int W, uint8_t *out_host, int capacity);
AEJ_API int aej_jfif_encode_batch(aej_ctx *ctx, const uint8_t *rgb, int batch, int H, int W, int n_q, const int32_t *qualities_host, uint8_t *out,
                                  uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host, void *workspace,
                                  uint64_t workspace_bytes);
AEJ_API int aej_jfif_recon_batch(aej_ctx *ctx, int batch, int H, int W, int n_q, uint8_t *rgb_out, void *workspace, uint64_t workspace_bytes);
/* The same with Pillow's subsampling= and optimize= keywords: subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (Pillow's integers; the MCU is
 * 8 x 8, 16 x 8, 16 x 16 pixels), optimize 0 / 1 = the Annex K Huffman tables / per file the tables libjpeg builds from the counts of that
 * file's own symbols (T.81 K.2; four DHT segments of variable length, never longer than the Annex K ones).  (2, 0) is exactly the calls
 * above; any other value is AEJ_ERR_ARG (workspace size 0).  With optimize the tables are built on the device between quantisation and
 * the bit-offset scan (symbol histogram, one table per wave, bit counts under the new codes); the call still waits once, at its end.
 * aej_jfif_recon_batch_opt takes the options of the encode that filled `workspace`.
 * aej_jfif_headers_host_opt: the markers of a file with the Annex K tables (optimize = 0) of that layout.
 * aej_jfif_huffman_host: HOST only, the routine the device runs per table.  counts_host: 257 symbol counts (entry 256, the reserved
 *   all-ones code, is taken as 1); ties between equal counts go to the larger symbol.  Writes BITS[1..16] to bits_host[16] and the
 *   symbols sorted by code length, then value, to huffval_host; returns their number (<= 256).  AEJ_ERR_ARG for a negative count or
 *   when counts 0..255 are all zero, AEJ_ERR_CAPACITY when capacity is smaller than the number of symbols. */
AEJ_API uint64_t aej_jfif_workspace_bytes_opt(int batch, int H, int W, int n_q, int subsampling, int optimize);
AEJ_API int aej_jfif_headers_host_opt(int quality, int H, int W, int subsampling, uint8_t *out_host, int capacity);
AEJ_API int aej_jfif_huffman_host(const int64_t *counts_host, uint8_t *bits_host, uint8_t *huffval_host, int capacity);
AEJ_API int aej_jfif_encode_batch_opt(aej_ctx *ctx, const uint8_t *rgb, int batch, int H, int W, int n_q, const int32_t *qualities_host,
                                      int subsampling, int optimize, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths,
                                      uint64_t *total_host, void *workspace, uint64_t workspace_bytes);
AEJ_API int aej_jfif_recon_batch_opt(aej_ctx *ctx, int batch, int H, int W, int n_q, int subsampling, int optimize, uint8_t *rgb_out,
                                     void *workspace, uint64_t workspace_bytes);

/* The progressive file of the same call: PIL.Image.fromarray(u8).save(buf, "JPEG", quality=q, subsampling=s, progressive=True) byte for
 * byte -- SOF2 and libjpeg's jpeg_simple_progression of ten scans (DC with successive approximation, luma 1-5 and 6-63, chroma 1-63,
 * then the refinements), every scan under its own optimal Huffman table, so optimize= makes no difference, as in Pillow.  Arguments as
 * the _opt family without `optimize`.  The file is SOI .. SOF2, then per scan [DHT] SOS data, then EOI.  The coefficients are those of
 * the baseline file, so aej_jfif_recon_batch_prog returns the same pixels; it takes the workspace an aej_jfif_encode_batch_prog of the
 * same shape filled.  The workspace is larger than the baseline one (aej_jfif_workspace_bytes_prog; 0 for arguments the call refuses).
 * The Annex G coder runs on the device: what each block emits and leaves pending, a prefix sum, the end-of-band runs cut where
 * libjpeg cuts them (0x7FFF blocks, more than 937 deferred bits), then histogram, tables, bit offsets and emit per scan. */
AEJ_API uint64_t aej_jfif_workspace_bytes_prog(int batch, int H, int W, int n_q, int subsampling);
AEJ_API int aej_jfif_encode_batch_prog(aej_ctx *ctx, const uint8_t *rgb, int batch, int H, int W, int n_q, const int32_t *qualities_host,
                                       int subsampling, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths,
                                       uint64_t *total_host, void *workspace, uint64_t workspace_bytes);
AEJ_API int aej_jfif_recon_batch_prog(aej_ctx *ctx, int batch, int H, int W, int n_q, int subsampling, uint8_t *rgb_out, void *workspace,
                                      uint64_t workspace_bytes);

/* ---- baseline JPEG files decoded on the device (standard_jpeg_decode_many) ---------------------------------------------------------
 * Pixel-identical to PIL.Image.open(file).convert("RGB") with libjpeg-turbo (islow IDCT, fancy up-sampling, fixed-point YCbCr -> RGB).
 * Supported: SOF0 / SOF1 with 8-bit samples, one interleaved scan, 1 component (grey, replicated into RGB) or 3 taken as YCbCr with luma
 * sampling 1x1, 2x1 or 2x2 and chroma 1x1, any DHT (codes up to 16 bits), 8- and 16-bit DQT, DRI / RSTn.  APPn, COM and EXIF are skipped
 * (orientation is ignored, as Image.open ignores it); the tables in force at SOS apply.
 *
 * aej_jpegdec_parse_host: HOST only.  Reads the markers SOI .. SOS of one file into *desc.  Returns 0; AEJ_ERR_UNSUPPORTED for a valid
 *   file outside the supported set (progressive, arithmetic, 12-bit, 2 or 4 components, Adobe transform 0, 'R','G','B' ids without JFIF,
 *   other sampling factors, DNL, a first scan that lists fewer components than the frame); AEJ_ERR_ARG for a malformed header (missing
 *   SOF / SOS, truncated segment, over-subscribed or undefined Huffman table, undefined quantisation table).  msg (may be NULL) gets the
 *   reason.  scan_offset is the first byte after the SOS segment; scan_length runs to the end of the file (the device stops at the
 *   first marker that is not RSTn).
 * aej_jpegdec_batch: n files.  descs_host [n] from the parser; scans: device bytes, the scan of file i at scan_offsets_host[i] (its
 *   scan_length bytes must lie inside scans_bytes); out: device uint8, image i as [height][width][3] at out_offsets_host[i] (inside
 *   out_bytes); status: device [n] int32, AEJ_JPEGDEC_*.  A bad file leaves the others alone and never reads outside its own scan.  The
 *   Huffman decode of a segment without restart markers is split into subsequences of "jpegdec_subseq_bits" bits (aej_set_option) that
 *   decode from a guessed state and are re-run until each one's entry state equals its predecessor's exit state; the call reads back one
 *   word every few of those rounds and returns after the last round has run.  Workspace: aej_jpegdec_workspace_bytes(ctx, descs_host, n)
 *   bytes (it depends on the context's subsequence length), 256-byte aligned.
 * aej_jpegdec_sync_rounds: sync rounds the last aej_jpegdec_batch of the context ran (0 when no segment needed more than one subsequence).
 * aej_jpegdec_batch_scaled / aej_jpegdec_workspace_bytes_scaled: the same calls with scales_host [n], each 1, 2, 4 or 8 (anything else:
 *   AEJ_ERR_ARG, 0 bytes): file i is decoded at 1 / scales_host[i] of its size straight from the coefficients, as libjpeg does for
 *   scale_num / scale_denom = 1 / scale and Pillow after Image.draft() has chosen that scale -- image i is
 *   [ceil(height / scale)][ceil(width / scale)][3] at out_offsets_host[i].  The entropy decode is the same; the reconstruction of a
 *   scaled file is one kernel of reduced IDCTs (4 x 4, 2 x 2, 1 x 1 for luma; 4:2:0 chroma one size larger, so it is not up-sampled)
 *   that needs no sample planes, so the workspace is smaller.  With every scale 1 both calls are aej_jpegdec_batch and
 *   aej_jpegdec_workspace_bytes byte for byte.  (Additions to ABI 3: no existing signature, struct or behaviour changed.)
 * aej_jpegdec_batch_mode / aej_jpegdec_workspace_bytes_mode: the _scaled calls with components_host [n] as well, each 3 or 1 (anything
 *   else: AEJ_ERR_ARG, 0 bytes).  3: image i is [h][w][3] as above.  1: image i is [h][w], h = ceil(height / scale), w = ceil(width /
 *   scale): the samples of a one-component file, the luma plane of a three-component one -- libjpeg's out_color_space = JCS_GRAYSCALE,
 *   Pillow's im.draft("L", ...); NOT a conversion of the RGB image (no ITU-R 601 weighting of clamped R, G, B).  out_offsets_host[i] +
 *   h * w * components must lie inside out_bytes, and exactly those bytes of out are written.  A NULL scales_host means every scale 1,
 *   a NULL components_host every count 3.  The entropy decode is the same (an interleaved scan carries its chroma, which is decoded);
 *   the reconstruction of a luma file is one kernel at every scale, full size included -- the IDCTs of its luma blocks into LDS, then
 *   whole-dword row stores -- that never reads a chroma block, so such a file adds no sample planes to the workspace: that of a call
 *   never exceeds the same call's with every count 3.  With every count 3 both calls are the _scaled ones byte for byte, launches
 *   included.  (Additions to ABI 3: no existing signature, struct or behaviour changed.)
 * aej_jpegdec_batch_box / aej_jpegdec_workspace_bytes_box: the _mode calls with boxes_host [n][4] as well -- left, top, right, bottom in
 *   pixels of the full-size image, Pillow's crop() box, 0 <= left < right <= width and 0 <= top < bottom <= height (anything else:
 *   AEJ_ERR_ARG naming the file, 0 bytes; nothing is padded).  Image i is then [bottom - top][right - left][components]: exactly the
 *   pixels [top, bottom) x [left, right) of what the _mode call gives.  A NULL boxes_host, or a box that is the whole image, is the
 *   _mode call for that file: the same layout, the same launches.  A box on a file whose scale is not 1 is AEJ_ERR_UNSUPPORTED ("a box
 *   at scale 2, 4 or 8 is not built").  Both refusals come before any device work and leave out untouched.  A boxed file is
 *   reconstructed by one kernel, coefficients to the box's pixels, and has no sample planes; of a boxed BASELINE file only the
 *   coefficients of the MCU rows of its window are stored, and a restart segment that holds no MCU of those rows is not Huffman-decoded
 *   (un-stuffing, segment finding and the restart-marker count check still cover the whole scan): status reports errors of the data that
 *   is read alone, so a malformed segment the box does not need goes unnoticed.
 * aej_jpegdec_box_window_host: HOST only.  window4_out_host gets mx0, my0, mx1, my1: the half-open rectangle of MCUs whose blocks the
 *   pixels of box4_host (left, top, right, bottom) of an RGB decode read -- the luma samples of those pixels and, per chroma component,
 *   the co-sited sample plus the one neighbour in each direction that libjpeg's fancy up-sampling filters across, after the edge rules
 *   of the FILE's chroma width and height (a plane at most 2 samples wide is replicated).  AEJ_ERR_ARG for a box outside the image.
 *   (A luma decode reads the luma samples' MCUs alone.)  aej_jpegprog_box_window_host: the same from a progressive file's frame.
 * aej_jpegdec_box_stats: out3_host gets, for the last aej_jpegdec_batch_box of the context in which a file had a box: the restart
 *   segments of its files, those that were Huffman-decoded, and the coefficient blocks stored -- computed on the host from the
 *   descriptors and the windows, nothing is read back.  (Additions to ABI 3: no existing signature, struct or behaviour changed.)
 * aej_jpegdec_batch_sbox / aej_jpegdec_workspace_bytes_sbox: the _box calls with one difference: boxes_host[i] is in pixels of the SCALED
 *   image of file i, ow = ceil(width / scale) by oh = ceil(height / scale) -- Pillow's crop() box of the drafted image, 0 <= left <
 *   right <= ow and 0 <= top < bottom <= oh (anything else: AEJ_ERR_ARG naming the file, 0 bytes, out untouched).  Image i is exactly
 *   [top, bottom) x [left, right) of what the _mode call gives at that scale.  At scale 1 the call is the _box call byte for byte,
 *   launches included; a NULL boxes_host, or a box that is the whole scaled image, is the _mode call for that file.  A file with such
 *   a box at scale 2, 4 or 8 is reconstructed by one kernel from the reduced inverse DCTs of the box's tiles alone, under libjpeg's
 *   up-sampling rules at that scale, and of a BASELINE file only the restart segments and the coefficient rows of the window are
 *   decoded and stored, as in the _box call (aej_jpegdec_box_stats reports these calls too).  The _box entries still refuse a box at
 *   scale 2, 4 or 8.
 * aej_jpegdec_sbox_window_host: HOST only.  aej_jpegdec_box_window_host for a box in pixels of the image at `scale` (1, 2, 4 or 8): the
 *   MCUs -- hs * 8 / scale by vs * 8 / scale scaled pixels each -- whose blocks the box's pixels read.  4:4:4, one-component and 4:2:0
 *   files: the pixel's own MCU (the 4:2:0 chroma IDCT is twice the luma's, so nothing is up-sampled).  4:2:2: one neighbour column after
 *   the edge clamps at scales 2 and 4 when the scaled chroma width (ow + 1) / 2 exceeds 2 (h2v1 fancy), none otherwise (replication).
 *   4:4:0: one neighbour row after the clamps at scales 2 and 4 (h1v2 fancy), none at scale 8.  AEJ_ERR_ARG for a box outside the scaled
 *   image or a scale that is none.  aej_jpegprog_sbox_window_host: the same from a progressive file's frame.
 *   (Additions to ABI 3: no existing signature, struct or behaviour changed.) */
enum {
    AEJ_JPEGDEC_OK = 0, AEJ_JPEGDEC_TRUNCATED = 1 /* the scan ends before the last MCU */, AEJ_JPEGDEC_BAD_CODE = 2 /* not in the table */,
    AEJ_JPEGDEC_RUN_PAST_63 = 3 /* an AC run beyond the block */, AEJ_JPEGDEC_BAD_DC = 4 /* DC category above 11 */,
    AEJ_JPEGDEC_BAD_RESTART = 5 /* a restart marker out of sequence, missing or unexpected */,
    AEJ_JPEGDEC_COEF_RANGE = 6 /* aej_jfif_transcode_batch only: a coefficient an 8-bit JPEG cannot hold (AC beyond +-1023, DC outside -1024 .. 1023) */
};
typedef struct aej_jpegdec_huff {
    uint16_t lut[512];         /* 9-bit look-ahead: (code length << 8) | symbol; 0 = the code is longer than 9 bits */
    int32_t maxcode[18];       /* [l]: largest code of length l (1..16), -1 if none */
    int32_t valoff[18];        /* [l]: symbol of code c of length l is vals[valoff[l] + c] */
    uint8_t vals[256];
} aej_jpegdec_huff;
typedef struct aej_jpegdec_desc {
    int32_t width, height;
    int32_t ncomp;             /* 1 or 3 */
    int32_t hs, vs;            /* luma sampling factors (1x1, 2x1, 2x2; 1x1 for grey) */
    int32_t mcux, mcuy;        /* MCUs per row / column of the scan (grey: one block per MCU) */
    int32_t blocks_per_mcu;    /* hs * vs + 2, or 1 */
    int32_t restart_interval;  /* MCUs per restart segment, 0 = none */
    int32_t n_segments;        /* restart segments of the scan */
    int32_t sof;               /* 0xC0 or 0xC1 */
    int32_t precision16;       /* 1 when a quantisation table in force is 16-bit */
    uint8_t comp_id[4], comp_h[4], comp_v[4], comp_tq[4];    /* frame components (as Pillow's im.layer) */
    uint16_t qt[3][64];        /* quantisation table of each component, natural (row-major) order */
    aej_jpegdec_huff dc[3], ac[3];      /* Huffman tables each component of the scan uses */
    int64_t scan_offset, scan_length;
} aej_jpegdec_desc;
AEJ_API int aej_jpegdec_parse_host(const uint8_t *data_host, uint64_t nbytes, aej_jpegdec_desc *desc_host, char *msg, int msg_capacity);
AEJ_API uint64_t aej_jpegdec_workspace_bytes(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n);
AEJ_API int aej_jpegdec_batch(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const uint8_t *scans, uint64_t scans_bytes,
                              const int64_t *scan_offsets_host, uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host,
                              int32_t *status, void *workspace, uint64_t workspace_bytes);
AEJ_API int64_t aej_jpegdec_sync_rounds(aej_ctx *ctx);
AEJ_API uint64_t aej_jpegdec_workspace_bytes_scaled(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host);
AEJ_API int aej_jpegdec_batch_scaled(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const uint8_t *scans,
                                     uint64_t scans_bytes, const int64_t *scan_offsets_host, uint8_t *out, uint64_t out_bytes,
                                     const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes);
AEJ_API uint64_t aej_jpegdec_workspace_bytes_mode(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host,
                                                  const int *components_host);
AEJ_API int aej_jpegdec_batch_mode(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const int *components_host,
                                   const uint8_t *scans, uint64_t scans_bytes, const int64_t *scan_offsets_host, uint8_t *out, uint64_t out_bytes,
                                   const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes);
AEJ_API uint64_t aej_jpegdec_workspace_bytes_box(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host,
                                                 const int *components_host, const int32_t *boxes_host);
AEJ_API int aej_jpegdec_batch_box(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const int *components_host,
                                  const int32_t *boxes_host, const uint8_t *scans, uint64_t scans_bytes, const int64_t *scan_offsets_host,
                                  uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host, int32_t *status, void *workspace,
                                  uint64_t workspace_bytes);
AEJ_API int aej_jpegdec_box_window_host(const aej_jpegdec_desc *desc_host, const int32_t *box4_host, int32_t *window4_out_host);
AEJ_API int aej_jpegdec_box_stats(aej_ctx *ctx, int64_t *out3_host);
AEJ_API uint64_t aej_jpegdec_workspace_bytes_sbox(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host,
                                                  const int *components_host, const int32_t *boxes_host);
AEJ_API int aej_jpegdec_batch_sbox(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const int *components_host,
                                   const int32_t *boxes_host, const uint8_t *scans, uint64_t scans_bytes, const int64_t *scan_offsets_host,
                                   uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host, int32_t *status, void *workspace,
                                   uint64_t workspace_bytes);
AEJ_API int aej_jpegdec_sbox_window_host(const aej_jpegdec_desc *desc_host, int scale, const int32_t *box4_host, int32_t *window4_out_host);

/* ---- progressive JPEG files decoded on the device (standard_jpeg_decode_many(..., progressive=True)) ----------------------------------
 * SOF2 files with Huffman coding, under the frame rules of aej_jpegdec_parse_host (8-bit, 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0 /
 * grey, the JFIF / Adobe colour rules, no DNL), pixel-identical to Pillow for every COMPLETE progression: one whose scans bring every
 * coefficient of every component down to Al = 0 (libjpeg-turbo then reconstructs exactly as for a baseline file, csrc/jpegprog.hip).
 *
 * aej_jpegprog_parse_host: HOST only.  Walks every marker SOI .. EOI of one file.  *frame always gets the frame and n_scans; scans (may
 *   be NULL: a count query) gets the scan descriptors when scan_capacity >= n_scans, otherwise the call returns AEJ_ERR_CAPACITY.  A
 *   scan's Huffman tables are those in force at its SOS (dc[i] for the scan's component i of a first DC scan, ac for an AC scan; the
 *   others are zero); data_offset / data_length are its entropy-coded bytes in the file, up to the first FF xx with xx not 00 / D0..D7;
 *   units_x x units_y is what it walks (the MCU grid when interleaved, the component's own block grid otherwise); level is its
 *   dependency level: one more than the highest level among earlier scans that touch the same (component, coefficient) cells.
 *   AEJ_ERR_ARG for a malformed file or a scan script that violates T.81 G.1.1.1 (Ss > Se, Se > 63, a DC scan with Se != 0, an AC
 *   scan of several components or before the component's DC, Al > 13, Ah not the previous Al, Al != Ah - 1, a repeated first scan, an
 *   undefined Huffman table, a scan that runs past the file, no EOI) -- libjpeg only warns on some of these; this library refuses.
 *   AEJ_ERR_UNSUPPORTED for a valid file outside the set: an INCOMPLETE progression (libjpeg-turbo would smooth between blocks),
 *   arithmetic coding (SOF10), an interleaved scan that does not list every component, a file that is not SOF2, and what the baseline
 *   parser refuses.
 * aej_jpegprog_batch: n files.  frames_host [n]; scans_host: the scan descriptors of file 0, then file 1, ... (frames_host[i].n_scans
 *   each); data: device bytes, the entropy-coded bytes of scan j (in that order) at data_offsets_host[j]; out / out_offsets_host /
 *   status as aej_jpegdec_batch (status values AEJ_JPEGDEC_*).  Every scan is un-stuffed and cut into restart segments at once; then
 *   one launch per dependency level decodes every restart segment of every scan of that level, one thread per segment (DC refinement:
 *   one thread per MCU), into the file's coefficients; the baseline path's IDCT and colour kernels finish.  A bad scan marks its file
 *   and never reads or writes outside its own bytes and its file's coefficients.  Workspace: aej_jpegprog_workspace_bytes.
 * aej_jpegprog_batch_scaled / aej_jpegprog_workspace_bytes_scaled: with scales_host [n], as aej_jpegdec_batch_scaled.
 * aej_jpegprog_batch_mode / aej_jpegprog_workspace_bytes_mode: with scales_host [n] and components_host [n] (either may be NULL), as
 *   aej_jpegdec_batch_mode: the progressive decoder finishes with the baseline path's reconstruction, the luma kernel included.
 *   (Additions to ABI 3: no existing signature, struct or behaviour changed.)
 * aej_jpegprog_batch_box / aej_jpegprog_workspace_bytes_box: with boxes_host [n][4] as well, as aej_jpegdec_batch_box (the same
 *   refusals): a boxed file finishes in the baseline path's boxed reconstruction kernel and has no sample planes.  Its entropy decode
 *   and its coefficients stay whole: every scan is decoded, so every scan's errors are reported.
 *   (Additions to ABI 3: no existing signature, struct or behaviour changed.) */
typedef struct aej_jpegprog_frame {
    int32_t width, height;
    int32_t ncomp;             /* 1 or 3 */
    int32_t hs, vs;            /* luma sampling factors (1x1 for grey) */
    int32_t mcux, mcuy, blocks_per_mcu;
    int32_t sof;               /* 0xC2 */
    int32_t precision16;       /* 1 when a quantisation table in force is 16-bit */
    int32_t n_scans, n_levels;
    uint8_t comp_id[4], comp_h[4], comp_v[4], comp_tq[4];
    uint16_t qt[3][64];        /* quantisation table of each component (in force at its first scan), natural order */
} aej_jpegprog_frame;
typedef struct aej_jpegprog_scan {
    int32_t ncomp;             /* components in the scan */
    int32_t comp[4];           /* their indices in the frame */
    int32_t td[4], ta[4];      /* the DC / AC table selectors of the SOS */
    int32_t ss, se, ah, al;
    int32_t restart_interval;  /* in force at the SOS; counts units */
    int32_t units_x, units_y;
    int32_t n_segments;
    int32_t level;
    aej_jpegdec_huff dc[3], ac;
    int64_t data_offset, data_length;
} aej_jpegprog_scan;
AEJ_API int aej_jpegprog_parse_host(const uint8_t *data_host, uint64_t nbytes, aej_jpegprog_frame *frame_host, aej_jpegprog_scan *scans_host,
                                    int scan_capacity, char *msg, int msg_capacity);
AEJ_API uint64_t aej_jpegprog_workspace_bytes(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n);
AEJ_API int aej_jpegprog_batch(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                               const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host, uint8_t *out, uint64_t out_bytes,
                               const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes);
AEJ_API uint64_t aej_jpegprog_workspace_bytes_scaled(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                     const int *scales_host);
AEJ_API int aej_jpegprog_batch_scaled(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                      const int *scales_host, const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host,
                                      uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host, int32_t *status, void *workspace,
                                      uint64_t workspace_bytes);
AEJ_API uint64_t aej_jpegprog_workspace_bytes_mode(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                   const int *scales_host, const int *components_host);
AEJ_API int aej_jpegprog_batch_mode(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                    const int *scales_host, const int *components_host, const uint8_t *data, uint64_t data_bytes,
                                    const int64_t *data_offsets_host, uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host,
                                    int32_t *status, void *workspace, uint64_t workspace_bytes);
AEJ_API uint64_t aej_jpegprog_workspace_bytes_box(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                  const int *scales_host, const int *components_host, const int32_t *boxes_host);
AEJ_API int aej_jpegprog_batch_box(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                   const int *scales_host, const int *components_host, const int32_t *boxes_host, const uint8_t *data,
                                   uint64_t data_bytes, const int64_t *data_offsets_host, uint8_t *out, uint64_t out_bytes,
                                   const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes);
AEJ_API int aej_jpegprog_box_window_host(const aej_jpegprog_frame *frame_host, const int32_t *box4_host, int32_t *window4_out_host);
/* aej_jpegprog_batch_sbox / aej_jpegprog_workspace_bytes_sbox, aej_jpegprog_sbox_window_host: the _box entries with the boxes in pixels
 * of each file's SCALED image, as aej_jpegdec_batch_sbox (the same refusals; scale 1: the _box call byte for byte).  The entropy decode
 * stays whole.  (Additions to ABI 3: no existing signature, struct or behaviour changed.) */
AEJ_API uint64_t aej_jpegprog_workspace_bytes_sbox(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                   const int *scales_host, const int *components_host, const int32_t *boxes_host);
AEJ_API int aej_jpegprog_batch_sbox(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                    const int *scales_host, const int *components_host, const int32_t *boxes_host, const uint8_t *data,
                                    uint64_t data_bytes, const int64_t *data_offsets_host, uint8_t *out, uint64_t out_bytes,
                                    const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes);
AEJ_API int aej_jpegprog_sbox_window_host(const aej_jpegprog_frame *frame_host, int scale, const int32_t *box4_host, int32_t *window4_out_host);

/* ---- CMYK, YCCK and RGB-coded files (standard_jpeg_decode_many(..., adobe=True)) -------------------------------------------------------
 * The files libjpeg reads with another colour model than YCbCr or grey: four components -- CMYK without an Adobe APP14 marker or with
 * transform 0, YCCK with transform 2 (any other transform: AEJ_ERR_UNSUPPORTED; libjpeg takes it as YCCK with a warning) -- and three
 * components coded as RGB (no JFIF marker, and APP14 transform 0 or the component ids 'R','G','B').  The parsers above refuse them; the
 * _adobe parsers take them and fill one aej_jpeg_adobe per file beside the descriptor, which keeps its three tables: the fourth
 * component's sampling factors and tables travel in the aej_jpeg_adobe.  A file of the kinds the parsers above take gets colour =
 * AEJ_JPEG_YCBCR and zeros.  Sampling: components 1 and 2 are 1 x 1, component 0 as for three components (hs, vs), component 3 either
 * component 0's factors (blocks_per_mcu = 2 hs vs + 2: 10 for 2 x 2) or 1 x 1 (blocks_per_mcu = hs vs + 3); a sub-sampled component 3
 * is up-sampled as the chroma planes are.  desc->ncomp is 4 for a four-component file, which the entries without _adobe refuse.
 *
 * aej_jpegdec_parse_host_adobe / aej_jpegprog_parse_host_adobe: the _440 parsers with adobe_host (one struct, not NULL) as well.
 * aej_jpegdec_batch_adobe / aej_jpegdec_workspace_bytes_adobe, aej_jpegprog_batch_adobe / aej_jpegprog_workspace_bytes_adobe: the _box
 *   calls with adobe_host [n] as well.  NULL, or every colour AEJ_JPEG_YCBCR: the _box call byte for byte, launches included.  For a file
 *   with another colour, components_host[i] (NULL: 3) is 3 -- image i is [height][width][3]: the samples of an RGB-coded file; of a
 *   four-component one Pillow's CMYK -> RGB of the image below, clip8(nk - MULDIV255(c, nk)) per channel with nk = 255 - K -- or 4
 *   (four-component files only): [height][width][4], Pillow's mode "CMYK" image: 255 - sample for CMYK; for YCCK libjpeg's YCbCr -> RGB
 *   of samples 0..2 and 255 - sample 3.  Refused with AEJ_ERR_UNSUPPORTED naming the file, before any device work and leaving out
 *   untouched: such a file with components 1, with a scale other than 1 or with a box that is not its whole image ("... of a
 *   four-component / RGB-coded file is not built").  components 4 on any other file is AEJ_ERR_ARG.  A call with such a file runs the
 *   four-component instantiations of the entropy kernels (a fourth DC predictor, a 4-bit block slot) and reconstructs these files
 *   with kernels of their own; every other file of the call is reconstructed as before.  A file whose components all decode under one
 *   DC and one AC table (what libjpeg writes for CMYK and RGB) says nothing about the block slot in its bits; the slot is then taken
 *   from the block counts, at the price of one more counting pass.
 *   (Additions to ABI 3: no existing signature, struct or behaviour changed.) */
enum { AEJ_JPEG_YCBCR = 0, AEJ_JPEG_RGB = 1, AEJ_JPEG_CMYK = 2, AEJ_JPEG_YCCK = 3 };
typedef struct aej_jpeg_adobe {
    int32_t colour;            /* AEJ_JPEG_*: YCbCr (or grey), RGB, CMYK, YCCK */
    int32_t h3, v3;            /* sampling factors of component 3; 0 unless the file has four components */
    int32_t tq3;               /* its quantisation table index in the frame header */
    uint16_t qt3[64];          /* its quantisation table, natural order */
    aej_jpegdec_huff dc3, ac3; /* its Huffman tables: a baseline file's scan; of a progressive file dc3 alone, from the interleaved DC scan */
} aej_jpeg_adobe;
AEJ_API int aej_jpegdec_parse_host_adobe(const uint8_t *data_host, uint64_t nbytes, aej_jpegdec_desc *desc_host, aej_jpeg_adobe *adobe_host,
                                         char *msg, int msg_capacity, int layout_440);
AEJ_API int aej_jpegprog_parse_host_adobe(const uint8_t *data_host, uint64_t nbytes, aej_jpegprog_frame *frame_host, aej_jpegprog_scan *scans_host,
                                          int scan_capacity, aej_jpeg_adobe *adobe_host, char *msg, int msg_capacity, int layout_440);
AEJ_API uint64_t aej_jpegdec_workspace_bytes_adobe(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host,
                                                   const int *components_host, const int32_t *boxes_host, const aej_jpeg_adobe *adobe_host);
AEJ_API int aej_jpegdec_batch_adobe(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n, const int *scales_host, const int *components_host,
                                    const int32_t *boxes_host, const aej_jpeg_adobe *adobe_host, const uint8_t *scans, uint64_t scans_bytes,
                                    const int64_t *scan_offsets_host, uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host,
                                    int32_t *status, void *workspace, uint64_t workspace_bytes);
AEJ_API uint64_t aej_jpegprog_workspace_bytes_adobe(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                                    const int *scales_host, const int *components_host, const int32_t *boxes_host,
                                                    const aej_jpeg_adobe *adobe_host);
AEJ_API int aej_jpegprog_batch_adobe(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                     const int *scales_host, const int *components_host, const int32_t *boxes_host,
                                     const aej_jpeg_adobe *adobe_host, const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host,
                                     uint8_t *out, uint64_t out_bytes, const int64_t *out_offsets_host, int32_t *status, void *workspace,
                                     uint64_t workspace_bytes);

/* ---- images of mixed sizes and qualities encoded in one call (standard_jpeg_encode_many) -------------------------------------------------
 * The files of aej_jfif_encode_batch_opt / _prog -- Pillow's Image.save(buf, "JPEG", quality, subsampling, optimize, progressive), byte
 * for byte -- for n images that each have their own size and quality.  One kernel covers every 8 x 8 block of every image (colour, edge
 * replication, h2v1 / h2v2 down-sampling, islow FDCT and the quantisation fused: an image has one quality); the images are then grouped
 * by (height, width), each group runs one entropy-encode chain as in aej_jfif_transcode_batch, image i of it under the quantisers and
 * markers of its own quality: optimize = 1 the file's own Huffman tables, optimize = 0 the Annex K tables, progressive = 1 (optimize is
 * then not looked at beyond its range) libjpeg's ten scans.  Launches grow with the number of distinct sizes, one chain each.
 *
 * aej_jfif_many_desc: image i is packed uint8 [height][width][3] at src + src_offset.  components (the field that was `reserved`, which
 *   had to be 0): 0 or 3 such an image; 1 a grey image, packed uint8 [height][width], written as the one-component file Pillow saves
 *   for a mode "L" image (one DQT, a one-component SOF, the luma Huffman tables alone, a non-interleaved scan -- six scans with
 *   progressive = 1 -- over the ceil(width / 8) x ceil(height / 8) blocks in raster order; subsampling does not bear on it).  Both
 *   kinds mix in one call; the groups are then by (height, width, components).  Any other value: AEJ_ERR_ARG naming the image.
 * aej_jfif_many_workspace_bytes: the workspace of such a call, 0 for descriptors the call refuses (ctx is not looked at).
 * aej_jfif_many_encode: src: device bytes, src_bytes of them.  out / out_capacity / offsets / lengths / total_host as
 *   aej_jfif_transcode_batch: offsets and lengths are device int64 [n] in the caller's order (the files are packed group after group),
 *   out may be NULL to size only; when the files do not fit, AEJ_ERR_CAPACITY returns with *total_host exact, a file that would end past
 *   out_capacity is not written and nothing is written past it (call again with that size).
 *   Every descriptor is checked before any device work: AEJ_ERR_ARG, the message naming the image, for a width or height outside
 *   1..65535, a quality outside 1..100 or an image that does not lie inside src_bytes.  An encode cannot fail per image: there are no
 *   status words.  *n_groups_host (may be NULL) gets the number of chains.  The call waits for the total at its end.
 * aej_jfif_many_coefs_host: HOST only, the code the kernel runs, on one image.  rgb_host: uint8 [height][width][3]; dst_host: int16
 *   [>= the result][64], zigzag order inside a block, the blocks in MCU order (MCUs in raster order; in each the hs x vs luma blocks in
 *   raster order, then Cb, Cr), the dummy luma blocks of edge MCUs as libjpeg writes them (AC zero, DC of the block before in the MCU).
 *   -> the image's blocks (also with both pointers NULL: a size query), AEJ_ERR_ARG for a size, quality or subsampling outside the
 *   encoder's or one pointer NULL, AEJ_ERR_CAPACITY for dst_blocks too small.
 * aej_jfif_headers_grey_host: HOST only, the markers SOI .. SOS of the grey file of one (quality, H, W) with the Annex K luma tables
 *   (optimize = 0), as aej_jfif_headers_host: one DQT, SOF0 with one component (id 1, 1 x 1, table 0), two DHT, SOS with Ns = 1.
 * aej_jfif_many_coefs_grey_host: the same for one grey image.  grey_host: uint8 [height][width]; the blocks are the component's
 *   ceil(width / 8) x ceil(height / 8) in raster order, none a dummy, under the luma quantiser of the quality.
 * (Additions to ABI 3: no existing signature, struct layout or behaviour of a valid call changed.) */
typedef struct aej_jfif_many_desc {
    int64_t src_offset;
    int32_t width, height, quality, components;
} aej_jfif_many_desc;
AEJ_API uint64_t aej_jfif_many_workspace_bytes(aej_ctx *ctx, const aej_jfif_many_desc *descs_host, int n, int subsampling, int optimize,
                                               int progressive);
AEJ_API int aej_jfif_many_encode(aej_ctx *ctx, const aej_jfif_many_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, int subsampling,
                                 int optimize, int progressive, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths,
                                 uint64_t *total_host, int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes);
AEJ_API int64_t aej_jfif_many_coefs_host(int width, int height, int quality, int subsampling, const uint8_t *rgb_host, int16_t *dst_host,
                                         int64_t dst_blocks);
AEJ_API int aej_jfif_headers_grey_host(int quality, int H, int W, uint8_t *out_host, int capacity);
AEJ_API int64_t aej_jfif_many_coefs_grey_host(int width, int height, int quality, const uint8_t *grey_host, int16_t *dst_host, int64_t dst_blocks);

/* ---- lossless transcode: existing files entropy-coded again (standard_jpeg_transcode_many) ----------------------------------------------
 * What jpegtran -optimize / -progressive do, on the device: the files are Huffman-decoded to their quantised coefficients by the stages of
 * aej_jpegdec_batch / aej_jpegprog_batch (no IDCT, no colour) and those coefficients -- every one, the dummy edge blocks of the MCU grid
 * included -- are coded again by the entropy stages of aej_jfif_encode_batch_opt with optimize (progressive = 0: a baseline SOF0 file
 * under its own optimal Huffman tables) or of aej_jfif_encode_batch_prog (progressive = 1: SOF2, libjpeg's ten scans).  One call takes
 * baseline sources (descs_host, n_base, scans ... as aej_jpegdec_batch) and progressive ones (frames_host, pscans_host, n_prog, data ...
 * as aej_jpegprog_batch) together; either count may be 0, not both.  File i of the call is baseline source i for i < n_base, otherwise
 * progressive source i - n_base.  Three-component files, and one-component (grey) files, which used to be refused
 * (AEJ_ERR_UNSUPPORTED for a file with a 16-bit quantisation table); restart markers of a source are never carried over: the output has
 * those the _rst entries below ask for (jpegtran -restart N / NB), and none through the entries without that suffix.
 * A one-component source is sampled 1 x 1 whatever its frame header says (the parsers' rule: hs = vs = 1, blocks_per_mcu = 1); its
 * output has one DQT -- its component's table, written as table 0 --, a one-component SOF with sampling 1 x 1, the two luma DHT and a
 * non-interleaved scan (progressive = 1: libjpeg's six scans for one component).
 *
 * Output file: SOI; JFIF 1.01 APP0 with the density density_host[3 i .. 3 i + 2] = units, Xdensity, Ydensity (density_host NULL: 0, 1, 1);
 * one 8-bit DQT per distinct table id the components reference, in order of first reference; SOF0 / SOF2 with the source's component
 * ids, sampling factors and table selectors; then DHT / SOS as the encoders write them (luma tables in slots 0, chroma in slots 1).
 * aej_jfif_transcode_headers_host: HOST only, the bytes SOI .. end of SOF of one source (exactly one of desc_host / frame_host given;
 *   density3_host may be NULL) -> their length, AEJ_ERR_CAPACITY, AEJ_ERR_UNSUPPORTED or AEJ_ERR_ARG.
 * aej_jfif_transcode_batch: out / out_capacity / offsets / lengths / total_host as aej_jfif_encode_batch_opt, offsets and lengths being
 *   device int64 [n_base + n_prog] in the call's file order (the files are packed group after group, not in that order).  status:
 *   device int32 [n_base + n_prog], AEJ_JPEGDEC_*: a source whose scan is malformed, or that decodes to a coefficient an 8-bit file
 *   cannot hold (AEJ_JPEGDEC_COEF_RANGE: the coders' per-block bounds rest on that range, so such a block never reaches them), gets
 *   its reason there and length 0; the other files are written.  Files are grouped by (height, width, sampling, components): each group runs one
 *   entropy-encode chain (*n_groups_host, may be NULL, gets their number).  The call waits for the decode's sync rounds and, at its
 *   end, for the total.  Workspace: aej_jfif_transcode_workspace_bytes with the same descriptors (0 for descriptors the call refuses). */
AEJ_API int aej_jfif_transcode_headers_host(const aej_jpegdec_desc *desc_host, const aej_jpegprog_frame *frame_host, const uint16_t *density3_host,
                                            int progressive, uint8_t *out_host, int capacity);
AEJ_API uint64_t aej_jfif_transcode_workspace_bytes(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                    const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                    int progressive);
AEJ_API int aej_jfif_transcode_batch(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                     const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                     const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                     const int64_t *data_offsets_host, const uint16_t *density_host, int progressive, uint8_t *out,
                                     uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host, int32_t *status,
                                     int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes);

/* ---- lossless flip, rotation and transposition (standard_jpeg_transform_many) -------------------------------------------------------
 * What jpegtran -flip / -rotate / -transpose / -transverse do with -perfect or -trim, on the device: the transcode above with one
 * transform per file, applied to the quantised coefficients between the decoders' and the coders' entropy stages by the one kernel that
 * takes the bridge's place (csrc/jfiftrans.hip, k_jt_transform; the mapping is csrc/jfif_transform_core.h).  The codes are jpegtran's
 * JXFORM order; with W, H the source size and rotations clockwise:
 *   0 none  1 flip_h  out[y][x] = in[y][W-1-x]   2 flip_v  in[H-1-y][x]   3 transpose  in[x][y]   4 transverse  in[H-1-x][W-1-y]
 *   5 rot90   6 rot180   7 rot270   (rot90 = transpose then flip_h, rot270 = flip_h then transpose, transverse = transpose then rot180)
 * On a block's coefficients c(v, u): flip_h multiplies by (-1)^u and reverses every component's block columns, flip_v by (-1)^v and
 * reverses the block rows, transpose reads c(u, v) of block (bx, by), swaps width and height and the luma sampling factors and writes
 * every quantisation table transposed.  A mirrored axis must be a whole number of the source's MCUs (flip_h and rot270: the width;
 * flip_v and rot90: the height; rot180 and transverse: both): with trim = 0 a file that is not is refused, with trim = 1 the partial
 * MCU column / row at its right / bottom edge is dropped first.  The dummy blocks of the output's edge MCUs are written as libjpeg
 * writes them (AC zero, DC of the block before in the MCU); a file with the code 0 is transcoded exactly as above, its dummy blocks
 * carried.  A transposing code on a 4:2:2 source would give a 4:4:0 file: AEJ_ERR_UNSUPPORTED.  Files are grouped by the (height,
 * width, sampling, components) of their OUTPUT.  A one-component source has 8 x 8 MCUs and no dummy blocks, so every code is allowed.
 *
 * aej_jfif_transform_geometry_host: HOST only.  out4_host (may be NULL) gets the output's height, width, hs, vs.  -> 0, AEJ_ERR_ARG,
 *   AEJ_ERR_UNSUPPORTED (4:4:0), AEJ_JFIF_TRANSFORM_NOT_PERFECT (trim = 0 and a mirrored axis with a partial MCU) or
 *   AEJ_JFIF_TRANSFORM_TRIMS_TO_ZERO (trim = 1 and nothing left of it).
 * aej_jfif_transform_coefs_host: HOST only, the code the kernel runs, on one file's coefficients.  src_host: int16 [src_blocks][64], natural
 *   order inside a block, the blocks in the SOURCE's MCU order (MCUs in raster order; in each the hs x vs luma blocks in raster order,
 *   then Cb, Cr), src_blocks = (hs vs + 2) x its MCUs.  dst_host: int16 [>= the result][64], zigzag order inside a block, the OUTPUT's MCU
 *   order.  -> the output's blocks (also with both pointers NULL: a size query), or the geometry entry's refusals, AEJ_ERR_ARG for a
 *   wrong src_blocks, AEJ_ERR_CAPACITY for dst_blocks too small.  No range check.
 * aej_jfif_transform_coefs_grey_host: the same for a one-component file: the blocks of both sides are the component's in raster order,
 *   src_blocks = ceil(W / 8) x ceil(H / 8).  Such a file can have one block or two, so a geometry that is not perfect or trims to
 *   zero is AEJ_ERR_ARG here (aej_jfif_transform_geometry_host with hs = vs = 1 tells which).
 * aej_jfif_transform_headers_host, _workspace_bytes, _batch: the aej_jfif_transcode_* entries with, before their output arguments,
 *   transforms_host [n_base + n_prog] int32 in the call's file order (headers: the one code) and trim (0 or 1).  The headers carry the
 *   output's size and sampling and the transposed tables; a refused geometry is AEJ_ERR_ARG (the message names the file), 4:4:0
 *   AEJ_ERR_UNSUPPORTED, and the workspace size of a refused call is 0. */
enum { AEJ_JFIF_TRANSFORM_NOT_PERFECT = 1, AEJ_JFIF_TRANSFORM_TRIMS_TO_ZERO = 2 };
AEJ_API int aej_jfif_transform_geometry_host(int H, int W, int hs, int vs, int transform, int trim, int32_t *out4_host);
AEJ_API int64_t aej_jfif_transform_coefs_host(int H, int W, int hs, int vs, int transform, int trim, const int16_t *src_host, int64_t src_blocks,
                                              int16_t *dst_host, int64_t dst_blocks);
AEJ_API int64_t aej_jfif_transform_coefs_grey_host(int H, int W, int transform, int trim, const int16_t *src_host, int64_t src_blocks,
                                                   int16_t *dst_host, int64_t dst_blocks);
AEJ_API int aej_jfif_transform_headers_host(const aej_jpegdec_desc *desc_host, const aej_jpegprog_frame *frame_host, const uint16_t *density3_host,
                                            int progressive, int transform, int trim, uint8_t *out_host, int capacity);
AEJ_API uint64_t aej_jfif_transform_workspace_bytes(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                    const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                    int progressive, const int32_t *transforms_host, int trim);
AEJ_API int aej_jfif_transform_batch(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                     const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                     const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                     const int64_t *data_offsets_host, const uint16_t *density_host, int progressive,
                                     const int32_t *transforms_host, int trim, uint8_t *out, uint64_t out_capacity, int64_t *offsets,
                                     int64_t *lengths, uint64_t *total_host, int32_t *status, int32_t *n_groups_host, void *workspace,
                                     uint64_t workspace_bytes);

/* ---- restart markers in the files the three writers above produce ---------------------------------------------------------------------
 * The _rst entries are their namesakes with two more arguments, Pillow's restart_marker_blocks and restart_marker_rows (libjpeg's
 * restart_interval and restart_in_rows, jpegtran's -restart NB and -restart N), each 0 .. 65535 (AEJ_ERR_ARG otherwise, a workspace size
 * of 0); the entries without the suffix are these with 0, 0.  A scan's interval R counts MCUs of that scan: restart_rows > 0 gives
 * min(restart_rows x the scan's MCUs per row, 65535), per scan, and overrides restart_blocks, which gives R = restart_blocks for every
 * scan.  An interleaved scan has ceil(W / (8 hs)) MCUs per row; a non-interleaved one (a grey file, a progressive AC scan) the
 * component's blocks per row.  `FF DD 00 04 Rhi Rlo` is written directly before a scan's SOS, after its DHT segments, when R differs from
 * the last R written in the file (0 at its start).  Before MCU k R of a scan (k >= 1) the coder flushes what is pending (a progressive
 * scan's end-of-band run with its correction bits), pads the byte with 1-bits (stuffed like any byte), writes FF D0 + ((k - 1) & 7) and
 * sets every DC predictor to 0; optimised tables are built from statistics gathered under the same resets.  R >= the scan's MCUs: the
 * DRI alone.  One setting holds for every file of a call.  The files are Pillow's / libjpeg-turbo's byte for byte.
 * On the device every interval is byte-aligned in the unstuffed stream (a second prefix sum over the intervals' byte lengths) and the
 * markers are inserted by the kernel that stuffs 0xFF bytes (csrc/jfif_restart_core.h holds the index rules, host + device).
 * The same-size encoders (aej_jfif_encode_batch*) write no restart markers: their Annex K bit count is fused into quantisation.
 * aej_jfif_headers_rst_host: HOST only, aej_jfif_headers_host_opt / _grey_host (components 1; 0 or 3: colour) with the DRI of the
 *   options before the SOS.
 * aej_jfif_restart_map_host: HOST only, the index rules on one image.  scan_r_host / scan_dri_host: int32 [10], every scan's R and
 *   whether a DRI precedes it (progressive = 0: the one scan; 1: libjpeg's ten, or six for one component).  For the first scan -- the
 *   baseline file's scan, interleaved MCU order -- interval_host (int32) and reset_host (uint8) [>= blocks] (either may be NULL) get every
 *   block's interval and whether its DC predictor is 0, marker_host [>= intervals] (may be NULL) the second byte of the marker before
 *   each interval (0 for the first); counts2_host (may be NULL) the blocks and the intervals.  -> the scans, AEJ_ERR_ARG, AEJ_ERR_CAPACITY.
 * (Additions to ABI 3: no existing signature, struct layout or behaviour of a valid call changed.) */
AEJ_API uint64_t aej_jfif_many_workspace_bytes_rst(aej_ctx *ctx, const aej_jfif_many_desc *descs_host, int n, int subsampling, int optimize,
                                                   int progressive, int restart_blocks, int restart_rows);
AEJ_API int aej_jfif_many_encode_rst(aej_ctx *ctx, const aej_jfif_many_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes,
                                     int subsampling, int optimize, int progressive, int restart_blocks, int restart_rows, uint8_t *out,
                                     uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host, int32_t *n_groups_host,
                                     void *workspace, uint64_t workspace_bytes);
AEJ_API uint64_t aej_jfif_transcode_workspace_bytes_rst(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                        const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                        int progressive, int restart_blocks, int restart_rows);
AEJ_API int aej_jfif_transcode_batch_rst(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                         const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                         const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                         const int64_t *data_offsets_host, const uint16_t *density_host, int progressive, int restart_blocks,
                                         int restart_rows, uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths,
                                         uint64_t *total_host, int32_t *status, int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes);
AEJ_API uint64_t aej_jfif_transform_workspace_bytes_rst(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                        const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                        int progressive, const int32_t *transforms_host, int trim, int restart_blocks,
                                                        int restart_rows);
AEJ_API int aej_jfif_transform_batch_rst(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                         const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                         const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                         const int64_t *data_offsets_host, const uint16_t *density_host, int progressive,
                                         const int32_t *transforms_host, int trim, int restart_blocks, int restart_rows, uint8_t *out,
                                         uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host, int32_t *status,
                                         int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes);
AEJ_API int aej_jfif_headers_rst_host(int quality, int H, int W, int subsampling, int components, int restart_blocks, int restart_rows,
                                      uint8_t *out_host, int capacity);
AEJ_API int aej_jfif_restart_map_host(int H, int W, int subsampling, int components, int restart_blocks, int restart_rows, int progressive,
                                      int32_t *scan_r_host, int32_t *scan_dri_host, int32_t *interval_host, uint8_t *reset_host,
                                      int64_t block_capacity, uint8_t *marker_host, int64_t marker_capacity, int64_t *counts2_host);

/* ---- the 4:4:0 layout: luma sampled 1 x 2 over 1 x 1 chroma ----------------------------------------------------------------------------
 * What `jpegtran -rotate 90` makes of a 4:2:2 file.  Opt-in: the _440 entries are their namesakes with one more argument, layout_440 (0 or
 * 1; AEJ_ERR_ARG otherwise, a workspace size of 0), and with 0 they answer exactly as their namesakes, which keep refusing the layout
 * (AEJ_ERR_UNSUPPORTED; aej_jfif_transform_geometry_host / _coefs_host given hs = 1, vs = 2: AEJ_ERR_ARG, as before).  With 1:
 *   aej_jpegdec_parse_host_440, aej_jpegprog_parse_host_440 also accept a three-component frame whose luma factors are 1 x 2 over 1 x 1
 *     chroma (hs = 1, vs = 2, blocks_per_mcu 4: two luma blocks stacked, then Cb, Cr; the lower one is a dummy in the last MCU row of
 *     an image with an odd number of block rows).  The decoders (aej_jpegdec_batch*, aej_jpegprog_batch*) take such descriptors as they
 *     are: chroma is up-sampled by libjpeg-turbo's h1v2 "fancy" rule -- the upper output row of chroma row j is (3 c[j] + c[j-1] + 1) >> 2,
 *     the lower (3 c[j] + c[j+1] + 2) >> 2, rows -1 and hc replicate the edge rows, at any width -- and at scale 2 and 4 still so (the
 *     chroma IDCT of this layout stays at the luma block's size), at scale 8 by replication.  Pixel-identical to Pillow's decode and draft().
 *   aej_jfif_transform_geometry_host_440, _coefs_host_440, _headers_host_440: hs = 1, vs = 2 is a source layout, a transposing code
 *     on a 4:2:2 source gives 4:4:0 (sampling byte 0x12) and on a 4:4:0 source 4:2:2; MCUs are 8 hs x 8 vs as for every layout.
 *   aej_jfif_transform_workspace_bytes_440, aej_jfif_transform_batch_440: the _rst entries with layout_440 after restart_rows;
 *     transforms_host may be NULL here, which is the transcode (code 0 for every file), so the transcoder needs no entry of its own.
 * (Additions to ABI 3: no existing signature, struct layout or behaviour of a valid call changed.) */
AEJ_API int aej_jpegdec_parse_host_440(const uint8_t *data_host, uint64_t nbytes, aej_jpegdec_desc *desc_host, char *msg, int msg_capacity,
                                       int layout_440);
AEJ_API int aej_jpegprog_parse_host_440(const uint8_t *data_host, uint64_t nbytes, aej_jpegprog_frame *frame_host, aej_jpegprog_scan *scans_host,
                                        int scan_capacity, char *msg, int msg_capacity, int layout_440);
AEJ_API int aej_jfif_transform_geometry_host_440(int H, int W, int hs, int vs, int transform, int trim, int layout_440, int32_t *out4_host);
AEJ_API int64_t aej_jfif_transform_coefs_host_440(int H, int W, int hs, int vs, int transform, int trim, int layout_440, const int16_t *src_host,
                                                  int64_t src_blocks, int16_t *dst_host, int64_t dst_blocks);
AEJ_API int aej_jfif_transform_headers_host_440(const aej_jpegdec_desc *desc_host, const aej_jpegprog_frame *frame_host, const uint16_t *density3_host,
                                                int progressive, int transform, int trim, int layout_440, uint8_t *out_host, int capacity);
AEJ_API uint64_t aej_jfif_transform_workspace_bytes_440(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                        const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                        int progressive, const int32_t *transforms_host, int trim, int restart_blocks,
                                                        int restart_rows, int layout_440);
AEJ_API int aej_jfif_transform_batch_440(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                         const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                         const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                         const int64_t *data_offsets_host, const uint16_t *density_host, int progressive,
                                         const int32_t *transforms_host, int trim, int restart_blocks, int restart_rows, int layout_440,
                                         uint8_t *out, uint64_t out_capacity, int64_t *offsets, int64_t *lengths, uint64_t *total_host,
                                         int32_t *status, int32_t *n_groups_host, void *workspace, uint64_t workspace_bytes);

/* ---- lossless crop and chroma drop in the transform (standard_jpeg_transform_many crop=, drop_chroma=) --------------------------------
 * What `jpegtran -crop WxH+X+Y` and `jpegtran -grayscale` do, on the device, with or without a transform in the same call.  The _cut
 * entries are the _440 entries with two more arguments after layout_440, and with boxes NULL and drop_chroma 0 they answer exactly as
 * those (the kernel of these entries, k_jt_cut, is launched only by a call in which a file has a crop or drops its chroma).
 *   boxes4_host (headers, geometry, coefs: box4_host, the one box): NULL, or int32 [n_base + n_prog][4] in the call's file order: left,
 *     upper, right, lower in Pillow's Image.crop convention, in the coordinates of the image AFTER the transform and its trim (H', W'
 *     below; the upright image of an EXIF auto-orient), where jpegtran applies -crop.  right == 0: no crop for that file.  Required:
 *     0 <= left < right <= W' and 0 <= upper < lower <= H'; nothing is clamped, and a box reaching into a strip the trim dropped is
 *     refused (AEJ_ERR_ARG, the message names the file; geometry: AEJ_JFIF_TRANSFORM_CROP_RANGE).  The corner moves up and left to the
 *     OUTPUT's MCU grid as jpegtran moves it: with mw = 8 hs', mh = 8 vs' (8, 8 for a one-component output) L = left - left % mw,
 *     U = upper - upper % mh, and the file written is right - L wide, lower - U high and holds [U, lower) x [L, right) of the transformed
 *     image: every block is the transformed image's block, none is quantised again.  Where the new right / bottom edge cuts an MCU the
 *     dummy blocks are written as libjpeg writes them.  trim / -perfect are decided on the whole source first, as without a crop.  The
 *     box of the whole image (0, 0, W', H') is no crop: the bytes are those of the call without it.  Restart intervals count on the
 *     cropped output's MCU grid; files are grouped by their output, so crops of equal size share an entropy chain.
 *   drop_chroma (0 or 1; AEJ_ERR_ARG otherwise, a workspace size of 0), for every file of the call: a three-component source is written
 *     as a one-component file, as the transcoder writes a one-component source: one DQT (the luma table as table 0, transposed by a
 *     transposing code), a one-component frame header (sampling byte 0x11) with the luma component's id, one non-interleaved scan or the
 *     six-scan progression.  Its blocks are the source's REAL luma blocks in raster order, and the MCU of every rule above is 8 x 8: a
 *     mirrored axis has to be a multiple of 8, trim drops the partial 8-pixel strip, the crop aligns to 8, and a transposing code on a
 *     4:2:2 source needs no layout_440.  A one-component source passes through unchanged.
 * aej_jfif_transform_geometry_host_cut, _coefs_host_cut take `components` (3, or 1: the aej_jfif_transform_coefs_grey_host layout of
 *   the source) after vs.  out6_host (may be NULL): the output's height, width, hs, vs, then L and U.  _coefs_host_cut: dst_host is in the
 *   output's order (MCU order; one component: raster order); a file of these can have 1 .. 3 blocks, so a refused geometry is AEJ_ERR_ARG
 *   here (the geometry entry tells which).  EXIF pixel-dimension tags of carried metadata are the caller's: nothing here rewrites them.
 * (Additions to ABI 3: no existing signature, struct layout or behaviour of a valid call changed.) */
enum { AEJ_JFIF_TRANSFORM_CROP_RANGE = 3 };
AEJ_API int aej_jfif_transform_geometry_host_cut(int H, int W, int hs, int vs, int components, int transform, int trim, int layout_440,
                                                 const int32_t *box4_host, int drop_chroma, int32_t *out6_host);
AEJ_API int64_t aej_jfif_transform_coefs_host_cut(int H, int W, int hs, int vs, int components, int transform, int trim, int layout_440,
                                                  const int32_t *box4_host, int drop_chroma, const int16_t *src_host, int64_t src_blocks,
                                                  int16_t *dst_host, int64_t dst_blocks);
AEJ_API int aej_jfif_transform_headers_host_cut(const aej_jpegdec_desc *desc_host, const aej_jpegprog_frame *frame_host, const uint16_t *density3_host,
                                                int progressive, int transform, int trim, int layout_440, const int32_t *box4_host, int drop_chroma,
                                                uint8_t *out_host, int capacity);
AEJ_API uint64_t aej_jfif_transform_workspace_bytes_cut(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base,
                                                        const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *pscans_host, int n_prog,
                                                        int progressive, const int32_t *transforms_host, int trim, int restart_blocks,
                                                        int restart_rows, int layout_440, const int32_t *boxes4_host, int drop_chroma);
AEJ_API int aej_jfif_transform_batch_cut(aej_ctx *ctx, const aej_jpegdec_desc *descs_host, int n_base, const uint8_t *scans, uint64_t scans_bytes,
                                         const int64_t *scan_offsets_host, const aej_jpegprog_frame *frames_host,
                                         const aej_jpegprog_scan *pscans_host, int n_prog, const uint8_t *data, uint64_t data_bytes,
                                         const int64_t *data_offsets_host, const uint16_t *density_host, int progressive,
                                         const int32_t *transforms_host, int trim, int restart_blocks, int restart_rows, int layout_440,
                                         const int32_t *boxes4_host, int drop_chroma, uint8_t *out, uint64_t out_capacity, int64_t *offsets,
                                         int64_t *lengths, uint64_t *total_host, int32_t *status, int32_t *n_groups_host, void *workspace,
                                         uint64_t workspace_bytes);

/* ---- Pillow's resize, reduce and thumbnail for packed 8-bit RGB (_ch entries: and mode-"L") images (resize_many, standard_jpeg_thumbnail_many) ------------------
 * Image.resize with the convolution filters, Image.reduce and the reducing_gap step of resize, bit for bit, for many images of
 * different sizes in one call (csrc/resample.hip).  An image is uint8 [h][w][3], packed.  Per image, in this order:
 *   1. reduce (only when reduce_x > 1 or reduce_y > 1): the region reduce_box = x0, y0, x1, y1 of the source is cut into reduce_x x
 *      reduce_y cells, clipped at its right and bottom edges, and becomes ceil((x1 - x0) / reduce_x) x ceil((y1 - y0) / reduce_y)
 *      pixels, each ((sum + n / 2) * (2^32 / (256 n))) >> 24 in uint32 over the n pixels really in its cell (Image.reduce);
 *   2. the horizontal pass, when dst_w differs from the width at hand or box[0] != 0 or box[2] != dst_w, rounded to uint8;
 *   3. the vertical pass, likewise with box[1], box[3], dst_h.
 *   box = x0, y0, x1, y1 is in the pixels of the image step 1 left (the source itself without a reduce): float32, as Pillow's C code
 *   takes it.  An image that needs no step is copied.  A pass is clip((2^21 + sum(pixel * tap)) >> 22, 0, 255) in int32.
 * NEAREST (filter 0) is not part of this (Pillow takes another path for it): it is an unknown filter, AEJ_ERR_ARG.  Nor is the image
 * more than 100 times as tall as wide that is made shorter (Pillow resizes it vertically first): AEJ_ERR_UNSUPPORTED.
 *
 * aej_resample_taps_host: HOST only, the table of one axis as Pillow precomputes it, in double and without fused multiply-adds:
 *   scale = double(in1 - in0) / out_size (the difference in float32), support = the filter's * max(scale, 1); for output xx:
 *   center = in0 + (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), count = min(int(center + support + 0.5), in_size) -
 *   xmin, k[x] = filter((x + xmin - center + 0.5) / max(scale, 1)) normalised by their sum, tap = int(k 2^22 +- 0.5).  -> ksize =
 *   2 ceil(support) + 1, the row length of taps_host; bounds_host [out_size][2] gets xmin and count, taps_host [out_size][ksize]
 *   the taps, zero past count.  Both NULL: a size query.  AEJ_ERR_ARG for an unknown filter, a size below 1 or in1 <= in0;
 *   AEJ_ERR_CAPACITY when taps_capacity (in int32) is below out_size * ksize.
 * aej_resample_batch: n images.  src / dst: device bytes; image i is read at src + descs_host[i].src_offset and written at dst +
 *   dst_offset, exactly dst_w * dst_h * 3 bytes and no other byte of dst.  Enqueues at most three kernels (reduce, horizontal,
 *   vertical: each one grid over every image that needs it) and one upload of the descriptors and tap tables, then waits for the
 *   upload; nothing is copied back.  Every descriptor is checked before any device work: AEJ_ERR_ARG naming the image for an unknown
 *   filter, a size below 1 or above 65535, a reduce factor below 1, an empty box or one outside the image, an image outside src_bytes
 *   / dst_bytes, a source image that overlaps dst ("source inside the output": no source image may overlap the dst_bytes at dst,
 *   as for aej_filter_batch and the entries after it; the _ch and _win calls alike.  Such a call read pixels it was overwriting; it
 *   is refused since the entries share one span check); AEJ_ERR_UNSUPPORTED naming the image for the tall one.  Workspace: aej_resample_workspace_bytes with the same descriptors (0 for descriptors the call refuses).
 * aej_resample_batch_ch / aej_resample_workspace_bytes_ch: the same calls with channels_host [n], each 3 or 1 (anything else:
 *   AEJ_ERR_ARG naming the image, 0 bytes; NULL: every image 3): image i is uint8 [h][w][channels], packed -- 1 is Pillow's mode "L",
 *   the same reduce and passes on one channel (Pillow's mode-"L" resize equals one channel of its RGB resize of three copies).  The
 *   descriptor is unchanged: its offsets are bytes.  Exactly dst_w * dst_h * channels bytes and no other byte of dst are written.
 *   Images of either count form launches of their own: at most six kernels for a mixed call, and with every count 3 the calls are
 *   aej_resample_batch and aej_resample_workspace_bytes byte for byte, launches included.  (Additions to ABI 3: no existing signature,
 *   struct or behaviour changed.)
 * aej_resample_batch_win / aej_resample_workspace_bytes_win: the _ch calls with windows_host [n][4] = x0, y0, vw, vh as well.  The stored
 *   source of image i -- src_w x src_h at src_offset, packed -- is the rectangle [y0, y0 + src_h) x [x0, x0 + src_w) of a virtual image
 *   vw x vh, and box and reduce_box are in the virtual image's coordinates.  The tap tables are computed from the virtual size, so they
 *   are bit for bit the whole image's, and the result is the _ch call's on the whole image as long as nothing outside the rectangle is
 *   read: that is checked per descriptor on the host before any device work -- a tap with a non-zero count, or the reduce box, that
 *   reaches outside the stored rectangle, or a rectangle outside its virtual image: AEJ_ERR_ARG naming the image, 0 bytes, dst
 *   untouched.  Only the base pointer and the pitch of the first stage move; the kernels are the same.  NULL windows_host: the _ch call
 *   byte for byte.  (Additions to ABI 3: no existing signature, struct or behaviour changed.) */
enum { AEJ_RESAMPLE_LANCZOS = 1, AEJ_RESAMPLE_BILINEAR = 2, AEJ_RESAMPLE_BICUBIC = 3, AEJ_RESAMPLE_BOX = 4, AEJ_RESAMPLE_HAMMING = 5 }; /* Pillow's integers */
typedef struct aej_resample_desc {
    int64_t src_offset, dst_offset;
    int32_t src_w, src_h, dst_w, dst_h;
    float box[4];
    int32_t filter;
    int32_t reduce_x, reduce_y;    /* 1, 1: no reduce */
    int32_t reduce_box[4];         /* read only with a reduce */
    int32_t reserved;              /* 0 */
} aej_resample_desc;
AEJ_API int aej_resample_taps_host(int in_size, float in0, float in1, int out_size, int filter, int32_t *bounds_host, int32_t *taps_host,
                                   int64_t taps_capacity);
AEJ_API uint64_t aej_resample_workspace_bytes(aej_ctx *ctx, const aej_resample_desc *descs_host, int n);
AEJ_API int aej_resample_batch(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, uint8_t *dst,
                               uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes);
AEJ_API uint64_t aej_resample_workspace_bytes_ch(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const int *channels_host);
AEJ_API int aej_resample_batch_ch(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const int *channels_host, const uint8_t *src,
                                  uint64_t src_bytes, uint8_t *dst, uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes);
AEJ_API uint64_t aej_resample_workspace_bytes_win(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const int *channels_host,
                                                  const int32_t *windows_host);
AEJ_API int aej_resample_batch_win(aej_ctx *ctx, const aej_resample_desc *descs_host, int n, const int *channels_host, const int32_t *windows_host,
                                   const uint8_t *src, uint64_t src_bytes, uint8_t *dst, uint64_t dst_bytes, void *workspace,
                                   uint64_t workspace_bytes);

/* ---- PNG files decoded on the device (png_decode_many) ------------------------------------------------------------------------------
 * Pixel-identical to PIL.Image.open(file).convert("RGB"), or to the image in Pillow's own mode, for files of colour type
 * 0 (grey: 1, 2, 4, 8, 16 bits), 2 (RGB: 8, 16), 3 (palette: 1, 2, 4, 8), 4 (grey + alpha: 8, 16) and 6 (RGBA: 8, 16), Adam7-interlaced
 * or not (a parser hands out 16-bit and interlaced descriptors only when asked: aej_png_parse_host_accept).  The zlib stream of a file -- its
 * IDAT chunks joined -- is inflated by aej_inflate_batch (or by the host); the scanline un-filter and the expansion to the output layout
 * run in csrc/png.hip.  IDAT chunk CRCs are not checked (the Adler-32 of the inflated data is, on the device).  No gamma, ICC or sRGB
 * handling, as Pillow applies none on open.
 *
 * aej_png_parse_host: HOST only, needs no context.  Walks the chunks of one file into *desc (all zero before) and the IDAT spans:
 *   spans_host [span_capacity][2] int64 = { offset of the chunk's data in the file, its length }, empty chunks included.  spans_host
 *   may be NULL (a count query: desc->n_idat and idat_bytes are still filled); with span_capacity < n_idat: AEJ_ERR_CAPACITY.  Returns 0;
 *   AEJ_ERR_UNSUPPORTED for a valid file outside the supported set (16-bit samples, Adam7 interlace, APNG: an acTL or fdAT chunk, an
 *   unknown critical chunk, a side above 2^24); AEJ_ERR_ARG for a malformed file (bad signature, missing IHDR / PLTE / IDAT, a bad CRC
 *   on IHDR, PLTE or tRNS, zero width or height, a bit depth the colour type does not allow, a chunk length that runs past the file).
 *   msg (may be NULL) gets the reason.  Unknown ancillary chunks are skipped; tRNS is noted and otherwise ignored.
 * aej_png_parse_host_accept: the same walk with a word of AEJ_PNG_ACCEPT_* flags (any other bit: AEJ_ERR_ARG); aej_png_parse_host is
 *   this entry with 0.  AEJ_PNG_ACCEPT_ADAM7 takes interlaced files (desc->interlace = 1; row_bytes stays the full-width scanline),
 *   AEJ_PNG_ACCEPT_16BIT files of bit depth 16 (mode "I;16" for colour type 0, "RGB" for 2, "RGBA" for 4 and 6, as Pillow opens them).
 * aej_png_raw_bytes: the inflated size a file of this descriptor must have: height x (1 + row_bytes), or for an interlaced file the sum
 *   over its non-empty passes of h_p x (1 + row_bytes_p) -- a pass without pixels has no bytes, not even filter bytes.  0 for a bad one.
 * aej_png_adam7_passes_host: passes_host [7][6] int32 = { x0, y0, dx, dy, w_p, h_p } of the seven passes of a width x height image
 *   (pass p holds the pixels (x0 + i dx, y0 + j dy); w_p = h_p = 0 for an empty pass).  AEJ_ERR_ARG for a side below 1.
 * aej_png_workspace_bytes: the workspace of aej_png_unfilter_batch (one carried scanline per file; for an interlaced file one per
 *   non-empty pass, its pass images and eight status words); 0 for bad descriptors.
 * aej_png_unfilter_batch: n files.  Only enqueues on the context's stream: no synchronisation, no read-back.  inflated: device bytes,
 *   the filtered scanlines of file i -- aej_png_raw_bytes of them -- at in_offsets_host[i], a multiple of 4, and with its length
 *   rounded up to 4 inside inflated_bytes (whole dwords are read).  inflate_out_bytes / inflate_status: the device arrays
 *   aej_inflate_batch wrote for the n streams, or both NULL for scanlines the host inflated (and whose sizes it has checked).
 *   palettes: device [n][768], the desc's palette of each file (NULL when no file has colour type 3).  layouts_host[i] (NULL: all RGB):
 *   AEJ_PNG_RGB -- [height][width][3]: alpha dropped, grey replicated, indices through the palette (one past its end reads black) -- or
 *   AEJ_PNG_AUTO -- colour type 0: [height][width] (1 bit -> 0 / 255, 2 bits x 85, 4 bits x 17), 4: [..][2], 2: [..][3], 6: [..][4],
 *   3: [..][3] through the palette; at bit depth 16 colour type 0: [height][width] uint16 in host byte order (Pillow's "I;16"; an even
 *   offset is the caller's business), 2: [..][3], 4 and 6: [..][4], the high byte of every sample (grey + alpha as Pillow's RGBA: the
 *   grey three times).  Under AEJ_PNG_RGB a 16-bit sample gives its high byte, but a 16-bit GREY sample is CLIPPED: min(sample, 255),
 *   which is what Pillow's convert("RGB") of an "I;16" image does.  An interlaced file gives the image of the non-interlaced file with
 *   the same samples: each pass is un-filtered into the workspace and a second kernel interleaves them.  Image i is written at out_offsets_host[i]; nothing else of out is touched.  status: device [n]
 *   int32, AEJ_PNG_*; a file whose status is not OK leaves its image partly written or untouched, the other files are not affected. */
enum { AEJ_PNG_OK = 0, AEJ_PNG_INFLATE_FAILED = 1, AEJ_PNG_SIZE_MISMATCH = 2 /* inflated bytes != height * (1 + row_bytes), or != aej_png_raw_bytes */,
       AEJ_PNG_BAD_FILTER = 3 /* a filter byte above 4 */ };
enum { AEJ_PNG_RGB = 0, AEJ_PNG_AUTO = 1 };
enum { AEJ_PNG_ACCEPT_ADAM7 = 1, AEJ_PNG_ACCEPT_16BIT = 2 };
typedef struct aej_png_desc {
    int32_t width, height;
    int32_t bit_depth, colour_type;
    int32_t channels;              /* samples per pixel in the file: 1, 3, 1, 2, 4 for colour type 0, 2, 3, 4, 6 */
    int32_t row_bytes;             /* ceil(width * channels * bit_depth / 8): a scanline without its filter byte */
    int32_t interlace;
    int32_t n_idat;                /* IDAT chunks, empty ones included */
    int32_t palette_len;           /* entries of PLTE (0: none) */
    int32_t has_trns;
    int64_t idat_bytes;            /* their data bytes together: the length of the zlib stream */
    uint8_t palette[768];          /* PLTE, zero past palette_len */
    char mode[8];                  /* Pillow's mode of the opened file: "1", "L", "P", "RGB", "LA", "RGBA", "I;16" */
} aej_png_desc;
AEJ_API int aej_png_parse_host(const uint8_t *data_host, uint64_t nbytes, aej_png_desc *desc_host, int64_t *spans_host, int span_capacity,
                               char *msg, int msg_capacity);
AEJ_API int aej_png_parse_host_accept(const uint8_t *data_host, uint64_t nbytes, uint32_t accept, aej_png_desc *desc_host, int64_t *spans_host,
                                      int span_capacity, char *msg, int msg_capacity);
AEJ_API uint64_t aej_png_raw_bytes(const aej_png_desc *desc_host);
AEJ_API int aej_png_adam7_passes_host(int width, int height, int32_t *passes_host);
AEJ_API uint64_t aej_png_workspace_bytes(aej_ctx *ctx, const aej_png_desc *descs_host, int n);
AEJ_API int aej_png_unfilter_batch(aej_ctx *ctx, const aej_png_desc *descs_host, int n, const uint8_t *inflated, uint64_t inflated_bytes,
                                   const int64_t *in_offsets_host, const int64_t *inflate_out_bytes, const int32_t *inflate_status,
                                   const uint8_t *palettes, const int32_t *layouts_host, uint8_t *out, uint64_t out_bytes,
                                   const int64_t *out_offsets_host, int32_t *status, void *workspace, uint64_t workspace_bytes);

/* ---- PNG encode: the scanline filter of png_encode_many (csrc/png.hip), Pillow's choice rule ----
 * Every row gets the filter Pillow's writer picks (not libpng's heuristic): cost(f) = sum of (v < 128 ? v : 256 - v) over the row's
 * filtered bytes v, the row above the first row all zeros; None (0) to start with and kept if its cost is 0, otherwise Up (2), Sub (1),
 * Average (3, only when optimize != 0) and Paeth (4) are tried in that order and taken only when strictly cheaper.
 * aej_png_filter_bytes: height x (1 + row_bytes), the bytes of one image's scanline stream; 0 for a shape the filter refuses (height
 *   outside 1 .. 2^24, bpp outside 1 .. 4, row_bytes outside bpp .. 2^24 or no multiple of bpp).
 * aej_png_filter_batch: descs_host = [n][5] int64: the image's DEVICE pointer, its height, row bytes, bytes per pixel, and the offset of
 *   its scanline stream in `out` (device, 4-byte aligned; the offsets need no alignment).  An image is `height` rows of `row_bytes`
 *   bytes, CONTIGUOUS, at any address; the call refuses a NULL pointer, a shape as above and a stream outside out_bytes with
 *   AEJ_ERR_ARG.  Rows are independent (a row is filtered against the raw row above): one wave per row, all rows of 64 images a launch.
 *   Only enqueues on the context's stream. */
AEJ_API uint64_t aej_png_filter_bytes(int height, int row_bytes, int bpp);
AEJ_API int aej_png_filter_batch(aej_ctx *ctx, const int64_t *descs_host, int n, int optimize, uint8_t *out, uint64_t out_bytes);

/* ---- Pillow's BoxBlur, GaussianBlur and UnsharpMask for packed 8-bit images of 1 to 4 channels (filter_many, csrc/filter.hip) --------
 * Image.filter with ImageFilter.BoxBlur / GaussianBlur / UnsharpMask, bit for bit, for many images of different sizes, channel counts
 * and filters in one call.  An image is uint8 [h][w][channels], packed; channels are filtered independently (no alpha
 * pre-multiplication).  The three filters are one family: `passes` runs of one extended box blur per axis, then an optional integer
 * epilogue, all in uint32 on uint8 samples with a defined rounding after every pass.
 *   box radius of a Gaussian radius (float32 steps, the square root and the floor in double), passes = 3:
 *     sigma2 = radius * radius / 3;  L = sqrt(12 sigma2 + 1);  l = floor((L - 1) / 2);
 *     a = (2 l + 1) (l (l + 1) - 3 sigma2) / (6 (sigma2 - (l + 1) (l + 1)));  box = l + a
 *   weights of one float32 box radius fr:  r = (int)fr;  ww = (uint32)(2^24 / (fr * 2 + 1)) (a float32 division);
 *     fw = (uint32)(2^24 - (2 r + 1) ww) / 2
 *   one pass along a line p of N samples, indices clamped to [0, N - 1]:
 *     out(x) = (ww * sum(p[x - r .. x + r]) + fw * (p[x - r - 1] + p[x + r + 1]) + 2^23) >> 24
 *   a filter with box radii (bx, by): if bx != 0, `passes` horizontal passes, each on the uint8 output of the one before; then, if
 *     by != 0, `passes` vertical ones; both 0: a copy.  AEJ_FILTER_BOX: passes = 1 and the radii as given; AEJ_FILTER_GAUSSIAN:
 *     passes = 3 and the mapping above per axis; AEJ_FILTER_UNSHARP: the Gaussian, then per sample diff = in - blur and
 *     out = clip(in + diff * percent / 100, 0, 255) (C division) where |diff| > threshold, in elsewhere.
 *
 * aej_filter_plan_host: HOST only, needs no context: the passes and, per axis (x, y), the float32 box radius and r, ww, fw of a
 *   filter -- the one place where the mapping and the weights are computed; the batch entry uses it.  AEJ_ERR_ARG for an unknown kind
 *   and a radius that is negative or not finite; AEJ_ERR_UNSUPPORTED for a box radius whose integer part exceeds 1024.
 * aej_filter_geometry_host: HOST only: out[0..5] = the fused kernel's tile width and height in pixels and its largest halo (the most
 *   passes * (r + 1) may be on an axis), the pixels of a row kernel's span, the rows of a column kernel's band and the byte columns
 *   of a column kernel's workgroup.
 * aej_filter_batch: n images.  src / dst: device bytes; image i is read at src + src_offset and written at dst + dst_offset, exactly
 *   width * height * channels bytes and no other byte of dst; src and dst must not overlap.  path: AEJ_FILTER_AUTO (per image: the
 *   fused kernel where its halo allows), AEJ_FILTER_FUSED (AEJ_ERR_ARG naming the image whose filter is beyond the halo) or
 *   AEJ_FILTER_PASSES.  Fused: one launch per channel count present, one read and one write of the image.  Passes: one launch per
 *   pass over every image that needs it -- at most 2 * passes launches per channel count present -- through two buffers per image in
 *   the workspace.  One upload of the entries, then the call waits for it; nothing is copied back.  Every descriptor is checked
 *   before any device work: AEJ_ERR_ARG naming the image for a size below 1 or above 65535, a channel count outside 1 .. 4, an
 *   unknown kind, a bad radius, an image outside src_bytes / dst_bytes; AEJ_ERR_UNSUPPORTED naming it for a box radius above 1024 and
 *   |percent| above 1000000.  Workspace: aej_filter_workspace_bytes with the same descriptors and path (0 for ones the call refuses). */
enum { AEJ_FILTER_BOX = 0, AEJ_FILTER_GAUSSIAN = 1, AEJ_FILTER_UNSHARP = 2 };
enum { AEJ_FILTER_AUTO = 0, AEJ_FILTER_FUSED = 1, AEJ_FILTER_PASSES = 2 };
typedef struct aej_filter_desc {
    int64_t src_offset, dst_offset;
    int32_t width, height, channels;
    int32_t kind;                  /* AEJ_FILTER_* */
    float xradius, yradius;        /* the filter's radii as given (AEJ_FILTER_UNSHARP: both its one radius) */
    int32_t percent, threshold;    /* read only for AEJ_FILTER_UNSHARP */
} aej_filter_desc;
typedef struct aej_filter_plan {
    int32_t passes;
    float box[2];                  /* x, y */
    int32_t r[2];
    uint32_t ww[2], fw[2];
} aej_filter_plan;
AEJ_API int aej_filter_plan_host(int kind, float xradius, float yradius, aej_filter_plan *out);
AEJ_API int aej_filter_geometry_host(int32_t *out);
AEJ_API uint64_t aej_filter_workspace_bytes(aej_ctx *ctx, const aej_filter_desc *descs_host, int n, int path);
AEJ_API int aej_filter_batch(aej_ctx *ctx, const aej_filter_desc *descs_host, int n, int path, const uint8_t *src, uint64_t src_bytes,
                             uint8_t *dst, uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes);

/* ---- Pillow's Kernel, rank and mode filters for packed 8-bit images of 1 to 4 channels (filter_many, csrc/window.hip) ----------------
 * Image.filter with ImageFilter.Kernel (and the ten built-ins, which are Kernels), RankFilter / MedianFilter / MinFilter / MaxFilter
 * and ModeFilter, bit for bit, for many images of different sizes, channel counts and filters in one call.  An image is uint8
 * [h][w][channels], packed; channels are filtered independently.  Three families, each with its own border rule:
 *   AEJ_WINDOW_KERNEL, size k = 3 or 5, r = k / 2: all in float32, every operation rounded (no fused multiply-add, no re-association):
 *     q[i] = kernel[i] / scale;  ss0 = offset + 0.5f -- both once, on the host, in the library;
 *     for r <= x < w - r and r <= y < h - r:  ss = ss0;  for j = 0 .. k - 1:
 *       ss = ss + (((q[j k] p[y + r - j][x - r] + q[j k + 1] p[y + r - j][x - r + 1]) + ...) + q[j k + k - 1] p[y + r - j][x + r])
 *     -- kernel row 0 meets the image row BELOW the sample (a vertical flip, no horizontal one), the products of a row are added left
 *     to right and the row's sum is added to ss --;  out = 0 if ss <= 0, 255 if ss >= 255, else ss truncated.
 *     Samples within r of an edge are copies of the source; an image with w < k or h < k is a copy.
 *   AEJ_WINDOW_RANK, size odd, 0 <= rank < size^2: out = the rank-th smallest (from 0) of the size x size window centred on the sample,
 *     window positions clamped to the image (edge replication); every sample is computed.  Min is rank 0, Max rank size^2 - 1, Median
 *     rank size^2 / 2.
 *   AEJ_WINDOW_MODE, r = size / 2 (an even size acts as size + 1): over the window [y - r, y + r] x [x - r, x + r] clipped to the image
 *     (positions outside do not vote) the most frequent value, the smallest one on a tie; out = that value if it occurs MORE THAN
 *     TWICE, else the sample itself.
 *
 * aej_window_geometry_host: HOST only: out[0..4] = the tile width and height in pixels and the largest halo (r) of a Kernel, a rank
 *   and a mode filter.
 * aej_window_batch: n images.  src / dst: device bytes; image i is read at src + src_offset and written at dst + dst_offset, exactly
 *   width * height * channels bytes and no other byte of dst; src and dst must not overlap.  One launch per kind (and Kernel size) and
 *   channel count present, one read and one write of the image: a workgroup stages a tile and its halo in LDS.  One upload of the
 *   entries, then the call waits for it; nothing is copied back.  Every descriptor is checked before any device work: AEJ_ERR_ARG
 *   naming the image for a size below 1 or above 65535, a channel count outside 1 .. 4, an unknown kind, a Kernel size other than 3
 *   or 5, a kernel value, scale, offset or quotient that is not finite, a scale of 0, a rank size that is even or below 1, a rank
 *   outside [0, size^2), a mode size below 1, an image outside src_bytes / dst_bytes; AEJ_ERR_UNSUPPORTED naming it for a rank size
 *   above 15, a mode size above 7 and a |kernel[i] / scale| or |offset| above 2^100 (below that no partial sum overflows float32, so
 *   no NaN reaches the clip).  Workspace: aej_window_workspace_bytes with the same descriptors (0 for ones the call refuses): the
 *   entries only. */
enum { AEJ_WINDOW_KERNEL = 0, AEJ_WINDOW_RANK = 1, AEJ_WINDOW_MODE = 2 };
typedef struct aej_window_desc {
    int64_t src_offset, dst_offset;
    int32_t width, height, channels;
    int32_t kind;                  /* AEJ_WINDOW_* */
    int32_t size;                  /* AEJ_WINDOW_KERNEL: 3 or 5; _RANK: odd, 1 .. 15; _MODE: 1 .. 7 */
    int32_t rank;                  /* read only for AEJ_WINDOW_RANK */
    float scale, offset;           /* read only for AEJ_WINDOW_KERNEL, as given */
    float kernel[25];              /* the first size * size values, row by row, as given */
    int32_t reserved;
} aej_window_desc;
AEJ_API int aej_window_geometry_host(int32_t *out);
AEJ_API uint64_t aej_window_workspace_bytes(aej_ctx *ctx, const aej_window_desc *descs_host, int n);
AEJ_API int aej_window_batch(aej_ctx *ctx, const aej_window_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes,
                             uint8_t *dst, uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes);

/* ---- Pillow's Color3DLUT for packed 8-bit images of 3 and 4 channels (filter_many, csrc/lut3d.hip) ------------------------------------
 * Image.filter with ImageFilter.Color3DLUT, bit for bit, for many images of different sizes, channel counts and tables in one call.  An
 * image is uint8 [h][w][channels_in], packed; its first three bytes are the coordinates in the table, R on axis 1, G on axis 2, B on
 * axis 3.  A table is INT16 [s3][s2][s1][table_channels] (axis 1 fastest), made from the floats by aej_lut3d_prepare_host.
 *
 * aej_lut3d_prepare_host: HOST only, the one place the float -> INT16 rule lives: n floats -> n INT16.  With K = 255 << 6 = 16320:
 *     v >= (32767 - 0.5) / K -> 32767;  v <= (-32768 + 0.5) / K -> -32768 (both compared in double: +-inf clamp);  otherwise
 *     p = v * K rounded to FLOAT32, then (int16)(p - 0.5) for v < 0, else (int16)(p + 0.5), the +-0.5 added in double and the
 *     conversion truncating toward zero.  AEJ_ERR_ARG for a NaN (Pillow's result for one is undefined) and for a NULL pointer.
 *
 * Per pixel, with s1, s2, s3 = size and tc = table_channels, all in integers:
 *     scale_d = (uint32)((s_d - 1) / 255.0 * (1 << 18))          -- once per image, on the host, in double, truncated
 *     i_d     = byte_d * scale_d;   cell_d = i_d >> 18;   shift_d = (i_d & 0x3FFFF) >> 3          -- shift_d in 0 .. 32767
 *     base    = tc * (cell_1 + cell_2 * s1 + cell_3 * s1 * s2)
 *     lerp(a, b, s) = (a * (32768 - s) + b * s) >> 15            -- int32, arithmetic shift, per channel
 *   along axis 1 four times (the corner pairs at base, base + s1 tc, base + s1 s2 tc, base + (s1 s2 + s1) tc, each with the entry tc
 *   further on) by shift_1, then along axis 2 twice by shift_2, then along axis 3 by shift_3;  out = clamp((v + 32) >> 6, 0, 255).
 *   255 divides no s_d - 1 in 1 .. 64, so 255 * scale_d < (s_d - 1) << 18 and cell_d <= s_d - 2: the further corner is always in the
 *   table.  |a| <= 2^15 and the two weights sum to 2^15, so no product or sum leaves int32.
 *   (channels_in, table_channels, channels_out): (3, 3, 3); (4, 3, 3) drops the fourth byte; (4, 3, 4) copies the source's fourth byte;
 *   (3, 4, 4) and (4, 4, 4) take the fourth byte from the table.  (., 4, 3) and (3, 3, 4) are refused, as Pillow refuses them.
 *
 * aej_lut3d_geometry_host: HOST only: out[0..2] = the lanes of a workgroup, the adjacent pixels a lane takes at a time and the pixels
 *   of a workgroup's tile.  (There is no LDS path for small tables: it was measured and not kept, EXPERIMENTS.md.)
 * aej_lut3d_batch: n images.  src / dst: device bytes; image i is read at src + src_offset (width * height * channels_in bytes) and
 *   written at dst + dst_offset, exactly width * height * channels_out bytes and no other byte of dst; src and dst must not overlap.
 *   tables_host: the call's n_tables distinct tables back to back, table t at INT16 elements [table_offsets[t], table_offsets[t + 1])
 *   (table_offsets has n_tables + 1 entries); a descriptor names its table by index, below n_tables and below n (a call has no use for more tables than
 *   images; the size query, which is not told n_tables, relies on it), and the images of one table share its upload.
 *   One launch per (channels_in, table_channels, channels_out) present, one read and one write of the image, the table read through
 *   the caches; a lane takes four adjacent pixels in dwords, whatever the alignment of the image.
 *   One upload of the entries and the tables (every entry padded to four INT16), then the call waits for it; nothing is copied back.
 *   Every descriptor is checked before any device work: AEJ_ERR_ARG naming the image for a side below 1 or above 65535, a size outside
 *   [2, 65], channel counts other than the five combinations above, a table index outside [0, n_tables), a table whose length is not
 *   s1 * s2 * s3 * table_channels, an image outside src_bytes / dst_bytes.  Workspace: aej_lut3d_workspace_bytes with the same
 *   descriptors (0 for ones the call refuses): the entries and the padded tables. */
typedef struct aej_lut3d_desc {
    int64_t src_offset, dst_offset;
    int32_t height, width;
    int32_t channels_in, channels_out, table_channels;      /* 3 or 4 each */
    int32_t size[3];               /* s1, s2, s3: 2 .. 65 */
    int32_t table;                 /* the image's table among the call's distinct tables */
    int32_t reserved;
} aej_lut3d_desc;
AEJ_API int aej_lut3d_prepare_host(const float *table, int64_t n, int16_t *out);
AEJ_API int aej_lut3d_geometry_host(int32_t *out);
AEJ_API uint64_t aej_lut3d_workspace_bytes(aej_ctx *ctx, const aej_lut3d_desc *descs_host, int n);
AEJ_API int aej_lut3d_batch(aej_ctx *ctx, const aej_lut3d_desc *descs_host, int n, const int16_t *tables_host,
                            const int64_t *table_offsets, int n_tables, const uint8_t *src, uint64_t src_bytes, uint8_t *dst,
                            uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes);

/* ---- Pillow's Image.transform, rotate and transpose for packed 8-bit images of 1 to 4 channels (geometry.py, csrc/warp.hip) ---------
 * Image.transform with AFFINE, PERSPECTIVE and QUAD under NEAREST, BILINEAR and BICUBIC, and Image.transpose with its seven methods,
 * bit for bit, for many images of different sizes, channel counts, paths and filters in one call.  An image is uint8
 * [h][w][channels], packed.  EXTENT and Image.rotate are AFFINE by the time they get here (geometry.py restates Image.py).
 *
 * All arithmetic is IEEE float64, every operation rounded, nothing fused or re-associated.  For output pixel (x, y), xin = x + 0.5,
 * yin = y + 0.5, coef = a:
 *   AEJ_WARP_AFFINE       xx = (a0 xin + a1 yin) + a2;  yy = (a3 xin + a4 yin) + a5
 *   AEJ_WARP_PERSPECTIVE  the same numerators, each divided by (a6 xin + a7 yin) + 1
 *   AEJ_WARP_QUAD         xx = ((a0 + a1 xin) + a2 yin) + (a3 xin) yin;  yy = ((a4 + a5 xin) + a6 yin) + (a7 xin) yin
 * AEJ_WARP_NEAREST under PERSPECTIVE and QUAD: the source pixel (trunc xx, trunc yy) if 0 <= xx < W and 0 <= yy < H, else outside.
 * AEJ_WARP_NEAREST under AFFINE never evaluates the above; the library resolves the image to one of two integer paths, as Pillow does:
 *   AEJ_WARP_TABLES (a1 == 0 and a3 == 0): xo = a2 + a0 0.5; for x = 0 .. w - 1 in turn: xtab[x] = xo < 0 ? -1 : trunc xo; xo += a0 --
 *     a running sum, built on the host -- and ytab likewise from a5 and a4; the source pixel is (xtab[x], ytab[y]) if in range.
 *   AEJ_WARP_FIXED (else), 16.16 fixed point with FIX(v) = floor(v 65536 + 0.5):  A0 = FIX(a0), A1 = FIX(a1), A3 = FIX(a3), A4 = FIX(a4),
 *     A2 = FIX((a2 + a0 0.5) + a1 0.5), A5 = FIX((a5 + a3 0.5) + a4 0.5);  xi = (A2 + x A0 + y A1) >> 16, yi = (A5 + x A3 + y A4) >> 16
 *     in int64; the source pixel is (xi, yi) if in range.  Pillow takes this path only while |x a0 + y a1 + a2| < 32768 and
 *     |x a3 + y a4 + a5| < 32768 at (0, 0), (w, 0), (0, h), (w, h); beyond that (and for a constant outside int32) the image is
 *     refused with AEJ_ERR_UNSUPPORTED: Pillow's float64 running-sum fallback is not built.  With sides up to 32767 the guard keeps
 *     Pillow's int32 sums and these int64 sums on the same side of every range test.
 * AEJ_WARP_BILINEAR: outside unless 0 <= xx < W and 0 <= yy < H.  xx -= 0.5, yy -= 0.5, x = floor xx, y = floor yy, dx = xx - x,
 *   dy = yy - y; columns x, x + 1 clamped to the image, row y clamped:  v1 = p[x0] + (p[x1] - p[x0]) dx on row y; v2 the same on row
 *   y + 1 if that row exists, else v2 = v1;  v = v1 + (v2 - v1) dy, truncated.
 * AEJ_WARP_BICUBIC: the same test, x, y, dx, dy; x -= 1, y -= 1; columns x .. x + 3 clamped; cub(v1, v2, v3, v4, d) = p1 + d (p2 + d (p3 +
 *   d p4)) with p1 = v2, p2 = -v1 + v3, p3 = ((2 (v1 - v2)) + v3) - v4, p4 = ((-v1 + v2) - v3) + v4.  Row y clamped; each of rows y + 1,
 *   y + 2, y + 3 is evaluated if it exists and else repeats the value of the row before it; cub over the four with dy; 0 if v <= 0,
 *   255 if v >= 255, else truncated.
 * A coordinate that is NaN (undefined in Pillow) makes the pixel an outside one.  Outside pixels take `fill`.
 * premultiply (read for 2 and 4 channels under BILINEAR and BICUBIC only; the last channel is alpha): a sample c becomes
 *   ((t >> 8) + t) >> 8 with t = c alpha + 128 as it is loaded, and the result (the fill as given included) is un-premultiplied as it
 *   is stored: unchanged for alpha 0 and 255, else min(255, 255 c / alpha) in integers.
 * AEJ_WARP_TRANSPOSE: `method` is Pillow's Image.Transpose value (0 FLIP_LEFT_RIGHT, 1 FLIP_TOP_BOTTOM, 2 ROTATE_90, 3 ROTATE_180,
 *   4 ROTATE_270, 5 TRANSPOSE, 6 TRANSVERSE); dst_w x dst_h must be the source's size for 0, 1, 3 and its transpose for the others.
 *
 * aej_warp_geometry_host: HOST only: out[0..5] = the warp kernel's tile width and height in pixels, the mirrored copy's tile in bytes
 *   of a row and rows, the transposing kernel's tile width and height in pixels.
 * aej_warp_plan_host: HOST only, no device and no context: what the library makes of ONE descriptor (offsets not read):
 *   out->path the resolved path, out->premultiply whether alpha is premultiplied, out->fixed A0 .. A5 for AEJ_WARP_FIXED; for
 *   AEJ_WARP_TABLES tables[0 .. dst_w) = xtab and tables[dst_w .. dst_w + dst_h) = ytab (tables_len >= dst_w + dst_h, else
 *   AEJ_ERR_CAPACITY; tables may be NULL for the other paths).  Returns the code aej_warp_batch would refuse the descriptor with.
 * aej_warp_batch: n images.  src / dst: device bytes; image i is read at src + src_offset (src_w src_h channels bytes) and written at
 *   dst + dst_offset, exactly dst_w dst_h channels bytes and no other byte of dst; no source image may overlap dst.  One launch per
 *   (channels, filter, path) present; one thread per output pixel, a workgroup owns a 32 x 8 output tile; one upload of the entries
 *   and tables, then the call waits for it; nothing is copied back.  Every descriptor is checked before any device work: AEJ_ERR_ARG
 *   naming the image for a size below 1 or above 32767, a channel count outside 1 .. 4, a path that is not one of TRANSPOSE, AFFINE,
 *   PERSPECTIVE, QUAD (TABLES and FIXED are what the library resolves AFFINE to, not inputs), an unknown filter or transpose method,
 *   a coefficient that is not finite, a transposed size that does not fit, an image outside src_bytes / dst_bytes;
 *   AEJ_ERR_UNSUPPORTED naming it for an AFFINE under NEAREST beyond the fixed-point guard.  Workspace: aej_warp_workspace_bytes with
 *   the same descriptors (0 for ones the call refuses): the entries and the tables. */
enum { AEJ_WARP_TRANSPOSE = 0, AEJ_WARP_TABLES = 1, AEJ_WARP_FIXED = 2, AEJ_WARP_AFFINE = 3, AEJ_WARP_PERSPECTIVE = 4, AEJ_WARP_QUAD = 5 };
enum { AEJ_WARP_NEAREST = 0, AEJ_WARP_BILINEAR = 2, AEJ_WARP_BICUBIC = 3 };      /* Pillow's Image.Resampling values */
typedef struct aej_warp_desc {
    int64_t src_offset, dst_offset;
    int32_t src_w, src_h, dst_w, dst_h, channels;
    int32_t path;                  /* AEJ_WARP_TRANSPOSE, _AFFINE, _PERSPECTIVE or _QUAD */
    int32_t method;                /* AEJ_WARP_TRANSPOSE: Pillow's Image.Transpose value */
    int32_t filter;                /* AEJ_WARP_NEAREST, _BILINEAR, _BICUBIC (not read for AEJ_WARP_TRANSPOSE) */
    double coef[8];                /* AFFINE: 6, PERSPECTIVE: 8, QUAD: the 8 of its bilinear form */
    uint8_t fill[4];               /* the outside pixel, one byte per channel */
    int32_t premultiply;           /* 0 or 1 */
    int32_t reserved[2];
} aej_warp_desc;
typedef struct aej_warp_plan {
    int32_t path, premultiply;
    int64_t fixed[6];              /* A0 .. A5 */
} aej_warp_plan;
AEJ_API int aej_warp_geometry_host(int32_t *out);
AEJ_API int aej_warp_plan_host(const aej_warp_desc *desc, aej_warp_plan *out, int32_t *tables, int64_t tables_len);
AEJ_API uint64_t aej_warp_workspace_bytes(aej_ctx *ctx, const aej_warp_desc *descs_host, int n);
AEJ_API int aej_warp_batch(aej_ctx *ctx, const aej_warp_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, uint8_t *dst,
                           uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes);

/* ---- Pillow's ImageEnhance, ImageOps point operations, Image.point and Image.histogram for packed 8-bit images (adjust.py, csrc/adjust.hip)
 * A chain of up to 8 ops per image, bit for bit, for many images of different sizes, channel counts and chains in one call.  An image
 * is uint8 [h][w][channels], packed: 1 L, 2 LA, 3 RGB, 4 RGBA; the last band of 2 and 4 channels is alpha.
 *
 * L of a pixel: band 0 for 1 and 2 channels, else (r 19595 + g 38470 + b 7471 + 0x8000) >> 16; alpha is ignored.
 * The enhancers are Image.blend(degenerate, image, factor), a = factor as float32, all float32, the product and the sum rounded
 * separately (no fused multiply-add):  t = float(d) + a float(s - d);  for 0 <= a <= 1 out = t truncated, otherwise
 * out = 0 if t <= 0, 255 if t >= 255, else t truncated.  The alpha band of every degenerate is the image's own, so alpha is unchanged.
 *   AEJ_ADJUST_BRIGHTNESS  d = 0
 *   AEJ_ADJUST_CONTRAST    d = int(sum_i(i h[i]) / pixels + 0.5) in float64, h the histogram of L (the sum is an exact integer)
 *   AEJ_ADJUST_COLOR       d = L in every colour band; an image of 1 or 2 channels is unchanged
 *   AEJ_ADJUST_SHARPNESS   d = filter(SMOOTH): the AEJ_WINDOW_KERNEL (1 1 1, 1 5 1, 1 1 1) / 13 of every band; samples within 1 of an
 *                          edge are copies of the image
 * The table ops map every band b through table[b][v]:
 *   AEJ_ADJUST_AUTOCONTRAST  ImageOps.autocontrast, loop for loop, per band from that band's histogram, or with preserve_tone one table
 *     from the histogram of L for all bands: bins with their bit in `ignore` are zeroed; n = the sum of the bins;
 *     cut = int(n cutoff[0] // 100) (float64 floor division as Python's) is taken off the low end bin by bin, int(n cutoff[1] // 100)
 *     off the high end; lo and hi = the first and last non-zero bin (255 and 0 if there is none); the identity if hi <= lo, else
 *     scale = 255.0 / (hi - lo), offset = -lo scale, table[i] = int(i scale + offset) clipped to 0 .. 255, in float64.
 *   AEJ_ADJUST_EQUALIZE  ImageOps.equalize per band: over the NON-ZERO bins, step = (their sum - the last of them) / 255 in integers;
 *     the identity with one non-zero bin or step 0; else n = step / 2 and for i = 0 .. 255: table[i] = min(n / step, 255), n += h[i].
 *   AEJ_ADJUST_LUT  table number `table` of the call's tables_host: 4 bands x 256 bytes (posterize, solarize, invert, Image.point).
 *   Both histogram ops take 1 and 3 channels only, as Pillow's _lut.
 * AEJ_ADJUST_GRAYSCALE  convert("L"): one channel, L; the ops after it see a 1-channel image.
 *
 * One chain runs as segments.  Every step rounds to uint8 as Pillow's intermediate image would, so a segment is evaluated per pixel in
 * registers: the source is read once and the result written once.  A CONTRAST, AUTOCONTRAST or EQUALIZE adds one histogram launch,
 * which re-evaluates the steps of its segment before it, and one table launch; no intermediate image is written for it.  A SHARPNESS
 * that is not the first op starts a new segment whose input is the previous segment's output in the workspace; every SHARPNESS adds
 * one SMOOTH launch (window.hip) of its segment's input into the workspace.  launches = 2 passes + smooths + segments.
 *
 * aej_adjust_geometry_host: HOST only: out[0..3] = the pixels of a chunk (one workgroup's share of an image in the histogram and apply
 *   kernels), the threads of a workgroup, the largest grid (beyond it workgroups stride) and the bytes of a table.
 * aej_adjust_plan_host: HOST only, no device and no context: what the library makes of ONE descriptor (offsets and table numbers not
 *   read).  Returns the code aej_adjust_batch would refuse the descriptor with.
 * aej_adjust_batch: n images.  src / dst: device bytes; image i is read at src + src_offset (width height channels bytes) and written
 *   at dst + dst_offset, exactly width height out_channels bytes and no other byte of dst; no source image may overlap dst.
 *   tables_host: n_tables tables of 1024 bytes on the HOST (may be NULL when n_tables is 0).  Each launch is one grid over every
 *   image (of one channel count) that needs it.  The call zeroes its histograms itself, uploads its entries and tables once, runs on
 *   the context's stream and waits once at the end; nothing is read back in between.  Every descriptor is checked before any device
 *   work: AEJ_ERR_ARG naming the image for a size below 1 or above 32767, a channel count outside 1 .. 4, n_ops outside 1 .. 8, an
 *   unknown op, a factor that is not finite, a cutoff that is negative or not finite, a table number outside tables_host, a
 *   histogram op where the image has 2 or 4 channels, an image outside src_bytes / dst_bytes.  Workspace:
 *   aej_adjust_workspace_bytes with the same descriptors (0 for ones the call refuses): entries, tables, histograms and the planes.
 * aej_histogram_batch: Image.histogram() of n images (descriptors with n_ops = 0; dst_offset counts int64 elements): image i gets
 *   channels x 256 int64 counts at hist + dst_offset, band by band.  The counts are kept as uint32 (32767^2 fits) and widened on
 *   the device.  Same checks, same workspace query (descriptors with n_ops = 0 size this call). */
enum { AEJ_ADJUST_BRIGHTNESS = 0, AEJ_ADJUST_CONTRAST = 1, AEJ_ADJUST_COLOR = 2, AEJ_ADJUST_SHARPNESS = 3, AEJ_ADJUST_AUTOCONTRAST = 4,
       AEJ_ADJUST_EQUALIZE = 5, AEJ_ADJUST_LUT = 6, AEJ_ADJUST_GRAYSCALE = 7 };
#define AEJ_ADJUST_MAX_OPS 8
#define AEJ_ADJUST_TABLE_BYTES 1024
typedef struct aej_adjust_op {
    int32_t kind;                  /* AEJ_ADJUST_* */
    int32_t table;                 /* AEJ_ADJUST_LUT: its table in tables_host */
    float factor;                  /* the enhancers */
    int32_t preserve_tone;         /* AEJ_ADJUST_AUTOCONTRAST: 0 or 1 */
    double cutoff[2];              /* AEJ_ADJUST_AUTOCONTRAST: per cent off the low and the high end */
    uint32_t ignore[8];            /* AEJ_ADJUST_AUTOCONTRAST: bit v of the 256 set: bin v is zeroed */
} aej_adjust_op;
typedef struct aej_adjust_desc {
    int64_t src_offset, dst_offset;
    int32_t width, height, channels;
    int32_t n_ops;                 /* 1 .. 8; 0 for aej_histogram_batch */
    aej_adjust_op ops[AEJ_ADJUST_MAX_OPS];
} aej_adjust_desc;
typedef struct aej_adjust_plan {
    int32_t out_channels, n_segments, n_passes, n_smooths, n_launches;
    int32_t segment_first[AEJ_ADJUST_MAX_OPS];      /* the first op of each segment */
    int32_t reserved[3];
} aej_adjust_plan;
AEJ_API int aej_adjust_geometry_host(int32_t *out);
AEJ_API int aej_adjust_plan_host(const aej_adjust_desc *desc, aej_adjust_plan *out);
AEJ_API uint64_t aej_adjust_workspace_bytes(aej_ctx *ctx, const aej_adjust_desc *descs_host, int n);
AEJ_API int aej_adjust_batch(aej_ctx *ctx, const aej_adjust_desc *descs_host, int n, const uint8_t *tables_host, int n_tables,
                             const uint8_t *src, uint64_t src_bytes, uint8_t *dst, uint64_t dst_bytes, void *workspace,
                             uint64_t workspace_bytes);
AEJ_API int aej_histogram_batch(aej_ctx *ctx, const aej_adjust_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes,
                                int64_t *hist, uint64_t hist_elements, void *workspace, uint64_t workspace_bytes);

/* ---- Pillow's two-image operations for packed 8-bit images (compose.py, csrc/compose.hip): Image.paste, Image.alpha_composite,
 * Image.blend, Image.composite and ImageChops, bit for bit, for many elements of different sizes and channel counts in one call.
 * An element has a BASE (uint8 [h][w][channels], packed: 1 L, 2 LA, 3 RGB, 4 RGBA), an OVERLAY of over_channels channels (0: the
 * constant `colour`) whose pixel (0, 0) lies at pixel (x, y) of the base -- x and y may be negative --, and a MASK that lies where the
 * overlay lies.  The output is out_w x out_h x channels: the base's size, except for AEJ_COMPOSE_CHOP, where it is the common top-left
 * rectangle (the minimum of each side).  The REGION is the intersection of the output, of the overlay's rectangle at (x, y) and of
 * box[] = left, top, right, bottom in the overlay's own coordinates, moved to (x, y) as well.  Outside the region the output is the
 * base; inside, with d the base's, s the overlay's and m the mask's sample at the same place, all integer divisions truncating:
 *
 * AEJ_COMPOSE_PASTE (Image.paste; Image.composite(im1, im2, mask) is the paste of im1 over im2)  per band.  An overlay with one
 *   channel more than the base (4 over 3, 2 over 1) loses its last band.  By mask_kind:
 *   AEJ_COMPOSE_MASK_NONE     out = s
 *   AEJ_COMPOSE_MASK_BIT      Pillow's mode "1": out = m != 0 ? s : d
 *   AEJ_COMPOSE_MASK_BYTE     m = the LAST band of the mask's mask_channels (L, or the alpha of LA and RGBA):
 *                             t = d (255 - m) + s m + 128;  out = ((t >> 8) + t) >> 8  -- ONE division of the sum, not one per product.
 *                             Pillow's fill: a COLOUR through a 1-channel mask into a base of 2 or 4 channels takes m = 255 in the
 *                             bands before the last wherever m != 0 and the base's last band is 0; a colour takes no 2-channel mask
 *   AEJ_COMPOSE_MASK_OVERLAY  the same with m = the last band of the overlay's own pixel (paste(im, at, im)); no mask is read
 * AEJ_COMPOSE_ALPHA  Image.alpha_composite, 2 or 4 channels on both sides, sa and da the two last bands:  sa == 0: out = d.  Otherwise
 *   outa = sa 255 + da (255 - sa);  c1 = sa 255 255 128 / outa;  c2 = 255 128 - c1;  div255(t) = ((t >> 8) + t) >> 8;
 *   colour bands: out = div255(s c1 + d c2 + (0x80 << 7)) >> 7;  last band: out = div255(outa + 0x80).
 * AEJ_COMPOSE_BLEND  Image.blend(base, overlay, alpha) on every band, the last included: the float32 form of the enhancers above,
 *   t = float(d) + alpha float(s - d), the product and the sum rounded separately; 0 <= alpha <= 1: t truncated, otherwise clipped
 *   to 0 .. 255 and then truncated.
 * AEJ_COMPOSE_CHOP  ImageChops.<op>(base, overlay) on every band, a = d, b = s.  CLIPPED to 0 .. 255:
 *   AEJ_CHOP_ADD       int(float(a + b) / scale + float(offset)), float32, the quotient and the sum rounded separately, truncated
 *   AEJ_CHOP_SUBTRACT  the same with a - b
 *   AEJ_CHOP_MULTIPLY  a b / 255          AEJ_CHOP_SCREEN  255 - (255 - a) (255 - b) / 255
 *   AEJ_CHOP_LIGHTER   max(a, b)          AEJ_CHOP_DARKER  min(a, b)          AEJ_CHOP_DIFFERENCE  |a - b|
 *   and WRAPPED to a byte (& 255):
 *   AEJ_CHOP_ADD_MODULO  a + b            AEJ_CHOP_SUBTRACT_MODULO  a - b
 *   AEJ_CHOP_HARD_LIGHT  b < 128 ? a b / 127 : 255 - (255 - b) (255 - a) / 127
 *   AEJ_CHOP_OVERLAY     a < 128 ? a b / 127 : 255 - (255 - a) (255 - b) / 127
 *   AEJ_CHOP_SOFT_LIGHT  ((255 - a) (a b)) / 65536 + (a (255 - (255 - a) (255 - b) / 255)) / 255
 *
 * aej_compose_geometry_host: HOST only: out[0..2] = the pixels of a chunk (one workgroup's share of an output image), the threads of a
 *   workgroup, the largest grid (beyond it workgroups stride).
 * aej_compose_plan_host: HOST only, no device and no context: what the library makes of ONE descriptor (offsets not read): the output's
 *   size and the clipped region.  Returns the code aej_compose_batch would refuse the descriptor with.
 * aej_compose_batch: n elements.  src / dst: device bytes; element i reads its base at src + base_offset, its overlay at src +
 *   over_offset (unless over_channels is 0), its mask at src + mask_offset (AEJ_COMPOSE_MASK_BIT and _BYTE only), and writes exactly
 *   out_w out_h channels bytes at dst + dst_offset and no other byte of dst; several elements may name the same source bytes; no
 *   source may overlap dst.  One launch per channel count of the call, each one grid over every element of that count.  The call
 *   uploads its entries once, runs on the context's stream and waits once at the end.  Every descriptor is checked before any device
 *   work: AEJ_ERR_ARG naming the element for a size below 1 or above 32767, a channel count outside 1 .. 4, an unknown kind, op or
 *   mask kind, a pair of channel counts that is not built, a mask whose size is not the overlay's, AEJ_COMPOSE_MASK_OVERLAY with an
 *   overlay of 1 or 3 channels, an alpha, scale or offset that is not finite, a scale of 0, a source outside src_bytes, an image
 *   outside dst_bytes.  Workspace: aej_compose_workspace_bytes with the same descriptors (0 for ones the call refuses). */
enum { AEJ_COMPOSE_PASTE = 0, AEJ_COMPOSE_ALPHA = 1, AEJ_COMPOSE_BLEND = 2, AEJ_COMPOSE_CHOP = 3 };
enum { AEJ_COMPOSE_MASK_NONE = 0, AEJ_COMPOSE_MASK_BIT = 1, AEJ_COMPOSE_MASK_BYTE = 2, AEJ_COMPOSE_MASK_OVERLAY = 3 };
enum { AEJ_CHOP_ADD = 0, AEJ_CHOP_SUBTRACT = 1, AEJ_CHOP_ADD_MODULO = 2, AEJ_CHOP_SUBTRACT_MODULO = 3, AEJ_CHOP_MULTIPLY = 4,
       AEJ_CHOP_SCREEN = 5, AEJ_CHOP_LIGHTER = 6, AEJ_CHOP_DARKER = 7, AEJ_CHOP_DIFFERENCE = 8, AEJ_CHOP_SOFT_LIGHT = 9,
       AEJ_CHOP_HARD_LIGHT = 10, AEJ_CHOP_OVERLAY = 11 };
typedef struct aej_compose_desc {
    int64_t base_offset, over_offset, mask_offset, dst_offset;
    int32_t kind;                  /* AEJ_COMPOSE_* */
    int32_t op;                    /* AEJ_COMPOSE_CHOP: AEJ_CHOP_* */
    int32_t width, height, channels;               /* the base */
    int32_t over_width, over_height, over_channels;      /* the overlay; over_channels 0: `colour`, and the size is the region's */
    int32_t mask_width, mask_height, mask_channels;      /* the mask: AEJ_COMPOSE_MASK_BIT (1 channel, bytes 0 / not 0) and _BYTE */
    int32_t mask_kind;             /* AEJ_COMPOSE_MASK_* */
    int32_t x, y;                  /* where pixel (0, 0) of the overlay lies in the base */
    int32_t box[4];                /* left, top, right, bottom: the part of the overlay that is used, in its own coordinates */
    float alpha;                   /* AEJ_COMPOSE_BLEND */
    float scale, offset;           /* AEJ_CHOP_ADD and AEJ_CHOP_SUBTRACT */
    uint8_t colour[4];
    int32_t reserved[2];
} aej_compose_desc;
typedef struct aej_compose_plan {
    int32_t out_width, out_height, out_channels;
    int32_t region[4];             /* left, top, right, bottom in the output; all 0 when nothing of the overlay is inside */
    int32_t reads_overlay, reads_mask;
    int32_t reserved[3];
} aej_compose_plan;
AEJ_API int aej_compose_geometry_host(int32_t *out);
AEJ_API int aej_compose_plan_host(const aej_compose_desc *desc, aej_compose_plan *out);
AEJ_API uint64_t aej_compose_workspace_bytes(aej_ctx *ctx, const aej_compose_desc *descs_host, int n);
AEJ_API int aej_compose_batch(aej_ctx *ctx, const aej_compose_desc *descs_host, int n, const uint8_t *src, uint64_t src_bytes, uint8_t *dst,
                              uint64_t dst_bytes, void *workspace, uint64_t workspace_bytes);

/* ---- Pillow's Image.convert between its 8-bit modes, hue adjustment and ImageOps.colorize for packed 8-bit images (convert.py,
 * csrc/convert.hip), bit for bit, for many images of different sizes, channel counts and conversions in one call.  An image is uint8
 * [h][w][channels], packed; source_mode says what its channels MEAN (AEJ_MODE_*: L 1 band, LA 2, RGB, YCbCr and HSV 3, RGBA and CMYK 4).
 *
 * The route.  Image.convert (Pillow 12.2) has a direct converter for: L, LA, RGB and RGBA -> every mode; YCbCr -> L, LA, RGB;
 * HSV -> RGB; CMYK -> RGB, RGBA, HSV; and a mode to itself (a copy).  Any other pair goes through the source's base mode -- RGB for
 * YCbCr, HSV and CMYK -- in two steps, the image between them being 8-bit: CMYK -> L is CMYK -> RGB -> L, YCbCr -> HSV goes through RGB.
 * Both steps run per pixel in registers.  `>>` is an arithmetic shift, clip8 clamps to 0 .. 255, (int) and (float) are C casts.
 *
 * One step.  A source with grey meaning (L, LA, and YCbCr when the target is L or LA: its Y) gives g; any other gives r, g, b:
 *   CMYK -> r, g, b   per band c with k:  nk = 255 - k;  t = c nk + 128;  clip8(nk - (((t >> 8) + t) >> 8))
 *   YCbCr -> r, g, b  U(coef)[i] = (int)(coef (i - 128) 64 + 0.5) in float64:  r = clip8(y + (U(1.402)[cr] >> 6));
 *                     g = clip8(y + ((U(-.34414)[cb] + U(-.71414)[cr]) >> 6));  b = clip8(y + (U(1.772)[cb] >> 6))
 *   HSV -> r, g, b    s == 0: grey v.  Else in float64:  x = h 6.0 / 255.0;  i = floor(x);  f = (float)(x - i);  fs = (float)(s / 255.0);
 *                     p = round(v (1.0 - fs));  q = round(v (1.0 - fs f));  t = round(v (1.0 - fs (1.0 - f))), C's round, each clip8;
 *                     i mod 6 selects (v,t,p), (q,v,p), (p,v,t), (p,q,v), (t,p,v), (v,p,q)
 * and the target takes it:
 *   L      g, or (r 19595 + g 38470 + b 7471 + 0x8000) >> 16          LA    the same and alpha
 *   RGB    g, g, g or r, g, b                                          RGBA  the same and alpha
 *   YCbCr  (g, 128, 128), or with T(coef)[i] = (int)(coef i 64 + 0.5) in float64:  Y = (T(.299)[r] + T(.587)[g] + T(.114)[b]) >> 6;
 *          Cb = clip8(((T(-.16874)[r] + T(-.33126)[g] + T(.5)[b]) >> 6) + 128);  Cr = clip8(((T(.5)[r] + T(-.41869)[g] + T(-.08131)[b]) >> 6) + 128)
 *   HSV    (0, 0, g), or:  v = max;  max == min: h = s = 0.  Else in float32:  cr = (float)(max - min);  s = cr / (float)max;
 *          rc = (float)(max - r) / cr, gc and bc likewise;  h = bc - gc if r is the max, else 2.0 + rc - bc if g is, else 4.0 + gc - rc,
 *          evaluated in float64 from those float32 values and rounded to float32 once;  h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
 *          H = clip8((int)((double)h 255.0));  S = clip8((int)((double)s 255.0))
 *   CMYK   (0, 0, 0, 255 - g), or (255 - r, 255 - g, 255 - b, 0)
 * Alpha is the source's where it has one (LA, RGBA), else 255.
 *
 * AEJ_CONVERT_MODE    the route from source_mode to target_mode.
 * AEJ_CONVERT_MATRIX  im.convert("L", matrix4) / im.convert("RGB", matrix12): source_mode RGB, target L (matrix[0..3]) or RGB (a row of
 *                     four per band).  Per band in float32, left to right, each product and sum rounded:
 *                     v = ((m0 r + m1 g) + m2 b) + m3 + 0.5f;  v <= 0: 0;  v >= 255: 255;  else v truncated.
 * AEJ_CONVERT_HUE     source_mode RGB or RGBA, target the same: RGB -> HSV, H = (H + hue_shift) & 255, HSV -> RGB; alpha is kept.
 * AEJ_CONVERT_TABLE   ImageOps.colorize: source_mode L, target RGB: band b = table[b 256 + L] of table number `table` of tables_host
 *                     (768 bytes each: red, green, blue).
 *
 * aej_convert_geometry_host: HOST only: out[0..2] = the pixels of a chunk (one workgroup's share of an image), the threads of a
 *   workgroup, the largest grid (beyond it workgroups stride).
 * aej_convert_plan_host: HOST only, no device and no context: the route of ONE descriptor (offsets and table numbers not read).
 *   Returns the code aej_convert_batch would refuse the descriptor with.
 * aej_convert_batch: n images.  src / dst: device bytes; image i is read at src + src_offset (width height channels bytes) and written
 *   at dst + dst_offset, exactly width height out_channels bytes and no other byte of dst; no source image may overlap dst.
 *   tables_host: n_tables tables of 768 bytes on the HOST (may be NULL when n_tables is 0).  One launch per pair of channel counts of
 *   the call, each one grid over every image of that pair.  The call uploads its entries and tables once, runs on the context's stream
 *   and waits once at the end.  Every descriptor is checked before any device work: AEJ_ERR_ARG naming the image for a size below 1 or
 *   above 32767, an unknown mode or kind, a source_mode whose bands are not `channels`, a MATRIX, HUE or TABLE on modes other than the
 *   ones above, a matrix entry that is not finite, a hue_shift outside 0 .. 255, a table number outside tables_host, an image outside
 *   src_bytes / dst_bytes.  Workspace: aej_convert_workspace_bytes with the same descriptors (0 for ones the call refuses). */
enum { AEJ_MODE_L = 0, AEJ_MODE_LA = 1, AEJ_MODE_RGB = 2, AEJ_MODE_RGBA = 3, AEJ_MODE_YCBCR = 4, AEJ_MODE_HSV = 5, AEJ_MODE_CMYK = 6 };
enum { AEJ_CONVERT_MODE = 0, AEJ_CONVERT_MATRIX = 1, AEJ_CONVERT_HUE = 2, AEJ_CONVERT_TABLE = 3 };
#define AEJ_CONVERT_TABLE_BYTES 768
typedef struct aej_convert_desc {
    int64_t src_offset, dst_offset;
    int32_t width, height, channels;
    int32_t source_mode, target_mode;      /* AEJ_MODE_* */
    int32_t kind;                  /* AEJ_CONVERT_* */
    int32_t hue_shift;             /* AEJ_CONVERT_HUE: 0 .. 255, added to H modulo 256 */
    int32_t table;                 /* AEJ_CONVERT_TABLE: its table in tables_host */
    float matrix[12];              /* AEJ_CONVERT_MATRIX */
    int32_t reserved[2];
} aej_convert_desc;
typedef struct aej_convert_plan {
    int32_t out_channels, n_steps; /* n_steps: 1 or 2 conversions (AEJ_CONVERT_HUE: 2; MATRIX and TABLE: 1) */
    int32_t step_from[2], step_to[2];      /* AEJ_MODE_* of each */
    int32_t reserved[2];
} aej_convert_plan;
AEJ_API int aej_convert_geometry_host(int32_t *out);
AEJ_API int aej_convert_plan_host(const aej_convert_desc *desc, aej_convert_plan *out);
AEJ_API uint64_t aej_convert_workspace_bytes(aej_ctx *ctx, const aej_convert_desc *descs_host, int n);
AEJ_API int aej_convert_batch(aej_ctx *ctx, const aej_convert_desc *descs_host, int n, const uint8_t *tables_host, int n_tables,
                              const uint8_t *src, uint64_t src_bytes, uint8_t *dst, uint64_t dst_bytes, void *workspace,
                              uint64_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* AEJ_H */
