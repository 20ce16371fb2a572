/*
 * aej_testing.h -- TEST-ONLY entry points of libaejpeg_hip.so.  Not part of the drop-in boundary (include/aej.h): nothing a caller of
 * the reference's API would bind.  Used by tests/ to reach error paths that cannot be provoked from outside.
 */
#ifndef AEJ_TESTING_H
#define AEJ_TESTING_H

#include "aej.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The next whole-path call (aej_encode_batch / _begin) fails with AEJ_ERR_STATE right after it has enqueued stage `stage` (an AEJ_STAGE_*
 * value; -1 disarms) of its first part, i.e. with work in flight -- the error paths must drain it.  One-shot. */
AEJ_API int aej_test_fail_after_stage(aej_ctx *ctx, int stage);

/* Progressive decode stopped early, for coefficient-level comparison with tests/progressive_reference.py: the coefficients of every
 * file (int16, natural order, blocks in MCU order, file after file; coef_blocks >= the sum of mcux * mcuy * blocks_per_mcu) after the
 * scans of dependency levels < n_levels have run.  aej_test_jpegprog_coefs: on the device, arguments as aej_jpegprog_batch, coef_out a
 * device buffer.  aej_test_jpegprog_coefs_host: one file, HOST only -- the same per-thread routines (csrc/jpegprog_core.h) stepped
 * through on the CPU, segment after segment; returns the first AEJ_JPEGDEC_* status met (0 = none) or an AEJ_ERR_*. */
AEJ_API int aej_test_jpegprog_coefs(aej_ctx *ctx, const aej_jpegprog_frame *frames_host, const aej_jpegprog_scan *scans_host, int n,
                                    const uint8_t *data, uint64_t data_bytes, const int64_t *data_offsets_host, int n_levels,
                                    int16_t *coef_out, uint64_t coef_blocks, int32_t *status, void *workspace, uint64_t workspace_bytes);
AEJ_API int aej_test_jpegprog_coefs_host(const aej_jpegprog_frame *frame_host, const aej_jpegprog_scan *scans_host, const uint8_t *file_host,
                                         uint64_t nbytes, int n_levels, int16_t *coef_out_host, uint64_t coef_blocks);

/* One progressive scan over given quantised coefficients (int16 [n_blocks][64] in zigzag order, |value| <= 2047; the blocks are one
 * component in scan order), for the cases pixels cannot reach: Ss..Se the band (0-0 a DC scan), Ah / Al the successive approximation
 * (Ah is 0 or Al + 1).  Writes the scan's bytes -- coded under the optimal table of its own symbols, padded with 1-bits, 0xFF stuffed --
 * to out_host, their number to *out_len_host, the count of every symbol to counts_host[257] and to cuts_host[2] how many end-of-band
 * runs were cut at 0x7FFF blocks and how many at more than 937 deferred bits.  AEJ_ERR_CAPACITY (with *out_len_host set) when capacity
 * is too small.  aej_test_jfif_prog_scan_host: HOST only, the per-block and partition routines of csrc/jfif_prog_core.h stepped through
 * on the CPU.  aej_test_jfif_prog_scan: the kernels of csrc/jfifprog.hip over the same coefficients (all pointers are host memory). */
AEJ_API int aej_test_jfif_prog_scan_host(const int16_t *coefs_host, int64_t n_blocks, int Ss, int Se, int Ah, int Al, uint8_t *out_host,
                                         uint64_t capacity, uint64_t *out_len_host, int64_t *counts_host, int64_t *cuts_host);
AEJ_API int aej_test_jfif_prog_scan(aej_ctx *ctx, const int16_t *coefs_host, int64_t n_blocks, int Ss, int Se, int Ah, int Al, uint8_t *out_host,
                                    uint64_t capacity, uint64_t *out_len_host, int64_t *counts_host, int64_t *cuts_host);

/* The baseline (sequential, interleaved) scan of given quantised coefficients, HOST only: the per-block coder, DC predictor, interval
 * placement, padding and stuffing of csrc/jfif_prog_core.h, jfif_restart_core.h and jfif_stream_core.h -- the text the kernels of
 * csrc/jfif.hip run -- stepped through on the CPU.  coefs_host: int16 [n_mcu * blocks per MCU][64], zigzag order, blocks in MCU order
 * (hs * vs luma blocks in raster order, then Cb, Cr), |value| <= 2047 -- the layout aej_jfif_many_coefs_host returns.  hs, vs: the luma
 * sampling factors, 1 or 2 each (1 x 2 is 4:4:0); ncomp 3, or 1 (grey: one block per MCU).  restart_interval: MCUs per restart
 * interval, 0 for none (an interval requires optimize, as in the encoders).  optimize 0: the Annex K tables; 1: the optimal tables of
 * the scan's own symbols.  hist_host gets the symbol counts [4][257] (DC luma, AC luma, DC chroma, AC chroma; grey: the first two),
 * out_host the entropy-coded segment -- padded with 1-bits, 0xFF stuffed, RSTn markers included, without EOI -- and *out_len_host its
 * length.  AEJ_ERR_ARG for a null pointer, a coefficient out of range, a bad layout or interval; AEJ_ERR_CAPACITY (with *out_len_host
 * set) when capacity is too small.  (Addition: the ABI version stays 3.) */
AEJ_API int aej_test_jfif_seq_scan_host(const int16_t *coefs_host, int64_t n_mcu, int hs, int vs, int ncomp, int restart_interval, int optimize,
                                        int64_t *hist_host, uint8_t *out_host, uint64_t capacity, uint64_t *out_len_host);

/* One block through the reduced inverse DCT of a scaled decode (aej_jpegdec_batch_scaled), HOST only: coef_host [64] quantised
 * coefficients and qt_host [64] quantisers, both in natural order; size 1, 2 or 4 (AEJ_ERR_ARG otherwise); out_host gets size x size
 * samples, row after row -- computed by the function of csrc/jpegdec_core.h that the kernel calls (jd_idct_sized). */
AEJ_API int aej_test_jpegdec_idct_host(const int16_t *coef_host, const uint16_t *qt_host, int size, uint8_t *out_host);

/* The chroma up-sampling rule of every JPEG reconstruction kernel (jd_up_chroma of csrc/jpegdec_core.h, the function the kernels call),
 * HOST only.  part_host: a chroma plane or a part of one with row stride `stride`, in which the plane's sample (row, column) is
 * part_host[row * stride + column - off]; wc x hc: the plane's real samples; uh, uv in 1, 2: the factors to up-sample by; fancy: 0 beside
 * a 1 x 1 IDCT (plain replication).  out_host gets the samples of the output pixels [y0, y1) x [x0, x1) of the uv * hc x uh * wc
 * up-sampled plane, row after row.  Only the samples the rule reads for those pixels are read: the part has to hold no others.
 * AEJ_ERR_ARG for a null pointer, a factor other than 1 and 2, uh = uv = 2 without fancy (no decoder uses it), or a rectangle that is
 * not inside the up-sampled plane. */
AEJ_API int aej_test_jpeg_upsample_host(const uint8_t *part_host, int64_t stride, int64_t off, int uh, int uv, int fancy, int wc, int hc,
                                        int x0, int y0, int x1, int y1, uint8_t *out_host);

/* The baseline entropy decode of one file, HOST only, for coefficient-level comparison with tests/scaled_decode_reference.py: desc_host as
 * aej_jpegdec_parse_host wrote it for file_host (one or three components).  The scan is un-stuffed with the byte classifier the kernels
 * use (jd_byte_class), and each restart segment is then decoded from its first bit to its last by the per-thread routine of
 * csrc/jpegdec_core.h (jd_run, jd_huff).  coef_out_host gets int16 [mcux * mcuy * blocks_per_mcu][64], natural order, blocks in MCU order
 * (coef_blocks: its capacity in blocks).  Returns the first AEJ_JPEGDEC_* status met (0 = none) or an AEJ_ERR_*. */
AEJ_API int aej_test_jpegdec_coefs_host(const aej_jpegdec_desc *desc_host, const uint8_t *file_host, uint64_t nbytes, int16_t *coef_out_host,
                                        uint64_t coef_blocks);

/* The per-pixel colour rules of the four-component / RGB-coded reconstruction (aej_jpegdec_batch_adobe), HOST only: samples4_host [n][4]
 * up-sampled samples of one pixel each, colour AEJ_JPEG_RGB, _CMYK or _YCCK, components 3 or 4 (4: not with _RGB) -> out_host
 * [n][components], computed by the functions of csrc/jpegdec_core.h that the kernel calls (jd_adobe_pixel: jd_cmyk_pixel, jd_ycck_pixel,
 * jd_cmyk_rgb).  AEJ_ERR_ARG for anything else. */
AEJ_API int aej_test_jpeg_adobe_pixels_host(const uint8_t *samples4_host, int64_t n, int colour, int components, uint8_t *out_host);

#ifdef __cplusplus
}
#endif
#endif /* AEJ_TESTING_H */
