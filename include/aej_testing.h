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

#ifdef __cplusplus
}
#endif
#endif /* AEJ_TESTING_H */
