// aej_ctx.h -- private to the host translation units of the C ABI (api.hip and its api_*.hip siblings; not installed beside include/aej.h):
// the context, the error and entry helpers every entry point starts with, the workspace carver and what crosses a file boundary.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/aej.h"
#include "../../include/aej_testing.h"
#include "aej_common.h"
#include "aej_launch.h"
#include "aej_sched.h"

struct aej_pending;
constexpr int kFlagWords = 16;       // [0] quadtree overflow flag, [1] entries that went through the hysteresis work queue (diagnostic)
constexpr int kMaxDevices = 64;      // aej_create refuses device >= kMaxDevices: the per-device chain state of api_encode.hip is indexed by it
struct aej_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool has_settings = false;
    int space = 0, bmin = 0, bmax = 0, nsizes = 0;
    void *tables = nullptr;            // one device allocation holding every table below
    const float *d_D[aej::kMaxSizes] = {};
    const int *d_zzinv[aej::kMaxSizes] = {};
    const int *d_zz[aej::kMaxSizes] = {};
    const int *d_qm[3][aej::kMaxSizes] = {};
    int *d_check = nullptr;            // device word in `tables`: aej_requantise_batch's "leaf tables / quantisers do not fit" flag
    const float *d_space_w = nullptr, *d_color_w = nullptr;
    float *d_bilateral = nullptr;      // [16 + 256] space / colour weights of the bilateral filter (own allocation: aej_set_canny_params rebuilds it)
    aej_canny_params canny = { 0.10, 0.30, 0.75, 75.0, 75.0, 1 };     // edge_detection.py:31-40 defaults
    int *h_flag = nullptr;             // pinned host words for counter read-backs (kFlagWords)
    long long last_hyst_queued = 0;    // tiles that went through the hysteresis work queue in the last whole-path call (diagnostic)
    bool capturing = false;            // the stream is being captured into a hipGraph: kernel nodes only (zero-fill by kernel, no copies)
    long long n_encode_calls = 0;      // aej_get_hysteresis_stats
    // launch-latency path (aej_set_graph_mode): the whole launch sequence of one encode call captured in a hipGraph,
    // keyed by everything its kernel arguments depend on, and replayed on a private stream
    int graph_mode = 0;                // 0 off (default: measured slower than eager launches), 1 automatic (small batches only), 2 always when possible
    hipStream_t gstream = nullptr;
    hipEvent_t gevent = nullptr;
    struct GraphEntry {
        const void *rgb; void *coeffs, *leaves, *states, *counts, *dct, *ws;
        int batch, H, W, in_u8;
        hipGraphExec_t exec;
        unsigned long long last_use;
    };
    std::vector<GraphEntry> graphs;
    unsigned long long graph_clock = 0, n_graph_launches = 0, n_graph_captures = 0;
    // sub-batch pipelining (aej_set_sub_batches): a large call is cut into sub-batches that run the whole chain on private streams,
    // each one stage behind the previous, so that HBM-bound stages (colour planes, DCT) of one run beside the issue-bound stages
    // (blur, Sobel / NMS, quadtree) of another
    int sub_mode = 0;                  // 0 automatic, 1 never split, n > 1 split into n (when the batch allows)
    int hw_queues = 4;                 // hardware queues the runtime maps streams onto, as the host states it (aej_set_hw_queues; HIP's default 4): streams beyond it share queues
    int fail_after = -1;               // aej_test_fail_after_stage (test instrumentation)
    static constexpr int kMaxSub = 8;
    int dct_crowded = 0;               // this call runs as sub-batches or beside other calls: DCT kernels that share CUs (aej_launch.h DctArgs::crowded)
    hipStream_t sub_stream[kMaxSub] = {};
    // stream priorities (aej_sched.h): with fewer than 8 hardware queues the part streams are created with priorities, so that the
    // runtime serves them from one queue pool per level instead of the one pool the caller's streams have filled already
    int stream_priorities = 1;         // aej_set_option "stream_priorities": 0 never, 1 automatic (hw_queues < 8), 2 always (A / B)
    int stream_priority_pattern = aej::kDefaultPriorityPattern;      // aej_set_option "stream_priority_pattern": the levels dealt (aej_sched.h)
    int sub_stream_key = 0;            // what the existing part streams were created under: 0 no priorities, 1 + pattern otherwise
    int n_priority_streams = 0;        // aej_get_option "priority_streams": part streams this context holds that were created with a priority
    hipEvent_t sub_color_done[kMaxSub] = {}, sub_in = nullptr;
    int *sub_flag[kMaxSub] = {};       // pinned read-back words per sub-batch (layout of h_flag)
    long long n_split_calls = 0;
    int sub_chain = -1;                // colour stages wait for a stage of the previous part (g_last_color_done): 1 its colour stage, 2 its blur, 3 its
                                       // Sobel / NMS; 0 no staggering; -1 (default) = 1, between the sub-batches of one call and between whole calls on
                                       // rotating contexts alike (round 4, profiles/r04_sched_sweep_final.txt: unsplit 64 x 4K calls on three contexts
                                       // 6.01 / 7.58 / 7.49 / 6.22 ms for 1 / 2 / 3 / 0; 6 x 4K 0.66 / 0.75 / 0.85 / 0.68; round 3's kernels had preferred 2
                                       // between whole calls).  aej_set_option "sub_chain" overrides.
    int chain_hook = 0;                // run_canny_chain publishes chain_event after the blur (2) / Sobel (3) stage of the part being enqueued
    hipEvent_t chain_event = nullptr;
    aej::Tuning tune;                  // aej_set_option: kernel / launch-shape choices (nothing in the library reads the environment)
    int qt_chunk_launches = 0;         // aej_get_option "qt_chunk_launches": quadtree stages the chunk-run kernels have served (aej_set_option resets it)
    int jd_subseq_bits = 2048;         // aej_set_option "jpegdec_subseq_bits": subsequence length of aej_jpegdec_batch's Huffman decode
    long long jd_sync_rounds = 0;      // sync rounds of the last aej_jpegdec_batch
    long long jd_box_stats[3] = { 0, 0, 0 };      // aej_jpegdec_box_stats: restart segments, those decoded, coefficient blocks stored of the last aej_jpegdec_batch_box with a box
    struct aej_pending *pending = nullptr;     // the call between aej_encode_batch_begin and aej_encode_batch_end
    // optional stage timing (aej_set_profiling): events on ctx->stream around each stage of aej_encode_batch
    bool profiling = false;
    hipEvent_t ev[24] = {};
    int ev_stage[24] = {};
    int n_ev = 0;
    float stage_ms[AEJ_N_STAGES] = {};
};

namespace aej {
inline int fail(aej_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}
int hip_fail(aej_ctx *ctx, hipError_t e, const char *expr, const char *file, int line);      // api.hip (AEJ_HIP_CHECK)

inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

// ---- workspace carving: every piece starts on a 256-byte boundary; a null base only measures ----------------------------------
struct Carver {
    char *base;
    unsigned long long off = 0;
    explicit Carver(void *p) : base(static_cast<char *>(p)) {}
    template <typename T> T *take(long long n)
    {
        off = (off + 255) & ~255ull;
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += (unsigned long long)n * sizeof(T);
        return p;
    }
    unsigned long long bytes() const { return (off + 255) & ~255ull; }      // the workspace size: whole 256-byte pieces
};

}  // namespace aej

// ---- api.hip: constant tables and geometry ---------------------------------------------------------------------------------------
extern const double kMid[7][3], kScale[7][3];
int check_encode_args(aej_ctx *ctx, int batch, int H, int W);
// The largest image or plane the codec takes: 2^29 pixels (H x W of one image; sides at most 65535).  Up to there pixel and element
// indices fit `int` and the byte offsets of a float32 plane `unsigned` (the kernels' 32-bit quantities: LeafWork::coef, the leaves'
// coefficient offsets, the strip kernel's plane offsets); only the float32 RGB input, 12 bytes a pixel, needs 64-bit addressing.
constexpr long long kMaxImagePixels = 1ll << 29;
int check_image_size(aej_ctx *ctx, const char *what, int H, int W);      // AEJ_ERR_UNSUPPORTED above either limit (make_geom and the stage entries)
int make_geom(aej_ctx *ctx, int space, int B, int H, int W, aej::Geom &g);
void make_plane_geom(int H, int W, aej::Geom &g);
int make_qtgeom(aej_ctx *ctx, const aej::Geom &g, int bmin, int bmax, aej::QtGeom &q, bool allow_small_root = false);
int make_geoms(aej_ctx *ctx, int batch, int H, int W, aej::Geom &g, aej::QtGeom &q);      // both, for the bound settings
long long big_scratch_floats(int bmax);

// ---- api_encode.hip: the call in flight, the captured graphs and the per-device chain state ---------------------------------------
bool call_in_flight(const aej_ctx *ctx);
void drop_graphs(aej_ctx *ctx);
void release_encode_state(aej_ctx *ctx);      // aej_destroy: drains a call in flight, frees aej_pending and the graphs, forgets the context's chain events

// ---- the guards of the entry points ------------------------------------------------------------------------------------------------
#define AEJ_TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)      // a step's error code is the entry's

inline int refuse_in_flight(aej_ctx *ctx, const char *fn)
{
    return call_in_flight(ctx) ? aej::fail(ctx, AEJ_ERR_STATE, "%s between aej_encode_batch_begin and aej_encode_batch_end", fn) : 0;
}
inline int enter(aej_ctx *ctx, const char *fn) { return ctx ? refuse_in_flight(ctx, fn) : AEJ_ERR_ARG; }
// (kept apart from enter(): an entry binds its device after it has validated its arguments, so that a call with two things wrong
// reports the one it always reported)
inline int bind_device(aej_ctx *ctx) { AEJ_HIP_CHECK(hipSetDevice(ctx->device)); return 0; }
inline int check_workspace(aej_ctx *ctx, unsigned long long need, uint64_t got)
{
    return need > got ? aej::fail(ctx, AEJ_ERR_CAPACITY, "workspace too small: need %llu bytes, got %llu", need, (unsigned long long)got) : 0;
}
inline int null_buffer(aej_ctx *ctx, const char *fn = nullptr)
{
    return fn ? aej::fail(ctx, AEJ_ERR_ARG, "%s: NULL buffer", fn) : aej::fail(ctx, AEJ_ERR_ARG, "NULL buffer");
}
// the span check of a packed-image entry (aej_spans.h) as its refusal: what the call reads lies in the input, what it writes in the
// output of dst_elements elements of dst_unit bytes, and no source meets the output
inline int check_spans(aej_ctx *ctx, const char *fn, const aej::Spans &spans, const void *src, uint64_t src_bytes, const void *dst,
                       uint64_t dst_elements, uint64_t dst_unit = 1)
{
    static const char *const what[] = { nullptr, "source outside the input", "image outside the output", "source inside the output" };
    const aej::SpanVerdict v = aej::span_fault(spans, (uintptr_t)src, src_bytes, (uintptr_t)dst, dst_elements, dst_unit);
    return v.fault ? aej::fail(ctx, AEJ_ERR_ARG, "%s: image %d: %s", fn, v.image, what[v.fault]) : 0;
}
// the plan of a packed-image call, or the refusal of its first bad descriptor (fn NULL: quietly, for the size query).
// plan(&bad, &why) is the entry's own plan function: -> 0, or its error code with `why` and, where one image is at fault, `bad`
template <class Plan>
inline int plan_or_refuse(aej_ctx *ctx, const char *fn, int n, Plan plan)
{
    if (n < 1) return fn ? aej::fail(ctx, AEJ_ERR_ARG, "%s: no images", fn) : AEJ_ERR_ARG;
    const char *why = nullptr;
    int bad = -1;
    const int code = plan(&bad, &why);
    if (!code || !fn) return code;
    return bad >= 0 ? aej::fail(ctx, code, "%s: image %d: %s", fn, bad, why) : aej::fail(ctx, code, "%s: %s", fn, why);
}
// a parser's message into the caller's buffer (truncated, always terminated)
inline void copy_msg(const std::string &m, char *msg, int msg_capacity)
{
    if (!msg || msg_capacity < 1) return;
    const size_t k = std::min(m.size(), (size_t)msg_capacity - 1);
    memcpy(msg, m.data(), k);
    msg[k] = 0;
}
