"""GPU (-m gpu): sub-batch streams created with priorities (option "stream_priorities", csrc/aej_sched.h, api_encode.hip).

With fewer than 8 hardware queues the part streams of a split call are created with stream priorities, which the HIP runtime serves from
one queue pool per level.  Nothing but the streams changes, so the outputs are bit-identical to those without priorities and equal to
the CPU oracle -- within one call cut into 2 and 4 parts, and on two contexts rotating four calls, where the colour chain crosses
streams of different priority.  With 8 queues or more no stream gets a priority.  The queue count is stated to each context
(aej_set_hw_queues) so that the tests do the same whatever the process was started with."""
import contextlib
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SETTINGS = ("YCbCr", (40, 80), (4, 64))
KEYS = ("states", "leaves", "leaf_coeff_offsets", "coeffs")


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


_refs = {}


def images_and_refs(oracle, B, H, W):
    """B small images of a shape and their oracle encodes, computed once"""
    key = (B, H, W)
    if key not in _refs:
        kinds = ("mixed", "noise", "mixed", "mixed")
        x = np.stack([oracle.synth_image(H, W, 4100 + 17 * i + W, kinds[i % 4]).astype(np.float32) / np.float32(255) for i in range(B)])
        _refs[key] = (x, [oracle.encode_image(x[b], *SETTINGS) for b in range(B)])
    return _refs[key]


def snapshot(enc, B):
    """everything a caller receives, on the host: counts, and states / leaves / offsets / coefficients of every image and layer"""
    return enc.counts_host.copy(), [[enc.layer(b, l) for l in range(3)] for b in range(B)]


def assert_equals_oracle(snap, refs, what):
    counts, layers = snap
    for b, ref in enumerate(refs):
        for l in range(3):
            got, w = layers[b][l], f"{what} image {b} layer {l}"
            assert np.array_equal(got["states"], ref[l]["states"]), w + ": states"
            assert np.array_equal(got["leaves"], ref[l]["leaves"]), w + ": leaves"
            assert np.array_equal(got["coeffs"], ref[l]["coeffs"]), w + ": coefficients"
            want = (ref[l]["coeffs"].size, len(ref[l]["leaves"]), len(ref[l]["states"]), ref[l]["root_size"])
            assert tuple(int(v) for v in counts[b, l]) == want, w + ": counts"


def assert_bit_identical(a, b, what):
    assert a[0].tobytes() == b[0].tobytes(), what + ": counts"
    for img, (la, lb) in enumerate(zip(a[1], b[1])):
        for l in range(3):
            for key in KEYS:
                assert la[l][key].dtype == lb[l][key].dtype and la[l][key].tobytes() == lb[l][key].tobytes(), f"{what} image {img} layer {l}: {key}"


@contextlib.contextmanager
def stated_queues(A, ctx, n):
    """the context schedules for n hardware queues; options, split and queue count are put back afterwards"""
    ctx.set_option("stream_priorities", 1)
    ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, n))
    try:
        yield
    finally:
        ctx.set_option("stream_priorities", 1)
        ctx.set_option("stream_priority_pattern", 3)
        ctx.set_sub_batches(0)
        ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, A.hw_queues()[0]))


def schedule_words(ctx, B, H, W):
    """aej_get_schedule_host: [queues stated, sub-batches, limited, queues the part streams spread over]"""
    buf = (ctypes.c_int32 * 4)()
    ctx.check(ctx.lib.aej_get_schedule_host(ctx.handle, B, H, W, ctypes.cast(buf, ctypes.c_void_p)))
    return [int(v) for v in buf]


@pytest.mark.parametrize("nsub", [2, 4])
def test_outputs_are_bit_identical_across_the_option(A, oracle, nsub):
    B, H, W = 8, 192, 256
    x, refs = images_and_refs(oracle, B, H, W)
    codec = A.Jpeg(A.JpegCompressionSettings(*SETTINGS))
    ctx = codec._bind()
    out = {}
    with stated_queues(A, ctx, 4):
        for mode in (0, 2):
            ctx.set_option("stream_priorities", mode)
            ctx.set_sub_batches(nsub)
            assert ctx.get_option("stream_priorities") == mode
            before = ctx.split_calls()
            enc = codec.compress_batch(x)
            assert ctx.split_calls() == before + 1, "the call was expected to run as sub-batches"
            assert ctx.get_option("priority_streams") == (nsub if mode else 0), f"stream_priorities={mode}: wrong kind of part streams"
            out[mode] = snapshot(enc, B)
            assert_equals_oracle(out[mode], refs, f"{nsub} sub-batches, stream_priorities={mode}")
    assert_bit_identical(out[0], out[2], f"{nsub} sub-batches, stream_priorities 0 against 2")


def test_outputs_are_bit_identical_on_rotating_contexts(A, oracle):
    """Two contexts, four calls (begin / end), each call in two parts: the colour stage of every part waits for the colour stage of the part
    enqueued before it -- on a stream of another priority, of this context or of the other."""
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import release_context
    from adaptive_edge_aware_jpeg_amd.jpeg import EncodedBatch
    B, H, W = 8, 128, 128
    x, refs = images_and_refs(oracle, B, H, W)
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize()
    codec = A.Jpeg(A.JpegCompressionSettings(*SETTINGS))
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    ctxs, outs, results = [], [], {0: [], 2: []}
    try:
        for s in streams:
            with torch.cuda.stream(s):
                c = codec._bind()
                plan = c.plan(B, H, W)
                ctxs.append(c)
                outs.append((c.empty((B * plan.coeff_stride,), torch.int32), c.empty((B * plan.leaf_stride, 4), torch.int32),
                             c.empty((B * plan.state_stride,), torch.uint8), c.empty((B, 3, 4), torch.int64)))
        with contextlib.ExitStack() as stack:
            for c in ctxs:
                stack.enter_context(stated_queues(A, c, 4))
            for mode in (0, 2):
                for c in ctxs:
                    c.set_option("stream_priorities", mode)
                    c.set_sub_batches(2)
                split0 = [c.split_calls() for c in ctxs]
                for i in range(4):
                    k = i % 2
                    with torch.cuda.stream(streams[k]):
                        if i >= 2:
                            codec.encode_end(ctxs[k])
                            results[mode].append(snapshot(EncodedBatch(plan, *outs[k]), B))
                            for t in outs[k]:
                                t.zero_()                      # the second call of the context must write everything again
                        codec.encode_begin(ctxs[k], xd, plan, *outs[k])
                for k in range(2):
                    with torch.cuda.stream(streams[k]):
                        codec.encode_end(ctxs[k])
                        results[mode].append(snapshot(EncodedBatch(plan, *outs[k]), B))
                assert [c.split_calls() - s0 for c, s0 in zip(ctxs, split0)] == [2, 2], "the calls were expected to run as sub-batches"
                assert [c.get_option("priority_streams") for c in ctxs] == ([2, 2] if mode else [0, 0])
                for n, snap in enumerate(results[mode]):
                    assert_equals_oracle(snap, refs, f"stream_priorities={mode}, call {n}")
        for n in range(4):
            assert_bit_identical(results[0][n], results[2][n], f"call {n}, stream_priorities 0 against 2")
    finally:
        torch.cuda.synchronize()
        for c in ctxs:
            release_context(c)


def test_priorities_only_below_eight_queues_and_the_query_says_so(A, oracle):
    B, H, W = 8, 128, 128
    x, refs = images_and_refs(oracle, B, H, W)
    codec = A.Jpeg(A.JpegCompressionSettings(*SETTINGS))
    ctx = codec._bind()
    assert ctx.get_option("stream_priorities") == 1 and ctx.get_option("stream_priority_pattern") == 3      # the defaults

    def encode_in_two_parts():
        ctx.set_sub_batches(2)
        before = ctx.split_calls()
        enc = codec.compress_batch(x)
        assert ctx.split_calls() == before + 1
        assert_equals_oracle(snapshot(enc, B), refs, "two parts")
        return ctx.get_option("priority_streams")

    with stated_queues(A, ctx, 16):
        # 16 queues: every stream has a queue of its own already -- nothing changes
        assert schedule_words(ctx, 64, 2160, 3840) == [16, 4, 0, 16]
        assert encode_in_two_parts() == 0
        # 4 queues: two levels, 8 queues for the part streams; the streams made without a priority are replaced
        ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, 4))
        w4 = schedule_words(ctx, 64, 2160, 3840)
        assert w4[0] == 4 and w4[3] == 8
        assert encode_in_two_parts() == 2
        ctx.set_option("stream_priority_pattern", 2)                  # three levels
        assert schedule_words(ctx, 64, 2160, 3840)[3] == 12
        assert encode_in_two_parts() == 2
        ctx.set_option("stream_priority_pattern", 3)
        ctx.set_option("stream_priorities", 0)                        # never
        assert schedule_words(ctx, 64, 2160, 3840)[3] == 4
        assert encode_in_two_parts() == 0
        ctx.set_option("stream_priorities", 1)
        ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, 7))           # the last count the automatic mode serves
        assert schedule_words(ctx, 64, 2160, 3840)[3] == 14
        ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, 8))
        assert schedule_words(ctx, 64, 2160, 3840)[3] == 8
        assert encode_in_two_parts() == 0
        # "always" is for A / B runs and stops at the 32 queues a process may hold
        ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, 16))
        ctx.set_option("stream_priorities", 2)
        assert schedule_words(ctx, 64, 2160, 3840)[3] == 32
        with pytest.raises(ValueError, match="32"):
            ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, 17))
        with pytest.raises(ValueError, match="32"):
            ctx.set_option("stream_priority_pattern", 2)              # 16 x 3
        assert ctx.get_option("stream_priority_pattern") == 3 and schedule_words(ctx, 64, 2160, 3840)[0] == 16      # both refusals changed nothing
        ctx.set_option("stream_priorities", 1)
        ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, 17))
        with pytest.raises(ValueError, match="32"):
            ctx.set_option("stream_priorities", 2)                    # 17 x 2
        assert ctx.get_option("stream_priorities") == 1
        with pytest.raises(ValueError, match="read-only"):
            ctx.set_option("priority_streams", 0)
        for bad in (-1, 3):
            with pytest.raises(ValueError):
                ctx.set_option("stream_priorities", bad)


def test_twenty_contexts_leave_no_streams_behind(A, oracle):
    """Every context creates two part streams with priorities and is destroyed; the process then still encodes (a leaked stream keeps its
    share of a hardware queue, and the runtime's stream and queue tables are finite)."""
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import release_context
    B, H, W = 8, 128, 128
    x, refs = images_and_refs(oracle, B, H, W)
    dev = torch.device("cuda", 0)
    codec = A.Jpeg(A.JpegCompressionSettings(*SETTINGS))
    for _ in range(20):
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):
            ctx = codec._bind()
            try:
                ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, 4))
                ctx.set_option("stream_priorities", 2)
                ctx.set_sub_batches(2)
                codec.compress_batch(x)
                assert ctx.get_option("priority_streams") == 2
            finally:
                torch.cuda.synchronize()
                release_context(ctx)
    ctx = codec._bind()
    with stated_queues(A, ctx, 4):
        ctx.set_sub_batches(2)
        enc = codec.compress_batch(x)
        assert ctx.get_option("priority_streams") == 2
        assert_equals_oracle(snapshot(enc, B), refs, "after twenty contexts")
