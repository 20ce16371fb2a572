"""GPU (-m gpu): every entry of the Python layer with poisoned workspace, output, status and staging memory (tests/poisoned_memory.py).

The rest of the suite controls the values that go INTO a call; this file controls what the memory the call is handed held BEFORE it.
Each row below is one subsystem at the smallest cases of its own test module (imported from there, not copied), run under the byte
patterns 0x00 (control), 0x01 (every counter 16843009, every float 2.4e-38) and 0xFF (ints -1, floats NaN, flags set), and compared
with that module's independent reference -- never with an unpoisoned run of the library, except for the two GPU-entropy rows, whose
streams have no outside byte reference: they must round-trip to the reference AND equal the bytes of the 0x00 run.  Every public call
goes through `Poison.call`, which arms the harness (the first workspace() / pinned() of the call poisons the whole reused buffer) and
asserts that the call really drew poisoned memory.  `test_call_order` then runs all rows in two seeded orders on one context under
0x01, so that a small call runs in the leftovers of a large one from another subsystem.

DESIGN.md section "What a call may assume about its memory" is the audit these tests hold the code to."""
import contextlib
import ctypes
import functools
import io
import os
import zlib

import numpy as np
import pytest

import poisoned_memory as PM

pytestmark = pytest.mark.gpu
PATTERN_IDS = [f"0x{b:02X}" for b in PM.PATTERNS]
ROWS = {}


def row(name):
    def deco(fn):
        assert name not in ROWS
        ROWS[name] = fn
        return fn
    return deco


class Env:
    def __init__(self, A, oracle):
        import torch
        from adaptive_edge_aware_jpeg_amd import _lib
        self.A, self.oracle, self.torch, self.lib = A, oracle, torch, _lib
        self.ctx = _lib.get_context()


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as A
    return Env(A, oracle)


# ---------------------------------------------------------------------------------------------------------------- the harness itself
def test_harness_self_test(env):
    """No library kernel: what the three replaced methods return holds the pattern over its whole length, and they are restored."""
    t, ctx = env.torch, env.ctx
    plain = {k: getattr(ctx, k).__func__ for k in ("empty", "workspace", "pinned")}
    with PM.poisoned(ctx, 0x01) as p:
        e = ctx.empty((4,), t.int32)
        assert e.is_cuda and e.cpu().tolist() == [0x01010101] * 4
        odd = ctx.empty((3, 7), t.uint8)                      # 21 bytes: not a multiple of 4
        assert (odd.cpu() == 1).all()
        assert 0 < float(ctx.empty((1,), t.float32).cpu()[0]) < 3e-38
        p.arm()
        ws = ctx.workspace(1000)
        assert ws.numel() >= 1000 and bool((ws == 1).all()) and p.workspace_fills == 1
        ws.fill_(7)
        assert ctx.workspace(10) is ws and bool((ws == 7).all()), "not armed: a call's own state in the workspace is kept"
        bigger = ws.numel() + 4097                            # a forced reallocation: poisoned although nobody armed
        ws2 = ctx.workspace(bigger)
        assert ws2.numel() == bigger and ws2.data_ptr() != 0 and bool((ws2 == 1).all()) and p.workspace_fills == 2
        p.arm()
        assert bool((ctx.workspace(16) == 1).all()) and p.workspace_fills == 3
        host = ctx.pinned(100)
        assert host.is_pinned() and bool((host == 1).all()) and p.pinned_fills == 1
        assert p.bytes >= 16 + 21 + 4 + ws.numel() + 2 * bigger + host.numel()
    with PM.poisoned(ctx, 0xFF) as p:
        assert ctx.empty((2,), t.int64).cpu().tolist() == [-1, -1] and bool(t.isnan(ctx.empty((3,), t.float64)).all())
    assert {k: getattr(ctx, k).__func__ for k in plain} == plain and not any(k in vars(ctx) for k in plain)


# ---------------------------------------------------------------------------------------------------------------- the codec's encode side
def _u8_levels(x):
    u8 = np.rint(x * np.float32(255)).astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32) / np.float32(255), x), "the test images are 8-bit levels"
    return u8


@contextlib.contextmanager
def _option(ctx, name, value):
    old = ctx.get_option(name)
    ctx.set_option(name, value)
    try:
        yield
    finally:
        ctx.set_option(name, old)


ENCODE_RANGES = ((4, 64), (4, 128), (8, 256), (32, 32))
ENCODE_SHAPES = ((136, 260), (72, 200), (9, 13))


@row("compress_batch")
def _compress_batch(e, p):
    """Jpeg.compress_batch, float and uint8 ingest, B = 3: the four block ranges (no pyramid and no fill in front of the quadtree; the
    upper pyramid and its fill; the general kernels) with both quadtree kernel sets forced where the chunk-run set can serve"""
    import test_gpu_quadtree_chunks as TQ
    for blocks in ENCODE_RANGES:
        codec = e.A.Jpeg(e.A.JpegCompressionSettings("YCbCr", (40, 80), blocks))
        for H, W in ENCODE_SHAPES:
            if blocks[0] > 16 and H < 16:
                continue                                                # a 4 x 6 chroma layer (root 8) cannot hold a block of 32: the oracle refuses it
            x, refs = TQ.oracle_refs(e.oracle, H, W, blocks)
            for chunks in (1, 0):
                ctx = codec._bind()
                with _option(ctx, "qt_chunks", chunks):
                    for batch in (x, _u8_levels(x)):
                        before = TQ.chunk_launches(ctx)
                        enc = p.call(codec.compress_batch, batch)
                        served = TQ.chunk_launches(ctx) > before
                        assert served == (chunks == 1 and blocks[0] == 4 and enc.plan.root_size[2] >= 64), (blocks, H, W, chunks)
                        for b in range(3):
                            TQ.check_against(enc, b, refs[b], f"{H}x{W} blocks {blocks} qt_chunks={chunks} {batch.dtype}")


@row("sub_batches")
def _sub_batches(e, p):
    """aej_set_sub_batches: one call of B = 5 cut 2 + 2 + 1 over slices of the one workspace, float and uint8; and the same batch uncut,
    with both quadtree kernel sets -- more than four images in one launch take the 256-thread scan kernels, which B = 3 never does"""
    import test_gpu_quadtree_chunks as TQ
    from test_gpu_full_size import check_image
    H, W, blocks = 72, 200, (4, 64)
    x3, refs = TQ.oracle_refs(e.oracle, H, W, blocks)
    x = np.concatenate([x3, x3[1:]])                                    # B = 5
    codec = e.A.Jpeg(e.A.JpegCompressionSettings("YCbCr", (40, 80), blocks))
    ctx = codec._bind()
    try:
        ctx.set_sub_batches(1)                                          # never split
        for chunks in (1, 0):
            with _option(ctx, "qt_chunks", chunks):
                c0, before = ctx.split_calls(), TQ.chunk_launches(ctx)
                enc = p.call(codec.compress_batch, x)
                assert ctx.split_calls() == c0 and (TQ.chunk_launches(ctx) > before) == (chunks == 1)
                for b in range(5):
                    check_image(enc, b, refs[b if b < 3 else b - 2], f"B = 5 uncut, qt_chunks={chunks}, image {b}")
        ctx.set_sub_batches(3)
        for batch in (x, _u8_levels(x)):
            c0 = ctx.split_calls()
            enc = p.call(codec.compress_batch, batch)
            assert ctx.split_calls() == c0 + 1, "the call must have been cut into sub-batches"
            for b in range(5):
                check_image(enc, b, refs[b if b < 3 else b - 2], f"3 sub-batches of 5, image {b}, {batch.dtype}")
    finally:
        ctx.set_sub_batches(0)


@row("compress_batches")
def _compress_batches(e, p):
    """Jpeg.compress_batches(in_flight=4): begin / end pairs on four private streams, each with a context and workspace of its own --
    all four poisoned with this row's pattern; slot 0 serves two batches, the second in the leftovers of the first"""
    import test_gpu_quadtree_chunks as TQ
    from test_gpu_full_size import check_image
    t = e.torch
    H, W, blocks = 72, 200, (4, 64)
    x, refs = TQ.oracle_refs(e.oracle, H, W, blocks)
    codec = _pipe_codec(e)
    batches = [x[[i % 3, (i + 1) % 3]] for i in range(5)]
    with contextlib.ExitStack() as stack:
        subs = []
        for s in codec._pipe_streams[:4]:
            with t.cuda.stream(s):
                subs.append(stack.enter_context(PM.poisoned(e.lib.get_context(), p.byte)))
        for q in subs:
            q.arm()
        got = list(codec.compress_batches(batches, in_flight=4))
        for q in subs:
            assert q.workspace_fills >= 1 and q.empties >= 4, "every private context must have drawn poisoned memory"
        assert subs[0].empties >= 8
        for q in subs:                                                  # the row's draws, booked where the tests look
            p.empties, p.workspace_fills, p.bytes = p.empties + q.empties, p.workspace_fills + q.workspace_fills, p.bytes + q.bytes
    assert len(got) == 5
    for i, enc in enumerate(got):
        for b in range(2):
            check_image(enc, b, refs[(i + b) % 3], f"batch {i} image {b}")
    p.calls += 1


@functools.lru_cache(maxsize=None)
def _pipe_codec_cached(A):
    return A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), (4, 64)))


def _pipe_codec(e):
    """one codec for every compress_batches row: its four private streams (and so their contexts) are made once"""
    codec = _pipe_codec_cached(e.A)
    if len(codec.__dict__.get("_pipe_streams", [])) < 4:
        x = np.zeros((1, 8, 8, 3), np.float32)
        list(codec.compress_batches([x] * 4, in_flight=4))
    return codec


@row("graph_mode_2")
def _graph_replay(e, p):
    """graph mode 2: six calls into the same buffers, workspace and outputs poisoned again before every call (the replays included);
    one capture, at least three launches"""
    import test_gpu_quadtree_chunks as TQ
    from test_gpu_full_size import check_image
    from adaptive_edge_aware_jpeg_amd.jpeg import EncodedBatch
    t = e.torch
    H, W, blocks = 72, 200, (4, 64)
    x3, refs = TQ.oracle_refs(e.oracle, H, W, blocks)
    codec = e.A.Jpeg(e.A.JpegCompressionSettings("YCbCr", (40, 80), blocks))
    ctx = codec._bind()
    ctx.set_graph_mode(2)
    try:
        plan = ctx.plan(1, H, W)
        out = (ctx.empty((plan.coeff_stride,), t.int32), ctx.empty((plan.leaf_stride, 4), t.int32),
               ctx.empty((plan.state_stride,), t.uint8), ctx.empty((1, 3, 4), t.int64))
        x = ctx.to_device(x3[:1], t.float32).clone()
        g0 = ctx.graph_stats()
        for it in range(6):
            which = it % 3
            x.copy_(ctx.to_device(x3[which:which + 1], t.float32))      # same input buffer, new contents
            for o in out:
                PM.fill_bytes(o, p.byte)
            p.call(codec.encode_into, ctx, x, plan, *out, _draws=("workspace_fills",))
            check_image(EncodedBatch(plan, *out), 0, refs[which], f"graph call {it}")
        g1 = ctx.graph_stats()
        assert g1["captures"] - g0["captures"] == 1 and g1["launches"] - g0["launches"] >= 3, (g0, g1)
    finally:
        ctx.set_graph_mode(0)


# ---------------------------------------------------------------------------------------------------------------- edges and quadtree
def _serpentine():
    """test_gpu_parity.test_hysteresis_serpentine_across_one_tile_border's plane: faint lines joined at alternating ends, which cross
    the border between two tile columns 72 times from a handful of strong seeds"""
    H, W = 448, 128
    plane = np.repeat(np.linspace(0.0, 0.2, H, dtype=np.float32)[:, None], W, axis=1).copy()
    amp = 0.036 + (0.05 - 0.036) * np.arange(W, dtype=np.float32) / W
    for k, y in enumerate(range(8, H - 8, 6)):
        plane[y, 6:W - 6] += amp[6:W - 6]
        x = W - 7 if k % 2 == 0 else 6
        plane[y:y + 6, x] += amp[x]
    return plane


@functools.lru_cache(maxsize=None)
def _serpentine_ref(oracle):
    plane = _serpentine()
    edge, stages, thr = oracle.edge_pipeline(plane, return_stages=True)
    _, nms = oracle.canny(stages[3], thr[0], thr[1], return_nms=True)
    assert int(edge.sum()) > int((nms == 2).sum()) + 3000, "the pattern must depend on hysteresis propagation"
    return plane, edge


@row("edge_detection")
def _edges(e, p):
    """EdgeDetection.canny with stages on the edge module's smallest shapes (float64 restatement of every stage), and the long
    hysteresis chain (oracle): the hysteresis flags, work queue and histograms live in the cleared part of the workspace"""
    import edge_reference as E
    import test_gpu_edge_reference as TE
    from test_oracle_edge_reference import PARAMS, SHAPES
    for name in ("tiny_2x2", "below4_3x50", "exact_64x64", "pad_both_97x131", "pad_cols_only_96x131", "pad_rows_only_97x132"):
        H, W = SHAPES[name]
        plane = E.test_plane(H, W, H * 7 + W)
        edge, st, thr = p.call(TE.run, e.A, plane, PARAMS["default-L2"])
        assert np.array_equal(st[0], (plane * np.float32(255)).astype(np.uint8))
        E.check_stages(st, edge, thr, PARAMS["default-L2"], label=name)
    plane, want = _serpentine_ref(e.oracle)
    assert np.array_equal(p.call(e.A.EdgeDetection.canny, plane).astype(np.uint8), want)


@functools.lru_cache(maxsize=None)
def _quadtree_refs(oracle):
    import test_gpu_quadtree_chunks as TQ
    out = []
    for H, W in ((4, 4), (5, 7), (24, 40), (72, 200)):
        for name, edge in TQ.edge_maps(H, W).items():
            for mn, mx in TQ.BLOCKS:
                out.append((f"{H}x{W} blocks {mn}-{mx} edges '{name}'", edge, mn, mx, oracle.quadtree(edge, mn, mx)))
    return out


@row("quadtree")
def _quadtree(e, p):
    """QuadTree alone (aej_quadtree): chunk-run kernels with and without the upper pyramid, general kernels"""
    import test_gpu_quadtree_chunks as TQ
    served = 0
    for what, edge, mn, mx, (lo, so, ro) in _quadtree_refs(e.oracle):
        before = TQ.chunk_launches(e.ctx)
        qt = p.call(e.A.QuadTree, edge, max_size=mx, min_size=mn)
        served += TQ.chunk_launches(e.ctx) - before
        assert qt.root_size == ro, what
        assert np.array_equal(qt._states, so), what + ": states"
        assert np.array_equal(qt._leaves[:, :3], lo), what + ": leaves"
        offs = np.concatenate([[0], np.cumsum(lo[:, 2].astype(np.int64) ** 2)[:-1]]) if len(lo) else np.zeros(0, np.int64)
        assert np.array_equal(qt._leaves[:, 3], offs), what + ": coefficient offsets"
    assert served > 0, "the chunk-run kernels must have served the 72 x 200 cases"


# ---------------------------------------------------------------------------------------------------------------- the codec's decode side
@row("decompress_batch")
def _decode_geometry(e, p):
    """Jpeg.decompress_batch on test_gpu_decode_reference's geometry cases: patterned coefficients written over a poisoned encode (what
    lies beyond every count stays poison), float64 decode reference; bit-exact against the oracle where the space has no matrix inverse"""
    import decode_reference as R
    import test_gpu_decode_reference as TD
    for case in TD.GEOMETRY:
        space, H, W = case
        br = (2, 16)
        codec = e.A.Jpeg(e.A.JpegCompressionSettings(space, (40, 80), br))
        enc = p.call(codec.compress_batch, TD.busy_corner(e.oracle, H, W, 4, 1.0, 1.0)[None])
        layers = TD.overwrite(e.A, codec, enc, 4, amp=(100.0, 60.0, 60.0))[0]
        got = p.call(codec.decompress_batch, enc).cpu().numpy()[0]
        if space in R.MATRIX_SPACES:
            ref, bound = R.decode(layers, space, H, W)
            R.assert_within(got, ref, bound, TD._geom_id(case))
        else:
            stream = [dict(root_size=enc.layer(0, l)["root_size"], states=enc.layer(0, l)["states"], coeffs=layers[l]["coeffs"]) for l in range(3)]
            assert np.array_equal(got, e.oracle.decode_image(e.oracle.write_ajpg(stream, H, W, space, (40, 80), br, ".png")), equal_nan=True), case


@functools.lru_cache(maxsize=None)
def _ajpg_fixtures(oracle):
    from conftest import GOLDEN
    out = []
    for name in ("crop_ycbcr_4_64", "house_ycocgr_2_32_q30_90"):
        with open(os.path.join(GOLDEN, name + ".ajpg"), "rb") as f:
            data = f.read()
        out.append((name, data, oracle.decode_image(data)))
    return out


@row("decompress_many")
def _decompress_many(e, p):
    """Jpeg.decompress_many with the inflate on the GPU and on the host: staging, stream descriptors, status words, leaf tables"""
    for name, data, want in _ajpg_fixtures(e.oracle):
        for entropy in ("gpu", "host"):
            for n in (1, 3):
                got = p.call(e.A.Jpeg(e.A.JpegCompressionSettings()).decompress_many, [data] * n, entropy=entropy,
                             _draws=("workspace_fills", "empties", "pinned_fills")).cpu().numpy()
                assert got.shape == (n,) + want.shape
                for b in range(n):
                    assert np.array_equal(got[b], want), (name, entropy, n, b)


def _unpack_ajpg(e, data):
    from adaptive_edge_aware_jpeg_amd.jpeg import parse_container
    meta, layers = parse_container(data)
    out = []
    for n_states, root, packed, stream in layers:
        pk = np.frombuffer(packed, np.uint8)
        st = np.stack([(pk >> 6) & 3, (pk >> 4) & 3, (pk >> 2) & 3, pk & 3], 1).reshape(-1)
        assert not st[n_states:].any(), "the bits behind a layer's last symbol are zero"
        out.append(dict(root_size=root, states=st[:n_states], coeffs=np.frombuffer(zlib.decompress(bytes(stream)), np.int32)))
    return meta, out


_CONTROL = {}


def _control(e, key, make):
    """the bytes of the 0x00 run of a GPU-entropy row (made under poisoned(ctx, 0x00), once)"""
    if key not in _CONTROL:
        with PM.poisoned(e.ctx, 0x00) as p0:
            _CONTROL[key] = make(p0)
    return _CONTROL[key]


@row("compress_many_gpu_entropy")
def _compress_many_gpu(e, p):
    """Jpeg.compress_many(entropy="gpu" / "gpu-fixed"): the deflate workspace (hash chains, tokens, error word), the histogram and the
    padded stream rows.  zlib reads every stream back to the oracle's coefficients; the bytes equal the 0x00 run's"""
    import test_gpu_quadtree_chunks as TQ
    H, W, blocks = 136, 260, (4, 64)
    x, refs = TQ.oracle_refs(e.oracle, H, W, blocks)
    codec = e.A.Jpeg(e.A.JpegCompressionSettings("YCbCr", (40, 80), blocks))
    for entropy in ("gpu", "gpu-fixed"):
        run = lambda q: q.call(codec.compress_many, x, extension=".png", entropy=entropy,               # noqa: E731
                               _draws=("workspace_fills", "empties", "pinned_fills"))
        files = run(p)
        for b, data in enumerate(files):
            meta, layers = _unpack_ajpg(e, data)
            assert (meta["height"], meta["width"], meta["color_space"]) == (H, W, "YCbCr")
            for l in range(3):
                assert layers[l]["root_size"] == refs[b][l]["root_size"]
                assert np.array_equal(layers[l]["states"], refs[b][l]["states"]), (entropy, b, l)
                assert np.array_equal(layers[l]["coeffs"], refs[b][l]["coeffs"]), (entropy, b, l)
        assert files == _control(e, ("compress_many", entropy), run), f"{entropy}: bytes differ from the 0x00 run"


# ---------------------------------------------------------------------------------------------------------------- sweep, metrics, LPIPS
@row("requantise")
def _requantise(e, p):
    """aej_requantise_batch: the DCT of one encode quantised again for two other quality ranges = the oracle's encode at those
    ranges; beyond every count the poisoned output is untouched"""
    import importlib
    import test_gpu_quadtree_chunks as TQ
    from test_gpu_sweep import layer_slices
    S = importlib.import_module("adaptive_edge_aware_jpeg_amd.sweep")
    t = e.torch
    H, W, br, qrs = 136, 260, (4, 64), [(10, 90), (75, 75)]
    x, _ = TQ.oracle_refs(e.oracle, H, W, br)
    refs = _requant_refs(e.oracle, H, W, br, tuple(qrs))
    codec = e.A.Jpeg(e.A.JpegCompressionSettings("YCbCr", (40, 80), br))
    enc = p.call(codec.compress_batch, x, want_dct=True)
    ctx = codec._bind()
    pl, cnt = enc.plan, enc.counts_host
    n = pl.batch * pl.coeff_stride

    def entry():
        out = ctx.empty((len(qrs) * n,), t.int32)
        blob = ctx.to_device(np.concatenate([S.qmats_blob("YCbCr", qr, br) for qr in qrs]).astype(np.int32), t.int32)
        ctx.check(ctx.lib.aej_requantise_batch(ctx.handle, enc.dct.data_ptr(), enc.leaves.data_ptr(), enc.counts.data_ptr(), pl.batch, pl.H, pl.W,
                                               len(qrs), blob.data_ptr(), out.data_ptr(), ctypes.c_uint64(n)))
        return out
    out = p.call(entry, _draws=("empties",)).view(len(qrs), -1).cpu().numpy()
    untouched = np.frombuffer(bytes([p.byte]) * 4, np.int32)[0]
    for j in range(len(qrs)):
        for b in range(3):
            for l in range(3):
                o, end_used, end = layer_slices(pl, cnt, b, l)
                assert np.array_equal(out[j, o:end_used], refs[j][b][l]["coeffs"]), (qrs[j], b, l)
                assert (out[j, end_used:end] == untouched).all(), (qrs[j], b, l, "written beyond n_coeffs")


@functools.lru_cache(maxsize=None)
def _requant_refs(oracle, H, W, br, qrs):
    import test_gpu_quadtree_chunks as TQ
    x = TQ.small_images(oracle, H, W)
    return [[oracle.encode_image(x[b], "YCbCr", qr, br) for b in range(3)] for qr in qrs]


@functools.lru_cache(maxsize=None)
def _sweep_inputs(oracle):
    return np.stack([oracle.synth_image(176, 200, 21).astype(np.float32) / np.float32(255),
                     oracle.synth_image(176, 200, 22, "noise").astype(np.float32) / np.float32(255)])


@functools.lru_cache(maxsize=None)
def _sweep_refs(oracle, space, qr, br):
    """per image: (container length, the oracle's decode) of the oracle's own encode"""
    out = []
    for img in _sweep_inputs(oracle):
        H, W = img.shape[:2]
        data = oracle.write_ajpg(oracle.encode_image(img, space, qr, br), H, W, space, qr, br, ".png")
        out.append((len(data), oracle.decode_image(data)))
    return out


@row("decode_batch_tables")
def _decode_tables(e, p):
    """aej_decode_batch_tables, the sweep's decode entry, with tables of another quality than the context's"""
    import importlib
    S = importlib.import_module("adaptive_edge_aware_jpeg_amd.sweep")
    t = e.torch
    x = _sweep_inputs(e.oracle)
    for space, qr, br in (("YCbCr", (10, 50), (4, 64)), ("YCoCg-R", (75, 90), (8, 8))):
        refs = _sweep_refs(e.oracle, space, qr, br)
        enc = p.call(e.A.Jpeg(e.A.JpegCompressionSettings(space, qr, br)).compress_batch, x)
        ctx = e.A.Jpeg(e.A.JpegCompressionSettings(space, (50, 50), br))._bind()      # the context's own tables are another quality's
        pl = enc.plan
        blob = ctx.to_device(S.qmats_blob(space, qr, br), t.int32)

        def entry():
            rgb = ctx.empty((pl.batch, pl.H, pl.W, 3), t.float32)
            nb = int(ctx.lib.aej_decode_workspace_bytes(ctx.handle, pl.batch, pl.H, pl.W))
            ws = ctx.workspace(nb)
            ctx.check(ctx.lib.aej_decode_batch_tables(ctx.handle, enc.coeffs.data_ptr(), enc.leaves.data_ptr(), enc.counts.data_ptr(), pl.batch, pl.H,
                                                      pl.W, blob.data_ptr(), rgb.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nb)))
            return rgb
        got = p.call(entry).cpu().numpy()
        for b in range(2):
            assert np.array_equal(got[b], refs[b][1], equal_nan=True), (space, qr, br, b)


def _check_metrics(got, a, b, which, label):
    import test_gpu_metrics as TM
    for i in range(len(a)):
        ref = TM.reference(a[i], b[i], which)
        for col, name in enumerate(("psnr", "ssim", "ms_ssim")):
            if not which & (1 << col):
                assert np.isnan(got[i, col]), (label, i, name)
                continue
            want, bound = ref[col]
            assert abs(float(got[i, col]) - want) <= bound, (label, i, name, float(got[i, col]), want, bound)


@row("sweep")
def _sweep(e, p):
    """sweep() over a 2 x 2 grid: one encode per block range, requantise per quality range, decode, metrics -- it asks for the workspace
    again in mid-operation and keeps state there, so it is armed once.  File sizes are the oracle's containers', the metrics are the
    float64 restatement's on the oracle's decode"""
    x = _sweep_inputs(e.oracle)
    qrs, brs = [(10, 50), (75, 90)], [(4, 64), (8, 8)]
    res = p.call(e.A.sweep, x, ("YCbCr",), qrs, brs, extension=".png")
    assert len(res.cells) == 4
    for j, (cs, qr, br) in enumerate(res.cells):
        refs = _sweep_refs(e.oracle, cs, qr, br)
        assert res.bytes[:, j].tolist() == [r[0] for r in refs], (cs, qr, br)
        got = np.stack([res.psnr[:, j], res.ssim[:, j], res.ms_ssim[:, j]], 1)
        _check_metrics(got, x, np.stack([r[1] for r in refs]), 7, f"sweep cell {cs} {qr} {br}")
    # the file sizes again from the streams written on the GPU: they round-trip by construction of the row above; here their lengths
    gpu = p.call(e.A.sweep, x, ("YCbCr",), qrs, brs, metrics=0, sizes="gpu")
    want = _control(e, "sweep gpu sizes", lambda q: q.call(e.A.sweep, x, ("YCbCr",), qrs, brs, metrics=0, sizes="gpu").bytes.copy())
    assert np.array_equal(gpu.bytes, want) and np.isnan(gpu.psnr).all()


@functools.lru_cache(maxsize=None)
def _metric_pairs(A, H, W, n, seed):
    import test_gpu_metrics as TM
    return TM.pairs(A, H, W, n, seed)


@row("evaluation_metrics")
def _metrics(e, p):
    """EvaluationMetrics.batch at the metrics module's grey-pool and strip-edge shapes, and one MS-SSIM pad chain"""
    for H, W, which in ((11, 11, 3), (11, 300, 3), (300, 11, 3), (41, 137, 3), (137, 265, 3), (161, 161, 7)):
        a, b = _metric_pairs(e.A, H, W, 3, H + W)
        got = p.call(e.A.EvaluationMetrics.batch, a, b, which).cpu().numpy()
        _check_metrics(got, a, b, which, f"{H}x{W}")


@functools.lru_cache(maxsize=None)
def _lpips_cases(A, oracle):
    import lpips_reference as R
    import test_gpu_lpips as TL
    sd = R.random_state_dicts(2024)
    out = []
    for H, W in ((31, 31), (97, 131)):
        x = TL.synth(oracle, H, W, H + W)[None]
        y = TL.jpeg_pair(A, x, (10, 25))
        out.append((H, W, x, y, R.lpips64(x[0], y[0], *sd)))
    return A.LpipsWeights.load(*sd), out


@row("lpips_batch")
def _lpips(e, p):
    """EvaluationMetrics.lpips_batch: feature maps and partial sums in the workspace, float64 scores"""
    import test_gpu_lpips as TL
    weights, cases = _lpips_cases(e.A, e.oracle)
    for H, W, x, y, want in cases:
        got = p.call(e.A.EvaluationMetrics.lpips_batch, x, y, weights).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (1,)
        TL.check(float(got[0]), want, f"{H}x{W} poisoned")


# ---------------------------------------------------------------------------------------------------------------- standard JPEG: encoders
def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def _pil_jpeg(x, q, **kw):
    """Pillow's file of an array (RGB [H, W, 3] or grey [H, W])"""
    from PIL import Image
    import test_gpu_jfif_many as TM
    return TM._pil_save(Image.fromarray(x), q, **kw)


JFIF_KINDS = (dict(), dict(subsampling="4:4:4", optimize=True), dict(subsampling="4:2:2", progressive=True), dict(optimize=True),
              dict(subsampling="4:4:4", progressive=True))


@functools.lru_cache(maxsize=None)
def _jfif_same_size_cases():
    """[(images [5, H, W, 3], keywords, qualities, Pillow's files [q][i], Pillow's decode of them)] at 17 x 33 and 37 x 53"""
    import test_gpu_jfif as T
    out = []
    for (H, W), qs in (((17, 33), (10, 90)), ((37, 53), (75,)), ((1, 1), (50,))):
        x = T._images(H, W, H * 7 + W)
        for kw in JFIF_KINDS:
            files = [[_pil_jpeg(x[i], q, **kw) for i in range(len(x))] for q in qs]
            out.append((x, kw, qs, files, [[T._pil_decode(f) for f in row] for row in files]))
    return out


@row("standard_jpeg_many_and_batch")
def _jfif_many_batch(e, p):
    """standard_jpeg_many / standard_jpeg_batch, plain, optimize and progressive: the workspace of these entries (coefficients, bit
    counts, the Huffman histograms of optimize and progressive, scan lengths and cuts) comes from ctx.empty; Pillow's bytes and pixels"""
    for x, kw, qs, files, pixels in _jfif_same_size_cases():
        for j, q in enumerate(qs):
            got = p.call(e.A.standard_jpeg_many, x, q, _draws=("empties",), **kw)
            assert got == files[j], (x.shape, kw, q)
        sizes, dec = p.call(e.A.standard_jpeg_batch, x, qs, _draws=("empties",), **kw)
        dec = dec.cpu().numpy()
        for j in range(len(qs)):
            for i in range(len(x)):
                assert sizes[i, j] == len(files[j][i]), (x.shape, kw, qs[j], i)
                assert np.array_equal(dec[j, i], pixels[j][i]), (x.shape, kw, qs[j], i)


@functools.lru_cache(maxsize=None)
def _jfif_mixed_cases():
    """[(images, keywords of the call, Pillow's files)]: mixed sizes, grey, grey and colour mixed, restart intervals"""
    import test_gpu_jfif_many as TM
    rgb = [TM._image(h, w, 11 * k + 1) for k, (h, w) in enumerate(TM.SIZES[:10])]
    qs = list(TM.QUALITIES[:10])
    grey = [np.ascontiguousarray(a[..., 1]) for a in rgb]
    auto = [g if k % 2 else a for k, (a, g) in enumerate(zip(rgb, grey))]
    out = []
    for kw in (dict(), dict(subsampling="4:4:4", optimize=True), dict(subsampling="4:2:2", progressive=True), dict(restart_marker_rows=1),
               dict(restart_marker_blocks=3, optimize=True), dict(restart_marker_rows=1, progressive=True)):
        out.append((rgb, dict(kw, quality=qs), [_pil_jpeg(a, q, **kw) for a, q in zip(rgb, qs)]))
    for kw in (dict(), dict(optimize=True), dict(progressive=True), dict(restart_marker_rows=2)):
        out.append((grey, dict(kw, quality=qs, mode="L"), [_pil_jpeg(a, q, **kw) for a, q in zip(grey, qs)]))
    out.append((auto, dict(quality=qs, mode="auto"), [_pil_jpeg(a, q) for a, q in zip(auto, qs)]))
    return out


@row("standard_jpeg_encode_many")
def _jfif_encode_many(e, p):
    """standard_jpeg_encode_many: mixed sizes in one call, every entropy kind, restart rows and blocks, grey, grey and colour mixed"""
    for images, kw, want in _jfif_mixed_cases():
        got = p.call(e.A.standard_jpeg_encode_many, images, **kw)
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert len(got) == len(want) and bad == [], ({k: v for k, v in kw.items() if k != "quality"}, bad)


# ---------------------------------------------------------------------------------------------------------------- standard JPEG: decoders
DEC_KW = dict(progressive=True, layout_440=True)


@functools.lru_cache(maxsize=None)
def _jpeg_files():
    """83 x 61 files Pillow wrote: the five layouts, baseline and progressive, and two baseline files with restart intervals"""
    import jpegdec_box_reference as R
    files = [R.make_file(layout, 83, 61, prog, seed=3 + k) for k, (layout, prog) in
             enumerate((l[0], pr) for l in R.LAYOUTS for pr in (False, True))]
    files.append(R.save(R.picture(61, 83, 21), quality=85, restart_marker_blocks=2))
    files.append(R.save(R.picture(61, 83, 22), quality=60, subsampling="4:4:4", restart_marker_rows=1))
    return files


@functools.lru_cache(maxsize=None)
def _jpeg_refs(scale, mode):
    import jpeg_luma_reference as LR
    out = []
    for d in _jpeg_files():
        if mode == "auto":
            im = LR.draft(d, None, scale)
            out.append(np.asarray(im if im.mode == "L" else im.convert("RGB")))
        else:
            im = LR.draft(d, "L" if mode == "L" else None, scale)
            out.append(np.asarray(im if mode == "L" else im.convert("RGB")))
    return out


@row("standard_jpeg_decode_many")
def _jpeg_decode(e, p):
    """standard_jpeg_decode_many: baseline alone, baseline and progressive mixed, scale 2 / 4 / 8, mode "L" and "auto", box, scaled_box,
    4:4:0 sources -- sync states, scan offsets, per-segment tables, status words, coefficient planes"""
    import jpegdec_box_reference as R
    files = _jpeg_files()
    dec = e.A.standard_jpeg_decode_many
    base = [k for k in range(len(files)) if k % 2 == 0 and k != 6 or k >= 10]                      # baseline, no 4:4:0
    for g, k in zip(_np(p.call(dec, [files[k] for k in base])), base):
        _same(g, _jpeg_refs(1, "RGB")[k], ("baseline only", k))
    for scale in (1, 2, 4, 8):
        for mode in ("RGB", "L", "auto"):
            for k, (g, w) in enumerate(zip(_np(p.call(dec, files, scale=scale, mode=mode, **DEC_KW)), _jpeg_refs(scale, mode))):
                _same(g, w, (scale, mode, k))
    scales = [(1, 2, 4, 8)[k % 4] for k in range(len(files))]
    modes = [("RGB", "L", "auto")[k % 3] for k in range(len(files))]
    for k, g in enumerate(_np(p.call(dec, files, scale=scales, mode=modes, **DEC_KW))):
        _same(g, _jpeg_refs(scales[k], modes[k])[k], ("mixed", k))
    boxes = R.forced_boxes()
    for start in (1, 9, 17):
        bx = [boxes[(start + 5 * k) % len(boxes)] if k % 4 else None for k in range(len(files))]
        for mode in ("RGB", "L"):
            for k, g in enumerate(_np(p.call(dec, files, box=bx, mode=mode, **DEC_KW))):
                w = _jpeg_refs(1, mode)[k]
                _same(g, w if bx[k] is None else w[bx[k][1]:bx[k][3], bx[k][0]:bx[k][2]], ("box", start, mode, k, bx[k]))
    for scale, sb in ((2, (3, 5, 40, 29)), (4, (0, 2, 19, 16)), (8, (5, 1, 11, 8))):
        for k, g in enumerate(_np(p.call(dec, files, scale=scale, scaled_box=sb, **DEC_KW))):
            _same(g, _jpeg_refs(scale, "RGB")[k][sb[1]:sb[3], sb[0]:sb[2]], ("scaled_box", scale, k))


@functools.lru_cache(maxsize=None)
def _adobe_golden():
    import json
    import test_gpu_jpeg_adobe as TA
    with open(os.path.join(TA.HERE, "meta.json")) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(TA.HERE, "pixels.npz")))


@row("standard_jpeg_decode_many_adobe")
def _jpeg_decode_adobe(e, p):
    """adobe=True: CMYK, YCCK and RGB-coded files, baseline and progressive, against Pillow's recorded pixels"""
    import test_gpu_jpeg_adobe as TA
    meta, px = _adobe_golden()
    names = [c["name"] for c in meta["cases"]]
    names = [names[(5 * i) % len(names)] for i in range(len(names))]
    files = [TA._file(n) for n in names]
    for mode in ("auto", "RGB"):
        for n, g in zip(names, _np(p.call(e.A.standard_jpeg_decode_many, files, progressive=True, adobe=True, mode=mode))):
            _same(g, px[f"{n}/{mode}"], (n, mode))
    for n in ("cmyk_2x2k", "ycck_2x1_prog"):
        _same(_np(p.call(e.A.standard_jpeg_decode_many, [TA._file(n)], progressive=True, adobe=True, mode="auto"))[0], px[f"{n}/auto"], n)


@functools.lru_cache(maxsize=None)
def _stream_cases():
    """one file per tag of the catalogue of conforming streams no encoder writes, with its reference decode -- and, since most cases
    carry no tag, one per group (the first part of the name), per layout and per kind (baseline, progressive).  The "large" tag's one
    file is among them: 1024 x 1024 grey, the progressive decoder's largest coefficient clear here"""
    import jpeg_stream_catalogue as C
    picked, seen = [], set()
    for c in C.catalogue():
        keys = set(c.tags) | {"group " + c.name.split("/")[0], "layout " + c.layout, "progressive" if c.progressive else "baseline"}
        if keys - seen:
            seen |= keys
            picked.append(c)
    return [(c, C.reference(c.data)) for c in picked]


@row("jpeg_stream_catalogue")
def _jpeg_streams(e, p):
    """the decoders on one stream per tag of jpeg_stream_catalogue, at the smallest subsequence length and the default one"""
    import test_gpu_jpeg_streams as TS
    cases = _stream_cases()
    assert len(cases) >= 8
    for family in TS.FAMILIES:
        mine = [(c, r) for c, r in cases if ("uniform" in c.tags) == (family == "uniform")]
        if not mine:
            continue
        for S in (32, 2048):
            try:
                TS._set_s(S)
                got = _np(p.call(e.A.standard_jpeg_decode_many, [c.data for c, _ in mine], **DEC_KW))
            finally:
                TS._set_s(2048)
            for (c, ref), g in zip(mine, got):
                _same(g, ref, (c.name, S))


# ---------------------------------------------------------------------------------------------------------------- thumbnails and resize
@functools.lru_cache(maxsize=None)
def _thumb_golden():
    import json
    import test_gpu_resample as TR
    with open(os.path.join(TR.HERE, "meta.json")) as f:
        cases = json.load(f)["cases"]
    return cases, dict(np.load(os.path.join(TR.HERE, "pixels.npz")))


@row("thumbnail_many")
def _thumbnails(e, p):
    """standard_jpeg_thumbnail_many on the recorded Pillow thumbnails: one call per (filter, reducing_gap) over baseline and progressive
    files of every layout, and the mixed call of test_gpu_resample"""
    import test_gpu_resample as TR
    cases, px = _thumb_golden()
    groups = {}
    for c in cases:
        if c["kind"] == "thumb":
            groups.setdefault((c["filter"], c["gap"]), []).append(c)
    for (f, gap), cs in sorted(groups.items(), key=str):
        got = _np(p.call(e.A.standard_jpeg_thumbnail_many, [TR._file(c["folder"], c["name"]) for c in cs], [tuple(c["size"]) for c in cs],
                         resample=f, reducing_gap=gap, progressive=True))
        for c, g in zip(cs, got):
            _same(g, px[c["key"]], c["key"])


@functools.lru_cache(maxsize=None)
def _thumb_jpeg_refs():
    import test_gpu_jfif_many as TM
    src = TM._thumbnailed_colour_files()
    files = [d for _, _, d in src]
    return files, [TM._pil_thumbnail_jpeg(d, (64, 64), 80) for d in files], [TM._pil_thumbnail_jpeg(d, (50, 70), 60, progressive=True) for d in files]


@row("thumbnail_jpeg_many")
def _thumbnail_jpeg(e, p):
    """standard_jpeg_thumbnail_jpeg_many: decode, resize and encode chained on the device, against Pillow's thumbnail-then-save"""
    files, want_a, want_b = _thumb_jpeg_refs()
    got = p.call(e.A.standard_jpeg_thumbnail_jpeg_many, files, (64, 64), quality=80, progressive=True)
    assert [i for i, (g, w) in enumerate(zip(got, want_a)) if g != w] == []
    got = p.call(e.A.standard_jpeg_thumbnail_jpeg_many, files, (50, 70), quality=60, progressive_out=True, progressive=True)
    assert [i for i, (g, w) in enumerate(zip(got, want_b)) if g != w] == []


@functools.lru_cache(maxsize=None)
def _crop_refs(size, gap, filt, mode):
    from PIL import Image
    import jpegdec_sbox_reference as SB
    import test_gpu_jpegdec_sbox as TSB
    files, dims = TSB._crop_files()
    boxes = TSB._crop_boxes(dims, size)
    out = []
    for d, b in zip(files, boxes):
        s = SB.crop_scale(b, size, gap)
        im = SB.pil_drafted(d, mode, s).resize(size, getattr(Image.Resampling, filt.upper()), box=tuple(v / s for v in b), reducing_gap=gap)
        out.append(np.asarray(im))
    return files, boxes, out


@row("resized_crop_many")
def _resized_crop(e, p):
    """standard_jpeg_resized_crop_many: the decode of a box at reduced scale and the resize in one call, against Pillow's draft + resize"""
    for size, gap, filt, mode in (((32, 24), None, "bilinear", "RGB"), ((32, 24), 1.0, "bicubic", "RGB"), ((32, 24), 2.0, "lanczos", "RGB"),
                                  ((96, 80), None, "hamming", "RGB"), ((32, 24), 1.0, "box", "L")):
        files, boxes, want = _crop_refs(size, gap, filt, mode)
        got = p.call(e.A.standard_jpeg_resized_crop_many, files, boxes, size, filt, reducing_gap=gap, mode=mode, **DEC_KW).cpu().numpy()
        for i, w in enumerate(want):
            _same(got[i], w, (size, gap, filt, mode, i, boxes[i]))


@row("resize_many")
def _resize(e, p):
    """resize_many: the recorded Pillow resizes (sources, sizes, filters and boxes per image) and the edge shapes against the model"""
    import resample_reference as M
    import test_gpu_resample as TR
    cases, px = _thumb_golden()
    for gap in (None, 1.0, 1.5, 2.0, 3.0):
        cs = [c for c in cases if c["kind"] == "resize" and c["gap"] == gap]
        got = _np(p.call(e.A.resize_many, [px[f"src/{c['source']}"] for c in cs], [tuple(c["size"]) for c in cs], resample=[c["filter"] for c in cs],
                         box=[c["box"] for c in cs], reducing_gap=gap))
        for c, g in zip(cs, got):
            _same(g, px[c["key"]], c["key"])
    one, small, thin, pic = TR._picture(1, 1, 5), TR._picture(5, 7, 6), TR._picture(23, 1, 7), TR._picture(12, 17, 8)
    jobs = [(one, (5, 7), None), (small, (1, 1), None), (thin, (1, 9), None), (thin, (4, 23), None), (thin, (3, 40), None),
            (pic, (6, 5), (0.5, 0.25, 16.4, 12)), (pic, (17, 12), (0, 0, 16.5, 12)), (pic, (17, 12), None)]      # test_edge_shapes' jobs
    for f in ("bicubic", "bilinear", "hamming"):
        got = _np(p.call(e.A.resize_many, [j[0] for j in jobs], [j[1] for j in jobs], resample=f, box=[j[2] for j in jobs]))
        for j, g in zip(jobs, got):
            _same(g, M.resize(j[0], j[1], f, j[2]), (f, j[0].shape, j[1], j[2]))


# ---------------------------------------------------------------------------------------------------------------- lossless transcode and transforms
@functools.lru_cache(maxsize=None)
def _transcode_cases():
    """(sources, Pillow's optimize=True files, Pillow's progressive=True files): every source kind of several settings and sizes"""
    import test_gpu_jfif_transcode as TT
    src, want_opt, want_prog = [], [], []
    for name, settings in (("noise_1x1", [dict(quality=75, subsampling="4:2:0")]), ("noise_9x3", [dict(quality=100, subsampling="4:2:2")]),
                           ("primaries_17x33", [dict(quality=50, subsampling="4:2:0"), dict(quality=50, subsampling="4:4:4")]),
                           ("noise_37x53", [dict(quality=1, subsampling="4:2:0"), dict(quality=95, subsampling="4:2:2"),
                                            dict(qtables=[list(TT.QT[0]), list(TT.QT[1])], subsampling="4:2:2")])):
        x = TT.IMAGES[name]()
        for s in settings:
            wo, wp = TT._pil(x, optimize=True, **s), TT._pil(x, progressive=True, **s)
            for k in TT.KINDS:
                src.append(TT._pil(x, **s, **k))
                want_opt.append(wo)
                want_prog.append(wp)
    return src, want_opt, want_prog


@functools.lru_cache(maxsize=None)
def _transcode_mixed():
    import test_gpu_jfif_transcode as TT
    src, _ = TT._mixed_sources()
    return src, [TT._pil_decode(s) for s in src]


@row("transcode_many")
def _transcode(e, p):
    """standard_jpeg_transcode_many both ways: Pillow's optimize=True and progressive=True files of the same pictures, byte for byte;
    the mixed call of the transcode module, whose outputs Pillow decodes to the sources' pixels"""
    import test_gpu_jfif_transcode as TT
    src, want_opt, want_prog = _transcode_cases()
    for prog, want in ((False, want_opt), (True, want_prog)):
        got = p.call(e.A.standard_jpeg_transcode_many, src, progressive=prog)
        assert [i for i, (g, w) in enumerate(zip(got, want)) if g != w] == [], prog
    mixed, pixels = _transcode_mixed()
    for prog in (False, True):
        got = p.call(e.A.standard_jpeg_transcode_many, mixed, progressive=prog)
        for i, (g, w) in enumerate(zip(got, pixels)):
            assert np.array_equal(TT._pil_decode(g), w), (prog, i)


@functools.lru_cache(maxsize=None)
def _seq_cases():
    """jfif_seq_cases' coefficient sets that no pixels produce (16-bit codes, the longest value fields, ZRL runs, blocks that end at
    coefficient 63) as conforming baseline files, and what the restatement expects of the scan without and with a restart interval
    of one MCU: (cases, files, {R: [(scan bytes, histograms)]})"""
    import jfif_seq_cases as C
    import jpeg_stream_writer as W
    cases = [(layout, name, coef) for layout in ("grey", "4:2:0") for name, coef in C.sets(layout)]
    files = [W.write(*C.LAYOUTS[layout][3:], C.writer_comps(coef, layout)) for layout, _, coef in cases]
    return cases, files, {R: [C.expected(coef, layout, R, 1) for layout, _, coef in cases] for R in (0, 1)}


@row("transcode_many_seq_cases")
def _transcode_seq(e, p):
    """the baseline entropy kernels of jfif.hip on blocks pixels never give, reached as test_gpu_jfif_seq reaches them: through the
    lossless transcoder (grey=True), without and with a restart interval of one MCU.  Scan bytes and the DHT segments of the scan's own
    histograms against the Python restatement (jfif_seq_cases.expected): the stream words cleared for exactly the stream's length,
    the per-segment 0xFF counts, bit offsets and histograms"""
    import jfif_restart_reference as RR
    import jfif_seq_cases as C
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as S
    from test_gpu_jfif_seq import _dht
    cases, files, want = _seq_cases()
    for R, kw in ((0, {}), (1, dict(restart_marker_blocks=1))):
        out = p.call(e.A.standard_jpeg_transcode_many, files, grey=True, **kw)
        assert len(out) == len(cases)
        for (layout, name, coef), o, (data, hist) in zip(cases, out, want[R]):
            segs = RR.walk(o)
            (sos,) = [(a, b) for m, a, b in segs if m == 0xDA]
            hdr = 2 + int.from_bytes(o[sos[0] + 2:sos[0] + 4], "big")
            assert o[sos[0] + hdr:sos[1]] == data and o[sos[1]:] == b"\xff\xd9", (layout, name, R)
            ids = [0x00, 0x10] if layout == "grey" else [0x00, 0x10, 0x01, 0x11]
            assert [o[a:b] for m, a, b in segs if m == 0xC4] == [_dht(i, *S.huffman_table(hist[t])) for t, i in enumerate(ids)], (layout, name, R)
            assert (RR.dri_sequence(o), len(RR.markers(o)[0])) == ([1 if R else None], C.blocks_of(layout) // (1 if layout == "grey" else 6) - 1 if R else 0)


@functools.lru_cache(maxsize=None)
def _transform_coef_cases():
    """[(files, transform names, trim, check(outputs))] with the source coefficients read from Pillow's own progressive twin of each file"""
    import jfif_transform_reference as R
    import progressive_reference as P
    import test_gpu_jfif_transform as TF
    out = []
    for case in ("9x3", "17x33", "37x53", "perfect_48x32_422", "one_mcu_16x16"):
        make, layouts, qualities, trim = TF.COEF_CASES[case]
        x = make()
        H, W = x.shape[:2]
        files, names, meta = [], [], []
        for layout in layouts:
            f = TF._pil(x, quality=qualities[0], subsampling=layout)
            coef = P.coefficients(TF._pil(x, quality=qualities[0], subsampling=layout, progressive=True))
            for name in TF._supported(H, W, layout, trim):
                if name != "none":
                    files.append(f)
                    names.append(name)
                    meta.append((layout, coef))
        out.append((case, H, W, trim, files, names, meta))
    return out


@row("transform_many")
def _transform(e, p):
    """standard_jpeg_transform_many with all eight transforms, trim, crop and drop_chroma: coefficients against the NumPy restatement
    applied to what Pillow's own progressive twin of each source holds; pixels where equality is exact"""
    import jfif_cut_reference as C
    import jfif_transform_reference as R
    import progressive_reference as P
    import test_gpu_jfif_cut as TC
    import test_gpu_jfif_transform as TF
    from PIL import Image
    tm = e.A.standard_jpeg_transform_many
    for case, H, W, trim, files, names, meta in _transform_coef_cases():
        out = p.call(tm, files, names, progressive=True, trim=trim)
        for o, name, (layout, coef) in zip(out, names, meta):
            hs, vs = R.LAYOUTS[layout]
            real, (oH, oW, ohs, ovs) = R.coefficients(coef, H, W, hs, vs, name, trim)
            frame, _ = P.walk(o)
            assert (frame["height"], frame["width"], frame["comps"][0]["h"], frame["comps"][0]["v"]) == (oH, oW, ohs, ovs), (case, name, layout)
            R.check_padded(P.coefficients(o), real, oH, oW, ohs, ovs, f"{case} {name} {layout}")
    src, dec = _tile_file()
    for prog in (False, True):
        for name, o in zip(R.NAMES, p.call(tm, [src] * 8, list(R.NAMES), progressive=prog)):
            assert np.array_equal(TF._pil_decode(o), R.pixels(dec, name)), (name, prog)
    files, names, shapes = _transform_mixed()
    for prog in (False, True):
        got = p.call(tm, files, names, progressive=prog, trim=True)
        for i, (f, name, g, (h, w, layout)) in enumerate(zip(files, names, got, shapes)):
            oH, oW, _, _ = R.out_geometry(h, w, *R.LAYOUTS[layout], name, True)
            im = Image.open(io.BytesIO(g))
            assert im.size == (oW, oH) and im.mode == "RGB" and im.info.get("progressive", 0) == int(prog), (i, name)
            if name == "none":
                assert np.array_equal(TF._pil_decode(g), TF._pil_decode(f)), i
    # crop and drop_chroma: the cut module's cases on sources whose coefficients Pillow's progressive twin gives
    for drop in (False, True):
        cut_files, cut_names, cut_boxes, cut_meta = _cut_cases(drop)
        got = p.call(tm, cut_files, cut_names, progressive=True, trim=True, crop=cut_boxes, drop_chroma=drop, **TC.ANY)
        for g, name, box, (key, planes, H, W, hs, vs, one) in zip(got, cut_names, cut_boxes, cut_meta):
            real, (oH, oW, ohs, ovs), _ = C.cut(planes, H, W, hs, vs, name, True, box, drop)
            frame, _ = P.walk(g)
            assert (frame["height"], frame["width"], len(frame["comps"])) == (oH, oW, 1 if (one or drop) else 3), (key, name, box, drop)
            C.check_padded(P.coefficients(g), real, oH, oW, ohs, ovs, f"{key} {name} {box} drop={drop}")


@functools.lru_cache(maxsize=None)
def _tile_file():
    import test_gpu_jfif_transform as TF
    tiles = np.random.default_rng(40).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    src = TF._pil(np.repeat(np.repeat(tiles, 8, 0), 8, 1), quality=100, subsampling="4:4:4")
    dec = TF._pil_decode(src)
    assert np.array_equal(dec, np.repeat(np.repeat(dec[::8, ::8], 8, 0), 8, 1))      # Pillow alone: the tiles decode as tiles
    return src, dec


@functools.lru_cache(maxsize=None)
def _transform_mixed():
    import test_gpu_jfif_transform as TF
    return TF._mixed()


@functools.lru_cache(maxsize=None)
def _cut_cases(drop):
    import jfif_cut_reference as C
    import jfif_transform_reference as R
    import progressive_reference as P
    import test_gpu_jfif_cut as TC
    import test_gpu_jfif_transcode as TT
    x = TT._noise(37, 50)
    src = {}
    for layout, kind in (("4:2:0", dict()), ("4:2:2", dict(progressive=True)), ("4:4:4", dict(restart_marker_blocks=1))):
        twin = TT._pil(x, quality=75, subsampling=layout, progressive=True)
        src[layout] = (TT._pil(x, quality=75, subsampling=layout, **kind), P.coefficients(twin), 37, 50, *C.LAYOUTS[layout], False)
    src["grey"] = (TC._grey(x, quality=75), P.coefficients(TC._grey(x, quality=75, progressive=True)), 37, 50, 1, 1, True)
    cases = [c for c in TC.CASES if c[0] in src and (drop or not (c[1] in R.TRANSPOSING and c[0] == "4:2:2"))]
    return ([src[c[0]][0] for c in cases], [c[1] for c in cases], [c[3] for c in cases], [(c[0],) + src[c[0]][1:] for c in cases])


# ---------------------------------------------------------------------------------------------------------------- PNG
@row("png_decode_many")
def _png_decode(e, p):
    """png_decode_many with the inflate on the GPU and on the host: the mixed call of test_gpu_png with a mode per file"""
    import png_reference as R
    import test_gpu_png as TP
    names, modes = TP._mixed()
    S = R.suite()
    files = [S[n] for n in names]
    for inflate in ("gpu", "host"):
        got = p.call(e.A.png_decode_many, files, mode=modes, inflate=inflate, _draws=("workspace_fills", "empties", "pinned_fills"))
        for n, m, g in zip(names, modes, got):
            _same(g.cpu().numpy(), R.expected(n, m), (n, m, inflate))


@functools.lru_cache(maxsize=None)
def _png_encode_cases():
    import test_gpu_png_encode as TPE
    cases = TPE.all_cases()
    names = sorted(cases)
    images = [cases[n] for n in names]
    return names, images, {(opt, lv): [TPE.pil_save(x, optimize=opt, compress_level=lv) for x in images] for opt, lv in ((False, 6), (False, 1), (True, 6))}


@row("png_encode_many_host_entropy")
def _png_encode_host(e, p):
    """png_encode_many(entropy="host"): the filter kernel's scanlines deflated by zlib on the host are Pillow's files, byte for byte"""
    names, images, want = _png_encode_cases()
    for (opt, lv), files in want.items():
        got = p.call(e.A.png_encode_many, images, optimize=opt, compress_level=lv, entropy="host", _draws=("empties", "pinned_fills"))
        assert [n for n, g, w in zip(names, got, files) if g != w] == [], (opt, lv)


@row("png_encode_many_gpu_entropy")
def _png_encode_gpu(e, p):
    """png_encode_many(entropy="gpu"): the byte-stream deflate's workspace, histograms and slots.  check_gpu_files (framing, zlib back to
    the reference scanlines, Pillow opens the file to the image), and the bytes equal the 0x00 run's"""
    import test_gpu_png_encode as TPE
    names, images, _ = _png_encode_cases()
    for opt in (False, True):
        run = lambda q: q.call(e.A.png_encode_many, images, optimize=opt, _draws=("workspace_fills", "empties", "pinned_fills"))      # noqa: E731
        files = run(p)
        TPE.check_gpu_files(e.A, images, files, opt)
        assert files == _control(e, ("png_encode_many", opt), run), f"optimize={opt}: bytes differ from the 0x00 run"


# ---------------------------------------------------------------------------------------------------------------- filters
@functools.lru_cache(maxsize=None)
def _filter_cases():
    import filter_reference as M
    import test_gpu_filter as TF
    Spec = M.Spec
    cases = TF._mixed()
    a = M.image((70, 133), 3, seed=5)
    cases += [(a, Spec("GaussianBlur", 5.4)), (a, Spec("BoxBlur", 14)), (a, Spec("UnsharpMask", 5.4, 130, 2)),          # the largest fused halo
              (a, Spec("GaussianBlur", 6.5)), (a, Spec("BoxBlur", 15.25)), (a, Spec("UnsharpMask", 6.5, 130, 2))]       # one above it
    return cases, [M.model(x, s) for x, s in cases]


@row("filter_many")
def _filters(e, p):
    """filter_many on the fused path and on the passes path (carried rows, column bands, the intermediate planes in the workspace)"""
    import test_gpu_filter as TF
    cases, want = _filter_cases()
    geometry = e.A.filters.filter_geometry()
    fused = [k for k, (_, s) in enumerate(cases) if TF._fits(e.A, s, geometry["max_halo"])]
    assert 0 < len(fused) < len(cases), "both sides of the halo limit"
    for path in ("fused", "passes", "auto"):
        pick = fused if path == "fused" else list(range(len(cases)))
        got = _np(p.call(e.A.filter_many, [cases[k][0] for k in pick], [cases[k][1] for k in pick], _path=path))
        for k, g in zip(pick, got):
            _same(g, want[k], (path, cases[k][0].shape, cases[k][1]))


# ---------------------------------------------------------------------------------------------------------------- error returns
_ERROR_TEXT = {}


def _raises_as_unpoisoned(p, key, fn, *args, **kwargs):
    """the call raises ValueError with the text the same call gives without the harness (asked once, before this row's first poisoned
    call of it could leave anything behind)"""
    assert key in _ERROR_TEXT, key
    with pytest.raises(ValueError) as got:
        p.call(fn, *args, _draws=(), **kwargs)
    assert not isinstance(got.value, NotImplementedError) and str(got.value) == _ERROR_TEXT[key], (key, str(got.value), _ERROR_TEXT[key])


def _error_cases(e):
    """[(key, entry, args, keywords, check of the good neighbours)]: each module's corrupt file between two good ones"""
    import png_reference as PR
    import test_gpu_decompress_many as TDM
    import test_gpu_resample as TR
    A = e.A
    good, good2 = TR._file("jpegdec", "lena_64x64_420_q75"), TR._file("jpegdec", "baboon_48x40_422_q50")
    data = TR._file("jpegdec", "buildings_96x128_crop_q95")
    d = A.standard_jpeg.parse_header(data)
    cut = data[:d.scan_offset + (len(data) - d.scan_offset) // 2]
    pdata = TR._file("jpegprog", "buildings_128x96_q90")
    pcut = pdata[:len(pdata) * 2 // 3]
    from test_gpu_jfif import _pil_decode
    pixels = [_pil_decode(good), _pil_decode(good2)]

    def jpeg_neighbours(p):
        for g, w in zip(_np(p.call(A.standard_jpeg_decode_many, [good, good2], progressive=True)), pixels):
            _same(g, w, "good neighbours after the error")
    out = [("jpegdec truncated", A.standard_jpeg_decode_many, ([good, cut, good2],), dict(), jpeg_neighbours),
           ("jpegprog truncated", A.standard_jpeg_decode_many, ([good, pcut, good2],), dict(progressive=True), jpeg_neighbours),
           ("thumbnail truncated", A.standard_jpeg_thumbnail_many, ([good, cut, good2], (20, 20)), dict(), jpeg_neighbours),
           ("thumbnail_jpeg truncated", A.standard_jpeg_thumbnail_jpeg_many, ([good, cut, good2], (20, 20)), dict(quality=80), jpeg_neighbours),
           ("transcode truncated", A.standard_jpeg_transcode_many, ([good, cut, good2],), dict(), jpeg_neighbours),
           ("transform truncated", A.standard_jpeg_transform_many, ([good, cut, good2], "flip_v"), dict(trim=True), jpeg_neighbours)]
    S = PR.suite()

    def png_neighbours(inflate):
        def check(p):
            for n, g in zip(("level9", "ga"), _np(p.call(A.png_decode_many, [S["level9"], S["ga"]], inflate=inflate, _draws=("empties",)))):
                _same(g, PR.expected(n, "RGB"), (n, inflate))
        return check
    for what, bad in PR.corrupt_files().items():
        for inflate in ("gpu", "host"):
            out.append((f"png {what} {inflate}", A.png_decode_many, ([S["level9"], bad, S["ga"]],), dict(inflate=inflate), png_neighbours(inflate)))
    name, ajpg, want = _ajpg_fixtures(e.oracle)[0]
    bad = [m for m in TDM.mutations(ajpg)]
    picks = [bad[k] for k in (0, 3, 6, 10, 12)]                       # a short header, a bad symbol, a wrong root, a short stream, a cut stream

    def ajpg_neighbours(entropy):
        def check(p):
            got = p.call(A.Jpeg(A.JpegCompressionSettings()).decompress_many, [ajpg, ajpg], entropy=entropy, _draws=("empties",)).cpu().numpy()
            assert np.array_equal(got[0], want) and np.array_equal(got[1], want), entropy
        return check
    for k, m in enumerate(picks):
        for entropy in ("gpu", "host"):
            out.append((f"ajpg mutation {k} {entropy}", lambda files, entropy=entropy: A.Jpeg(A.JpegCompressionSettings()).decompress_many(files, entropy=entropy),
                        ([ajpg, m, ajpg],), dict(), ajpg_neighbours(entropy)))
    return out


@row("error_returns")
def _errors(e, p):
    """a corrupt file between two good ones: the same ValueError text as without the harness (a status word or an error flag that
    started as poison must not change which file is named, or why), and the good neighbours decode correctly afterwards"""
    cases = _error_cases(e)
    for key, fn, args, kw, _ in cases:
        if key not in _ERROR_TEXT:
            with p.suspended(), pytest.raises(ValueError) as plain:                                        # the plain methods, for this one call
                fn(*args, **kw)
            _ERROR_TEXT[key] = str(plain.value)
            text = _ERROR_TEXT[key]                                  # pinned where the cause is known, and it names file (or image) 1
            if key.endswith(" truncated") and not key.startswith("jpegprog"):
                assert text == "file 1: truncated scan (it ends before the last MCU)", (key, text)
            else:
                assert text.startswith("file 1") or "image 1" in text, (key, text)
    for key, fn, args, kw, neighbours in cases:
        _raises_as_unpoisoned(p, key, fn, *args, **kw)
        neighbours(p)


# ---------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("byte", PM.PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize("name", list(ROWS))
def test_row(env, name, byte):
    with PM.poisoned(env.ctx, byte) as p:
        ROWS[name](env, p)
        assert p.calls >= 1 and p.bytes > 0, "the row must have made its calls through the harness"


# rows that come first in one of the two orders so that a large call of one subsystem is followed by a small one of another
LARGE_FIRST = ("png_encode_many_gpu_entropy", "quadtree", "sweep", "standard_jpeg_many_and_batch", "filter_many", "decompress_batch")


@pytest.mark.parametrize("seed", [20250718, 99], ids=["order_A", "order_B"])
def test_call_order(env, seed):
    """All rows on one context in a seeded order, 0x01 between calls only: what the helpers cannot poison -- the library's own device
    buffers, cached plans and tables, its check word, the chain hooks -- is whatever the previous subsystem left.  Order A puts large
    calls in front of small ones of other subsystems (LARGE_FIRST alternating with the rest), order B is a plain shuffle."""
    rng = np.random.default_rng(seed)
    names = list(ROWS)
    order = [names[i] for i in rng.permutation(len(names))]
    if seed == 20250718:
        large = [n for n in order if n in LARGE_FIRST]
        rest = [n for n in order if n not in LARGE_FIRST]
        order = []
        while large or rest:
            order += large[:1] + rest[:2]
            large, rest = large[1:], rest[2:]
    assert sorted(order) == sorted(names)
    with PM.poisoned(env.ctx, 0x01) as p:
        for name in order:
            before = p.calls
            try:
                ROWS[name](env, p)
            except AssertionError as err:
                raise AssertionError(f"row {name!r} after {order[:order.index(name)]}: {err}") from err
            assert p.calls > before
