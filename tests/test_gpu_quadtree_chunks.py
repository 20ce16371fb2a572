"""GPU (-m gpu): the quadtree's chunk-run kernels (option "qt_chunks", csrc/quadtree.hip) against the CPU oracle.

With min block 4 and at least 16 cells per root side the count and emit passes run over the in-plane chunks only, several per wave, count
from ballot masks, and the scan pass produces the one symbol an out-of-plane chunk can originate; every other shape takes the general
kernels.  The yardstick is the oracle throughout; the two kernel sets are compared with each other on top of that."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (24, 40),                       # less than one chunk
          (64, 64), (64, 128), (128, 64),         # exact chunks
          (72, 200), (136, 260),                  # cut on both borders
          (20, 520), (520, 20),                   # a root square that is almost entirely out of plane: many '10' symbols, few waves
          (5, 7)]                                 # general path
BLOCKS = [(4, 64), (4, 16), (4, 4), (4, 128), (4, 256),      # the last two: upper pyramid and its zero-fill
          (8, 64), (16, 64)]                                 # these fall back to the general kernels


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def edge_maps(H, W):
    """name -> float32 edge map (1.0 = edge)"""
    z = np.zeros((H, W), np.float32)
    maps = {"zeros": z, "ones": np.ones((H, W), np.float32)}

    def with_pixels(pts):
        m = z.copy()
        for y, x in pts:
            m[y, x] = 1.0
        return m
    maps["first pixel"] = with_pixels([(0, 0)])
    maps["last pixel"] = with_pixels([(H - 1, W - 1)])
    maps["first pixel of every chunk"] = with_pixels([(y, x) for y in range(0, H, 64) for x in range(0, W, 64)])
    # the last in-plane pixel of the chunks in the last chunk row / column (cut by the border unless the side is a multiple of 64)
    maps["last in-plane pixel of border chunks"] = with_pixels([(H - 1, min(x + 63, W - 1)) for x in range(0, W, 64)] +
                                                               [(min(y + 63, H - 1), W - 1) for y in range(0, H, 64)])
    for x in (63, 64):
        if x < W:
            m = z.copy(); m[:, x] = 1.0
            maps[f"vertical line x={x}"] = m
    for y in (63, 64):
        if y < H:
            m = z.copy(); m[y, :] = 1.0
            maps[f"horizontal line y={y}"] = m
    for p, seed in ((0.001, 11), (0.02, 12), (0.5, 13)):
        maps[f"noise p={p}"] = (np.random.default_rng(seed + 1000 * H + W).random((H, W)) < p).astype(np.float32)
    return maps


def chunk_launches(ctx):
    """quadtree stages the chunk-run kernels have served on this context so far"""
    return ctx.get_option("qt_chunk_launches")


@pytest.mark.parametrize("H,W", SHAPES)
def test_quadtree_one_image_against_oracle(A, oracle, H, W):
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    ctx = get_context()
    assert ctx.get_option("qt_chunks") == 1 and ctx.get_option("qt_chunk_run") == 0
    checked = 0
    for name, edge in edge_maps(H, W).items():
        for mn, mx in BLOCKS:
            before = chunk_launches(ctx)
            qt = A.QuadTree(edge, max_size=mx, min_size=mn)
            # min block 4 and at least 16 cells per root side (root = 2 * largest power of two <= max(H, W)) take the chunk-run kernels,
            # everything else the general ones: which set served the call is part of what is checked
            assert chunk_launches(ctx) - before == (1 if mn == 4 and qt.root_size >= 64 else 0), f"{H}x{W} blocks {mn}-{mx}: wrong kernel set"
            lo, so, ro = oracle.quadtree(edge, mn, mx)
            what = f"{H}x{W} blocks {mn}-{mx} edges '{name}'"
            assert qt.root_size == ro, what
            assert np.array_equal(qt._states, so), what + ": states"
            assert np.array_equal(qt._leaves[:, :3], lo), what + ": leaves"
            offs = np.concatenate([[0], np.cumsum(lo[:, 2].astype(np.int64) ** 2)[:-1]]) if len(lo) else np.zeros(0, np.int64)
            assert np.array_equal(qt._leaves[:, 3], offs), what + ": coefficient offsets"
            checked += 1
    assert checked >= 9 * len(BLOCKS)


def small_images(oracle, H, W):
    kinds = ("mixed", "noise", "mixed")
    return np.stack([oracle.synth_image(H, W, 700 + 13 * i + H, kinds[i]).astype(np.float32) / np.float32(255) for i in range(3)])


_refs = {}


def oracle_refs(oracle, H, W, blocks):
    """the three small images of a shape and their oracle encodes, computed once"""
    key = (H, W, blocks)
    if key not in _refs:
        x = small_images(oracle, H, W)
        _refs[key] = (x, [oracle.encode_image(x[b], "YCbCr", (40, 80), blocks) for b in range(3)])
    return _refs[key]


def check_against(enc, b, ref, what):
    for l in range(3):
        got, w = enc.layer(b, l), f"{what} image {b} layer {l}"
        assert np.array_equal(got["states"], ref[l]["states"]), w + ": states"
        assert np.array_equal(got["leaves"], ref[l]["leaves"]), w + ": leaves"
        assert np.array_equal(got["coeffs"], ref[l]["coeffs"]), w + ": coefficients"
        want = (ref[l]["coeffs"].size, len(ref[l]["leaves"]), len(ref[l]["states"]), ref[l]["root_size"])
        assert tuple(int(v) for v in enc.counts_host[b, l]) == want, w + ": counts"


@pytest.mark.parametrize("H,W", [(72, 200), (136, 260)])
@pytest.mark.parametrize("blocks", [(4, 64), (4, 128)])
def test_whole_path_batch_of_three_against_oracle(A, oracle, H, W, blocks):
    """Per-image and per-layer offsets and the work lists through the DCT, with the automatic run length (one chunk per wave at this size)."""
    x, refs = oracle_refs(oracle, H, W, blocks)
    codec = A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), blocks))
    ctx = codec._bind()
    assert ctx.get_option("qt_chunks") == 1 and ctx.get_option("qt_chunk_run") == 0
    before = chunk_launches(ctx)
    enc = codec.compress_batch(x)
    assert chunk_launches(ctx) > before, "the chunk-run kernels must have served the call"
    for b in range(3):
        check_against(enc, b, refs[b], f"{H}x{W} blocks {blocks}")


@pytest.mark.parametrize("H,W", [(72, 200), (136, 260)])
@pytest.mark.parametrize("blocks", [(4, 64), (4, 128)])
def test_runs_of_several_chunks_cross_layers_and_images(A, oracle, H, W, blocks):
    """Several chunks per wave (option "qt_chunk_run").  An image of 72 x 200 has 8 + 2 + 2 in-plane chunks, one of 136 x 260 has 15 + 6 + 6:
    runs of 2, 3, 5, 7 and 16 chunks end inside layers, cross from one layer into the next and from one image into the next, and the
    last run of the call is short (16: the front-loaded reads of the emit pass past the run's end)."""
    x, refs = oracle_refs(oracle, H, W, blocks)
    codec = A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), blocks))
    ctx = codec._bind()
    try:
        for run in (2, 3, 5, 7, 16):
            ctx.set_option("qt_chunk_run", run)
            assert ctx.get_option("qt_chunk_run") == run
            before = chunk_launches(ctx)
            enc = codec.compress_batch(x)
            assert chunk_launches(ctx) > before, "the chunk-run kernels must have served the call"
            for b in range(3):
                check_against(enc, b, refs[b], f"{H}x{W} blocks {blocks} run {run}")
    finally:
        ctx.set_option("qt_chunk_run", 0)


def test_automatic_run_length_above_one_chunk_per_wave(A, oracle):
    """200 images of 136 x 260 are 5400 in-plane chunks: the automatic run length is 2 (more than 4096 chunks), and with 15 + 6 + 6 chunks
    per image the runs cross layers and images.  The whole batch with both kernel sets, byte for byte over the used lengths, and three
    images against the oracle."""
    B, H, W = 200, 136, 260
    base, refs = oracle_refs(oracle, H, W, (4, 64))
    x = np.stack([np.roll(base[i % 3], (5 * (i // 3), 11 * (i // 3)), axis=(0, 1)) for i in range(B)])      # image i < 3 is base[i]
    codec = A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), (4, 64)))
    ctx = codec._bind()
    assert ctx.get_option("qt_chunk_run") == 0
    host = {}
    try:
        for v in (0, 1):
            ctx.set_option("qt_chunks", v)
            before = chunk_launches(ctx)
            enc = codec.compress_batch(x)
            assert (chunk_launches(ctx) > before) == (v == 1), "wrong kernel set"
            host[v] = (enc.counts_host.copy(), enc.coeffs.cpu().numpy(), enc.leaves.cpu().numpy(), enc.states.cpu().numpy())
            if v == 1:
                for b in range(3):
                    check_against(enc, b, refs[b], "batch of 200")
                p = enc.plan
    finally:
        ctx.set_option("qt_chunks", 1)
    assert host[0][0].tobytes() == host[1][0].tobytes(), "counts"
    for b in range(B):
        for l in range(3):
            n_coef, n_leaf, n_state, _ = (int(v) for v in host[1][0][b, l])
            co, lo, so = b * p.coeff_stride + p.coeff_off[l], b * p.leaf_stride + p.leaf_off[l], b * p.state_stride + p.state_off[l]
            for k, off, n in ((1, co, n_coef), (2, lo, n_leaf), (3, so, n_state)):
                assert host[0][k][off:off + n].tobytes() == host[1][k][off:off + n].tobytes(), f"image {b} layer {l} buffer {k}"


def test_the_two_kernel_sets_agree_byte_for_byte(A, oracle):
    import torch
    B, H, W = 2, 540, 960
    rng = np.random.default_rng(77)
    # blocks of random size and contrast on a noisy ground: edges at every scale, flat stretches between them
    x = np.full((B, H, W, 3), 0.5, np.float32)
    for b in range(B):
        for _ in range(400):
            y0, x0, s = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(2, 90))
            x[b, y0:y0 + s, x0:x0 + s] = rng.random(3, dtype=np.float32)
        x[b, : H // 2] += (rng.random((H // 2, W, 3), dtype=np.float32) - 0.5) * 0.2
    x = np.clip(x, 0, 1)
    codec = A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), (4, 64)))
    ctx = codec._bind()
    out = {}
    try:
        for v in (0, 1):
            ctx.set_option("qt_chunks", v)
            assert ctx.get_option("qt_chunks") == v
            before = chunk_launches(ctx)
            enc = codec.compress_batch(x)
            assert (chunk_launches(ctx) > before) == (v == 1), "wrong kernel set"
            torch.cuda.synchronize()
            out[v] = (enc.counts_host.copy(), [[enc.layer(b, l) for l in range(3)] for b in range(B)])
    finally:
        ctx.set_option("qt_chunks", 1)
    assert out[0][0].tobytes() == out[1][0].tobytes(), "counts"
    sizes = set()
    for b in range(B):
        for l in range(3):
            g0, g1 = out[0][1][b][l], out[1][1][b][l]
            for key in ("states", "leaves", "leaf_coeff_offsets", "coeffs"):
                assert g0[key].tobytes() == g1[key].tobytes(), f"image {b} layer {l}: {key}"
            sizes.update(int(s) for s in np.unique(g1["leaves"][:, 2]))
    assert sizes == {4, 8, 16, 32, 64}, "every block size must occur"
    ref = oracle.encode_image(x[1], "YCbCr", (40, 80), (4, 64))
    for l in range(3):
        assert np.array_equal(out[1][1][1][l]["states"], ref[l]["states"]) and np.array_equal(out[1][1][1][l]["leaves"], ref[l]["leaves"])
