"""GPU (-m gpu): convert_many, hue_many and colorize_many against the NumPy model of tests/convert_reference.py (itself pinned to live
Pillow by test_convert_host.py): every byte triple through the colour converters, the catalogue, sizes taken from the kernel's own
geometry, the outputs read in place by the encoder, and the C entry's refusals.  The exhaustive comparisons must show zero differing
bytes."""
import ctypes
import functools
import io

import numpy as np
import pytest

import convert_reference as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as A
    return A


@pytest.fixture(scope="module")
def geometry(A):
    from adaptive_edge_aware_jpeg_amd.convert import convert_geometry
    return convert_geometry()


@functools.lru_cache(maxsize=None)
def _all_rgb():
    a = M.all_rgb()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _model(source, target):
    """the model of the exhaustive image taken as `source`, once per module"""
    m = M.convert(_all_rgb(), target, source)
    m.setflags(write=False)
    return m


@pytest.fixture(scope="module")
def all_rgb_device(A):
    import torch
    return torch.from_numpy(_all_rgb().copy()).cuda()


def differing(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape)
    return int(np.count_nonzero(got != want))


@pytest.mark.parametrize("source,target", [("RGB", "L"), ("RGB", "YCbCr"), ("RGB", "HSV"), ("RGB", "CMYK"), ("YCbCr", "RGB"), ("HSV", "RGB")])
def test_exhaustive(A, all_rgb_device, source, target):
    """one 4096 x 4096 x 3 image that holds every byte triple once"""
    (got,) = A.convert_many([all_rgb_device], target, source_mode=source)
    assert differing(got, _model(source, target)) == 0


def test_exhaustive_cmyk(A):
    """CMYK -> RGB over all 2^16 (c, k) pairs and a 64 x 64 x 64 x 4 grid of the four bands together"""
    a = M.all_cmyk()
    (got,) = A.convert_many([a], "RGB", source_mode="CMYK")
    assert differing(got, M.convert(a, "RGB", "CMYK")) == 0


@pytest.mark.parametrize("factor", M.HUE_FACTORS)
def test_hue_exhaustive(A, all_rgb_device, factor):
    """every byte triple at one factor, as RGB and as RGBA with an alpha that varies.  The model: H moved in the exhaustive HSV model,
    then looked up in the exhaustive HSV -> RGB model (pixel (h, s, v) of that image is the triple itself)"""
    import torch
    hsv = _model("RGB", "HSV").reshape(-1, 3).astype(np.int64)
    h = (hsv[:, 0] + M.hue_shift(factor)) & 255
    want = _model("HSV", "RGB").reshape(-1, 3)[(h << 16) | (hsv[:, 1] << 8) | hsv[:, 2]].reshape(4096, 4096, 3)
    small = _all_rgb()[::64, ::61]
    assert np.array_equal(M.hue(small, factor), want[::64, ::61])      # the lookup is the model
    alpha = ((torch.arange(1 << 24, device="cuda") * 37) >> 5).to(torch.uint8).reshape(4096, 4096, 1)
    rgba = torch.cat([all_rgb_device, alpha], dim=2)
    got = A.hue_many([all_rgb_device, rgba], factor)
    assert differing(got[0], want) == 0
    assert differing(got[1][:, :, :3], want) == 0
    assert torch.equal(got[1][:, :, 3:], alpha)


def test_hue_leaves_grey_modes_and_takes_a_factor_per_image(A):
    rng = np.random.default_rng(3)
    images = [M.random_image(rng, 5, 7, 1), M.random_image(rng, 9, 3, 2), M.random_image(rng, 17, 33, 3), M.random_image(rng, 64, 61, 4)]
    factors = [0.3, -0.2, 0.25, -0.45]
    got = A.hue_many(images, factors)
    for a, f, g in zip(images, factors, got):
        assert differing(g, M.hue(a, f)) == 0
    assert differing(got[0], images[0]) == 0 and differing(got[1], images[1]) == 0


def _half_on_device(images):
    import torch
    return [torch.from_numpy(a).cuda() if i % 2 else a for i, a in enumerate(images)]


def test_catalogue_one_call_per_case(A):
    cases = M.mode_cases()
    assert len({(s, t) for _, s, t in cases}) == 49
    import torch
    bad = []
    for i, (a, s, t) in enumerate(cases):
        (got,) = A.convert_many([torch.from_numpy(a).cuda() if i % 2 else a], t, source_mode=s)
        if differing(got, M.convert(a, t, s)):
            bad.append((s, t, a.shape))
    assert bad == []


def test_catalogue_mixed_in_one_call(A):
    """all cases in one call, a list of targets and of source modes (None where the channel count says it), half from the device"""
    cases = M.mode_cases()
    sources = [None if s == M.DEFAULT_MODE[M.BANDS[s]] else s for _, s, _ in cases]
    got = A.convert_many(_half_on_device([a for a, _, _ in cases]), [t for _, _, t in cases], source_mode=sources)
    assert [(s, t, a.shape) for (a, s, t), g in zip(cases, got) if differing(g, M.convert(a, t, s))] == []
    storage = {g.untyped_storage().data_ptr() for g in got}
    assert len(storage) == 1                                   # one packed allocation


def test_matrices_and_colorize(A):
    rng = np.random.default_rng(11)
    a, b = M.random_image(rng, 64, 61, 3), M.random_image(rng, 17, 33, 3)
    for target, m in M.MATRICES:
        got = A.convert_many([a, b], target, matrix=m)
        assert differing(got[0], M.convert_matrix(a, target, m)) == 0 and differing(got[1], M.convert_matrix(b, target, m)) == 0
    rgb_ms = [m for t, m in M.MATRICES if t == "RGB"]
    got = A.convert_many([a] * len(rgb_ms), "RGB", matrix=list(rgb_ms))      # a matrix per image
    for g, m in zip(got, rgb_ms):
        assert differing(g, M.convert_matrix(a, "RGB", m)) == 0
    greys = [np.arange(256, dtype=np.uint8).reshape(16, 16), M.random_image(rng, 64, 61, 1), M.random_image(rng, 1, 1, 1)]
    for kw in M.COLORIZE:
        got = A.colorize_many(_half_on_device(greys), **kw)
        for g, grey in zip(got, greys):
            assert differing(g, M.colorize(grey, **kw)) == 0


def test_lane_groups_and_tails(A, geometry):
    """for each channel count, images of k * lane_pixels + j pixels for every j, of one pixel, and around a workgroup's sweep and a
    chunk, all views into ONE packed source in which every image starts at an odd offset; to every output channel count and HSV"""
    import torch
    rng = np.random.default_rng(7)
    images, targets, sources = [], [], []
    for c in (1, 2, 3, 4):
        lane = {1: 16, 2: 8, 3: 4, 4: 4}[c]
        sizes = [1] + [2 * lane + j for j in range(lane)] + [geometry["threads"] * lane - 1, geometry["chunk"] - 1, geometry["chunk"], geometry["chunk"] + 1]
        for n in sizes:
            a = M.random_image(rng, 1, n, c)
            for t in ("L", "LA", "HSV", "CMYK") + (("YCbCr",) if n < 64 else ()):
                images.append(a)
                targets.append(t)
                sources.append("CMYK" if c == 4 and n % 2 else None)
    nbytes = [a.size + a.size % 2 for a in images]            # an even number of bytes on from an odd start: every image starts odd
    starts = 1 + np.concatenate([[0], np.cumsum(nbytes)[:-1]])
    packed = torch.zeros(int(starts[-1] + nbytes[-1]), dtype=torch.uint8, device="cuda")
    views = []
    for a, s in zip(images, starts):
        v = packed[int(s):int(s) + a.size].view(*a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 2 == (packed.data_ptr() + 1) % 2
        views.append(v)
    got = A.convert_many(views, targets, source_mode=sources)
    bad = [(a.shape, s, t) for a, s, t, g in zip(images, sources, targets, got) if differing(g, M.convert(a, t, s))]
    assert bad == []


def test_more_chunks_than_the_grid(A, geometry):
    """more chunks in one launch than the largest grid, so that workgroups stride to a second chunk: max_grid + 37 images of one to
    three pixels (every image is at least a chunk), and with them an image that spans several chunks.  The conversion is per pixel, so
    the model runs once on all pixels together"""
    import torch
    n = geometry["max_grid"] + 37
    rng = np.random.default_rng(5)
    widths = 1 + np.arange(n) % 3
    pixels = rng.integers(0, 256, (int(widths.sum()), 1, 3), dtype=np.uint8)
    ends = np.cumsum(widths)
    images = [pixels[e - w:e].reshape(1, w, 3) for w, e in zip(widths, ends)]
    long = M.random_image(rng, 1, 3 * geometry["chunk"] + 5, 3)
    got = A.convert_many(images + [long], "HSV")
    assert len(got) == n + 1
    flat = torch.cat([g.reshape(-1) for g in got[:n]]).cpu().numpy()
    assert np.array_equal(flat, M.convert(pixels, "HSV").reshape(-1))
    assert differing(got[n], M.convert(long, "HSV")) == 0


def test_outputs_feed_the_encoder_in_place(A):
    """convert_many(rgba, "RGB") -> standard_jpeg_encode_many gives Pillow's file; a CMYK decode converted with source_mode="CMYK"
    equals the library's own [H, W, 3] decode of that file"""
    from PIL import Image
    import test_gpu_jpeg_adobe as TA
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:47, 0:61]
    rgba = np.stack([(xx * 4) & 255, (yy * 5) & 255, (xx + yy) & 255, rng.integers(0, 256, (47, 61))], axis=2).astype(np.uint8)
    (rgb,) = A.convert_many([rgba], "RGB")
    assert differing(rgb, rgba[:, :, :3]) == 0
    (jpg,) = A.standard_jpeg_encode_many([rgb], 85)
    buf = io.BytesIO()
    Image.fromarray(rgba, "RGBA").convert("RGB").save(buf, "JPEG", quality=85)
    assert jpg == buf.getvalue()
    files = [TA._file("cmyk_2x2k")]
    (cmyk,) = A.standard_jpeg_decode_many(files, adobe=True, mode="auto")
    assert cmyk.shape[2] == 4
    (want,) = A.standard_jpeg_decode_many(files, adobe=True, mode="RGB")
    (got,) = A.convert_many([cmyk], "RGB", source_mode="CMYK")
    assert differing(got, want.cpu().numpy()) == 0


def test_c_entry_refusals_and_untouched_bytes(A):
    """aej_convert_batch itself: exactly the image's bytes written; workspace too small, bad spans, n < 1, and a bad mode in one
    descriptor of several, each with its code and text and with the output untouched"""
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import ConvertDesc, get_context
    ctx = get_context(0)
    lib = ctx.lib
    rng = np.random.default_rng(2)
    a = M.random_image(rng, 20, 30, 3)
    n = a.size
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:n] = torch.from_numpy(a).cuda().reshape(-1)
    d = (ConvertDesc * 3)()
    m = 30 * 20 * 4
    for k in range(3):
        d[k].src_offset, d[k].dst_offset, d[k].width, d[k].height, d[k].channels = 0, 32 + k * m, 30, 20, 3
        d[k].source_mode, d[k].target_mode, d[k].kind = 2, 6, 0          # RGB -> CMYK
    total = 32 + 3 * m + 64
    dst = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    nws = int(lib.aej_convert_workspace_bytes(ctx.handle, ctypes.addressof(d), 3))
    assert nws > 0
    ws = ctx.workspace(max(nws, 256))

    def call(count, src_ptr, sb, dst_ptr, db, wsb, n_tables=0):
        rc = lib.aej_convert_batch(ctx.handle, ctypes.addressof(d), count, None, n_tables, src_ptr, ctypes.c_uint64(sb), dst_ptr, ctypes.c_uint64(db),
                                   ws.data_ptr(), ctypes.c_uint64(wsb))
        return rc, lib.aej_last_error(ctx.handle)

    def untouched():
        torch.cuda.synchronize()
        return bool((dst == 0xA5).all())

    rc, msg = call(3, buf.data_ptr(), n, dst.data_ptr(), total, nws - 1)
    assert rc == -4 and b"workspace too small" in msg
    rc, msg = call(3, buf.data_ptr(), n - 1, dst.data_ptr(), total, ws.numel())
    assert rc == -1 and b"image 0: source outside the input" in msg
    rc, msg = call(3, buf.data_ptr(), n, dst.data_ptr(), 32 + 3 * m - 1, ws.numel())
    assert rc == -1 and b"image 2: image outside the output" in msg
    rc, msg = call(1, buf.data_ptr(), n, buf.data_ptr() + n - 1, total, ws.numel())
    assert rc == -1 and b"image 0: source inside the output" in msg
    for count in (0, -1):
        rc, msg = call(count, buf.data_ptr(), n, dst.data_ptr(), total, ws.numel())
        assert rc == -1 and b"no images" in msg
    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), total, ws.numel(), n_tables=1)
    assert rc == -1 and b"NULL buffer" in msg
    for field, value, text in (("target_mode", 7, b"image 1: unknown mode"), ("source_mode", 3, b"image 1: a source mode whose bands are not the image's channels"),
                               ("kind", 4, b"image 1: unknown kind"), ("kind", 3, b"image 1: a colorize table takes L and leaves RGB"),
                               ("kind", 2, b"image 1: a hue shift takes RGB or RGBA and leaves the same")):
        old = getattr(d[1], field)
        setattr(d[1], field, value)
        rc, msg = call(3, buf.data_ptr(), n, dst.data_ptr(), total, ws.numel())
        assert rc == -1 and text in msg, msg
        assert lib.aej_convert_workspace_bytes(ctx.handle, ctypes.addressof(d), 3) == 0
        setattr(d[1], field, old)
    assert untouched()                                         # every refused call left the output as it was
    rc, msg = call(3, buf.data_ptr(), n, dst.data_ptr(), total, ws.numel())
    assert rc == 0, msg
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    want = M.convert(a, "CMYK")
    for k in range(3):
        assert np.array_equal(out[32 + k * m:32 + (k + 1) * m].reshape(20, 30, 4), want)
    assert (out[:32] == 0xA5).all() and (out[32 + 3 * m:] == 0xA5).all()
