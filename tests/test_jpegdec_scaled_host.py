"""CPU: the scaled JPEG decode (standard_jpeg_decode_many(..., scale=)) without a device -- the NumPy model of its arithmetic
(tests/scaled_decode_reference.py) against live Pillow, the library's reduced inverse DCTs (aej_test_jpegdec_idct_host: the function
the kernel calls, run on the CPU) against that model, draft_scale against Image.draft, and the refusals of a bad scale."""
import ctypes
import io

import numpy as np
import pytest

import scaled_decode_reference as R

SCALES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


def _picture(H, W, seed):
    """smooth colour ramps plus noise: every coefficient band is populated"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(H + W - 2, 1)], -1)
    return np.clip(base + rng.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)


# ---- (a) the model is Pillow --------------------------------------------------------------------------------------------------------
LAYOUTS = [("444", dict(subsampling=0)), ("422", dict(subsampling=1)), ("420", dict(subsampling=2)), ("grey", dict())]


@pytest.mark.parametrize("H,W", [(8, 9), (17, 33), (37, 53)])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[n for n, _ in LAYOUTS])
def test_model_equals_pillow(H, W, layout):
    Image = pytest.importorskip("PIL.Image")
    name, opts = layout
    for k, quality in enumerate((30, 92)):
        img = Image.fromarray(_picture(H, W, 100 * H + k))
        buf = io.BytesIO()
        (img.convert("L") if name == "grey" else img).save(buf, "JPEG", quality=quality, progressive=True, **opts)
        data = buf.getvalue()
        for s in SCALES:
            im = Image.open(io.BytesIO(data))
            if s > 1:
                im.draft("RGB", (W // s, H // s))
                assert im.decoderconfig == (s, 0)
            want = np.asarray(im.convert("RGB"))
            got = R.decode(data, s)
            assert got.shape == (-(-H // s), -(-W // s), 3) and np.array_equal(got, want), (name, quality, s)


# ---- (b) the library's reduced IDCTs are the model's ---------------------------------------------------------------------------------
def _lib_idct(lib, coef, qt, n):
    c = np.ascontiguousarray(coef, np.int16).reshape(64)
    q = np.ascontiguousarray(qt, np.uint16).reshape(64)
    out = np.full(n * n + 8, 0xA5, np.uint8)
    assert lib.aej_test_jpegdec_idct_host(c.ctypes.data, q.ctypes.data, n, out.ctypes.data) == 0
    assert (out[n * n:] == 0xA5).all()
    return out[:n * n].reshape(n, n)


def _blocks():
    rng = np.random.default_rng(5)
    out = []
    for k in range(40):                                            # natural-looking, dense, and full-range blocks
        amp = (4, 60, 1023, 32767)[k % 4]
        c = rng.integers(-amp, amp + 1, (8, 8))
        if k % 4 == 0:
            c[0, 0] = rng.integers(-1024, 1024)
        q = rng.integers(1, (256, 256, 256, 65536)[k % 4], (8, 8))
        out.append((c, q))
    for sign in (1, -1):                                           # saturating: every coefficient +-1023 under quantiser 255
        out.append((np.full((8, 8), sign * 1023), np.full((8, 8), 255)))
    chk = np.indices((8, 8)).sum(0) % 2 * 2 - 1
    out.append((chk * 1023, np.full((8, 8), 255)))
    return out


@pytest.mark.parametrize("n", [4, 2, 1])
def test_reduced_idct_equals_model(lib, n):
    for c, q in _blocks():
        assert np.array_equal(_lib_idct(lib, c, q, n), R.idct_reduced(c, q.reshape(64), n)), (n, c, q)


@pytest.mark.parametrize("n", [4, 2, 1])
def test_reduced_idct_ignores_row_and_column_4(lib, n):
    q = np.full((8, 8), 255)
    zero = _lib_idct(lib, np.zeros((8, 8)), q, n)
    assert (zero == 128).all()
    for k in range(8):
        for r, col in ((4, k), (k, 4)):
            c = np.zeros((8, 8), np.int64)
            c[r, col] = 1023
            assert np.array_equal(_lib_idct(lib, c, q, n), zero), (n, r, col)
            assert np.array_equal(R.idct_reduced(c, q.reshape(64), n), zero), (n, r, col)
    if n == 2:                                                     # ... and rows / columns 2 and 6 of the 2 x 2 one
        for r in (2, 6):
            c = np.zeros((8, 8), np.int64)
            c[r, 1] = c[1, r] = -1023
            assert np.array_equal(_lib_idct(lib, c, q, n), zero)


def test_idct_entry_refuses_other_sizes(lib):
    c, q, out = np.zeros(64, np.int16), np.ones(64, np.uint16), np.zeros(64, np.uint8)
    for n in (0, 3, 8, -1):
        assert lib.aej_test_jpegdec_idct_host(c.ctypes.data, q.ctypes.data, n, out.ctypes.data) == -1
    assert lib.aej_test_jpegdec_idct_host(None, q.ctypes.data, 4, out.ctypes.data) == -1


# ---- (c) draft_scale is Image.draft's choice -----------------------------------------------------------------------------------------
def test_draft_scale_equals_pillow(SJ):
    Image = pytest.importorskip("PIL.Image")
    import adaptive_edge_aware_jpeg_amd as A
    assert A.draft_scale is SJ.draft_scale
    sizes = [(1, 1), (7, 9), (16, 16), (17, 33), (64, 48), (100, 37), (255, 257), (640, 480)]
    for W, H in sizes:
        buf = io.BytesIO()
        Image.new("RGB", (W, H)).save(buf, "JPEG")
        for req in [(1, 1), (2, 3), (8, 8), (16, 5), (31, 33), (32, 32), (64, 64), (100, 100), (1000, 1)]:
            im = Image.open(io.BytesIO(buf.getvalue()))
            im.draft(None, req)
            s = im.decoderconfig[0] if im.decoderconfig else 1
            assert SJ.draft_scale(W, H, req) == s, (W, H, req)
            assert im.size == (-(-W // s), -(-H // s))


def test_draft_scale_by_rule(SJ):
    assert [SJ.draft_scale(640, 480, (w, w)) for w in (1, 60, 61, 120, 121, 240, 241, 10 ** 6)] == [8, 8, 4, 4, 2, 2, 1, 1]
    assert SJ.draft_scale(640, 16, (10, 10)) == 1 and SJ.draft_scale(3840, 2160, (256, 256)) == 8
    for bad in ((0, 10), (10, 0), (-1, 5)):
        with pytest.raises(ValueError):
            SJ.draft_scale(640, 480, bad)


# ---- (d) scale validation, before any parsing or device work -------------------------------------------------------------------------
def test_scale_validation(SJ):
    files = [b"\xff\xd8 not parsed before the scale is checked"] * 2
    for bad in (0, 3, 16, -2, True, False, 2.0, "2", None, np.bool_(True)):
        with pytest.raises(ValueError, match="scale"):
            SJ.standard_jpeg_decode_many(files, scale=bad)
        with pytest.raises(ValueError, match="scale"):
            SJ.standard_jpeg_decode_many(files, scale=[2, bad])
    with pytest.raises(ValueError, match="scale 3"):
        SJ.standard_jpeg_decode_many(files, scale=3)
    with pytest.raises(ValueError, match="scale 16"):
        SJ.standard_jpeg_decode_many(files, scale=(1, 16))
    for wrong in ([2], [2, 2, 2], (), np.array([1, 2, 4])):
        with pytest.raises(ValueError, match="for 2 files"):
            SJ.standard_jpeg_decode_many(files, scale=wrong)
    assert list(SJ._check_scales(4, 3)) == [4, 4, 4] and list(SJ._check_scales(np.array([1, 8]), 2)) == [1, 8]
    assert list(SJ._check_scales((np.int64(2), 1), 2)) == [2, 1]


# ---- (e) the C entries: present, and refusing without a device -----------------------------------------------------------------------
def test_c_entries_refuse_without_a_device(lib, SJ):
    """No context can exist on a machine without a GPU, so what can be pinned here is that the four entries are exported and that they
    refuse -- 0 bytes, AEJ_ERR_ARG -- before anything else when the context or the scales are missing; that a bad scale under a live
    context is refused with AEJ_ERR_ARG, its value in the message and no byte written is tests/test_gpu_jpegdec_scaled.py's."""
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc, JpegProgFrame, JpegProgScan
    d, f, s = JpegDecDesc(), JpegProgFrame(), JpegProgScan()
    scales = (ctypes.c_int * 1)(3)
    a = ctypes.addressof
    assert lib.aej_jpegdec_workspace_bytes_scaled(None, a(d), 1, a(scales)) == 0
    assert lib.aej_jpegprog_workspace_bytes_scaled(None, a(f), a(s), 1, a(scales)) == 0
    assert lib.aej_jpegdec_batch_scaled(None, a(d), 1, a(scales), None, 0, None, None, 0, None, None, None, 0) == -1
    assert lib.aej_jpegprog_batch_scaled(None, a(f), a(s), 1, a(scales), None, 0, None, None, 0, None, None, None, 0) == -1
    assert lib.aej_abi_version() == 3                              # additions only
