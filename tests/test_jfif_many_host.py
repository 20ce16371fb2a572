"""The ragged JPEG encoder on the host side (no GPU needed): aej_jfif_many_coefs_host -- the index mapping and arithmetic the kernel
k_jm_coefs runs (csrc/jfif_many_core.h, csrc/jfif_arith.h) -- against the quantised coefficients of the numpy model, the argument checks
of standard_jpeg_encode_many and standard_jpeg_thumbnail_jpeg_many, and the refusals of the ABI entries."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_options_reference as O  # noqa: E402
import jfif_reference as R  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
from adaptive_edge_aware_jpeg_amd import standard_jpeg as S  # noqa: E402
from adaptive_edge_aware_jpeg_amd._lib import AEJ_ERR_ARG, SIGNATURES, JfifManyDesc, load_library  # noqa: E402

LAYOUTS = ("4:4:4", "4:2:2", "4:2:0")
QUALITIES = (1, 50, 75, 100)
SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 53), (1, 64), (64, 1), (2, 2), (3, 5)]      # (H, W)
AEJ_ERR_CAPACITY = -4


def _image(h, w, seed):
    """noise over a gradient: every coefficient is exercised and the edge pixels differ from their neighbours"""
    rng = np.random.default_rng(seed)
    ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5)[:, :, None] % 256
    return ((rng.integers(0, 256, (h, w, 3)) + ramp) // 2).astype(np.uint8)


def _coefs(lib, x, q, ss):
    h, w = x.shape[:2]
    n = lib.aej_jfif_many_coefs_host(w, h, q, ss, None, None, 0)
    assert n > 0
    out = np.full((n + 1, 64), 12345, np.int16)                      # one guard block behind
    x = np.ascontiguousarray(x)
    assert lib.aej_jfif_many_coefs_host(w, h, q, ss, x.ctypes.data, out.ctypes.data, n) == n
    assert (out[n] == 12345).all()
    return out[:n]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H,W", SIZES)
def test_coefs_host_equal_the_numpy_model(H, W, layout):
    lib = load_library()
    ss = S.SUBSAMPLING[layout]
    hs, vs = O.FACTORS[ss]
    x = _image(H, W, 31 * H + W)
    for q in QUALITIES:
        want = O.coefficients(x, q, ss)
        got = _coefs(lib, x, q, ss)
        assert len(want) == got.shape[0] == (hs * vs + 2) * (-(-H // (8 * vs))) * (-(-W // (8 * hs)))
        assert np.array_equal(got, np.array([b for _, b in want], np.int64)), (H, W, layout, q)
        if ss == 2:
            assert np.array_equal(got, np.array([b for _, b in R.coefficients(x, q)], np.int64))


def test_dummy_blocks_follow_libjpeg():
    """17 x 33 at 4:2:0: two MCU rows of three MCUs, the real luma grid 3 x 5 blocks: the right column of the last MCU of a row and the
    bottom row of the second MCU row are dummies -- AC zero, DC that of the block before in the MCU"""
    lib = load_library()
    x = _image(17, 33, 5)
    c = _coefs(lib, x, 90, 2).reshape(2, 3, 6, 64)
    for my in range(2):
        for mx in range(3):
            for k in range(4):
                real = 2 * my + k // 2 < 3 and 2 * mx + k % 2 < 5
                if not real:
                    assert k > 0 and (c[my, mx, k, 1:] == 0).all() and c[my, mx, k, 0] == c[my, mx, k - 1, 0], (my, mx, k)
    assert (c[1, 2, 1:4, 1:] == 0).all() and (c[1, 2, 1:4, 0] == c[1, 2, 0, 0]).all()      # the corner MCU: one real block
    assert c[0, 0, :4, 1:].any(axis=1).all()                         # and the real ones are not empty


def test_coefs_host_refusals():
    lib = load_library()
    x = np.zeros((8, 8, 3), np.uint8)
    out = np.zeros((6, 64), np.int16)
    assert lib.aej_jfif_many_coefs_host(8, 8, 75, 2, x.ctypes.data, out.ctypes.data, 6) == 6
    assert lib.aej_jfif_many_coefs_host(8, 8, 75, 2, x.ctypes.data, out.ctypes.data, 5) == AEJ_ERR_CAPACITY
    for args in ((0, 8, 75, 2), (8, 65536, 75, 2), (8, 8, 0, 2), (8, 8, 101, 2), (8, 8, 75, 3), (8, 8, 75, -1)):
        assert lib.aej_jfif_many_coefs_host(*args, x.ctypes.data, out.ctypes.data, 6) == AEJ_ERR_ARG, args
    assert lib.aej_jfif_many_coefs_host(8, 8, 75, 2, x.ctypes.data, None, 6) == AEJ_ERR_ARG
    assert lib.aej_jfif_many_coefs_host(65535, 65535, 75, 0, None, None, 0) == 3 * 8192 * 8192


def _descs(rows):
    return (JfifManyDesc * len(rows))(*[JfifManyDesc(o, w, h, q, 0) for o, w, h, q in rows])


def test_abi_symbols_and_workspace_refusals():
    lib = load_library()
    for name in ("aej_jfif_many_workspace_bytes", "aej_jfif_many_encode", "aej_jfif_many_coefs_host"):
        assert name in SIGNATURES and hasattr(lib, name)
    assert lib.aej_abi_version() == 3
    good = [(0, 33, 17, 75), (33 * 17 * 3, 8, 8, 1), (0, 33, 17, 100)]

    def size(rows, ss=2, opt=0, prog=0):
        d = _descs(rows)                                             # (kept alive over the call)
        return lib.aej_jfif_many_workspace_bytes(None, ctypes.addressof(d), len(rows), ss, opt, prog)

    base = size(good)
    assert base > 0 and size(good, 0) > base and size(good, 2, 1) > 0 and size(good, 2, 0, 1) > 0
    assert size(good + good) > base                                  # more images of the same sizes: more slots
    for bad in ((0, 0, 17, 75), (0, 33, 65536, 75), (0, 33, 17, 0), (0, 33, 17, 101)):
        for at in range(3):
            rows = list(good)
            rows[at] = bad
            assert size(rows) == 0, (bad, at)
    assert size(good, 3) == 0 and size(good, -1) == 0 and size(good, 2, 2) == 0 and size(good, 2, 0, 2) == 0
    assert lib.aej_jfif_many_workspace_bytes(None, None, 1, 2, 0, 0) == 0
    d = _descs(good)
    assert lib.aej_jfif_many_workspace_bytes(None, ctypes.addressof(d), 0, 2, 0, 0) == 0
    # without a context the encode entry refuses at once, as every entry does
    assert lib.aej_jfif_many_encode(None, ctypes.addressof(d), 3, None, 0, 2, 0, 0, None, 0, None, None, None, None, None, 0) == AEJ_ERR_ARG


@pytest.fixture()
def no_context(monkeypatch):
    """any attempt to reach a device context fails the test"""
    def boom(*a, **k):
        raise AssertionError("a device context was asked for before the arguments were checked")
    monkeypatch.setattr(S, "get_context", boom)


def test_encode_many_checks_arguments_before_any_device_work(no_context):
    ok = np.zeros((4, 5, 3), np.uint8)
    for images in ([], (), "abc", np.zeros((2, 4, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            A.standard_jpeg_encode_many(images)
    for bad in (np.zeros((4, 5), np.uint8), np.zeros((4, 5, 4), np.uint8), np.zeros((0, 5, 3), np.uint8), np.zeros((1, 4, 5, 3), np.uint8)):
        with pytest.raises(ValueError, match="image 1"):
            A.standard_jpeg_encode_many([ok, bad])
    for bad in (np.zeros((4, 5, 3), np.float64), np.zeros((4, 5, 3), np.int16), np.zeros((4, 5, 3), bool)):
        with pytest.raises(TypeError, match="image 2"):
            A.standard_jpeg_encode_many([ok, ok, bad])
    for q in (0, 101, 7.5, True, "75"):
        with pytest.raises(ValueError):
            A.standard_jpeg_encode_many([ok], quality=q)
        with pytest.raises(ValueError, match="image 1"):
            A.standard_jpeg_encode_many([ok, ok], quality=[75, q])
    for q in ([75], [75, 75, 75], []):
        with pytest.raises(ValueError, match="2 images"):
            A.standard_jpeg_encode_many([ok, ok], quality=q)
    with pytest.raises(ValueError):
        A.standard_jpeg_encode_many([ok], subsampling="4:1:1")
    import torch
    t = torch.zeros((4, 5, 3), dtype=torch.uint8)
    t.jpeg_comment = "text"                                          # bytes required
    with pytest.raises(TypeError, match="image 1"):
        A.standard_jpeg_encode_many([ok, t])
    for kw in ({"optimize": 1}, {"progressive": 0}, {"optimize": "yes"}):
        with pytest.raises(TypeError):
            A.standard_jpeg_encode_many([ok], **kw)


def test_thumbnail_jpeg_many_checks_arguments_before_any_device_work(no_context):
    from conftest import GOLDEN
    d = os.path.join(GOLDEN, "jpegdec")
    name = sorted(f for f in os.listdir(d) if f.endswith(".jpg"))[0]
    with open(os.path.join(d, name), "rb") as f:
        jpg = f.read()
    with pytest.raises(ValueError):
        A.standard_jpeg_thumbnail_jpeg_many([], (64, 64))
    for q in (0, 101, True):
        with pytest.raises(ValueError):
            A.standard_jpeg_thumbnail_jpeg_many([jpg], (64, 64), quality=q)
    with pytest.raises(ValueError, match="file 1"):
        A.standard_jpeg_thumbnail_jpeg_many([jpg, jpg], (64, 64), quality=[80, 0])
    with pytest.raises(ValueError, match="2 files"):
        A.standard_jpeg_thumbnail_jpeg_many([jpg, jpg], (64, 64), quality=[80])
    with pytest.raises(ValueError):
        A.standard_jpeg_thumbnail_jpeg_many([jpg], (64, 64), subsampling=5)
    for kw in ({"optimize": 1}, {"progressive_out": 1}):
        with pytest.raises(TypeError):
            A.standard_jpeg_thumbnail_jpeg_many([jpg], (64, 64), **kw)
    with pytest.raises(ValueError):
        A.standard_jpeg_thumbnail_jpeg_many([jpg], (0, 64))          # the thumbnail's own checks, still on the host
    with pytest.raises(ValueError, match="file 1"):
        A.standard_jpeg_thumbnail_jpeg_many([jpg, jpg[:100]], (64, 64))
