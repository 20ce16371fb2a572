"""CPU: Pillow's ImageEnhance, ImageOps point operations, Image.point and Image.histogram without a device -- the NumPy model
(tests/adjust_reference.py) against live Pillow over the shared catalogue and over all 65 536 byte pairs of Image.blend, the wrong
variants of the model shown to differ from Pillow there, the library's host plan (aej_adjust_plan_host) against the model's, and the
interface, the C ABI and the refusals of adjust_many and histogram_many.  Every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest

import adjust_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _pil_op(im, op):
    from PIL import ImageEnhance, ImageOps
    k = op[0]
    if k in M.ENHANCERS:
        return getattr(ImageEnhance, k.capitalize())(im).enhance(op[1])
    if k == "autocontrast":
        return ImageOps.autocontrast(im, op[1], op[2], preserve_tone=op[3])
    if k == "point":
        return im.point(op[1])
    return getattr(ImageOps, k)(im, *op[1:])


def pillow(case):
    """the ops of the chain applied one after another to a PIL image"""
    from PIL import Image
    im = Image.fromarray(case[0])
    for op in M.chain_of(case[1]):
        im = _pil_op(im, op)
    return np.asarray(im)


@pytest.fixture(scope="module")
def catalogue():
    """the shared cases with Pillow's answer, computed once"""
    return [(c, pillow(c)) for c in M.catalogue()]


def _channels(a):
    return 1 if a.ndim == 2 else a.shape[2]


# ---- (a) the model is Pillow ------------------------------------------------------------------------------------------------------
def test_model_equals_pillow(catalogue):
    seen = set()
    for c, want in catalogue:
        got = M.model(c)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (c[0].shape, c[1])
        for op in M.chain_of(c[1]):
            seen.add((op[0], _channels(c[0])))
    for ch in (1, 2, 3, 4):
        assert all((k, ch) in seen for k in M.ENHANCERS + ("grayscale", "point"))
    for ch in (1, 3):
        assert all((k, ch) in seen for k in M.LUT_OPS)


def test_histogram_equals_pillow(catalogue):
    from PIL import Image
    for c, _ in catalogue[::7]:
        got = M.histogram(c[0])
        assert got.dtype == np.int64 and got.tolist() == Image.fromarray(c[0]).histogram()


def test_catalogue_covers_its_ground(catalogue):
    cases = [c for c, _ in catalogue]
    assert max(max(c[0].shape[:2]) for c in cases) <= 67
    single = [c for c in cases if isinstance(c[1][0], str)]
    chains = [c[1] for c in cases if not isinstance(c[1][0], str)]
    for kind in M.ENHANCERS:
        assert {c[1][1] for c in single if c[1][0] == kind} == set(M.FACTORS)
    assert {c[0].shape[:2] for c in single if c[1][0] == "sharpness"} == set(M.SHAPES)
    assert {(16, 16), (16, 17)} <= {c[0].shape[:2] for c in single if c[1][0] == "equalize"}
    auto = [c[1] for c in single if c[1][0] == "autocontrast"]
    assert {a[1] for a in auto} == {0, 5, (2, 10), 49.9, 60} and {a[2] for a in auto} == {None, 0, (0, 255)} and {a[3] for a in auto} == {False, True}
    assert any(c[1][0] == "autocontrast" and c[0].min() == c[0].max() for c in single)
    assert any(c[1][0] == "autocontrast" and 100 <= c[0].min() and c[0].max() <= 103 and c[0].min() < c[0].max() for c in single)
    assert {c[1][1] for c in single if c[1][0] == "posterize"} == {0, 1, 4, 8} and {c[1][1] for c in single if c[1][0] == "solarize"} == {0, 128, 100.5, 256}
    assert {_channels(c[0]) for c in single if c[1][0] == "grayscale"} == {1, 2, 3, 4}
    names = [tuple(op[0] for op in ch) for ch in chains]
    jitter = ("brightness", "contrast", "color", "sharpness")
    assert jitter in names and jitter[::-1] in names and ("contrast", "equalize") in names and ("grayscale", "equalize") in names
    assert any(n[0] == "sharpness" for n in names) and any(n[-1] == "sharpness" for n in names) and any("sharpness" in n[1:-1] for n in names)
    assert any(len(n) == 8 for n in names)
    # Equalize's identity threshold, both sides
    a16, a17 = M.image(16, 16, 1, 1), M.image(16, 17, 1, 1)
    a16[0, :2] = 255                                       # (256 - 2) // 255 == 0, while (272 - n) // 255 == 1 for any n below 18
    assert np.array_equal(M.model((a16, ("equalize",))), a16) and not np.array_equal(M.model((a17, ("equalize",))), a17)
    assert np.array_equal(pillow((a16, ("equalize",))), a16)
    # a cut-off of 60 per cent from each end empties the histogram: the identity
    assert any(c[1][0] == "autocontrast" and c[1][1] == 60 and np.array_equal(w, c[0]) for c, w in catalogue if isinstance(c[1][0], str))


@pytest.mark.parametrize("f", M.FACTORS + (2.0, -1.0))
def test_blend_model_equals_pillow_on_every_byte_pair(f):
    from PIL import Image
    d, s = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    want = np.asarray(Image.blend(Image.fromarray(d), Image.fromarray(s), f))
    assert np.array_equal(M.blend(d, s, f), want)


def test_fused_and_float64_blends_are_wrong():
    """the counts over all byte pairs: at 1.1 a fused multiply-add changes 929 of the 65 536 pairs, at -0.3 it changes 262"""
    d, s = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for f, n in ((1.1, 929), (-0.3, 262)):
        assert int((M.blend(d, s, f, fma=True) != M.blend(d, s, f)).sum()) == n
        assert (M.blend(d, s, f, f64=True) != M.blend(d, s, f)).any()


@pytest.mark.parametrize("switch", ["fma", "f64", "round_l", "mean_floor", "eq_all_bins", "alpha_zero", "sharp_border"])
def test_wrong_variant_differs_from_pillow(catalogue, switch):
    """a condition of the catalogue: every wrong variant of the model differs from Pillow on at least one of its cases"""
    differs = sum(not np.array_equal(M.model(c, **{switch: True}), want) for c, want in catalogue)
    assert differs >= 1


# ---- (b) the library's host plan ----------------------------------------------------------------------------------------------------
def test_plan_host_equals_the_model(A, catalogue):
    seen = set()
    for c, _ in catalogue:
        ch = _channels(c[0])
        p = A.adjust_plan(ch, M.library_ops(A, c[1]))
        want = M.plan_of(ch, c[1])
        assert {k: p[k] for k in want} == want and p["out_channels"] == M.channels_after(ch, c[1]), (c[1], p, want)
        seen.add((len(p["segments"]), p["passes"]))
    assert {(1, 0), (1, 1), (2, 1), (1, 2), (2, 0)} <= seen and max(s for s, _ in seen) >= 3
    jitter = A.adjust_plan(3, (A.Brightness(1.2), A.Contrast(0.8), A.Color(1.1), A.Sharpness(1.5)))
    assert jitter == dict(segments=[["brightness", "contrast", "color"], ["sharpness"]], passes=1, launches=5, out_channels=3)
    assert A.adjust_plan(1, A.Sharpness(2))["launches"] == 2 and A.adjust_plan(3, A.Invert())["launches"] == 1
    two = A.adjust_plan(1, (A.Contrast(1.3), A.Equalize()))
    assert two["passes"] == 2 and two["launches"] == 5 and len(two["segments"]) == 1      # k statistics ops: k histograms, k tables, one apply


def test_exports_and_abi(A):
    from adaptive_edge_aware_jpeg_amd import _lib, adjust
    for name in ("adjust_many", "histogram_many", "adjust_plan", "Brightness", "Contrast", "Color", "Sharpness", "AutoContrast", "Equalize", "Posterize",
                 "Solarize", "Invert", "Grayscale", "Point"):
        assert name in A.__all__ and getattr(A, name) is getattr(adjust, name), name
    header = open(os.path.join(ROOT, "include", "aej.h")).read()
    declared = set(re.findall(r"AEJ_API[^;(]*?\b(aej_(?:adjust|histogram)_\w+)\s*\(", header))
    assert declared == {"aej_adjust_geometry_host", "aej_adjust_plan_host", "aej_adjust_workspace_bytes", "aej_adjust_batch", "aej_histogram_batch"}
    assert declared == {k for k in _lib.SIGNATURES if k.startswith(("aej_adjust_", "aej_histogram_"))}
    lib = _lib.load_library()
    assert all(hasattr(lib, name) for name in declared)
    assert lib.aej_abi_version() == 3                     # entries were added: the version stays
    assert ctypes.sizeof(_lib.AdjustOp) == 64 and ctypes.sizeof(_lib.AdjustDesc) == 32 + 8 * 64 and ctypes.sizeof(_lib.AdjustPlan) == 64
    assert (_lib.AdjustOp.cutoff.offset, _lib.AdjustOp.ignore.offset, _lib.AdjustDesc.ops.offset) == (16, 32, 32)
    g = adjust.adjust_geometry()
    assert g["chunk"] % (16 * g["threads"] // 16) == 0 and g["chunk"] >= g["threads"] and g["table_bytes"] == 1024


def test_entries_without_a_context_or_buffers(A):
    """the no-context and null-pointer codes, without a device"""
    from adaptive_edge_aware_jpeg_amd import _lib
    lib = _lib.load_library()
    d = (_lib.AdjustDesc * 1)()
    p = _lib.AdjustPlan()
    assert lib.aej_adjust_geometry_host(None) == -1
    assert lib.aej_adjust_plan_host(None, ctypes.addressof(p)) == -1 and lib.aej_adjust_plan_host(ctypes.addressof(d), None) == -1
    assert lib.aej_adjust_workspace_bytes(None, ctypes.addressof(d), 1) == 0
    assert lib.aej_adjust_batch(None, ctypes.addressof(d), 1, None, 0, None, 0, None, 0, None, 0) == -1
    assert lib.aej_histogram_batch(None, ctypes.addressof(d), 1, None, 0, None, 0, None, 0) == -1
    # the plan's own refusals
    d[0].width = d[0].height = 4
    d[0].channels, d[0].n_ops = 3, 1
    d[0].ops[0].kind, d[0].ops[0].factor = 1, 1.5
    assert lib.aej_adjust_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == 0 and (p.n_passes, p.n_segments, p.n_launches, p.out_channels) == (1, 1, 3, 3)
    for field, value in (("n_ops", 0), ("n_ops", 9), ("channels", 5), ("channels", 0), ("width", 0), ("height", 32768)):
        e = (_lib.AdjustDesc * 1)()
        ctypes.memmove(e, d, ctypes.sizeof(d))
        setattr(e[0], field, value)
        assert lib.aej_adjust_plan_host(ctypes.addressof(e), ctypes.addressof(p)) == -1, (field, value)
    for kind, factor, channels in ((8, 1.0, 3), (-1, 1.0, 3), (0, float("inf"), 3), (3, float("nan"), 3), (5, 1.0, 4), (4, 1.0, 2)):
        e = (_lib.AdjustDesc * 1)()
        ctypes.memmove(e, d, ctypes.sizeof(d))
        e[0].ops[0].kind, e[0].ops[0].factor, e[0].channels = kind, factor, channels
        assert lib.aej_adjust_plan_host(ctypes.addressof(e), ctypes.addressof(p)) == -1, (kind, factor, channels)
    d[0].ops[0].kind = 4
    d[0].ops[0].cutoff[0] = -1.0
    assert lib.aej_adjust_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == -1


# ---- (c) refusals, all without a device -----------------------------------------------------------------------------------------
def test_refusals_need_no_device_and_no_library(A, monkeypatch):
    from PIL import Image

    from adaptive_edge_aware_jpeg_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("refused calls must not reach the device")

    def no_library(*a, **k):
        raise AssertionError("refused calls must not reach the library")
    monkeypatch.setattr(_lib, "get_context", no_device)
    monkeypatch.setattr(_lib, "load_library", no_library)
    rgb, rgba, la, grey = (np.zeros(s, np.uint8) for s in ((6, 7, 3), (6, 7, 4), (6, 7, 2), (6, 7)))
    J = A.adjust_many

    def refused(exc, text, fn, *args, **kw):
        with pytest.raises(exc) as e:
            fn(*args, **kw)
        assert text in str(e.value), str(e.value)

    # a _lut op on a 2- or 4-channel image: Pillow raises OSError, here ValueError naming the image
    for op in (A.AutoContrast(), A.Equalize(), A.Posterize(4), A.Solarize(), A.Invert()):
        for k, img in enumerate((la, rgba)):
            refused(ValueError, f"image 1: {type(op).__name__}: not supported for mode {'LA' if k == 0 else 'RGBA'}", J, [rgb, img], op)
            with pytest.raises(OSError):
                _pil_op(Image.fromarray(img), (type(op).__name__.lower(),) + ((4,) if isinstance(op, A.Posterize) else (0, None, False) if isinstance(op, A.AutoContrast) else ()))
    refused(ValueError, "image 0: Invert: not supported for mode RGBA", J, [rgba], (A.Brightness(1.0), A.Invert()))
    refused(ValueError, "image 0: Equalize: not supported for mode LA", J, [la], (A.Color(1.0), A.Equalize()))
    # the count after the earlier ops: Grayscale makes RGBA a 1-channel image; a 3-channel table no longer fits it
    refused(ValueError, "image 0: Point: a table of 768 entries: exactly 256", J, [rgb], (A.Grayscale(), A.Point([0] * 768)))
    refused(ValueError, "image 1: Point: a table of 256 entries: exactly 768", J, [grey, rgb], A.Point([0] * 256))
    refused(ValueError, "Point: table entries must be ints from 0 to 255", J, [grey], A.Point([0] * 255 + [256]))
    refused(ValueError, "Point: table entries must be ints from 0 to 255", J, [grey], A.Point([0.5] * 256))
    # factors
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39, -3.5e38 * 10):
        for E in (A.Brightness, A.Contrast, A.Color, A.Sharpness):
            refused(ValueError, f"image 0: {E.__name__}: factor", J, [rgb], E(bad))
    refused(ValueError, "image 1: Contrast: factor", J, [rgb, rgb], [A.Contrast(1.0), A.Contrast(float("nan"))])
    refused(ValueError, "a number required", J, [rgb], A.Color("1.0"))
    # chains
    refused(ValueError, "every image: a chain of 9 ops: at most 8", J, [rgb], (A.Invert(),) * 9)
    refused(ValueError, "image 1: a chain of 9 ops", J, [rgb, rgb], [A.Invert(), (A.Invert(),) * 9])
    refused(ValueError, "every image: an empty chain", J, [rgb], ())
    refused(ValueError, "ops: 3 entries for 2 images", J, [rgb, rgb], [A.Invert()] * 3)
    refused(TypeError, "an op of adjust.py", J, [rgb], "invert")
    refused(TypeError, "an op of adjust.py", J, [rgb], [[A.Invert(), A.Invert()]])      # a chain is a tuple; a list inside a list is not an op
    # the other arguments of the ops
    refused(ValueError, "Posterize: bits 9", J, [rgb], A.Posterize(9))
    refused(ValueError, "Posterize: bits -1", J, [rgb], A.Posterize(-1))
    refused(ValueError, "AutoContrast: cutoff", J, [rgb], A.AutoContrast(-1))
    refused(ValueError, "AutoContrast: cutoff", J, [rgb], A.AutoContrast((1, 2, 3)))
    refused(ValueError, "AutoContrast: cutoff", J, [rgb], A.AutoContrast(float("nan")))
    refused(ValueError, "AutoContrast: ignore", J, [rgb], A.AutoContrast(ignore=256))
    # not built, by name
    refused(NotImplementedError, "image 0: AutoContrast: mask= is not built", J, [rgb], A.AutoContrast(mask=grey))
    refused(NotImplementedError, "Equalize: mask= is not built", J, [rgb], A.Equalize(mask=grey))
    refused(NotImplementedError, "Colorize is not built", J, [grey], A.Colorize("black", "white"))
    refused(NotImplementedError, "Hue is not built", J, [rgb], A.Hue(0.1))
    for fn, args in ((J, (A.Invert(),)), (A.histogram_many, ())):
        refused(NotImplementedError, "image 1: images of mode 'P' are not built", fn, [rgb, Image.new("P", (4, 4))], *args)
        refused(NotImplementedError, "image 0: images of mode '1'", fn, [Image.new("1", (4, 4))], *args)
        refused(NotImplementedError, "image 0: images of mode '1'", fn, [np.zeros((4, 4), bool)], *args)
        refused(ValueError, "image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4]", fn, [rgb, np.zeros((4, 4, 5), np.uint8)], *args)
        refused(ValueError, "image 0: uint8 [H, W]", fn, [np.zeros((0, 4), np.uint8)], *args)
        refused(TypeError, "image 1: uint8 required, got float32", fn, [rgb, np.zeros((4, 4), np.float32)], *args)
        refused(ValueError, "image 0: sizes up to 32767 a side", fn, [np.zeros((1, 32768), np.uint8)], *args)
        refused(ValueError, "needs at least one image", fn, [], *args)
    # what is accepted gets as far as the device
    for ops in (A.Contrast(np.float32(1.5)), (A.Brightness(1), A.AutoContrast((2, 10), (0, 255), True)), [A.Point(list(range(256)) * 3)],
                (A.Grayscale(), A.Equalize(), A.Solarize(100.5), A.Posterize(0)), [(A.Sharpness(2), A.Invert())]):
        with pytest.raises(AssertionError, match="must not reach the device"):
            J([rgb], ops)
    with pytest.raises(AssertionError, match="must not reach the device"):
        A.histogram_many([rgba, grey])
