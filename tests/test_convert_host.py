"""CPU: Pillow's Image.convert between its 8-bit modes, convert(mode, matrix), hue adjustment and ImageOps.colorize without a device --
the NumPy model (tests/convert_reference.py) against live Pillow over the shared catalogue and over every byte triple, the route the
library reports against the one Pillow takes, aej_convert_plan_host against the Python plan, and the interface, the C ABI and the
refusals of convert_many, hue_many and colorize_many.  Every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest

import convert_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def pillow(a, target, source=None):
    from PIL import Image
    return np.asarray(Image.fromarray(a, source).convert(target))


def same(got, want):
    return got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


# ---- (a) the model is Pillow ------------------------------------------------------------------------------------------------------
def test_model_equals_pillow_on_the_catalogue():
    cases = M.mode_cases()
    assert {(s, t) for _, s, t in cases} == {(s, t) for s in M.MODES for t in M.MODES}
    assert {a.shape[:2] for a, _, _ in cases} == set(M.SIZES)
    for a, s, t in cases:
        assert same(M.convert(a, t, s), pillow(a, t, s)), (s, t, a.shape)
    for bands, mode in M.DEFAULT_MODE.items():               # the mode a channel count stands for
        a = M.random_image(np.random.default_rng(bands), 3, 5, bands)
        assert same(M.convert(a, "HSV"), pillow(a, "HSV", mode))


@pytest.mark.parametrize("source,target", [("RGB", "L"), ("RGB", "YCbCr"), ("RGB", "HSV"), ("RGB", "CMYK"), ("YCbCr", "RGB"), ("HSV", "RGB")])
def test_model_equals_pillow_on_every_byte_triple(source, target):
    a = M.all_rgb()
    if (source, target) == ("RGB", "L"):                      # the image is what its name says: pixel k is the triple k
        assert a.shape == (4096, 4096, 3) and np.array_equal(a.reshape(-1, 3).astype(np.uint32) @ np.array([65536, 256, 1], np.uint32), np.arange(1 << 24))
    assert np.count_nonzero(M.convert(a, target, source) != pillow(a, target, source)) == 0


def test_model_equals_pillow_on_every_cmyk_pair():
    a = M.all_cmyk()
    pairs = a.reshape(-1, 4)[:65536]
    assert len({(int(c), int(k)) for c, k in pairs[:, (0, 3)]}) == 65536
    assert np.count_nonzero(M.convert(a, "RGB", "CMYK") != pillow(a, "RGB", "CMYK")) == 0


@pytest.mark.parametrize("factor", M.HUE_FACTORS)
def test_hue_model_equals_the_pillow_expression(factor):
    from PIL import Image
    a = M.all_rgb()[::3, ::5]
    h, s, v = Image.fromarray(a).convert("HSV").split()
    moved = Image.fromarray(((np.asarray(h).astype(np.int64) + int(factor * 255)) & 255).astype(np.uint8))
    want = np.asarray(Image.merge("HSV", (moved, s, v)).convert("RGB"))
    assert same(M.hue(a, factor), want)
    rgba = np.concatenate([a, (a[:, :, :1] * 7 + a[:, :, 1:2]).astype(np.uint8)], axis=2)
    got = M.hue(rgba, factor)
    assert same(got[:, :, :3], want) and np.array_equal(got[:, :, 3], rgba[:, :, 3])
    grey = a[:, :, 0]
    assert same(M.hue(grey, factor), grey) and same(M.hue(a[:, :, :2], factor), np.ascontiguousarray(a[:, :, :2]))


def test_colorize_model_equals_pillow(A):
    from PIL import Image, ImageOps

    from adaptive_edge_aware_jpeg_amd.convert import colorize_table
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    noise = M.random_image(np.random.default_rng(1), 64, 61, 1)
    assert any("mid" in kw for kw in M.COLORIZE) and any("mid" not in kw for kw in M.COLORIZE)
    assert any(kw.get("blackpoint") is not None and kw.get("blackpoint") == kw.get("midpoint") for kw in M.COLORIZE)
    for kw in M.COLORIZE:
        for g in (ramp, noise):
            assert same(M.colorize(g, **kw), np.asarray(ImageOps.colorize(Image.fromarray(g), **kw))), kw
        assert colorize_table(**kw) == M.colorize_table(**kw).tobytes() and len(colorize_table(**kw)) == 768      # the library's restatement


def test_matrix_model_equals_pillow():
    from PIL import Image
    rng = np.random.default_rng(4)
    a = np.concatenate([M.random_image(rng, 96, 128, 3), M.all_rgb()[::256, ::32]])
    matrices = list(M.MATRICES)
    for k in range(200):
        n = 12 if k % 2 else 4
        m = rng.normal(0, (0.01, 1.0, 100.0)[k % 3], n)
        m[3::4] = rng.normal(0, 100, n // 4)
        if k % 5 == 0:
            m = np.round(m * 4) / 4                           # quarters: sums that tie at .5
        matrices.append(("RGB" if k % 2 else "L", tuple(float(x) for x in m)))
    assert len(matrices) >= 200 + 7
    for target, m in matrices:
        want = np.asarray(Image.fromarray(a).convert(target, m))
        assert np.count_nonzero(M.convert_matrix(a, target, m) != want) == 0, (target, m)


# ---- (b) the route, the plan and the ABI -------------------------------------------------------------------------------------------
def _pillow_has_converter(source, target):
    from PIL import Image
    try:
        Image.new(source, (2, 2)).im.convert(target, 0)
        return True
    except ValueError:
        return False


def test_plan_is_the_route_pillow_takes(A):
    from PIL import Image
    two_step = set()
    for s in M.MODES:
        for t in M.MODES:
            direct = _pillow_has_converter(s, t)
            assert direct == (t in M.DIRECT[s]), (s, t)
            p = A.convert_plan(M.BANDS[s], t, source_mode=s)
            base = Image.getmodebase(s)
            want = (f"{s}>{t}",) if direct else (f"{s}>{base}", f"{base}>{t}")
            assert p == dict(steps=want, out_channels=M.BANDS[t]), (s, t, p)
            assert tuple(f"{a}>{b}" for a, b in M.route(s, t)) == want
            if not direct:
                assert _pillow_has_converter(s, base) and _pillow_has_converter(base, t)
                two_step.add((s, t))
    assert ("CMYK", "L") in two_step and ("YCbCr", "HSV") in two_step and ("HSV", "CMYK") in two_step
    assert A.convert_plan(4, "L", source_mode="CMYK") == dict(steps=("CMYK>RGB", "RGB>L"), out_channels=1)
    assert A.convert_plan(2, "RGBA") == dict(steps=("LA>RGBA",), out_channels=4)
    assert A.convert_plan(3, "RGB") == dict(steps=("RGB>RGB",), out_channels=3)


def test_plan_host_agrees_with_the_python_plan(A):
    from adaptive_edge_aware_jpeg_amd import _lib
    from adaptive_edge_aware_jpeg_amd.convert import MODES
    assert MODES == M.MODES
    lib = _lib.load_library()
    for si, s in enumerate(MODES):
        for ti, t in enumerate(MODES):
            d, p = _lib.ConvertDesc(), _lib.ConvertPlan()
            d.width, d.height, d.channels, d.source_mode, d.target_mode = 5, 3, M.BANDS[s], si, ti
            assert lib.aej_convert_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == 0
            steps = tuple((MODES[p.step_from[k]], MODES[p.step_to[k]]) for k in range(p.n_steps))
            assert steps == M.route(s, t) and p.out_channels == M.BANDS[t]
    d, p = _lib.ConvertDesc(), _lib.ConvertPlan()
    d.width, d.height, d.channels, d.source_mode, d.target_mode, d.kind, d.hue_shift = 5, 3, 4, 3, 3, 2, 25
    assert lib.aej_convert_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == 0
    assert (p.n_steps, p.out_channels, tuple(p.step_from), tuple(p.step_to)) == (2, 4, (2, 5), (5, 2))      # RGB > HSV, HSV > RGB


def test_exports_and_abi(A):
    from adaptive_edge_aware_jpeg_amd import _lib
    from adaptive_edge_aware_jpeg_amd import convert as by_name      # (the package attribute `convert` is the colour-space function)
    import importlib
    mod = importlib.import_module("adaptive_edge_aware_jpeg_amd.convert")
    assert callable(A.convert) and by_name is A.convert and A.convert.__module__.endswith(".color")
    for name in ("convert_many", "hue_many", "colorize_many", "convert_plan"):
        assert name in A.__all__ and getattr(A, name) is getattr(mod, name), name
    header = open(os.path.join(ROOT, "include", "aej.h")).read()
    declared = set(re.findall(r"AEJ_API[^;(]*?\b(aej_convert_\w+)\s*\(", header))
    assert declared == {"aej_convert_geometry_host", "aej_convert_plan_host", "aej_convert_workspace_bytes", "aej_convert_batch"}
    assert declared == {k for k in _lib.SIGNATURES if k.startswith("aej_convert_")}
    lib = _lib.load_library()
    assert all(hasattr(lib, name) for name in declared)
    assert ctypes.sizeof(_lib.ConvertDesc) == 16 + 8 * 4 + 48 + 8 and ctypes.sizeof(_lib.ConvertPlan) == 32
    assert (_lib.ConvertDesc.width.offset, _lib.ConvertDesc.matrix.offset) == (16, 48)
    g = mod.convert_geometry()
    assert set(g) == {"chunk", "threads", "max_grid"} and g["chunk"] % (16 * g["threads"]) == 0 and g["max_grid"] >= 1


def test_entries_without_a_context_or_buffers(A):
    """the no-context and null-pointer codes and the plan's own refusals, without a device"""
    from adaptive_edge_aware_jpeg_amd import _lib
    lib = _lib.load_library()
    d = (_lib.ConvertDesc * 1)()
    p = _lib.ConvertPlan()
    assert lib.aej_convert_geometry_host(None) == -1
    assert lib.aej_convert_plan_host(None, ctypes.addressof(p)) == -1 and lib.aej_convert_plan_host(ctypes.addressof(d), None) == -1
    assert lib.aej_convert_workspace_bytes(None, ctypes.addressof(d), 1) == 0
    assert lib.aej_convert_batch(None, ctypes.addressof(d), 1, None, 0, None, 0, None, 0, None, 0) == -1
    d[0].width, d[0].height, d[0].channels, d[0].source_mode, d[0].target_mode = 4, 4, 3, 2, 0
    assert lib.aej_convert_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == 0 and (p.n_steps, p.out_channels) == (1, 1)
    for fields in (dict(width=0), dict(height=32768), dict(channels=5), dict(channels=4), dict(source_mode=-1), dict(source_mode=7), dict(target_mode=7),
                   dict(kind=4), dict(kind=-1), dict(kind=1, target_mode=5), dict(kind=2, target_mode=0), dict(kind=2, target_mode=2, hue_shift=256),
                   dict(kind=2, target_mode=2, hue_shift=-1), dict(kind=3, target_mode=2), dict(src_offset=-1), dict(dst_offset=-1)):
        e = (_lib.ConvertDesc * 1)()
        ctypes.memmove(e, d, ctypes.sizeof(d))
        for k, v in fields.items():
            setattr(e[0], k, v)
        assert lib.aej_convert_plan_host(ctypes.addressof(e), ctypes.addressof(p)) == -1, fields
    for bad in (float("inf"), float("nan")):
        d[0].kind = 1
        d[0].matrix[3] = bad
        assert lib.aej_convert_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == -1
        d[0].matrix[3], d[0].matrix[7] = 0.0, bad              # target L reads four entries only
        assert lib.aej_convert_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == 0
        d[0].target_mode = 2
        assert lib.aej_convert_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == -1
        d[0].target_mode, d[0].matrix[7] = 0, 0.0


# ---- (c) refusals, all without a device -----------------------------------------------------------------------------------------
def test_refusals_need_no_device(A, monkeypatch):
    from PIL import Image

    from adaptive_edge_aware_jpeg_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("refused calls must not reach the device")
    monkeypatch.setattr(_lib, "get_context", no_device)
    rgb, rgba, la, grey = (np.zeros(s, np.uint8) for s in ((6, 7, 3), (6, 7, 4), (6, 7, 2), (6, 7)))
    C, H, Z = A.convert_many, A.hue_many, A.colorize_many

    def refused(exc, text, fn, *args, **kw):
        with pytest.raises(exc) as e:
            fn(*args, **kw)
        assert text in str(e.value), str(e.value)

    # modes
    refused(ValueError, "every image: unknown mode 'XYZ'", C, [rgb], "XYZ")
    refused(ValueError, "image 1: unknown mode 'rgb'", C, [rgb, rgb], ["RGB", "rgb"])
    refused(ValueError, "every image: unknown mode 'BGR'", C, [rgb], "L", source_mode="BGR")
    refused(ValueError, "mode: 1 entries for 2 images", C, [rgb, rgb], ["RGB"])
    refused(ValueError, "image 1: source_mode 'CMYK' has 4 bands, the image 3 channels", C, [rgba, rgb], "RGB", source_mode="CMYK")
    refused(ValueError, "image 0: source_mode 'HSV' has 3 bands, the image 1 channels", C, [grey, rgb], "RGB", source_mode=["HSV", None])
    for m in ("1", "P", "PA", "I", "I;16", "F", "LAB", "RGBa", "La", "RGBX"):
        refused(NotImplementedError, f"every image: mode {m!r} is not built", C, [rgb], m)
    refused(NotImplementedError, "image 1: mode 'P' is not built", C, [rgb, rgb], ["L", "P"])
    for name in ("dither", "palette", "colors"):
        refused(NotImplementedError, f"every image: {name}= is not built", C, [rgb], "L", **{name: 0})
    # matrices
    refused(ValueError, "every image: a matrix of 5 entries", C, [rgb], "RGB", matrix=(1, 2, 3, 4, 5))
    refused(ValueError, "image 0: a matrix of 4 entries for target 'RGB': 12 required", C, [rgb], "RGB", matrix=(1, 0, 0, 0))
    refused(ValueError, "image 0: a matrix of 12 entries for target 'L': 4 required", C, [rgb], "L", matrix=M.XYZ)
    refused(ValueError, "image 1: a matrix takes an RGB source, not RGBA", C, [rgb, rgba], "L", matrix=(1, 0, 0, 0))
    refused(ValueError, "image 0: a matrix takes an RGB source, not HSV", C, [rgb], "L", source_mode="HSV", matrix=(1, 0, 0, 0))
    refused(ValueError, "image 0: a matrix takes the target \"L\" or \"RGB\", not 'HSV'", C, [rgb], "HSV", matrix=M.XYZ)
    refused(ValueError, "every image: a matrix entry that is not finite", C, [rgb], "L", matrix=(1, float("nan"), 0, 0))
    refused(ValueError, "image 1: a matrix entry that is not finite", C, [rgb, rgb], "L", matrix=[(1, 0, 0, 0), (1, 0, 1e39, 0)])
    refused(ValueError, "matrix: 1 entries for 2 images", C, [rgb, rgb], "L", matrix=[(1, 0, 0, 0)])
    # hue and colorize
    for f in (0.51, -0.6, float("nan"), "0.1", None):
        refused(ValueError, "every image: hue factor", H, [rgb], f)
    refused(ValueError, "image 1: hue factor 2", H, [rgb, rgb], [0.1, 2])
    refused(TypeError, "ImageColor.getrgb", Z, [grey], "black", (255, 255, 255))
    refused(TypeError, "every image: mid 'grey'", Z, [grey], (0, 0, 0), (255, 255, 255), mid="grey")
    refused(ValueError, "every image: white (255, 255, 256)", Z, [grey], (0, 0, 0), (255, 255, 256))
    refused(ValueError, "every image: black (0, 0)", Z, [grey], (0, 0), (255, 255, 255))
    refused(ValueError, "image 1: colorize takes 1-channel (L) images, got 3 channels", Z, [grey, rgb], (0, 0, 0), (255, 255, 255))
    refused(ValueError, "blackpoint <= whitepoint <= 255 required", Z, [grey], (0, 0, 0), (255, 255, 255), blackpoint=200, whitepoint=100)
    refused(ValueError, "blackpoint <= midpoint <= whitepoint <= 255 required", Z, [grey], (0, 0, 0), (255, 255, 255), mid=(1, 2, 3), midpoint=10, blackpoint=20)
    # the images, as every packed-image call refuses them
    for fn, args in ((C, ("L",)), (H, (0.1,)), (Z, ((0, 0, 0), (255, 255, 255)))):
        refused(ValueError, "needs at least one image", fn, [], *args)
        refused(TypeError, "image 1: uint8 required, got float32", fn, [grey, np.zeros((4, 4), np.float32)], *args)
        refused(ValueError, "image 0: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4]", fn, [np.zeros((4, 4, 5), np.uint8)], *args)
        refused(ValueError, "image 0: sizes up to 32767 a side", fn, [np.zeros((1, 32768), np.uint8)], *args)
        refused(TypeError, "image 0: a uint8 array or tensor required, got a PIL image", fn, [Image.new("RGB", (4, 4))], *args)
        refused(NotImplementedError, "image 1: images of mode 'P' are not built", fn, [grey, Image.new("P", (4, 4))], *args)
        refused(NotImplementedError, "image 0: images of mode '1' (bool) are not built", fn, [np.zeros((4, 4), bool)], *args)


def test_adjust_many_names_the_new_calls(A):
    grey, rgb = np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="Hue is not built.*hue_many"):
        A.adjust_many([rgb], A.Hue(0.1))
    with pytest.raises(NotImplementedError, match="Colorize is not built.*colorize_many"):
        A.adjust_many([grey], A.Colorize("black", "white"))
