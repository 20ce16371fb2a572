"""CPU: Pillow's Image.transform, rotate and transpose without a device -- the NumPy model (tests/warp_reference.py) against live Pillow
over the shared catalogue, the wrong variants of the model shown to differ from Pillow there, the library's host plan
(aej_warp_plan_host: the fixed-point constants, the guard, the running-sum tables) against the model's, and the interface, the C ABI
and the refusals of transform_many, rotate_many and transpose_many."""
import ctypes
import os
import re

import numpy as np
import pytest

import warp_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def catalogue():
    """the shared cases with Pillow's answer, computed once"""
    return [(c, M.pillow(c)) for c in M.catalogue()]


def _channels(a):
    return 1 if a.ndim == 2 else a.shape[2]


# ---- (a) the model is Pillow ------------------------------------------------------------------------------------------------------
def test_model_equals_pillow(catalogue):
    seen = set()
    for c, want in catalogue:
        got = M.model(c)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (c[0], c[1].shape, c[2])
        seen.add((c[0], c[2].get("method"), c[2].get("resample"), _channels(c[1])))
    for ch in (1, 2, 3, 4):
        for f in (0, 2, 3):
            assert all(("transform", m, f, ch) in seen for m in (M.AFFINE, M.EXTENT, M.PERSPECTIVE, M.QUAD)) and ("rotate", None, f, ch) in seen
        assert all(("transpose", m, None, ch) in seen for m in M.TRANSPOSE_NAMES)


def test_catalogue_holds_what_tells_the_variants_apart(catalogue):
    cases = [c for c, _ in catalogue]
    assert max(max(c[1].shape[:2]) for c in cases) <= 70 and max(max(w.shape[:2]) for _, w in catalogue) <= 75
    tf = [c for c in cases if c[0] == "transform"]
    assert any(c[2]["data"][:2] == (1 / 3, 0.7) and min(c[2]["size"]) >= 60 for c in tf)                  # 16.16 cannot hold them, over 60 pixels and more
    assert any(c[2]["data"] == (0.1, 0, 0.25, 0, 0.1, 0.25) and min(c[2]["size"]) >= 60 for c in tf)      # the step of 0.1 from 0.25
    for c in cases:
        if _channels(c[1]) in (2, 4):
            alpha = c[1][..., -1]
            assert ((alpha > 0) & (alpha < 255)).any() and (alpha == 0).any() and (alpha == 255).any()
    rot = [c[2] for c in cases if c[0] == "rotate"]
    assert any(k.get("expand") for k in rot) and any(k.get("center") for k in rot) and any(k.get("translate") for k in rot)
    assert {0, 90, 180, 270, 360, -180, 450} <= {k["angle"] for k in rot} and any(k["fillcolor"] is not None for k in rot)
    paths = {M.nearest_path(*M.coefficients(c[2]["method"], c[2]["data"], *c[2]["size"]), *c[2]["size"]) for c in tf if c[2]["resample"] == 0}
    assert paths == {"tables", "fixed", "generic"}


@pytest.mark.parametrize("switch", [dict(half=False), dict(f32=True), dict(round_result=True), dict(generic_nearest=True), dict(direct_tables=True),
                                    dict(premultiply=False), dict(premul_fill=True)], ids=lambda s: next(iter(s)))
def test_wrong_variant_differs_from_pillow(catalogue, switch):
    """a condition of the catalogue: every wrong variant of the model differs from Pillow on at least one of its cases"""
    differs = 0
    for c, want in catalogue:
        if c[0] != "transpose":
            got = M.model(c, **switch)
            differs += got.shape != want.shape or not np.array_equal(got, want)
    assert differs >= 1


def test_running_sum_tables_are_not_a_product():
    """step 0.1 from offset 0.25 over 3840 entries: the running sum and a0 (x + 0.5) + a2 disagree in 241 places"""
    a = (0.1, 0, 0.25, 0, 0.1, 0.25)
    (x1, _), (x2, _) = M.scale_tables(a, 3840, 1), M.scale_tables(a, 3840, 1, direct=True)
    assert int((x1 != x2).sum()) == 241


# ---- (b) the library's host plan ----------------------------------------------------------------------------------------------------
def test_plan_host_equals_the_model(A, catalogue):
    """aej_warp_plan_host through transform_plan: the path, A0 .. A5 and the two tables of every transform case of the catalogue"""
    seen = set()
    for c, _ in catalogue:
        if c[0] != "transform":
            continue
        kw, (H, W), ch = c[2], c[1].shape[:2], _channels(c[1])
        w, h = kw["size"]
        p = A.transform_plan(W, H, kw["size"], kw["method"], kw["data"], kw["resample"], channels=ch)
        kind, co = M.coefficients(kw["method"], kw["data"], w, h)
        assert p["coefficients"] == co and p["premultiply"] == (ch in (2, 4) and kw["resample"] != 0)
        want = kind
        if kw["resample"] == 0 and kind == M.AFFINE:
            want = M.nearest_path(kind, co, w, h)
        assert p["path"] == want, (kw, p["path"], want)
        seen.add(want)
        assert (p["fixed"] == M.fixed_constants(co)) if want == "fixed" else p["fixed"] is None
        if want == "tables":
            xt, yt = M.scale_tables(co, w, h)
            assert p["xtab"].dtype == np.int32 and np.array_equal(p["xtab"], xt) and np.array_equal(p["ytab"], yt)
        else:
            assert p["xtab"] is None and p["ytab"] is None
    assert seen == {"tables", "fixed", "affine", "perspective", "quad"}
    assert A.transform_plan(5, 5, (4, 4), "affine", (1, 0, 0, 0, 1, 0), "bicubic", channels=4, premultiply=False)["premultiply"] is False
    # a long table: 3840 entries by running sums, -1 where the sum is negative or beyond an int
    p = A.transform_plan(100, 100, (3840, 3), "affine", (0.1, 0, 0.25, 0, -1e12, 5e11), 0)
    assert np.array_equal(p["xtab"], M.scale_tables((0.1, 0, 0.25, 0, -1e12, 5e11), 3840, 3)[0]) and p["ytab"].tolist() == [0, -1, -1]
    assert A.transform_plan(9, 9, (2, 3), "affine", (1e300, 0, 0, 0, 5e9, 0), 0)["ytab"].tolist() == [-1, -1, -1]


def test_fixed_point_guard(A):
    """Pillow leaves 16.16 once a corner coordinate reaches 32768: refused, naming the image; just below it is taken"""
    lib_ok = A.transform_plan(10, 10, (100, 50), "affine", (327.0, 0.5, 40.0, 0.25, 1.0, 0.0), "nearest")
    assert lib_ok["path"] == "fixed" and lib_ok["fixed"] == M.fixed_constants((327.0, 0.5, 40.0, 0.25, 1.0, 0.0))
    for data, size in (((327.0, 0.5, 70.0, 0.25, 1.0, 0.0), (100, 50)), ((1.0, 0.5, 0.0, 0.25, 1.0, -32768.0), (10, 10)), ((1.0, 1e-9, 32768.0, 0.0, 1.0, 0.0), (1, 1)),
                       ((40000.0, 1.0, -39000.0, 0.0, 1.0, 0.0), (1, 1))):
        assert not M.fixed_guard(data, *size) or abs(M.fix(data[0])) >= 2 ** 31
        with pytest.raises(NotImplementedError, match="transform_plan: .*32768"):
            A.transform_plan(10, 10, size, "affine", data, "nearest")
        assert A.transform_plan(10, 10, size, "affine", data, "bilinear")["path"] == "affine"      # only NEAREST has the guard
    img = np.zeros((10, 10), np.uint8)
    with pytest.raises(NotImplementedError, match="image 1: .*32768"):
        A.transform_many([img, img], (100, 50), "affine", [(1, 0, 0, 0, 1, 0), (327.0, 0.5, 70.0, 0.25, 1.0, 0.0)])


def test_rotate_restated(A):
    """geometry._rotate is Image.rotate's matrix and size, value for value"""
    from adaptive_edge_aware_jpeg_amd import geometry as G
    rng = np.random.default_rng(3)
    for k in range(300):
        W, H = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        angle = [float(rng.uniform(-400, 400)), int(rng.integers(-8, 9)) * 45, int(rng.integers(-4, 5)) * 90][k % 3]
        expand = bool(k & 1)
        center = None if k % 5 else (float(rng.uniform(0, W)), int(rng.integers(0, H + 1)))
        translate = None if k % 7 else (int(rng.integers(-5, 6)), float(rng.uniform(-5, 5)))
        assert G._rotate(W, H, angle, expand, center, translate) == M.rotate_plan(W, H, angle, expand, center, translate)


# ---- (c) interface and ABI --------------------------------------------------------------------------------------------------------
def test_exports_and_abi(A):
    from adaptive_edge_aware_jpeg_amd import _lib, geometry
    for name in ("transform_many", "rotate_many", "transpose_many", "transform_plan"):
        assert name in A.__all__ and getattr(A, name) is getattr(geometry, name), name
    header = open(os.path.join(ROOT, "include", "aej.h")).read()
    declared = set(re.findall(r"AEJ_API[^;(]*?\b(aej_warp_\w+)\s*\(", header))
    assert declared == {"aej_warp_geometry_host", "aej_warp_plan_host", "aej_warp_workspace_bytes", "aej_warp_batch"}
    assert declared <= set(_lib.SIGNATURES)
    lib = _lib.load_library()
    assert all(hasattr(lib, name) for name in declared)
    assert lib.aej_abi_version() == 3                     # entries were added: the version stays
    assert ctypes.sizeof(_lib.WarpDesc) == 128 and ctypes.sizeof(_lib.WarpPlan) == 56 and ctypes.sizeof(_lib.WindowDesc) == 152
    assert (_lib.WarpDesc.coef.offset, _lib.WarpDesc.fill.offset, _lib.WarpDesc.premultiply.offset, _lib.WarpPlan.fixed.offset) == (48, 112, 116, 8)
    d = (_lib.WarpDesc * 1)()
    assert lib.aej_warp_workspace_bytes(None, ctypes.addressof(d), 1) == 0      # no context: nothing to size
    p = _lib.WarpPlan()
    assert lib.aej_warp_plan_host(None, ctypes.addressof(p), None, 0) == -1 and lib.aej_warp_plan_host(ctypes.addressof(d), None, None, 0) == -1
    d[0].src_w = d[0].src_h = d[0].dst_w = d[0].dst_h = 4
    d[0].channels, d[0].path = 3, 3                        # AEJ_WARP_AFFINE under NEAREST, a pure scale: the tables need room
    d[0].coef[0] = d[0].coef[4] = 1.0
    tab = (ctypes.c_int32 * 8)()
    assert lib.aej_warp_plan_host(ctypes.addressof(d), ctypes.addressof(p), ctypes.addressof(tab), 7) == -4
    assert lib.aej_warp_plan_host(ctypes.addressof(d), ctypes.addressof(p), None, 0) == -4
    assert lib.aej_warp_plan_host(ctypes.addressof(d), ctypes.addressof(p), ctypes.addressof(tab), 8) == 0 and p.path == 1 and list(tab) == [0, 1, 2, 3] * 2
    for field, value in (("path", 1), ("path", 2), ("path", 6), ("filter", 1), ("filter", 4), ("channels", 5), ("src_w", 0), ("dst_h", 32768)):
        e = (_lib.WarpDesc * 1)()
        ctypes.memmove(e, d, ctypes.sizeof(d))
        setattr(e[0], field, value)
        assert lib.aej_warp_plan_host(ctypes.addressof(e), ctypes.addressof(p), ctypes.addressof(tab), 8) == -1, (field, value)
    d[0].path, d[0].method = 0, 2                          # AEJ_WARP_TRANSPOSE: ROTATE_90 of a square fits, method 7 does not exist
    assert lib.aej_warp_plan_host(ctypes.addressof(d), ctypes.addressof(p), None, 0) == 0 and p.path == 0
    d[0].dst_w = 5
    assert lib.aej_warp_plan_host(ctypes.addressof(d), ctypes.addressof(p), None, 0) == -1
    d[0].dst_w, d[0].method = 4, 7
    assert lib.aej_warp_plan_host(ctypes.addressof(d), ctypes.addressof(p), None, 0) == -1
    g = geometry.warp_geometry()
    assert (g["tile_w"], g["tile_h"]) == (32, 8) and g["flip_bytes"] % 4 == 0 and g["swap_w"] == g["swap_h"]


# ---- (d) refusals, all without a device -----------------------------------------------------------------------------------------
def test_refusals_need_no_device(A, monkeypatch):
    from PIL import Image

    from adaptive_edge_aware_jpeg_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("refused calls must not reach the device")
    monkeypatch.setattr(_lib, "get_context", no_device)
    img = np.zeros((6, 7, 3), np.uint8)
    ident = (1, 0, 0, 0, 1, 0)

    def refused(exc, text, fn, *args, **kw):
        with pytest.raises(exc) as e:
            fn(*args, **kw)
        assert text in str(e.value), str(e.value)

    T, R, P = A.transform_many, A.rotate_many, A.transpose_many
    # methods
    for bad in ("shear", 5, -1, None, 1.0, True):
        refused(ValueError, "every image: unknown transformation method", T, [img], (4, 4), bad, ident)
    refused(ValueError, "image 1: unknown transformation method", T, [img, img], (4, 4), ["affine", "warp"], ident)
    refused(NotImplementedError, "every image: MESH", T, [img], (4, 4), "mesh", ident)
    refused(NotImplementedError, "every image: MESH", T, [img], (4, 4), Image.Transform.MESH, ident)
    refused(NotImplementedError, "ImageTransformHandler", T, [img], (4, 4), type("H", (), {"transform": lambda *a: None})(), ident)
    refused(NotImplementedError, "ImageTransformHandler", T, [img], (4, 4), type("H", (), {"getdata": lambda *a: None})(), ident)
    for bad in ("hflip", 7, -1, None, 2.0):
        refused(ValueError, "every image: unknown transpose method", P, [img], bad)
    refused(ValueError, "image 1: unknown transpose method", P, [img, img], ["ROTATE_90", "ROTATE_45"])
    # filters, with Pillow's own text
    use = "Use Image.Resampling.NEAREST (0), Image.Resampling.BILINEAR (2) or Image.Resampling.BICUBIC (3)"
    for bad, text in ((Image.Resampling.BOX, "Image.Resampling.BOX (4) cannot be used. "), ("hamming", "Image.Resampling.HAMMING (5) cannot be used. "),
                      (1, "Image.Resampling.LANCZOS (1) cannot be used. "), (6, "Unknown resampling filter (6). "), ("cubic", "Unknown resampling filter (cubic). ")):
        refused(ValueError, "every image: " + text + use, T, [img], (4, 4), "affine", ident, bad)
        refused(ValueError, "image 1: " + text + use, R, [img, img], 10, ["nearest", bad])
        with pytest.raises(ValueError) as e:
            Image.fromarray(img).transform((4, 4), Image.Transform.AFFINE, ident, bad if not isinstance(bad, str) else {"hamming": 5, "cubic": "cubic"}[bad])
        assert str(e.value) == text + use
    # data
    for method, n in (("affine", 6), ("extent", 4), ("perspective", 8), ("quad", 8)):
        for m in (n - 1, n + 1):
            refused(ValueError, f"image 0: data of {m} values: '{method}' takes {n}", T, [img], (4, 4), method, (1.0,) * m)
    refused(ValueError, "image 1: data of 4 values", T, [img, img], (4, 4), "affine", [ident, (0, 0, 1, 1)])
    for bad in ((1, 0, 0, 0, 1, float("nan")), (1, 0, 0, 0, float("inf"), 0), (1, 0, 0, 0, 1, "0"), (1, 0, 0, 0, 1, None), (), "affine", None, 3):
        refused(ValueError, "data", T, [img], (4, 4), "affine", bad)
    # per-image lists of the wrong length
    refused(ValueError, "size: 3 entries for 2 images", T, [img, img], [(4, 4)] * 3, "affine", ident)
    refused(ValueError, "method: 1 entries for 2 images", T, [img, img], (4, 4), ["affine"], ident)
    refused(ValueError, "data: 3 entries for 2 images", T, [img, img], (4, 4), "affine", [ident] * 3)
    refused(ValueError, "resample: 3 entries for 2 images", T, [img, img], (4, 4), "affine", ident, [0, 2, 3])
    refused(ValueError, "fillcolor: 3 entries for 2 images", T, [img, img], (4, 4), "affine", ident, 0, [1, 2, 3])
    refused(ValueError, "angle: 1 entries for 2 images", R, [img, img], [10])
    refused(ValueError, "center: 3 entries for 2 images", R, [img, img], 10, center=[None, (1, 2), None])
    refused(ValueError, "method: 3 entries for 2 images", P, [img, img], [0, 1, 2])
    # sizes, images
    for bad in ((0, 4), (4, 32768), (4,), (4.0, 4), 4, None, (4, 4, 4), (True, 4)):
        refused(ValueError, "size", T, [img], bad, "affine", ident)
    for fn, args in ((T, ((4, 4), "affine", ident)), (R, (10,)), (P, (0,))):
        refused(ValueError, "image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4]", fn, [img, np.zeros((4, 4, 5), np.uint8)], *args)
        refused(ValueError, "image 0: uint8 [H, W]", fn, [np.zeros((4, 4, 1), np.uint8)], *args)
        refused(ValueError, "image 0: uint8 [H, W]", fn, [np.zeros((0, 4), np.uint8)], *args)
        refused(TypeError, "image 1: uint8 required, got float32", fn, [img, np.zeros((4, 4), np.float32)], *args)
        refused(TypeError, "image 0: uint8 required, got uint16", fn, [np.zeros((4, 4), np.uint16)], *args)
        refused(ValueError, "image 0: sizes up to 32767 a side", fn, [np.zeros((1, 32768), np.uint8)], *args)
        refused(ValueError, "needs at least one image", fn, [], *args)
    # fill colours
    for bad, text in (("red", "colour names are refused"), (256, "each 0 to 255"), (-1, "each 0 to 255"), (1.0, "each 0 to 255"), ((1, 2, 300), "each 0 to 255"), ((), "each 0 to 255")):
        refused(ValueError, "every image: fillcolor " + repr(bad) + ": " + ("colour" if "colour" in text else "None"), T, [img], (4, 4), "affine", ident, 0, bad)
    refused(ValueError, "image 0: fillcolor (1, 2): 2 values for 3 channels", T, [img], (4, 4), "affine", ident, 0, (1, 2))
    refused(ValueError, "image 1: fillcolor (1, 2, 3): 3 values for 1 channel", R, [img, img[..., 0]], 10, fillcolor=[(1, 2, 3), (1, 2, 3)])
    # rotate's own
    for bad in (float("nan"), float("inf"), "10", None):
        refused(ValueError, "every image: angle", R, [img], bad)
    for bad in ((1,), (1, 2, 3), (1, float("nan")), "ab", 5):
        refused(ValueError, "center", R, [img], 10, center=bad)
        refused(ValueError, "translate", R, [img], 10, translate=bad)
    refused(TypeError, "every image: expand", R, [img], 10, expand="yes")
    refused(TypeError, "every image: premultiply", T, [img], (4, 4), "affine", ident, premultiply=None)
    refused(ValueError, "image 0: an output of", R, [_Shape((30000, 30000))], 45, expand=True)
    refused(NotImplementedError, "image 0: an affine transform under 'nearest' beyond 16.16", R, [_Shape((30000, 30000))], 45, center=(4e4, 0))
    # what is accepted gets as far as the device
    for fn, args, kw in ((T, ((4, 4), Image.Transform.QUAD, (0, 0, 0, 6, 7, 6, 7, 0)), dict(resample=Image.Resampling.BICUBIC, fillcolor=(1, 2, 3))),
                         (T, ([(4, 4)], ["extent"], [[0, 0, 7, 6]], ["bilinear"], [5]), {}), (T, ((4, 4), 2, np.arange(8.0).tolist(), 3, None, False), {}),
                         (R, (np.float32(33.5), "bicubic", True, (1, 2), (0.5, np.int64(2)), 9), {}), (R, (90,), {}), (R, (0,), {}),
                         (P, ("transverse",), {}), (P, (Image.Transpose.FLIP_LEFT_RIGHT,), {}), (P, ([np.int64(3)],), {})):
        with pytest.raises(AssertionError, match="must not reach the device"):
            fn([img], *args, **kw)


class _Shape:
    """an image by its shape alone: what the host checks read"""
    dtype = "uint8"

    def __init__(self, shape):
        self.shape = shape
