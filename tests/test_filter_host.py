"""CPU: Pillow's BoxBlur / GaussianBlur / UnsharpMask without a device -- the NumPy model (tests/filter_reference.py) against live
Pillow, the library's host plan (aej_filter_plan_host: the Gaussian's box radius and the weights of a pass) against that model, and the
refusals and interface of filter_many."""
import ctypes
import os
import re

import numpy as np
import pytest

import filter_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_RADII = [0.0, 1e-30, 1e-3, 0.49999997, 0.5, 0.99999994, 1.0, 1.0000001, 1023.9999, 1024.0, 1024.5, 1024.9999]


@pytest.fixture(scope="module")
def A():
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _pillow(a, spec):
    from PIL import Image
    return np.asarray(Image.fromarray(a).filter(spec.pil()))


def _impulses():
    row = np.zeros((1, 257), np.uint8)
    row[0, 40], row[0, 200] = 255, 131
    return row


# ---- (a) the model is Pillow ------------------------------------------------------------------------------------------------------------
def test_model_equals_pillow():
    cases = M.catalogue()
    assert len(cases) == len(M.SHAPES) * len(M.CHANNELS) * (5 * len(M.RADII) + len(M.UNSHARP))
    for a, spec in cases:
        want = _pillow(a, spec)
        got = M.model(a, spec)
        assert got.dtype == np.uint8 and got.shape == a.shape == want.shape and np.array_equal(got, want), (a.shape, spec)


def test_model_radius_sweep_equals_pillow():
    row = _impulses()
    for radius in M.SWEEP:
        spec = M.Spec("GaussianBlur", radius)
        assert np.array_equal(M.model(row, spec), _pillow(row, spec)), radius
    for radius in M.SWEEP[::40]:
        for spec in (M.Spec("BoxBlur", radius), M.Spec("UnsharpMask", radius, 170, 1)):
            assert np.array_equal(M.model(row, spec), _pillow(row, spec)), spec


# ---- (b) the library's host plan is the model's ----------------------------------------------------------------------------------------
def test_plan_host_equals_model(A):
    F = A.filters
    for radius in M.SWEEP + [float(np.float32(r)) for r in M.RADII] + [0.0, 1e-30, 1e-3, 400.0, 1000.0]:
        for kind in ("GaussianBlur", "UnsharpMask"):
            p = F.filter_plan(kind, radius, radius / 2)
            assert p["passes"] == 3
            for axis, rad in enumerate((radius, radius / 2)):
                box = M.gaussian_box(rad)
                assert (np.float32(p["box"][axis]), p["r"][axis], p["ww"][axis], p["fw"][axis]) == (box,) + M.box_weights(box), (kind, radius, axis)
    assert F.filter_plan("GaussianBlur", 0, 0)["box"] == (0.0, 0.0)
    for k in list(range(0, 16400)) + [r * 16 for r in EDGE_RADII]:      # (k = 16400 is radius 1025, the first one refused: below)
        radius = float(np.float32(k / 16))
        p = F.filter_plan("BoxBlur", radius, 3)
        assert p["passes"] == 1 and p["box"] == (radius, 3.0)
        assert (p["r"][0], p["ww"][0], p["fw"][0]) == M.box_weights(radius), radius
        assert (p["r"][1], p["ww"][1], p["fw"][1]) == M.box_weights(3)
        r, ww, fw = M.box_weights(radius)
        assert 0 <= (1 << 24) - ((2 * r + 1) * ww + 2 * fw) <= 1
    for kind, radius in (("BoxBlur", 1025.0), ("BoxBlur", 1e9), ("GaussianBlur", 2000.0), ("GaussianBlur", 1e30), ("UnsharpMask", 3e38)):
        with pytest.raises(NotImplementedError):
            F.filter_plan(kind, radius, 1)
        with pytest.raises(NotImplementedError):
            F.filter_plan(kind, 1, radius)
    for radius in (-1.0, -1e-30, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            F.filter_plan("BoxBlur", radius, 1)
        with pytest.raises(ValueError):
            F.filter_plan("GaussianBlur", 1, radius)
    assert max(F.filter_plan("GaussianBlur", 1024, 1020)["r"]) <= 1024       # a Gaussian's box radius is about its own


def test_geometry_host(A):
    g = A.filters.filter_geometry()
    assert set(g) == {"tile_w", "tile_h", "max_halo", "row_span", "col_band", "col_bytes"} and all(v >= 1 for v in g.values())
    assert g["tile_w"] % 4 == 0 and g["col_bytes"] % 4 == 0
    # UnsharpMask's default radius and GaussianBlur(2) are served by the fused kernel
    p = A.filters.filter_plan("GaussianBlur", 2, 2)
    assert p["passes"] * (p["r"][0] + 1) <= g["max_halo"]


# ---- (c) interface and refusals, all without a device -------------------------------------------------------------------------------------
def test_exports_and_abi(A):
    from adaptive_edge_aware_jpeg_amd import _lib, filters
    for name in ("BoxBlur", "GaussianBlur", "UnsharpMask", "filter_many"):
        assert name in A.__all__ and getattr(A, name) is getattr(filters, name)
    assert (A.BoxBlur(2).name, A.GaussianBlur().radius, A.UnsharpMask().percent, A.UnsharpMask().threshold) == ("BoxBlur", 2, 150, 3)
    header = open(os.path.join(ROOT, "include", "aej.h")).read()
    declared = set(re.findall(r"AEJ_API[^;(]*?\b(aej_filter_\w+)\s*\(", header))
    assert declared == {"aej_filter_plan_host", "aej_filter_geometry_host", "aej_filter_workspace_bytes", "aej_filter_batch"}
    assert declared <= set(_lib.SIGNATURES)
    lib = _lib.load_library()
    assert lib.aej_abi_version() == 3
    assert ctypes.sizeof(_lib.FilterDesc) == 48 and ctypes.sizeof(_lib.FilterPlan) == 36
    d = (_lib.FilterDesc * 1)()
    assert lib.aej_filter_workspace_bytes(None, ctypes.addressof(d), 1, 0) == 0      # no context: nothing to size


def test_refusals_need_no_device(A, monkeypatch):
    from adaptive_edge_aware_jpeg_amd import _lib, filters

    def no_device(*a, **k):
        raise AssertionError("refused calls must not reach the device")
    monkeypatch.setattr(_lib, "get_context", no_device)
    img = np.zeros((4, 5, 3), np.uint8)
    f = A.GaussianBlur(2)

    def refused(exc, images, flt, text, **kw):
        with pytest.raises(exc) as e:
            A.filter_many(images, flt, **kw)
        assert text in str(e.value), str(e.value)

    refused(ValueError, [], f, "at least one image")
    for bad in (np.zeros((4,), np.uint8), np.zeros((4, 5, 1), np.uint8), np.zeros((4, 5, 5), np.uint8), np.zeros((2, 2, 3, 1), np.uint8),
                np.zeros((0, 5, 3), np.uint8), np.zeros((4, 0), np.uint8)):
        refused(ValueError, [img, bad], f, "image 1:")
    refused(ValueError, [img, np.zeros((1, 65536), np.uint8)], f, "image 1:")
    refused(TypeError, [img, img.astype(np.float32)], f, "image 1:")
    refused(TypeError, [img.astype(np.int8)], f, "image 0:")
    refused(ValueError, [img, img], [f], "1 entries for 2 images")
    refused(ValueError, [img, img], [f, f, f], "3 entries for 2 images")
    for bad in (None, "GaussianBlur", 2, object(), type("Kernel", (), {"name": "Kernel", "radius": 1})(), type("NoRadius", (), {"name": "BoxBlur"})()):
        refused(ValueError, [img], bad, "every image:")
        refused(ValueError, [img, img], [f, bad], "image 1:")
    for radius in (float("nan"), float("inf"), -1, -0.5, (1, -1), (float("nan"), 1), (1, 2, 3), (1,), "2", None, (1, "2"), True):
        for cls in (A.BoxBlur, A.GaussianBlur):
            refused(ValueError, [img], cls(radius), "every image:")
            refused(ValueError, [img, img], [f, cls(radius)], "image 1:")
    for radius in (float("nan"), -2, (1, 1), None):
        refused(ValueError, [img], A.UnsharpMask(radius), "every image:")
    for percent, threshold in ((150.0, 3), (150, 3.0), (True, 3), (150, False), (None, 3), ("150", 3)):
        refused(TypeError, [img], A.UnsharpMask(2, percent, threshold), "every image:")
        refused(TypeError, [img, img], [f, A.UnsharpMask(2, percent, threshold)], "image 1:")
    for flt in (A.BoxBlur(1025), A.BoxBlur((1, 1025.5)), A.GaussianBlur(1100), A.GaussianBlur((1100, 1)), A.UnsharpMask(1100), A.UnsharpMask(2, 1000001, 3),
                A.UnsharpMask(2, -1000001, 3)):
        refused(NotImplementedError, [img], flt, "every image:")
        refused(NotImplementedError, [img, img], [f, flt], "image 1:")
    refused(ValueError, [img], f, "_path", _path="tiles")
    refused(ValueError, [img, img], [f, A.GaussianBlur(20)], "image 1:", _path="fused")
    # what is accepted gets as far as the device: the largest radii, any threshold, PIL's own filter objects
    from PIL import ImageFilter
    for flt in (A.BoxBlur(1024.9), A.GaussianBlur(1020), A.UnsharpMask(2, 1000000, -5), A.UnsharpMask(2, -1000000, 10 ** 12), ImageFilter.BoxBlur((0, 3)),
                ImageFilter.GaussianBlur(1.5), ImageFilter.UnsharpMask(), A.BoxBlur(np.float32(1.5)), A.UnsharpMask(np.float64(2), np.int64(120), np.int32(2))):
        with pytest.raises(AssertionError, match="must not reach the device"):
            A.filter_many([img], flt)
    assert filters.filter_many is A.filter_many
