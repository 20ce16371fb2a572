"""CPU: Pillow's resize / reduce / thumbnail without a device -- the NumPy model (tests/resample_reference.py) against live Pillow and
against the committed fixtures (tests/golden/resample), the library's host tap tables (aej_resample_taps_host) and thumbnail_plan
against that model, and the refusals and interface of resize_many / standard_jpeg_thumbnail_many."""
import io
import json
import os

import numpy as np
import pytest

import resample_reference as M
from conftest import GOLDEN

HERE = os.path.join(GOLDEN, "resample")
NAMES = tuple(M.FILTERS)


@pytest.fixture(scope="module")
def A():
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "meta.json")) as f:
        return json.load(f)["cases"], dict(np.load(os.path.join(HERE, "pixels.npz")))


def _file(folder, name):
    with open(os.path.join(GOLDEN, folder, name + ".jpg"), "rb") as f:
        return f.read()


# ---- (a) the model is Pillow ------------------------------------------------------------------------------------------------------------
def test_model_resize_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    done = 0
    for it in range(240):
        H, W = int(rng.integers(1, 50)), int(rng.integers(1, 50))
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        f = NAMES[it % 5]
        box = None
        if it % 2:                                   # half of them with a fractional box
            x0, x1 = sorted(rng.uniform(0, W, 2))
            y0, y1 = sorted(rng.uniform(0, H, 2))
            if x1 - x0 < 0.25 or y1 - y0 < 0.25:
                continue
            box = (float(x0), float(y0), float(x1), float(y1))
        gap = (None, 1.0, 2.0, 1.5)[(it // 5) % 4]
        try:
            got = M.resize(a, (w, h), f, box, gap)
        except NotImplementedError:                  # the tall image
            continue
        want = np.asarray(Image.fromarray(a).resize((w, h), M.FILTERS[f], box=box, reducing_gap=gap))
        assert got.shape == want.shape and np.array_equal(got, want), (it, (H, W), (w, h), f, box, gap)
        done += 1
    assert done > 150


def test_model_reduce_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(12)
    for it in range(120):
        H, W = int(rng.integers(1, 50)), int(rng.integers(1, 50))
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if it % 9 == 0:
            a[:] = 255
        fx, fy = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        if (fx, fy) == (1, 1):
            fx = 2
        want = np.asarray(Image.fromarray(a).reduce((fx, fy)))
        assert np.array_equal(M.reduce(a, (fx, fy)), want), (it, H, W, fx, fy)


def test_model_thumbnail_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(13)
    for k, (H, W, opts) in enumerate([(61, 83, dict(subsampling=0)), (83, 61, dict(subsampling=1)), (96, 128, dict(subsampling=2)), (70, 45, None)]):
        y, x = np.mgrid[0:H, 0:W]
        img = Image.fromarray(np.clip(np.stack([x * 3, y * 2 + x, x + y], -1) % 256 + rng.integers(-30, 31, (H, W, 3)), 0, 255).astype(np.uint8))
        buf = io.BytesIO()
        (img if opts else img.convert("L")).save(buf, "JPEG", quality=80, **(opts or {}))
        data = buf.getvalue()
        for j in range(14):
            size = (int(rng.integers(1, 100)), int(rng.integers(1, 100)))
            f, gap = NAMES[(j + k) % 5], (2.0, 1.0, None, 3.0, 1.5)[j % 5]
            im = Image.open(io.BytesIO(data))
            im.thumbnail(size, M.FILTERS[f], reducing_gap=gap)
            assert np.array_equal(M.thumbnail(data, size, f, gap), np.asarray(im.convert("RGB"))), (k, size, f, gap)


# ---- (b) the model is the committed fixtures (no Pillow needed) -------------------------------------------------------------------------
def test_model_equals_goldens(golden):
    cases, px = golden
    for c in cases:
        if c["kind"] == "thumb":
            got = M.thumbnail(_file(c["folder"], c["name"]), c["size"], c["filter"], c["gap"])
        else:
            got = M.resize(px[f"src/{c['source']}"], tuple(c["size"]), c["filter"], c["box"], c["gap"])
        assert got.dtype == np.uint8 and np.array_equal(got, px[c["key"]]), c["key"]


# ---- (c) the library's tap tables are the model's -----------------------------------------------------------------------------------------
TAP_CASES = [(381, 0, 380.5, 5), (77, 0, 380.5 / 5, 30), (77, 0.1, 380.5 / 5, 77),      # float32-inexact edges
             (100, 0, 100, 100), (100, 0.3, 99.7, 250), (10, 0, 10, 20), (50, 2.5, 47.25, 13), (9, 1, 8, 7),      # scale at, below, above 1
             (1, 0, 1, 5), (1, 0, 1, 1), (1, 0.25, 0.75, 3), (7, 0, 7, 1), (1101, 0, 1101, 3),      # in_size 1; one output; the long loop
             (12, 0, 12, 4), (12, 0, 12, 3), (12, 0, 12, 6), (12, 1, 11, 5), (13, 0.5, 12.5, 4)]      # the box filter at exact half-pixel centres


@pytest.mark.parametrize("f", NAMES)
def test_taps_equal_the_model(A, f):
    from adaptive_edge_aware_jpeg_amd.resample import resample_taps
    for n, a, b, o in TAP_CASES:
        xmin, cnt, taps = resample_taps(n, a, b, o, f)
        mx, mn, mt = M.taps_for(n, a, b, o, f)
        assert np.array_equal(xmin, mx) and np.array_equal(cnt, mn), (f, n, a, b, o)
        for i in range(o):
            assert list(taps[i, :mn[i]]) == mt[i] and not taps[i, mn[i]:].any(), (f, n, a, b, o, i)
        assert (xmin >= 0).all() and (xmin + cnt <= n).all()


def test_taps_refusals(A):
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    lib = load_library()
    for args in [(10, 0, 10, 5, 0), (10, 0, 10, 5, 6), (0, 0, 1, 5, 3), (10, 0, 10, 0, 3), (10, 5, 5, 4, 3), (10, -1, 5, 4, 3), (10, 0, 10.5, 4, 3)]:
        assert lib.aej_resample_taps_host(*args, None, None, 0) == -1, args
    b, t = np.zeros((5, 2), np.int32), np.zeros(8, np.int32)
    assert lib.aej_resample_taps_host(10, 0, 10, 5, 3, b.ctypes.data, t.ctypes.data, t.size) == -4
    assert not t.any()


# ---- (d) thumbnail_plan ----------------------------------------------------------------------------------------------------------------------
def test_plan_equals_the_model_everywhere(A):
    for W in range(1, 41):
        for H in range(1, 41):
            for sw in range(1, 13):
                for sh in range(1, 13):
                    assert A.thumbnail_plan(W, H, (sw, sh)) == M.thumbnail_plan(W, H, (sw, sh)), (W, H, sw, sh)
    for gap in (None, 1.0, 3.0):
        for W, H, sw, sh in [(40, 33, 3, 5), (17, 39, 12, 2), (1, 1, 1, 1), (128, 96, 3, 3)]:
            assert A.thumbnail_plan(W, H, (sw, sh), gap) == M.thumbnail_plan(W, H, (sw, sh), gap)


def test_plan_equals_the_goldens(A, golden):
    for c in golden[0]:
        if c["kind"] != "thumb":
            continue
        plan = A.thumbnail_plan(*c["file_size"], c["size"], c["gap"])
        assert (plan is None) == c["unchanged"], c["key"]
        if plan is not None:
            assert plan[0] == c["scale"] and list(plan[1]) == c["factors"] and list(plan[2]) == c["final"], c["key"]
            assert plan[3] == (0, 0, c["file_size"][0] / c["scale"], c["file_size"][1] / c["scale"])


def test_plan_final_size_equals_pillows_everywhere(A):
    """Image.thumbnail's resulting im.size for every W, H <= 40 and every size with components <= 12.  The final size does not depend on
    the file format (draft() changes the decode, not preserve_aspect_ratio), so a plain image stands for the file here; the draft scale
    is checked on JPEG files below."""
    Image = pytest.importorskip("PIL.Image")
    for W in range(1, 41):
        for H in range(1, 41):
            src = Image.new("L", (W, H))
            for sw in range(1, 13):
                for sh in range(1, 13):
                    im = src.copy()
                    im.thumbnail((sw, sh), 4, reducing_gap=None)
                    plan = A.thumbnail_plan(W, H, (sw, sh))
                    assert im.size == ((W, H) if plan is None else plan[2]), (W, H, sw, sh)


def test_plan_equals_pillows_size(A):
    Image = pytest.importorskip("PIL.Image")
    for W, H in [(40, 33), (17, 39), (1, 1), (39, 2), (3, 40), (25, 25)]:
        buf = io.BytesIO()
        Image.new("RGB", (W, H), (90, 120, 30)).save(buf, "JPEG")
        for sw in range(1, 13):
            for sh in range(1, 13):
                im = Image.open(io.BytesIO(buf.getvalue()))
                im.thumbnail((sw, sh))
                plan = A.thumbnail_plan(W, H, (sw, sh))
                assert im.size == ((W, H) if plan is None else plan[2]), (W, H, sw, sh)
                assert (im.decoderconfig[0] if im.decoderconfig else 1) == (1 if plan is None else plan[0])


# ---- (e) refusals and interface ------------------------------------------------------------------------------------------------------------------
def test_interface(A):
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    assert load_library().aej_abi_version() == 3
    for name in ("resize_many", "standard_jpeg_thumbnail_many", "thumbnail_plan"):
        assert name in A.__all__ and callable(getattr(A, name))
    assert A.standard_jpeg.standard_jpeg_thumbnail_many is A.standard_jpeg_thumbnail_many


def test_resize_refusals_name_the_image(A):
    a = np.zeros((8, 9, 3), np.uint8)
    for r in ("nearest", 0):
        with pytest.raises(NotImplementedError, match="every image: resample .*nearest"):
            A.resize_many([a], (4, 4), resample=r)
        with pytest.raises(NotImplementedError, match="image 1: resample .*nearest"):
            A.resize_many([a, a], (4, 4), resample=["box", r])
    for r in ("cubic", 6, True, 2.0, None):
        with pytest.raises(ValueError, match="every image: resample"):
            A.resize_many([a], (4, 4), resample=r)
        with pytest.raises(ValueError, match="image 1: resample"):
            A.resize_many([a, a], (4, 4), resample=[3, r])
    for g in (0.5, 0, -1.0, True):
        with pytest.raises(ValueError, match="every image: reducing_gap must be 1.0 or greater"):
            A.resize_many([a], (4, 4), reducing_gap=g)
    for s in ((0, 4), (4, -1), (True, 4), (4.5, 4), (4,), "44"):
        with pytest.raises(ValueError, match="size"):
            A.resize_many([a], s)
    with pytest.raises(ValueError, match="image 1: size"):
        A.resize_many([a, a], [(4, 4), (4, 0)])
    with pytest.raises(NotImplementedError, match="image 1: a 2 x 300 image, more than 100 times as tall"):
        A.resize_many([a, np.zeros((300, 2, 3), np.uint8)], (2, 100))
    for box, why in [((-1, 0, 5, 5), "negative"), ((0, 0, 9.5, 8), "exceed"), ((3, 0, 3, 8), "empty"), ((0, 5, 9, 4), "empty"), ((0, 0, 9), "four numbers")]:
        with pytest.raises(ValueError, match="image 1: box .*" + why):
            A.resize_many([a, a], (4, 4), box=[None, box])
    with pytest.raises(ValueError, match="image 0: uint8"):
        A.resize_many([np.zeros((8, 9), np.uint8)], (4, 4))
    with pytest.raises(TypeError, match="image 1: uint8"):
        A.resize_many([a, np.zeros((8, 9, 3), np.float32)], (4, 4))
    with pytest.raises(ValueError, match="at least one image"):
        A.resize_many([], (4, 4))


def test_thumbnail_refusals_name_the_file(A):
    good = _file("jpegdec", "lena_64x64_420_q75")
    prog = _file("jpegprog", "lena_64x64_420_q75")
    for r in ("nearest", 0):
        with pytest.raises(NotImplementedError, match="every file: resample .*nearest"):
            A.standard_jpeg_thumbnail_many([good], (4, 4), resample=r)
        with pytest.raises(NotImplementedError, match="file 1: resample .*nearest"):
            A.standard_jpeg_thumbnail_many([good, good], (4, 4), resample=["lanczos", r])
    with pytest.raises(ValueError, match="file 0: resample 'cubic'"):
        A.standard_jpeg_thumbnail_many([good, good], (4, 4), resample=["cubic", "box"])
    with pytest.raises(ValueError, match="every file: reducing_gap must be 1.0 or greater"):
        A.standard_jpeg_thumbnail_many([good], (4, 4), reducing_gap=0.99)
    for s in ((0, 4), (4, -2), (True, 4), (0.5, 4)):
        with pytest.raises(ValueError, match="size"):
            A.standard_jpeg_thumbnail_many([good], s)
    with pytest.raises(ValueError, match="file 1: size"):
        A.standard_jpeg_thumbnail_many([good, good], [(4, 4), (0, 4)])
    with pytest.raises(ValueError, match="at least one file"):
        A.standard_jpeg_thumbnail_many([], (4, 4))
    # what standard_jpeg_decode_many refuses, with its words
    for files, kw in (([good, prog], {}), ([good, good[:100]], {}), ([good, b"no jpeg"], dict(progressive=True))):
        with pytest.raises((ValueError, NotImplementedError)) as want:
            A.standard_jpeg_decode_many(files, **kw)
        with pytest.raises(type(want.value)) as got:
            A.standard_jpeg_thumbnail_many(files, (8, 8), **kw)
        assert str(got.value) == str(want.value) and "file 1" in str(got.value)


def test_thumbnail_refuses_the_tall_file(A):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.new("RGB", (2, 300), (10, 200, 90)).save(buf, "JPEG")
    with pytest.raises(NotImplementedError, match="file 1: a 2 x 300 image, more than 100 times as tall"):
        A.standard_jpeg_thumbnail_many([_file("jpegdec", "lena_64x64_420_q75"), buf.getvalue()], (2, 100), reducing_gap=None)
