"""CPU: scaled_box= of standard_jpeg_decode_many and standard_jpeg_resized_crop_many without a device -- the MCU window of a box of the
scaled image (decode_box_window(..., scale=s), aej_jpegdec_sbox_window_host) against a per-pixel brute force written from libjpeg's
up-sampling rules at that scale (tests/jpegdec_sbox_reference.py), resized_crop_plan against its stated rules, and the refusals of the
new keyword and call, all of which come before any device work."""
import ctypes

import numpy as np
import pytest

import jpeg_adobe_reference as AR
import jpegdec_box_reference as R
import jpegdec_sbox_reference as S

FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


def _c_window(lib, W, H, hs, vs, ncomp, s):
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc, JpegProgFrame
    d, f = JpegDecDesc(), JpegProgFrame()
    for q in (d, f):
        q.width, q.height, q.hs, q.vs, q.ncomp = W, H, hs, vs, ncomp
    box, win = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()

    def ask(b, prog=False):
        box[:] = b
        fn, q = (lib.aej_jpegprog_sbox_window_host, f) if prog else (lib.aej_jpegdec_sbox_window_host, d)
        assert fn(ctypes.addressof(q), s, ctypes.addressof(box), ctypes.addressof(win)) == 0, b
        return tuple(win)
    return ask


# ---- the window -----------------------------------------------------------------------------------------------------------------------------
def _check_every_box(SJ, lib, layout, W, H, s):
    _, hs, vs, ncomp = layout
    ow, oh = S.scaled_size(W, H, s)
    pm, pml = S.pixel_mcus(W, H, hs, vs, ncomp, s), S.pixel_mcus(W, H, hs, vs, ncomp, s, luma=True)
    ask = _c_window(lib, W, H, hs, vs, ncomp, s)
    for k, box in enumerate(S.all_boxes(ow, oh)):
        want = S.brute_window(pm, box)
        assert SJ.decode_box_window(W, H, hs, vs, ncomp, box, scale=s) == want, (layout, (W, H), s, box)
        assert ask(box) == want, (layout, (W, H), s, box)
        if k % 7 == 0:
            assert ask(box, prog=True) == want, (layout, (W, H), s, box)
            assert SJ.decode_box_window(W, H, hs, vs, ncomp, box, luma=True, scale=s) == S.brute_window(pml, box), (layout, s, box)


@pytest.mark.parametrize("s", S.SCALES)
@pytest.mark.parametrize("layout", S.LAYOUTS, ids=[l[0] for l in S.LAYOUTS])
def test_window_equals_brute_force_41x29(SJ, lib, layout, s):
    assert S.scaled_size(41, 29, s) == {2: (21, 15), 4: (11, 8), 8: (6, 4)}[s]
    _check_every_box(SJ, lib, layout, 41, 29, s)


@pytest.mark.parametrize("layout", S.LAYOUTS, ids=[l[0] for l in S.LAYOUTS])
def test_window_equals_brute_force_narrow(SJ, lib, layout):
    for W, H in R.NARROW:                                    # (w, 20), w = 1 .. 5: scaled 1 .. 3 wide, where replication decides
        _check_every_box(SJ, lib, layout, W, H, 2)


def test_the_window_follows_the_scaled_rules(SJ):
    w = SJ.decode_box_window
    assert w(83, 61, 2, 2, 3, (8, 8, 16, 16), scale=2) == (1, 1, 2, 2)       # 4:2:0: MCUs of 8 x 8 scaled pixels, no neighbours
    assert w(83, 61, 2, 1, 3, (8, 4, 16, 8), scale=2) == (0, 1, 3, 2)        # 4:2:2: pixel 8 is even, chroma column 3 of MCU 0; pixel 15 odd, column 8
    assert w(83, 61, 2, 1, 3, (9, 4, 15, 8), scale=2) == (1, 1, 2, 2)
    assert w(83, 61, 2, 1, 3, (2, 0, 4, 1), scale=8) == (1, 0, 2, 1)         # scale 8: replication
    assert w(83, 61, 1, 2, 3, (4, 8, 8, 16), scale=2) == (1, 0, 2, 3)        # 4:4:0: row 8 even reads chroma row 3, row 15 odd row 8
    assert w(83, 61, 1, 2, 3, (4, 8, 8, 16), scale=2, luma=True) == (1, 1, 2, 2)
    assert w(83, 61, 2, 2, 3, (16, 16, 32, 32), scale=1) == w(83, 61, 2, 2, 3, (16, 16, 32, 32))      # scale 1: the full-size window


def test_c_window_refuses(lib):
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc
    d = JpegDecDesc()
    d.width, d.height, d.hs, d.vs, d.ncomp = 83, 61, 2, 2, 3
    win = (ctypes.c_int32 * 4)(9, 9, 9, 9)
    for s, bad in ((2, (0, 0, 43, 31)), (2, (0, 0, 42, 32)), (4, (0, 0, 22, 16)), (8, (0, 0, 11, 9)), (2, (-1, 0, 4, 4)), (2, (4, 4, 4, 8)), (3, (0, 0, 4, 4))):
        box = (ctypes.c_int32 * 4)(*bad)
        assert lib.aej_jpegdec_sbox_window_host(ctypes.addressof(d), s, ctypes.addressof(box), ctypes.addressof(win)) == -1, (s, bad)
        assert tuple(win) == (9, 9, 9, 9)
    assert lib.aej_jpegdec_sbox_window_host(None, 2, None, None) == -1
    assert lib.aej_jpegprog_sbox_window_host(None, 2, None, None) == -1


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------
def test_plan_scale_table(SJ):
    # (box, size, gap) -> s, worked by hand
    table = [((0, 0, 3840, 2160), (224, 224), None, 1),
             ((0, 0, 3840, 2160), (224, 224), 2.0, 4),       # min(3840 // 448, 2160 // 448) = min(8, 4)
             ((0, 0, 3840, 2160), (224, 224), 1.0, 8),       # min(17, 9)
             ((100, 100, 996, 996), (224, 224), 2.0, 2),     # 896 // 448 = 2
             ((100, 100, 995.9, 996), (224, 224), 2.0, 1),   # int(895.9) // 448 = 1
             ((0.5, 0.5, 1792.6, 1792.6), (224, 224), 2.0, 4),      # int(1792.1) // 448 = 4
             ((0, 0, 83, 61), (1, 1), 1.0, 8),
             ((0, 0, 83, 61), (10, 10), 1.0, 4),             # min(8, 6)
             ((0, 0, 83, 61), (10, 10), 1.5, 4),             # int(15.0) = 15: min(5, 4)
             ((10, 10, 30, 26), (96, 80), 2.0, 1)]           # up-scaling: ratio 0
    for box, size, gap, want in table:
        p = SJ.resized_crop_plan(3840, 2160, box, size, "bilinear", gap)
        assert p["scale"] == want == S.crop_scale(box, size, gap), (box, size, gap)
        assert p["box"] == tuple(v / want for v in box)


def test_plan_without_a_gap_is_the_resize_itself(SJ):
    for box in ((3, 5, 60, 40), (0.25, 1.5, 82.75, 60.5), (0, 0, 83, 61)):
        p = SJ.resized_crop_plan(83, 61, box, (32, 24), "bicubic", None)
        assert p["scale"] == 1 and p["box"] == tuple(float(v) for v in box) == tuple(box) and p["factors"] == (1, 1)


@pytest.mark.parametrize("filt", FILTERS)
def test_plan_window_is_the_hull_of_the_taps(SJ, filt):
    from adaptive_edge_aware_jpeg_amd.resample import resample_taps
    for box, size in (((3, 5, 60, 40), (32, 24)), ((10, 10, 30, 26), (96, 80)), ((0.25, 1.5, 82.75, 60.5), (17, 50)), ((0, 0, 83, 61), (83, 61))):
        p = SJ.resized_crop_plan(83, 61, box, size, filt, None)
        xm, xn, _ = resample_taps(83, box[0], box[2], size[0], filt)
        ym, yn, _ = resample_taps(61, box[1], box[3], size[1], filt)
        hull = (int(xm.min()), int(ym.min()), int((xm + xn).max()), int((ym + yn).max()))
        assert p["window"] == hull, (filt, box, size)
        assert 0 <= hull[0] < hull[2] <= 83 and 0 <= hull[1] < hull[3] <= 61
    p = SJ.resized_crop_plan(83, 61, (10, 10, 30, 26), (96, 80), filt, None)      # up-scaling: more than Pillow's safe box where the support is wide
    assert p["window"][0] <= 10 and p["window"][2] >= 30
    q = SJ.resized_crop_plan(332, 244, (8, 4, 320, 240), (32, 24), filt, 1.0)     # min(312 // 32, 236 // 24) = 9: s = 8; 39 / 32 leaves no reduce
    assert q["scale"] == 8 and q["factors"] == (1, 1)
    r = SJ.resized_crop_plan(83, 61, (1, 1, 82, 60), (8, 6), filt, 1.0)           # min(81 // 8, 59 // 6) = 9: s = 8
    assert r["scale"] == 8
    t = SJ.resized_crop_plan(83, 61, (0, 0, 83, 30), (8, 12), filt, 1.0)          # s = 2 (min(10, 2)), then factors (int(41.5 / 8), int(15 / 12)) = (5, 1)
    assert t["scale"] == 2 and t["factors"] == (5, 1) and t["window"] == tuple(t["reduce_box"])


def test_plan_window_equals_the_tap_bounds_on_random_axes(SJ):
    """the plan computes the hull from the two end outputs alone; aej_resample_taps_host's bounds are the reference for every axis"""
    from adaptive_edge_aware_jpeg_amd.resample import resample_taps
    rng = np.random.default_rng(11)
    for k in range(400):
        W, H = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        l, t = float(rng.uniform(0, W - 0.01)), float(rng.uniform(0, H - 0.01))
        r, b = float(rng.uniform(l + 0.005, W)), float(rng.uniform(t + 0.005, H))
        if k % 3 == 0:
            l, t, r, b = int(l), int(t), max(int(r), int(l) + 1), max(int(b), int(t) + 1)
        size, filt = (int(rng.integers(1, 200)), int(rng.integers(1, 200))), FILTERS[k % 5]
        if not (np.float32(r) - np.float32(l) > 0 and np.float32(b) - np.float32(t) > 0) or np.float32(r) > W or np.float32(b) > H:
            continue
        if (H > W * 100 and size[1] < H):
            continue
        p = SJ.resized_crop_plan(W, H, (l, t, r, b), size, filt, None)
        xm, xn, _ = resample_taps(W, l, r, size[0], filt)
        ym, yn, _ = resample_taps(H, t, b, size[1], filt)
        assert p["window"] == (int(xm.min()), int(ym.min()), int((xm + xn).max()), int((ym + yn).max())), (W, H, (l, t, r, b), size, filt)


# ---- refusals, before any device work -------------------------------------------------------------------------------------------------------
def _files():
    return [R.make_file("420", 83, 61), R.make_file("grey", 40, 30), R.make_file("444", 32, 32, progressive=True)]


def _no_device(monkeypatch, SJ):
    def refuse(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(SJ, "get_context", refuse)


def test_scaled_box_refusals(SJ, monkeypatch):
    _no_device(monkeypatch, SJ)
    files = _files()
    kw = dict(progressive=True, scale=2)
    for bad in (True, 1.5, 7, "0,0,8,8", (0, 0, 8), (0, 0, 8.0, 8), (0, 0, True, 8)):
        with pytest.raises(TypeError):
            SJ.standard_jpeg_decode_many(files, scaled_box=bad, **kw)
    with pytest.raises(TypeError, match="file 1"):
        SJ.standard_jpeg_decode_many(files, scaled_box=[None, (0, 0, 8.0, 8), None], **kw)
    for bad in ([None, None], [(0, 0, 8, 8)] * 4, []):
        with pytest.raises(ValueError, match="box"):
            SJ.standard_jpeg_decode_many(files, scaled_box=bad, **kw)
    for bad in ((0, 0, 21, 15), (0, 0, 20, 16), (-1, 0, 8, 8), (8, 8, 8, 9)):      # file 1 is 40 x 30: 20 x 15 at scale 2
        with pytest.raises(ValueError, match="file 1.*20 x 15"):
            SJ.standard_jpeg_decode_many(files, scaled_box=[(0, 0, 42, 31), bad, None], **kw)
    with pytest.raises(ValueError, match="file 0"):
        SJ.standard_jpeg_decode_many(files, scaled_box=(0, 0, 43, 10), **kw)
    with pytest.raises(ValueError, match="both"):
        SJ.standard_jpeg_decode_many(files, progressive=True, box=(0, 0, 8, 8), scaled_box=(0, 0, 8, 8))


def test_adobe_files_are_refused(SJ, monkeypatch):
    _no_device(monkeypatch, SJ)
    cmyk = AR.make_file("cmyk", AR.LAYOUTS[0], 40, 30)
    with pytest.raises(NotImplementedError, match="file 0.*a box of a four-component / RGB-coded file is not built"):
        SJ.standard_jpeg_decode_many([cmyk], adobe=True, scaled_box=(0, 0, 8, 8))
    with pytest.raises(NotImplementedError, match="file 1"):
        SJ.standard_jpeg_resized_crop_many([_files()[0], cmyk], (0, 0, 30, 20), (8, 8))


def test_resized_crop_refusals(SJ, monkeypatch):
    _no_device(monkeypatch, SJ)
    files = _files()
    call = SJ.standard_jpeg_resized_crop_many
    for bad in (True, 7, "box", (0, 0, 8), (0, 0, True, 8), (0, 0, "8", 8), None):
        with pytest.raises(TypeError):
            call(files, bad, (8, 8), progressive=True)
    with pytest.raises(TypeError, match="file 1"):
        call(files, [(0, 0, 8, 8), (0, 0, 8), (0, 0, 8, 8)], (8, 8), progressive=True)
    with pytest.raises(ValueError, match="box"):
        call(files, [(0, 0, 8, 8)] * 2, (8, 8), progressive=True)
    for bad in ((0, 0, 40.5, 30), (0, 0, 40, 31), (-0.5, 0, 8, 8), (8, 8, 8, 9), (9, 8, 8, 9)):
        with pytest.raises(ValueError, match="file 1"):
            call(files, [(0, 0, 83, 61), bad, (0, 0, 32, 32)], (8, 8), progressive=True)
    with pytest.raises(ValueError, match="auto"):
        call(files, (0, 0, 8, 8), (8, 8), progressive=True, mode="auto")
    with pytest.raises(TypeError):
        call(files, (0, 0, 8, 8), (8, 8), progressive=True, mode=["RGB"] * 3)
    with pytest.raises(NotImplementedError):
        call(files, (0, 0, 8, 8), (8, 8), "nearest", progressive=True)
    with pytest.raises(ValueError):
        call(files, (0, 0, 8, 8), (8, 8), reducing_gap=0.5, progressive=True)
    with pytest.raises(ValueError):
        call(files, (0, 0, 8, 8), (0, 8), progressive=True)
    with pytest.raises(NotImplementedError, match="progressive"):
        call(files, (0, 0, 8, 8), (8, 8))


def test_a_box_at_another_scale_is_still_not_built(SJ, monkeypatch):
    _no_device(monkeypatch, SJ)
    with pytest.raises(NotImplementedError, match="file 1.*a box at scale 2, 4 or 8 is not built"):
        SJ.standard_jpeg_decode_many(_files(), progressive=True, scale=[1, 2, 4], box=[(0, 0, 8, 8), (0, 0, 8, 8), None])
    with pytest.raises(NotImplementedError, match="file 0.*a box at scale 2, 4 or 8 is not built"):
        SJ.standard_jpeg_decode_many(_files(), progressive=True, scale=2, box=(1, 1, 2, 2))


def test_the_new_entries_resolve(lib):
    import adaptive_edge_aware_jpeg_amd as A
    assert A.resized_crop_plan is A.standard_jpeg.resized_crop_plan and callable(A.standard_jpeg_resized_crop_many)
    for name in ("aej_jpegdec_batch_sbox", "aej_jpegdec_workspace_bytes_sbox", "aej_jpegprog_batch_sbox", "aej_jpegprog_workspace_bytes_sbox",
                 "aej_jpegdec_sbox_window_host", "aej_jpegprog_sbox_window_host", "aej_resample_batch_win", "aej_resample_workspace_bytes_win"):
        assert getattr(lib, name) is not None
    assert lib.aej_jpegdec_workspace_bytes_sbox(None, None, 1, None, None, None) == 0
    assert lib.aej_resample_workspace_bytes_win(None, None, 1, None, None) == 0
