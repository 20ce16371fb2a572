"""CPU: box= of standard_jpeg_decode_many without a device -- decode_box_window and its C twin aej_jpegdec_box_window_host against a
brute force written from the up-sampling rule (tests/jpegdec_box_reference.py: every pixel's luma sample and every chroma sample
libjpeg reads for it, then the first and last MCU), and the refusals of the keyword, all of which come before any device work."""
import ctypes

import pytest

import jpegdec_box_reference as R

SMALL = ((16, 16), (17, 33)) + R.NARROW                      # (W, H): every box of these


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


def _c_window(lib, W, H, hs, vs, ncomp):
    """aej_jpegdec_box_window_host and its progressive twin for one file shape -> box -> (window of the one, of the other)"""
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc, JpegProgFrame
    d, f = JpegDecDesc(), JpegProgFrame()
    for s in (d, f):
        s.width, s.height, s.hs, s.vs, s.ncomp = W, H, hs, vs, ncomp
    box, win = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()

    def ask(b):
        box[:] = b
        out = []
        for fn, s in ((lib.aej_jpegdec_box_window_host, d), (lib.aej_jpegprog_box_window_host, f)):
            assert fn(ctypes.addressof(s), ctypes.addressof(box), ctypes.addressof(win)) == 0, b
            out.append(tuple(win))
        return out
    return ask


def _boxes(W, H):
    return R.all_boxes(W, H) if (W, H) in SMALL else R.forced_boxes(W, H) + R.random_boxes(W, H, 400, 7)


@pytest.mark.parametrize("size", SMALL + ((83, 61),), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=[l[0] for l in R.LAYOUTS])
def test_window_equals_brute_force(SJ, lib, layout, size):
    import adaptive_edge_aware_jpeg_amd as A
    assert A.decode_box_window is SJ.decode_box_window
    _, hs, vs, ncomp = layout
    W, H = size
    pm = R.pixel_mcus(W, H, hs, vs, ncomp)
    ask = _c_window(lib, W, H, hs, vs, ncomp)
    for box in _boxes(W, H):
        want = R.brute_window(pm, box)
        assert SJ.decode_box_window(W, H, hs, vs, ncomp, box) == want, (layout, size, box)
        assert ask(box) == [want, want], (layout, size, box)


@pytest.mark.parametrize("layout", R.LAYOUTS, ids=[l[0] for l in R.LAYOUTS])
def test_luma_window_is_the_luma_samples_alone(SJ, layout):
    _, hs, vs, ncomp = layout
    W, H = 83, 61
    pm = R.pixel_mcus(W, H, hs, vs, ncomp, luma=True)
    for box in R.forced_boxes(W, H) + R.random_boxes(W, H, 200, 11):
        l, t, r, b = box
        mw, mh = (8 * hs, 8 * vs) if ncomp == 3 else (8, 8)
        want = (l // mw, t // mh, (r - 1) // mw + 1, (b - 1) // mh + 1)
        assert R.brute_window(pm, box) == want
        assert SJ.decode_box_window(W, H, hs, vs, ncomp, box, luma=True) == want, (layout, box)


def test_the_window_depends_on_the_files_edges_not_the_boxs(SJ):
    """4:2:0, 83 x 61 (chroma 42 x 31): a box edge inside the picture reads its real neighbour, the file's edge has none"""
    w = SJ.decode_box_window
    assert w(83, 61, 2, 2, 3, (16, 16, 32, 32)) == (0, 0, 3, 3)          # even left / top edge: column 7 and row 7 of the chroma; odd right / bottom: 16
    assert w(83, 61, 2, 2, 3, (17, 17, 31, 31)) == (1, 1, 2, 2)          # odd left edge reads to the right, even right edge to the left
    assert w(83, 61, 2, 2, 3, (0, 0, 16, 16)) == (0, 0, 2, 2)            # the file's own corner: no neighbour above or to the left
    assert w(83, 61, 2, 2, 3, (80, 48, 83, 61)) == (4, 2, 6, 4)          # pixel 80 is even: chroma column 39 of MCU 4; the last column has no right neighbour
    assert w(96, 80, 2, 2, 3, (0, 36, 96, 44)) == (0, 2, 6, 3)           # chroma rows 17 .. 22: MCU row 2 alone
    assert w(96, 80, 2, 2, 3, (0, 32, 96, 48)) == (0, 1, 6, 4)           # chroma rows 15 and 24 too
    assert w(3, 20, 2, 2, 3, (0, 0, 3, 20)) == (0, 0, 1, 2)              # chroma 2 wide: replication


def test_c_window_refuses_a_box_outside(lib):
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc
    d = JpegDecDesc()
    d.width, d.height, d.hs, d.vs, d.ncomp = 83, 61, 2, 2, 3
    win = (ctypes.c_int32 * 4)(9, 9, 9, 9)
    for bad in ((0, 0, 84, 61), (0, 0, 83, 62), (-1, 0, 4, 4), (4, 4, 4, 8), (8, 4, 4, 8), (0, 5, 3, 5)):
        box = (ctypes.c_int32 * 4)(*bad)
        assert lib.aej_jpegdec_box_window_host(ctypes.addressof(d), ctypes.addressof(box), ctypes.addressof(win)) == -1, bad
        assert tuple(win) == (9, 9, 9, 9)
    assert lib.aej_jpegdec_box_window_host(None, None, None) == -1


# ---- the keyword's refusals: all before any device work, so they show without a device ---------------------------------------------------
def _files():
    return [R.make_file("420", 83, 61), R.make_file("grey", 40, 30), R.make_file("444", 32, 32, progressive=True)]


def _no_device(monkeypatch, SJ):
    def refuse(*a, **k):
        raise AssertionError("device work before the keyword was checked")
    monkeypatch.setattr(SJ, "get_context", refuse)


def test_a_box_outside_the_image_is_a_value_error_naming_the_file(SJ, monkeypatch):
    _no_device(monkeypatch, SJ)
    files = _files()
    for bad in ((0, 0, 41, 30), (0, 0, 40, 31), (-1, 0, 8, 8), (8, 8, 8, 16), (16, 8, 8, 16), (0, 9, 8, 9), (0, 9, 8, 3)):
        with pytest.raises(ValueError, match="file 1"):
            SJ.standard_jpeg_decode_many(files, progressive=True, box=[(0, 0, 83, 61), bad, None])
    with pytest.raises(ValueError, match="file 0"):
        SJ.standard_jpeg_decode_many(files, progressive=True, box=(0, 0, 84, 10))      # one box for every file: the first it does not fit
    with pytest.raises(ValueError, match="file 1"):
        SJ.standard_jpeg_decode_many(files, progressive=True, box=(0, 0, 41, 30))      # fits file 0
    with pytest.raises(ValueError, match="file 2"):
        SJ.standard_jpeg_decode_many(files, progressive=True, box=[None, None, (0, 0, 33, 32)])


def test_what_is_not_a_box_is_a_type_error(SJ, monkeypatch):
    _no_device(monkeypatch, SJ)
    files = _files()
    for bad in (True, 1.5, 7, "0,0,8,8", (0, 0, 8), (0, 0, 8, 8, 8), (0, 0, 8.0, 8), (0, 0, True, 8), (0.5, 0, 8, 8)):
        with pytest.raises(TypeError):
            SJ.standard_jpeg_decode_many(files, progressive=True, box=bad)
    for bad in (True, 1.5, (0, 0, 8), (0, 0, 8.0, 8), (False, 0, 8, 8)):
        with pytest.raises(TypeError, match="file 1"):
            SJ.standard_jpeg_decode_many(files, progressive=True, box=[None, bad, (0, 0, 8, 8)] if isinstance(bad, tuple) else [None, bad, None])


def test_a_list_of_another_length_is_a_value_error(SJ, monkeypatch):
    _no_device(monkeypatch, SJ)
    files = _files()
    for bad in ([None, None], [(0, 0, 8, 8)] * 4, [], [None] * 4):
        with pytest.raises(ValueError, match="box"):
            SJ.standard_jpeg_decode_many(files, progressive=True, box=bad)


def test_a_box_at_another_scale_is_not_built(SJ, monkeypatch):
    _no_device(monkeypatch, SJ)
    files = _files()
    with pytest.raises(NotImplementedError, match="file 1.*a box at scale 2, 4 or 8 is not built"):
        SJ.standard_jpeg_decode_many(files, progressive=True, scale=[1, 2, 4], box=[(0, 0, 8, 8), (0, 0, 8, 8), None])
    with pytest.raises(NotImplementedError, match="file 0.*a box at scale 2, 4 or 8 is not built"):
        SJ.standard_jpeg_decode_many(files, progressive=True, scale=8, box=(1, 1, 2, 2))


def test_decode_box_window_refusals(SJ):
    with pytest.raises(ValueError):
        SJ.decode_box_window(83, 61, 2, 2, 3, (0, 0, 84, 61))
    with pytest.raises(ValueError):
        SJ.decode_box_window(83, 61, 2, 2, 3, (5, 5, 5, 6))
    with pytest.raises(ValueError):
        SJ.decode_box_window(83, 61, 4, 1, 3, (0, 0, 8, 8))
    for bad in ((0, 0, 8), (0, 0, 8.0, 8), True, None):
        with pytest.raises(TypeError):
            SJ.decode_box_window(83, 61, 2, 2, 3, bad)


def test_the_new_entries_resolve(lib):
    for name in ("aej_jpegdec_batch_box", "aej_jpegdec_workspace_bytes_box", "aej_jpegprog_batch_box", "aej_jpegprog_workspace_bytes_box",
                 "aej_jpegdec_box_window_host", "aej_jpegprog_box_window_host", "aej_jpegdec_box_stats"):
        assert getattr(lib, name) is not None
    assert lib.aej_jpegdec_box_stats(None, None) == -1
    assert lib.aej_jpegdec_workspace_bytes_box(None, None, 1, None, None, None) == 0
