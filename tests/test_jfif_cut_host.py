"""CPU: the host side of crop= and drop_chroma= of standard_jpeg_transform_many -- the mapping k_jt_cut runs
(aej_jfif_transform_coefs_host_cut) and the geometry entry against a NumPy restatement (jfif_cut_reference), the markers of a cut file
(transform_prefix), transform_crop_box and every refusal.  No device is touched."""
import ctypes
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_cut_reference as C  # noqa: E402
import jfif_transform_reference as R  # noqa: E402

# (H, W) drawn from {1, 7, 8, 9, 15, 16, 17, 31, 33, 40}^2: one block, partial blocks, one MCU of every layout and one pixel more or less,
# several MCUs with a partial one on either axis, whole MCUs of every layout
SIZES = ((1, 1), (8, 8), (7, 9), (16, 16), (15, 17), (17, 33), (33, 31), (16, 40), (40, 33), (9, 15), (31, 8), (40, 40))
# (name, hs, vs, components, layout_440)
LAYOUTS = (("4:4:4", 1, 1, 3, 0), ("4:2:2", 2, 1, 3, 0), ("4:2:0", 2, 2, 3, 0), ("4:4:0", 1, 2, 3, 1), ("4:2:2 to 4:4:0", 2, 1, 3, 1),
           ("grey", 1, 1, 1, 0))


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


def _boxes(h, w):
    """boxes of an h x w transformed image: the whole image, unaligned corners, right / lower edges that leave an odd number of luma
    blocks (so that a 2 x 2 MCU gets dummies), single pixels"""
    out = [(0, 0, w, h), (min(3, w - 1), min(5, h - 1), w, h), (0, 0, min(w, 17), min(h, 9)), (0, 0, min(w, 24), min(h, 23)),
           (min(9, w - 1), min(10, h - 1), min(w, 9 + 17), min(h, 10 + 7)), (min(19, w - 1), min(9, h - 1), w, min(h, 30)),
           (w - 1, h - 1, w, h), (0, 0, 1, 1), (min(17, w - 1), min(8, h - 1), min(17, w - 1) + 1, min(8, h - 1) + 1)]
    return sorted(set(out))


def _geometry(lib, H, W, hs, vs, nc, code, trim, allow, box, drop):
    out = (ctypes.c_int32 * 6)()
    b = (ctypes.c_int32 * 4)(*box) if box is not None else None
    rc = lib.aej_jfif_transform_geometry_host_cut(H, W, hs, vs, nc, code, int(trim), allow, ctypes.addressof(b) if b is not None else None, int(drop),
                                                  ctypes.addressof(out))
    return rc, tuple(out)


def _coefs(lib, H, W, hs, vs, nc, code, trim, allow, box, drop, src, n_src, dst, n_dst):
    b = (ctypes.c_int32 * 4)(*box) if box is not None else None
    return lib.aej_jfif_transform_coefs_host_cut(H, W, hs, vs, nc, code, int(trim), allow, ctypes.addressof(b) if b is not None else None, int(drop),
                                                 src.ctypes.data if src is not None else None, n_src, dst.ctypes.data if dst is not None else None, n_dst)


@pytest.mark.parametrize("drop", (False, True), ids=("keep", "drop_chroma"))
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0].replace(" ", "_") for l in LAYOUTS])
@pytest.mark.parametrize("name", R.NAMES)
def test_coefficients_equal_numpy_restatement(lib, name, layout, drop):
    _, hs, vs, nc, allow = layout
    grey = nc == 1
    code = R.NAMES.index(name)
    ran = cut_ran = dummies = 0
    for H, W in SIZES:
        n_src = -(-W // 8) * -(-H // 8) if grey else (hs * vs + 2) * -(-W // (8 * hs)) * -(-H // (8 * vs))
        src = np.random.default_rng(H * 100 + W).integers(-32767, 32768, (n_src, 64)).astype(np.int16)
        planes = C.source_planes(src.astype(np.int64), H, W, hs, vs, grey)
        for trim in (False, True):
            rc, _ = _geometry(lib, H, W, hs, vs, nc, code, trim, allow, None, drop)
            if name in R.TRANSPOSING and hs != vs and not allow and not drop:
                assert rc == -5                                   # AEJ_ERR_UNSUPPORTED: it would be 4:4:0
                ran += 1
                continue
            try:
                (tH, tW, ohs, ovs), _ = C.geometry(H, W, hs, vs, name, trim, None, drop, grey)
            except ValueError as e:
                assert rc == (2 if str(e) == "nothing left" else 1), (H, W, trim, rc)
                assert _coefs(lib, H, W, hs, vs, nc, code, trim, allow, None, drop, None, 0, None, 0) == -1
                continue
            assert rc == 0
            for box in [None] + _boxes(tH, tW):
                real, (oH, oW, ohs, ovs), kept = C.cut(planes, H, W, hs, vs, name, trim, box, drop)
                rc, geo = _geometry(lib, H, W, hs, vs, nc, code, trim, allow, box, drop)
                assert rc == 0 and geo == (oH, oW, ohs, ovs, kept[0], kept[1]), (H, W, trim, box, rc, geo)
                one = len(real) == 1
                assert one == (drop or grey)
                n_out = -(-oW // 8) * -(-oH // 8) if one else (ohs * ovs + 2) * -(-oW // (8 * ohs)) * -(-oH // (8 * ovs))
                assert _coefs(lib, H, W, hs, vs, nc, code, trim, allow, box, drop, None, 0, None, 0) == n_out
                dst = np.full((n_out + 1, 64), 12345, np.int16)      # one block of canary
                assert _coefs(lib, H, W, hs, vs, nc, code, trim, allow, box, drop, src, n_src, dst, n_out) == n_out
                assert (dst[n_out] == 12345).all()
                want = C.to_output_order(real, oH, oW, ohs, ovs)
                whole = tuple(kept) == (0, 0, tW, tH)            # after the alignment: the whole image is no crop
                if name == "none" and whole and not (drop and not grey):      # the transcode: every block carried as it is, the dummies too
                    want = src.astype(np.int64)
                natural = np.zeros((n_out, 64), np.int64)
                natural[:, R.ZZ] = dst[:n_out]                    # the entry writes the coders' zigzag order
                assert np.array_equal(natural, want), (name, layout, H, W, trim, box, drop)
                if whole and not drop:                            # no cut: the _440 entry's answer
                    old = np.zeros_like(dst)
                    fn = lib.aej_jfif_transform_coefs_grey_host
                    got = fn(H, W, code, int(trim), src.ctypes.data, n_src, old.ctypes.data, n_out) if grey else \
                        lib.aej_jfif_transform_coefs_host_440(H, W, hs, vs, code, int(trim), allow, src.ctypes.data, n_src, old.ctypes.data, n_out)
                    assert got == n_out and np.array_equal(old[:n_out], dst[:n_out])
                assert _coefs(lib, H, W, hs, vs, nc, code, trim, allow, box, drop, src, n_src + 1, dst, n_out) == -1
                assert _coefs(lib, H, W, hs, vs, nc, code, trim, allow, box, drop, src, n_src, dst, n_out - 1) == -4
                ran += 1
                cut_ran += not whole
                dummies += (not one) and (-(-oW // 8) % ohs != 0 or -(-oH // 8) % ovs != 0)
            # boxes that do not lie inside the (trimmed) transformed image
            for box in ((0, 0, tW + 1, tH), (0, 0, tW, tH + 1), (-1, 0, tW, tH), (0, -8, tW, tH), (tW, 0, tW, tH), (0, tH - 1, tW, tH - 1), (5, 0, 5, tH),
                        (min(3, tW - 1), 0, min(2, tW - 1), tH)):
                if box[2] == 0:
                    continue                                      # right == 0 is the ABI's "no crop"
                assert _geometry(lib, H, W, hs, vs, nc, code, trim, allow, box, drop)[0] == 3, (H, W, box)
                assert _coefs(lib, H, W, hs, vs, nc, code, trim, allow, box, drop, None, 0, None, 0) == -1
    assert ran >= 6 and (cut_ran >= 20 or ran == 24)
    if layout[0] == "4:2:0" and not drop:
        assert dummies > 10


def test_restatement_agrees_with_pixels_on_dc_only_tiles():
    """the restatement itself, checked on pixels: an image of constant 8 x 8 tiles has DC-only blocks, so the cut of its DC grid is the
    DC grid of the cut of the transformed image"""
    tiles = np.random.default_rng(5).integers(0, 256, (3, 5), dtype=np.int64)
    coef = np.zeros((3, 5, 64), np.int64)
    coef[:, :, 0] = tiles
    for name in R.NAMES:
        t = R.pixels(np.repeat(np.repeat(tiles, 8, 0), 8, 1), name)
        for box in ((9, 3, 23, 24), (8, 16, 9, 17), (0, 0, 24, 24), (17, 9, 24, 10)):
            real, (oH, oW, _, _), (L, U, right, lower) = C.cut([coef] * 3, 24, 40, 1, 1, name, False, box)
            assert (L, U) == (box[0] // 8 * 8, box[1] // 8 * 8) and (oH, oW) == (lower - U, right - L)
            want = t[U:lower, L:right][::8, ::8]
            assert np.array_equal(real[0][:, :, 0], want) and np.array_equal(real[1][:, :, 0], want), (name, box)


def _noise(H, W, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _pil(x, **opts):
    from PIL import Image
    img = x if isinstance(x, Image.Image) else Image.fromarray(x)
    buf = io.BytesIO()
    img.save(buf, "JPEG", **opts)
    return buf.getvalue()


def _segments(data):
    """[(marker, whole segment bytes)] of a run of marker segments after SOI -- an independent walk"""
    i, out = 2, []
    while i < len(data):
        assert data[i] == 0xFF
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((data[i + 1], data[i:i + 2 + n]))
        i += 2 + n
    return out


def _tail(data):
    """a file's bytes from its first DHT on"""
    return data[data.index(b"\xff\xc4"):]


def want0(plain, name):
    """the luma table of a prefix in natural order, transposed by a transposing transform"""
    t = np.zeros(64, np.int64)
    t[R.ZZ] = list(_segments(plain)[1][1][5:])
    return t.reshape(8, 8).T.reshape(64) if name in R.TRANSPOSING else t


QT = ([(3 * i) % 254 + 1 for i in range(64)], [(7 * i + 5) % 255 + 1 for i in range(64)])


def test_prefix(SJ):
    """transform_prefix(crop=, drop_chroma=), walked by hand and parsed back by parse_header (completed to a file by the tables and
    scan of a Pillow file of the same kind, which the header parser does not decode)"""
    from PIL import Image
    x = _noise(37, 50)
    grey_tail = _tail(_pil(Image.fromarray(x).convert("L"), quality=75))
    for layout, (hs, vs) in (("4:2:0", (2, 2)), ("4:2:2", (2, 1)), ("4:4:4", (1, 1))):
        src = _pil(x, qtables=[list(QT[0]), list(QT[1])], subsampling=layout, dpi=(300, 72))
        colour_tail = _tail(src)
        for prog in (False, True):
            plain = SJ.transform_prefix(src, "none", progressive=prog)
            assert SJ.transform_prefix(src, "none", progressive=prog, crop=None, drop_chroma=False) == plain
            assert SJ.transform_prefix(src, "none", progressive=prog, crop=(0, 0, 50, 37)) == plain
            for name, trim, box in (("none", False, (19, 9, 43, 30)), ("rot90", True, (3, 5, 20, 31)), ("flip_v", True, (0, 17, 50, 18)),
                                    ("transverse", True, (9, 9, 10, 10))):
                for drop in (False, True):
                    if name in R.TRANSPOSING and hs != vs and not drop:
                        with pytest.raises(NotImplementedError, match=r"file 0.*4:4:0"):
                            SJ.transform_prefix(src, name, progressive=prog, trim=trim, crop=box)
                        continue
                    (oH, oW, ohs, ovs), kept = C.geometry(37, 50, hs, vs, name, trim, box, drop)
                    assert SJ.transform_crop_box(src, name, box, trim=trim, drop_chroma=drop) == kept
                    got = SJ.transform_prefix(src, name, progressive=prog, trim=trim, crop=box, drop_chroma=drop)
                    segs = _segments(got)
                    assert got[:20] == plain[:20]                 # SOI and the JFIF APP0 with the source's density
                    assert [m for m, _ in segs] == [0xE0] + [0xDB] * (1 if drop else 2) + [0xC2 if prog else 0xC0]
                    sof = segs[-1][1]
                    assert struct.unpack(">HH", sof[5:9]) == (oH, oW) and sof[9] == (1 if drop else 3)
                    assert sof[11] == (0x11 if drop else (ohs << 4) | ovs) and sof[10] == 1 and sof[12] == 0
                    if not drop:
                        assert bytes(sof[13:19]) == bytes([2, 0x11, 1, 3, 0x11, 1])
                    for k, (_, dqt) in enumerate(segs[1:-1]):     # the source's tables (the plain prefix's), transposed with the image
                        t, want = np.zeros(64, np.int64), np.zeros(64, np.int64)
                        t[R.ZZ] = list(dqt[5:])
                        want[R.ZZ] = list(_segments(plain)[1 + k][1][5:])
                        want = want.reshape(8, 8)
                        assert not np.array_equal(want, want.T)
                        assert dqt[4] == k and np.array_equal(t.reshape(8, 8), want.T if name in R.TRANSPOSING else want), (name, k)
                    if prog:
                        continue
                    d = SJ.parse_header(got + (grey_tail if drop else colour_tail))
                    assert (d.height, d.width, d.ncomp) == (oH, oW, 1 if drop else 3)
                    assert (d.hs, d.vs) == (ohs, ovs)
                    assert [int(v) for v in d.qt[0]] == [int(v) for v in want0(plain, name)]
    # a grey source: with grey=True, and drop_chroma changes nothing
    g = _pil(Image.fromarray(x).convert("L"), quality=60)
    for drop in (False, True):
        got = SJ.transform_prefix(g, "rot270", trim=True, grey=True, crop=(9, 9, 30, 40), drop_chroma=drop)
        sof = _segments(got)[-1][1]
        assert struct.unpack(">HH", sof[5:9]) == (32, 22) and sof[9] == 1      # 48 x 37 after the trim of 50 to 48; the corner on (8, 8)
        assert SJ.transform_crop_box(g, "rot270", (9, 9, 30, 40), trim=True, grey=True, drop_chroma=drop) == (8, 8, 30, 40)
    assert SJ.transform_prefix(g, "none", grey=True, drop_chroma=True) == SJ.transcode_prefix(g, grey=True)
    # a 4:2:2 source transposed into 4:4:0 with a crop: the corner on the 8 x 16 grid
    src = _pil(x, quality=75, subsampling="4:2:2")
    assert SJ.transform_crop_box(src, "transpose", (9, 17, 30, 40), layout_440=True) == (8, 16, 30, 40)
    assert SJ.transform_crop_box(src, "transpose", (9, 17, 30, 40), drop_chroma=True) == (8, 16, 30, 40)
    assert SJ.transform_crop_box(src, "none", (17, 9, 30, 30)) == (16, 8, 30, 30)
    assert SJ.transform_crop_box(src, "none", (17, 9, 30, 30), drop_chroma=True) == (16, 8, 30, 30)
    src = _pil(x, quality=75, subsampling="4:2:0")
    assert SJ.transform_crop_box(src, "none", (19, 9, 43, 30)) == (16, 0, 43, 30)
    assert SJ.transform_crop_box(src, "none", (19, 9, 43, 30), drop_chroma=True) == (16, 8, 43, 30)
    assert SJ.transform_crop_box(src, "rot90", (19, 9, 32, 50), trim=True) == (16, 0, 32, 50)      # 32 x 50: the height 37 trims to 32


def test_refusals_before_any_device_work(SJ, monkeypatch):
    from PIL import Image
    from adaptive_edge_aware_jpeg_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a refusal reached the device")
    monkeypatch.setattr(_lib, "get_context", no_device)
    monkeypatch.setattr(SJ, "get_context", no_device)
    ok = _pil(_noise(37, 50), quality=50, subsampling="4:2:0")
    T = SJ.standard_jpeg_transform_many
    # out of range, in the transformed image's coordinates (rot90: 37 wide, 50 high); nothing is clamped
    for box in ((0, 0, 51, 37), (0, 0, 50, 38), (-1, 0, 50, 37), (0, -1, 50, 37), (50, 0, 51, 37)):
        with pytest.raises(ValueError, match=r"file 1: crop .* does not lie inside the 50 x 37 image"):
            T([ok, ok], "none", crop=[None, box])
        with pytest.raises(ValueError, match=r"file 0: crop .* does not lie inside the 50 x 37 image"):
            SJ.transform_prefix(ok, "none", crop=box)
        with pytest.raises(ValueError, match=r"file 3: crop .* does not lie inside the 50 x 37 image"):
            SJ.transform_crop_box(ok, "none", box, index=3)
    with pytest.raises(ValueError, match=r"file 1: crop .* does not lie inside the 32 x 50 image"):
        T([ok, ok], ["none", "rot90"], trim=True, crop=[None, (0, 0, 37, 50)])
    assert SJ.transform_crop_box(ok, "rot90", (0, 0, 32, 50), trim=True) == (0, 0, 32, 50)
    # left >= right, upper >= lower
    for box in ((10, 0, 10, 37), (11, 0, 10, 37), (0, 20, 50, 20), (0, 21, 50, 20)):
        with pytest.raises(ValueError, match=r"file 0: crop .* does not lie inside"):
            T([ok, ok], "none", crop=box)
        with pytest.raises(ValueError, match=r"file 1: crop .* does not lie inside"):
            T([ok, ok], "none", crop=[(0, 0, 8, 8), box])
    # a box inside the strip the trim dropped: flip_h trims 50 to 48
    with pytest.raises(ValueError, match=r"file 1: crop .* does not lie inside the 48 x 37 image that flip_h with trim=True leaves"):
        T([ok, ok], "flip_h", trim=True, crop=[None, (40, 0, 49, 37)])
    with pytest.raises(ValueError, match=r"file 0.*trim=True"):     # perfect is decided on the whole source first
        T([ok], "flip_h", crop=(0, 0, 16, 16))
    with pytest.raises(ValueError, match=r"file 0.*8 x 8 MCUs.*trim=True"):
        T([ok], "flip_h", drop_chroma=True)                       # 50 is no multiple of 8 either
    # entries that are no boxes
    for bad in ((0, 0, True, 8), (0, 0, 8.0, 8), (0, 0, 8), (0, 0, 8, 8, 8), "abcd", (0, 0, "8", 8), (False, 0, 8, 8)):
        with pytest.raises(ValueError, match=r"file 1: crop .*four ints"):
            T([ok, ok], "none", crop=[None, bad])
        with pytest.raises(ValueError, match=r"file 2: crop .*four ints"):
            SJ.transform_crop_box(ok, "none", bad, index=2)
        with pytest.raises(ValueError, match=r"file 2: crop .*four ints"):
            SJ.transform_prefix(ok, "none", crop=bad, index=2)
    for bad in ((0, 0, True, 8), (0, 0, 8.0, 8), (0, 0, 8), (0, 0, 8, 8, 8)):      # plain values: one box for every file
        with pytest.raises(ValueError, match=r"file 0: crop .*four ints"):
            T([ok, ok], "none", crop=bad)
    for bad in (5, "0,0,8,8", 1.5):
        with pytest.raises(ValueError, match=r"file 0: crop"):
            T([ok, ok], "none", crop=bad)
    with pytest.raises(ValueError, match=r"file 0: crop None"):
        SJ.transform_crop_box(ok, "none", None)
    # a sequence of the wrong length: the message shape of transform=
    with pytest.raises(ValueError, match="file 1: 1 crop boxes for 2 files"):
        T([ok, ok], "none", crop=[(0, 0, 8, 8)])
    with pytest.raises(ValueError, match="file 2: 3 crop boxes for 2 files"):
        T([ok, ok], "none", crop=[None, None, (0, 0, 8, 8)])
    with pytest.raises(ValueError, match="file 0: 0 crop boxes for 2 files"):
        T([ok, ok], "none", crop=[])
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="drop_chroma"):
            T([ok], "none", drop_chroma=bad)
        with pytest.raises(TypeError, match="drop_chroma"):
            SJ.transform_prefix(ok, "none", drop_chroma=bad)
        with pytest.raises(TypeError, match="drop_chroma"):
            SJ.transform_crop_box(ok, "none", (0, 0, 8, 8), drop_chroma=bad)
    # what the call refused before is refused still, in the same words
    wide = _pil(_noise(32, 48), quality=50, subsampling="4:2:2")
    with pytest.raises(NotImplementedError, match=r"file 1.*rot90.*4:4:0"):
        T([ok, wide], "rot90", trim=True, crop=(0, 0, 8, 8))
    grey = _pil(Image.fromarray(_noise(16, 16)).convert("L"), quality=50)
    with pytest.raises(NotImplementedError, match="file 1"):
        T([ok, grey], "none", crop=(0, 0, 8, 8), drop_chroma=True)      # one-component sources still need grey=True
    e = Image.Exif()
    e[0x0112] = 6                                                # "exif": the box is in the upright image's coordinates
    turned = _pil(_noise(37, 50), quality=50, subsampling="4:2:0", exif=e.tobytes())
    with pytest.raises(ValueError, match=r"file 1: crop .* does not lie inside the 32 x 50 image that rot90 with trim=True"):
        T([ok, turned], "exif", trim=True, crop=[None, (0, 0, 33, 50)])


def test_abi(SJ, lib):
    import adaptive_edge_aware_jpeg_amd as A
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "aej.h")) as f:
        header = f.read()
    for name in ("aej_jfif_transform_geometry_host_cut", "aej_jfif_transform_coefs_host_cut", "aej_jfif_transform_headers_host_cut",
                 "aej_jfif_transform_workspace_bytes_cut", "aej_jfif_transform_batch_cut"):
        assert getattr(lib, name) is not None and f"{name}(" in header
    assert lib.aej_abi_version() == 3
    assert A.transform_crop_box is SJ.transform_crop_box and A.transform_prefix is SJ.transform_prefix
    assert "transform_crop_box" in A.__all__ and "transform_prefix" in A.__all__
    box = (ctypes.c_int32 * 4)(0, 0, 8, 8)
    at = ctypes.addressof(box)
    assert lib.aej_jfif_transform_geometry_host_cut(8, 8, 1, 1, 3, 0, 0, 0, at, 2, None) == -1       # drop_chroma: 0 or 1
    assert lib.aej_jfif_transform_geometry_host_cut(8, 8, 1, 1, 2, 0, 0, 0, at, 0, None) == -1       # components: 1 or 3
    assert lib.aej_jfif_transform_geometry_host_cut(8, 8, 1, 2, 3, 0, 0, 0, at, 1, None) == -1       # a 4:4:0 source without layout_440
    assert lib.aej_jfif_transform_geometry_host_cut(8, 8, 1, 2, 3, 0, 0, 1, at, 1, None) == 0
    assert lib.aej_jfif_transform_geometry_host_cut(8, 8, 1, 1, 3, 0, 0, 0, at, 0, None) == 0
    zero = (ctypes.c_int32 * 4)(5, 5, 0, 0)                      # right == 0: no crop, whatever the rest holds
    out = (ctypes.c_int32 * 6)()
    assert lib.aej_jfif_transform_geometry_host_cut(9, 17, 2, 2, 3, 0, 0, 0, ctypes.addressof(zero), 0, ctypes.addressof(out)) == 0
    assert tuple(out) == (9, 17, 2, 2, 0, 0)
    buf = (ctypes.c_uint8 * 16)()
    assert lib.aej_jfif_transform_headers_host_cut(None, None, None, 0, 1, 0, 0, at, 0, ctypes.addressof(buf), 16) == -1
