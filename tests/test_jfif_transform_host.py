"""CPU: the host side of standard_jpeg_transform_many -- the coefficient mapping the kernel runs (aej_jfif_transform_coefs_host) against
a NumPy restatement, the markers of a transformed file (transform_prefix), the EXIF Orientation reader, the refusals and the new ABI
symbols.  No device is touched."""
import ctypes
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_transform_reference as R  # noqa: E402

QT = ([(3 * i) % 254 + 1 for i in range(64)], [(7 * i + 5) % 255 + 1 for i in range(64)])
# (H, W): one block, one MCU of every layout, partial blocks and partial MCUs on either axis, several MCUs
SIZES = ((1, 1), (8, 8), (3, 9), (16, 16), (33, 17), (53, 37), (32, 48), (48, 64), (24, 40), (9, 41))


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


def _noise(H, W, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _pil(x, **opts):
    from PIL import Image
    img = x if isinstance(x, Image.Image) else Image.fromarray(x)
    buf = io.BytesIO()
    img.save(buf, "JPEG", **opts)
    return buf.getvalue()


def _segments(data):
    """[(marker, whole segment bytes)] between SOI and the first SOS -- an independent walk"""
    i, out = 2, []
    while data[i + 1] != 0xDA:
        assert data[i] == 0xFF
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((data[i + 1], data[i:i + 2 + n]))
        i += 2 + n
    return out


def _geometry(lib, H, W, hs, vs, code, trim):
    out = (ctypes.c_int32 * 4)()
    return lib.aej_jfif_transform_geometry_host(H, W, hs, vs, code, int(trim), ctypes.addressof(out)), tuple(out)


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("name", R.NAMES)
def test_coefficients_equal_numpy_restatement(lib, name, layout):
    hs, vs = R.LAYOUTS[layout]
    code = R.NAMES.index(name)
    ran = 0
    for H, W in SIZES:
        for trim in (False, True):
            rc, geo = _geometry(lib, H, W, hs, vs, code, trim)
            if name in R.TRANSPOSING and hs != vs:
                assert rc == -5                                   # AEJ_ERR_UNSUPPORTED: it would be 4:4:0
                assert lib.aej_jfif_transform_coefs_host(H, W, hs, vs, code, int(trim), None, 0, None, 0) == -5
                ran += 1
                continue
            try:
                want_geo = R.out_geometry(H, W, hs, vs, name, trim)
            except ValueError as e:
                assert rc == (2 if str(e) == "nothing left" else 1), (H, W, trim, rc)
                assert lib.aej_jfif_transform_coefs_host(H, W, hs, vs, code, int(trim), None, 0, None, 0) == rc
                continue
            assert rc == 0 and geo == want_geo, (H, W, trim, rc, geo, want_geo)
            n_src = (hs * vs + 2) * -(-W // (8 * hs)) * -(-H // (8 * vs))
            oH, oW, ohs, ovs = want_geo
            n_out = (ohs * ovs + 2) * -(-oW // (8 * ohs)) * -(-oH // (8 * ovs))
            assert lib.aej_jfif_transform_coefs_host(H, W, hs, vs, code, int(trim), None, 0, None, 0) == n_out
            src = np.random.default_rng(H * 100 + W).integers(-32767, 32768, (n_src, 64)).astype(np.int16)
            dst = np.full((n_out + 1, 64), 12345, np.int16)      # one block of canary
            got = lib.aej_jfif_transform_coefs_host(H, W, hs, vs, code, int(trim), src.ctypes.data, n_src, dst.ctypes.data, n_out)
            assert got == n_out and (dst[n_out] == 12345).all()
            real, _ = R.coefficients(R.to_planes(src.astype(np.int64), H, W, hs, vs), H, W, hs, vs, name, trim)
            want = R.to_mcu_order(real, oH, oW, ohs, ovs)
            if name == "none":                                    # the transcode: every block carried as it is, the dummies too
                want = src.astype(np.int64)
            natural = np.zeros((n_out, 64), np.int64)
            natural[:, R.ZZ] = dst[:n_out]                        # the entry writes the coders' zigzag order
            assert np.array_equal(natural, want), (name, layout, H, W, trim)
            # wrong block counts are refused and nothing is written
            assert lib.aej_jfif_transform_coefs_host(H, W, hs, vs, code, int(trim), src.ctypes.data, n_src + 1, dst.ctypes.data, n_out) == -1
            assert lib.aej_jfif_transform_coefs_host(H, W, hs, vs, code, int(trim), src.ctypes.data, n_src, dst.ctypes.data, n_out - 1) == -4
            ran += 1
    assert ran >= 6


def test_restatement_agrees_with_pillow_on_dc_only_tiles():
    """the restatement itself, checked on pixels: an image of constant 8 x 8 tiles has DC-only blocks, so the transform of its DC grid is
    the DC grid of the transformed image"""
    tiles = np.random.default_rng(5).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    x = np.repeat(np.repeat(tiles, 8, 0), 8, 1)
    for name in R.NAMES:
        y = R.pixels(x, name)
        assert y.shape[:2] == R.out_geometry(24, 40, 1, 1, name, False)[:2]
        grid = tiles[:, :, 0].astype(np.int64)
        coef = np.zeros((3, 5, 64), np.int64)
        coef[:, :, 0] = grid
        real, _ = R.coefficients([coef] * 3, 24, 40, 1, 1, name, False)
        assert np.array_equal(real[0][:, :, 0], R.pixels(grid, name)) and not real[0][:, :, 1:].any()


def _frame(data):
    sof = next(s for m, s in _segments(data) if m in (0xC0, 0xC2))
    h, w = struct.unpack(">HH", sof[5:9])
    return h, w, [(sof[10 + 3 * k], sof[11 + 3 * k] >> 4, sof[11 + 3 * k] & 15, sof[12 + 3 * k]) for k in range(3)]


@pytest.mark.parametrize("opts", (dict(quality=75, subsampling="4:2:0"), dict(qtables=[list(QT[0]), list(QT[1])], subsampling="4:2:0"),
                                  dict(quality=30, subsampling="4:4:4", dpi=(300, 72))), ids=("q75", "qtables", "dpi-444"))
def test_prefix_of_transposing_transforms(SJ, opts):
    from PIL import Image
    x = np.ascontiguousarray(_noise(61, 90))
    for kind in (dict(), dict(progressive=True)):
        src = _pil(x, **opts, **kind)
        sh, sw, scomps = _frame(src)
        assert (sh, sw) == (61, 90)
        sq = Image.open(io.BytesIO(src)).quantization
        for prog in (False, True):
            plain = SJ.transcode_prefix(src, progressive=prog)
            assert SJ.transform_prefix(src, "none", progressive=prog) == plain
            for name in R.TRANSPOSING:
                got = SJ.transform_prefix(src, name, progressive=prog, trim=True)
                oH, oW, ohs, ovs = R.out_geometry(61, 90, scomps[0][1], scomps[0][2], name, True)
                h, w, comps = _frame(got + b"\xff\xda")
                assert (h, w) == (oH, oW) and (comps[0][1], comps[0][2]) == (ohs, ovs) == (scomps[0][2], scomps[0][1]), name
                assert [(c[0], c[3]) for c in comps] == [(c[0], c[3]) for c in scomps] and comps[1][1:3] == comps[2][1:3] == (1, 1)
                assert [m for m, _ in _segments(got + b"\xff\xda")] == [m for m, _ in _segments(plain + b"\xff\xda")]
                assert got[:20] == plain[:20]                     # SOI and the JFIF APP0 with the source's density
                assert got[-19] == 0xFF and got[-18] == (0xC2 if prog else 0xC0)
                # Pillow reads the tables of the prefix (completed to a file it can open by the source's own scans)
                oq = Image.open(io.BytesIO(got + src[len(plain):])).quantization
                assert set(oq) == set(sq)
                for k in sq:
                    assert list(oq[k]) == list(np.array(sq[k]).reshape(8, 8).T.reshape(64)), (name, k)
                if "qtables" in opts:
                    assert list(oq[0]) != list(sq[0])


def test_prefix_of_mirroring_transforms(SJ):
    for layout, (hs, vs) in R.LAYOUTS.items():
        src = _pil(_noise(61, 90), quality=60, subsampling=layout)
        plain = SJ.transcode_prefix(src)
        for name in ("flip_h", "flip_v", "rot180"):
            oH, oW, _, _ = R.out_geometry(61, 90, hs, vs, name, True)
            want = bytearray(plain)
            want[-14:-10] = struct.pack(">HH", oH, oW)            # SOF: FF C0, length, precision, then height and width
            assert (oH, oW) != (61, 90)
            assert SJ.transform_prefix(src, name, trim=True) == bytes(want), (layout, name)
        perfect = _pil(_noise(48, 64), quality=60, subsampling=layout)
        for name in ("flip_h", "flip_v", "rot180"):
            for trim in (False, True):
                assert SJ.transform_prefix(perfect, name, trim=trim) == SJ.transcode_prefix(perfect)
                assert SJ.transform_prefix(perfect, name, progressive=True, trim=trim) == SJ.transcode_prefix(perfect, progressive=True)


def _with_app1(data, payload):
    assert data[2:4] == b"\xff\xe0"
    return data[:20] + b"\xff\xe1" + struct.pack(">H", 2 + len(payload)) + payload + data[20:]


def _tiff(order, entries, ifd_at=8):
    """a TIFF block of one IFD by hand: order '<' or '>'; entries [(tag, type, count, the four value bytes)]"""
    head = (b"II*\x00" if order == "<" else b"MM\x00*") + struct.pack(order + "I", ifd_at) + bytes(ifd_at - 8)
    body = struct.pack(order + "H", len(entries))
    for tag, typ, count, value in entries:
        body += struct.pack(order + "HHI", tag, typ, count) + value
    return b"Exif\x00\x00" + head + body + bytes(4)


def _oracle(data):
    from PIL import Image
    return Image.open(io.BytesIO(data)).getexif().get(0x0112, 1)


def test_exif_orientation(SJ):
    from PIL import Image
    import adaptive_edge_aware_jpeg_amd as A
    assert A.exif_orientation is SJ.exif_orientation
    x = _noise(16, 16)
    plain = _pil(x, quality=75)
    assert SJ.exif_orientation(plain) == 1 == _oracle(plain)      # no APP1
    written = set()
    for v in range(1, 9):
        e = Image.Exif()
        e[0x010E] = "a description"
        e[0x0112] = v
        f = _pil(x, quality=75, exif=e.tobytes())
        order = "<" if e.tobytes()[6:8] == b"II" else ">"
        written.add(order)
        assert SJ.exif_orientation(f) == v == _oracle(f), v
        other = "<" if order == ">" else ">"                      # the byte order Pillow does not write, by hand
        g = _with_app1(plain, _tiff(other, [(0x0112, 3, 1, struct.pack(other + "HH", v, 0))]))
        assert SJ.exif_orientation(g) == v == _oracle(g), (other, v)
        g = _with_app1(plain, _tiff(other, [(0x010F, 2, 2, b"a\x00\x00\x00"), (0x0112, 3, 1, struct.pack(other + "HH", v, 0))], ifd_at=12))
        assert SJ.exif_orientation(g) == v == _oracle(g), (other, v, "second entry, IFD not at 8")
    assert len(written) == 1
    # nothing usable -> 1: the tag absent, values outside 1..8, a truncated block, another APP1, a bad byte order mark
    e = Image.Exif()
    e[0x010E] = "no orientation here"
    f = _pil(x, quality=75, exif=e.tobytes())
    assert SJ.exif_orientation(f) == 1 == _oracle(f)
    for v in (0, 9, 0x0100):
        assert SJ.exif_orientation(_with_app1(plain, _tiff(">", [(0x0112, 3, 1, struct.pack(">HH", v, 0))]))) == 1
    whole = _tiff(">", [(0x0112, 3, 1, struct.pack(">HH", 6, 0))])
    for cut in (6, 10, 14, 16, 20, 25):
        assert SJ.exif_orientation(_with_app1(plain, whole[:cut])) == 1, cut
    assert SJ.exif_orientation(_with_app1(plain, b"http://ns.adobe.com/xap/1.0/\x00<x/>")) == 1
    assert SJ.exif_orientation(_with_app1(plain, whole.replace(b"MM\x00*", b"MM\x00+"))) == 1
    assert SJ.exif_orientation(_with_app1(plain, whole.replace(struct.pack(">I", 8), struct.pack(">I", 4000), 1))) == 1      # IFD0 outside
    assert SJ.exif_orientation(b"\xff\xd8\xff") == 1 and SJ.exif_orientation(b"") == 1


def test_refusals_before_any_device_work(SJ, monkeypatch):
    from PIL import Image
    from adaptive_edge_aware_jpeg_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a refusal reached the device")
    monkeypatch.setattr(_lib, "get_context", no_device)
    monkeypatch.setattr(SJ, "get_context", no_device)
    ok = _pil(_noise(16, 16), quality=50, subsampling="4:2:0")
    with pytest.raises(ValueError, match="file 0.*unknown transform 'rot45'"):
        SJ.standard_jpeg_transform_many([ok, ok], "rot45")
    with pytest.raises(ValueError, match="file 1.*unknown transform 'flip'"):
        SJ.standard_jpeg_transform_many([ok, ok], ["flip_h", "flip"])
    with pytest.raises(ValueError, match="file 1.*unknown transform 'exif'"):
        SJ.standard_jpeg_transform_many([ok, ok], ["flip_h", "exif"])
    with pytest.raises(ValueError, match="file 1.*unknown transform 5"):
        SJ.standard_jpeg_transform_many([ok, ok], ["flip_h", 5])
    with pytest.raises(ValueError, match="file 1: 1 transforms for 2 files"):
        SJ.standard_jpeg_transform_many([ok, ok], ["flip_h"])
    with pytest.raises(ValueError, match="file 2: 3 transforms for 2 files"):
        SJ.standard_jpeg_transform_many([ok, ok], ["flip_h"] * 3)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="trim"):
            SJ.standard_jpeg_transform_many([ok], "flip_h", trim=bad)
        with pytest.raises(TypeError, match="trim"):
            SJ.transform_prefix(ok, "flip_h", trim=bad)
    for kw in (dict(progressive=1), dict(keep_metadata=None)):
        with pytest.raises(TypeError):
            SJ.standard_jpeg_transform_many([ok], "flip_h", **kw)
    with pytest.raises(ValueError):
        SJ.standard_jpeg_transform_many([], "flip_h")
    small = _pil(_noise(3, 9), quality=50, subsampling="4:4:4")              # 9 x 3: a partial block column
    with pytest.raises(ValueError, match=r"file 1.*trim=True"):
        SJ.standard_jpeg_transform_many([ok, small], "flip_h")
    with pytest.raises(ValueError, match=r"file 1.*trim=True"):
        SJ.standard_jpeg_transform_many([ok, small], ["none", "rot270"])
    with pytest.raises(ValueError, match=r"file 0.*trim=True"):
        SJ.transform_prefix(small, "flip_h")
    small420 = _pil(_noise(3, 9), quality=50, subsampling="4:2:0")            # one 16-wide MCU: the trim leaves nothing
    with pytest.raises(ValueError, match=r"file 1.*leaves nothing"):
        SJ.standard_jpeg_transform_many([ok, small420], "flip_h", trim=True)
    wide = _pil(_noise(32, 48), quality=50, subsampling="4:2:2")
    for name in R.TRANSPOSING:
        with pytest.raises(NotImplementedError, match=r"file 1.*4:4:0"):
            SJ.standard_jpeg_transform_many([ok, wide], name)
        with pytest.raises(NotImplementedError, match=r"file 0.*4:4:0"):
            SJ.transform_prefix(wide, name)
    grey = _pil(Image.fromarray(_noise(16, 16)).convert("L"), quality=50)
    with pytest.raises(NotImplementedError, match="file 1"):
        SJ.standard_jpeg_transform_many([ok, grey], "flip_h")
    with pytest.raises(ValueError, match="file 1"):
        SJ.standard_jpeg_transform_many([ok, ok[:40]], "exif")
    # "exif" picks the refused transform from the file
    e = Image.Exif()
    e[0x0112] = 6
    with pytest.raises(NotImplementedError, match=r"file 1.*rot90.*4:4:0"):
        SJ.standard_jpeg_transform_many([ok, _pil(_noise(32, 48), quality=50, subsampling="4:2:2", exif=e.tobytes())], "exif")
    e[0x0112] = 2
    with pytest.raises(ValueError, match=r"file 0.*flip_h.*trim=True"):
        SJ.standard_jpeg_transform_many([_pil(_noise(3, 9), quality=50, subsampling="4:4:4", exif=e.tobytes())], "exif")


def test_abi(SJ, lib):
    import adaptive_edge_aware_jpeg_amd as A
    for name in ("aej_jfif_transform_geometry_host", "aej_jfif_transform_coefs_host", "aej_jfif_transform_headers_host",
                 "aej_jfif_transform_workspace_bytes", "aej_jfif_transform_batch"):
        assert getattr(lib, name) is not None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "aej.h")) as f:
        header = f.read()
    for name in ("aej_jfif_transform_geometry_host", "aej_jfif_transform_coefs_host", "aej_jfif_transform_headers_host",
                 "aej_jfif_transform_workspace_bytes", "aej_jfif_transform_batch"):
        assert f"{name}(" in header
    assert A.standard_jpeg_transform_many is SJ.standard_jpeg_transform_many and "standard_jpeg_transform_many" in A.__all__
    assert SJ.TRANSFORMS == R.NAMES
    buf = (ctypes.c_uint8 * 16)()
    assert lib.aej_jfif_transform_headers_host(None, None, None, 0, 1, 0, ctypes.addressof(buf), 16) == -1
    assert lib.aej_jfif_transform_geometry_host(8, 8, 1, 1, 8, 0, None) == -1
    assert lib.aej_jfif_transform_geometry_host(8, 8, 1, 2, 0, 0, None) == -1
    assert lib.aej_jfif_transform_geometry_host(8, 8, 1, 1, 1, 2, None) == -1
    assert lib.aej_jfif_transform_geometry_host(8, 8, 1, 1, 1, 0, None) == 0
