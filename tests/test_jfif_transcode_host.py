"""CPU: the host side of standard_jpeg_transcode_many -- the markers SOI .. SOF the transcoder writes (aej_jfif_transcode_headers_host)
against Pillow's own files, the refusals, the metadata splice and the new ABI symbols.  No device is touched."""
import ctypes
import io
import struct

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_transcode_helpers as H  # noqa: E402

QUALITIES = (1, 10, 50, 75, 95, 100)
LAYOUTS = ("4:4:4", "4:2:2", "4:2:0")


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


def _noise(H, W, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _pil(x, **opts):
    from PIL import Image, ImageFile
    img = x if isinstance(x, Image.Image) else Image.fromarray(x)
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * img.size[0] * img.size[1] + (1 << 17))
    try:
        img.save(buf, "JPEG", **opts)
    finally:
        ImageFile.MAXBLOCK = old
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


def _own_prefix(data):
    """the file's own bytes from SOI to the end of its SOF segment"""
    n = 2
    for m, seg in _segments(data):
        n += len(seg)
        if m in (0xC0, 0xC2):
            return data[:n]
    raise AssertionError("no SOF")


QT = ([(3 * i) % 254 + 1 for i in range(64)], [(7 * i + 5) % 255 + 1 for i in range(64)])
CASES = [dict(quality=q, subsampling=s) for q in QUALITIES for s in LAYOUTS] + [
    dict(qtables=[list(QT[0]), list(QT[1])], subsampling="4:2:2"), dict(quality=30, subsampling="4:2:0", dpi=(300, 72))]


@pytest.mark.parametrize("opts", CASES, ids=lambda o: "-".join(f"{k}{v if not isinstance(v, list) else ''}" for k, v in o.items()))
def test_prefix_equals_pillows_own_bytes(SJ, opts):
    x = _noise(19, 35)
    plain, opt, prog = _pil(x, **opts), _pil(x, optimize=True, **opts), _pil(x, progressive=True, **opts)
    want = _own_prefix(plain)
    assert _own_prefix(opt) == want
    want_prog = _own_prefix(prog)
    assert want_prog == want.replace(b"\xff\xc0\x00\x11", b"\xff\xc2\x00\x11")
    for src in (plain, opt, prog):
        assert SJ.transcode_prefix(src, progressive=False) == want
        assert SJ.transcode_prefix(src, progressive=True) == want_prog


def test_single_shared_table_gives_one_dqt(SJ):
    f = _pil(_noise(8, 8), quality=60, subsampling="4:4:4")
    segs = _segments(f)
    dqt = [s for m, s in segs if m == 0xDB]
    assert len(dqt) == 2
    sof = next(s for m, s in segs if m == 0xC0)
    sof1 = bytearray(sof)
    sof1[12], sof1[15], sof1[18] = 0, 0, 0               # every component selects table 0
    edited = f.replace(dqt[1], b"").replace(sof, bytes(sof1))
    got = SJ.transcode_prefix(edited)
    assert [m for m, _ in _segments(got + b"\xff\xda")] == [0xE0, 0xDB, 0xC0]
    assert got == edited[:len(got)]
    assert got[-19:] == bytes(sof1)


def test_prefix_keeps_foreign_component_ids(SJ):
    x = _noise(37, 53)
    for ids in ((0, 1, 2), (ord("Y"), ord("C"), ord("c"))):
        for kind in (dict(), dict(progressive=True)):
            f = _pil(x, quality=75, subsampling="4:2:0", **kind)
            g = H.with_ids(f, ids)
            assert g != f and H.ids_of(g)[0] == list(ids) and all(set(sc) <= set(ids) for sc in H.ids_of(g)[1])
            for prog in (False, True):
                got = SJ.transcode_prefix(g, progressive=prog)
                assert got == H.with_ids(SJ.transcode_prefix(f, progressive=prog) + b"\xff\xd9", ids)[:-2]
                assert [got[-9], got[-6], got[-3]] == list(ids)


def test_refusals(SJ):
    from PIL import Image
    ok = _pil(_noise(9, 9), quality=50)
    grey = _pil(Image.fromarray(_noise(9, 9)).convert("L"), quality=50)
    cmyk = _pil(Image.fromarray(_noise(9, 9)).convert("CMYK"), quality=50)
    dqt = next(s for m, s in _segments(ok) if m == 0xDB)
    wide = b"\xff\xdb" + struct.pack(">H", 2 + 1 + 128) + bytes([0x10 | dqt[4]]) + b"".join(struct.pack(">H", v) for v in dqt[5:])
    sixteen = ok.replace(dqt, wide)
    assert np.asarray(Image.open(io.BytesIO(sixteen))).shape == (9, 9, 3)      # still a file Pillow reads
    for bad in (grey, sixteen, cmyk):
        with pytest.raises(NotImplementedError, match="file 1"):
            SJ.standard_jpeg_transcode_many([ok, bad])
        with pytest.raises(NotImplementedError, match="file 0"):
            SJ.transcode_prefix(bad)
    with pytest.raises(ValueError):
        SJ.standard_jpeg_transcode_many([])
    with pytest.raises(ValueError, match="file 1"):
        SJ.standard_jpeg_transcode_many([ok, ok[:40]])
    for kw in (dict(progressive=1), dict(progressive="yes"), dict(keep_metadata=0), dict(keep_metadata=None)):
        with pytest.raises(TypeError):
            SJ.standard_jpeg_transcode_many([ok], **kw)


def test_metadata_splice(SJ):
    from PIL import Image
    exif = Image.Exif()
    exif[0x010E] = "a description"
    icc = bytes(range(256)) * 273 + bytes(112)             # 70 000 bytes: two APP2 segments
    assert len(icc) == 70000
    f = _pil(_noise(16, 16), quality=75, exif=exif.tobytes(), icc_profile=icc, comment=b"hello")
    assert [m for m, _ in _segments(f)][:5] == [0xE0, 0xE1, 0xE2, 0xE2, 0xFE]
    meta = SJ.metadata_segments(f)
    spliced = SJ.splice_metadata(SJ.transcode_prefix(f), meta)
    assert [m for m, _ in _segments(spliced + b"\xff\xda")] == [0xE0, 0xE1, 0xE2, 0xE2, 0xFE, 0xDB, 0xDB, 0xC0]
    assert spliced == _own_prefix(f)
    info = Image.open(io.BytesIO(spliced + f[len(spliced):])).info
    assert info["icc_profile"] == icc and info["comment"] == b"hello" and info["exif"] == exif.tobytes()
    # an Adobe APP14 and a JFXX APP0 in the source are not carried over
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    jfxx = b"\xff\xe0\x00\x08JFXX\x00\x13"
    g = f[:20] + jfxx + adobe + f[20:]
    assert SJ.metadata_segments(g) == meta
    assert SJ.splice_metadata(SJ.transcode_prefix(f), b"") == SJ.transcode_prefix(f)


def test_abi(SJ):
    from adaptive_edge_aware_jpeg_amd._lib import JPEGDEC_STATUS, load_library
    lib = load_library()
    for name in ("aej_jfif_transcode_headers_host", "aej_jfif_transcode_workspace_bytes", "aej_jfif_transcode_batch"):
        assert getattr(lib, name) is not None
    assert lib.aej_abi_version() == 3
    assert len(JPEGDEC_STATUS) == 7 and "out of range" in JPEGDEC_STATUS[6] and JPEGDEC_STATUS[5].startswith("restart marker")
    import adaptive_edge_aware_jpeg_amd as A
    assert A.standard_jpeg_transcode_many is SJ.standard_jpeg_transcode_many
    buf = (ctypes.c_uint8 * 16)()
    assert lib.aej_jfif_transcode_headers_host(None, None, None, 0, ctypes.addressof(buf), 16) == -1
