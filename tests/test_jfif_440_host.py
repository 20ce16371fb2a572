"""CPU: the host side of layout_440= -- 4:4:0 files (luma 1 x 2 over 1 x 1 chroma) in the two parsers, and the geometry, coefficient
mapping and markers of the transforms that make them from 4:2:2 files and 4:2:2 files from them.  The 4:4:0 sources are Pillow 4:2:2
files with a patched frame header (jfif_440_reference.py); the mapping's oracle is the NumPy restatement of the transform tests, which
is written in (hs, vs).  No device is touched."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_440_reference as F  # noqa: E402
import jfif_transform_reference as R  # noqa: E402
import test_jfif_transform_host as TH  # noqa: E402  (its sizes and its marker walk)

LAYOUTS = {"4:2:2": (2, 1), "4:4:0": (1, 2)}


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


@pytest.fixture(scope="module")
def patched():
    """{(H, W, option): the 4:4:0 file}, H x W the source's size"""
    return {(H, W, o): F.make_440(H, W, o) for H, W in F.SIZES for o in F.OPTIONS}


def test_patcher_files_are_440_for_pillow(patched):
    for (H, W, o), f in patched.items():
        px, layer = F.pil_decode(f)
        assert layer == (1, 1, 2, 0) and px.shape == (W, H, 3), (H, W, o, layer)
        assert F.frame(f)[:2] == (W, H) and F.frame(f)[2][0][1:3] == (1, 2)
        for s in (2, 4, 8):
            assert F.pil_decode(f, s)[1] == (1, 1, 2, 0)


def test_parsers_with_and_without_the_flag(SJ, patched):
    for (H, W, o), f in patched.items():
        prog = "progressive" in o
        if prog:
            with pytest.raises(NotImplementedError, match=r"file 3: sampling factors 1x2,1x1,1x1"):
                SJ.parse_scans(f, 3)
            frame, scans = SJ.parse_scans(f, 3, layout_440=True)
            assert len(scans) == frame.n_scans == 10
        else:
            with pytest.raises(NotImplementedError, match=r"file 3: sampling factors 1x2,1x1,1x1"):
                SJ.parse_header(f, 3)
            frame = SJ.parse_header(f, 3, layout_440=True)
        assert (frame.hs, frame.vs, frame.height, frame.width, frame.ncomp) == (1, 2, W, H, 3), (H, W, o)
        assert (frame.mcux, frame.mcuy, frame.blocks_per_mcu) == (-(-H // 8), -(-W // 16), 4)
    # the flag changes nothing for the other layouts, and nothing else is let through with it
    x = F.noise(24, 40)
    for ss in ("4:4:4", "4:2:2", "4:2:0"):
        f = TH._pil(x, quality=60, subsampling=ss)
        assert bytes(SJ.parse_header(f)) == bytes(SJ.parse_header(f, layout_440=True))
    f = bytearray(F.pil_422(x))
    f[F.sof_at(f) + 11] = 0x14                                    # 1 x 4
    with pytest.raises(NotImplementedError, match="sampling factors 1x4"):
        SJ.parse_header(bytes(f), layout_440=True)
    f[F.sof_at(f) + 11], f[F.sof_at(f) + 14] = 0x12, 0x12         # chroma not 1 x 1
    with pytest.raises(NotImplementedError, match="sampling factors 1x2,1x2"):
        SJ.parse_header(bytes(f), layout_440=True)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="layout_440"):
            SJ.parse_header(bytes(f), layout_440=bad)
        with pytest.raises(TypeError, match="layout_440"):
            SJ.parse_scans(bytes(f), layout_440=bad)


def _geometry(lib, H, W, hs, vs, code, trim, flag=1):
    out = (ctypes.c_int32 * 4)()
    return lib.aej_jfif_transform_geometry_host_440(H, W, hs, vs, code, int(trim), flag, ctypes.addressof(out)), tuple(out)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", R.NAMES)
def test_geometry_and_coefficients_equal_numpy_restatement(lib, name, layout):
    hs, vs = LAYOUTS[layout]
    code = R.NAMES.index(name)
    ran = 0
    for H, W in TH.SIZES:
        for trim in (False, True):
            rc, geo = _geometry(lib, H, W, hs, vs, code, trim)
            query = lib.aej_jfif_transform_coefs_host_440(H, W, hs, vs, code, int(trim), 1, None, 0, None, 0)
            try:
                want_geo = R.out_geometry(H, W, hs, vs, name, trim)
            except ValueError as e:
                assert rc == (2 if str(e) == "nothing left" else 1) == query, (H, W, trim, rc)
                continue
            assert rc == 0 and geo == want_geo, (H, W, trim, rc, geo, want_geo)
            oH, oW, ohs, ovs = want_geo
            assert (ohs, ovs) == ((vs, hs) if name in R.TRANSPOSING else (hs, vs))
            n_src = 4 * -(-W // (8 * hs)) * -(-H // (8 * vs))
            n_out = 4 * -(-oW // (8 * ohs)) * -(-oH // (8 * ovs))
            assert query == n_out
            src = np.random.default_rng(H * 100 + W).integers(-32767, 32768, (n_src, 64)).astype(np.int16)
            dst = np.full((n_out + 1, 64), 12345, np.int16)      # one block of canary
            got = lib.aej_jfif_transform_coefs_host_440(H, W, hs, vs, code, int(trim), 1, src.ctypes.data, n_src, dst.ctypes.data, n_out)
            assert got == n_out and (dst[n_out] == 12345).all()
            natural = np.zeros((n_out, 64), np.int64)
            natural[:, R.ZZ] = dst[:n_out]                        # the entry writes the coders' zigzag order
            if name == "none":                                    # the transcode: every block carried as it is, the dummies too
                assert np.array_equal(natural, src.astype(np.int64))
            else:                                                 # every output block, the dummies by their rule
                real, _ = R.coefficients(R.to_planes(src.astype(np.int64), H, W, hs, vs), H, W, hs, vs, name, trim)
                R.check_padded(R.to_planes(natural, oH, oW, ohs, ovs), real, oH, oW, ohs, ovs, f"{name} {layout} {H}x{W} trim={trim}")
            assert lib.aej_jfif_transform_coefs_host_440(H, W, hs, vs, code, int(trim), 1, src.ctypes.data, n_src + 1, dst.ctypes.data, n_out) == -1
            assert lib.aej_jfif_transform_coefs_host_440(H, W, hs, vs, code, int(trim), 1, src.ctypes.data, n_src, dst.ctypes.data, n_out - 1) == -4
            ran += 1
    assert ran >= 6


def test_entries_without_the_permission_answer_as_before(lib):
    out = (ctypes.c_int32 * 4)()
    for H, W in TH.SIZES:
        for code, name in enumerate(R.NAMES):
            for hs, vs in ((1, 1), (2, 1), (2, 2), (1, 2)):
                old = lib.aej_jfif_transform_geometry_host(H, W, hs, vs, code, 1, ctypes.addressof(out))
                a = tuple(out)
                assert lib.aej_jfif_transform_geometry_host_440(H, W, hs, vs, code, 1, 0, ctypes.addressof(out)) == old and tuple(out) == a
                assert lib.aej_jfif_transform_coefs_host_440(H, W, hs, vs, code, 1, 0, None, 0, None, 0) == \
                    lib.aej_jfif_transform_coefs_host(H, W, hs, vs, code, 1, None, 0, None, 0)
                if (hs, vs) == (1, 2):
                    assert old == -1                              # AEJ_ERR_ARG, as test_jfif_transform_host pins it
                elif (hs, vs) == (2, 1) and name in R.TRANSPOSING:
                    assert old == -5
                if hs >= vs and not (hs != vs and name in R.TRANSPOSING):      # the permission changes no answer that was not a refusal
                    assert lib.aej_jfif_transform_geometry_host_440(H, W, hs, vs, code, 1, 1, ctypes.addressof(out)) == old
                    assert old != 0 or tuple(out) == a
    assert lib.aej_jfif_transform_geometry_host_440(8, 8, 1, 2, 0, 0, 2, None) == -1
    assert lib.aej_jfif_transform_geometry_host_440(8, 8, 1, 3, 0, 0, 1, None) == -1
    assert lib.aej_jfif_transform_geometry_host_440(8, 8, 1, 2, 0, 0, 1, None) == 0


@pytest.mark.parametrize("prog", (False, True))
def test_header_bytes_of_a_transposed_422_file(SJ, prog):
    src = F.pil_422(F.noise(32, 48), 60, qtables=[list(TH.QT[0]), list(TH.QT[1])])
    plain = SJ.transcode_prefix(src, progressive=prog)
    assert SJ.transcode_prefix(src, progressive=prog, layout_440=True) == plain
    assert SJ.transform_prefix(src, "none", progressive=prog, layout_440=True) == plain
    assert SJ.transform_prefix(src, "flip_h", progressive=prog, layout_440=True) == SJ.transform_prefix(src, "flip_h", progressive=prog)
    for name in R.TRANSPOSING:
        got = SJ.transform_prefix(src, name, progressive=prog, layout_440=True)
        h, w, comps = TH._frame(got + b"\xff\xda")
        assert (h, w) == (48, 32) and [c[1:3] for c in comps] == [(1, 2), (1, 1), (1, 1)], name
        assert got[-19] == 0xFF and got[-18] == (0xC2 if prog else 0xC0) and got[-8] == 0x12      # the frame header ends the prefix
        assert got[:20] == plain[:20] and len(got) == len(plain)
        dqt = [s for m, s in TH._segments(got + b"\xff\xda") if m == 0xDB]
        sdqt = [s for m, s in TH._segments(plain + b"\xff\xda") if m == 0xDB]
        assert len(dqt) == len(sdqt) == 2
        for k, (a, b) in enumerate(zip(dqt, sdqt)):
            nat_a, nat_b = np.zeros(64, int), np.zeros(64, int)
            nat_a[R.ZZ], nat_b[R.ZZ] = list(a[5:]), list(b[5:])
            assert a[:5] == b[:5] and np.array_equal(nat_a.reshape(8, 8), nat_b.reshape(8, 8).T) and not np.array_equal(nat_a, nat_b), (name, k)
        # and back: the prefix of a 4:4:0 source under the same transform is a 4:2:2 frame
        p440 = F.patch_440(src)                                    # 48 x 32 (H x W), luma 1 x 2
        back = SJ.transform_prefix(p440, name, progressive=prog, layout_440=True)
        h, w, comps = TH._frame(back + b"\xff\xda")
        assert (h, w) == (32, 48) and comps[0][1:3] == (2, 1) and back[-8] == 0x21
        with pytest.raises(NotImplementedError, match=r"file 0: sampling factors 1x2"):
            SJ.transform_prefix(p440, name, progressive=prog)
        with pytest.raises(NotImplementedError, match=r"file 0.*4:4:0"):
            SJ.transform_prefix(src, name, progressive=prog)


def test_refusals_before_any_device_work(SJ, monkeypatch):
    from PIL import Image
    from adaptive_edge_aware_jpeg_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a refusal reached the device")
    monkeypatch.setattr(_lib, "get_context", no_device)
    monkeypatch.setattr(SJ, "get_context", no_device)
    ok = TH._pil(F.noise(16, 16), quality=50, subsampling="4:2:0")
    wide = F.pil_422(F.noise(32, 48))
    f440 = F.patch_440(wide)
    e = Image.Exif()
    e[0x0112] = 6
    turned = F.pil_422(F.noise(32, 48), exif=e.tobytes())
    # without the keyword: the old words
    for call in (lambda: SJ.standard_jpeg_decode_many([ok, f440]), lambda: SJ.standard_jpeg_decode_many([ok, f440], progressive=True, scale=2),
                 lambda: SJ.standard_jpeg_thumbnail_many([ok, f440], (8, 8)), lambda: SJ.standard_jpeg_thumbnail_jpeg_many([ok, f440], (8, 8)),
                 lambda: SJ.standard_jpeg_transcode_many([ok, f440]), lambda: SJ.standard_jpeg_transform_many([ok, f440], "flip_h"),
                 lambda: SJ.transcode_prefix(f440, index=1)):
        with pytest.raises(NotImplementedError, match=r"file 1: sampling factors 1x2,1x1,1x1"):
            call()
    for name in R.TRANSPOSING:
        with pytest.raises(NotImplementedError, match=r"file 1.*4:4:0"):
            SJ.standard_jpeg_transform_many([ok, wide], name)
    with pytest.raises(NotImplementedError, match=r"file 1.*rot90.*4:4:0"):
        SJ.standard_jpeg_transform_many([ok, turned], "exif")
    # a value that is not a bool
    for bad in (1, 0, None, "yes"):
        for call in (lambda: SJ.standard_jpeg_decode_many([ok], layout_440=bad), lambda: SJ.standard_jpeg_thumbnail_many([ok], (8, 8), layout_440=bad),
                     lambda: SJ.standard_jpeg_thumbnail_jpeg_many([ok], (8, 8), layout_440=bad),
                     lambda: SJ.standard_jpeg_transcode_many([ok], layout_440=bad), lambda: SJ.standard_jpeg_transform_many([ok], "flip_h", layout_440=bad),
                     lambda: SJ.transcode_prefix(ok, layout_440=bad), lambda: SJ.transform_prefix(ok, "flip_h", layout_440=bad)):
            with pytest.raises(TypeError, match="layout_440"):
                call()
    # with it: the MCU rules hold with the new layout's 8 x 16 MCUs, and the encoders still have no 4:4:0
    odd = F.make_440(9, 17)                                       # 17 x 9 (H x W): partial MCUs on both axes
    with pytest.raises(ValueError, match=r"file 1.*flip_h.*8 x 16 MCUs.*trim=True"):
        SJ.standard_jpeg_transform_many([ok, odd], "flip_h", layout_440=True)
    with pytest.raises(ValueError, match=r"file 0.*leaves nothing"):
        SJ.standard_jpeg_transform_many([F.make_440(1, 1)], "rot180", trim=True, layout_440=True)
    with pytest.raises(ValueError):
        SJ.standard_jpeg_encode_many([F.noise(8, 8)], subsampling="4:4:0")


def test_abi(SJ, lib):
    names = ("aej_jpegdec_parse_host_440", "aej_jpegprog_parse_host_440", "aej_jfif_transform_geometry_host_440", "aej_jfif_transform_coefs_host_440",
             "aej_jfif_transform_headers_host_440", "aej_jfif_transform_workspace_bytes_440", "aej_jfif_transform_batch_440")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "aej.h")) as f:
        header = f.read()
    for name in names:
        assert getattr(lib, name) is not None and f"{name}(" in header
    assert lib.aej_abi_version() == 3
    f = F.make_440(24, 40)
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc
    buf, d, msg = (ctypes.c_uint8 * len(f)).from_buffer_copy(f), JpegDecDesc(), ctypes.create_string_buffer(256)
    head = (ctypes.addressof(buf), len(f), ctypes.addressof(d), ctypes.addressof(msg), 256)
    assert lib.aej_jpegdec_parse_host(*head) == -5 and msg.value.startswith(b"sampling factors 1x2")
    assert lib.aej_jpegdec_parse_host_440(*head, 0) == -5 and msg.value.startswith(b"sampling factors 1x2")
    assert lib.aej_jpegdec_parse_host_440(*head, 2) == -1
    assert lib.aej_jpegdec_parse_host_440(*head, 1) == 0 and (d.hs, d.vs) == (1, 2)
    out = (ctypes.c_uint8 * 512)()
    assert lib.aej_jfif_transform_headers_host(ctypes.addressof(d), None, None, 0, 0, 0, ctypes.addressof(out), 512) == -5
    assert lib.aej_jfif_transcode_headers_host(ctypes.addressof(d), None, None, 0, ctypes.addressof(out), 512) == -5
    assert lib.aej_jfif_transform_headers_host_440(ctypes.addressof(d), None, None, 0, 0, 0, 0, ctypes.addressof(out), 512) == -5
    n = lib.aej_jfif_transform_headers_host_440(ctypes.addressof(d), None, None, 0, 0, 0, 1, ctypes.addressof(out), 512)
    assert n > 0 and bytes(out[:n]) == SJ.transcode_prefix(f, layout_440=True)
    assert struct.unpack(">HH", bytes(out[n - 14:n - 10])) == (40, 24) and out[n - 8] == 0x12
