"""CPU: the host side of grey (one-component) JPEG in the ragged encoder, the transcoder and the transforms -- no GPU needed.
aej_jfif_many_coefs_grey_host (the code k_jm_coefs runs for a grey image) against a NumPy restatement and against the coefficients of
Pillow's own files; aej_jfif_transform_coefs_grey_host (the code k_jt_transform runs) against a NumPy block and coefficient mapping;
the header bytes against the prefixes of the fixtures under tests/golden/jfif_grey (Pillow's files of mode-"L" images); Pillow's
progressive grey file put together on the host from the six scans the coder is given; the argument checks of the new keywords, and the
refusals that stay when they are not passed."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_reference as R  # noqa: E402
import jfif_transform_reference as T  # noqa: E402

from conftest import GOLDEN  # noqa: E402

FIXTURES = os.path.join(GOLDEN, "jfif_grey")
SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (1, 40), (40, 1), (37, 53), (255, 257)]      # (H, W): the issue's
AEJ_ERR_ARG, AEJ_ERR_CAPACITY = -1, -4
GREY_SCANS = [(0, 0, 0, 1), (1, 5, 0, 2), (6, 63, 0, 2), (1, 63, 2, 1), (0, 0, 1, 0), (1, 63, 1, 0)]      # (Ss, Se, Ah, Al): jpeg_simple_progression, one component


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


@pytest.fixture(scope="module")
def cases():
    """[(name, source pixels, quality)] of the fixtures"""
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        meta = json.load(f)
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    out = [(c["name"], px[c["name"] + "_src"], c["quality"]) for c in meta["cases"]]
    assert [x.shape for _, x, _ in out] == SIZES and {q for _, _, q in out} == {1, 10, 50, 75, 95, 100}
    return out


def _file(name):
    with open(os.path.join(FIXTURES, name + ".jpg"), "rb") as f:
        return f.read()


def _segments(data):
    """[(marker, whole segment)] from SOI to the first SOS, that one included"""
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        n = int.from_bytes(data[i + 2:i + 4], "big")
        out.append((data[i + 1], data[i:i + 2 + n]))
        if data[i + 1] == 0xDA:
            return out
        i += 2 + n


# ---- the encoder's host entry -------------------------------------------------------------------------------------------------------------
def _model(x, q):
    """the luma path of jfif_reference without colour conversion: edge replication, level shift, islow FDCT, the luma quantiser;
    -> [block][64] zigzag, the blocks in raster order"""
    H, W = x.shape
    by, bx = -(-H // 8), -(-W // 8)
    Y = np.pad(x.astype(np.int64), ((0, 8 * by - H), (0, 8 * bx - W)), mode="edge")
    c = R.quantise(R.fdct(R._blocks(Y)), R.quant_tables(q)[0])
    return c.reshape(by * bx, 64)[:, R.ZIGZAG]


def _coefs(lib, x, q):
    h, w = x.shape
    n = lib.aej_jfif_many_coefs_grey_host(w, h, q, None, None, 0)
    assert n == (-(-h // 8)) * (-(-w // 8))                          # no dummy blocks
    out = np.full((n + 1, 64), 12345, np.int16)                      # one guard block behind
    x = np.ascontiguousarray(x)
    assert lib.aej_jfif_many_coefs_grey_host(w, h, q, x.ctypes.data, out.ctypes.data, n) == n
    assert (out[n] == 12345).all()
    return out[:n]


def _file_coefficients(SJ, lib, data):
    """the quantised coefficients of a progressive file, [block][64] natural order, by the library's host-stepped decoder"""
    from adaptive_edge_aware_jpeg_amd import _lib
    frame, scans = SJ.parse_scans(data)
    arr = (_lib.JpegProgScan * len(scans))(*scans)
    nb = frame.mcux * frame.mcuy * frame.blocks_per_mcu
    out = np.zeros((nb, 64), np.int16)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    assert lib.aej_test_jpegprog_coefs_host(ctypes.addressof(frame), ctypes.addressof(arr), ctypes.addressof(buf), len(data), 1 << 30,
                                            out.ctypes.data, nb) == 0
    return out


def test_coefs_host_equal_the_numpy_model_and_pillows_files(SJ, lib, cases):
    for name, x, q in cases:
        got = _coefs(lib, x, q)
        assert np.array_equal(got, _model(x, q)), name
        assert np.array_equal(got, _file_coefficients(SJ, lib, _file(name + "_prog"))[:, R.ZIGZAG]), name
    x = cases[7][1]                                                  # 37 x 53: every quality of the issue
    for q in (1, 10, 50, 75, 95, 100):
        assert np.array_equal(_coefs(lib, x, q), _model(x, q)), q


def test_coefs_host_refusals(lib):
    x, out = np.zeros((8, 8), np.uint8), np.zeros((1, 64), np.int16)
    assert lib.aej_jfif_many_coefs_grey_host(8, 8, 75, x.ctypes.data, out.ctypes.data, 1) == 1
    assert lib.aej_jfif_many_coefs_grey_host(9, 8, 75, x.ctypes.data, out.ctypes.data, 1) == AEJ_ERR_CAPACITY
    for args in ((0, 8, 75), (8, 65536, 75), (8, 8, 0), (8, 8, 101)):
        assert lib.aej_jfif_many_coefs_grey_host(*args, x.ctypes.data, out.ctypes.data, 1) == AEJ_ERR_ARG, args
    assert lib.aej_jfif_many_coefs_grey_host(8, 8, 75, x.ctypes.data, None, 1) == AEJ_ERR_ARG
    assert lib.aej_jfif_many_coefs_grey_host(65535, 65535, 75, None, None, 0) == 8192 * 8192


# ---- the transform's host entry -----------------------------------------------------------------------------------------------------------
def _transformed(c, H, W, name, trim):
    """c: [block rows][block columns][64] natural order of a one-component file -> the output's blocks the same way; ValueError as
    jfif_transform_reference.trimmed_source (hs = vs = 1: a mirrored axis is a multiple of 8)"""
    h, w = T.trimmed_source(H, W, 1, 1, name, trim)
    c = c[:-(-h // 8), :-(-w // 8)]
    for s in T.STEPS[name]:
        c = T._step(c, s)
    return c


@pytest.mark.parametrize("H,W", [(16, 24), (37, 53), (8, 8)])
@pytest.mark.parametrize("name", T.NAMES)
def test_transform_coefs_host_equal_the_numpy_mapping(lib, name, H, W):
    code = T.NAMES.index(name)
    rows, cols = -(-H // 8), -(-W // 8)
    src = np.random.default_rng(100 * H + W).integers(-1023, 1024, (rows, cols, 64)).astype(np.int16)
    flat = np.ascontiguousarray(src.reshape(-1, 64))
    for trim in (False, True):
        try:
            want = _transformed(src.astype(np.int64), H, W, name, trim)
        except ValueError:
            assert not trim or min(H, W) < 8
            assert lib.aej_jfif_transform_coefs_grey_host(H, W, code, int(trim), None, 0, None, 0) == AEJ_ERR_ARG
            out4 = (ctypes.c_int32 * 4)()
            assert lib.aej_jfif_transform_geometry_host(H, W, 1, 1, code, int(trim), ctypes.addressof(out4)) in (1, 2)      # the reason
            continue
        n_out = want.shape[0] * want.shape[1]
        assert lib.aej_jfif_transform_coefs_grey_host(H, W, code, int(trim), None, 0, None, 0) == n_out
        dst = np.full((n_out + 1, 64), 12345, np.int16)
        assert lib.aej_jfif_transform_coefs_grey_host(H, W, code, int(trim), flat.ctypes.data, rows * cols, dst.ctypes.data, n_out) == n_out
        assert (dst[n_out] == 12345).all()
        assert np.array_equal(dst[:n_out], want.reshape(-1, 64)[:, T.ZZ]), (name, H, W, trim)       # zigzag inside a block, raster order
        assert lib.aej_jfif_transform_coefs_grey_host(H, W, code, int(trim), flat.ctypes.data, rows * cols + 1, dst.ctypes.data, n_out) == AEJ_ERR_ARG
        assert lib.aej_jfif_transform_coefs_grey_host(H, W, code, int(trim), flat.ctypes.data, rows * cols, dst.ctypes.data, n_out - 1) == AEJ_ERR_CAPACITY
    # what the mapping says about this size: every transform of an exact size, and for 37 x 53 the mirrors only with the trim
    perfect = (H % 8 == 0 or name not in T.NEEDS_H) and (W % 8 == 0 or name not in T.NEEDS_W)
    assert (lib.aej_jfif_transform_coefs_grey_host(H, W, code, 0, None, 0, None, 0) > 0) == perfect


def test_transposing_transforms_need_no_square_sampling(lib):
    """a one-component file is 1 x 1 whatever its frame header says: all eight codes fit a size that is a multiple of 8"""
    for code in range(8):
        assert lib.aej_jfif_transform_coefs_grey_host(16, 24, code, 0, None, 0, None, 0) == 6
    assert lib.aej_jfif_transform_coefs_grey_host(16, 24, 8, 0, None, 0, None, 0) == AEJ_ERR_ARG


# ---- headers --------------------------------------------------------------------------------------------------------------------------------
def test_encoder_headers_equal_the_fixture_prefixes(SJ, cases):
    for name, x, q in cases:
        want = _file(name)
        got = SJ.headers(q, x.shape[0], x.shape[1], mode="L")
        assert want.startswith(got) and want[len(got) - 10:len(got) - 8] == b"\xff\xda", name
        assert [m for m, _ in _segments(got)] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDA]      # one DQT, two DHT
        segs = dict(_segments(got))
        assert segs[0xC0][4:] == bytes([8]) + x.shape[0].to_bytes(2, "big") + x.shape[1].to_bytes(2, "big") + bytes([1, 1, 0x11, 0])
        assert segs[0xDA][4:] == bytes([1, 1, 0, 0, 63, 0])
        assert SJ.headers(q, x.shape[0], x.shape[1], "4:4:4", mode="L") == got           # subsampling does not bear on a grey file
    with pytest.raises(ValueError):
        SJ.headers(75, 8, 8, mode="auto")
    with pytest.raises(ValueError):
        SJ.headers(0, 8, 8, mode="L")


def test_transcoder_prefix_equals_the_fixture_prefixes(SJ, cases):
    for name, x, q in cases:
        for src in ("", "_opt", "_prog"):
            data = _file(name + src)
            for prog, want in ((False, _file(name + "_opt")), (True, _file(name + "_prog"))):
                got = SJ.transcode_prefix(data, progressive=prog, grey=True)
                assert want.startswith(got) and got[-13:-11] == (b"\xff\xc2" if prog else b"\xff\xc0"), (name, src, prog)
                assert want[len(got):len(got) + 2] == b"\xff\xc4"
    data = _file("ramp_37x53_q100")
    sof = next(s for m, s in _segments(data) if m == 0xC0)
    dqt = next(s for m, s in _segments(data) if m == 0xDB)
    t = SJ.transform_prefix(data, "transpose", grey=True)
    tq = np.frombuffer(dqt[5:], np.uint8)
    nat = np.zeros(64, np.uint8)
    nat[R.ZIGZAG] = tq
    assert t[-13:] == sof[:5] + (53).to_bytes(2, "big") + (37).to_bytes(2, "big") + sof[9:]
    assert t[-13 - 69:-13] == dqt[:5] + nat.reshape(8, 8).T.reshape(64)[R.ZIGZAG].tobytes()
    with pytest.raises(ValueError, match="file 0"):
        SJ.transform_prefix(data, "flip_h", grey=True)               # 53 is no multiple of 8
    assert SJ.transform_prefix(data, "flip_h", trim=True, grey=True)[-13:] == sof[:7] + (48).to_bytes(2, "big") + sof[9:]
    # the frame header's sampling byte means nothing for one component: 2 x 2 gives the same prefix, 1 x 1 in it
    at = data.index(sof) + 11
    assert data[at] == 0x11
    assert SJ.transcode_prefix(data[:at] + b"\x22" + data[at + 1:], grey=True) == SJ.transcode_prefix(data, grey=True)
    # a foreign component id and table selector: the id stays, the table becomes table 0
    sel = data[:at - 1] + bytes([7, 0x11, 1]) + data[at + 2:]
    sel = sel.replace(dqt, dqt[:4] + b"\x01" + dqt[5:]).replace(b"\xff\xda\x00\x08\x01\x01", b"\xff\xda\x00\x08\x01\x07")
    assert SJ.transcode_prefix(sel, grey=True) == SJ.transcode_prefix(data, grey=True)[:-3] + bytes([7, 0x11, 0])


# ---- Pillow's progressive grey file, assembled on the host from the coder's six scans ----------------------------------------------------
def test_six_scans_assemble_pillows_progressive_file(SJ, lib, cases):
    for name, x, q in cases[:8]:
        coef = np.ascontiguousarray(_coefs(lib, x, q))
        n = coef.shape[0]
        out = SJ.transcode_prefix(_file(name), progressive=True, grey=True)
        for Ss, Se, Ah, Al in GREY_SCANS:
            buf = np.zeros(n * 512 + 64, np.uint8)
            length, counts, cuts = ctypes.c_uint64(), np.zeros(257, np.int64), np.zeros(2, np.int64)
            assert lib.aej_test_jfif_prog_scan_host(coef.ctypes.data, n, Ss, Se, Ah, Al, buf.ctypes.data, ctypes.c_uint64(buf.size),
                                                    ctypes.addressof(length), counts.ctypes.data, cuts.ctypes.data) == 0
            if not (Ss == 0 and Ah):                                 # the DC refinement scan has no table
                bits, vals = np.zeros(16, np.uint8), np.zeros(256, np.uint8)
                k = lib.aej_jfif_huffman_host(counts.ctypes.data, bits.ctypes.data, vals.ctypes.data, 256)
                assert k > 0
                out += b"\xff\xc4" + (19 + k).to_bytes(2, "big") + bytes([0x10 if Ss else 0]) + bits.tobytes() + vals[:k].tobytes()
            out += b"\xff\xda" + bytes([0, 8, 1, 1, 0, Ss, Se, (Ah << 4) | Al]) + buf[:length.value].tobytes()
        assert out + b"\xff\xd9" == _file(name + "_prog"), name


# ---- the new keywords, before any device context exists ---------------------------------------------------------------------------------
@pytest.fixture()
def no_context(SJ, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device context was asked for before the arguments were checked")
    monkeypatch.setattr(SJ, "get_context", boom)


def test_mode_is_checked_before_any_device_work(SJ, no_context):
    rgb, grey = np.zeros((4, 5, 3), np.uint8), np.zeros((4, 5), np.uint8)
    for mode in ("l", "RGBA", "", None, 1, b"L"):
        with pytest.raises(ValueError, match="mode"):
            SJ.standard_jpeg_encode_many([grey], mode=mode)
    for mode, images in (("L", [grey, rgb]), ("RGB", [rgb, grey]), ("auto", [grey, np.zeros((4, 5, 1), np.uint8)]),
                         ("auto", [rgb, np.zeros((4, 5, 4), np.uint8)]), ("L", [grey, np.zeros((0, 5), np.uint8)]),
                         ("auto", [grey, np.zeros(5, np.uint8)])):
        with pytest.raises(ValueError, match="image 1"):
            SJ.standard_jpeg_encode_many(images, mode=mode)
    with pytest.raises(TypeError, match="image 1"):
        SJ.standard_jpeg_encode_many([grey, np.zeros((4, 5), np.float64)], mode="L")
    with pytest.raises(ValueError, match="image 1"):
        SJ.standard_jpeg_encode_many([grey, grey], quality=[75, 0], mode="L")
    with pytest.raises(ValueError):
        SJ.standard_jpeg_encode_many([grey], subsampling="4:1:1", mode="L")      # still validated
    import torch
    t = torch.zeros((4, 5), dtype=torch.uint8)
    t.jpeg_comment = "text"
    with pytest.raises(TypeError, match="image 1"):
        SJ.standard_jpeg_encode_many([grey, t], mode="L")


def test_grey_keyword_is_checked_before_any_device_work(SJ, no_context):
    ok = _file("ramp_16x16_q10")
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="grey"):
            SJ.standard_jpeg_transcode_many([ok], grey=bad)
        with pytest.raises(TypeError, match="grey"):
            SJ.standard_jpeg_transform_many([ok], "rot90", grey=bad)
        with pytest.raises(TypeError, match="grey"):
            SJ.transcode_prefix(ok, grey=bad)
    with pytest.raises(ValueError, match="file 1"):                  # the grey geometry's refusal names the file
        SJ.standard_jpeg_transform_many([ok, _file("ramp_37x53_q100")], "flip_h", grey=True)
    with pytest.raises(ValueError, match="file 0"):
        SJ.standard_jpeg_transform_many([_file("ramp_7x9_q100")], "rot180", trim=True, grey=True)      # 7 rows trim to nothing


def test_the_defaults_still_refuse(SJ, no_context):
    grey_file, rgb = _file("ramp_16x16_q10"), np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError, match="image 1"):
        SJ.standard_jpeg_encode_many([rgb, np.zeros((4, 5), np.uint8)])
    for call in (lambda: SJ.standard_jpeg_transcode_many([grey_file]), lambda: SJ.standard_jpeg_transform_many([grey_file], "rot90"),
                 lambda: SJ.standard_jpeg_transcode_many([grey_file], grey=False), lambda: SJ.transcode_prefix(grey_file),
                 lambda: SJ.transform_prefix(grey_file, "rot90")):
        with pytest.raises(NotImplementedError, match=r"file 0.*grey=True"):
            call()


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_descriptor_refusals(lib):
    from adaptive_edge_aware_jpeg_amd._lib import SIGNATURES, JfifManyDesc
    for name in ("aej_jfif_many_coefs_grey_host", "aej_jfif_transform_coefs_grey_host", "aej_jfif_headers_grey_host"):
        assert name in SIGNATURES and hasattr(lib, name)
    assert lib.aej_abi_version() == 3
    assert [f[0] for f in JfifManyDesc._fields_] == ["src_offset", "width", "height", "quality", "components"] and ctypes.sizeof(JfifManyDesc) == 24

    def size(rows, ss=2, opt=0, prog=0):
        d = (JfifManyDesc * len(rows))(*[JfifManyDesc(*r) for r in rows])
        return lib.aej_jfif_many_workspace_bytes(None, ctypes.addressof(d), len(rows), ss, opt, prog)

    colour, grey = (0, 33, 17, 75, 0), (0, 33, 17, 75, 1)
    assert size([colour]) == size([(0, 33, 17, 75, 3)]) > size([grey]) > 0       # 0 means three; one component needs fewer blocks
    assert size([grey], 0) == size([grey], 1) == size([grey], 2)                   # the call's subsampling does not bear on a grey image
    assert size([colour, grey]) > size([colour]) and size([grey], 2, 1) > 0 and size([grey], 2, 0, 1) > 0
    for bad in ((0, 33, 17, 75, 2), (0, 33, 17, 75, 4), (0, 33, 17, 75, -1), (0, 0, 17, 75, 1), (0, 33, 65536, 75, 1), (0, 33, 17, 0, 1),
                (0, 33, 17, 101, 1)):
        assert size([grey, bad]) == 0 and size([bad, colour]) == 0, bad
