"""CPU: adobe=True of standard_jpeg_decode_many without a device -- the parsers on every kind and layout of four-component and RGB-coded
file (tests/jpeg_adobe_reference.py makes them), the refusals with and without the keyword, the checks that come before any device
work, the host twins of the kernel's per-pixel colour functions, exhaustively, and the numpy statement of those rules against Pillow."""
import ctypes
import io
import json
import os

import numpy as np
import pytest

import jpeg_adobe_reference as R
from conftest import GOLDEN

HERE = os.path.join(GOLDEN, "jpeg_adobe")
FACTORS = {"1x1": (1, 1), "2x1": (2, 1), "2x2": (2, 2), "2x1k": (2, 1), "2x2k": (2, 2)}
COLOUR = {"cmyk": "CMYK", "plain": "CMYK", "ycck": "YCCK", "rgb": "RGB"}


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "meta.json")) as f:
        return json.load(f), dict(np.load(os.path.join(HERE, "pixels.npz")))


def _file(name):
    with open(os.path.join(HERE, name + ".jpg"), "rb") as f:
        return f.read()


# ---- the parsers --------------------------------------------------------------------------------------------------------------------------------
def test_every_case_parses_with_the_keyword(SJ, golden):
    meta = golden[0]
    W, H = meta["size"]
    seen = set()
    for c in meta["cases"]:
        data = _file(c["name"])
        parsed = SJ.parse_scans(data, adobe=True) if c["progressive"] else SJ.parse_header(data, adobe=True)
        f = parsed[0] if c["progressive"] else parsed
        hs, vs = FACTORS[c["layout"]]
        four, full = c["kind"] != "rgb", c["layout"].endswith("k")
        assert f.colour == COLOUR[c["kind"]] and f.ncomp == (4 if four else 3), c
        assert (f.hs, f.vs) == (hs, vs) and (f.mcux, f.mcuy) == (-(-W // (8 * hs)), -(-H // (8 * vs))), c
        assert (f.adobe.h3, f.adobe.v3) == ((hs, vs) if full else (1, 1) if four else (0, 0)), c
        assert f.blocks_per_mcu == hs * vs + 2 + (hs * vs if full else 1 if four else 0), c
        if four:                                     # component 3's tables: Pillow gives all four components table 0, the writer 1 to all but the first
            t = 1 if full else 0
            assert f.adobe.tq3 == t and bytes(f.adobe.qt3) == bytes(f.qt[t]) and f.comp_tq[3] == t, c
            if not c["progressive"]:
                assert bytes(f.adobe.dc3) == bytes(f.dc[t]) and bytes(f.adobe.ac3) == bytes(f.ac[t]), c
                assert not full or bytes(f.adobe.dc3) != bytes(f.dc[0]), c
        seen.add((f.colour, f.blocks_per_mcu))
    assert {("CMYK", 10), ("YCCK", 6), ("CMYK", 7), ("CMYK", 4), ("RGB", 3), ("RGB", 6)} <= seen


def test_without_the_keyword_every_refusal_is_todays(SJ):
    ids_only = R.drop_segments(R.make_file("rgb", "1x1", 16, 16), 0xEE)      # ids 'R','G','B', neither JFIF nor Adobe
    for data, words in ((R.make_file("cmyk", "2x2", 16, 16), "4 components (only 1 or 3)"),
                        (R.make_file("ycck", "1x1", 16, 16, True), "4 components (only 1 or 3)"),
                        (R.make_file("rgb", "2x2", 16, 16), "Adobe APP14 transform 0 (RGB colour)"),
                        (R.make_file("rgb", "1x1", 16, 16, True), "Adobe APP14 transform 0 (RGB colour)"),
                        (ids_only, "component ids 'R','G','B' without JFIF (RGB colour)")):
        for kw in ({}, {"adobe": False}):
            with pytest.raises(NotImplementedError) as e:
                SJ.standard_jpeg_decode_many([data], progressive=True, **kw)
            assert str(e.value).startswith("file 0: " + words), str(e.value)
    assert SJ.parse_header(ids_only, adobe=True).colour == "RGB"
    with pytest.raises(TypeError):
        SJ.standard_jpeg_decode_many([ids_only], adobe=1)


def test_refusals_with_the_keyword_name_the_file(SJ):
    good = R.make_file("cmyk", "1x1", 16, 16)
    odd = R.set_transform(good, 1)                   # libjpeg: "unknown Adobe color transform code", then YCCK
    rng = np.random.default_rng(3)
    k_21 = R.write_baseline(32, 32, [(2, 2, R.random_blocks(rng, 4, 4)), (1, 1, R.random_blocks(rng, 2, 2)), (1, 1, R.random_blocks(rng, 2, 2)),
                                     (2, 1, R.random_blocks(rng, 2, 4))], transform=0)
    for data, words in ((odd, "Adobe APP14 transform 1"), (k_21, "sampling factors 2x2,1x1,1x1,2x1")):
        with pytest.raises(NotImplementedError, match="file 1: .*" + words):
            SJ.standard_jpeg_decode_many([good, data], adobe=True)
    with pytest.raises(NotImplementedError, match="file 0: sampling factors 1x2,1x1,1x1,1x1"):      # 1 x 2 needs layout_440=True, as for three components
        SJ.parse_header(R.write_baseline(8, 16, [(1, 2, R.random_blocks(rng, 2, 1))] + [(1, 1, R.random_blocks(rng, 1, 1))] * 3, transform=0), adobe=True)


def test_progressive_scan_script_of_a_pillow_cmyk_file(SJ):
    """libjpeg's script for four components: an interleaved DC scan of all four, then AC scans per component"""
    frame, scans = SJ.parse_scans(R.make_file("cmyk", "2x2", 83, 61, True), adobe=True)
    got = [(s.ncomp, tuple(s.comp[:s.ncomp]), s.ss, s.se, s.ah, s.al, s.level) for s in scans]
    per = lambda ss, se, ah, al, lv: [(1, (c,), ss, se, ah, al, lv) for c in range(4)]  # noqa: E731
    assert got == [(4, (0, 1, 2, 3), 0, 0, 0, 1, 0)] + per(1, 5, 0, 2, 0) + per(6, 63, 0, 2, 0) + per(1, 63, 2, 1, 1) + \
        [(4, (0, 1, 2, 3), 0, 0, 1, 0, 1)] + per(1, 63, 1, 0, 2)
    assert frame.n_levels == 3 and frame.blocks_per_mcu == 7
    assert (scans[0].units_x, scans[0].units_y) == (6, 4) and (scans[1].units_x, scans[1].units_y) == (11, 8)
    assert (scans[4].units_x, scans[4].units_y) == (6, 4)      # K sampled 1 x 1: the MCU grid
    assert any(scans[0].dc[0].lut) and any(frame.adobe.dc3.lut)


# ---- what is checked before any device work -------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def test_argument_checks_come_before_device_work(SJ, monkeypatch):
    def no_device(*a, **k):
        raise _Reached()
    monkeypatch.setattr(SJ, "get_context", no_device)
    old = R._save(R.picture(16, 16, 3), "RGB", quality=80)
    for new in (R.make_file("cmyk", "2x2", 16, 16), R.make_file("ycck", "2x1", 16, 16, True), R.make_file("rgb", "1x1", 16, 16)):
        files = [old, new]
        for kw in ({"mode": "L"}, {"mode": ["RGB", "L"]}, {"scale": 2}, {"scale": [1, 4]}, {"box": (0, 0, 8, 8)}, {"box": [None, (1, 1, 16, 16)]}):
            with pytest.raises(NotImplementedError, match="file 1: .* of a four-component / RGB-coded file is not built"):
                SJ.standard_jpeg_decode_many(files, progressive=True, adobe=True, **kw)
        for kw in ({}, {"mode": "auto"}, {"mode": "RGB"}, {"mode": ["L", "auto"]}, {"scale": [2, 1]}, {"box": [(0, 0, 8, 8), None]},
                   {"box": [None, (0, 0, 16, 16)]}):
            with pytest.raises(_Reached):                # every check passed: the call went on to the device
                SJ.standard_jpeg_decode_many(files, progressive=True, adobe=True, **kw)


# ---- the colour rules ---------------------------------------------------------------------------------------------------------------------------------
def _host_pixels(lib, samples, colour, components):
    s = np.ascontiguousarray(samples, np.uint8).reshape(-1, 4)
    out = np.zeros((len(s), components), np.uint8)
    assert lib.aej_test_jpeg_adobe_pixels_host(s.ctypes.data, len(s), colour, components, out.ctypes.data) == 0
    return out


def test_numpy_rules_equal_pillow(golden):
    from PIL import Image
    px = golden[1]
    c, k = np.mgrid[0:256, 0:256]
    grid = np.stack([c, 255 - c, (c * 7 + 3) % 256, k], -1).astype(np.uint8)      # every (c, k) pair in channel 0, and 65536 other pairs in 1 and 2
    for a in (grid, R.noise_picture(64, 64, 4)):
        assert np.array_equal(R.cmyk_to_rgb(a), np.asarray(Image.fromarray(a, "CMYK").convert("RGB")))
    for n in ("1x1", "2x2"):                         # the same bytes but for the transform: the CMYK decode gives the samples of the YCCK one
        samples = 255 - px[f"cmyk_{n}/auto"].astype(np.int64)
        assert np.array_equal(R.cmyk_pixels(samples.astype(np.uint8)), px[f"cmyk_{n}/auto"])
        assert np.array_equal(R.ycck_pixels(samples.astype(np.uint8)), px[f"ycck_{n}/auto"])
    for key in px:
        if key.endswith("/auto") and px[key].shape[-1] == 4:
            assert np.array_equal(R.cmyk_to_rgb(px[key]), px[key[:-4] + "RGB"]), key


def test_host_colour_functions_exhaustive(lib):
    c, k = np.mgrid[0:256, 0:256]
    pixels = np.stack([c, 255 - c, (c * 7 + 3) % 256, k], -1).astype(np.uint8).reshape(-1, 4)
    samples = 255 - pixels                           # CMYK: the pixel is the inverted sample
    assert np.array_equal(_host_pixels(lib, samples, 2, 4), pixels)
    assert np.array_equal(_host_pixels(lib, samples, 2, 3), R.cmyk_to_rgb(pixels))
    v = np.array(sorted(set(range(0, 256, 5)) | {127, 128, 255}))
    assert {0, 127, 128, 255} <= set(v.tolist())
    y, cb, cr = np.meshgrid(v, v, v, indexing="ij")
    for kk in (0, 1, 127, 128, 254, 255):
        s = np.stack([y, cb, cr, np.full_like(y, kk)], -1).astype(np.uint8).reshape(-1, 4)
        want = R.ycck_pixels(s)
        assert np.array_equal(_host_pixels(lib, s, 3, 4), want)
        assert np.array_equal(_host_pixels(lib, s, 3, 3), R.cmyk_to_rgb(want))
    rgb = R.noise_picture(32, 32, 4).reshape(-1, 4)
    assert np.array_equal(_host_pixels(lib, rgb, 1, 3), rgb[:, :3])
    out = np.zeros(4, np.uint8)
    assert lib.aej_test_jpeg_adobe_pixels_host(rgb.ctypes.data, 1, 1, 4, out.ctypes.data) == -1      # four channels of an RGB-coded file
    assert lib.aej_test_jpeg_adobe_pixels_host(rgb.ctypes.data, 1, 0, 3, out.ctypes.data) == -1      # YCbCr: not this function's


# ---- the C symbols --------------------------------------------------------------------------------------------------------------------------------------
def test_c_symbols_and_the_null_array(SJ, lib):
    from adaptive_edge_aware_jpeg_amd._lib import JpegAdobe
    for name in ("aej_jpegdec_parse_host_adobe", "aej_jpegprog_parse_host_adobe", "aej_jpegdec_workspace_bytes_adobe", "aej_jpegdec_batch_adobe",
                 "aej_jpegprog_workspace_bytes_adobe", "aej_jpegprog_batch_adobe"):
        assert hasattr(lib, name), name
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "aej.h")) as f:
        text = f.read()
    assert "typedef struct aej_jpeg_adobe" in text and "uint16_t qt[3][64]" in text and "aej_jpegdec_huff dc[3], ac[3];" in text
    # an old file through the new parser: the same descriptor, colour YCbCr, nothing else
    old = R._save(R.picture(40, 56, 3), "RGB", quality=80, subsampling=2)
    a, b = SJ.parse_header(old), SJ.parse_header(old, adobe=True)
    assert bytes(a) == bytes(b) and b.colour == "YCbCr" and bytes(b.adobe) == bytes(JpegAdobe())
    assert ctypes.sizeof(JpegAdobe) == 16 + 128 + 2 * ctypes.sizeof(type(a.dc[0]))
