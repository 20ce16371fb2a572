"""CPU: the progressive side of standard_jpeg_decode_many without a device -- tests/progressive_reference.py pinned to Pillow, the
multi-scan parser (aej_jpegprog_parse_host) against Pillow and an independent marker walk, the library's per-thread decoders stepped
through on the host (aej_test_jpegprog_coefs_host) against the reference's coefficients, and the refusals."""
import ctypes
import io
import json
import os

import numpy as np
import pytest

import progressive_reference as R
from conftest import GOLDEN

FIXTURES = os.path.join(GOLDEN, "jpegprog")
BASELINE = os.path.join(GOLDEN, "jpegdec")


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


def _meta():
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        return json.load(f)


NAMES = [c["name"] for c in _meta()["cases"]]


def _file(name, folder=FIXTURES):
    with open(os.path.join(folder, name + ".jpg"), "rb") as f:
        return f.read()


def _pil(x, **opts):
    from PIL import Image
    img = Image.fromarray(x)
    if opts.pop("grey", False):
        img = img.convert("L")
    buf = io.BytesIO()
    img.save(buf, "JPEG", **opts)
    return buf.getvalue()


def _pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _live_files(seed, count):
    from PIL import Image
    rng = np.random.default_rng(seed)
    src = np.asarray(Image.open(os.path.join(GOLDEN, "natural", "peppers.png")).convert("RGB"))
    out = []
    for k in range(count):
        H, W = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        y, x = int(rng.integers(0, src.shape[0] - H)), int(rng.integers(0, src.shape[1] - W))
        opts = dict(quality=int(rng.integers(1, 101)), progressive=True)
        if k % 4 == 3:
            opts["grey"] = True
        else:
            opts["subsampling"] = k % 4
        if k % 3 == 1:
            opts["restart_marker_blocks"] = int(rng.integers(1, 7))
        if k % 3 == 2:
            opts["restart_marker_rows"] = 1
        out.append(_pil(np.ascontiguousarray(src[y:y + H, x:x + W]), **opts))
    return out


# ---- the reference decoder is itself pinned ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_reference_decoder_equals_pillow_on_fixtures(name):
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    data = _file(name)
    assert np.array_equal(R.decode(data), px[name])
    assert np.array_equal(px[name], _pil_decode(data))


def test_reference_decoder_equals_pillow_on_live_files():
    for k, data in enumerate(_live_files(17, 24)):
        assert np.array_equal(R.decode(data), _pil_decode(data)), k


def test_fixture_meta_matches_files():
    from PIL import Image
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    for c in _meta()["cases"]:
        im = Image.open(io.BytesIO(_file(c["name"])))
        assert list(im.size) == c["size"] and px[c["name"]].shape == (im.size[1], im.size[0], 3)
        assert len(c["scans"]) == (6 if im.mode == "L" else 10)


# ---- the parser --------------------------------------------------------------------------------------------------------------------------
def _huff_lut(counts, symbols):
    """(length << 8 | symbol) for every 9-bit prefix, 0 where the code is longer -- the look-ahead table of aej_jpegdec_huff"""
    lut, code, k = [0] * 512, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if length <= 9:
                for e in range(1 << (9 - length)):
                    lut[(code << (9 - length)) + e] = (length << 8) | symbols[k]
            code += 1
            k += 1
        code <<= 1
    return lut


@pytest.mark.parametrize("name", NAMES)
def test_parse_scans_matches_pillow_and_a_marker_walk(SJ, name):
    from PIL import Image
    data = _file(name)
    im = Image.open(io.BytesIO(data))
    frame, scans = SJ.parse_scans(data)
    assert (frame.width, frame.height) == im.size and frame.sof == 0xC2
    assert frame.ncomp == len(im.layer) == (1 if im.mode == "L" else 3)
    layer = [(frame.comp_id[i], frame.comp_h[i], frame.comp_v[i], frame.comp_tq[i]) for i in range(frame.ncomp)]
    assert layer == [(int(c[0]) if not isinstance(c[0], str) else ord(c[0]), c[1], c[2], c[3]) for c in im.layer]
    for i in range(frame.ncomp):
        assert list(frame.qt[i]) == list(im.quantization[frame.comp_tq[i]])
    assert frame.precision16 == ("qt16" in name)
    rframe, rscans = R.walk(data)
    assert frame.n_scans == len(scans) == len(rscans) and frame.n_levels == 3
    pos = None
    for s, r in zip(scans, rscans):
        assert [(s.comp[i], s.td[i], s.ta[i]) for i in range(s.ncomp)] == r["comps"]
        assert (s.ss, s.se, s.ah, s.al, s.restart_interval) == (r["ss"], r["se"], r["ah"], r["al"], r["ri"])
        assert (s.data_offset, s.data_offset + s.data_length) == (r["start"], r["end"])
        assert ("rst" in name) == (s.restart_interval > 0)
        sos = s.data_offset - (8 + 2 * s.ncomp)
        assert data[sos:sos + 2] == b"\xff\xda"
        if pos is not None:                                      # between two scans: nothing but DRI and the DHT segments the walk saw
            gap, q = [], pos
            while q < sos:
                assert data[q] == 0xFF and data[q + 1] in (0xC4, 0xDD)
                n = int.from_bytes(data[q + 2:q + 4], "big")
                gap.append((data[q + 1], data[q + 4:q + 2 + n]))
                q += 2 + n
            assert q == sos and [b for m, b in gap if m == 0xC4] == r["dht"]
        pos = s.data_offset + s.data_length
        if s.ss == 0 and s.ah == 0:
            for i in range(s.ncomp):
                assert list(s.dc[i].lut) == _huff_lut(*r["dc"][s.td[i]])
                assert bytes(s.dc[i].vals)[:len(r["dc"][s.td[i]][1])] == bytes(r["dc"][s.td[i]][1])
        if s.ss > 0:
            assert list(s.ac.lut) == _huff_lut(*r["ac"][s.ta[0]])
            assert bytes(s.ac.vals)[:len(r["ac"][s.ta[0]][1])] == bytes(r["ac"][s.ta[0]][1])
        if s.ncomp == 1 and frame.ncomp == 3 and s.comp[0] == 0:  # a non-interleaved luma scan walks the image's own blocks
            assert (s.units_x, s.units_y) == (-(-frame.width // 8), -(-frame.height // 8))
        else:
            assert (s.units_x, s.units_y) == (frame.mcux, frame.mcuy)
        units = s.units_x * s.units_y
        assert s.n_segments == (-(-units // s.restart_interval) if s.restart_interval else 1)
    assert data[pos:] == b"\xff\xd9"                              # the scans tile the file up to EOI
    levels = [s.level for s in scans]
    assert levels == ([0, 0, 0, 0, 0, 1, 1, 1, 1, 2] if frame.ncomp == 3 else [0, 0, 0, 1, 1, 2])


# ---- the library's decoders, stepped through on the host ------------------------------------------------------------------------------
def _host_coefficients(SJ, data, n_levels):
    from adaptive_edge_aware_jpeg_amd import _lib
    lib = _lib.load_library()
    frame, scans = SJ.parse_scans(data)
    arr = (_lib.JpegProgScan * len(scans))(*scans)
    nb = frame.mcux * frame.mcuy * frame.blocks_per_mcu
    out = np.zeros((nb, 64), np.int16)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    rc = lib.aej_test_jpegprog_coefs_host(ctypes.addressof(frame), ctypes.addressof(arr), ctypes.addressof(buf), len(data), n_levels,
                                          out.ctypes.data, nb)
    return rc, out, scans


@pytest.mark.parametrize("name", NAMES)
def test_host_stepped_decoders_equal_the_reference_after_each_level(SJ, name):
    data = _file(name)
    for lv in (1, 2, 3):
        rc, got, scans = _host_coefficients(SJ, data, lv)
        assert rc == 0
        ref = R.mcu_order(data, R.coefficients(data, only={i for i, s in enumerate(scans) if s.level < lv}))
        assert np.array_equal(got, ref), lv


def test_host_stepped_decoders_on_live_files(SJ):
    for k, data in enumerate(_live_files(29, 24)):
        rc, got, _ = _host_coefficients(SJ, data, 99)
        assert rc == 0 and np.array_equal(got, R.mcu_order(data, R.coefficients(data))), k


def test_host_stepped_decoders_report_a_truncated_scan(SJ):
    data = _file("buildings_128x96_q90")
    _, scans = SJ.parse_scans(data)
    for k in (0, 1, 5, 6, 9):
        a, n = scans[k].data_offset, scans[k].data_length
        rc, _, _ = _host_coefficients(SJ, data[:a + n // 2] + data[a + n:], 99)
        assert rc > 0, k                                          # an AEJ_JPEGDEC_* status, not a crash and not success


# ---- refusals, byte-patched from a valid file; all before any device work --------------------------------------------------------------
def _sos_positions(data):
    _, scans = R.walk(data)
    return [s["start"] for s in scans], scans


def _patch_sos(data, k, **fields):
    """scan k's SOS with Ss / Se / AhAl / Ns replaced"""
    starts, scans = _sos_positions(data)
    ns = len(scans[k]["comps"])
    b = bytearray(data)
    tail = starts[k] - 3
    if "ss" in fields:
        b[tail] = fields["ss"]
    if "se" in fields:
        b[tail + 1] = fields["se"]
    if "ahal" in fields:
        b[tail + 2] = fields["ahal"]
    assert ns >= 1
    return bytes(b)


def _malformed(SJ):
    good = _file("lena_64x64_420_q75")
    starts, scans = _sos_positions(good)
    sos = [s - (8 + 2 * len(sc["comps"])) for s, sc in zip(starts, scans)]
    two = good[:sos[1]] + b"\xff\xda" + (10).to_bytes(2, "big") + bytes([2, 1, 0x00, 2, 0x00, 1, 5, 0x02]) + good[starts[1]:]
    repeated = good[:sos[2]] + good[sos[1]:sos[2]] + good[sos[2]:]          # luma AC 1-5 a second time
    return {
        "Ss > Se": _patch_sos(good, 1, ss=6, se=5),
        "AC scan with two components": two,
        "Ah is not the previous Al": _patch_sos(good, 5, ahal=0x32),
        "repeated first scan": repeated,
        "missing EOI": good[:-2],
        "truncated last scan": good[:starts[-1] + 7],
        "DC scan with Se != 0": _patch_sos(good, 0, se=3),
        "Al above 13": _patch_sos(good, 1, ahal=0x0E),
    }


@pytest.mark.parametrize("kind", ["Ss > Se", "AC scan with two components", "Ah is not the previous Al", "repeated first scan", "missing EOI",
                                  "truncated last scan", "DC scan with Se != 0", "Al above 13"])
def test_malformed_scripts_raise_value_error(SJ, kind):
    bad = _malformed(SJ)[kind]
    with pytest.raises(ValueError, match="file 0"):
        SJ.parse_scans(bad)
    with pytest.raises(ValueError, match="file 2"):
        SJ.standard_jpeg_decode_many([_file("lena_64x64_420_q75"), _file("lena_64x64_420_q75", BASELINE), bad], progressive=True)


def _unsupported(SJ):
    good = _file("lena_64x64_420_q75")
    starts, scans = _sos_positions(good)
    last_sos = starts[-1] - 10
    p = good.index(b"\xff\xc2")
    return {
        "incomplete": good[:last_sos] + b"\xff\xd9",
        "SOF10": good[:p] + b"\xff\xca" + good[p + 2:],
    }


@pytest.mark.parametrize("kind", ["incomplete", "SOF10"])
def test_unsupported_raise_not_implemented(SJ, kind):
    bad = _unsupported(SJ)[kind]
    with pytest.raises(NotImplementedError, match="file 0"):
        SJ.parse_scans(bad)
    with pytest.raises(NotImplementedError, match="file 1"):
        SJ.standard_jpeg_decode_many([_file("lena_64x64_420_q75"), bad], progressive=True)


def test_incomplete_is_what_pillow_would_smooth(SJ):
    """the control of the refusal above: Pillow still opens that file, so refusing it is this library's choice"""
    bad = _unsupported(SJ)["incomplete"]
    assert _pil_decode(bad).shape == (64, 64, 3)
    assert not np.array_equal(_pil_decode(bad), _pil_decode(_file("lena_64x64_420_q75")))


def test_baseline_file_is_not_a_progressive_one(SJ):
    with pytest.raises(NotImplementedError, match="file 3"):
        SJ.parse_scans(_file("lena_64x64_420_q75", BASELINE), 3)


def test_default_call_still_refuses_progressive(SJ):
    with pytest.raises(NotImplementedError, match="file 1.*progressive"):
        SJ.standard_jpeg_decode_many([_file("lena_64x64_420_q75", BASELINE), _file("lena_64x64_420_q75")])
    with pytest.raises(NotImplementedError, match="file 0"):
        SJ.parse_header(_file("lena_64x64_420_q75"))


def test_decode_many_takes_the_progressive_argument(SJ):
    import inspect
    p = inspect.signature(SJ.standard_jpeg_decode_many).parameters
    assert list(p)[:3] == ["files", "device", "progressive"] and p["progressive"].default is False
    with pytest.raises(ValueError):
        SJ.standard_jpeg_decode_many([], progressive=True)


def test_scan_capacity_query(SJ):
    from adaptive_edge_aware_jpeg_amd import _lib
    lib = _lib.load_library()
    data = _file("house_45x61_grey_q60")
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    frame, few = _lib.JpegProgFrame(), (_lib.JpegProgScan * 2)()
    assert lib.aej_jpegprog_parse_host(ctypes.addressof(buf), len(data), ctypes.addressof(frame), None, 0, None, 0) == 0 and frame.n_scans == 6
    assert lib.aej_jpegprog_parse_host(ctypes.addressof(buf), len(data), ctypes.addressof(frame), ctypes.addressof(few), 2, None, 0) == _lib.AEJ_ERR_CAPACITY
    assert ctypes.sizeof(_lib.JpegProgScan) == 88 + 4 * ctypes.sizeof(_lib.JpegDecHuff) + 16
