"""CPU: the host half of png_decode_many for Adam7-interlaced and 16-bit files -- the two references of the GPU test
(tests/png_adam7_reference.py: the reader and live Pillow) against each other on every file that test decodes, png_adam7_passes against
the specification's 8 x 8 pattern, png_parse_header with interlaced=True / depth16=True against Pillow's mode and the writer's stream
length, the unchanged refusals without the keywords, and the new C entries called directly."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import png_adam7_reference as Z
import png_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _groups():
    """the suite in a few dozen groups, so that a failure names a family of files and the run is not a thousand tests"""
    out = {}
    for n in sorted(Z.suite()):
        out.setdefault(re.sub(r"^s\dx(\d)_", r"s_h\1_", n) if n.startswith("s") else n.split("_")[0] + "_" + n.split("_")[1], []).append(n)
    return out


@pytest.mark.parametrize("group", sorted(_groups()))
def test_reader_and_pillow_agree(group):
    for name in _groups()[group]:
        head, _ = Z.read_png(Z.suite()[name])
        for mode in ("RGB", "auto"):
            want = Z.expected(name, mode)                # asserts the agreement
            h, w, ct, depth = head["height"], head["width"], head["colour_type"], head["bit_depth"]
            if mode == "RGB" or ct == 3:
                shape, dtype = (h, w, 3), np.uint8
            elif depth == 16:
                shape, dtype = ((h, w), np.uint16) if ct == 0 else ((h, w, 3 if ct == 2 else 4), np.uint8)
            else:
                shape, dtype = ((h, w) if ct == 0 else (h, w, head["channels"])), np.uint8
            assert want.shape == shape and want.dtype == dtype, (name, mode)
        assert head["interlace"] == int(name.endswith("_i")), name


def test_an_interlaced_file_is_its_plain_twin():
    """the same samples written both ways read back equal, at the sizes where passes are empty, and the 16-bit samples show the clip
    and bytes that differ"""
    rng = np.random.default_rng(3)
    for ct, depth in Z.KINDS:
        for w, h in ((1, 1), (2, 3), (5, 4), (9, 11)):
            s = Z.random_samples(rng, w, h, depth, ct)
            extra = [R.palette_chunk(rng, 1 << depth)] if ct == 3 else []
            a = Z.make_png(w, h, depth, ct, s, 0, 0, extra_chunks=extra)
            b = Z.make_png(w, h, depth, ct, s, [(r * 3) % 5 for r in range(h)], 1, extra_chunks=extra)
            for mode in ("RGB", "auto"):
                assert np.array_equal(Z.reference(a, mode), Z.reference(b, mode)) and np.array_equal(Z.pillow(a, mode), Z.pillow(b, mode))
                assert np.array_equal(Z.reference(b, mode), Z.pillow(b, mode)), (ct, depth, w, h, mode)
    g = Z.read_png(Z.suite()["grey16_7x5"])[1]
    assert (g > 255).any() and (g < 255).any() and ((g >> 8) != (g & 255)).any()
    assert Z.expected("grey16_7x5", "RGB").max() == 255 and Z.expected("grey16_7x5", "auto").max() > 255


def test_adam7_passes_against_the_pattern(A):
    for w in range(1, 18):
        for h in range(1, 18):
            passes = A.png_adam7_passes(w, h)
            assert len(passes) == 7
            seen = np.zeros((h, w), np.int32)
            for p, (x0, y0, dx, dy, wp, hp) in enumerate(passes, 1):
                ys, xs = Z.pass_pixels(w, h, p)
                assert (wp, hp) == (len(xs), len(ys)), (w, h, p)
                assert (wp == 0) == (hp == 0)
                assert [x0 + i * dx for i in range(wp)] == xs and [y0 + j * dy for j in range(hp)] == ys, (w, h, p)
                for y in ys:
                    for x in xs:
                        assert Z.ADAM7[y & 7][x & 7] == p
                        seen[y, x] += 1
            assert (seen == 1).all()
    for bad in ((0, 4), (4, 0), (-1, 3), (2.5, 3), ("3", 3)):
        with pytest.raises(ValueError):
            A.png_adam7_passes(*bad)
    assert "png_adam7_passes" in A.__all__


@pytest.mark.parametrize("interlace", (0, 1))
@pytest.mark.parametrize("ct,depth", Z.KINDS)
def test_header_with_the_keywords(A, ct, depth, interlace):
    from PIL import Image
    rng = np.random.default_rng(4)
    for w, h in ((13, 7), (1, 1), (2, 3), (3, 2), (300, 2), (9, 11)):
        data = Z.kind_file(rng, w, h, ct, depth, 0, interlace)
        d = A.png_parse_header(data, interlaced=True, depth16=True)
        im = Image.open(io.BytesIO(data))
        assert (d.width, d.height) == im.size == (w, h) and d.mode == im.mode, (d.mode, im.mode)
        assert (d.bit_depth, d.colour_type, d.channels, d.interlace) == (depth, ct, R.CHANNELS[ct], interlace)
        assert d.row_bytes == (w * R.CHANNELS[ct] * depth + 7) // 8
        assert d.raw_bytes == Z.raw_bytes(w, h, depth, ct, interlace) == Z.read_png(data)[0]["raw_bytes"]
        if interlace:                                    # a pass without pixels has no bytes, not even filter bytes
            rb = lambda wp: (wp * R.CHANNELS[ct] * depth + 7) // 8  # noqa: E731
            assert d.raw_bytes == sum(hp * (1 + rb(wp)) for _, _, _, _, wp, hp in A.png_adam7_passes(w, h) if wp)
        else:
            assert d.raw_bytes == h * (1 + d.row_bytes)


def test_refusals_without_the_keywords_are_unchanged(A):
    rng = np.random.default_rng(5)
    good = R.kind_file(rng, 8, 4, 2, 8, 0)
    inter, deep, both = (Z.kind_file(rng, 8, 4, 2, d, 0, i) for d, i in ((8, 1), (16, 0), (16, 1)))
    for data, text, keyword, other in ((inter, "Adam7 interlace is not built", "interlaced=True", dict(depth16=True)),
                                       (deep, "16-bit samples are not built", "depth16=True", dict(interlaced=True))):
        for kw in ({}, other):
            with pytest.raises(NotImplementedError, match=r"^file 5: " + text + ".*" + keyword):
                A.png_parse_header(data, 5, **kw)
            with pytest.raises(NotImplementedError, match=r"^file 1: " + text + ".*" + keyword):      # before any device work
                A.png_decode_many([good, data], **kw)
    with pytest.raises(NotImplementedError, match="16-bit"):
        A.png_parse_header(both, interlaced=True)
    with pytest.raises(NotImplementedError, match="Adam7"):
        A.png_parse_header(both, depth16=True)
    assert A.png_parse_header(both, interlaced=True, depth16=True).interlace == 1
    for kw in (dict(interlaced=1), dict(depth16="yes"), dict(interlaced=None)):
        with pytest.raises(TypeError):
            A.png_parse_header(good, **kw)
        with pytest.raises(TypeError):
            A.png_decode_many([good], **kw)
    # APNG stays refused with both keywords; palette files have no depth 16
    apng = R.make_png(8, 4, 8, 2, np.zeros((4, 8, 3), np.uint8), 0, extra_chunks=[(b"acTL", b"\0\0\0\1\0\0\0\0")])
    with pytest.raises(NotImplementedError, match="APNG"):
        A.png_parse_header(apng, interlaced=True, depth16=True)
    with pytest.raises(ValueError, match="not a PNG image type"):
        A.png_parse_header(Z.make_png(4, 4, 16, 3, np.zeros((4, 4, 1), np.uint16), 0), depth16=True)


def test_parse_entry_directly(A):
    """aej_png_parse_host_accept without the Python layer: the flag word, the old entry as its call with 0, aej_png_raw_bytes"""
    from adaptive_edge_aware_jpeg_amd._lib import AEJ_ERR_ARG, AEJ_ERR_UNSUPPORTED, PngDesc, load_library
    lib = load_library()
    rng = np.random.default_rng(6)
    data = Z.kind_file(rng, 9, 5, 6, 16, 0, 1)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    d, msg = PngDesc(), ctypes.create_string_buffer(64)
    spans = np.zeros((2, 2), np.int64)
    args = lambda accept: (ctypes.addressof(buf), len(data), accept, ctypes.addressof(d), spans.ctypes.data, 2, ctypes.addressof(msg), 64)  # noqa: E731
    assert lib.aej_png_parse_host_accept(*args(0)) == AEJ_ERR_UNSUPPORTED and msg.value == b"16-bit samples are not built"
    assert lib.aej_png_parse_host(ctypes.addressof(buf), len(data), ctypes.addressof(d), None, 0, ctypes.addressof(msg), 64) == AEJ_ERR_UNSUPPORTED
    assert msg.value == b"16-bit samples are not built"
    assert lib.aej_png_parse_host_accept(*args(2)) == AEJ_ERR_UNSUPPORTED and msg.value == b"Adam7 interlace is not built"
    assert lib.aej_png_parse_host_accept(*args(1)) == AEJ_ERR_UNSUPPORTED and b"16-bit" in msg.value
    assert lib.aej_png_parse_host_accept(*args(4)) == AEJ_ERR_ARG and lib.aej_png_parse_host_accept(*args(7)) == AEJ_ERR_ARG
    assert lib.aej_png_parse_host_accept(*args(3)) == 0 and msg.value == b""
    assert (d.width, d.height, d.bit_depth, d.colour_type, d.interlace, d.row_bytes, d.mode) == (9, 5, 16, 6, 1, 72, "RGBA")
    assert d.n_idat == 1 and spans[0].tolist() == [R.read_chunks(data)[1][2], len(R.read_chunks(data)[1][1])]
    assert lib.aej_png_raw_bytes(ctypes.addressof(d)) == Z.raw_bytes(9, 5, 16, 6, 1)
    d.interlace = 0
    assert lib.aej_png_raw_bytes(ctypes.addressof(d)) == 5 * 73
    d.bit_depth = 12
    assert lib.aej_png_raw_bytes(ctypes.addressof(d)) == 0 and lib.aej_png_raw_bytes(None) == 0
    t = np.full((8, 6), -1, np.int32)
    assert lib.aej_png_adam7_passes_host(9, 5, t.ctypes.data) == 0 and (t[7] == -1).all()
    assert t[:7].tolist() == [list(p) for p in A.png_adam7_passes(9, 5)]
    assert lib.aej_png_adam7_passes_host(0, 5, t.ctypes.data) == AEJ_ERR_ARG and lib.aej_png_adam7_passes_host(3, 5, None) == AEJ_ERR_ARG


def test_header_symbols_resolve():
    from adaptive_edge_aware_jpeg_amd import _lib, png
    with open(os.path.join(ROOT, "include", "aej.h")) as f:
        h = f.read()
    lib = _lib.load_library()
    for name, res in (("aej_png_parse_host_accept", "int"), ("aej_png_raw_bytes", "uint64_t"), ("aej_png_adam7_passes_host", "int")):
        assert re.search(r"AEJ_API " + res + " " + name + r"\(", h) and name in _lib.SIGNATURES and hasattr(lib, name)
    for k, v in (("AEJ_PNG_ACCEPT_ADAM7", png.ACCEPT_ADAM7), ("AEJ_PNG_ACCEPT_16BIT", png.ACCEPT_16BIT)):
        assert re.search(k + r" = " + str(v) + r"\b", h), k
    assert (png.ACCEPT_ADAM7, png.ACCEPT_16BIT) == (1, 2)
