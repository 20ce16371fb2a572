"""GPU: standard_jpeg_transform_many (csrc/jfiftrans.hip, k_jt_transform) -- lossless flips, rotations and transpositions of JPEG files
on the device.  The main oracle is the coefficients: the output's, read by the tests' own decoder, against a NumPy restatement applied
to the source's.  Then the exact byte relations between transforms, pixels through Pillow where equality holds by construction, the
EXIF mode and the error returns."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_transform_reference as R  # noqa: E402
import progressive_reference as P  # noqa: E402
import test_gpu_jfif_transcode as TT  # noqa: E402  (its helpers: _pil, _pil_decode, _noise, IMAGES, _one_block_file)

pytestmark = pytest.mark.gpu
_pil, _pil_decode, _noise = TT._pil, TT._pil_decode, TT._noise
KINDS = (dict(), dict(progressive=True), dict(restart_marker_blocks=1))


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _supported(H, W, layout, trim):
    """the transforms a source admits, by the restatement's rules"""
    hs, vs = R.LAYOUTS[layout]
    out = []
    for name in R.NAMES:
        if name in R.TRANSPOSING and hs != vs:
            continue
        try:
            R.out_geometry(H, W, hs, vs, name, trim)
        except ValueError:
            continue
        out.append(name)
    return out


# (image, layouts, qualities, trim): the smallest shapes that can still go wrong
COEF_CASES = {
    "one_block_8x8": (lambda: _noise(8, 8), ("4:4:4",), (75,), False),
    "one_mcu_16x16": (lambda: _noise(16, 16), ("4:2:0",), (75,), False),
    "1x1": (lambda: _noise(1, 1), ("4:4:4", "4:2:0"), (75,), True),
    "9x3": (lambda: _noise(3, 9), ("4:4:4", "4:2:2", "4:2:0"), (90,), True),
    "17x33": (lambda: TT.IMAGES["primaries_17x33"](), ("4:4:4", "4:2:2", "4:2:0"), (50,), True),
    "37x53": (lambda: _noise(37, 53), ("4:4:4", "4:2:2", "4:2:0"), (75,), True),
    "perfect_48x32_422": (lambda: _noise(32, 48), ("4:2:2",), (75,), False),
    "perfect_64x48_420": (lambda: _noise(48, 64), ("4:2:0",), (75,), False),
    "lena_61x90": (lambda: TT.IMAGES["lena_61x90"](), ("4:2:0",), (10, 95), True),
}


@pytest.mark.parametrize("case", list(COEF_CASES))
def test_coefficients(A, case):
    make, layouts, qualities, trim = COEF_CASES[case]
    x = make()
    H, W = x.shape[:2]
    src, names, meta = [], [], []
    for layout in layouts:
        for q in qualities:
            f = _pil(x, quality=q, subsampling=layout)
            for name in _supported(H, W, layout, trim):
                src.append(f)
                names.append(name)
                meta.append((layout, q, f))
    assert len(set(names)) >= 2 and ("transpose" in names or layouts == ("4:2:2",))
    out = A.standard_jpeg_transform_many(src, names, progressive=True, trim=trim)
    source_coef = {}
    seen = set()
    for o, name, (layout, q, f) in zip(out, names, meta):
        hs, vs = R.LAYOUTS[layout]
        if (layout, q) not in source_coef:
            source_coef[layout, q] = P.coefficients(A.standard_jpeg_transcode_many([f], progressive=True)[0])
        if name == "none":
            assert o == A.standard_jpeg_transcode_many([f], progressive=True)[0]
            continue
        real, (oH, oW, ohs, ovs) = R.coefficients(source_coef[layout, q], H, W, hs, vs, name, trim)
        frame, _ = P.walk(o)
        assert (frame["height"], frame["width"]) == (oH, oW), (case, name, layout)
        assert (frame["comps"][0]["h"], frame["comps"][0]["v"]) == (ohs, ovs), (case, name, layout)
        R.check_padded(P.coefficients(o), real, oH, oW, ohs, ovs, f"{case} {name} {layout} q{q}")
        seen.add(name)
    assert seen


PERFECT = ((16, 16, "4:2:0"), (32, 48, "4:4:4"), (48, 64, "4:2:0"), (8, 8, "4:4:4"))
PERFECT_422 = ((32, 48, "4:2:2"), (8, 16, "4:2:2"))


def _sources(shapes, quality=75):
    return [_pil(_noise(h, w), quality=quality, subsampling=s, **KINDS[i % len(KINDS)]) for i, (h, w, s) in enumerate(shapes)] + \
           [_pil(_noise(h, w), quality=quality, subsampling=s, **KINDS[(i + 1) % len(KINDS)]) for i, (h, w, s) in enumerate(shapes)]


@pytest.mark.parametrize("prog", (False, True))
@pytest.mark.parametrize("which", ("small", "noise_256"))
def test_byte_relations(A, which, prog):
    """exact for sources of whole MCUs (no dummy block to regenerate): involutions, the compositions, none"""
    if which == "small":
        src, src422 = _sources(PERFECT), _sources(PERFECT_422)
    else:
        x = _noise(256, 256)                                     # quality 100: several decoder sync rounds
        src = [_pil(x, quality=100, subsampling="4:4:4"), _pil(x, quality=100, subsampling="4:2:0", progressive=True)]
        src422 = [_pil(x, quality=100, subsampling="4:2:2", restart_marker_rows=1)]

    def T(files, name):
        return A.standard_jpeg_transform_many(files, name, progressive=prog)

    for files, names in ((src, R.NAMES), (src422, ("none", "flip_h", "flip_v", "rot180"))):
        base = A.standard_jpeg_transcode_many(files, progressive=prog)
        assert T(files, "none") == base
        for name in ("flip_h", "flip_v", "rot180") + (("transpose", "transverse") if "transpose" in names else ()):
            once = T(files, name)
            assert all(a != b for a, b in zip(once, base)), name
            assert T(once, name) == base, f"{name} twice"
        assert T(T(files, "flip_h"), "flip_v") == T(files, "rot180")
        if "rot90" not in names:
            continue
        r90 = T(files, "rot90")
        assert r90 == T(T(files, "transpose"), "flip_h")
        assert T(r90, "rot270") == base
        assert T(T(T(r90, "rot90"), "rot90"), "rot90") == base
        assert T(T(r90, "rot90"), "none") == T(files, "rot180")
        assert T(files, "rot270") == T(T(files, "flip_h"), "transpose")
        assert T(files, "transverse") == T(T(files, "transpose"), "rot180")
    if which == "noise_256":
        from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
        T(src[:1], "rot90")
        assert SJ.decode_sync_rounds() > 0


def _mixed():
    cases = [((1, 1), "4:2:0", "transpose", dict()), ((8, 8), "4:4:4", "rot90", dict(progressive=True)), ((8, 8), "4:4:4", "none", dict()),
             ((3, 9), "4:4:4", "flip_h", dict(restart_marker_blocks=1)), ((17, 33), "4:2:0", "rot270", dict(optimize=True)),
             ((17, 33), "4:2:2", "rot180", dict()), ((37, 53), "4:2:0", "transverse", dict(progressive=True)),
             ((37, 53), "4:2:0", "none", dict(restart_marker_rows=1)), ((61, 90), "4:4:4", "rot90", dict(progressive=True)),
             ((61, 90), "4:2:2", "flip_v", dict()), ((256, 256), "4:2:0", "rot90", dict()), ((256, 256), "4:2:0", "flip_h", dict(progressive=True)),
             ((53, 37), "4:2:0", "flip_v", dict())]
    order = np.random.default_rng(12).permutation(len(cases))
    files, names, shapes = [], [], []
    for i in order:
        (h, w), layout, name, kind = cases[i]
        files.append(_pil(_noise(h, w), quality=(10, 75, 95)[i % 3], subsampling=layout, **kind))
        names.append(name)
        shapes.append((h, w, layout))
    return files, names, shapes


@pytest.mark.parametrize("prog", (False, True))
def test_mixed_call(A, prog):
    """per-file transforms over shuffled sizes, layouts and source kinds, with trim: every file equals its single-file call, Pillow opens
    it with the right size, and this library's decoder agrees with Pillow on it pixel for pixel"""
    from PIL import Image
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    files, names, shapes = _mixed()
    got = A.standard_jpeg_transform_many(files, names, progressive=prog, trim=True)
    geos = [R.out_geometry(h, w, *R.LAYOUTS[layout], name, True) for (h, w, layout), name in zip(shapes, names)]
    assert SJ.transcode_groups() == len(set(geos))
    ours = A.standard_jpeg_decode_many(got, progressive=True)
    for i, (f, name, g, (oH, oW, ohs, ovs)) in enumerate(zip(files, names, got, geos)):
        alone = A.standard_jpeg_transform_many([f], name, progressive=prog, trim=True)
        assert SJ.transcode_groups() == 1
        assert g == alone[0], f"file {i} ({name}): the mixed call and the single call differ"
        im = Image.open(io.BytesIO(g))
        assert im.size == (oW, oH) and im.mode == "RGB" and im.info.get("progressive", 0) == (1 if prog else 0), (i, name)
        assert np.array_equal(ours[i].cpu().numpy(), _pil_decode(g)), (i, name)
        if name == "none":
            assert np.array_equal(_pil_decode(g), _pil_decode(f))


def test_groups_follow_the_output_geometry(A):
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    a = _pil(_noise(32, 48), quality=75, subsampling="4:2:0")
    b = _pil(_noise(48, 32), quality=50, subsampling="4:2:0", progressive=True)
    c = _pil(_noise(32, 48), quality=75, subsampling="4:4:4")
    out = A.standard_jpeg_transform_many([a, b, c], ["rot90", "flip_h", "rot90"])
    assert SJ.transcode_groups() == 2                            # a turned and b share 32 x 48 (W x H) 4:2:0; c is 4:4:4
    assert out == [A.standard_jpeg_transform_many([f], n)[0] for f, n in zip((a, b, c), ("rot90", "flip_h", "rot90"))]
    A.standard_jpeg_transform_many([a, b, c], ["none", "flip_h", "flip_v"])
    assert SJ.transcode_groups() == 3
    A.standard_jpeg_transcode_many([a, b, c])
    assert SJ.transcode_groups() == 3


def test_pixels_where_equality_is_exact(A):
    # constant 8 x 8 tiles of distinct colours, 4:4:4, quality 100: DC-only blocks, so the decoded image is tiles again, whatever the
    # transform -- placement and geometry end to end
    tiles = np.random.default_rng(40).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    x = np.repeat(np.repeat(tiles, 8, 0), 8, 1)
    assert x.shape == (24, 40, 3) and len({tuple(t) for t in tiles.reshape(-1, 3)}) == 15
    src = _pil(x, quality=100, subsampling="4:4:4")
    dec = _pil_decode(src)
    assert np.array_equal(dec, np.repeat(np.repeat(dec[::8, ::8], 8, 0), 8, 1))      # Pillow alone: the tiles decode as tiles
    for prog in (False, True):
        out = A.standard_jpeg_transform_many([src] * 8, list(R.NAMES), progressive=prog)
        for name, o in zip(R.NAMES, out):
            assert np.array_equal(_pil_decode(o), R.pixels(dec, name)), name
    # flip_v of any 4:4:4 image: libjpeg's column pass comes first and reverses exactly
    for h, w in ((40, 37), (8, 8), (64, 90)):
        y = _noise(h, w) if h != 64 else np.ascontiguousarray(TT.T._png("lena")[200:264, 230:320])
        for q in (10, 75, 95):
            f = _pil(y, quality=q, subsampling="4:4:4")
            o = A.standard_jpeg_transform_many([f], "flip_v")[0]
            assert np.array_equal(_pil_decode(o), _pil_decode(f)[::-1]), (h, w, q)


def _segment(data, marker, start=b""):
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    return [bytes(data[a:b]) for m, a, b in SJ.marker_segments(data) if m == marker and bytes(data[a + 4:a + 4 + len(start)]) == start]


def test_exif(A):
    from PIL import Image
    x = _noise(32, 48)
    icc = bytes(range(256)) * 4
    want_name = (None, "none", "flip_h", "rot180", "flip_v", "transpose", "rot90", "transverse", "rot270")
    files = []
    for v in range(1, 9):
        e = Image.Exif()
        e[0x010E] = "a description"
        e[0x0112] = v
        files.append(_pil(x, quality=75, subsampling="4:2:0", exif=e.tobytes(), icc_profile=icc, comment=b"hello"))
        assert A.exif_orientation(files[-1]) == v
    plain = _pil(x, quality=75, subsampling="4:2:0")
    for prog in (False, True):
        got = A.standard_jpeg_transform_many(files + [plain], "exif", progressive=prog)
        assert got[:8] == A.standard_jpeg_transform_many(files, list(want_name[1:]), progressive=prog)
        assert got[8] == A.standard_jpeg_transcode_many([plain], progressive=prog)[0]      # no EXIF: the plain transcode
        kept = A.standard_jpeg_transform_many(files + [plain], "exif", progressive=prog, keep_metadata=True)
        assert kept[8] == got[8]
        for v, (f, g, k) in enumerate(zip(files, got, kept), 1):
            im = Image.open(io.BytesIO(k))
            assert im.getexif().get(0x0112) == 1 and im.getexif().get(0x010E) == "a description", v
            assert im.info["icc_profile"] == icc and im.info["comment"] == b"hello"
            assert np.array_equal(np.asarray(im.convert("RGB")), _pil_decode(g))
            assert im.size == ((32, 48) if want_name[v] in R.TRANSPOSING else (48, 32))
            (a,), (b,) = _segment(f, 0xE1, b"Exif"), _segment(k, 0xE1, b"Exif")
            at = a.index(b"\x01\x12\x00\x03\x00\x00\x00\x01") + 8      # Pillow writes the big-endian order: the entry's value follows
            assert a[at:at + 2] == bytes([0, v]) and b[at:at + 2] == bytes([0, 1]), v
            assert len(a) == len(b) and a[:at] + a[at + 2:] == b[:at] + b[at + 2:], v      # the segment differs in exactly those two bytes
            assert _segment(f, 0xE2) == _segment(k, 0xE2) and _segment(f, 0xFE) == _segment(k, 0xFE)
            meta = len(a) + sum(map(len, _segment(f, 0xE2) + _segment(f, 0xFE)))
            assert k[:20] + k[20 + meta:] == g                    # and the rest is the file without metadata
        # explicit names leave the metadata untouched
        named = A.standard_jpeg_transform_many(files[5:6], "rot90", progressive=prog, keep_metadata=True)[0]
        assert _segment(named, 0xE1, b"Exif") == _segment(files[5], 0xE1, b"Exif") and Image.open(io.BytesIO(named)).getexif().get(0x0112) == 6


def test_errors(A):
    good = _pil(_noise(37, 53), quality=75, subsampling="4:2:0")
    other = _pil(_noise(8, 8), quality=75, subsampling="4:4:4", progressive=True)
    want = A.standard_jpeg_transform_many([good, other], ["rot90", "transpose"], trim=True)
    cut = good[:good.index(b"\xff\xda") + 14 + 40]           # the scan ends after 40 bytes
    with pytest.raises(ValueError, match=r"file 1: truncated scan"):
        A.standard_jpeg_transform_many([good, cut, other], ["rot90", "rot270", "transpose"], trim=True)
    inside = [TT._one_block_file(1023, 1023), TT._one_block_file(-1024, -1023), TT._one_block_file(1023, -1023, 63),
              TT._one_block_file(-1024, 1023, 63)]
    for prog in (False, True):
        for name in ("flip_h", "flip_v", "transpose", "rot90"):  # the limits are symmetric but for the DC, which keeps its sign
            out = A.standard_jpeg_transform_many(inside, name, progressive=prog)
            assert A.standard_jpeg_transform_many(out, name if name != "rot90" else "rot270", progressive=prog) == \
                A.standard_jpeg_transcode_many(inside, progressive=prog), name
        bad = TT._one_block_file(3, 1024)
        for name in ("flip_h", "transverse"):
            with pytest.raises(ValueError, match=r"file 2: coefficient out of range"):
                A.standard_jpeg_transform_many([good, other, bad], ["flip_v", "rot180", name], progressive=prog, trim=True)
        bad_dc = TT._one_block_file(1024, 5)
        with pytest.raises(ValueError, match=r"file 0: coefficient out of range"):
            A.standard_jpeg_transform_many([bad_dc, other], "rot270", progressive=prog)
    assert A.standard_jpeg_transform_many([good, other], ["rot90", "transpose"], trim=True) == want      # the device goes on working
