"""GPU: crop= and drop_chroma= of standard_jpeg_transform_many (csrc/jfiftrans.hip, k_jt_cut) -- jpegtran's -crop and -grayscale on the
device.  The main oracle is the coefficients: the output's, read by the tests' own decoder, against the NumPy restatement
(jfif_cut_reference) applied to the source's.  Then pixels through Pillow where equality holds by construction, the exact byte
relations, a mixed call and the error returns."""
import io
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_440_reference as F  # noqa: E402
import jfif_cut_reference as C  # noqa: E402
import jfif_restart_reference as RR  # noqa: E402
import jfif_transcode_helpers as H  # noqa: E402
import jfif_transform_reference as R  # noqa: E402
import progressive_reference as P  # noqa: E402
import test_gpu_jfif_transcode as TT  # noqa: E402  (its helpers: _pil, _pil_decode, _noise, IMAGES, _one_block_file)

pytestmark = pytest.mark.gpu
_pil, _pil_decode, _noise = TT._pil, TT._pil_decode, TT._noise
ANY = dict(grey=True, layout_440=True)                          # every source layout the call can take


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _grey(x, **opts):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(x).convert("L").save(buf, "JPEG", **opts)
    return buf.getvalue()


def _luma(data):
    """Pillow's decode of the luma plane alone (libjpeg's grey output of a colour file: the Y samples, no chroma involved)"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    assert im.mode == "L"
    return np.asarray(im)


BOX = (19, 9, 43, 30)                                            # an unaligned corner; on 4:2:0 3 luma block columns over 2 MCU columns


def _sources():
    """name -> (file, H, W, hs, vs, one component), 50 x 37 each: noise, and the small natural image of the transcode tests"""
    x = _noise(37, 50)
    lena = np.ascontiguousarray(TT.IMAGES["lena_61x90"]()[:37, :50])
    out = {layout: (_pil(x, quality=75, subsampling=layout, **kind), 37, 50, *C.LAYOUTS[layout], False)
           for layout, kind in (("4:2:0", dict()), ("4:2:2", dict(progressive=True)), ("4:4:4", dict(restart_marker_blocks=1)))}
    out["4:4:0"] = (F.make_440(50, 37), 37, 50, 1, 2, False)
    out["grey"] = (_grey(x, quality=75), 37, 50, 1, 1, True)
    out["lena"] = (_pil(lena, quality=90, subsampling="4:2:0"), 37, 50, 2, 2, False)
    return out


# (source, transform, trim, box); the boxes of the turned cases lie in the 32 x 50 (rot90) and 32 x 48 (transverse) images the trim leaves
CASES = (("4:2:0", "none", False, BOX), ("4:2:2", "none", False, BOX), ("4:4:4", "none", False, BOX), ("4:4:0", "none", False, BOX),
         ("grey", "none", False, BOX), ("lena", "none", False, BOX), ("4:2:0", "rot90", True, (19, 9, 30, 43)),
         ("4:2:0", "transverse", True, (19, 9, 30, 43)), ("4:2:0", "none", False, (20, 20, 21, 21)), ("4:4:0", "rot270", True, (9, 3, 28, 24)),
         ("4:2:2", "flip_h", True, (17, 0, 48, 37)), ("grey", "rot180", True, (9, 9, 41, 26)), ("4:2:0", "flip_v", True, None),
         ("4:2:2", "transpose", False, (3, 17, 30, 50)), ("4:4:4", "transverse", True, (0, 0, 9, 9)))


@pytest.fixture(scope="module")
def sources(A):
    src = _sources()
    prog = A.standard_jpeg_transcode_many([s[0] for s in src.values()], progressive=True, **ANY)
    return src, {k: P.coefficients(p) for k, p in zip(src, prog)}


@pytest.mark.parametrize("drop", (False, True), ids=("keep", "drop_chroma"))
@pytest.mark.parametrize("prog", (False, True), ids=("baseline", "progressive"))
def test_coefficients(A, sources, prog, drop):
    src, coef = sources
    cases = [c for c in CASES if drop or not (c[1] in R.TRANSPOSING and c[0] == "4:2:2")]      # 4:2:2 turned with its chroma: see test_440
    got = A.standard_jpeg_transform_many([src[c[0]][0] for c in cases], [c[1] for c in cases], progressive=prog, trim=True,
                                         crop=[c[3] for c in cases], drop_chroma=drop, **ANY)
    readable = got if prog else A.standard_jpeg_transcode_many(got, progressive=True, **ANY)      # the same coefficients in a file the tests' decoder reads
    for (key, name, _, box), g, p in zip(cases, got, readable):
        _, H, W, hs, vs, one = src[key]
        planes = coef[key]
        real, (oH, oW, ohs, ovs), kept = C.cut(planes, H, W, hs, vs, name, True, box, drop)
        what = f"{key} {name} {box} prog={prog} drop={drop}"
        frame, _ = P.walk(p)
        assert (frame["height"], frame["width"], len(frame["comps"])) == (oH, oW, 1 if (one or drop) else 3), what
        if not (one or drop):
            assert (frame["comps"][0]["h"], frame["comps"][0]["v"]) == (ohs, ovs), what
        C.check_padded(P.coefficients(p), real, oH, oW, ohs, ovs, what)
        if box is not None:
            from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
            assert SJ.transform_crop_box(src[key][0], name, box, trim=True, drop_chroma=drop, **ANY) == kept, what


def test_440_output_with_a_crop(A, sources):
    """a 4:2:2 source turned into 4:4:0 and cropped on its 8 x 16 grid"""
    src, coef = sources
    f, H, W, hs, vs, _ = src["4:2:2"]
    for prog in (False, True):
        g = A.standard_jpeg_transform_many([f], "rot90", progressive=prog, trim=True, crop=(9, 17, 30, 47), layout_440=True)[0]
        p = g if prog else A.standard_jpeg_transcode_many([g], progressive=True, layout_440=True)[0]
        real, (oH, oW, ohs, ovs), kept = C.cut(coef["4:2:2"], H, W, hs, vs, "rot90", True, (9, 17, 30, 47))
        assert (ohs, ovs) == (1, 2) and kept == (8, 16, 30, 47)
        frame, _ = P.walk(p)
        assert (frame["height"], frame["width"], frame["comps"][0]["h"], frame["comps"][0]["v"]) == (oH, oW, 1, 2)
        C.check_padded(P.coefficients(p), real, oH, oW, ohs, ovs, f"4:2:2 rot90 to 4:4:0 prog={prog}")


def test_pixels_where_equality_is_exact(A, sources):
    from PIL import Image
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    src, _ = sources
    for prog in (False, True):
        for key in ("4:4:4", "grey", "4:2:0", "4:2:2", "4:4:0", "lena"):
            f = src[key][0]
            for name, box in (("none", BOX), ("flip_v", (3, 11, 50, 32)), ("rot90", (9, 17, 30, 47))):
                if name == "rot90" and key == "4:2:2":
                    continue
                whole = A.standard_jpeg_transform_many([f], name, progressive=prog, trim=True, **ANY)[0]
                g = A.standard_jpeg_transform_many([f], name, progressive=prog, trim=True, crop=box, **ANY)[0]
                L, U, right, lower = SJ.transform_crop_box(f, name, box, trim=True, **ANY)
                im = Image.open(io.BytesIO(g))
                assert im.size == (right - L, lower - U) and im.info.get("progressive", 0) == int(prog), (key, name)
                if key in ("4:4:4", "grey"):                  # no up-sampling: every pixel comes from its own blocks alone
                    assert im.mode == ("L" if key == "grey" else "RGB")
                    assert np.array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(whole)))[U:lower, L:right]), (key, name, prog)
                else:                                             # the luma IDCT is per block
                    assert np.array_equal(_luma(g), _luma(whole)[U:lower, L:right]), (key, name, prog)


def test_drop_chroma(A, sources):
    from PIL import Image
    src, _ = sources
    wide = _pil(_noise(32, 48), quality=75, subsampling="4:2:2")         # whole MCUs under both the 16 x 8 and the 8 x 8 rule
    odd = _pil(_noise(24, 40), quality=75, subsampling="4:2:0")          # 40 x 24: perfect at 8, not at 16
    for prog in (False, True):
        for f, name, kw in ((wide, "rot90", dict()), (wide, "transpose", dict()), (wide, "flip_h", dict()), (src["4:2:0"][0], "none", dict()),
                            (src["4:4:0"][0], "none", dict(layout_440=True)), (src["lena"][0], "flip_v", dict(trim=True))):
            g = A.standard_jpeg_transform_many([f], name, progressive=prog, drop_chroma=True, **kw)[0]      # (4:2:2 turned: no layout_440)
            plain = A.standard_jpeg_transform_many([f], name, progressive=prog, **dict(kw, layout_440=True))[0]
            im = Image.open(io.BytesIO(g))
            assert im.mode == "L" and im.info.get("progressive", 0) == int(prog)
            want = _luma(plain)
            if name == "flip_v":                                  # 37 rows: the 8 x 8 rule trims to 32 as the 16 x 16 rule does
                assert want.shape == (32, 50)
            assert np.array_equal(np.asarray(im), want), (name, prog)
            assert g == A.standard_jpeg_transcode_many([g], progressive=prog, grey=True)[0]      # the transcoder's grey file of itself
        g = A.standard_jpeg_transform_many([odd], "flip_h", progressive=prog, drop_chroma=True)[0]
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(g))), _luma(odd)[:, ::-1])      # a grey file's mirror is exact (test_gpu_jfif_grey)
        with pytest.raises(ValueError, match=r"file 0: flip_h of a 40 x 24 file mirrors an axis that is not a whole number of its 16 x 16 MCUs"):
            A.standard_jpeg_transform_many([odd], "flip_h", progressive=prog)
        # a one-component source passes through unchanged
        grey = src["grey"][0]
        assert A.standard_jpeg_transform_many([grey], "none", progressive=prog, grey=True, drop_chroma=True) == \
            A.standard_jpeg_transcode_many([grey], progressive=prog, grey=True)
        # a colour file whose chroma is flat: the luma plane is the grey file's
        y = Image.fromarray(_noise(37, 50)[:, :, 0])
        flat = Image.new("L", y.size, 128)
        buf, buf_l = io.BytesIO(), io.BytesIO()
        Image.merge("YCbCr", (y, flat, flat)).save(buf, "JPEG", quality=80, subsampling="4:2:0")
        y.save(buf_l, "JPEG", quality=80)
        g = A.standard_jpeg_transform_many([buf.getvalue()], "none", progressive=prog, drop_chroma=True)[0]
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(g))), np.asarray(Image.open(io.BytesIO(buf_l.getvalue()))))


def test_foreign_component_ids(A, sources):
    """the ids of the output's components alone decide: a dropped chroma takes its ids with it"""
    from PIL import Image
    src, _ = sources
    f = src["4:2:0"][0]
    for prog in (False, True):
        want = A.standard_jpeg_transform_many([f], "rot90", progressive=prog, trim=True, crop=BOX[:2] + (30, 43), drop_chroma=True)[0]
        for ids in ((0, 1, 2), (1, 7, 9), (ord("Y"), ord("C"), ord("c"))):
            g = A.standard_jpeg_transform_many([H.with_ids(f, ids)], "rot90", progressive=prog, trim=True, crop=BOX[:2] + (30, 43), drop_chroma=True)[0]
            frame, scans = H.ids_of(g)
            assert frame == [ids[0]] and scans == [[ids[0]]] * (6 if prog else 1), (ids, prog)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(g))), np.asarray(Image.open(io.BytesIO(want))))
            kept = A.standard_jpeg_transform_many([H.with_ids(f, ids)], "none", progressive=prog, crop=BOX)[0]
            assert H.ids_of(kept)[0] == list(ids) and H.ids_of(kept)[1][0] == list(ids)
            assert np.array_equal(_pil_decode(kept), _pil_decode(A.standard_jpeg_transform_many([f], "none", progressive=prog, crop=BOX)[0]))


@pytest.mark.parametrize("prog", (False, True), ids=("baseline", "progressive"))
def test_byte_relations(A, sources, prog):
    src, _ = sources
    files = [s[0] for s in src.values()]
    sizes = [(s[2], s[1]) for s in src.values()]

    def T(f, name="none", **kw):
        return A.standard_jpeg_transform_many(f, name, progressive=prog, **ANY, **kw)

    # the box of the whole image is no crop
    assert T(files, crop=(0, 0, 50, 37)) == T(files) == A.standard_jpeg_transcode_many(files, progressive=prog, **ANY)
    assert T(files, crop=[(0, 0, w, h) for w, h in sizes], restart_marker_rows=1) == T(files, restart_marker_rows=1)
    assert T(files[:1], "rot90", trim=True, crop=(0, 0, 32, 50)) == T(files[:1], "rot90", trim=True)
    assert T(files[:1], "rot90", trim=True, crop=(7, 15, 32, 50)) == T(files[:1], "rot90", trim=True)      # the corner moves to (0, 0)
    # aligned crop, then aligned crop: the composed crop
    x = _pil(_noise(64, 96), quality=75, subsampling="4:2:0")
    first = T([x], crop=(16, 16, 83, 61))
    assert T(first, crop=(16, 16, 60, 40)) == T([x], crop=(32, 32, 76, 56))
    assert T(T([x], "rot180", crop=(16, 16, 83, 61)), crop=(16, 16, 60, 40)) == T([x], "rot180", crop=(32, 32, 76, 56))
    # a cut file is a file like any other: the transcoder leaves it as it is (its dummy blocks follow libjpeg's rule)
    cut = T(files, crop=BOX)
    assert cut == A.standard_jpeg_transcode_many(cut, progressive=prog, **ANY)
    assert all(a != b for a, b in zip(cut, T(files)))
    dropped = T(files, crop=BOX, drop_chroma=True)
    assert dropped == A.standard_jpeg_transcode_many(dropped, progressive=prog, grey=True)
    assert dropped == T(T(files, drop_chroma=True), crop=BOX) and dropped[4] == cut[4]      # (the grey source: the drop changes nothing)
    # crop then drop is drop then crop where the two grids agree (a corner on the 16 x 16 grid)
    assert T(T(files[:1], crop=(16, 16, 43, 30)), drop_chroma=True) == T(files[:1], crop=(16, 16, 43, 30), drop_chroma=True)


def test_mixed_call(A, sources):
    """colour, grey and 4:4:0 sources, a box or None per file, "exif" with the metadata carried, a restart marker per MCU row"""
    from PIL import Image
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    src, _ = sources
    e = Image.Exif()
    e[0x0112] = 6
    turned = _pil(_noise(37, 50), quality=75, subsampling="4:2:0", exif=e.tobytes(), comment=b"hello")
    e[0x0112] = 3
    upside = _pil(_noise(32, 48), quality=60, subsampling="4:2:2", exif=e.tobytes(), progressive=True)
    files = [src["4:2:0"][0], turned, src["grey"][0], src["4:4:0"][0], upside, src["4:4:4"][0], src["lena"][0], src["4:2:2"][0]]
    boxes = [BOX, (9, 17, 30, 47), (3, 9, 27, 30), None, (16, 8, 48, 32), (19, 9, 43, 30), BOX, None]
    names = ["none", "rot90", "none", "none", "rot180", "none", "none", "none"]
    layouts = [(2, 2), (2, 2), (1, 1), (1, 2), (2, 1), (1, 1), (2, 2), (2, 1)]
    shapes = [(37, 50), (37, 50), (37, 50), (37, 50), (32, 48), (37, 50), (37, 50), (37, 50)]
    for prog in (False, True):
        kw = dict(progressive=prog, trim=True, keep_metadata=True, restart_marker_rows=1, **ANY)
        got = A.standard_jpeg_transform_many(files, "exif", crop=boxes, **kw)
        geos = [C.geometry(h, w, hs, vs, name, True, box, False, i == 2)[0] + (i == 2,)
                for i, ((h, w), (hs, vs), name, box) in enumerate(zip(shapes, layouts, names, boxes))]
        assert SJ.transcode_groups() == len(set(geos)) == 7     # files 0 and 6 share a geometry; 2 and 5 a size, but 2 is grey
        for i, (f, g, box, geo) in enumerate(zip(files, got, boxes, geos)):
            assert g == A.standard_jpeg_transform_many([f], "exif", crop=box, **kw)[0], f"file {i}: the mixed call and the single call differ"
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                im = Image.open(io.BytesIO(g))
                im.load()
            oH, oW, ohs, ovs, one = geo
            assert im.size == (oW, oH) and im.mode == ("L" if one else "RGB"), i
            assert im.getexif().get(0x0112, 1) == 1
            if prog:
                continue
            per_row, rows = -(-oW // (8 * ohs)), -(-oH // (8 * ovs))      # the cropped output's MCU grid
            assert RR.dri_sequence(g) == [per_row], i
            assert RR.markers(g) == [[0xD0 + (k & 7) for k in range(rows - 1)]], i
        assert Image.open(io.BytesIO(got[1])).info["comment"] == b"hello"


def test_errors(A, sources):
    src, _ = sources
    good = src["4:2:0"][0]
    want = A.standard_jpeg_transform_many([good], "none", crop=BOX)
    for box in ((0, 0, 51, 37), (43, 9, 43, 30), (0, 0, 50, 38)):
        with pytest.raises(ValueError, match=r"file 1: crop .* does not lie inside the 50 x 37 image"):
            A.standard_jpeg_transform_many([good, good], "none", crop=[BOX, box])
    with pytest.raises(ValueError, match=r"file 0: crop .* does not lie inside the 48 x 32 image that rot180 with trim=True leaves"):
        A.standard_jpeg_transform_many([good], "rot180", trim=True, crop=(0, 0, 49, 32))
    with pytest.raises(ValueError, match="file 1: 1 crop boxes for 2 files"):
        A.standard_jpeg_transform_many([good, good], "none", crop=[BOX])
    with pytest.raises(TypeError, match="drop_chroma"):
        A.standard_jpeg_transform_many([good], "none", drop_chroma=1)
    # the status protocol of the bridge, through the cut: a coefficient libjpeg's coder cannot hold, and a truncated scan
    bad = TT._one_block_file(3, 1024)
    for kw in (dict(drop_chroma=True), dict(crop=[BOX, (0, 0, 5, 5)])):
        with pytest.raises(ValueError, match=r"file 1: coefficient out of range"):
            A.standard_jpeg_transform_many([good, bad], "none", **kw)
    short = good[:good.index(b"\xff\xda") + 14 + 40]
    with pytest.raises(ValueError, match=r"file 1: truncated scan"):
        A.standard_jpeg_transform_many([good, short], "none", crop=BOX)
    assert A.standard_jpeg_transform_many([good], "none", crop=BOX) == want      # the device goes on working
