"""GPU: restart markers (restart_marker_blocks= / restart_marker_rows=) in the baseline files of standard_jpeg_encode_many,
standard_jpeg_thumbnail_jpeg_many, standard_jpeg_transcode_many and standard_jpeg_transform_many (csrc/jfif.hip over
csrc/jfif_restart_core.h).  The yardstick is Pillow's live save with the same keywords, byte for byte; every output is also decoded by
this library's decoder and compared with Pillow's pixels.  The progressive files are tests/test_gpu_jfif_restart_progressive.py."""
import io
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_restart_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ["4:4:4", "4:2:2", "4:2:0", "L"]
PADDED_FF_BEFORE_MARKER = re.compile(rb"\xff\x00\xff[\xd0-\xd7]")
OPTIONS = [dict(restart_marker_rows=1), dict(restart_marker_blocks=5), dict(restart_marker_blocks=100), dict(restart_marker_rows=5),
           dict(restart_marker_rows=1, restart_marker_blocks=3)]


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _pil(x, kind, q=75, **kw):
    return RR.pil_save(x[:, :, 0], q, **kw) if kind == "L" else RR.pil_save(x, q, subsampling=kind, **kw)


def _ours(A, x, kind, q=75, **kw):
    if kind == "L":
        return A.standard_jpeg_encode_many([x[:, :, 0]], q, mode="L", **kw)[0]
    return A.standard_jpeg_encode_many([x], q, subsampling=kind, **kw)[0]


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("kind", ["4:4:4", "4:2:0", "L"])
def test_noise_pads_to_ff_before_a_marker_and_the_numbers_wrap(A, kind, optimize):
    x = RR.noise()
    want = _pil(x, kind, 100, optimize=optimize, restart_marker_blocks=1)
    assert PADDED_FF_BEFORE_MARKER.search(want)                          # a padded byte that had to be stuffed directly before a marker
    (found,) = RR.markers(want)
    assert len(found) > 8 and found[:9] == [0xD0 + (k & 7) for k in range(9)]
    RR.same_files_and_pixels(A, [_ours(A, x, kind, 100, optimize=optimize, restart_marker_blocks=1)], [want])


def test_flat_image_has_dozens_of_boundaries_in_one_chunk(A):
    x = RR.flat()
    want = _pil(x, "4:4:4", 75, restart_marker_blocks=1)
    assert len(want) == 949 and len(RR.markers(want)[0]) == 63
    RR.same_files_and_pixels(A, [_ours(A, x, "4:4:4", 75, restart_marker_blocks=1)], [want])


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_partial_mcus(A, kind, optimize):
    x = RR.gradient(40, 56)
    ours = [_ours(A, x, kind, optimize=optimize, **opt) for opt in OPTIONS]
    want = [_pil(x, kind, optimize=optimize, **opt) for opt in OPTIONS]
    if kind == "4:2:0":                                                  # a 4 x 3 MCU grid: rows of 4; 5, 5, 2; a DRI and no marker, twice; rows win
        assert RR.dri_sequence(want[0]) == [4] and RR.dri_sequence(want[1]) == [5] and RR.dri_sequence(want[4]) == [4]
        assert [len(RR.markers(f)[0]) for f in want] == [2, 2, 0, 0, 2]
    RR.same_files_and_pixels(A, ours, want)
    assert b"\xff\xdd" not in RR.header_until_sos(_ours(A, x, kind, optimize=optimize))      # both 0: no DRI


@pytest.mark.parametrize("optimize", [False, True])
def test_mixed_sizes_in_one_call(A, optimize):
    sizes = [(40, 56), (64, 64), (8, 8), (9, 200)]
    images = [RR.gradient(h, w, 7 + i) for i, (h, w) in enumerate(sizes)]
    images += [x[:, :, 1].copy() for x in images]                        # the same sizes, grey
    kw = dict(subsampling="4:2:0", optimize=optimize, mode="auto")
    A.standard_jpeg_encode_many(images, 80, **kw)
    groups = A.encode_groups()
    got = A.standard_jpeg_encode_many(images, 80, restart_marker_rows=1, **kw)
    assert A.encode_groups() == groups == 8
    alone = [A.standard_jpeg_encode_many([x], 80, restart_marker_rows=1, **kw)[0] for x in images]
    assert got == alone
    want = [RR.pil_save(x, 80, optimize=optimize, restart_marker_rows=1, **({} if x.ndim == 2 else {"subsampling": "4:2:0"})) for x in images]
    RR.same_files_and_pixels(A, got, want)
    assert RR.dri_sequence(got[2]) == [1] and RR.markers(got[2]) == [[]]  # one MCU: the DRI alone


def test_thumbnails(A):
    from PIL import Image
    files = [RR.pil_save(RR.gradient(120, 168, 21), 90), RR.pil_save(RR.gradient(96, 96, 22), 85, subsampling="4:4:4")]
    got = A.standard_jpeg_thumbnail_jpeg_many(files, (64, 40), quality=80, restart_marker_rows=1)
    want = []
    for f in files:
        im = Image.open(io.BytesIO(f))
        im.thumbnail((64, 40), Image.BICUBIC, reducing_gap=2.0)
        want.append(RR.pil_save(im, 80, subsampling="4:2:0", restart_marker_rows=1))
    assert all(len(RR.markers(f)[0]) > 0 for f in want)
    RR.same_files_and_pixels(A, got, want)


SOURCES = [dict(), dict(optimize=True), dict(progressive=True), dict(restart_marker_blocks=1), dict(restart_marker_rows=1)]


@pytest.mark.parametrize("opt", [dict(restart_marker_rows=1), dict(restart_marker_blocks=2)], ids=str)
def test_transcoder(A, opt):
    images = [RR.gradient(40, 56), RR.noise()]
    colour = [RR.pil_save(x, 75, subsampling="4:2:0", **src) for x in images for src in SOURCES]
    grey = [RR.pil_save(x[:, :, 0], 75, **src) for x in images for src in SOURCES]
    want = [RR.pil_save(x, 75, subsampling="4:2:0", optimize=True, **opt) for x in images for _ in SOURCES]
    want += [RR.pil_save(x[:, :, 0], 75, optimize=True, **opt) for x in images for _ in SOURCES]
    got = A.standard_jpeg_transcode_many(colour + grey, grey=True, **opt)
    RR.same_files_and_pixels(A, got, want)
    # a source's own markers are never carried over, and the closure: back with 0, 0 is the plain transcode
    plain = A.standard_jpeg_transcode_many(colour + grey, grey=True)
    assert all(b"\xff\xdd" not in RR.header_until_sos(f) and RR.markers(f) == [[]] for f in plain)
    assert A.standard_jpeg_transcode_many(got, grey=True) == plain


def test_transcoder_keeps_metadata_around_the_dri(A):
    x = RR.gradient(40, 56)
    src = RR.pil_save(x, 75, subsampling="4:2:0", comment=b"a comment", icc_profile=b"\x01\x02" * 100)
    (bare,) = A.standard_jpeg_transcode_many([src], restart_marker_rows=1)
    (kept,) = A.standard_jpeg_transcode_many([src], restart_marker_rows=1, keep_metadata=True)
    meta = A.standard_jpeg.metadata_segments(src)
    assert len(meta) > 200 and kept == A.standard_jpeg.splice_metadata(bare, meta)
    segs = [m for m, _, _ in RR.walk(kept)]
    assert segs[segs.index(0xDA) - 1] == 0xDD and RR.dri_sequence(kept) == [4]
    assert bare == RR.pil_save(x, 75, subsampling="4:2:0", optimize=True, restart_marker_rows=1)
    RR.same_files_and_pixels(A, [kept], [kept])


def test_transforms(A):
    from PIL import Image
    x = RR.gradient(32, 48)
    src = RR.pil_save(x, 75, subsampling="4:2:0")
    for name in ("rot90", "flip_h"):
        (plain,) = A.standard_jpeg_transform_many([src], name)
        (got,) = A.standard_jpeg_transform_many([src], name, restart_marker_rows=1)
        assert b"\xff\xdd" not in RR.header_until_sos(plain)
        assert [got] == A.standard_jpeg_transcode_many([plain], restart_marker_rows=1) and len(RR.markers(got)[0]) > 0
        RR.same_files_and_pixels(A, [got], [got])
    e = Image.Exif()
    e[0x0112] = 6
    tagged = RR.pil_save(x, 75, subsampling="4:2:0", exif=e.tobytes())
    assert A.exif_orientation(tagged) == 6
    (plain,) = A.standard_jpeg_transform_many([tagged], "exif")
    (got,) = A.standard_jpeg_transform_many([tagged], "exif", restart_marker_rows=1)
    assert plain == A.standard_jpeg_transform_many([src], "rot90")[0]
    assert [got] == A.standard_jpeg_transcode_many([plain], restart_marker_rows=1)
    assert RR.dri_sequence(got) == [2]                                   # the OUTPUT is 48 x 32 (H x W): two MCUs per row
