"""GPU: restart markers in the progressive files (csrc/jfifprog.hip over csrc/jfif_restart_core.h): every scan has its own interval, a
DRI where it changes, end-of-band runs and deferred correction bits flushed at every restart.  The inputs are those of
tests/test_gpu_jfif_restart.py; the yardstick is Pillow's live save(progressive=True) with the same keywords, byte for byte, and every
output is decoded by this library's progressive decoder and compared with Pillow's pixels."""
import io
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_restart_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ["4:4:4", "4:2:2", "4:2:0", "L"]
OPTIONS = [dict(restart_marker_rows=1), dict(restart_marker_blocks=5), dict(restart_marker_blocks=100), dict(restart_marker_rows=5),
           dict(restart_marker_rows=1, restart_marker_blocks=3)]


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _pil(x, kind, q=75, **kw):
    kw["progressive"] = True
    return RR.pil_save(x[:, :, 0], q, **kw) if kind == "L" else RR.pil_save(x, q, subsampling=kind, **kw)


def _ours(A, x, kind, q=75, **kw):
    if kind == "L":
        return A.standard_jpeg_encode_many([x[:, :, 0]], q, mode="L", progressive=True, **kw)[0]
    return A.standard_jpeg_encode_many([x], q, subsampling=kind, progressive=True, **kw)[0]


def _same(A, ours, want):
    RR.same_files_and_pixels(A, ours, want, progressive=True)


@pytest.mark.parametrize("kind", ["4:4:4", "4:2:0", "L"])
def test_noise_flushes_deferred_correction_bits_at_restarts(A, kind):
    x = RR.noise()
    want = _pil(x, kind, 100, restart_marker_blocks=1)
    assert all(len(m) > 8 for m in RR.markers(want))                     # every scan's numbering wraps
    _same(A, [_ours(A, x, kind, 100, restart_marker_blocks=1)], [want])


def test_flat_image(A):
    x = RR.flat()
    _same(A, [_ours(A, x, "4:4:4", 75, restart_marker_blocks=1)], [_pil(x, "4:4:4", 75, restart_marker_blocks=1)])


@pytest.mark.parametrize("opt", [dict(restart_marker_blocks=2), dict(restart_marker_rows=1)], ids=str)
@pytest.mark.parametrize("kind", ["4:2:0", "4:4:4", "L"])
def test_long_end_of_band_runs_are_cut_at_every_restart(A, kind, opt):
    x = RR.spike()
    _same(A, [_ours(A, x, kind, **opt)], [_pil(x, kind, **opt)])


@pytest.mark.parametrize("kind", KINDS)
def test_partial_mcus(A, kind):
    x = RR.gradient(40, 56)
    want = [_pil(x, kind, **opt) for opt in OPTIONS]
    if kind == "4:2:0":                                                  # the issue's example: the ten scans' DRI under rows = 1
        assert RR.dri_sequence(want[0]) == [4, 7, 4, None, 7, None, 4, None, None, 7]
    _same(A, [_ours(A, x, kind, **opt) for opt in OPTIONS], want)
    assert not any(RR.dri_sequence(_ours(A, x, kind)))                   # both 0: no DRI


def test_mixed_sizes_in_one_call(A):
    sizes = [(40, 56), (64, 64), (8, 8), (9, 200)]
    images = [RR.gradient(h, w, 7 + i) for i, (h, w) in enumerate(sizes)]
    images += [x[:, :, 1].copy() for x in images]
    kw = dict(subsampling="4:2:0", progressive=True, mode="auto")
    A.standard_jpeg_encode_many(images, 80, **kw)
    groups = A.encode_groups()
    got = A.standard_jpeg_encode_many(images, 80, restart_marker_rows=1, **kw)
    assert A.encode_groups() == groups == 8
    assert got == [A.standard_jpeg_encode_many([x], 80, restart_marker_rows=1, **kw)[0] for x in images]
    _same(A, got, [RR.pil_save(x, 80, progressive=True, restart_marker_rows=1, **({} if x.ndim == 2 else {"subsampling": "4:2:0"})) for x in images])


def test_thumbnails(A):
    from PIL import Image
    files = [RR.pil_save(RR.gradient(120, 168, 21), 90), RR.pil_save(RR.gradient(96, 96, 22), 85, subsampling="4:4:4")]
    got = A.standard_jpeg_thumbnail_jpeg_many(files, (64, 40), quality=80, progressive_out=True, restart_marker_rows=1)
    want = []
    for f in files:
        im = Image.open(io.BytesIO(f))
        im.thumbnail((64, 40), Image.BICUBIC, reducing_gap=2.0)
        want.append(RR.pil_save(im, 80, subsampling="4:2:0", progressive=True, restart_marker_rows=1))
    _same(A, got, want)


SOURCES = [dict(), dict(optimize=True), dict(progressive=True), dict(restart_marker_blocks=1), dict(restart_marker_rows=1)]


@pytest.mark.parametrize("opt", [dict(restart_marker_rows=1), dict(restart_marker_blocks=2)], ids=str)
def test_transcoder(A, opt):
    images = [RR.gradient(40, 56), RR.noise()]
    colour = [RR.pil_save(x, 75, subsampling="4:2:0", **src) for x in images for src in SOURCES]
    grey = [RR.pil_save(x[:, :, 0], 75, **src) for x in images for src in SOURCES]
    want = [RR.pil_save(x, 75, subsampling="4:2:0", progressive=True, **opt) for x in images for _ in SOURCES]
    want += [RR.pil_save(x[:, :, 0], 75, progressive=True, **opt) for x in images for _ in SOURCES]
    got = A.standard_jpeg_transcode_many(colour + grey, progressive=True, grey=True, **opt)
    _same(A, got, want)
    plain = A.standard_jpeg_transcode_many(colour + grey, progressive=True, grey=True)
    assert all(RR.dri_sequence(f) == [None] * len(RR.dri_sequence(f)) and not any(RR.markers(f)) for f in plain)
    assert A.standard_jpeg_transcode_many(got, progressive=True, grey=True) == plain


def test_transforms(A):
    x = RR.gradient(32, 48)
    src = RR.pil_save(x, 75, subsampling="4:2:0")
    for name in ("rot90", "flip_h"):
        (plain,) = A.standard_jpeg_transform_many([src], name, progressive=True)
        (got,) = A.standard_jpeg_transform_many([src], name, progressive=True, restart_marker_rows=1)
        assert [got] == A.standard_jpeg_transcode_many([plain], progressive=True, restart_marker_rows=1) and any(RR.markers(got))
        _same(A, [got], [got])
