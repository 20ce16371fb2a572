"""GPU: box= of standard_jpeg_decode_many (csrc/jpegdec.hip: k_jd_box, the segment skip, the coefficient window).  Everything is exact
equality against two references: this package's own decode without box=, sliced -- which the other decoder tests pin to Pillow -- and
live Pillow's crop(), asked where its libjpeg-turbo is the one that made the luma fixtures (the gate of test_gpu_jpeg_luma.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

import jpegdec_box_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
N_COPIES = 150


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def live():
    from PIL import features
    with open(os.path.join(GOLDEN, "jpeg_luma", "meta.json")) as f:
        return features.version("libjpeg_turbo") == json.load(f)["libjpeg_turbo"]


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), what


def _crop(a, box):
    l, t, r, b = box
    return a[t:b, l:r]


KW = dict(progressive=True, layout_440=True)
_pairs = {}


def _pair(layout, W=83, H=61):
    """the baseline and the progressive save of one picture"""
    if (layout, W, H) not in _pairs:
        _pairs[layout, W, H] = [R.make_file(layout, W, H, progressive=p) for p in (False, True)]
    return _pairs[layout, W, H]


def _boxes_83x61():
    forced = R.forced_boxes(83, 61)
    return forced + R.random_boxes(83, 61, N_COPIES - len(forced), 20261019)


# ---- 1. layouts x boxes: one call per layout and mode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["RGB", "L"])
@pytest.mark.parametrize("layout", [l[0] for l in R.LAYOUTS])
def test_layouts_and_boxes(A, live, layout, mode):
    pair, boxes = _pair(layout), _boxes_83x61()
    assert len(boxes) == N_COPIES
    files = [pair[k & 1] for k in range(N_COPIES)]
    whole = _np(A.standard_jpeg_decode_many(pair, mode=mode, **KW))
    got = _np(A.standard_jpeg_decode_many(files, mode=mode, box=boxes, **KW))
    pil = [np.asarray(R.pil_rgb(f) if mode == "RGB" else R.pil_l(f)) for f in pair] if live else None
    for k, (g, box) in enumerate(zip(got, boxes)):
        _same(g, _crop(whole[k & 1], box), (layout, mode, k, box))
        if live:
            _same(g, _crop(pil[k & 1], box), ("pillow", layout, mode, k, box))
    if live:                                                 # Pillow's own crop(), not a slice of its pixels, for the forced boxes
        ims = [R.pil_rgb(f) if mode == "RGB" else R.pil_l(f) for f in pair]
        for k, box in enumerate(R.forced_boxes(83, 61)):
            _same(got[k], np.asarray(ims[k & 1].crop(box)), ("crop()", layout, mode, box))


def test_mode_auto_grey_and_colour_mixed(A):
    boxes = _boxes_83x61()[:40]
    layouts = ["grey", "420", "444", "grey", "422", "440"]
    files = [_pair(layouts[k % 6])[k & 1] for k in range(len(boxes))]
    whole = _np(A.standard_jpeg_decode_many(files, mode="auto", **KW))
    got = _np(A.standard_jpeg_decode_many(files, mode="auto", box=boxes, **KW))
    for k, (g, w, box) in enumerate(zip(got, whole, boxes)):
        assert g.ndim == (2 if layouts[k % 6] == "grey" else 3)
        _same(g, _crop(w, box), (k, box))


# ---- 2. narrow planes: the replication rule (chroma <= 2 wide) beside the fancy one (3 wide) ---------------------------------------------
@pytest.mark.parametrize("layout", ["420", "422"])
def test_narrow_planes_every_box(A, layout):
    files, boxes, src = [], [], []
    pairs = [_pair(layout, W, H) for W, H in R.NARROW]
    whole = [_np(A.standard_jpeg_decode_many(p, **KW)) for p in pairs]
    for s, (W, H) in enumerate(R.NARROW):
        for k, box in enumerate(R.all_boxes(W, H)):
            files.append(pairs[s][k & 1]); boxes.append(box); src.append((s, k & 1))
    got = _np(A.standard_jpeg_decode_many(files, box=boxes, **KW))
    for g, box, (s, p) in zip(got, boxes, src):
        _same(g, _crop(whole[s][p], box), (layout, R.NARROW[s], box))


# ---- 3. boxed and unboxed entries, kinds and layouts mixed in one call -------------------------------------------------------------------
def test_mixed_call(A):
    files = [_pair("420")[0], _pair("444")[1], _pair("grey")[0], _pair("440")[1], _pair("422")[0], _pair("420")[1], _pair("grey")[1],
             _pair("420", 96, 80)[0]]
    boxes = [(5, 7, 70, 50), None, (0, 0, 83, 61), (16, 16, 17, 60), None, (33, 1, 83, 2), (1, 1, 2, 2), (0, 36, 96, 44)]
    modes = ["RGB", "L", "auto", "RGB", "RGB", "L", "RGB", "auto"]
    whole = A.standard_jpeg_decode_many(files, mode=modes, **KW)
    got = A.standard_jpeg_decode_many(files, mode=modes, box=boxes, **KW)
    off = 0
    for k, (g, w, box) in enumerate(zip(got, whole, boxes)):
        want = w.cpu().numpy() if box is None else _crop(w.cpu().numpy(), box)
        _same(g.cpu().numpy(), want, (k, box))
        assert g.data_ptr() == got[0].data_ptr() + off, k    # views into one packed allocation, in input order
        off += g.numel()


# ---- 4. restart segments outside the window are skipped ----------------------------------------------------------------------------------
def _rst_file(A, **kw):
    return A.standard_jpeg_encode_many([R.picture(80, 96)], 90, "4:2:0", **kw)[0]


def test_restart_skip(A):
    rows = _rst_file(A, restart_marker_rows=1)
    (whole,) = _np(A.standard_jpeg_decode_many([rows]))
    for box, stats in (((0, 36, 96, 44), (5, 1, 1 * 6 * 6)), ((0, 32, 96, 48), (5, 3, 3 * 6 * 6)), ((40, 36, 41, 37), (5, 1, 36)),
                       ((0, 0, 96, 1), (5, 1, 36)), ((95, 79, 96, 80), (5, 1, 36))):
        (g,) = _np(A.standard_jpeg_decode_many([rows], box=box))
        _same(g, _crop(whole, box), box)
        assert A.decode_box_stats() == stats, box
    blocks = _rst_file(A, restart_marker_blocks=2)           # 15 segments of 2 MCUs, 6 MCUs a row: rows 36 .. 44 are MCUs 12 .. 17
    (whole2,) = _np(A.standard_jpeg_decode_many([blocks]))
    (g,) = _np(A.standard_jpeg_decode_many([blocks], box=(0, 36, 96, 44)))
    _same(g, _crop(whole2, (0, 36, 96, 44)), "2-MCU segments")
    assert A.decode_box_stats() == (15, 3, 36)
    (g,) = _np(A.standard_jpeg_decode_many([blocks], box=(0, 36, 96, 44), mode="L"))
    _same(g, _crop(_np(A.standard_jpeg_decode_many([blocks], mode="L"))[0], (0, 36, 96, 44)), "2-MCU segments, L")
    got = _np(A.standard_jpeg_decode_many([rows, blocks, rows], box=[(0, 36, 96, 44), None, (0, 32, 96, 48)]))      # summed over the call's files
    _same(got[1], whole2, "unboxed beside boxed")
    assert A.decode_box_stats() == (5 + 15 + 5, 1 + 15 + 3, 36 + 5 * 36 + 3 * 36)


# ---- 5. a bad segment the box does not need goes unnoticed; one it needs is reported ----------------------------------------------------
def _flip_in_segment(data, A, g):
    """one byte changed inside restart segment g of a file with one marker per MCU row: neither it nor its neighbours are or become
    0xFF, so the marker count stands"""
    d = A.standard_jpeg.parse_header(data)
    marks = [i for i in range(d.scan_offset, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(marks) == 4
    lo = d.scan_offset if g == 0 else marks[g - 1] + 2
    hi = marks[g] if g < 4 else len(data) - 2
    for p in range(lo + (hi - lo) // 3, hi - 2):
        new = data[p] ^ 0x55
        if 0xFF not in (data[p - 1], data[p], data[p + 1], new):
            return data[:p] + bytes([new]) + data[p + 1:]
    raise AssertionError("no byte to change")


def test_bad_segment_outside_the_window(A):
    good = _rst_file(A, restart_marker_rows=1)
    (whole,) = _np(A.standard_jpeg_decode_many([good]))
    box = (0, 36, 96, 44)
    bad4 = _flip_in_segment(good, A, 4)
    try:
        (other,) = _np(A.standard_jpeg_decode_many([bad4]))
        assert not np.array_equal(other, whole)
    except ValueError as e:
        assert "file 0" in str(e)
    (g,) = _np(A.standard_jpeg_decode_many([bad4], box=box))
    _same(g, _crop(whole, box), "the bad segment is not read")
    bad2 = _flip_in_segment(good, A, 2)                      # the segment the box needs
    with pytest.raises(ValueError, match="file 1"):
        A.standard_jpeg_decode_many([good, bad2], box=[None, box])
    d = A.standard_jpeg.parse_header(good)
    marks = [i for i in range(d.scan_offset, len(good) - 1) if good[i] == 0xFF and 0xD0 <= good[i + 1] <= 0xD7]
    short2 = good[:marks[1] + 6] + good[marks[2]:]           # that segment cut down to four bytes: 36 blocks cannot be in them
    with pytest.raises(ValueError, match="file 0"):
        A.standard_jpeg_decode_many([short2], box=box)
    (g,) = _np(A.standard_jpeg_decode_many([short2], box=(0, 0, 96, 8)))      # ... which a box in MCU row 0 does not read
    _same(g, _crop(whole, (0, 0, 96, 8)), "the short segment is not read")


# ---- 6. no restart markers: the write pass stops after the window --------------------------------------------------------------------------
def test_truncated_file_without_markers(A):
    good = R.make_file("420", 96, 80)
    d = A.standard_jpeg.parse_header(good)
    cut = good[:d.scan_offset + (len(good) - 2 - d.scan_offset) * 7 // 10]
    with pytest.raises(ValueError, match="file 0.*(?i:truncated)"):
        A.standard_jpeg_decode_many([cut])
    (whole,) = _np(A.standard_jpeg_decode_many([good]))
    for box in ((0, 0, 96, 8), (90, 3, 96, 4)):
        (g,) = _np(A.standard_jpeg_decode_many([cut], box=box))
        _same(g, _crop(whole, box), box)
        assert A.decode_box_stats() == (1, 1, 6 * 6)
    with pytest.raises(ValueError, match="file 0"):
        A.standard_jpeg_decode_many([cut], box=(0, 70, 96, 80))      # the rows the cut took away


# ---- 7. the C entry: refusals before any device work, workspace sizes ----------------------------------------------------------------------
def _c_call(A, data, scale, box, out):
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc, get_context
    import torch
    ctx = get_context(0)
    lib = ctx.lib
    d = A.standard_jpeg.parse_header(data)
    descs = (JpegDecDesc * 1)(d)
    scan = torch.frombuffer(bytearray(data[d.scan_offset:d.scan_offset + d.scan_length]), dtype=torch.uint8).cuda()
    sc, bx = (ctypes.c_int * 1)(scale), (ctypes.c_int32 * 4)(*box)
    so, oo = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(0)
    status = torch.full((1,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")      # 0xA5 bytes: the entry clears its status words itself
    nws = int(lib.aej_jpegdec_workspace_bytes_mode(ctx.handle, ctypes.addressof(descs), 1, None, None))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    return lib.aej_jpegdec_batch_box(ctx.handle, ctypes.addressof(descs), 1, ctypes.addressof(sc), None, ctypes.addressof(bx), scan.data_ptr(),
                                     ctypes.c_uint64(scan.numel()), ctypes.addressof(so), out.data_ptr(), ctypes.c_uint64(out.numel()),
                                     ctypes.addressof(oo), status.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws))


def test_c_entry_refusals_leave_the_output_untouched(A):
    import torch
    data = _pair("420")[0]
    pattern = (torch.arange(83 * 61 * 3, device="cuda") % 251).to(torch.uint8)
    out = pattern.clone()
    assert _c_call(A, data, 2, (0, 0, 8, 8), out) == -5      # AEJ_ERR_UNSUPPORTED: a box at scale 2
    torch.cuda.synchronize()
    assert torch.equal(out, pattern)
    for bad in ((0, 0, 84, 61), (0, 0, 83, 62), (-1, 0, 8, 8), (8, 8, 8, 9), (9, 8, 8, 9)):
        assert _c_call(A, data, 1, bad, out) == -1, bad      # AEJ_ERR_ARG
        torch.cuda.synchronize()
        assert torch.equal(out, pattern)
    half = pattern.clone()
    assert _c_call(A, data, 2, (0, 0, 83, 61), half) == 0    # the whole image is no box: the scaled decode
    torch.cuda.synchronize()
    _same(half[:42 * 31 * 3].view(31, 42, 3).cpu().numpy(), _np(A.standard_jpeg_decode_many([data], scale=2))[0], "no box at scale 2")
    assert _c_call(A, data, 1, (3, 5, 30, 40), out) == 0
    torch.cuda.synchronize()
    (whole,) = _np(A.standard_jpeg_decode_many([data]))
    _same(out[:27 * 35 * 3].view(35, 27, 3).cpu().numpy(), whole[5:40, 3:30], "the C entry's box")
    assert torch.equal(out[27 * 35 * 3:], pattern[27 * 35 * 3:])


def test_workspace_shrinks_with_the_box(A):
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc, JpegProgFrame, JpegProgScan, get_context
    ctx = get_context(0)
    lib = ctx.lib
    base, prog = (R.make_file("420", 256, 256, progressive=p) for p in (False, True))
    descs = (JpegDecDesc * 1)(A.standard_jpeg.parse_header(base))
    full = int(lib.aej_jpegdec_workspace_bytes_mode(ctx.handle, ctypes.addressof(descs), 1, None, None))
    assert full > 0 and int(lib.aej_jpegdec_workspace_bytes_box(ctx.handle, ctypes.addressof(descs), 1, None, None, None)) == full
    whole = (ctypes.c_int32 * 4)(0, 0, 256, 256)
    assert int(lib.aej_jpegdec_workspace_bytes_box(ctx.handle, ctypes.addressof(descs), 1, None, None, ctypes.addressof(whole))) == full
    inside = (ctypes.c_int32 * 4)(129, 129, 142, 142)        # inside one MCU, its chroma neighbours too
    assert A.decode_box_window(256, 256, 2, 2, 3, tuple(inside)) == (8, 8, 9, 9)
    small = int(lib.aej_jpegdec_workspace_bytes_box(ctx.handle, ctypes.addressof(descs), 1, None, None, ctypes.addressof(inside)))
    planes, coefs = 256 * 256 * 3 // 2, 15 * 16 * 6 * 128    # what a boxed file does not have: sample planes, 15 of 16 MCU rows of coefficients
    assert 0 < small <= full - planes - coefs
    outside = (ctypes.c_int32 * 4)(0, 0, 257, 256)
    assert int(lib.aej_jpegdec_workspace_bytes_box(ctx.handle, ctypes.addressof(descs), 1, None, None, ctypes.addressof(outside))) == 0
    two = (ctypes.c_int * 1)(2)
    assert int(lib.aej_jpegdec_workspace_bytes_box(ctx.handle, ctypes.addressof(descs), 1, ctypes.addressof(two), None, ctypes.addressof(inside))) == 0
    frame, scans = A.standard_jpeg.parse_scans(prog)
    frames, arr = (JpegProgFrame * 1)(frame), (JpegProgScan * len(scans))(*scans)
    head = (ctx.handle, ctypes.addressof(frames), ctypes.addressof(arr), 1, None, None)
    pfull = int(lib.aej_jpegprog_workspace_bytes_mode(*head))
    assert int(lib.aej_jpegprog_workspace_bytes_box(*head, None)) == pfull
    psmall = int(lib.aej_jpegprog_workspace_bytes_box(*head, ctypes.addressof(inside)))
    assert 0 < psmall <= pfull - planes                      # a progressive file keeps its coefficients
    assert int(lib.aej_jpegprog_workspace_bytes_box(*head, ctypes.addressof(outside))) == 0
