"""GPU: scaled_box= of standard_jpeg_decode_many (csrc/jpegdec.hip: k_jd_sbox, with the segment skip and the coefficient window of box=),
the source window of the resampler (aej_resample_batch_win) and standard_jpeg_resized_crop_many, which joins the two.  Everything is
exact equality: against this package's own calls without the new keyword, sliced or composed -- which the other tests pin to Pillow --
and against live Pillow where its libjpeg-turbo is the one that made the luma fixtures (the gate of test_gpu_jpegdec_box.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

import jpegdec_box_reference as R
import jpegdec_sbox_reference as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
N_COPIES = 150
FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")
KW = dict(progressive=True, layout_440=True)


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


_pairs = {}


def _pair(layout, W=83, H=61):
    """the baseline and the progressive save of one picture"""
    if (layout, W, H) not in _pairs:
        _pairs[layout, W, H] = [R.make_file(layout, W, H, progressive=p) for p in (False, True)]
    return _pairs[layout, W, H]


def _mcu(layout, s):
    _, hs, vs, ncomp = next(l for l in S.LAYOUTS if l[0] == layout)
    m = 8 // s
    return (hs * m, vs * m) if ncomp == 3 else (m, m)


# ---- 1. layouts x scales x boxes: one call per case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["RGB", "L"])
@pytest.mark.parametrize("s", S.SCALES)
@pytest.mark.parametrize("layout", [l[0] for l in S.LAYOUTS])
def test_layouts_scales_and_boxes(A, live, layout, s, mode):
    pair = _pair(layout)
    ow, oh = S.scaled_size(83, 61, s)
    boxes = S.boxes_for(ow, oh, *_mcu(layout, s), N_COPIES, 20261019 + s)
    assert len(boxes) == N_COPIES and boxes[0] == (0, 0, ow, oh)
    files = [pair[k & 1] for k in range(N_COPIES)]
    whole = _np(A.standard_jpeg_decode_many(pair, scale=s, mode=mode, **KW))
    assert whole[0].shape[:2] == (oh, ow)
    got = _np(A.standard_jpeg_decode_many(files, scale=s, mode=mode, scaled_box=boxes, **KW))
    ims = [S.pil_drafted(f, mode, s) for f in pair] if live else None
    pil = [np.asarray(im) for im in ims] if live else None
    for k, (g, box) in enumerate(zip(got, boxes)):
        _same(g, _crop(whole[k & 1], box), (layout, s, mode, k, box))
        if live:
            _same(g, _crop(pil[k & 1], box), ("pillow", layout, s, mode, k, box))
    if live:                                                 # Pillow's own crop() of the drafted image for the forced boxes
        for k, box in enumerate(S.forced_boxes(ow, oh, *_mcu(layout, s))):
            _same(got[k], np.asarray(ims[k & 1].crop(box)), ("crop()", layout, s, mode, box))


# ---- 2. narrow files: replication beside the fancy rule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("layout", ["422", "420"])
def test_narrow_files_every_box(A, layout, s):
    files, boxes, src = [], [], []
    pairs = [_pair(layout, W, H) for W, H in R.NARROW]
    whole = [_np(A.standard_jpeg_decode_many(p, scale=s, **KW)) for p in pairs]
    for q, (W, H) in enumerate(R.NARROW):
        for k, box in enumerate(S.all_boxes(*S.scaled_size(W, H, s))):
            files.append(pairs[q][k & 1]); boxes.append(box); src.append((q, k & 1))
    got = _np(A.standard_jpeg_decode_many(files, scale=s, scaled_box=boxes, **KW))
    for g, box, (q, p) in zip(got, boxes, src):
        _same(g, _crop(whole[q][p], box), (layout, s, R.NARROW[q], box))


# ---- 3. more than one tile both ways: 1100 x 300 is 138 x 38 at scale 8, tiles are 128 x 32 scaled pixels ----------------------------------------
@pytest.mark.parametrize("layout", [l[0] for l in S.LAYOUTS])
def test_more_than_one_tile(A, layout):
    data = R.make_file(layout, 1100, 300)
    files, scales, boxes = [], [], []
    for s in S.SCALES:
        ow, oh = S.scaled_size(1100, 300, s)
        assert ow > 128 and oh > 32
        for box in ((5, 3, 135, 37), (1, 1, ow - 1, oh - 1), (40, 10, 60, 20)):      # across a tile corner; all but the rim; inside one tile
            files.append(data); scales.append(s); boxes.append(box)
    whole = dict(zip(S.SCALES, _np(A.standard_jpeg_decode_many([data] * 3, scale=list(S.SCALES), layout_440=True))))
    got = _np(A.standard_jpeg_decode_many(files, scale=scales, scaled_box=boxes, layout_440=True))
    for g, s, box in zip(got, scales, boxes):
        _same(g, _crop(whole[s], box), (layout, s, box))


# ---- 4. the segment skip carries over ------------------------------------------------------------------------------------------------------------
def test_restart_skip_at_scale_4(A):
    rows = A.standard_jpeg_encode_many([R.picture(80, 96)], 90, "4:2:0", restart_marker_rows=1)[0]      # 6 x 5 MCUs, 5 segments
    (whole,) = _np(A.standard_jpeg_decode_many([rows], scale=4))
    assert whole.shape == (20, 24, 3)
    for box in ((0, 9, 24, 11), (3, 4, 10, 8), (0, 0, 24, 1), (23, 19, 24, 20), (0, 3, 24, 5)):
        win = A.decode_box_window(96, 80, 2, 2, 3, box, scale=4)
        nrows = win[3] - win[1]
        assert nrows == (2 if box == (0, 3, 24, 5) else 1)
        (g,) = _np(A.standard_jpeg_decode_many([rows], scale=4, scaled_box=box))
        _same(g, _crop(whole, box), box)
        assert A.decode_box_stats() == (5, nrows, nrows * 6 * 6), box      # segments decoded, blocks stored: what the window predicts


# ---- 5. scale 1 is box=; the whole scaled image is no box ---------------------------------------------------------------------------------------
def test_scale_1_and_whole_image(A):
    files = [_pair("420")[0], _pair("422")[1], _pair("grey")[0], _pair("440")[1]]
    boxes = [(5, 7, 70, 50), (16, 16, 17, 60), None, (33, 1, 83, 2)]
    for g, w in zip(_np(A.standard_jpeg_decode_many(files, scaled_box=boxes, **KW)), _np(A.standard_jpeg_decode_many(files, box=boxes, **KW))):
        _same(g, w, "scale 1")
    for s in S.SCALES:
        ow, oh = S.scaled_size(83, 61, s)
        for g, w in zip(_np(A.standard_jpeg_decode_many(files, scale=s, scaled_box=(0, 0, ow, oh), **KW)),
                        _np(A.standard_jpeg_decode_many(files, scale=s, **KW))):
            _same(g, w, ("whole", s))
    mixed = _np(A.standard_jpeg_decode_many(files, scale=[1, 2, 4, 8], scaled_box=[(5, 7, 70, 50), (3, 2, 40, 30), None, (1, 1, 10, 7)], mode=["RGB", "L", "auto", "RGB"], **KW))
    plain = _np(A.standard_jpeg_decode_many(files, scale=[1, 2, 4, 8], mode=["RGB", "L", "auto", "RGB"], **KW))
    for g, w, box in zip(mixed, plain, [(5, 7, 70, 50), (3, 2, 40, 30), (0, 0, 21, 16), (1, 1, 10, 7)]):
        _same(g, _crop(w, box), ("mixed", box))


# ---- 6. the call --------------------------------------------------------------------------------------------------------------------------------
def _crop_files():
    files = [f for layout in [l[0] for l in S.LAYOUTS] for f in _pair(layout)]      # the five layouts, baseline and progressive
    files += [R.make_file("grey", 90, 70), R.make_file("420", 176, 131)]           # one more grey file; one large enough for scale 4
    dims = [(83, 61)] * 10 + [(90, 70), (176, 131)]
    return files, dims


def _crop_boxes(dims, size):
    if size == (96, 80):                                     # up-scaling a 20 x 16 box
        return [(10 + k, 10, 30 + k, 26) if k % 3 else (10.5 + k, 10.25, 30.5 + k, 26.25) for k in range(len(dims))]
    kinds = [lambda W, H: (0, 5, W // 2, H - 3), lambda W, H: (7, 0, W, H // 2), lambda W, H: (3, H // 2, W - 2, H),
             lambda W, H: (1.25, 2.5, W - 3.75, H - 1.5), lambda W, H: (0, 0, W, H), lambda W, H: (0, 0, W, 30)]
    boxes = [kinds[k % 6](W, H) for k, (W, H) in enumerate(dims)]
    boxes[11] = (2, 1, 166, 127)                             # 164 x 126 of the large file: scale 4 under reducing_gap 1.0
    boxes[4] = (0, 0, 83, 61)                                # the whole of an 83 x 61 file: scale 2 under reducing_gap 1.0
    return boxes


_decoded = {}


def _composition(A, files, boxes, size, filt, gap, mode):
    """element i by its definition: the decode at the scale the stated rule gives, then resize_many over box / s"""
    scales = [S.crop_scale(b, size, gap) for b in boxes]
    for i, s in enumerate(scales):
        if (i, s, mode) not in _decoded:
            _decoded[i, s, mode] = A.standard_jpeg_decode_many([files[i]], scale=s, mode=mode, **KW)[0]
    res = A.resize_many([_decoded[i, s, mode] for i, s in enumerate(scales)], size, filt, box=[tuple(v / s for v in b) for b, s in zip(boxes, scales)],
                        reducing_gap=gap, mode=mode)
    return scales, _np(res)


@pytest.mark.parametrize("gap", [None, 1.0, 2.0])
@pytest.mark.parametrize("size", [(32, 24), (96, 80)])
def test_resized_crop(A, live, size, gap):
    from PIL import Image
    files, dims = _crop_files()
    assert len(files) == 12
    boxes = _crop_boxes(dims, size)
    seen, reduced = set(), False
    for filt in FILTERS:
        got = A.standard_jpeg_resized_crop_many(files, boxes, size, filt, reducing_gap=gap, **KW)
        assert tuple(got.shape) == (12, size[1], size[0], 3) and got.is_contiguous()
        got = got.cpu().numpy()
        scales, want = _composition(A, files, boxes, size, filt, gap, "RGB")
        for i in range(12):
            _same(got[i], want[i], (size, gap, filt, i, boxes[i], scales[i]))
            p = A.resized_crop_plan(*dims[i], boxes[i], size, filt, gap)
            assert p["scale"] == scales[i]
            reduced |= p["factors"] != (1, 1)
            if live:
                s = scales[i]
                im = S.pil_drafted(files[i], "RGB", s).resize(size, getattr(Image.Resampling, filt.upper()), box=tuple(v / s for v in boxes[i]), reducing_gap=gap)
                _same(got[i], np.asarray(im), ("pillow", size, gap, filt, i, boxes[i], s))
        seen |= set(scales)
    if size == (32, 24):
        assert seen == {None: {1}, 1.0: {1, 2, 4}, 2.0: {1, 2}}[gap]
        assert reduced == (gap == 1.0)                       # the wide, short box of file 5: scale 1, then a reduce by (2, 1)
    else:
        assert seen == {1}


def test_resized_crop_one_box_for_all_and_luma(A, live):
    files, dims = _crop_files()
    got = A.standard_jpeg_resized_crop_many(files, (2.5, 1, 80, 59.5), (32, 24), "bilinear", reducing_gap=1.0, mode="L", **KW)
    assert tuple(got.shape) == (12, 24, 32)
    scales, want = _composition(A, files, [(2.5, 1, 80, 59.5)] * 12, (32, 24), "bilinear", 1.0, "L")
    assert set(scales) == {2}
    for i in range(12):
        _same(got[i].cpu().numpy(), want[i], ("L", i))
    if live:
        from PIL import Image
        im = S.pil_drafted(files[0], "L", 2).resize((32, 24), Image.Resampling.BILINEAR, box=(1.25, 0.5, 40.0, 29.75), reducing_gap=1.0)
        _same(got[0].cpu().numpy(), np.asarray(im), "pillow L")
    one = A.standard_jpeg_resized_crop_many(files[:2], (0, 0, 83, 61), (83, 61), **KW)      # the whole image at its own size
    for g, w in zip(one.cpu().numpy(), _np(A.standard_jpeg_decode_many(files[:2], **KW))):
        _same(g, w, "identity")


# ---- 7. the C entries ---------------------------------------------------------------------------------------------------------------------------
def _c_decode(A, entry, data, scale, box, out):
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
    return getattr(lib, entry)(ctx.handle, ctypes.addressof(descs), 1, ctypes.addressof(sc), None, ctypes.addressof(bx), scan.data_ptr(),
                               ctypes.c_uint64(scan.numel()), ctypes.addressof(so), out.data_ptr(), ctypes.c_uint64(out.numel()),
                               ctypes.addressof(oo), status.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws))


def test_c_decode_entries(A):
    import torch
    data = _pair("420")[0]
    pattern = (torch.arange(83 * 61 * 3, device="cuda") % 251).to(torch.uint8)
    out = pattern.clone()
    for bad in ((0, 0, 43, 31), (0, 0, 42, 32), (-1, 0, 8, 8), (8, 8, 8, 9)):      # 42 x 31 at scale 2
        assert _c_decode(A, "aej_jpegdec_batch_sbox", data, 2, bad, out) == -1, bad      # AEJ_ERR_ARG
        torch.cuda.synchronize()
        assert torch.equal(out, pattern)
    assert _c_decode(A, "aej_jpegdec_batch_box", data, 2, (0, 0, 8, 8), out) == -5      # AEJ_ERR_UNSUPPORTED, as it was
    torch.cuda.synchronize()
    assert torch.equal(out, pattern)
    assert _c_decode(A, "aej_jpegdec_batch_sbox", data, 2, (3, 5, 30, 29), out) == 0
    torch.cuda.synchronize()
    (half,) = _np(A.standard_jpeg_decode_many([data], scale=2))
    _same(out[:27 * 24 * 3].view(24, 27, 3).cpu().numpy(), half[5:29, 3:30], "the C entry's scaled box")
    assert torch.equal(out[27 * 24 * 3:], pattern[27 * 24 * 3:])


def _c_resample(A, entry, src, src_wh, box, size, windows, out):
    from adaptive_edge_aware_jpeg_amd._lib import ResampleDesc, get_context
    import torch
    ctx = get_context(0)
    lib = ctx.lib
    descs = (ResampleDesc * 1)()
    d = descs[0]
    d.src_offset, d.dst_offset = 0, 0
    (d.src_w, d.src_h), (d.dst_w, d.dst_h) = src_wh, size
    d.box = (ctypes.c_float * 4)(*box)
    d.filter, d.reduce_x, d.reduce_y = 2, 1, 1
    ch = (ctypes.c_int * 1)(3)
    how = (ctypes.addressof(ch),)
    if entry.endswith("_win"):
        ww = (ctypes.c_int32 * 4)(*windows) if windows is not None else None
        how += (ctypes.addressof(ww) if ww is not None else None,)
    nws = int(getattr(lib, entry.replace("batch", "workspace_bytes"))(ctx.handle, ctypes.addressof(descs), 1, *how))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device="cuda")
    rc = getattr(lib, entry)(ctx.handle, ctypes.addressof(descs), 1, *how, src.data_ptr(), ctypes.c_uint64(src.numel()), out.data_ptr(),
                             ctypes.c_uint64(out.numel()), ws.data_ptr(), ctypes.c_uint64(ws.numel()))
    return rc, nws


def test_c_resample_window(A):
    import torch
    img = torch.from_numpy(R.picture(61, 83)).cuda()
    box, size = (3.5, 5, 60, 40.25), (32, 24)
    (want,) = _np(A.resize_many([img], size, "bilinear", box=box))
    x0, y0, x1, y1 = A.resized_crop_plan(83, 61, box, size, "bilinear")["window"]
    assert (x0, y0) != (0, 0) and x1 < 83 and y1 < 61
    pattern = (torch.arange(32 * 24 * 3 + 64, device="cuda") % 251).to(torch.uint8)
    part = img[y0:y1, x0:x1].contiguous()
    out = pattern.clone()
    rc, nws = _c_resample(A, "aej_resample_batch_win", part, (x1 - x0, y1 - y0), box, size, (x0, y0, 83, 61), out)
    assert rc == 0 and nws > 0
    torch.cuda.synchronize()
    _same(out[:32 * 24 * 3].view(24, 32, 3).cpu().numpy(), want, "the window")
    assert torch.equal(out[32 * 24 * 3:], pattern[32 * 24 * 3:])
    for small, origin in ((img[y0:y1, x0:x1 - 1], (x0, y0)), (img[y0:y1 - 1, x0:x1], (x0, y0)), (img[y0:y1, x0 + 1:x1], (x0 + 1, y0)),
                          (img[y0 + 1:y1, x0:x1], (x0, y0 + 1))):      # one pixel too small on either side
        out = pattern.clone()
        rc, nws = _c_resample(A, "aej_resample_batch_win", small.contiguous(), (small.shape[1], small.shape[0]), box, size, origin + (83, 61), out)
        assert rc == -1 and nws == 0                         # AEJ_ERR_ARG before any device work
        torch.cuda.synchronize()
        assert torch.equal(out, pattern)
    out = pattern.clone()
    assert _c_resample(A, "aej_resample_batch_win", part, (x1 - x0, y1 - y0), box, size, (x0, y0, x1 - x0, 61), out)[0] == -1      # the rectangle leaves its virtual image
    a, b = pattern.clone(), pattern.clone()
    assert _c_resample(A, "aej_resample_batch_win", img, (83, 61), box, size, None, a)[0] == 0      # NULL windows: the _ch call
    assert _c_resample(A, "aej_resample_batch_ch", img, (83, 61), box, size, None, b)[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    _same(a[:32 * 24 * 3].view(24, 32, 3).cpu().numpy(), want, "no window")
