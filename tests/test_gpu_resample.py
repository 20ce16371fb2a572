"""GPU: resize_many, standard_jpeg_thumbnail_many and aej_resample_batch (csrc/resample.hip: k_rs_reduce, k_rs_horizontal,
k_rs_vertical) pixel-identical to Pillow's Image.resize / Image.thumbnail: against recorded Pillow pixels (tests/golden/resample) and,
for shapes chosen for the kernels, against the NumPy model tests/resample_reference.py.  Exactness is the criterion."""
import ctypes
import json
import os

import numpy as np
import pytest

import resample_reference as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
HERE = os.path.join(GOLDEN, "resample")


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "meta.json")) as f:
        return json.load(f)["cases"], dict(np.load(os.path.join(HERE, "pixels.npz")))


def _file(folder, name):
    with open(os.path.join(GOLDEN, folder, name + ".jpg"), "rb") as f:
        return f.read()


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), what


def _picture(H, W, seed=3):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return np.clip(np.stack([(x * 7) % 256, (y * 13 + x) % 256, (x * 3 + y * 5) % 256], -1) + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
def test_thumbnail_fixtures(A, golden):
    """every thumbnail fixture, one call per (folder, filter, reducing_gap), sizes per file"""
    cases, px = golden
    groups = {}
    for c in cases:
        if c["kind"] == "thumb":
            groups.setdefault((c["folder"], c["filter"], c["gap"]), []).append(c)
    assert len(groups) > 10
    for (folder, f, gap), cs in groups.items():
        got = _np(A.standard_jpeg_thumbnail_many([_file(folder, c["name"]) for c in cs], [tuple(c["size"]) for c in cs], resample=f,
                                                 reducing_gap=gap, progressive=folder == "jpegprog"))
        for c, g in zip(cs, got):
            _same(g, px[c["key"]], c["key"])


def test_resize_fixtures(A, golden):
    """every resize fixture, one call per reducing_gap: sources, sizes, filters and boxes vary per image; NumPy and device inputs"""
    import torch
    cases, px = golden
    for gap in (None, 1.0, 1.5, 2.0, 3.0):
        cs = [c for c in cases if c["kind"] == "resize" and c["gap"] == gap]
        assert cs
        imgs = [px[f"src/{c['source']}"] for c in cs]
        imgs = [torch.from_numpy(a).cuda() if k % 2 else a for k, a in enumerate(imgs)]
        got = _np(A.resize_many(imgs, [tuple(c["size"]) for c in cs], resample=[c["filter"] for c in cs], box=[c["box"] for c in cs], reducing_gap=gap))
        for c, g in zip(cs, got):
            _same(g, px[c["key"]], c["key"])
    one = A.resize_many([px["src/0"]], (20, 11), resample=3)                      # Pillow's integer, one size, one image
    _same(_np(one)[0], px["resize/0"], "resize/0 by integer")


def test_mixed_call_and_allocation(A, golden):
    """baseline and progressive files interleaved, sizes and filters per file, every class of case in one call; one packed storage"""
    cases, px = golden
    th = [c for c in cases if c["kind"] == "thumb" and c["gap"] == 1.0]
    th = [th[(7 * i) % len(th)] for i in range(len(th))]
    assert len({c["folder"] for c in th[:6]}) == 2
    assert {c["scale"] for c in th if not c["unchanged"]} == {1, 2, 4, 8} and any(c["unchanged"] for c in th) and any(c["drafted_is_final"] for c in th)
    assert any(max(c["factors"]) > 1 for c in th) and any(max(c["factors"]) == 1 and not c["unchanged"] for c in th) and any(c["grey"] for c in th) and any(c["restart"] for c in th)
    assert any(c["file_size"] == [1, 1] for c in th) and len({c["filter"] for c in th}) == 5
    ts = A.standard_jpeg_thumbnail_many([_file(c["folder"], c["name"]) for c in th], [tuple(c["size"]) for c in th],
                                        resample=[c["filter"] for c in th], reducing_gap=1.0, progressive=True)
    assert len({t.untyped_storage().data_ptr() for t in ts}) == 1
    assert ts[0].untyped_storage().nbytes() == sum(px[c["key"]].size for c in th)
    for c, g in zip(th, _np(ts)):
        _same(g, px[c["key"]], c["key"])
    # a call in which nothing changes is the decode
    small = [c for c in th if c["unchanged"]]
    ts = A.standard_jpeg_thumbnail_many([_file(c["folder"], c["name"]) for c in small], (500, 500), progressive=True)
    for c, g in zip(small, _np(ts)):
        _same(g, px[c["key"]], c["key"])


# ---- shapes chosen for the kernels, against the model ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    return _picture(19, 1101)


@pytest.mark.parametrize("f", ["lanczos", "box"])
def test_tile_borders_and_long_tap_loops(A, wide, f):
    """rows wider than a workgroup's 256 pixels; 1101 -> 3 under lanczos is a loop of about 2200 taps"""
    sizes = [(3, 19), (1101, 5), (1500, 40), (550, 9)]
    got = _np(A.resize_many([wide] * len(sizes), sizes, resample=f))
    for s, g in zip(sizes, got):
        _same(g, M.resize(wide, s, f), (f, s))


def test_edge_shapes(A):
    one, small, thin, pic = _picture(1, 1, 5), _picture(5, 7, 6), _picture(23, 1, 7), _picture(12, 17, 8)
    jobs = [(one, (5, 7), None), (small, (1, 1), None), (thin, (1, 9), None), (thin, (4, 23), None), (thin, (3, 40), None),
            (pic, (6, 5), (0.5, 0.25, 16.4, 12)),          # the last column is partly covered
            (pic, (17, 12), (0, 0, 16.5, 12)), (pic, (17, 12), None)]
    for f in ("bicubic", "bilinear", "hamming"):
        got = _np(A.resize_many([j[0] for j in jobs], [j[1] for j in jobs], resample=f, box=[j[2] for j in jobs]))
        for j, g in zip(jobs, got):
            _same(g, M.resize(j[0], j[1], f, j[2]), (f, j[0].shape, j[1], j[2]))


def test_reduce_alone(A):
    """reducing_gap=1.0: whole factors first, equal and different per axis, with partial cells at the right and bottom edges"""
    a = _picture(37, 53, 9)
    white = np.full_like(a, 255)
    for (fx, fy), size in [((2, 2), (20, 15)), ((3, 5), (15, 7)), ((7, 1), (7, 30))]:
        assert M.reduce_factors((0, 0, 53, 37), size, 1.0) == (fx, fy) and (53 % fx or 37 % fy)
        for f in ("box", "bicubic"):
            got = _np(A.resize_many([a, white], size, resample=f, reducing_gap=1.0))
            _same(got[0], M.resize(a, size, f, None, 1.0), (fx, fy, f))
            assert got[1].shape == (size[1], size[0], 3) and (got[1] == 255).all(), (fx, fy, f)
    b = _picture(48, 64, 10)                          # 64 x 48 -> 8 x 6 by (8, 8): the reduce writes the result itself
    _same(_np(A.resize_many([b], (8, 6), reducing_gap=1.0))[0], M.reduce(b, (8, 8)), "reduce only")


def test_truncated_scan_raises_the_decoders_error(A):
    data = _file("jpegdec", "buildings_96x128_crop_q95")
    d = A.standard_jpeg.parse_header(data)
    cut = data[:d.scan_offset + (len(data) - d.scan_offset) // 2]
    good = _file("jpegdec", "lena_64x64_420_q75")
    with pytest.raises(ValueError) as want:
        A.standard_jpeg_decode_many([good, cut])
    with pytest.raises(ValueError) as got:
        A.standard_jpeg_thumbnail_many([good, cut], (20, 20))
    assert str(got.value) == str(want.value) and str(got.value).startswith("file 1:")


# ---- the C entry, called directly ---------------------------------------------------------------------------------------------------------------
def _c_batch(A, imgs, steps, filters, gap, break_desc=None):
    """aej_resample_batch into an output pre-filled with 0xA5, image i followed by `gap` spare bytes -> (rc, output, offsets)"""
    from adaptive_edge_aware_jpeg_amd._lib import ResampleDesc, get_context
    ctx = get_context(0)
    t, lib, n = ctx.torch, ctx.lib, len(imgs)
    src = t.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(ctx.device)
    descs = (ResampleDesc * n)()
    spos = dpos = 5                                    # an odd start as well
    off = []
    for i, (a, s) in enumerate(zip(imgs, steps)):
        d = descs[i]
        d.src_offset, d.dst_offset = spos - 5, dpos
        (d.src_w, d.src_h), (d.dst_w, d.dst_h) = s["src"], s["dst"]
        d.box = (ctypes.c_float * 4)(*s["box"])
        d.filter = filters[i]
        d.reduce_x, d.reduce_y = s["factors"]
        d.reduce_box = (ctypes.c_int32 * 4)(*s["reduce_box"])
        off.append(dpos)
        spos += a.size
        dpos += d.dst_w * d.dst_h * 3 + gap
    if break_desc:
        break_desc(descs)
    out = t.full((dpos + 16,), 0xA5, dtype=t.uint8, device=ctx.device)
    nws = int(lib.aej_resample_workspace_bytes(ctx.handle, ctypes.addressof(descs), n))
    ws = ctx.workspace(max(nws, 1 << 16))
    rc = lib.aej_resample_batch(ctx.handle, ctypes.addressof(descs), n, src.data_ptr(), ctypes.c_uint64(src.numel()), out.data_ptr(),
                                ctypes.c_uint64(out.numel()), ws.data_ptr(), ctypes.c_uint64(ws.numel()))
    t.cuda.synchronize()
    return rc, out.cpu().numpy(), off, nws


def test_c_bytes_outside_each_image_are_untouched(A):
    from adaptive_edge_aware_jpeg_amd import resample as RS
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    imgs = [_picture(37, 53, 1), _picture(19, 40, 2), _picture(5, 7, 3), _picture(48, 64, 4), _picture(9, 9, 5)]
    jobs = [((20, 11), None, 3, None), ((5, 4), None, 5, 2.0), ((21, 15), None, 1, None), ((8, 6), (1.5, 2, 60, 47.5), 4, 1.0), ((9, 9), None, 2, None)]
    steps = [RS._steps(f"image {i}", a.shape[1], a.shape[0], s, b, f, g) for i, (a, (s, b, f, g)) in enumerate(zip(imgs, jobs))]
    filters = [j[2] for j in jobs]
    for gap in (61, 3):                                # odd gaps: images start at every alignment
        rc, out, off, nws = _c_batch(A, imgs, steps, filters, gap)
        assert rc == 0 and nws > 0
        end = 0
        for a, (s, b, f, g), o in zip(imgs, jobs, off):
            assert (out[end:o] == 0xA5).all(), (s, gap)
            assert np.array_equal(out[o:o + s[0] * s[1] * 3].reshape(s[1], s[0], 3), M.resize(a, s, f, b, g)), (s, f, gap)
            end = o + s[0] * s[1] * 3
        assert (out[end:] == 0xA5).all()

    def breaker(field, value, index=None):
        def run(descs):
            if index is None:
                setattr(descs[2], field, value)
            else:
                getattr(descs[2], field)[index] = value
        return run
    bad = [(breaker("filter", 0), "image 2: unknown filter"), (breaker("filter", 6), "image 2: unknown filter"), (breaker("dst_w", 0), "image 2: a size below 1"),
           (breaker("src_h", -3), "image 2: a size below 1"), (breaker("box", 7.0, 0), "image 2: an empty box"), (breaker("box", 7.5, 2), "image 2: a box outside"),
           (breaker("box", -0.5, 1), "image 2: a box outside"), (breaker("reduce_x", 0), "image 2: reduce factors"), (breaker("dst_offset", 1 << 40), "image 2: image outside")]
    for run, msg in bad:
        rc, out, _, nws = _c_batch(A, imgs, steps, filters, 3, run)
        assert rc == -1 and (out == 0xA5).all(), msg
        with pytest.raises(ValueError, match=msg):
            get_context(0).check(rc)
