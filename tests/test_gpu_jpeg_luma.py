"""GPU: mode="L" / "auto" of standard_jpeg_decode_many, standard_jpeg_thumbnail_many and standard_jpeg_thumbnail_jpeg_many, [H, W] images in
resize_many, and the C entries behind them (aej_jpegdec_batch_mode, aej_jpegprog_batch_mode, aej_resample_batch_ch; csrc/jpegdec.hip
k_jd_luma, the one-channel kernels of csrc/resample.hip).  The references are Pillow's own: ``im.draft("L", ...)`` -- the luma plane, not
``convert("L")`` -- live and as the fixtures tests/golden/jpeg_luma record it, and tests/resample_reference.py on three stacked copies.
Everything is pixel- or byte-exact."""
import ctypes
import io
import json
import os

import numpy as np
import pytest

import jpeg_luma_reference as LR
import resample_reference as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
HERE = os.path.join(GOLDEN, "jpeg_luma")
SCALES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "meta.json")) as f:
        return json.load(f), dict(np.load(os.path.join(HERE, "pixels.npz")))


@pytest.fixture(scope="module")
def live(golden):
    """live Pillow is asked only where its libjpeg-turbo is the one that made the fixtures; the fixtures are compared always"""
    from PIL import features
    return features.version("libjpeg_turbo") == golden[0]["libjpeg_turbo"]


def _file(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), what


def _picture(H, W, seed=3):
    """saturated colours under noise: the clamped RGB makes convert("L") differ from the luma plane"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return np.clip(np.stack([(x * 37) % 256, (y * 53 + x * 11) % 256, 255 - (x * 29 + y * 5) % 256], -1) + rng.integers(-60, 61, (H, W, 3)), 0, 255).astype(np.uint8)


def _save(a, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_fixtures_L_and_auto(A, golden, scale):
    """every fixture file, baseline and progressive mixed in one call per scale"""
    meta, px = golden
    names = [c["name"] for c in meta["cases"]]
    names = [names[(7 * i) % len(names)] for i in range(len(names))]
    files = [_file(n) for n in names]
    for n, g in zip(names, _np(A.standard_jpeg_decode_many(files, progressive=True, scale=scale, mode="L"))):
        _same(g, px[f"{n}/L{scale}"], (n, scale, "L"))
    if scale == 1:
        ts = A.standard_jpeg_decode_many(files, progressive=True, mode="auto")
        for n, g in zip(names, _np(ts)):
            _same(g, px[f"{n}/auto"], (n, "auto"))
        assert len({t.untyped_storage().data_ptr() for t in ts}) == 1 and ts[0].untyped_storage().nbytes() == sum(t.numel() for t in ts)
    else:                                            # "auto" at a scale: a grey file's samples, a colour file as without the keyword
        rgb = _np(A.standard_jpeg_decode_many(files, progressive=True, scale=scale))
        for n, g, r in zip(names, _np(A.standard_jpeg_decode_many(files, progressive=True, scale=scale, mode="auto")), rgb):
            _same(g, px[f"{n}/L{scale}"] if g.ndim == 2 else r, (n, scale, "auto"))
            assert (g.ndim == 2) == ("grey" in n)


def test_fixtures_mixed_modes_and_scales(A, golden):
    meta, px = golden
    names = [c["name"] for c in meta["cases"]]
    names = [names[(11 * i) % len(names)] for i in range(len(names))]
    files = [_file(n) for n in names]
    modes = [("RGB", "L", "auto")[i % 3] for i in range(len(names))]
    scales = [SCALES[(i // 3) % 4] for i in range(len(names))]
    ts = A.standard_jpeg_decode_many(files, progressive=True, scale=scales, mode=modes)
    plain = _np(A.standard_jpeg_decode_many(files, progressive=True, scale=scales))
    assert len({t.untyped_storage().data_ptr() for t in ts}) == 1 and ts[0].untyped_storage().nbytes() == sum(t.numel() for t in ts)
    seen = set()
    for n, m, s, g, p in zip(names, modes, scales, _np(ts), plain):
        one = m == "L" or (m == "auto" and "grey" in n)
        _same(g, px[f"{n}/L{s}"] if one else p, (n, m, s))
        seen.add((m, s, one))
    assert len(seen) >= 12
    # "RGB", by name or by default, is the call as it was: the same bytes in the same allocation layout
    again = A.standard_jpeg_decode_many(files, progressive=True, scale=scales, mode="RGB")
    assert all(np.array_equal(a, b) for a, b in zip(_np(again), plain))


def test_the_fixtures_tell_luma_from_convert_L(A, golden):
    """the maker's condition, asserted on what the device returns: for every sampling a colour fixture whose mode-"L" decode is NOT
    convert("RGB").convert("L")"""
    meta, px = golden
    differ = {}
    for c in meta["cases"]:
        if c["sampling"] != "grey" and c["luma_vs_convert_l"] > 0:
            data = _file(c["name"])
            got = A.standard_jpeg_decode_many([data], progressive=True, mode="L")[0].cpu().numpy()
            _same(got, px[c["name"] + "/L1"], c["name"])
            differ[c["sampling"]] = differ.get(c["sampling"], 0) + int((got != LR.convert_l(data)).sum())
    assert all(differ.get(s, 0) >= 1 for s in ("4:4:4", "4:2:2", "4:2:0")), differ


# ---- shapes chosen for the kernel, live against Pillow ----------------------------------------------------------------------------------
SHAPES = [(1, 1), (7, 9), (8, 8), (17, 33), (37, 53), (1, 40), (40, 1)]      # (H, W); 53: an L image's rows start on all four alignments


def _live_files():
    """(label, bytes): every shape at 4:4:4, 4:2:2 and 4:2:0; the wide ones -- 65 MCUs per row at 4:2:0 (a second run of one MCU),
    67 at 4:4:4 -- and a wide grey one; each baseline and progressive"""
    out = []
    for prog in (False, True):
        for k, (H, W) in enumerate(SHAPES):
            for ss in (0, 1, 2):
                out.append((f"{H}x{W} ss{ss} prog{int(prog)}", _save(_picture(H, W, k), quality=90, subsampling=ss, progressive=prog)))
        out.append((f"24x1040 ss2 prog{int(prog)}", _save(_picture(24, 1040, 11), quality=70, subsampling=2, progressive=prog)))
        out.append((f"9x530 ss0 prog{int(prog)}", _save(_picture(9, 530, 12), quality=80, subsampling=0, progressive=prog)))
        out.append((f"13x600 grey prog{int(prog)}", _save(_picture(13, 600, 13)[..., 1], quality=85, progressive=prog)))
    return out


@pytest.mark.parametrize("scale", SCALES)
def test_kernel_shapes_against_live_pillow(A, live, scale):
    if not live:
        pytest.skip("another libjpeg-turbo than the fixtures': its IDCT need not be bit-identical")
    items = _live_files()
    got = _np(A.standard_jpeg_decode_many([d for _, d in items], progressive=True, scale=scale, mode="L"))
    for (label, d), g in zip(items, got):
        _same(g, LR.draft_l(d, scale), (label, scale))


def test_440_and_restart_sources(A, golden, live):
    meta, px = golden
    for n in ("jpegdec/buildings_50x66_rst3_q70", "jpegdec/jelly_40x70_rstrow_422_q80", "jpegdec/grey_33x47_rst3_q40", "jpegprog/bikes_53x37_420_rst3_q50",
              "jpegprog/grey_40x24_rstrow_q85"):
        for s, g in zip(SCALES, _np(A.standard_jpeg_decode_many([_file(n)] * 4, progressive=True, scale=list(SCALES), mode="L"))):
            _same(g, px[f"{n}/L{s}"], (n, s))
    if not live:
        pytest.skip("another libjpeg-turbo than the fixtures'")
    src = [_file("jpegdec/baboon_48x40_422_q50"), _file("jpegprog/jelly_40x70_rstrow_422_q80")]
    for prog in (False, True):
        turned = A.standard_jpeg_transform_many(src, "rot90", progressive=prog, trim=True, layout_440=True)      # prog: the output's kind
        assert all(LR.sampling(t) == "4:4:0" for t in turned)
        for s in SCALES:
            for k, g in enumerate(_np(A.standard_jpeg_decode_many(turned, progressive=True, scale=s, mode="L", layout_440=True))):
                _same(g, LR.draft_l(turned[k], s), ("4:4:0", prog, k, s))


# ---- the C entries, called directly -------------------------------------------------------------------------------------------------------
def _c_decode(A, files, scales, comps, gaps, entry="mode", short=0):
    """aej_jpegdec_batch_mode ("mode"; comps None: a NULL components_host) or aej_jpegdec_batch_scaled ("scaled") into an output pre-filled
    with 0xA5, image i followed by gaps[i % len(gaps)] spare bytes -> (rc, output, offsets, byte counts, status, workspace bytes)"""
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc, get_context
    SJ = A.standard_jpeg
    ctx = get_context(0)
    t, lib, n = ctx.torch, ctx.lib, len(files)
    parsed = [SJ.parse_header(f, i) for i, f in enumerate(files)]
    views = [memoryview(f).cast("B") for f in files]
    descs = (JpegDecDesc * n)(*parsed)
    scans, scan_off = SJ._stage(ctx, views, [(i, parsed[i].scan_offset, parsed[i].scan_length) for i in range(n)])
    sc = np.ascontiguousarray(scales, np.int32)
    cc = None if comps is None else np.ascontiguousarray(comps, np.int32)
    nb = [-(-d.height // max(int(s), 1)) * -(-d.width // max(int(s), 1)) * (3 if cc is None or cc[i] != 1 else 1) for i, (d, s) in enumerate(zip(parsed, sc))]
    off, pos = np.zeros(n, np.int64), 0
    for i in range(n):
        off[i] = pos
        pos += nb[i] + gaps[i % len(gaps)]
    total = pos - gaps[(n - 1) % len(gaps)] - short if short else pos + 16
    out = t.full((pos + 16,), 0xA5, dtype=t.uint8, device=ctx.device)
    status = t.full((n,), 77, dtype=t.int32, device=ctx.device)
    how = (sc.ctypes.data,) if entry == "scaled" else (sc.ctypes.data, None if cc is None else cc.ctypes.data)
    nbytes = lib.aej_jpegdec_workspace_bytes_scaled if entry == "scaled" else lib.aej_jpegdec_workspace_bytes_mode
    batch = lib.aej_jpegdec_batch_scaled if entry == "scaled" else lib.aej_jpegdec_batch_mode
    nws = int(nbytes(ctx.handle, ctypes.addressof(descs), n, *how))
    ws = ctx.workspace(max(nws, 1 << 20))
    rc = batch(ctx.handle, ctypes.addressof(descs), n, *how, scans.data_ptr(), ctypes.c_uint64(scans.numel()), scan_off.ctypes.data,
               out.data_ptr(), ctypes.c_uint64(total), off.ctypes.data, status.data_ptr(), ws.data_ptr(), ctypes.c_uint64(ws.numel()))
    t.cuda.synchronize()
    return rc, out.cpu().numpy(), off, nb, status.cpu().numpy(), nws


def _baseline_names(golden):
    return [c["name"] for c in golden[0]["cases"] if c["name"].startswith("jpegdec/")]


def test_c_decode_bytes_outside_each_image_are_untouched(A, golden):
    """L and RGB images, every scale, with 1-, 2- and 3-byte gaps between them: rows of L images start and end on every alignment"""
    meta, px = golden
    names = _baseline_names(golden)
    files = [_file(n) for n in names]
    scales = [SCALES[i % 4] for i in range(len(names))]
    comps = [(1, 1, 3)[(i // 2) % 3] for i in range(len(names))]
    rgb = _np(A.standard_jpeg_decode_many(files, scale=scales))
    for gaps in ((1, 2, 3), (3, 1, 2, 2)):
        rc, out, off, nb, st, nws = _c_decode(A, files, scales, comps, gaps)
        assert rc == 0 and not st.any() and nws > 0
        end = 0
        for n, s, c, o, b, r in zip(names, scales, comps, off, nb, rgb):
            assert (out[end:o] == 0xA5).all(), (n, s, c)
            want = px[f"{n}/L{s}"] if c == 1 else r
            assert b == want.size and np.array_equal(out[o:o + b].reshape(want.shape), want), (n, s, c)
            end = o + b
        assert (out[end:] == 0xA5).all()
    # a luma file adds no sample planes: the workspace of an all-L call is below the same call's as RGB, at full size too
    ones = [1] * len(files)
    all_l, all_rgb = _c_decode(A, files, ones, [1] * len(files), (0,))[5], _c_decode(A, files, ones, [3] * len(files), (0,))[5]
    assert 0 < all_l < all_rgb


def test_c_decode_refusals(A, golden):
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    files = [_file(n) for n in _baseline_names(golden)[:3]]
    for bad in (2, 0, 4, -1):
        rc, out, _, _, st, nws = _c_decode(A, files, [1, 2, 4], [1, bad, 3], (0,))
        assert rc == -1 and nws == 0 and (out == 0xA5).all() and (st == 77).all(), bad
        with pytest.raises(ValueError, match=f"file 1: {bad} output components"):
            get_context(0).check(rc)
    # out_bytes one byte short of the last image, an L one: refused before any device work; with that byte: done
    rc, out, _, _, st, _ = _c_decode(A, files, [1, 2, 1], [3, 1, 1], (0,), short=1)
    assert rc == -1 and (out == 0xA5).all() and (st == 77).all()
    with pytest.raises(ValueError, match="file 2: image outside the output"):
        get_context(0).check(rc)
    # (the same sizes as RGB would need three times the bytes: the check uses the image's real count)
    rc, out, off, nb, st, _ = _c_decode(A, files, [1, 2, 1], [3, 1, 1], (0,))
    assert rc == 0 and not st.any() and (out[off[2]:off[2] + nb[2]] != 0xA5).any()


def test_truncated_scan_under_mode_L(A):
    data = _file("jpegdec/buildings_96x128_crop_q95")
    d = A.standard_jpeg.parse_header(data)
    cut = data[:d.scan_offset + (len(data) - d.scan_offset) // 2]
    good = _file("jpegdec/lena_64x64_420_q75")
    with pytest.raises(ValueError) as want:
        A.standard_jpeg_decode_many([good, cut])
    for s in (1, 4):
        with pytest.raises(ValueError) as e:
            A.standard_jpeg_decode_many([good, cut], scale=s, mode="L")
        assert str(e.value) == str(want.value) and str(e.value).startswith("file 1:")
    with pytest.raises(ValueError, match="file 1:"):
        A.standard_jpeg_thumbnail_many([good, cut], (16, 16), mode="L")


def test_c_mode_entries_with_all_three_are_the_scaled_entries(A, golden):
    names = _baseline_names(golden)
    files = [_file(n) for n in names]
    scales = [SCALES[(i + 1) % 4] for i in range(len(names))]
    rc0, out0, _, _, st0, ws0 = _c_decode(A, files, scales, None, (5,), entry="scaled")
    rc1, out1, _, _, st1, ws1 = _c_decode(A, files, scales, [3] * len(files), (5,))
    rc2, out2, _, _, st2, ws2 = _c_decode(A, files, scales, None, (5,))      # NULL: every file 3
    assert rc0 == rc1 == rc2 == 0 and ws0 == ws1 == ws2 and not (st0.any() or st1.any() or st2.any())
    assert np.array_equal(out0, out1) and np.array_equal(out0, out2) and (out0 != 0xA5).any()


def _c_resample(A, imgs, steps, filters, gaps, entry="ch", channels="own"):
    """aej_resample_batch_ch (channels: "own" -- each image's rank --, None for a NULL channels_host, or a list) or aej_resample_batch into
    an output pre-filled with 0xA5 -> (rc, output, offsets, workspace bytes)"""
    from adaptive_edge_aware_jpeg_amd._lib import ResampleDesc, get_context
    ctx = get_context(0)
    t, lib, n = ctx.torch, ctx.lib, len(imgs)
    src = t.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(ctx.device)
    ch = [3 if a.ndim == 3 else 1 for a in imgs]
    descs = (ResampleDesc * n)()
    spos, dpos, off = 0, 5, []
    for i, (a, s) in enumerate(zip(imgs, steps)):
        d = descs[i]
        d.src_offset, d.dst_offset = spos, dpos
        (d.src_w, d.src_h), (d.dst_w, d.dst_h) = s["src"], s["dst"]
        d.box = (ctypes.c_float * 4)(*s["box"])
        d.filter = filters[i]
        d.reduce_x, d.reduce_y = s["factors"]
        d.reduce_box = (ctypes.c_int32 * 4)(*s["reduce_box"])
        off.append(dpos)
        spos += a.size
        dpos += d.dst_w * d.dst_h * ch[i] + gaps[i % len(gaps)]
    out = t.full((dpos + 16,), 0xA5, dtype=t.uint8, device=ctx.device)
    cc = None if channels is None else np.array(ch if channels == "own" else channels, np.int32)
    how = () if entry == "plain" else (None if cc is None else cc.ctypes.data,)
    sfx = "" if entry == "plain" else "_ch"
    nws = int(getattr(lib, "aej_resample_workspace_bytes" + sfx)(ctx.handle, ctypes.addressof(descs), n, *how))
    ws = ctx.workspace(max(nws, 1 << 16))
    rc = getattr(lib, "aej_resample_batch" + sfx)(ctx.handle, ctypes.addressof(descs), n, *how, src.data_ptr(), ctypes.c_uint64(src.numel()),
                                                  out.data_ptr(), ctypes.c_uint64(out.numel()), ws.data_ptr(), ctypes.c_uint64(ws.numel()))
    t.cuda.synchronize()
    return rc, out.cpu().numpy(), off, nws


def _model(a, size, f, box, gap):
    """tests/resample_reference.py, which takes [H, W, 3]: a one-channel image is channel 0 of three stacked copies"""
    return M.resize(a, size, f, box, gap) if a.ndim == 3 else M.resize(np.stack([a] * 3, -1), size, f, box, gap)[..., 0]


JOBS = [((20, 11), None, 3, None), ((5, 4), None, 5, 2.0), ((21, 15), None, 1, None), ((8, 6), (1.5, 2, 60, 47.5), 4, 1.0), ((9, 9), None, 2, None),
        ((13, 7), None, 1, 2.0)]


def _job_images():
    p = [_picture(37, 53, 1), _picture(19, 40, 2)[..., 0], _picture(5, 7, 3)[..., 1], _picture(48, 64, 4)[..., 2], _picture(9, 9, 5)[..., 0], _picture(31, 29, 6)]
    return [np.ascontiguousarray(a) for a in p]


def test_c_resample_bytes_outside_each_image_are_untouched(A):
    """mixed channels (reduce, horizontal, vertical and copy stages of both counts), 1-, 2- and 3-byte gaps"""
    from adaptive_edge_aware_jpeg_amd import resample as RS
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    imgs = _job_images()
    steps = [RS._steps(f"image {i}", a.shape[1], a.shape[0], s, b, f, g) for i, (a, (s, b, f, g)) in enumerate(zip(imgs, JOBS))]
    filters = [j[2] for j in JOBS]
    for gaps in ((1, 2, 3), (3, 2, 1, 1)):
        rc, out, off, nws = _c_resample(A, imgs, steps, filters, gaps)
        assert rc == 0 and nws > 0
        end = 0
        for a, (s, b, f, g), o in zip(imgs, JOBS, off):
            want = _model(a, s, f, b, g)
            assert (out[end:o] == 0xA5).all(), (s, gaps)
            assert np.array_equal(out[o:o + want.size].reshape(want.shape), want), (s, f, gaps)
            end = o + want.size
        assert (out[end:] == 0xA5).all()
    for bad in (2, 0, 4):
        rc, out, _, nws = _c_resample(A, imgs, steps, filters, (0,), channels=[3, 1, bad, 1, 1, 3])
        assert rc == -1 and nws == 0 and (out == 0xA5).all()
        with pytest.raises(ValueError, match="image 2: a channel count other than 1 or 3"):
            get_context(0).check(rc)


def test_c_resample_ch_with_all_three_is_the_plain_entry(A):
    from adaptive_edge_aware_jpeg_amd import resample as RS
    imgs = [_picture(37, 53, 1), _picture(19, 40, 2), _picture(5, 7, 3), _picture(48, 64, 4), _picture(9, 9, 5), _picture(31, 29, 6)]
    steps = [RS._steps(f"image {i}", a.shape[1], a.shape[0], s, b, f, g) for i, (a, (s, b, f, g)) in enumerate(zip(imgs, JOBS))]
    filters = [j[2] for j in JOBS]
    rc0, out0, _, ws0 = _c_resample(A, imgs, steps, filters, (3,), entry="plain")
    rc1, out1, _, ws1 = _c_resample(A, imgs, steps, filters, (3,))
    rc2, out2, _, ws2 = _c_resample(A, imgs, steps, filters, (3,), channels=None)
    assert rc0 == rc1 == rc2 == 0 and ws0 == ws1 == ws2
    assert np.array_equal(out0, out1) and np.array_equal(out0, out2) and (out0 != 0xA5).any()


# ---- resize_many ------------------------------------------------------------------------------------------------------------------------------
def test_resize_L_images_mixed_with_rgb(A):
    import torch
    from PIL import Image
    rng = np.random.default_rng(17)
    imgs, sizes, filters, boxes = [], [], [], []
    for k in range(20):                              # all five filters, fractional boxes, up- and down-scaling, both ranks, both homes
        H, W = int(rng.integers(3, 70)), int(rng.integers(3, 70))
        a = _picture(H, W, k)
        imgs.append(a if k % 3 == 2 else np.ascontiguousarray(a[..., k % 3]))
        sizes.append((int(rng.integers(1, 90)), int(rng.integers(1, 90))))
        filters.append(tuple(M.FILTERS)[k % 5])
        boxes.append(None if k % 2 else (0.5, 1.25, W - 0.75, H - 0.5))
    for gap in (None, 1.0, 2.0):                     # 1.0 and 2.0 reduce first, with partial cells at the right and bottom edges
        given = [torch.from_numpy(a).cuda() if k % 2 else a for k, a in enumerate(imgs)]
        got = A.resize_many(given, sizes, resample=filters, box=boxes, reducing_gap=gap, mode="auto")
        assert len({t.untyped_storage().data_ptr() for t in got}) == 1
        for k, (a, g) in enumerate(zip(imgs, _np(got))):
            assert g.ndim == a.ndim
            _same(g, _model(a, sizes[k], filters[k], boxes[k], gap), (k, gap))
    # the wide picture: several workgroups per row, down to a handful of columns and to half
    wide = np.ascontiguousarray(_picture(19, 1101, 9)[..., 1])
    for w in (3, 550):
        for f in ("lanczos", "box"):
            for gap in (None, 2.0):
                _same(A.resize_many([wide], (w, 11), resample=f, reducing_gap=gap, mode="L")[0].cpu().numpy(), _model(wide, (w, 11), f, None, gap), (w, f, gap))
    # live Pillow on a mode-"L" image
    a = imgs[0]
    assert a.ndim == 2
    for size, f, box, gap in (((23, 17), "lanczos", None, 1.5), ((90, 61), "bicubic", (0.5, 1.25, a.shape[1] - 0.75, a.shape[0] - 0.5), None)):
        want = np.asarray(Image.fromarray(a).resize(size, M.FILTERS[f], box=box, reducing_gap=gap))
        _same(A.resize_many([a], size, resample=f, box=box, reducing_gap=gap, mode="L")[0].cpu().numpy(), want, (size, f))
    # an identity copy returns the bytes
    same = A.resize_many([a, imgs[2]], [(a.shape[1], a.shape[0]), (imgs[2].shape[1], imgs[2].shape[0])], mode="auto")
    _same(same[0].cpu().numpy(), a, "copy L")
    _same(same[1].cpu().numpy(), imgs[2], "copy RGB")


# ---- thumbnails ------------------------------------------------------------------------------------------------------------------------------
def test_thumbnail_fixtures(A, golden):
    """every thumbnail fixture: one call per (size, filter, gap), the files and the modes "L" / "auto" mixed per file"""
    meta, px = golden
    names = [c["name"] for c in meta["cases"]]
    files = [_file(n) for n in names]
    for size in meta["sizes"]:
        for r in meta["resample"]:
            for g in meta["gaps"]:
                for flip in (0, 1):
                    modes = [("L", "auto")[(i + flip) % 2] for i in range(len(names))]
                    got = _np(A.standard_jpeg_thumbnail_many(files, tuple(size), resample=r, reducing_gap=g, progressive=True, mode=modes))
                    for n, m, t in zip(names, modes, got):
                        key = f"{n}/t{m}_{size[0]}x{size[1]}_{r}_{g}"
                        _same(t, px[key], key)


def test_thumbnails_against_live_pillow(A, live):
    if not live:
        pytest.skip("another libjpeg-turbo than the fixtures'")
    SJ = A.standard_jpeg
    grey, colour = _file("jpegdec/house_45x61_grey_q60"), _file("jpegdec/buildings_96x128_crop_q95")
    com = _file("jpegdec/peppers_24x40_exif_com_q75")
    # (w, h) requests: covers the image (full size comes back); 64 x 48 is the drafted size of the 128 x 96 file at scale 2 (no resize
    # step); ordinary ones
    for size, f, gap in (((200, 200), "bicubic", 2.0), ((64, 48), "lanczos", 1.0), ((30, 30), "bicubic", 2.0), ((21, 50), "lanczos", None), ((9, 9), "box", 3.0)):
        files = [grey, colour, com, colour, grey]
        modes = ["auto", "L", "L", "auto", "L"]
        got = A.standard_jpeg_thumbnail_many(files, size, resample=f, reducing_gap=gap, mode=modes)
        for k, (d, m, t) in enumerate(zip(files, modes, got)):
            _same(t.cpu().numpy(), LR.thumbnail(d, size, f, gap, m, SJ.thumbnail_plan), (size, f, gap, k, m))
        assert got[2].jpeg_comment == b"a COM segment" and not hasattr(got[0], "jpeg_comment")
    plan = SJ.thumbnail_plan(128, 96, (64, 48), 1.0)
    assert plan[0] == 2 and plan[2] == (64, 48) and SJ.thumbnail_plan(128, 96, (200, 200), 2.0) is None


def _pil_thumbnail_jpeg(A, d, size, q, mode, f="bicubic", gap=2.0, **kw):
    im = LR.thumbnail_image(d, size, f, gap, mode, A.standard_jpeg.thumbnail_plan)
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=q, **kw)
    return buf.getvalue()


def test_jpeg_to_jpeg(A, live):
    if not live:
        pytest.skip("another libjpeg-turbo than the fixtures'")
    from PIL import Image
    SJ = A.standard_jpeg
    names = ["jpegdec/house_45x61_grey_q60", "jpegdec/buildings_96x128_crop_q95", "jpegprog/grey_33x47_rst3_q40", "jpegdec/peppers_24x40_exif_com_q75",
             "jpegdec/grey_33x47_rst3_q40", "jpegprog/lena_64x64_420_q75"]
    files = [_file(n) for n in names]
    got = A.standard_jpeg_thumbnail_jpeg_many(files, (32, 32), quality=80, progressive=True, mode="auto")
    plain = A.standard_jpeg_thumbnail_jpeg_many(files, (32, 32), quality=80, progressive=True)
    for n, d, g, p in zip(names, files, got, plain):
        if "grey" in n:                              # Pillow keeps mode "L" over thumbnail() and saves a one-component file
            assert g == _pil_thumbnail_jpeg(A, d, (32, 32), 80, "auto"), n
            assert SJ.parse_header(g).ncomp == 1 and Image.open(io.BytesIO(g)).mode == "L" and SJ.parse_header(p).ncomp == 3
        else:                                        # a colour source: the call without the keyword
            assert g == p and SJ.parse_header(g).ncomp == 3, n
    # "L": colour sources leave grey as well, from their luma plane; a COM segment is carried
    got = A.standard_jpeg_thumbnail_jpeg_many(files, (40, 24), quality=[60, 70, 80, 90, 75, 50], optimize=True, progressive_out=True, resample="lanczos",
                                              progressive=True, mode="L")
    for n, d, q, g in zip(names, files, [60, 70, 80, 90, 75, 50], got):
        assert g == _pil_thumbnail_jpeg(A, d, (40, 24), q, "L", "lanczos", optimize=True, progressive=True), n
        assert Image.open(io.BytesIO(g)).mode == "L"
    assert b"\xff\xfe\x00\x0fa COM segment" in got[3]
    # a COM segment carried through a grey file
    src = _save(_picture(40, 56, 3)[..., 0], quality=90, comment=b"grey words")
    g = A.standard_jpeg_thumbnail_jpeg_many([src], (20, 20), quality=70, mode="auto")[0]
    assert g == _pil_thumbnail_jpeg(A, src, (20, 20), 70, "auto") and b"\xff\xfe\x00\x0cgrey words" in g and SJ.parse_header(g).ncomp == 1
    # a per-file list
    mixed = A.standard_jpeg_thumbnail_jpeg_many(files[:2], (32, 32), quality=80, mode=["L", "RGB"])
    assert mixed[0] == _pil_thumbnail_jpeg(A, files[0], (32, 32), 80, "L") and mixed[1] == plain[1]
