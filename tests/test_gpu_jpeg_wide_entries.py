"""The package binds the widest C entry of every JPEG-file operation and hands it the neutral value of each option no file uses (DESIGN.md,
"What the JPEG file calls share").  That rests on a claim of include/aej.h: a wider entry fed neutral values IS the narrower entry -- the
same return code, the same workspace size, the same bytes.  Here both are called, on files at the smallest shapes where the decoders'
and coders' paths differ, with the neutral values as NULL and as arrays that say nothing (scales all 1, components all 3, transforms all
0, crop boxes whose right edge is 0, channels all 3; restart_* = layout_440 = drop_chroma = 0).  Every comparison is exact; the host-only
rows need no device."""
import ctypes
import io

import numpy as np
import pytest

import adaptive_edge_aware_jpeg_amd.resample as RS
import adaptive_edge_aware_jpeg_amd.standard_jpeg as SJ
from adaptive_edge_aware_jpeg_amd._lib import JfifManyDesc, JpegDecDesc, JpegProgFrame, JpegProgScan, ResampleDesc, load_library

gpu = pytest.mark.gpu
#        name          (H, W)    save keywords
SHAPES = (("one_mcu", (16, 16), dict(subsampling=2)),
          ("edge_444", (9, 17), dict(subsampling=0)),
          ("h2v1", (40, 24), dict(subsampling=1)),
          ("grey", (9, 9), dict()),
          ("progressive", (16, 16), dict(subsampling=2, progressive=True)),
          ("restarts", (32, 32), dict(subsampling=2, restart_marker_rows=1)))
PATTERN = 0xA5


def _pixels(name, shape):
    rng = np.random.RandomState(sum(name.encode()))
    h, w = shape
    smooth = np.add.outer(np.arange(h) * 5, np.arange(w) * 3)[..., None] + np.array([0, 40, 90])
    x = (smooth + rng.randint(0, 48, (h, w, 3))).astype(np.uint8)
    return x[..., 1].copy() if name == "grey" else x


@pytest.fixture(scope="module")
def pictures():
    return {name: _pixels(name, shape) for name, shape, _ in SHAPES}


@pytest.fixture(scope="module")
def files(pictures):
    from PIL import Image
    out = {}
    for name, _, kw in SHAPES:
        buf = io.BytesIO()
        Image.fromarray(pictures[name]).save(buf, "JPEG", quality=85, **kw)
        out[name] = buf.getvalue()
    return out


@pytest.fixture(scope="module")
def sources(files):
    """the six files parsed by the narrowest parsers: (baseline names, JpegDecDesc [5]), (the progressive name, its frame and scans)"""
    base = [n for n, _, kw in SHAPES if not kw.get("progressive")]
    descs = [SJ.parse_header(files[n]) for n in base]
    assert [d.restart_interval > 0 for d in descs] == [False, False, False, False, True] and [d.ncomp for d in descs] == [3, 3, 3, 1, 3]
    frame, scans = SJ.parse_scans(files["progressive"])
    return (base, descs), ("progressive", frame, scans)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    return get_context(0)


def _addr(a):
    return None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else ctypes.addressof(a)


def _device_bytes(pieces):
    """byte strings back to back on the device -> (uint8 tensor, int64 offsets)"""
    import torch
    off = np.concatenate(([0], np.cumsum([len(p) for p in pieces])[:-1])).astype(np.int64)
    return torch.frombuffer(bytearray(b"".join(pieces)), dtype=torch.uint8).cuda(), off


def _filled(n, dtype):
    import torch
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), PATTERN, dtype=torch.uint8, device="cuda").view(dtype)


def _run(ctx, query, batch, lead, options, tail_of):
    """one size query and one batch call -> (workspace size, return code, the device tensors it wrote, as host arrays)"""
    import torch
    nws = int(query(*lead, *options))
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    tail, written = tail_of()
    rc = batch(*lead, *options, *tail, ws.data_ptr(), ctypes.c_uint64(nws))
    torch.cuda.synchronize()
    return nws, rc, [w.cpu().numpy() for w in written]


def _all_equal(results, what):
    first = results[0]
    assert first[1] == 0, (what, first[1])
    for k, r in enumerate(results[1:], 1):
        assert r[0] == first[0] and r[1] == first[1], (what, k, "workspace size or return code", r[:2], first[:2])
        assert len(r[2]) == len(first[2])
        for a, b in zip(r[2], first[2]):
            assert np.array_equal(a, b), (what, k)
    return first


# ---- decode ----------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_baseline_decode(ctx, files, sources):
    import torch
    (names, ds), _ = sources
    lib, n = ctx.lib, len(ds)
    descs = (JpegDecDesc * n)(*ds)
    scans, so = _device_bytes([files[m][d.scan_offset:d.scan_offset + d.scan_length] for m, d in zip(names, ds)])
    sizes = [d.width * d.height * 3 for d in ds]
    oo = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    ones, threes = np.ones(n, np.int32), np.full(n, 3, np.int32)

    def tail_of():
        out, status = _filled(sum(sizes), torch.uint8), _filled(n, torch.int32)
        return (scans.data_ptr(), ctypes.c_uint64(scans.numel()), _addr(so), out.data_ptr(), ctypes.c_uint64(out.numel()), _addr(oo), status.data_ptr()), [out, status]

    lead = (ctx.handle, _addr(descs), n)
    res = [_run(ctx, lib.aej_jpegdec_workspace_bytes, lib.aej_jpegdec_batch, lead, (), tail_of)]
    for options in ((None, None, None, None), (_addr(ones), _addr(threes), None, None)):
        res.append(_run(ctx, lib.aej_jpegdec_workspace_bytes_adobe, lib.aej_jpegdec_batch_adobe, lead, options, tail_of))
    out, status = _all_equal(res, "aej_jpegdec_batch")[2]
    assert not status.any()
    from PIL import Image
    for m, d, o in zip(names, ds, oo):                        # and what both wrote is the picture Pillow decodes
        want = np.asarray(Image.open(io.BytesIO(files[m])).convert("RGB"))
        assert np.array_equal(out[o:o + want.size].reshape(want.shape), want), m


@gpu
def test_progressive_decode(ctx, files, sources):
    import torch
    _, (name, frame, scan_list) = sources
    lib = ctx.lib
    frames, scans = (JpegProgFrame * 1)(frame), (JpegProgScan * len(scan_list))(*scan_list)
    data, do = _device_bytes([files[name][s.data_offset:s.data_offset + s.data_length] for s in scan_list])
    oo = np.zeros(1, np.int64)
    ones, threes = np.ones(1, np.int32), np.full(1, 3, np.int32)

    def tail_of():
        out, status = _filled(frame.width * frame.height * 3, torch.uint8), _filled(1, torch.int32)
        return (data.data_ptr(), ctypes.c_uint64(data.numel()), _addr(do), out.data_ptr(), ctypes.c_uint64(out.numel()), _addr(oo), status.data_ptr()), [out, status]

    lead = (ctx.handle, _addr(frames), _addr(scans), 1)
    res = [_run(ctx, lib.aej_jpegprog_workspace_bytes, lib.aej_jpegprog_batch, lead, (), tail_of)]
    for options in ((None, None, None, None), (_addr(ones), _addr(threes), None, None)):
        res.append(_run(ctx, lib.aej_jpegprog_workspace_bytes_adobe, lib.aej_jpegprog_batch_adobe, lead, options, tail_of))
    out, status = _all_equal(res, "aej_jpegprog_batch")[2]
    assert not status.any()
    from PIL import Image
    want = np.asarray(Image.open(io.BytesIO(files[name])).convert("RGB"))
    assert np.array_equal(out.reshape(want.shape), want)


# ---- transcode and transform -------------------------------------------------------------------------------------------------------------------
ROT180 = SJ.TRANSFORMS.index("rot180")      # allowed for every layout; with trim = 1 for every size here (17 x 9 -> 16 x 8, 24 x 40 -> 16 x 40, 9 x 9 -> 8 x 8)


#                          narrow entries          their options after `progressive`     the _cut entries' options for the same call
@pytest.mark.parametrize("narrow, options, cut", [
    ("aej_jfif_transcode_%s", (), (None, 0, 0, 0, 0, None, 0)),
    ("aej_jfif_transcode_%s", (), ("zeros", 0, 0, 0, 0, "no boxes", 0)),
    ("aej_jfif_transcode_%s_rst", (0, 1), (None, 0, 0, 1, 0, None, 0)),
    ("aej_jfif_transform_%s", ("rot180", 1), ("rot180", 1, 0, 0, 0, None, 0)),
    ("aej_jfif_transform_%s_rst", ("rot180", 1, 2, 0), ("rot180", 1, 2, 0, 0, "no boxes", 0)),
    ("aej_jfif_transform_%s_440", ("rot180", 1, 0, 0, 1), ("rot180", 1, 0, 0, 1, None, 0)),
], ids=["transcode", "transcode-arrays", "transcode_rst", "transform", "transform_rst", "transform_440"])
@pytest.mark.parametrize("progressive", [0, 1])
@gpu
def test_transcode_and_transform(ctx, files, sources, narrow, options, cut, progressive):
    import torch
    (names, ds), (pname, frame, scan_list) = sources
    lib, nb = ctx.lib, len(ds)
    n = nb + 1
    descs, frames, pscans = (JpegDecDesc * nb)(*ds), (JpegProgFrame * 1)(frame), (JpegProgScan * len(scan_list))(*scan_list)
    data, off = _device_bytes([files[m][d.scan_offset:d.scan_offset + d.scan_length] for m, d in zip(names, ds)] +
                              [files[pname][s.data_offset:s.data_offset + s.data_length] for s in scan_list])
    so, do = np.ascontiguousarray(off[:nb]), np.ascontiguousarray(off[nb:])
    dens = np.tile(np.array([0, 1, 1], np.uint16), n)
    arrays = {"zeros": np.zeros(n, np.int32), "rot180": np.full(n, ROT180, np.int32), "no boxes": np.zeros((n, 4), np.int32)}
    given = lambda opts: tuple(_addr(arrays[o]) if isinstance(o, str) else o for o in opts)  # noqa: E731
    cap = 2 * sum(len(f) for f in files.values()) + SJ.PROGRESSIVE_HEADER_CAPACITY * n
    lead = (ctx.handle, _addr(descs), nb)

    def run(query, batch, opts):
        nws = int(query(*lead, _addr(frames), _addr(pscans), 1, progressive, *opts))
        assert nws > 0
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        out, offsets, lengths, status = _filled(cap, torch.uint8), _filled(n, torch.int64), _filled(n, torch.int64), _filled(n, torch.int32)
        total, groups = ctypes.c_uint64(), ctypes.c_int32()
        rc = batch(*lead, data.data_ptr(), ctypes.c_uint64(data.numel()), _addr(so), _addr(frames), _addr(pscans), 1, data.data_ptr(),
                   ctypes.c_uint64(data.numel()), _addr(do), _addr(dens), progressive, *opts, out.data_ptr(), ctypes.c_uint64(cap), offsets.data_ptr(),
                   lengths.data_ptr(), ctypes.addressof(total), status.data_ptr(), ctypes.addressof(groups), ws.data_ptr(), ctypes.c_uint64(nws))
        torch.cuda.synchronize()
        return nws, rc, [np.array([total.value, groups.value])] + [v.cpu().numpy() for v in (out, offsets, lengths, status)]

    res = [run(getattr(lib, narrow % "workspace_bytes"), getattr(lib, narrow % "batch"), given(options)),
           run(lib.aej_jfif_transform_workspace_bytes_cut, lib.aej_jfif_transform_batch_cut, given(cut))]
    (total, _), out, offsets, lengths, status = _all_equal(res, narrow)[2]
    assert not status.any() and 0 < total <= cap and int((offsets + lengths).max()) == total
    if not options:                                           # the transcode: the same pixels as its source, file by file
        from PIL import Image
        for k, m in enumerate(names + [pname]):
            got = Image.open(io.BytesIO(out[offsets[k]:offsets[k] + lengths[k]].tobytes()))
            assert np.array_equal(np.asarray(got), np.asarray(Image.open(io.BytesIO(files[m])))), m


# ---- encode ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimize, progressive", [(0, 0), (1, 0), (0, 1)])
@gpu
def test_encode_many(ctx, pictures, optimize, progressive):
    import torch
    lib, n = ctx.lib, len(SHAPES)
    src, off = _device_bytes([pictures[m].tobytes() for m, _, _ in SHAPES])
    descs = (JfifManyDesc * n)(*[JfifManyDesc(int(off[i]), w, h, 85, 1 if m == "grey" else 3) for i, (m, (h, w), _) in enumerate(SHAPES)])
    cap = sum(SJ.PROGRESSIVE_HEADER_CAPACITY + 3 * h * w for _, (h, w), _ in SHAPES)
    lead = (ctx.handle, _addr(descs), n)

    def run(query, batch, rst):
        nws = int(query(*lead, 2, optimize, progressive, *rst))
        assert nws > 0
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        out, offsets, lengths = _filled(cap, torch.uint8), _filled(n, torch.int64), _filled(n, torch.int64)
        total, groups = ctypes.c_uint64(), ctypes.c_int32()
        rc = batch(*lead, src.data_ptr(), ctypes.c_uint64(src.numel()), 2, optimize, progressive, *rst, out.data_ptr(), ctypes.c_uint64(cap),
                   offsets.data_ptr(), lengths.data_ptr(), ctypes.addressof(total), ctypes.addressof(groups), ws.data_ptr(), ctypes.c_uint64(nws))
        torch.cuda.synchronize()
        return nws, rc, [np.array([total.value, groups.value])] + [v.cpu().numpy() for v in (out, offsets, lengths)]

    res = [run(lib.aej_jfif_many_workspace_bytes, lib.aej_jfif_many_encode, ()),
           run(lib.aej_jfif_many_workspace_bytes_rst, lib.aej_jfif_many_encode_rst, (0, 0))]
    (total, _), out, offsets, lengths = _all_equal(res, "aej_jfif_many_encode")[2]
    assert 0 < total <= cap and int((offsets + lengths).max()) == total
    from PIL import Image
    for k, (m, _, _) in enumerate(SHAPES):                    # and the files are Pillow's
        buf = io.BytesIO()
        kw = {} if m == "grey" else dict(subsampling=2)      # (Pillow writes an explicit subsampling into a grey file's frame header)
        Image.fromarray(pictures[m]).save(buf, "JPEG", quality=85, optimize=bool(optimize), progressive=bool(progressive), **kw)
        assert out[offsets[k]:offsets[k] + lengths[k]].tobytes() == buf.getvalue(), m


# ---- resample ----------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_resample(ctx, pictures):
    import torch
    lib = ctx.lib
    names = [m for m, _, _ in SHAPES if m != "grey"]
    n = len(names)
    src, off = _device_bytes([pictures[m].tobytes() for m in names])
    #        size (w, h)   filter       reducing_gap: a copy, an enlargement, a reduction, one with whole factors first, a box filter
    jobs = [((16, 16), "bicubic", None), ((23, 11), "bilinear", None), ((7, 13), "lanczos", None), ((5, 5), "bicubic", 1.0), ((9, 31), "box", None)]
    descs, pos = (ResampleDesc * n)(), 0
    for i, (m, (size, f, gap)) in enumerate(zip(names, jobs)):
        h, w = pictures[m].shape[:2]
        s = RS._steps(m, w, h, size, None, RS._check_filter(f), gap)
        d = descs[i]
        d.src_offset, d.dst_offset, d.filter = int(off[i]), pos, RS._check_filter(f)
        (d.src_w, d.src_h), (d.dst_w, d.dst_h), (d.reduce_x, d.reduce_y) = s["src"], s["dst"], s["factors"]
        d.box, d.reduce_box = (ctypes.c_float * 4)(*s["box"]), (ctypes.c_int32 * 4)(*s["reduce_box"])
        pos += size[0] * size[1] * 3
    assert any(descs[i].reduce_x > 1 for i in range(n))
    threes = np.full(n, 3, np.int32)
    lead = (ctx.handle, _addr(descs), n)

    def tail_of():
        out = _filled(pos, torch.uint8)
        return (src.data_ptr(), ctypes.c_uint64(src.numel()), out.data_ptr(), ctypes.c_uint64(pos)), [out]

    res = [_run(ctx, lib.aej_resample_workspace_bytes, lib.aej_resample_batch, lead, (), tail_of)]
    for options in ((None, None), (_addr(threes), None)):
        res.append(_run(ctx, lib.aej_resample_workspace_bytes_win, lib.aej_resample_batch_win, lead, options, tail_of))
    out, = _all_equal(res, "aej_resample_batch")[2]
    from PIL import Image
    for i, (m, (size, f, gap)) in enumerate(zip(names, jobs)):
        want = np.asarray(Image.fromarray(pictures[m]).resize(size, RS._check_filter(f), reducing_gap=gap))
        assert np.array_equal(out[descs[i].dst_offset:descs[i].dst_offset + want.size].reshape(want.shape), want), m


# ---- the host-only entries: no device ----------------------------------------------------------------------------------------------------------
def _frames(sources):
    (names, ds), (pname, frame, _) = sources
    return [(m, d, False) for m, d in zip(names, ds)] + [(pname, frame, True)]


def test_geometry_host(sources):
    """every code, trimmed and not, of every file: the entries that take three components as read and the _cut entry given the frame's own
    count answer alike -- a parsed one-component frame carries hs = vs = 1, for which the count does not bear on the geometry"""
    lib = load_library()
    seen = set()
    for m, f, _ in _frames(sources):
        assert f.ncomp in (1, 3) and (f.ncomp == 3 or (f.hs, f.vs) == (1, 1))
        for code in range(8):
            for trim in (0, 1):
                for l440 in (0, 1):
                    narrow, wide = (ctypes.c_int32 * 4)(*[-1] * 4), (ctypes.c_int32 * 6)(*[-1] * 6)
                    if l440:
                        rc = lib.aej_jfif_transform_geometry_host_440(f.height, f.width, f.hs, f.vs, code, trim, 1, ctypes.addressof(narrow))
                    else:
                        rc = lib.aej_jfif_transform_geometry_host(f.height, f.width, f.hs, f.vs, code, trim, ctypes.addressof(narrow))
                    for box in (None, (ctypes.c_int32 * 4)(0, 0, 0, 0)):
                        rc_cut = lib.aej_jfif_transform_geometry_host_cut(f.height, f.width, f.hs, f.vs, f.ncomp, code, trim, l440, _addr(box), 0,
                                                                          ctypes.addressof(wide))
                        assert rc_cut == rc, (m, code, trim, l440)
                        assert tuple(wide) == (tuple(narrow) + (0, 0) if rc == 0 else (-1,) * 6), (m, code, trim, l440)
                    seen.add(rc)
    assert seen == {0, 1, -5}                                 # accepted, not perfect, a transposed 4:2:2 without layout_440 (no size here trims to nothing)


def test_headers_host(files, sources):
    lib = load_library()
    dens = (ctypes.c_uint16 * 3)(1, 72, 72)
    for m, f, is_prog in _frames(sources):
        src = (None if is_prog else ctypes.addressof(f), ctypes.addressof(f) if is_prog else None, ctypes.addressof(dens))
        for progressive in (0, 1):
            calls = [(lib.aej_jfif_transcode_headers_host, (), (0, 0, 0))]
            for code, trim in ((0, 0), (ROT180, 1), (SJ.TRANSFORMS.index("transpose"), 0)):
                calls.append((lib.aej_jfif_transform_headers_host, (code, trim), (code, trim, 0)))
                calls.append((lib.aej_jfif_transform_headers_host_440, (code, trim, 1), (code, trim, 1)))
            for entry, options, cut in calls:
                a, b, c = ((ctypes.c_uint8 * 512)(*[PATTERN] * 512) for _ in range(3))
                na = entry(*src, progressive, *options, ctypes.addressof(a), 512)
                nb = lib.aej_jfif_transform_headers_host_cut(*src, progressive, *cut, None, 0, ctypes.addressof(b), 512)
                zero = (ctypes.c_int32 * 4)(0, 0, 0, 0)
                nc = lib.aej_jfif_transform_headers_host_cut(*src, progressive, *cut, ctypes.addressof(zero), 0, ctypes.addressof(c), 512)
                assert na == nb == nc and bytes(a) == bytes(b) == bytes(c), (m, progressive, options)
                assert na > 0 or (na == -5 and m == "h2v1" and options[:1] == (SJ.TRANSFORMS.index("transpose"),) and options[2:] != (1,)), (m, options, na)
