"""GPU: transform_many, rotate_many, transpose_many and aej_warp_batch (csrc/warp.hip: k_warp, k_flip, k_transpose) bit-identical to
Pillow's Image.transform, rotate and transpose: against the NumPy model tests/warp_reference.py (itself pinned to live Pillow by
test_warp_host.py) for the shared catalogue and for sizes taken from the kernels' own geometry, and against Pillow's files for the
chains decode -> rotate -> JPEG and scan -> rotate -> PNG.  Exactness is the criterion; every test is one or a few batched calls."""
import ctypes
import io
import os

import numpy as np
import pytest

import warp_reference as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FILTERS = (M.NEAREST, M.BILINEAR, M.BICUBIC)
ROTATE_DEFAULTS = dict(resample=0, expand=False, center=None, translate=None, fillcolor=None)


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def geometry(A):
    return A.geometry.warp_geometry()


def run(A, cases, **extra):
    """catalogue-style cases [(kind, image, kwargs)] -> arrays, in order: one call per kind, every argument one per image"""
    got = [None] * len(cases)
    for kind, fn in (("transform", A.transform_many), ("rotate", A.rotate_many), ("transpose", A.transpose_many)):
        idx = [k for k, c in enumerate(cases) if c[0] == kind]
        if not idx:
            continue
        kws = [dict(ROTATE_DEFAULTS, **cases[k][2]) if kind == "rotate" else dict({"fillcolor": None}, **cases[k][2]) for k in idx]
        if kind == "transpose":
            kws = [{"method": cases[k][2]["method"]} for k in idx]
        args = {name: [kw[name] for kw in kws] for name in kws[0]}
        out = fn([cases[k][1] for k in idx], **args, **(extra if kind != "transpose" else {}))
        for k, o in zip(idx, out):
            got[k] = o
    return got


def check(A, cases, want=None, **extra):
    want = want or [M.model(c, **extra) for c in cases]
    got = [g.cpu().numpy() for g in run(A, cases, **extra)]
    bad = [(k, c[0], c[1].shape, c[2]) for k, (c, g, w) in enumerate(zip(cases, got, want)) if g.dtype != np.uint8 or g.shape != w.shape or not np.array_equal(g, w)]
    assert bad == [], (len(bad), bad[:6])


def tf(a, size, method, data, resample=0, fillcolor=None):
    return ("transform", a, dict(size=size, method=method, data=data, resample=resample, fillcolor=fillcolor))


def test_catalogue(A):
    cases = M.catalogue()
    assert {c[0] for c in cases} == {"transform", "rotate", "transpose"}
    check(A, cases)


def test_premultiply_off_treats_channels_independently(A):
    cases = [c for c in M.catalogue() if c[0] != "transpose" and c[1].ndim == 3 and c[1].shape[2] in (2, 4) and c[2]["resample"] != 0][::3]
    assert len(cases) >= 8
    want = [M.model(c, premultiply=False) for c in cases]
    assert any(not np.array_equal(w, M.model(c)) for c, w in zip(cases, want))
    check(A, cases, want, premultiply=False)


def test_tile_geometry(A, geometry):
    """output sizes one below, at and one above the tile on each axis, two tiles and a pixel, three tiles by three -- every channel
    count and filter --, and sources of one pixel, one row and one column, where every clamp and every repeated row is taken"""
    tw, th = geometry["tile_w"], geometry["tile_h"]
    assert (tw, th) == (32, 8)
    sizes = [(w, h) for w in (tw - 1, tw, tw + 1) for h in (th - 1, th, th + 1)] + [(2 * tw + 1, 2 * th + 1), (3 * tw, 3 * th)]
    cases = []
    for c in (1, 2, 3, 4):
        src = M.image(13, 17, c, 5)
        for f in FILTERS:
            for k, (w, h) in enumerate(sizes):
                s = 15.0 / max(w, h)
                cases.append(tf(src, (w, h), M.AFFINE, (0.9 * s, 0.3 * s, -0.7, -0.3 * s, 0.9 * s, 2.1), f, (k * 20 % 256,) * c))
                if k % 4 == 0:
                    cases.append(tf(src, (w, h), M.AFFINE, (17.0 / w, 0, 0, 0, 13.0 / h, 0), f))                       # the tables under NEAREST
                    cases.append(tf(src, (w, h), M.PERSPECTIVE, (s, 0.01, -1.0, 0.02, s, -0.5, 0.001, 0.002), f))
            for shape in ((1, 1), (1, 40), (40, 1)):
                tiny = M.image(shape[0], shape[1], c, 6)
                W, H = shape[1], shape[0]
                cases.append(tf(tiny, (37, 11), M.AFFINE, (W / 30.0, W / 400.0, -0.1 * W, H / 300.0, H / 9.0, -0.1 * H), f, (9,) * c))
                cases.append(tf(tiny, (9, 37), M.QUAD, (-0.2, -0.2, 0.0, H + 0.1, W * 1.0, H * 1.0, W + 0.3, 0.1), f, (200,) * c))
                cases.append(tf(tiny, (33, 9), M.EXTENT, (-0.5, -0.5, W + 0.5, H + 0.5), f))
    check(A, cases)
    # the transposing kernels at their own tiles
    sw, fb = geometry["swap_w"], geometry["flip_bytes"]
    cases = []
    for c in (1, 2, 3, 4):
        for h, w in ((sw - 1, sw + 1), (sw, 2 * sw), (2 * sw + 1, sw), (1, 1), (1, 40), (40, 1), (5, fb // c + 3), (geometry["flip_rows"] + 1, fb // c)):
            a = M.image(h, w, c, 7)
            cases += [("transpose", a, dict(method=m)) for m in M.TRANSPOSE_NAMES]
    check(A, cases)


def test_identities(A):
    """(alpha is 255 throughout: premultiplying any other alpha loses bits, in Pillow as here)"""
    srcs = [M.image(19, 23, c, 8) for c in (1, 2, 3, 4)]
    for a in srcs[1::2]:
        a[..., -1] = 255
    fills = [(7,), (7, 255), (7, 8, 9), (7, 8, 9, 255)]
    for f in FILTERS:
        got = A.transform_many(srcs, [(23, 19)] * 4, "affine", (1, 0, 0, 0, 1, 0), f)
        rot = A.rotate_many(srcs, 0, f)
        for a, g, r in zip(srcs, got, rot):
            assert np.array_equal(g.cpu().numpy(), a) and np.array_equal(r.cpu().numpy(), a), f
        # integer translations: shifted copies with fill
        got = A.transform_many(srcs, (23, 19), "affine", (1, 0, 4, 0, 1, -3), f, fills)
        for a, g, fill in zip(srcs, got, fills):
            want = np.empty_like(a)
            want[...] = np.array(fill, np.uint8) if a.ndim == 3 else fill[0]
            want[3:, :19] = a[:16, 4:]
            assert np.array_equal(g.cpu().numpy(), want), (f, a.shape)
    r90 = A.rotate_many(srcs, 90, expand=True)
    t90 = A.transpose_many(srcs, "ROTATE_90")
    again = t90
    for _ in range(3):
        again = A.transpose_many(again, 2)
    for a, r, t, g in zip(srcs, r90, t90, again):
        assert np.array_equal(r.cpu().numpy(), t.cpu().numpy()) and np.array_equal(t.cpu().numpy(), np.rot90(a)) and np.array_equal(g.cpu().numpy(), a)


def test_path_selection(A):
    a = M.image(37, 53, 3)
    extent = dict(size=(31, 23), method="extent", data=(-3.5, 2.25, 49.0, 40.0))
    scale = dict(size=(70, 64), method="affine", data=(0.1, 0, 0.25, 0, 0.1, 0.25))
    for kw in (extent, scale):
        assert A.transform_plan(53, 37, kw["size"], kw["method"], kw["data"], "nearest")["path"] == "tables"
    assert A.transform_plan(53, 37, (64, 41), "affine", (0.9, 0.1, 0, -0.1, 0.9, 0), "nearest")["path"] == "fixed"
    nan = (1, 0, -1.5, 0, 1, -0.5, 0, -2)                     # 0 / 0 at the centre of pixel (1, 0); the rest of row 0 divides by zero
    cases = []
    for f in FILTERS:
        cases += [tf(a, resample=f, fillcolor=(1, 2, 3), **extent), tf(a, resample=f, fillcolor=(1, 2, 3), **scale),
                  tf(a, (40, 30), M.PERSPECTIVE, (0.9, 0.1, 2.0, -0.1, 1.0, 3.0, -0.05, 0.01), f, (4, 5, 6)),      # the denominator changes sign
                  tf(a, (17, 15), M.QUAD, (5.0, 8.0, 0.5, 0.5, 5.5, 0.0, 0.0, 7.5), f, (4, 5, 6)),                  # crossed corners
                  tf(a, (12, 9), M.PERSPECTIVE, nan, f, (250, 251, 252))]
    den = -0.05 * (np.arange(40) + 0.5)[None, :] + 0.01 * (np.arange(30) + 0.5)[:, None] + 1
    assert (den > 0).any() and (den < 0).any()
    check(A, cases)
    got = run(A, [c for c in cases if c[2]["data"] == nan])
    for g in got:
        assert g.cpu().numpy()[0].tolist() == [[250, 251, 252]] * 12      # the NaN pixel and its row are filled


def _mixed(n=24):
    """n images mixing channels, sizes, methods, filters and fill colours"""
    datas = {M.AFFINE: (0.8, 0.35, -2.0, -0.35, 0.8, 9.0), M.EXTENT: (-2.0, 1.0, 20.5, 17.0), M.PERSPECTIVE: (1.0, 0.1, -1.0, 0.05, 0.9, 0.5, 0.003, 0.001),
             M.QUAD: (-1.0, 2.0, 1.5, 25.0, 30.0, 20.0, 26.0, -1.0)}
    cases = []
    for k in range(n):
        c = 1 + k % 4
        method = (M.AFFINE, M.EXTENT, M.PERSPECTIVE, M.QUAD)[(k // 4) % 4]
        cases.append(tf(M.image(11 + 3 * k, 40 - k, c, k), (20 + 2 * k, 37 - k), method, datas[method], FILTERS[k % 3], M.FILLS[c][k % 3]))
    return cases


def test_one_call_with_mixed_arguments(A):
    cases = _mixed(24)
    assert len({(c[1].shape, c[2]["size"]) for c in cases}) == 24
    got = run(A, cases)
    st = got[0].untyped_storage().data_ptr()
    pos = got[0].data_ptr()
    for c, g in zip(cases, got):
        assert g.is_contiguous() and g.untyped_storage().data_ptr() == st and g.data_ptr() == pos      # one packed allocation, in input order
        pos += g.numel()
        assert np.array_equal(g.cpu().numpy(), M.model(c)), c[2]


def _file(folder, name):
    with open(os.path.join(GOLDEN, folder, name + ".jpg"), "rb") as f:
        return f.read()


def test_chains_equal_pillow(A):
    """JPEG decode -> rotate_many(7, bicubic, expand=True) -> standard_jpeg_encode_many gives the bytes of Pillow's open(); rotate();
    save(), and a grey scan -> rotate_many(-1.5, bilinear, fillcolor=255) -> png_encode_many(entropy="host") gives Pillow's PNG file."""
    from PIL import Image
    files = [_file("jpegdec", "lena_64x64_420_q75"), _file("jpegdec", "buildings_96x128_crop_q95")]
    rot = A.rotate_many(A.standard_jpeg_decode_many(files), 7, "bicubic", expand=True)
    got = A.standard_jpeg_encode_many(rot, 85)
    for k, (d, g, r) in enumerate(zip(files, got, rot)):
        want = Image.open(io.BytesIO(d)).convert("RGB").rotate(7, Image.Resampling.BICUBIC, expand=True)
        assert np.array_equal(r.cpu().numpy(), np.asarray(want)), k
        buf = io.BytesIO()
        want.save(buf, "JPEG", quality=85)
        assert g == buf.getvalue(), k
    scan = M.image(61, 47, 1, 9)
    (deskewed,) = A.rotate_many([scan], -1.5, "bilinear", fillcolor=255)
    (png,) = A.png_encode_many([deskewed], entropy="host")
    buf = io.BytesIO()
    Image.fromarray(scan).rotate(-1.5, Image.Resampling.BILINEAR, fillcolor=255).save(buf, "PNG")
    assert png == buf.getvalue()


def test_c_entry_refusals_and_untouched_bytes(A):
    """aej_warp_batch itself: exactly the image's bytes written; workspace too small, source outside the input, source inside the
    output and n < 1, each with its code and text"""
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import WarpDesc, get_context
    ctx = get_context(0)
    lib = ctx.lib
    a = M.image(20, 30, 3, 1)
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    n = a.size
    buf[:n] = torch.from_numpy(a).cuda().reshape(-1)
    d = (WarpDesc * 1)()
    d[0].src_offset, d[0].dst_offset, d[0].src_w, d[0].src_h, d[0].dst_w, d[0].dst_h, d[0].channels = 0, 32, 30, 20, 25, 16, 3
    d[0].path, d[0].filter = 3, 2                             # AEJ_WARP_AFFINE, bilinear
    data = (1.1, 0.2, -1.0, -0.2, 1.1, 3.0)
    d[0].coef[:6] = data
    d[0].fill[:3] = (9, 8, 7)
    m = 25 * 16 * 3
    dst = torch.full((m + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    nws = int(lib.aej_warp_workspace_bytes(ctx.handle, ctypes.addressof(d), 1))
    assert nws > 0
    ws = ctx.workspace(max(nws, 256))

    def call(count, src_ptr, sb, dst_ptr, db, wsb):
        rc = lib.aej_warp_batch(ctx.handle, ctypes.addressof(d), count, src_ptr, ctypes.c_uint64(sb), dst_ptr, ctypes.c_uint64(db), ws.data_ptr(),
                                ctypes.c_uint64(wsb))
        return rc, lib.aej_last_error(ctx.handle)

    rc, _ = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 64, ws.numel())
    assert rc == 0
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.array_equal(out[32:32 + m].reshape(16, 25, 3), M.transform(a, (25, 16), M.AFFINE, data, M.BILINEAR, (9, 8, 7)))
    assert (out[:32] == 0xA5).all() and (out[32 + m:] == 0xA5).all()
    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 64, nws - 1)
    assert rc == -4 and b"workspace too small" in msg
    rc, msg = call(1, buf.data_ptr(), n - 1, dst.data_ptr(), m + 64, ws.numel())
    assert rc == -1 and b"image 0: source outside the input" in msg
    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 31, ws.numel())
    assert rc == -1 and b"image 0: image outside the output" in msg
    rc, msg = call(1, buf.data_ptr(), n, buf.data_ptr() + n - 1, m + 64, ws.numel())
    assert rc == -1 and b"image 0: source inside the output" in msg
    for count in (0, -1):
        rc, msg = call(count, buf.data_ptr(), n, dst.data_ptr(), m + 64, ws.numel())
        assert rc == -1 and b"no images" in msg
    d[0].path, d[0].filter = 3, 0                             # NEAREST beyond the fixed-point guard
    d[0].coef[:6] = (2000.0, 1.0, 0.0, 0.0, 1.0, 0.0)
    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 64, ws.numel())
    assert rc == -5 and b"image 0:" in msg and lib.aej_warp_workspace_bytes(ctx.handle, ctypes.addressof(d), 1) == 0
    d[0].path = 1                                             # AEJ_WARP_TABLES is what the library resolves to, not an input
    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 64, ws.numel())
    assert rc == -1 and b"image 0: unknown path" in msg
    torch.cuda.synchronize()
    assert (dst.cpu().numpy()[32 + m:] == 0xA5).all()
