"""GPU: filter_many and aej_filter_batch (csrc/filter.hip: k_filter_tile, k_filter_rows, k_filter_cols) bit-identical to Pillow's
BoxBlur / GaussianBlur / UnsharpMask, on both kernel paths: against the NumPy model tests/filter_reference.py (itself pinned to Pillow by
test_filter_host.py) for the shared catalogue and for sizes taken from the kernels' own geometry, and against Pillow's files for the
chain thumbnail -> filter -> save.  Exactness is the criterion; every test is one or a few batched calls."""
import io
import os

import numpy as np
import pytest

import filter_reference as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PATHS = ("passes", "fused", "auto")
Spec = M.Spec


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def geometry(A):
    return A.filters.filter_geometry()


@pytest.fixture(scope="module")
def catalogue():
    """the shared cases with the model's answer, computed once"""
    return [(a, spec, M.model(a, spec)) for a, spec in M.catalogue()]


def _fits(A, spec, limit):
    """the fused kernel takes this filter"""
    xy = M.radii_of(spec.radius)
    return max(A.filters._halo(A.filters.filter_plan(spec.name, float(xy[0]), float(xy[1])))) <= limit


def _check(A, geometry, cases, paths=PATHS, want=None):
    """cases [(image, spec)] through filter_many in one call per path, each against the model; -> the cases the fused path took"""
    want = want or [M.model(a, s) for a, s in cases]
    fused = [k for k, (_, s) in enumerate(cases) if _fits(A, s, geometry["max_halo"])]
    for path in paths:
        pick = fused if path == "fused" else range(len(cases))
        if not len(pick):
            continue
        got = A.filter_many([cases[k][0] for k in pick], [cases[k][1] for k in pick], _path=path)
        got = [g.cpu().numpy() for g in got]
        bad = [(path, cases[k][0].shape, cases[k][1]) for k, g in zip(pick, got)
               if g.dtype != np.uint8 or g.shape != want[k].shape or not np.array_equal(g, want[k])]
        assert bad == [], (len(bad), bad[:8])
    return fused


@pytest.mark.parametrize("path", PATHS)
def test_catalogue(A, geometry, catalogue, path):
    cases = [(a, s) for a, s, _ in catalogue]
    fused = _check(A, geometry, cases, (path,), [w for _, _, w in catalogue])
    assert 0 < len(fused) < len(cases)               # both sides of the halo limit are in the catalogue


def test_sizes_at_every_kernel_constant(A, geometry):
    """one below, at and one above the tile, the span, the band and the workgroup's byte columns, on both axes; an image of two tiles
    and a pixel each way; the largest fused halo and one above it"""
    g = geometry
    tw, th, halo, span, band, colb = (g[k] for k in ("tile_w", "tile_h", "max_halo", "row_span", "col_band", "col_bytes"))
    shapes = [(2 * th + 1, 2 * tw + 1, c) for c in (1, 2, 3, 4)]
    shapes += [(5, w, 3) for w in (tw - 1, tw, tw + 1)] + [(h, 6, 3) for h in (th - 1, th, th + 1)]
    shapes += [(3, w, c) for c in (1, 3) for w in (span - 1, span, span + 1)]
    shapes += [(h, 5, c) for c in (1, 4) for h in (band - 1, band, band + 1, 2 * band + 1)]
    shapes += [(3, w, c) for c in (1, 2, 3, 4) for w in (colb // c - 1, colb // c, colb // c + 1, -(-colb // c) + 1)]
    at_halo = [Spec("BoxBlur", halo - 1), Spec("BoxBlur", (halo - 1 + 0.75, 0)), Spec("GaussianBlur", (0, 5.4)), Spec("UnsharpMask", 5.4, 130, 2)]
    above = [Spec("BoxBlur", halo), Spec("BoxBlur", (0, halo + 0.25)), Spec("GaussianBlur", 6.5), Spec("UnsharpMask", 6.5, 130, 2)]
    assert all(_fits(A, s, halo) for s in at_halo) and not any(_fits(A, s, halo) for s in above)
    p = A.filters.filter_plan("GaussianBlur", 5.4, 5.4)
    assert 3 * (p["r"][0] + 1) in (halo - 1, halo)
    common = [Spec("GaussianBlur", 2), Spec("UnsharpMask", 2, 150, 3), Spec("BoxBlur", 5), Spec("GaussianBlur", (20, 3)), Spec("BoxBlur", (0.4, 70))]
    cases = []
    for k, (h, w, c) in enumerate(shapes):
        a = M.image((h, w), c, seed=5)
        specs = common + at_halo + above if k < 4 else [common[k % 5], common[(k + 2) % 5], at_halo[k % 4], above[k % 4]]
        cases += [(a, s) for s in specs]
    fused = _check(A, geometry, cases)
    assert len(fused) >= len(cases) // 3


def test_tiles_without_an_image_border(A, geometry):
    """images three tiles and a bit wide, so that the fused kernel has tiles whose whole halo lies inside the image beside those that
    clamp on one side or on both, for every r it takes (0 to 4 for its Gaussians, up to 15 for a box)"""
    tw, th = geometry["tile_w"], geometry["tile_h"]
    specs = [Spec("GaussianBlur", 0.5), Spec("GaussianBlur", 2), Spec("GaussianBlur", 3), Spec("GaussianBlur", (4.2, 1)), Spec("GaussianBlur", 5.4),
             Spec("GaussianBlur", (5.4, 0)), Spec("BoxBlur", 0.3), Spec("BoxBlur", 1), Spec("BoxBlur", (4.9, 2)), Spec("BoxBlur", (5, 0)), Spec("BoxBlur", 15),
             Spec("UnsharpMask", 2, 150, 3), Spec("UnsharpMask", 5.4, 70, 0)]
    assert sorted({A.filters.filter_plan(s.name, *(float(v) for v in M.radii_of(s.radius)))["r"][0] for s in specs}) == [0, 1, 2, 3, 4, 5, 15]
    cases = [(M.image((th + 5, 3 * tw + 9 + c), c, seed=8), s) for c in (1, 2, 3, 4) for s in specs]
    cases += [(M.image((2 * th + 3, 4 * tw), 3, seed=6), s) for s in specs]
    fused = _check(A, geometry, cases, ("fused", "auto"))
    assert len(fused) == len(cases)


def test_narrow_lines(A, geometry):
    """lines shorter than, as long as and just longer than the window, on each axis with the other axis large; r = 1024 on 5 x 9"""
    cases = []
    for r in (1, 3, 17):
        for n in sorted({1, 2, r, r + 1, r + 2, 2 * r + 1, 2 * r + 2}):
            for c, (h, w) in ((1, (70, n)), (3, (n, 70)), (4, (70, n)), (2, (n, 70))):
                a = M.image((h, w), c, seed=r)
                cases += [(a, Spec("BoxBlur", r)), (a, Spec("BoxBlur", (r + 0.5, r + 0.25))), (a, Spec("GaussianBlur", (r, 0.7 * r))),
                          (a, Spec("UnsharpMask", r, 90, 1))]
    for c in (1, 3):
        a = M.image((5, 9), c, seed=9)
        cases += [(a, Spec("BoxBlur", 1024)), (a, Spec("BoxBlur", (1024.9, 0))), (a, Spec("BoxBlur", (0, 1024.5))), (a, Spec("GaussianBlur", 1020)),
                  (a, Spec("UnsharpMask", 1000, 200, 0))]
    _check(A, geometry, cases)


def test_saturation_and_rounding(A, geometry):
    cases = []
    filters = [Spec("BoxBlur", 2.5), Spec("GaussianBlur", 3), Spec("GaussianBlur", 30), Spec("UnsharpMask", 2, 150, 3), Spec("UnsharpMask", 2, -400, -1),
               Spec("BoxBlur", (0.01, 0)), Spec("BoxBlur", (0, 1024.99)), Spec("BoxBlur", (1e-30, 1e-9))]      # (the last: a weight of 2^24 itself)
    for c in (1, 3):
        for v in (0, 255, 1, 127, 128, 254):
            flat = np.full((37, 41) + ((c,) if c > 1 else ()), v, np.uint8)
            for s in filters:
                cases.append((flat, s))
    want = [a for a, _ in cases]                      # a flat image stays as it is under every filter
    assert all(np.array_equal(M.model(a, s), a) for a, s in cases[::5])
    _check(A, geometry, cases, want=want)
    y, x = np.mgrid[0:45, 0:67]
    boards = [(((x + y) % 2) * 255).astype(np.uint8), (((x // 3 + y // 2) % 2) * 255).astype(np.uint8)]
    boards += [np.stack([b, 255 - b, b], -1) for b in boards]
    sharp = [Spec("UnsharpMask", 1, 100000, 0), Spec("UnsharpMask", 3, -100000, 0), Spec("UnsharpMask", 2, 1000000, 40), Spec("UnsharpMask", 2, -1000000, -7),
             Spec("UnsharpMask", 2, 150, 255), Spec("UnsharpMask", 2, 150, 254), Spec("UnsharpMask", 0, 500, -1), Spec("UnsharpMask", 9, 99, 0)]
    cases = [(b, s) for b in boards + [M.image((45, 67), 3, seed=2)] for s in filters + sharp]
    got = [M.model(a, s) for a, s in cases]
    assert any(g.min() == 0 and g.max() == 255 and not np.array_equal(g, a) for g, (a, _) in zip(got, cases))      # both clips are met
    _check(A, geometry, cases, want=got)


def _mixed(n=24):
    specs = [Spec("GaussianBlur", 2), Spec("UnsharpMask", 2, 150, 3), Spec("BoxBlur", 5), Spec("GaussianBlur", 20), Spec("BoxBlur", (0, 3)),
             Spec("UnsharpMask", 7, 60, 5), Spec("BoxBlur", 0), Spec("GaussianBlur", (1.5, 0))]
    return [(M.image((9 + 11 * (k % 7), 150 - 13 * (k % 9)), 1 + k % 4, seed=k), specs[k % len(specs)]) for k in range(n)]


@pytest.mark.parametrize("path", PATHS)
def test_batch_equals_single_calls(A, geometry, path):
    cases = _mixed()
    if path == "fused":
        cases = [c for c in cases if _fits(A, c[1], geometry["max_halo"])]
    together = A.filter_many([a for a, _ in cases], [s for _, s in cases], _path=path)
    for k, ((a, s), t) in enumerate(zip(cases, together)):
        alone = A.filter_many([a], s, _path=path)[0]
        assert tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy(), alone.cpu().numpy()), (k, a.shape, s)
        assert np.array_equal(alone.cpu().numpy(), M.model(a, s)), (k, a.shape, s)
    st = together[0].untyped_storage().data_ptr()
    assert all(t.untyped_storage().data_ptr() == st and t.is_contiguous() and t.is_cuda for t in together)
    spans = sorted((t.data_ptr(), t.data_ptr() + t.numel()) for t in together)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_sources_of_every_kind_and_one_filter_for_all(A):
    import torch
    from PIL import ImageFilter
    rng = np.random.default_rng(4)
    arrays = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((40, 50, 3), (33, 20), (21, 64, 4), (50, 37, 2), (64, 48, 3), (31, 31))]
    wide = torch.from_numpy(rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)).cuda()
    view = wide[3:60:2, 5:90, :]                     # a non-contiguous device view
    assert not view.is_contiguous()
    images = [arrays[0], torch.from_numpy(arrays[1].copy()), torch.from_numpy(arrays[2]).cuda(), arrays[3], view, torch.from_numpy(arrays[4]).cuda(),
              torch.from_numpy(arrays[5])[::2, 1:]]
    plain = [arrays[0], arrays[1], arrays[2], arrays[3], view.cpu().numpy(), arrays[4], arrays[5][::2, 1:]]
    before = [x.clone() if isinstance(x, torch.Tensor) else x.copy() for x in images] + [wide.clone()]
    for f in (A.UnsharpMask(1, 120, 2), ImageFilter.GaussianBlur((3, 1)), A.BoxBlur(np.float32(40))):
        for path in ("auto", "passes"):
            got = A.filter_many(images, f, _path=path)
            assert len(got) == len(images)
            for g, a in zip(got, plain):
                assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == a.shape
                assert np.array_equal(g.cpu().numpy(), M.model(a, f))
            st = got[0].untyped_storage()
            assert all(g.untyped_storage().data_ptr() == st.data_ptr() for g in got)
            for x in images:                                     # no output lies in an input
                if isinstance(x, torch.Tensor) and x.is_cuda:
                    xs = x.untyped_storage()
                    assert st.data_ptr() + st.nbytes() <= xs.data_ptr() or xs.data_ptr() + xs.nbytes() <= st.data_ptr()
    for x, b in zip(images + [wide], before):
        assert np.array_equal(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x), np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b))
    t = torch.from_numpy(arrays[0]).cuda()
    t.jpeg_comment = b"kept"
    got = A.filter_many([t, torch.from_numpy(arrays[4]).cuda()], A.GaussianBlur(1))
    assert got[0].jpeg_comment == b"kept" and not hasattr(got[1], "jpeg_comment")


def test_c_entry_refusals_and_untouched_bytes(A):
    """aej_filter_batch itself: bounds named by image, and exactly the image's bytes written"""
    import ctypes

    import torch
    from adaptive_edge_aware_jpeg_amd._lib import FilterDesc, get_context
    ctx = get_context(0)
    lib = ctx.lib
    a = M.image((20, 30), 3, seed=1)
    src = torch.from_numpy(a).cuda().reshape(-1)
    n = src.numel()
    d = (FilterDesc * 1)()
    d[0].src_offset, d[0].dst_offset, d[0].width, d[0].height, d[0].channels = 0, 32, 30, 20, 3
    d[0].kind, d[0].percent, d[0].threshold = 2, 150, 3
    dst = torch.empty((n + 64,), dtype=torch.uint8, device="cuda")

    def call(path, radius, sb, db):
        d[0].xradius = d[0].yradius = radius
        nws = int(lib.aej_filter_workspace_bytes(ctx.handle, ctypes.addressof(d), 1, path))
        ws = ctx.workspace(max(nws, 256))
        rc = lib.aej_filter_batch(ctx.handle, ctypes.addressof(d), 1, path, src.data_ptr(), ctypes.c_uint64(sb), dst.data_ptr(), ctypes.c_uint64(db),
                                  ws.data_ptr(), ctypes.c_uint64(ws.numel()))
        return rc, nws, lib.aej_last_error(ctx.handle)

    for path in (0, 1, 2):                           # AEJ_FILTER_AUTO, _FUSED, _PASSES
        dst.fill_(0xA5)
        rc, nws, _ = call(path, 2.0, n, n + 64)
        assert rc == 0 and nws > 0
        torch.cuda.synchronize()
        out = dst.cpu().numpy()
        assert np.array_equal(out[32:32 + n].reshape(a.shape), M.model(a, Spec("UnsharpMask", 2, 150, 3)))
        assert (out[:32] == 0xA5).all() and (out[32 + n:] == 0xA5).all()
        rc, _, msg = call(path, 2.0, n - 1, n + 64)
        assert rc == -1 and b"image 0: source outside" in msg
        rc, _, msg = call(path, 2.0, n, n + 31)
        assert rc == -1 and b"image 0: image outside" in msg
        rc, nws, msg = call(path, 1100.0, n, n + 64)
        assert rc == -5 and nws == 0 and b"image 0:" in msg
    assert call(2, 6.5, n, n + 64)[0] == 0
    rc, nws, msg = call(1, 6.5, n, n + 64)
    assert rc == -1 and nws == 0 and b"image 0: filter beyond" in msg


def _file(folder, name):
    with open(os.path.join(GOLDEN, folder, name + ".jpg"), "rb") as f:
        return f.read()


def test_chain_thumbnail_filter_save_equals_pillow(A):
    """standard_jpeg_thumbnail_many -> filter_many(UnsharpMask(1, 120, 2)) -> standard_jpeg_encode_many gives the bytes of Pillow's
    thumbnail(); filter(); save() -- the COM segment of the second file included -- and the encoder reads the filtered images where
    they lie."""
    from PIL import Image, ImageFilter
    files = [_file("jpegdec", "lena_64x64_420_q75"), _file("jpegdec", "peppers_24x40_exif_com_q75"), _file("jpegdec", "buildings_96x128_crop_q95")]
    assert b"a COM segment" in files[1]
    thumbs = A.standard_jpeg_thumbnail_many(files, (48, 40))
    sharp = A.filter_many(thumbs, A.UnsharpMask(1, 120, 2))
    st = sharp[0].untyped_storage().data_ptr()
    assert all(s.is_contiguous() and s.untyped_storage().data_ptr() == st for s in sharp)      # the encoder's packed-source shortcut applies
    assert sharp[1].jpeg_comment == b"a COM segment"
    got = A.standard_jpeg_encode_many(sharp, 85)
    for k, (d, g, s) in enumerate(zip(files, got, sharp)):
        im = Image.open(io.BytesIO(d))
        im.thumbnail((48, 40))
        im = im.filter(ImageFilter.UnsharpMask(1, 120, 2))
        assert np.array_equal(s.cpu().numpy(), np.asarray(im)), k
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=85)
        assert g == buf.getvalue(), k
