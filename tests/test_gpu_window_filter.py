"""GPU: filter_many and aej_window_batch (csrc/window.hip: k_window_conv, k_window_rank, k_window_mode) bit-identical to Pillow's
Kernel (the ten built-ins among them), rank and mode filters: against the NumPy models tests/window_filter_reference.py (themselves
pinned to Pillow by test_window_filter_host.py) for the shared catalogue and for sizes taken from the kernels' own geometry, and
against Pillow's files for the chains thumbnail -> SHARPEN -> JPEG and MedianFilter -> PNG.  Exactness is the criterion; every test is
one or a few batched calls."""
import io
import os

import numpy as np
import pytest

import filter_reference as B
import window_filter_reference as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def geometry(A):
    return A.filters.window_geometry()


def _model(a, f):
    return B.model(a, f) if getattr(f, "name", None) in B.PASSES else M.model(a, f)


def _check(A, cases, want=None):
    """cases [(image, filter)] through filter_many in one call, each against the model"""
    want = want or [_model(a, f) for a, f in cases]
    got = [g.cpu().numpy() for g in A.filter_many([a for a, _ in cases], [f for _, f in cases])]
    bad = [(k, a.shape, f) for k, ((a, f), g, w) in enumerate(zip(cases, got, want)) if g.dtype != np.uint8 or g.shape != w.shape or not np.array_equal(g, w)]
    assert bad == [], (len(bad), bad[:8])


def test_catalogue(A):
    cases = M.catalogue()
    want = [M.model(a, f) for a, f in cases]
    M.check_catalogue(cases, want)
    _check(A, cases, want)


def _some_filters():
    b = {f.name: f for f in M.builtins()}
    return {"Kernel": [b["Sharpen"], b["Smooth More"], M.kernel_filters()[14], M.kernel_filters()[17]],
            "Rank": [M.Rank(3, 4), M.Rank(3, 0), M.Rank(5, 24), M.Rank(7, 16), M.Rank(15, 112), M.Rank(15, 223)],
            "Mode": [M.Mode(3), M.Mode(5), M.Mode(6), M.Mode(7)]}


def test_sizes_at_every_kernel_constant(A, geometry):
    """one below, at and one above the tile on each axis; two tiles and a pixel each way; three tiles and 9 wide, so that there are
    tiles with no image border; rank 15 and mode 7 on images narrower and shorter than their halo"""
    tw, th = geometry["tile_w"], geometry["tile_h"]
    filters = _some_filters()
    assert len(M.kernel_filters()[14].filterargs[3]) == 9 and len(M.kernel_filters()[17].filterargs[3]) == 25
    assert geometry["rank_halo"] == 7 and geometry["mode_halo"] == 3 and geometry["kernel_halo"] == 2
    cases = []
    for c in (1, 2, 3, 4):
        shapes = [(5, w) for w in (tw - 1, tw, tw + 1)] + [(h, 6) for h in (th - 1, th, th + 1)] + [(2 * th + 1, 2 * tw + 1), (th + 5, 3 * tw + 9)]
        for kind, fs in filters.items():
            for k, shape in enumerate(shapes):
                a = M.image(shape, c, seed=3, levels=8 if kind == "Mode" else 256)
                pick = fs if k >= 6 else [fs[k % len(fs)], fs[(k + 1) % len(fs)]]
                cases += [(a, f) for f in pick]
        for shape in ((1, 40), (40, 1), (3, 9)):
            cases += [(M.image(shape, c, seed=4), M.Rank(15, 112)), (M.image(shape, c, seed=4), M.Rank(15, 0)), (M.image(shape, c, seed=4, levels=8), M.Mode(7))]
    _check(A, cases)


def test_kernel_border_rule(A):
    """w or h equal to k - 1, k and k + 1, for both k: an image smaller than the kernel is a copy, and so is every sample within r of an edge"""
    filters = _some_filters()["Kernel"] + [M.Kernel(3, [1] * 9, 1, 0), M.Kernel(5, [1] * 25, 1, 0)]      # (the last two: gain 9 and 25, nothing like a copy)
    cases, copies = [], 0
    for k in (3, 5):
        for n in (k - 1, k, k + 1):
            for c, shape in ((1, (n, 9)), (3, (9, n)), (4, (n, n)), (2, (n, 70))):
                a = M.image(shape, c, seed=k)
                for f in filters:
                    cases.append((a, f))
                    copies += f.filterargs[0][0] > n and np.array_equal(M.model(a, f), a)
    assert copies >= 8
    _check(A, cases)


def test_flat_images_and_checkerboard(A):
    filters = M.rank_filters() + M.mode_filters() + [M.delta(3, 4), M.delta(5, 12), M.builtins()[0]]
    assert M.builtins()[0].name == "Sharpen" and sum(M.kernel_args(M.builtins()[0])[1], np.float32(0)) == 1
    cases = []
    for v in (0, 1, 127, 128, 254, 255):
        for c in (1, 3):
            flat = np.full((37, 70) + ((c,) if c > 1 else ()), v, np.uint8)
            cases += [(flat, f) for f in filters]
    want = [a for a, _ in cases]                          # a flat image stays as it is under each of these
    assert all(np.array_equal(M.model(a, f), a) for a, f in cases[::7])
    _check(A, cases, want)
    y, x = np.mgrid[0:45, 0:67]
    board = (((x + y) % 2) * 255).astype(np.uint8)
    cases = [(b, f) for b in (board, np.stack([board, 255 - board, board], -1)) for f in (M.Rank(3, 0), M.Rank(3, 8), M.Rank(3, 4))]
    _check(A, cases)


def _mixed(n=24):
    """blurs and all three window kinds alternating, our objects and plain data"""
    b = M.builtins()
    filters = [B.Spec("GaussianBlur", 2), b[0], M.Rank(3, 4), M.Mode(3), B.Spec("UnsharpMask", 2, 150, 3), b[2], M.Rank(5, 0), M.Mode(5),
               B.Spec("BoxBlur", 20), M.kernel_filters()[15], M.Rank(15, 200), M.Mode(2)]
    return [(M.image((9 + 11 * (k % 7), 150 - 13 * (k % 9)), 1 + k % 4, seed=k, levels=8 if k % 4 == 3 else 256), filters[k % len(filters)]) for k in range(n)]


def test_batch_equals_single_calls(A):
    import torch
    cases = _mixed()
    sources = [torch.from_numpy(a).cuda() if k % 3 == 0 else a for k, (a, _) in enumerate(cases)]
    before = [s.clone() if isinstance(s, torch.Tensor) else s.copy() for s in sources]
    together = A.filter_many(sources, [f for _, f in cases])
    for k, ((a, f), t) in enumerate(zip(cases, together)):
        alone = A.filter_many([a], f)[0]
        assert tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy(), alone.cpu().numpy()), (k, a.shape, f)
        assert np.array_equal(alone.cpu().numpy(), _model(a, f)), (k, a.shape, f)
    st = together[0].untyped_storage()
    assert all(t.untyped_storage().data_ptr() == st.data_ptr() and t.is_contiguous() and t.is_cuda for t in together)
    spans = [(t.data_ptr(), t.data_ptr() + t.numel()) for t in together]
    assert spans == sorted(spans) and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))      # in input order, not overlapping
    for s, b in zip(sources, before):
        if isinstance(s, torch.Tensor):
            xs = s.untyped_storage()
            assert st.data_ptr() + st.nbytes() <= xs.data_ptr() or xs.data_ptr() + xs.nbytes() <= st.data_ptr()      # no output lies in an input
            assert torch.equal(s, b)
        else:
            assert np.array_equal(s, b)


def test_sources_of_every_kind_and_one_filter_for_all(A):
    import torch
    from PIL import ImageFilter
    rng = np.random.default_rng(4)
    arrays = [rng.integers(0, 256, s, dtype=np.uint8) // 32 * 32 for s in ((40, 50, 3), (33, 20), (21, 64, 4), (50, 37, 2), (64, 48, 3), (31, 31))]
    wide = torch.from_numpy(rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)).cuda()
    view = wide[3:60:2, 5:90, :]                          # a non-contiguous device view
    assert not view.is_contiguous()
    images = [arrays[0], torch.from_numpy(arrays[1].copy()), torch.from_numpy(arrays[2]).cuda(), arrays[3], view, torch.from_numpy(arrays[4]).cuda(),
              torch.from_numpy(arrays[5])[::2, 1:]]
    plain = [arrays[0], arrays[1], arrays[2], arrays[3], view.cpu().numpy(), arrays[4], arrays[5][::2, 1:]]
    before = [x.clone() if isinstance(x, torch.Tensor) else x.copy() for x in images] + [wide.clone()]
    for f, spec in ((ImageFilter.SHARPEN, M.builtins()[0]), (ImageFilter.MedianFilter(3), M.Rank(3, 4)), (A.ModeFilter(3), M.Mode(3))):
        got = A.filter_many(images, f)
        assert len(got) == len(images)
        for g, a in zip(got, plain):
            assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == a.shape
            assert np.array_equal(g.cpu().numpy(), M.model(a, spec))
        st = got[0].untyped_storage()
        assert all(g.untyped_storage().data_ptr() == st.data_ptr() for g in got)
        for x in images:                                  # no output lies in an input
            if isinstance(x, torch.Tensor) and x.is_cuda:
                xs = x.untyped_storage()
                assert st.data_ptr() + st.nbytes() <= xs.data_ptr() or xs.data_ptr() + xs.nbytes() <= st.data_ptr()
    for x, b in zip(images + [wide], before):
        assert np.array_equal(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x), np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b))
    t = torch.from_numpy(arrays[0]).cuda()
    t.jpeg_comment = b"kept"
    got = A.filter_many([t, torch.from_numpy(arrays[4]).cuda(), t], [A.SHARPEN, A.MedianFilter(3), A.GaussianBlur(1)])
    assert got[0].jpeg_comment == b"kept" and not hasattr(got[1], "jpeg_comment") and got[2].jpeg_comment == b"kept"


def test_c_entry_refusals_and_untouched_bytes(A):
    """aej_window_batch itself: bounds named by image, exactly the image's bytes written, the cases that are not built"""
    import ctypes

    import torch
    from adaptive_edge_aware_jpeg_amd._lib import WindowDesc, get_context
    ctx = get_context(0)
    lib = ctx.lib
    a = M.image((20, 30), 3, seed=1, levels=8)
    src = torch.from_numpy(a).cuda().reshape(-1)
    n = src.numel()
    d = (WindowDesc * 1)()
    d[0].src_offset, d[0].dst_offset, d[0].width, d[0].height, d[0].channels = 0, 32, 30, 20, 3
    dst = torch.empty((n + 64,), dtype=torch.uint8, device="cuda")
    sharpen = M.builtins()[0]

    def call(kind, size, rank, sb, db, scale=16.0, offset=0.0):
        d[0].kind, d[0].size, d[0].rank, d[0].scale, d[0].offset = kind, size, rank, scale, offset
        d[0].kernel[:9] = [float(v) for v in sharpen.filterargs[3]]
        nws = int(lib.aej_window_workspace_bytes(ctx.handle, ctypes.addressof(d), 1))
        ws = ctx.workspace(max(nws, 256))
        rc = lib.aej_window_batch(ctx.handle, ctypes.addressof(d), 1, src.data_ptr(), ctypes.c_uint64(sb), dst.data_ptr(), ctypes.c_uint64(db),
                                  ws.data_ptr(), ctypes.c_uint64(ws.numel()))
        return rc, nws, lib.aej_last_error(ctx.handle)

    for kind, size, rank, spec in ((0, 3, 0, sharpen), (1, 5, 7, M.Rank(5, 7)), (2, 3, 0, M.Mode(3))):      # AEJ_WINDOW_KERNEL, _RANK, _MODE
        dst.fill_(0xA5)
        rc, nws, _ = call(kind, size, rank, n, n + 64)
        assert rc == 0 and nws > 0
        torch.cuda.synchronize()
        out = dst.cpu().numpy()
        assert np.array_equal(out[32:32 + n].reshape(a.shape), M.model(a, spec))
        assert (out[:32] == 0xA5).all() and (out[32 + n:] == 0xA5).all()
        rc, _, msg = call(kind, size, rank, n - 1, n + 64)
        assert rc == -1 and b"image 0: source outside" in msg
        rc, _, msg = call(kind, size, rank, n, n + 31)
        assert rc == -1 and b"image 0: image outside" in msg
    for kind, size, rank, kw in ((1, 17, 5, {}), (2, 8, 0, {}), (0, 3, 0, {"scale": float(2.0 ** -101)}), (0, 3, 0, {"offset": float(2.0 ** 101)})):
        rc, nws, msg = call(kind, size, rank, n, n + 64, **kw)
        assert rc == -5 and nws == 0 and b"image 0:" in msg, (kind, size, kw)
    for kind, size, rank, kw in ((0, 4, 0, {}), (0, 3, 0, {"scale": 0.0}), (0, 3, 0, {"offset": float("inf")}), (1, 4, 0, {}), (1, 3, 9, {}), (1, 3, -1, {}), (2, 0, 0, {}),
                                 (3, 3, 0, {})):
        rc, nws, msg = call(kind, size, rank, n, n + 64, **kw)
        assert rc == -1 and nws == 0 and b"image 0:" in msg, (kind, size, kw)


def _file(folder, name):
    with open(os.path.join(GOLDEN, folder, name + ".jpg"), "rb") as f:
        return f.read()


def test_chains_equal_pillow(A):
    """standard_jpeg_thumbnail_many -> filter_many(SHARPEN) -> standard_jpeg_encode_many gives the bytes of Pillow's thumbnail();
    filter(ImageFilter.SHARPEN); save() -- the COM segment of the second file included --, and MedianFilter(3) -> png_encode_many gives
    Pillow's PNG file."""
    from PIL import Image, ImageFilter
    files = [_file("jpegdec", "lena_64x64_420_q75"), _file("jpegdec", "peppers_24x40_exif_com_q75"), _file("jpegdec", "buildings_96x128_crop_q95")]
    assert b"a COM segment" in files[1]
    thumbs = A.standard_jpeg_thumbnail_many(files, (48, 40))
    sharp = A.filter_many(thumbs, ImageFilter.SHARPEN)
    st = sharp[0].untyped_storage().data_ptr()
    assert all(s.is_contiguous() and s.untyped_storage().data_ptr() == st for s in sharp)      # the encoder's packed-source shortcut applies
    assert sharp[1].jpeg_comment == b"a COM segment"
    got = A.standard_jpeg_encode_many(sharp, 85)
    median = A.filter_many(thumbs, A.MedianFilter(3))
    pngs = A.png_encode_many(median, entropy="host")
    for k, (d, g, s, p) in enumerate(zip(files, got, sharp, pngs)):
        im = Image.open(io.BytesIO(d))
        im.thumbnail((48, 40))
        want = im.filter(ImageFilter.SHARPEN)
        assert np.array_equal(s.cpu().numpy(), np.asarray(want)), k
        buf = io.BytesIO()
        want.save(buf, "JPEG", quality=85)
        assert g == buf.getvalue(), k
        buf = io.BytesIO()
        im.filter(ImageFilter.MedianFilter(3)).save(buf, "PNG")
        assert p == buf.getvalue(), k
