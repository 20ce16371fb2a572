"""GPU: filter_many and aej_lut3d_batch (csrc/lut3d.hip: k_lut3d) bit-identical to Pillow's Color3DLUT:
against the NumPy model tests/lut3d_reference.py (itself pinned to Pillow by test_lut3d_host.py) for the shared catalogue
and for image sizes taken from the kernel's own geometry, and against live Pillow for its own filter objects.  Exactness is the
criterion; every test is one or a few batched calls."""
import ctypes

import numpy as np
import pytest

import filter_reference as B
import lut3d_reference as M
import window_filter_reference as WM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def geometry(A):
    return A.filters.lut3d_geometry()


def _entries(f):
    return f.size[0] * f.size[1] * f.size[2]


def _objects(A, cases, pil=False):
    """one filter object per Lut of the cases (a Lut shared by several cases is one object, so one table of the call)"""
    made = {}
    return [made.setdefault(id(f), f.pil() if pil else f.ours(A)) for _, f in cases]


def _check(A, cases, want=None, filters=None, **kw):
    """cases [(image, Lut)] through filter_many in one call, each against the model"""
    want = want or [M.model(a, f) for a, f in cases]
    got = [g.cpu().numpy() for g in A.filter_many([a for a, _ in cases], filters or _objects(A, cases), **kw)]
    bad = [(k, a.shape, f) for k, ((a, f), g, w) in enumerate(zip(cases, got, want)) if g.dtype != np.uint8 or g.shape != w.shape or not np.array_equal(g, w)]
    assert bad == [], (kw, len(bad), bad[:8])


@pytest.fixture(scope="module")
def catalogue():
    cases = M.catalogue()
    M.check_catalogue(cases)
    return cases, [M.model(a, f) for a, f in cases]


def test_catalogue(A, catalogue):
    cases, want = catalogue
    _check(A, cases, want)


def test_catalogue_with_pillows_objects(A, catalogue):
    cases, want = catalogue
    _check(A, cases, want, filters=_objects(A, cases, pil=True))


def test_sizes_at_every_kernel_constant(A, geometry):
    """images of one pixel fewer than a tile, a tile, two more, two tiles and a lane's run, and the same around 16 tiles (many
    workgroups an image); 3 and 4 channels, every combination"""
    run, tile = geometry["run"], geometry["tile"]
    assert (run, tile) == (4, 4096)

    def shapes(t):
        return [(1, t - 1), (2, t // 2), (2, t // 2 + 1), (3, (2 * t + run) // 3 + 1)]      # (t - 1, t, t + 2 and 2 t + run + 3 pixels or so)
    for shp, size in ((shapes(tile), 33), (shapes(tile), 17), (shapes(16 * tile), 17), (shapes(tile), 20)):
        cases = []
        for k, shape in enumerate(shp):
            for j, combo in enumerate(M.COMBOS):
                if (k + j) % 2 == 0 or shape[1] < 10000:
                    cases.append((M.image(shape, combo[0], seed=k), M.lut(size, M.KINDS[1 + (k + j) % 2], combo[1], M.MODES[combo])))
        assert {(a.shape[2], f.channels, f.bands(a.shape[2])) for a, f in cases} == set(M.COMBOS)
        _check(A, cases)


def _mixed(n=15):
    """tables, blurs and window filters alternating; every third table changes the channel count"""
    b = WM.builtins()
    luts = [(3, M.lut(17, "mild", 3, None)), (4, M.lut(5, "wild", 3, "RGB")), (3, M.lut((2, 3, 65), "mild", 4, "RGBA")), (4, M.lut(33, "wild", 4, None)),
            (4, M.lut(21, "ties", 3, None))]
    cases = []
    for k in range(n):
        shape = (9 + 11 * (k % 7), 150 - 13 * (k % 9))
        if k % 5 in (0, 4):
            c, f = luts[(k // 5 * 2 + (k % 5 == 4)) % len(luts)]
            cases.append((M.image(shape, c, seed=k), f))
        else:
            cases.append((WM.image(shape, 1 + k % 4, seed=k), [B.Spec("GaussianBlur", 2), b[0], WM.Rank(3, 4)][k % 5 - 1]))
    return cases


def _mixed_model(a, f):
    return M.model(a, f) if isinstance(f, M.Lut) else B.model(a, f) if getattr(f, "name", None) in B.PASSES else WM.model(a, f)


def _mixed_filters(A, cases):
    made = {}
    return [made.setdefault(id(f), f.ours(A)) if isinstance(f, M.Lut) else f for _, f in cases]


def test_mixed_list_in_input_order_in_one_allocation(A):
    import torch
    cases = _mixed()
    assert all(sum(pick(f) for _, f in cases) >= 3 for pick in (lambda f: isinstance(f, M.Lut), lambda f: getattr(f, "name", None) == "GaussianBlur",
                                                              lambda f: hasattr(f, "filterargs"), lambda f: hasattr(f, "rank")))
    assert any(isinstance(f, M.Lut) and f.bands(a.shape[2]) != a.shape[2] for a, f in cases)      # a table that changes the channel count
    sources = [torch.from_numpy(a).cuda() if k % 3 == 0 else a for k, (a, _) in enumerate(cases)]
    sources[0].jpeg_comment = b"kept"
    before = [s.clone() if isinstance(s, torch.Tensor) else s.copy() for s in sources]
    together = A.filter_many(sources, _mixed_filters(A, cases))
    assert together[0].jpeg_comment == b"kept" and not hasattr(together[1], "jpeg_comment")
    for k, ((a, f), t) in enumerate(zip(cases, together)):
        want = _mixed_model(a, f)
        assert tuple(t.shape) == want.shape and np.array_equal(t.cpu().numpy(), want), (k, a.shape, f)
    st = together[0].untyped_storage()
    assert all(t.untyped_storage().data_ptr() == st.data_ptr() and t.is_contiguous() and t.is_cuda for t in together)
    spans = [(t.data_ptr(), t.data_ptr() + t.numel()) for t in together]
    assert spans == sorted(spans) and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))      # in input order, back to back
    assert st.nbytes() >= spans[-1][1] - spans[0][0] == sum(int(np.prod(_mixed_model(a, f).shape)) for a, f in cases)
    for s, b in zip(sources, before):
        if isinstance(s, torch.Tensor):
            xs = s.untyped_storage()
            assert st.data_ptr() + st.nbytes() <= xs.data_ptr() or xs.data_ptr() + xs.nbytes() <= st.data_ptr()      # no output lies in an input
            assert torch.equal(s, b)
        else:
            assert np.array_equal(s, b)


def test_one_table_for_twelve_images_and_twelve_tables(A, monkeypatch):
    """a table object given for many images -- as the one filter of the call, or twelve times in its list -- is prepared once and is
    one table of the C call; twelve objects are twelve"""
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    lib = get_context(0).lib
    seen = {"prepared": 0, "tables": []}
    real_prepare, real_batch = lib.aej_lut3d_prepare_host, lib.aej_lut3d_batch

    def prepare(*a):
        seen["prepared"] += 1
        return real_prepare(*a)

    def batch(*a):
        seen["tables"].append(int(a[5]))
        return real_batch(*a)
    monkeypatch.setattr(lib, "aej_lut3d_prepare_host", prepare, raising=False)
    monkeypatch.setattr(lib, "aej_lut3d_batch", batch, raising=False)
    spec = M.lut(17, "mild", 3, None)
    images = [M.image((5 + 3 * k, 40 - 2 * k), 3 + k % 2, seed=k) for k in range(12)]
    images[5] = torch.from_numpy(images[5]).cuda()
    plain = [np.asarray(x.cpu()) if isinstance(x, torch.Tensor) else x for x in images]
    one = spec.ours(A)
    for filters in (one, [one] * 12):
        got = A.filter_many(images, filters)
        assert all(np.array_equal(g.cpu().numpy(), M.model(a, spec)) for g, a in zip(got, plain))
    assert seen == {"prepared": 2, "tables": [1, 1]}
    specs = [M.lut(s, M.KINDS[k % len(M.KINDS)], 3 + (k % 4 == 3), None) for k, s in enumerate((2, 3, (2, 3, 65), 5, 16, 17, 20, 21, (65, 2, 3), 9, 33, (3, 65, 2)))]
    images4 = [M.image((5 + 3 * k, 40 - 2 * k), 4, seed=k) for k in range(12)]
    got = A.filter_many(images4, [s.ours(A) for s in specs])
    assert all(np.array_equal(g.cpu().numpy(), M.model(a, s)) for g, a, s in zip(got, images4, specs))
    assert seen == {"prepared": 14, "tables": [1, 1, 12]}


def test_pillows_own_objects_and_sources_of_every_kind(A):
    import torch
    from PIL import Image, ImageFilter
    rng = np.random.default_rng(4)
    arrays = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((40, 50, 3), (33, 20, 4), (21, 64, 4), (50, 37, 3))]
    wide = torch.from_numpy(rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)).cuda()
    view = wide[3:60:2, 5:90, :]                              # a non-contiguous device view
    images = [arrays[0], torch.from_numpy(arrays[1].copy()), torch.from_numpy(arrays[2]).cuda(), arrays[3], view]
    plain = [arrays[0], arrays[1], arrays[2], arrays[3], view.cpu().numpy()]
    sepia = ImageFilter.Color3DLUT.generate(9, lambda r, g, b: (0.393 * r + 0.769 * g + 0.189 * b, 0.349 * r + 0.686 * g + 0.168 * b, 0.272 * r + 0.534 * g + 0.131 * b))
    for f in (sepia, sepia.transform(lambda r, g, b: (1 - r, g * g, b + 0.1, r), channels=4, target_mode="RGBA"),
              ImageFilter.Color3DLUT.generate((3, 4, 65), lambda r, g, b: (b, r, g), target_mode="HSV")):
        got = A.filter_many(images, f)
        for k, g in enumerate(got):
            want = np.asarray(Image.fromarray(plain[k]).filter(f))
            assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == want.shape and np.array_equal(g.cpu().numpy(), want), (k, f)


def test_c_entry_refusals_and_untouched_bytes(A, geometry):
    """aej_lut3d_batch itself: refusals named by image, exactly the image's bytes written, a workspace that is too small"""
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import Lut3dDesc, get_context
    ctx = get_context(0)
    lib = ctx.lib
    d = (Lut3dDesc * 1)()

    def call(a, spec, co, sb=None, db=None, table=0, offsets=None, ws_bytes=None, dst=None, **fields):
        src = torch.from_numpy(a).cuda().reshape(-1)
        d[0].src_offset, d[0].dst_offset, d[0].height, d[0].width, d[0].channels_in = 0, 32, a.shape[0], a.shape[1], a.shape[2]
        d[0].channels_out, d[0].table_channels, d[0].table = co, spec.channels, table
        d[0].size[:] = spec.size
        for k, v in fields.items():
            if k == "size":
                d[0].size[:] = v
            else:
                setattr(d[0], k, v)
        offs = np.asarray(offsets if offsets is not None else [0, spec.prepared.size], np.int64)
        n_out = a.shape[0] * a.shape[1] * co
        dst = torch.full((n_out + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        nws = int(lib.aej_lut3d_workspace_bytes(ctx.handle, ctypes.addressof(d), 1))
        ws = ctx.workspace(max(nws, 256))
        rc = lib.aej_lut3d_batch(ctx.handle, ctypes.addressof(d), 1, spec.prepared.ctypes.data, offs.ctypes.data, len(offs) - 1, src.data_ptr(),
                                 ctypes.c_uint64(src.numel() if sb is None else sb), dst.data_ptr(), ctypes.c_uint64(n_out + 64 if db is None else db),
                                 ws.data_ptr(), ctypes.c_uint64(ws.numel() if ws_bytes is None else ws_bytes))
        torch.cuda.synchronize()
        return rc, nws, lib.aej_last_error(ctx.handle), dst.cpu().numpy(), n_out

    for combo in M.COMBOS:
        for size in ((3, 4, 5), 33):
            a, spec = M.image((20, 31), combo[0], seed=1), M.lut(size, "wild", combo[1], M.MODES[combo])
            rc, nws, _, out, n = call(a, spec, combo[2])
            assert rc == 0 and nws >= 256 + 8 * _entries(spec)
            assert np.array_equal(out[32:32 + n].reshape(20, 31, combo[2]), M.model(a, spec)), (combo, size)
            assert (out[:32] == 0xA5).all() and (out[32 + n:] == 0xA5).all(), (combo, size)
    a, spec = M.image((20, 31), 4, seed=1), M.lut((3, 4, 5), "wild", 3, "RGB")
    n_in, n_out = a.size, 20 * 31 * 3
    rc, _, msg, out, _ = call(a, spec, 3, sb=n_in - 1)
    assert rc == -1 and b"image 0: source outside" in msg and (out == 0xA5).all()
    rc, _, msg, out, _ = call(a, spec, 3, db=n_out + 31)
    assert rc == -1 and b"image 0: image outside" in msg and (out == 0xA5).all()
    rc, nws, msg, out, _ = call(a, spec, 3, ws_bytes=255)
    assert rc == -4 and nws > 255 and b"workspace too small" in msg and (out == 0xA5).all()
    for co, fields in ((3, {"table_channels": 4}), (4, {"channels_in": 3}), (3, {"channels_in": 2}), (2, {}), (5, {}), (3, {"table_channels": 2}),
                       (3, {"size": (1, 4, 5)}), (3, {"size": (3, 66, 5)}), (3, {"size": (3, 4, 0)}), (3, {"width": 65536}), (3, {"height": 0}),
                       (3, {"src_offset": -1}), (3, {"dst_offset": -4})):
        rc, nws, msg, out, _ = call(a, spec, co, **fields)
        assert rc == -1 and nws == 0 and b"image 0:" in msg and (out == 0xA5).all(), (co, fields)
    for kw in ({"table": 1}, {"table": -1}, {"offsets": [0, spec.prepared.size - 3]}, {"offsets": [0, spec.prepared.size + 3]}):
        rc, _, msg, out, _ = call(a, spec, 3, **kw)
        assert rc == -1 and b"image 0:" in msg and (out == 0xA5).all(), kw
