"""GPU: adjust_many, histogram_many and aej_adjust_batch (csrc/adjust.hip: k_adjust_hist, k_adjust_luts, k_adjust_apply) bit-identical
to Pillow's ImageEnhance, ImageOps point operations, Image.point and Image.histogram: against the NumPy model tests/adjust_reference.py
(itself pinned to live Pillow by test_adjust_host.py) for the shared catalogue and for sizes taken from the kernels' own geometry, and
against Pillow's files for the chains adjust -> JPEG and adjust -> PNG.  Exactness is the criterion; every test is one or a few batched
calls."""
import ctypes
import io

import numpy as np
import pytest

import adjust_reference as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def geometry(A):
    return A.adjust.adjust_geometry()


@pytest.fixture(scope="module")
def catalogue():
    """the shared cases with the model's answer, computed once"""
    cases = M.catalogue()
    return cases, [M.model(c) for c in cases]


def bad_ones(cases, got, want):
    got = [g.cpu().numpy() for g in got]
    return [(k, c[0].shape, str(c[1])[:120]) for k, (c, g, w) in enumerate(zip(cases, got, want)) if g.dtype != np.uint8 or g.shape != w.shape or not np.array_equal(g, w)]


def test_catalogue_one_op_per_call(A, catalogue):
    """every distinct op or chain of the catalogue in a call of its own, as ONE value for all its images"""
    cases, want = catalogue
    groups = {}
    for k, c in enumerate(cases):
        groups.setdefault(repr(c[1]), []).append(k)
    assert len(groups) >= 80
    bad = []
    for idx in groups.values():
        got = A.adjust_many([cases[k][0] for k in idx], M.library_ops(A, cases[idx[0]][1]))
        bad += bad_ones([cases[k] for k in idx], got, [want[k] for k in idx])
    assert bad == [], (len(bad), bad[:6])


def test_catalogue_mixed_in_one_call(A, catalogue):
    """all cases in one call, one entry per image; the outputs are views of one packed allocation in input order"""
    cases, want = catalogue
    got = A.adjust_many([c[0] for c in cases], [M.library_ops(A, c[1]) for c in cases])
    bad = bad_ones(cases, got, want)
    assert bad == [], (len(bad), bad[:6])
    st, pos = got[0].untyped_storage().data_ptr(), got[0].data_ptr()
    for g in got:
        assert g.is_contiguous() and g.untyped_storage().data_ptr() == st and g.data_ptr() == pos
        pos += g.numel()


def test_sources_on_host_and_device(A, catalogue):
    import torch
    cases, want = catalogue
    idx = list(range(0, len(cases), 9))
    sources = []
    for j, k in enumerate(idx):
        a = cases[k][0]
        sources.append([a, torch.from_numpy(a), torch.from_numpy(a).cuda(), torch.from_numpy(a).cuda()][j % 4])
    got = A.adjust_many(sources, [M.library_ops(A, cases[k][1]) for k in idx])
    assert bad_ones([cases[k] for k in idx], got, [want[k] for k in idx]) == []
    for k, s, g in zip(idx, sources, got):
        if torch.is_tensor(s) and s.is_cuda:
            assert g.untyped_storage().data_ptr() != s.untyped_storage().data_ptr()
            assert np.array_equal(s.cpu().numpy(), cases[k][0])      # the input is not written


def _two_chunks(geometry, c, seed, flat=None):
    """an image of two chunks plus 5 pixels: the smallest with a merge of workgroups' histograms"""
    n = 2 * geometry["chunk"] + 5
    w = next(w for w in range(300, 1, -1) if n % w == 0)
    h = n // w
    assert h * w == n and n <= 300 * 200
    a = M.image(h, w, c, seed)
    if flat is not None:
        a[...] = flat
    return a


def test_histogram_many(A, geometry):
    images = [_two_chunks(geometry, 1, 1), _two_chunks(geometry, 3, 2), _two_chunks(geometry, 1, 3, flat=200), _two_chunks(geometry, 4, 4, flat=7),
              M.image(1, 1, 1), M.image(5, 4, 2), M.image(67, 35, 3), M.image(16, 17, 4)]
    got = A.histogram_many(images)
    import torch
    for a, g in zip(images, got):
        b = a.reshape(a.shape[0] * a.shape[1], -1)
        want = np.concatenate([np.bincount(b[:, c], minlength=256) for c in range(b.shape[1])])
        assert g.dtype == torch.int64 and g.shape == (256 * b.shape[1],) and np.array_equal(g.cpu().numpy(), want)
        assert np.array_equal(want, M.histogram(a))
    assert int(got[2].cpu().numpy()[200]) == 2 * geometry["chunk"] + 5
    again = A.histogram_many(images)                       # integer adds: the same counts every time
    assert all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(got, again))


def test_statistics_across_chunks(A, geometry):
    """an Equalize and a Contrast (and the other statistics ops) of images whose histogram is merged from three workgroups"""
    cases = []
    for c in (1, 3):
        a = _two_chunks(geometry, c, 5 + c)
        cases += [(a, ("equalize",)), (a, ("contrast", 1.3)), (a, ("autocontrast", (2, 10), None, False)), (a, ("autocontrast", 5, 0, True)),
                  (a, (("brightness", 1.1), ("contrast", 0.5), ("equalize",), ("sharpness", 2.0), ("autocontrast", 1, None, False)))]
    cases += [(_two_chunks(geometry, 4, 9), ("contrast", 1.9)), (_two_chunks(geometry, 2, 10), (("contrast", -0.3), ("grayscale",), ("equalize",))),
              (_two_chunks(geometry, 3, 11, flat=90), ("equalize",)), (_two_chunks(geometry, 1, 12, flat=90), ("contrast", 3.0))]
    got = A.adjust_many([c[0] for c in cases], [M.library_ops(A, c[1]) for c in cases])
    assert bad_ones(cases, got, [M.model(c) for c in cases]) == []


def test_lane_groups_and_tails(A, geometry):
    """pixel counts around a lane's group (16, 8, 4 and 4 pixels for 1 to 4 channels) and around a workgroup's sweep: every vector
    access and every byte tail, with a source that starts at an odd address"""
    cases = []
    for c in (1, 2, 3, 4):
        for n in (1, 3, 4, 5, 15, 16, 17, 31, 33, geometry["threads"] * 4 - 1, geometry["threads"] * 16 + 1, geometry["chunk"] - 1, geometry["chunk"], geometry["chunk"] + 1):
            a = M.image(1, n, c, n)
            cases += [(a, ("brightness", 1.1)), (a, (("color", 1.9), ("grayscale",))), (a, ("sharpness", 0.5))]
            if c in (1, 3):
                cases.append((a, ("equalize",)))
    got = A.adjust_many([c[0] for c in cases], [M.library_ops(A, c[1]) for c in cases])
    assert bad_ones(cases, got, [M.model(c) for c in cases]) == []


def test_outputs_feed_the_encoders_in_place(A):
    """adjust_many -> standard_jpeg_encode_many and -> png_encode_many: Pillow's files from the model's pixels"""
    from PIL import Image
    rgb, grey = M._natural(61, 47, 3, 1), M._natural(40, 52, 1, 2)
    chain = (("brightness", 1.2), ("contrast", 0.8), ("color", 1.1), ("sharpness", 1.5))
    out = A.adjust_many([rgb, grey], [M.library_ops(A, chain), M.library_ops(A, ("equalize",))])
    want = [M.model((rgb, chain)), M.model((grey, ("equalize",)))]
    assert bad_ones([(rgb, chain), (grey, ("equalize",))], out, want) == []
    (jpg,) = A.standard_jpeg_encode_many(out[:1], 85)
    buf = io.BytesIO()
    Image.fromarray(want[0]).save(buf, "JPEG", quality=85)
    assert jpg == buf.getvalue()
    pngs = A.png_encode_many(out, entropy="host")
    for p, w in zip(pngs, want):
        buf = io.BytesIO()
        Image.fromarray(w).save(buf, "PNG")
        assert p == buf.getvalue()


def test_c_entry_refusals_and_untouched_bytes(A):
    """aej_adjust_batch itself: exactly the image's bytes written; workspace too small, source outside the input, source inside the
    output and n < 1, each with its code and text"""
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import AdjustDesc, get_context
    ctx = get_context(0)
    lib = ctx.lib
    a = M.image(20, 30, 3, 1)
    chain = (("contrast", 1.3), ("sharpness", 2.0), ("grayscale",))
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    n = a.size
    buf[:n] = torch.from_numpy(a).cuda().reshape(-1)
    d = (AdjustDesc * 1)()
    d[0].src_offset, d[0].dst_offset, d[0].width, d[0].height, d[0].channels, d[0].n_ops = 0, 32, 30, 20, 3, 3
    d[0].ops[0].kind, d[0].ops[0].factor = 1, 1.3
    d[0].ops[1].kind, d[0].ops[1].factor = 3, 2.0
    d[0].ops[2].kind = 7
    m = 30 * 20
    dst = torch.full((m + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    nws = int(lib.aej_adjust_workspace_bytes(ctx.handle, ctypes.addressof(d), 1))
    assert nws > 0
    ws = ctx.workspace(max(nws, 256))

    def call(count, src_ptr, sb, dst_ptr, db, wsb, n_tables=0):
        rc = lib.aej_adjust_batch(ctx.handle, ctypes.addressof(d), count, None, n_tables, src_ptr, ctypes.c_uint64(sb), dst_ptr, ctypes.c_uint64(db),
                                  ws.data_ptr(), ctypes.c_uint64(wsb))
        return rc, lib.aej_last_error(ctx.handle)

    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 64, ws.numel())
    assert rc == 0, msg
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.array_equal(out[32:32 + m].reshape(20, 30), M.model((a, chain)))
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
    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 64, ws.numel(), n_tables=1)
    assert rc == -1 and b"NULL buffer" in msg
    d[0].ops[2].kind = 6                                       # a table op whose table the call does not bring
    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 64, ws.numel())
    assert rc == -1 and b"image 0: a table number outside the tables" in msg
    d[0].ops[2].kind, d[0].channels = 5, 4                     # EQUALIZE of 4 channels
    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 64, ws.numel())
    assert rc == -1 and b"image 0: a histogram table op on an image of 2 or 4 channels" in msg
    assert lib.aej_adjust_workspace_bytes(ctx.handle, ctypes.addressof(d), 1) == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy()[32 + m:] == 0xA5).all()


def test_more_chunks_than_the_grid(A, geometry):
    """more chunks in one launch than the largest grid, so that workgroups stride to a second chunk: max_grid + 37 images of one to
    three pixels (every image is at least a chunk).  The chain is per-pixel, so the model runs once on all pixels together"""
    import torch
    n = geometry["max_grid"] + 37
    rng = np.random.default_rng(5)
    widths = 1 + np.arange(n) % 3
    pixels = rng.integers(0, 256, (int(widths.sum()), 1, 3), dtype=np.uint8)
    ends = np.cumsum(widths)
    images = [pixels[e - w:e].reshape(1, w, 3) for w, e in zip(widths, ends)]
    chain = (("brightness", 1.1), ("color", 1.9), ("invert",), ("grayscale",))
    want = M.model((pixels, chain))
    got = A.adjust_many(images, M.library_ops(A, chain))
    assert len(got) == n and got[0].untyped_storage().nbytes() == pixels.shape[0]
    flat = torch.cat([g.reshape(-1) for g in got]).cpu().numpy()
    assert np.array_equal(flat, want.reshape(-1))
    hists = A.histogram_many(images)
    assert len(hists) == n
    counts = torch.stack(hists).cpu().numpy().reshape(n, 3, 256)
    want_counts = np.zeros((n, 3, 256), np.int64)
    owner = np.repeat(np.arange(n), widths)
    for b in range(3):
        np.add.at(want_counts, (owner, b, pixels[:, 0, b]), 1)
    assert np.array_equal(counts, want_counts)
