"""GPU: paste_many, alpha_composite_many, blend_many, composite_many, chop_many and aej_compose_batch (csrc/compose.hip: k_compose)
bit-identical to Pillow's Image.paste, alpha_composite, blend, composite and ImageChops: against the NumPy model
tests/compose_reference.py (itself pinned to live Pillow by test_compose_host.py) for the shared catalogue, for the exhaustive inputs
and for sizes taken from the kernel's own geometry, and against Pillow's files for the chains paste -> JPEG and PNG -> alpha composite
-> PNG.  Exactness is the criterion; every test is one or a few batched calls."""
import ctypes
import io

import numpy as np
import pytest

import compose_reference as M

pytestmark = pytest.mark.gpu
KINDS = ("paste", "alpha_composite", "blend", "composite", "chop")


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def geometry(A):
    return A.compose.compose_geometry()


@pytest.fixture(scope="module")
def catalogue():
    """the shared cases with the model's answer, computed once"""
    cases = M.catalogue()
    return cases, [M.model(c) for c in cases]


def bad_ones(cases, got, want):
    got = [g.cpu().numpy() for g in got]
    return [(k, M.signature(c), c.get("geometry")) for k, (c, g, w) in enumerate(zip(cases, got, want))
            if g.dtype != np.uint8 or g.shape != w.shape or not np.array_equal(g, w)]


def _one_for_all(A, c):
    """the case's call with its second image, place and mask as ONE value for two copies of its first image"""
    k = c["kind"]
    if k == "paste":
        return A.paste_many([c["base"], c["base"]], c["overlay"], c["at"], c["mask"])
    if k == "alpha_composite":
        return A.alpha_composite_many([c["base"], c["base"]], c["overlay"], c["dest"], c["source"])
    if k == "blend":
        return A.blend_many([c["im1"], c["im1"]], c["im2"], c["alpha"])
    if k == "composite":
        return A.composite_many([c["im1"], c["im1"]], c["im2"], c["mask"])
    return A.chop_many([c["im1"], c["im1"]], c["im2"], M.library_op(A, c["op"]))


def test_catalogue_one_value_for_all_images(A, catalogue):
    cases, want = catalogue
    bad = []
    for c, w in zip(cases, want):
        bad += bad_ones([c, c], _one_for_all(A, c), [w, w])
    assert bad == [], (len(bad), bad[:6])


def test_catalogue_mixed_in_one_call(A, catalogue):
    """all cases of a kind in one call, one entry per image; the outputs are views of one packed allocation in input order"""
    cases, want = catalogue
    for kind in KINDS:
        idx = [k for k, c in enumerate(cases) if c["kind"] == kind]
        assert idx
        got = M.call(A, [cases[k] for k in idx])
        bad = bad_ones([cases[k] for k in idx], got, [want[k] for k in idx])
        assert bad == [], (kind, len(bad), bad[:6])
        st, pos = got[0].untyped_storage().data_ptr(), got[0].data_ptr()
        for g in got:
            assert g.is_contiguous() and g.untyped_storage().data_ptr() == st and g.data_ptr() == pos
            pos += g.numel()


def test_sources_on_host_and_device(A, catalogue):
    import torch
    cases, want = catalogue
    made = []

    def wrap_with(j):
        def wrap(a):
            s = [a, torch.from_numpy(a), torch.from_numpy(a).cuda(), torch.from_numpy(a).cuda()][j % 4]
            made.append((s, a))
            return s
        return wrap
    for kind in KINDS:
        idx = [k for k, c in enumerate(cases) if c["kind"] == kind][::3]
        got = []
        for j, k in enumerate(idx):
            got += M.call(A, [cases[k]], wrap_with(j))
        assert bad_ones([cases[k] for k in idx], got, [want[k] for k in idx]) == [], kind
        outs = {g.untyped_storage().data_ptr() for g in got}
        for s, a in made:
            if torch.is_tensor(s) and s.is_cuda:
                assert s.untyped_storage().data_ptr() not in outs
                assert np.array_equal(s.cpu().numpy(), a)     # the input is not written
    base = torch.from_numpy(M.image(9, 11, 3, 1)).cuda()
    base.jpeg_comment = b"kept"
    (out,) = A.paste_many([base], (1, 2, 3), (2, 2, 5, 5))
    assert out.jpeg_comment == b"kept"


def test_one_overlay_shared_by_16_bases(A, monkeypatch):
    """one logo object, pasted by its own alpha at 16 places, is staged once"""
    from adaptive_edge_aware_jpeg_amd import compose
    logo = M.image(9, 13, 4, 3)
    bases = [M.image(20 + i, 31 - i, 3, i) for i in range(16)]
    ats = [(3 * i - 8, 2 * i - 5) for i in range(16)]
    staged = []
    real = compose.gather_u8

    def counting(ctx, arrays, *a, **k):
        staged.append(len(arrays))
        return real(ctx, arrays, *a, **k)
    monkeypatch.setattr(compose, "gather_u8", counting)
    got = A.paste_many(bases, logo, ats, "alpha")
    assert staged == [17]
    cases = [dict(kind="paste", base=b, overlay=logo, at=at, mask="alpha") for b, at in zip(bases, ats)]
    assert bad_ones(cases, got, [M.model(c) for c in cases]) == []
    staged.clear()
    got = A.paste_many(bases, logo, ats, logo)                 # the overlay passed again as its own mask
    assert staged == [17]
    assert bad_ones(cases, got, [M.model(c) for c in cases]) == []


def test_masked_paste_on_all_2_24_triples(A):
    case = M.exhaustive_paste()
    assert bad_ones([case], M.call(A, [case]), [M.model(case)]) == []


def test_every_chop_on_all_byte_pairs(A):
    cases = M.exhaustive_chops()
    assert bad_ones(cases, M.call(A, cases), [M.model(c) for c in cases]) == []


def test_blend_on_all_byte_pairs(A):
    cases = M.exhaustive_blends()
    assert bad_ones(cases, M.call(A, cases), [M.model(c) for c in cases]) == []


def test_alpha_composite_on_all_alpha_pairs(A):
    cases = [M.exhaustive_alpha(4), M.exhaustive_alpha(2)]
    assert bad_ones(cases, M.call(A, cases), [M.model(c) for c in cases]) == []


def test_chunks_and_region_edges(A, geometry):
    """sizes from the kernel's geometry, for every channel count: an image of two chunks plus 5 pixels, a region whose rows straddle the
    chunk boundary, and one that begins on a chunk's last pixel"""
    chunk = geometry["chunk"]
    n = 2 * chunk + 5
    w = next(w for w in range(300, 1, -1) if n % w == 0)
    h = n // w
    assert h * w == n
    W, H = 100, (2 * chunk) // 100 + 2                         # the chunk boundary falls inside a row
    by, bx = divmod(chunk, W)
    assert 10 < bx < W - 2
    ly, lx = divmod(chunk - 1, w)
    groups = {"paste": [], "alpha_composite": [], "blend": [], "chop": []}
    for c in (1, 2, 3, 4):
        oc = {1: 2, 3: 4}.get(c, c)
        two, wide = M.image(h, w, c, c), M.image(H, W, c, 10 + c)
        groups["paste"] += [
            dict(kind="paste", base=two, overlay=M.image(h, w, oc, 20 + c), at=(0, 0), mask="alpha"),
            dict(kind="paste", base=two, overlay=M.image(5, 3, c, 30 + c), at=(lx, ly), mask=M.image(5, 3, 1, 40 + c)),      # begins on a chunk's last pixel
            dict(kind="paste", base=wide, overlay=M.image(6, 12, oc, 50 + c), at=(bx - 6, by - 2), mask="alpha"),             # rows straddle the boundary
            dict(kind="paste", base=wide, overlay=M.image(4, 30, c, 60 + c), at=((chunk - 1) % W, (chunk - 1) // W), mask=None),
            dict(kind="paste", base=wide, overlay=M._colour(c, c), at=(bx - 20, by - 1), mask=M.make_mask("bit", 3, 40, c))]
        groups["blend"].append(dict(kind="blend", im1=two, im2=M.image(h, w, c, 70 + c), alpha=0.4))
        groups["chop"].append(dict(kind="chop", im1=wide, im2=M.image(H + 3, W - 1, c, 80 + c), op="screen"))                  # the base's rows are longer than the output's
        if c in (2, 4):
            groups["alpha_composite"].append(dict(kind="alpha_composite", base=wide, overlay=M.image(6, 12, c, 90 + c), dest=(bx - 6, by - 2), source=(1, 1)))
            groups["alpha_composite"].append(dict(kind="alpha_composite", base=two, overlay=M.image(h, w, c, 95 + c), dest=(0, 0), source=(0, 0)))
    for kind, cases in groups.items():
        assert bad_ones(cases, M.call(A, cases), [M.model(c) for c in cases]) == [], kind


def test_outputs_feed_the_encoders_in_place(A):
    """paste -> standard_jpeg_encode_many, and png_decode_many(mode="auto") -> alpha_composite_many over white -> png_encode_many:
    Pillow's files"""
    from PIL import Image
    rng = np.random.default_rng(4)
    y, x = np.mgrid[0:47, 0:61]
    photo = np.stack([np.clip(60 + 2 * x + k * y + rng.normal(0, 6, x.shape), 0, 255) for k in range(3)], axis=2).astype(np.uint8)
    logo = M.image(12, 17, 4, 2)
    (out,) = A.paste_many([photo], logo, (40, 30), "alpha")
    want = Image.fromarray(photo)
    want.paste(Image.fromarray(logo), (40, 30), Image.fromarray(logo))
    assert np.array_equal(out.cpu().numpy(), np.asarray(want))
    (jpg,) = A.standard_jpeg_encode_many([out], 85)
    buf = io.BytesIO()
    want.save(buf, "JPEG", quality=85)
    assert jpg == buf.getvalue()
    rgba = M.image(33, 29, 4, 5)
    buf = io.BytesIO()
    Image.fromarray(rgba).save(buf, "PNG")
    (decoded,) = A.png_decode_many([buf.getvalue()], mode="auto")
    assert tuple(decoded.shape) == (33, 29, 4)
    white = np.full((33, 29, 4), 255, np.uint8)
    (flat,) = A.alpha_composite_many([white], [decoded])
    want = Image.alpha_composite(Image.fromarray(white), Image.fromarray(rgba))
    assert np.array_equal(flat.cpu().numpy(), np.asarray(want))
    (png,) = A.png_encode_many([flat], entropy="host")
    buf = io.BytesIO()
    want.save(buf, "PNG")
    assert png == buf.getvalue()


def test_c_entry_refusals_and_untouched_bytes(A):
    """aej_compose_batch itself: exactly the image's bytes written; workspace too small, source outside the input, source inside the
    output, image outside the output and n < 1, each with its code and text"""
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import ComposeDesc, get_context
    ctx = get_context(0)
    lib = ctx.lib
    base, logo = M.image(20, 30, 3, 1), M.image(6, 7, 4, 2)
    nb, nl = base.size, logo.size
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:nb] = torch.from_numpy(base).cuda().reshape(-1)
    buf[nb:nb + nl] = torch.from_numpy(logo).cuda().reshape(-1)
    d = (ComposeDesc * 1)()
    d[0].base_offset, d[0].over_offset, d[0].dst_offset = 0, nb, 32
    d[0].width, d[0].height, d[0].channels, d[0].over_width, d[0].over_height, d[0].over_channels = 30, 20, 3, 7, 6, 4
    d[0].mask_kind, d[0].x, d[0].y = 3, 26, -2
    d[0].box[:] = (0, 0, 7, 6)
    dst = torch.full((nb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    nws = int(lib.aej_compose_workspace_bytes(ctx.handle, ctypes.addressof(d), 1))
    assert nws > 0
    ws = ctx.workspace(max(nws, 256))

    def call(count, src_ptr, sb, dst_ptr, db, wsb):
        rc = lib.aej_compose_batch(ctx.handle, ctypes.addressof(d), count, src_ptr, ctypes.c_uint64(sb), dst_ptr, ctypes.c_uint64(db), ws.data_ptr(),
                                   ctypes.c_uint64(wsb))
        return rc, lib.aej_last_error(ctx.handle)

    rc, msg = call(1, buf.data_ptr(), nb + nl, dst.data_ptr(), nb + 64, ws.numel())
    assert rc == 0, msg
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.array_equal(out[32:32 + nb].reshape(20, 30, 3), M.paste(base, logo, (26, -2), "alpha"))
    assert (out[:32] == 0xA5).all() and (out[32 + nb:] == 0xA5).all()
    rc, msg = call(1, buf.data_ptr(), nb + nl, dst.data_ptr(), nb + 64, nws - 1)
    assert rc == -4 and b"workspace too small" in msg
    rc, msg = call(1, buf.data_ptr(), nb + nl - 1, dst.data_ptr(), nb + 64, ws.numel())
    assert rc == -1 and b"image 0: source outside the input" in msg
    rc, msg = call(1, buf.data_ptr(), nb + nl, dst.data_ptr(), nb + 31, ws.numel())
    assert rc == -1 and b"image 0: image outside the output" in msg
    rc, msg = call(1, buf.data_ptr(), nb + nl, buf.data_ptr() + nb + nl - 1, nb + 64, ws.numel())
    assert rc == -1 and b"image 0: source inside the output" in msg
    for count in (0, -1):
        rc, msg = call(count, buf.data_ptr(), nb + nl, dst.data_ptr(), nb + 64, ws.numel())
        assert rc == -1 and b"no images" in msg
    rc, msg = call(1, None, nb + nl, dst.data_ptr(), nb + 64, ws.numel())
    assert rc == -1 and b"NULL buffer" in msg
    d[0].over_channels = 3                                     # the overlay as its own mask, without alpha
    rc, msg = call(1, buf.data_ptr(), nb + nl, dst.data_ptr(), nb + 64, ws.numel())
    assert rc == -1 and b"image 0: the overlay as its own mask needs 2 or 4 channels" in msg
    assert lib.aej_compose_workspace_bytes(ctx.handle, ctypes.addressof(d), 1) == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy()[32 + nb:] == 0xA5).all()


def test_more_chunks_than_the_grid(A, geometry):
    """more chunks in one launch than the largest grid, so that workgroups stride to a second chunk: max_grid + 37 bases of one to three
    pixels, all blended with one shared second image per width"""
    import torch
    n = geometry["max_grid"] + 37
    rng = np.random.default_rng(5)
    widths = 1 + np.arange(n) % 3
    pixels = rng.integers(0, 256, (int(widths.sum()), 3), dtype=np.uint8)
    ends = np.cumsum(widths)
    bases = [pixels[e - w:e].reshape(1, w, 3) for w, e in zip(widths, ends)]
    seconds = {w: rng.integers(0, 256, (1, w, 3), dtype=np.uint8) for w in (1, 2, 3)}
    got = A.chop_many(bases, [seconds[int(w)] for w in widths], "difference")
    assert len(got) == n and got[0].untyped_storage().nbytes() == pixels.size
    flat = torch.cat([g.reshape(-1) for g in got]).cpu().numpy()
    want = np.concatenate([M.chop(b, seconds[int(w)], "difference").reshape(-1) for b, w in zip(bases, widths)])
    assert np.array_equal(flat, want)
