"""CPU: the NumPy model tests/compose_reference.py against live Pillow, pixel for pixel, over the shared catalogue and over the
exhaustive inputs (all 2^24 masked-paste triples, every chop and blend on all byte pairs, every alpha pair over 64 colour pairs); the
catalogue's coverage of what is built; the refusals of compose.py by type and text, Pillow's own for dest= and source=; the exports,
the ABI and compose_plan's clipping.  No device anywhere."""
import ctypes
import os
import re

import numpy as np
import pytest

import compose_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module", autouse=True)
def library(A):
    """the model and the library are one feature: the chops the model knows are the ones the library builds"""
    from adaptive_edge_aware_jpeg_amd import compose
    assert compose.CHOPS == M.CHOPS


def pil(a):
    from PIL import Image
    return Image.fromarray(a)


def pillow(case):
    """Pillow's own answer for one case"""
    from PIL import Image, ImageChops
    k = case["kind"]
    if k == "paste":
        b = pil(case["base"]).copy()
        ov = pil(case["overlay"]) if isinstance(case["overlay"], np.ndarray) else case["overlay"]
        mask = case["mask"]
        b.paste(ov, case["at"], ov if isinstance(mask, str) else None if mask is None else pil(mask))
        return np.asarray(b)
    if k == "alpha_composite":
        b = pil(case["base"]).copy()
        b.alpha_composite(pil(case["overlay"]), case["dest"], case["source"])
        return np.asarray(b)
    if k == "blend":
        return np.asarray(Image.blend(pil(case["im1"]), pil(case["im2"]), case["alpha"]))
    if k == "composite":
        return np.asarray(Image.composite(pil(case["im1"]), pil(case["im2"]), pil(case["mask"])))
    op = case["op"] if isinstance(case["op"], tuple) else (case["op"],)
    return np.asarray(getattr(ImageChops, op[0])(pil(case["im1"]), pil(case["im2"]), *op[1:]))


@pytest.fixture(scope="module")
def catalogue():
    return M.catalogue()


def _differ(cases):
    bad = []
    for k, c in enumerate(cases):
        got, want = M.model(c), pillow(c)
        if got.dtype != np.uint8 or got.shape != want.shape or not np.array_equal(got, want):
            bad.append((k, M.signature(c), c.get("geometry")))
    return bad


# ---- (a) the model is Pillow ------------------------------------------------------------------------------------------------------
def test_model_equals_pillow(catalogue):
    bad = _differ(catalogue)
    assert bad == [], (len(bad), bad[:8])


def test_catalogue_covers_what_is_built(catalogue):
    """every built combination of kind, base channels, overlay channels and mask kind (or chop) has a case; the region cases are there"""
    have = {M.signature(c) for c in catalogue}
    missing = [row for row in M.built() if row not in have]
    assert missing == [] and len(M.built()) == len(set(M.built())) >= 100
    assert not [s for s in have if s not in set(M.built())]
    for row in M.EVERY_GEOMETRY:
        names = {c["geometry"] for c in catalogue if M.signature(c) == row}
        assert names >= {g[0] for g in M.GEOMETRIES}, row
    names = {g[0] for g in M.GEOMETRIES}
    assert names >= {"inside", "left", "top", "right", "bottom", "left and top", "right and bottom", "outside right", "outside left", "outside below",
                     "1 x 1 overlay", "larger than the base", "width 1", "width 3", "width 17", "width 61"}
    for c in catalogue:                                        # a region wholly outside leaves the base
        if c["kind"] == "paste" and str(c["geometry"]).startswith("outside"):
            assert np.array_equal(M.model(c), c["base"])
    assert max(max(v.shape[:2]) for c in catalogue for v in c.values() if isinstance(v, np.ndarray)) <= 64
    assert M.model(dict(kind="chop", im1=M.image(7, 5, 1), im2=M.image(3, 9, 1), op="add")).shape == (3, 5)      # 5 x 7 and 9 x 3 give 5 x 3


def test_masked_paste_on_all_2_24_triples():
    case = M.exhaustive_paste()
    want = pillow(case)
    assert np.array_equal(M.model(case), want)
    wrong = M.model(case, split_division=True)                  # one division per product is not Pillow's
    assert 3_000_000 < int((wrong != want).sum()) < 6_000_000


def test_every_chop_on_all_byte_pairs():
    cases = M.exhaustive_chops()
    assert {M.signature(c)[3] for c in cases} == set(M.CHOPS)
    assert any(s < 1 for s, _ in M.CHOP_PARAMETERS) and any(o < 0 for _, o in M.CHOP_PARAMETERS)
    assert _differ(cases) == []


def test_blend_on_all_byte_pairs():
    assert set(M.BLEND_ALPHAS) >= {0, 1, 0.3, -0.7, 1.7} and min(abs(a) for a in M.BLEND_ALPHAS if a) < 1e-20
    assert _differ(M.exhaustive_blends()) == []


@pytest.mark.parametrize("c", [4, 2])
def test_alpha_composite_on_all_alpha_pairs(c):
    pairs = M.colour_pairs()
    assert len(pairs) >= 64 and {v for p in pairs[:36] for v in p} == {0, 1, 127, 128, 254, 255}
    case = M.exhaustive_alpha(c)
    assert case["base"].shape == (256, 256 * 64, c)
    assert np.array_equal(M.model(case), pillow(case))


# ---- (b) the library's host side ----------------------------------------------------------------------------------------------------
def test_exports_and_abi(A):
    from adaptive_edge_aware_jpeg_amd import _lib, compose
    for name in ("paste_many", "alpha_composite_many", "blend_many", "composite_many", "chop_many", "compose_plan", "ChopAdd", "ChopSubtract"):
        assert name in A.__all__ and getattr(A, name) is getattr(compose, name), name
    header = open(os.path.join(ROOT, "include", "aej.h")).read()
    declared = set(re.findall(r"AEJ_API[^;(]*?\b(aej_compose_\w+)\s*\(", header))
    assert declared == {"aej_compose_geometry_host", "aej_compose_plan_host", "aej_compose_workspace_bytes", "aej_compose_batch"}
    assert declared == {k for k in _lib.SIGNATURES if k.startswith("aej_compose_")}
    lib = _lib.load_library()
    assert all(hasattr(lib, name) for name in declared)
    assert lib.aej_abi_version() == 3                     # entries were added: the version stays
    assert ctypes.sizeof(_lib.ComposeDesc) == 128 and ctypes.sizeof(_lib.ComposePlan) == 48
    assert (_lib.ComposeDesc.kind.offset, _lib.ComposeDesc.box.offset, _lib.ComposeDesc.colour.offset) == (32, 88, 116)
    assert compose.CHOPS == M.CHOPS
    g = compose.compose_geometry()
    assert g["chunk"] % g["threads"] == 0 and g["chunk"] >= 16 * g["threads"] // 16 and g["max_grid"] >= 1


def test_entries_without_a_context_or_buffers(A):
    from adaptive_edge_aware_jpeg_amd import _lib
    lib = _lib.load_library()
    d, p = (_lib.ComposeDesc * 1)(), _lib.ComposePlan()
    assert lib.aej_compose_geometry_host(None) == -1
    assert lib.aej_compose_plan_host(None, ctypes.addressof(p)) == -1 and lib.aej_compose_plan_host(ctypes.addressof(d), None) == -1
    assert lib.aej_compose_workspace_bytes(None, ctypes.addressof(d), 1) == 0
    assert lib.aej_compose_batch(None, ctypes.addressof(d), 1, None, 0, None, 0, None, 0) == -1
    d[0].width, d[0].height, d[0].channels, d[0].over_width, d[0].over_height, d[0].over_channels = 9, 8, 3, 4, 5, 4
    d[0].x, d[0].y, d[0].mask_kind = 7, -2, 3
    d[0].box[:] = (0, 0, 4, 5)
    assert lib.aej_compose_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == 0
    assert tuple(p.region) == (7, 0, 9, 3) and (p.out_width, p.out_height, p.out_channels, p.reads_overlay, p.reads_mask) == (9, 8, 3, 1, 0)
    for field, value in (("width", 0), ("height", 32768), ("channels", 5), ("over_width", 0), ("over_channels", 3), ("over_channels", 2), ("kind", 4),
                         ("kind", -1), ("mask_kind", 4), ("kind", 1), ("kind", 2), ("base_offset", -1)):
        e = (_lib.ComposeDesc * 1)()
        ctypes.memmove(e, d, ctypes.sizeof(d))
        setattr(e[0], field, value)
        assert lib.aej_compose_plan_host(ctypes.addressof(e), ctypes.addressof(p)) == -1, (field, value)
    d[0].mask_kind, d[0].mask_channels, d[0].mask_width, d[0].mask_height = 2, 3, 4, 5      # a 3-channel mask; then one of another size
    assert lib.aej_compose_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == -1
    d[0].mask_channels, d[0].mask_width = 1, 3
    assert lib.aej_compose_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == -1
    d[0].mask_width = 4
    assert lib.aej_compose_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == 0 and p.reads_mask == 1
    d[0].kind, d[0].mask_kind, d[0].over_channels, d[0].x, d[0].y, d[0].op, d[0].scale = 3, 0, 3, 0, 0, 0, 0.0      # ADD with scale 0
    assert lib.aej_compose_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == -1
    d[0].scale = 2.0
    assert lib.aej_compose_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == 0 and (p.out_width, p.out_height) == (4, 5)
    d[0].op = 12
    assert lib.aej_compose_plan_host(ctypes.addressof(d), ctypes.addressof(p)) == -1


def test_plan_clipping_equals_the_model(A, catalogue):
    for c in catalogue:
        k = c["kind"]
        if k == "paste":
            plan = A.compose_plan("paste", c["base"], c["overlay"], at=c["at"], mask=c["mask"])
            H, W = c["base"].shape[:2]
            if isinstance(c["overlay"], np.ndarray):
                oh, ow = c["overlay"].shape[:2]
            elif isinstance(c["mask"], np.ndarray):
                oh, ow = c["mask"].shape[:2]
            else:
                ow, oh = c["at"][2] - c["at"][0], c["at"][3] - c["at"][1]
            want = M.region(W, H, c["at"][0], c["at"][1], ow, oh)
            reads = ("base",) + (("overlay",) if want and isinstance(c["overlay"], np.ndarray) else ()) + (("mask",) if want and isinstance(c["mask"], np.ndarray) else ())
        elif k == "alpha_composite":
            plan = A.compose_plan(k, c["base"], c["overlay"], dest=c["dest"], source=c["source"])
            H, W = c["base"].shape[:2]
            oh, ow = c["overlay"].shape[:2]
            box = tuple(c["source"]) + ((ow, oh) if len(c["source"]) == 2 else ())
            want = M.region(W, H, c["dest"][0] - box[0], c["dest"][1] - box[1], ow, oh, box)
            reads = ("base",) + (("overlay",) if want else ())
        elif k == "composite":
            plan = A.compose_plan(k, c["im1"], c["im2"], c["mask"])
            H, W = c["im1"].shape[:2]
            want, reads = (0, 0, W, H), ("base", "overlay", "mask")
        else:
            plan = A.compose_plan(k, c["im1"], c["im2"], c["alpha"] if k == "blend" else M.library_op(A, c["op"]))
            H, W = M.model(c).shape[:2]
            want, reads = (0, 0, W, H), ("base", "overlay")
            assert plan["op"] == (M.signature(c)[3] if k == "chop" else None)
        assert (plan["kind"], plan["size"], plan["region"], plan["reads"]) == (k, (W, H), want, reads), (M.signature(c), c["geometry"], plan)
        assert plan["channels"] == M.signature(c)[1]
    rgb, logo = np.zeros((10, 12, 3), np.uint8), np.zeros((5, 4, 4), np.uint8)
    assert A.compose_plan("paste", rgb, logo, (-2, 7), "alpha") == dict(kind="paste", op=None, size=(12, 10), channels=3, region=(0, 7, 2, 10),
                                                                         reads=("base", "overlay"))
    with pytest.raises(ValueError, match="kind"):
        A.compose_plan("logical_and", rgb, rgb)
    with pytest.raises(TypeError, match="alpha is missing"):
        A.compose_plan("blend", rgb, rgb)


# ---- (c) refusals, all without a device -----------------------------------------------------------------------------------------
def test_refusals_need_no_device(A, monkeypatch):
    from PIL import Image, ImageChops

    from adaptive_edge_aware_jpeg_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("refused calls must not reach the device")
    monkeypatch.setattr(_lib, "get_context", no_device)
    rgb, rgba, la, grey = (np.zeros(s, np.uint8) for s in ((6, 7, 3), (6, 7, 4), (6, 7, 2), (6, 7)))
    small = np.zeros((2, 3, 3), np.uint8)

    def refused(exc, text, fn, *args, **kw):
        with pytest.raises(exc) as e:
            fn(*args, **kw)
        assert text in str(e.value), str(e.value)

    P = A.paste_many
    # ---- paste
    refused(ValueError, "image 1: mask: a 3-channel image is no mask", P, [rgb, rgb], small, (0, 0), [None, np.zeros((2, 3, 3), np.uint8)])
    refused(ValueError, "image 0: images do not match: a mask of 4 x 2", P, [rgb], small, (0, 0), np.zeros((2, 4), np.uint8))
    refused(ValueError, "image 0: images do not match: at (1, 1, 5, 5)", P, [rgb], small, (1, 1, 5, 5))
    with pytest.raises(ValueError, match="images do not match"):
        pil(rgb).paste(pil(small), (1, 1, 5, 5))
    with pytest.raises(ValueError, match="images do not match"):
        pil(rgb).paste(pil(small), (0, 0), pil(np.zeros((2, 4), np.uint8)))
    with pytest.raises(ValueError, match="bad transparency mask"):
        pil(rgb).paste(pil(small), (0, 0), pil(small))
    refused(ValueError, "image 0: mask 'alpha' needs an overlay with an alpha band, got mode RGB", P, [rgb], small, (0, 0), "alpha")
    refused(ValueError, "image 0: mask 'alpha' needs an overlay with an alpha band, got mode L", P, [grey], grey, (0, 0), "alpha")
    refused(ValueError, "image 0: mask 'alpha' needs an overlay image", P, [rgb], (1, 2, 3), (0, 0, 2, 2), "alpha")
    refused(ValueError, "image 0: bad transparency mask", P, [rgb], (1, 2, 3), (0, 0), np.zeros((2, 2, 2), np.uint8))
    with pytest.raises(ValueError, match="bad transparency mask"):
        pil(rgb).paste((1, 2, 3), (0, 0), pil(np.zeros((2, 2, 2), np.uint8)))
    refused(ValueError, "image 0: cannot determine region size", P, [rgb], (1, 2, 3))
    with pytest.raises(ValueError, match="cannot determine region size"):
        pil(rgb).paste((1, 2, 3), (0, 0))
    refused(ValueError, "image 0: overlay 5: an image, or a colour of mode RGB", P, [rgb], 5, (0, 0, 2, 2))
    refused(ValueError, "image 0: overlay (1, 2): an image, or a colour of mode L", P, [grey], (1, 2), (0, 0, 2, 2))
    refused(ValueError, "image 0: overlay (1, 2, 300)", P, [rgb], (1, 2, 300), (0, 0, 2, 2))
    refused(ValueError, "image 0: at (0, 0, 0, 2): a colour needs a box", P, [rgb], (1, 2, 3), (0, 0, 0, 2))
    refused(ValueError, "image 0: at (1, 2, 3)", P, [rgb], small, (1, 2, 3))
    refused(ValueError, "image 0: mask 'beta'", P, [rgb], small, (0, 0), "beta")
    refused(ValueError, "overlays: 1 entries for 2 images", P, [rgb, rgb], [small])
    refused(ValueError, "mask: 3 entries for 2 images", P, [rgb, rgb], small, (0, 0), [None, None, None])
    refused(ValueError, "paste_many needs at least one image", P, [], small)
    refused(ValueError, "image 1: image: uint8 [H, W]", P, [rgb, np.zeros((3, 3, 5), np.uint8)], small)
    refused(ValueError, "image 0: overlay: sizes up to 32767", P, [rgb], np.zeros((1, 32768), np.uint8))
    refused(TypeError, "image 0: overlay: uint8 required, got float32", P, [rgb], np.zeros((2, 2, 3), np.float32))
    refused(NotImplementedError, "image 0: images of mode '1' (bool) are not built", P, [np.zeros((3, 3), bool)], 1, (0, 0, 1, 1))
    refused(NotImplementedError, "image 0: images of mode 'P' are not built", P, [Image.new("P", (3, 3))], 1, (0, 0, 1, 1))
    for (b, o), text in (((rgb, grey), "mode L onto mode RGB"), ((rgb, la), "mode LA onto mode RGB"), ((grey, rgb), "mode RGB onto mode L"),
                         ((grey, rgba), "mode RGBA onto mode L"), ((rgba, rgb), "mode RGB onto mode RGBA"), ((la, rgba), "mode RGBA onto mode LA"),
                         ((la, grey), "mode L onto mode LA"), ((rgba, la), "mode LA onto mode RGBA")):
        refused(NotImplementedError, f"image 0: a paste of {text} is not built", P, [b], o)
    # ---- alpha_composite: Pillow's own ValueErrors for dest= and source=, word for word
    C = A.alpha_composite_many
    for dest, source in (((0, 0), (1, 2, 3)), ((0, 0, 0), (0, 0)), ((0, 0), (-1, 0)), ((0, 0), (3, 0, 2, 4)), ((0, 0), (0, 3, 2, 1)), ((0, 0), 5), (5, (0, 0))):
        with pytest.raises(ValueError) as theirs:
            pil(rgba).alpha_composite(pil(rgba), dest, source)
        refused(ValueError, "image 0: " + str(theirs.value), C, [rgba], rgba, dest, source)
    for b, o in ((rgb, rgb), (grey, grey), (rgb, rgba)):
        with pytest.raises(ValueError, match="image has wrong mode"):
            pil(b).alpha_composite(pil(o))
        refused(ValueError, "image 0: image has wrong mode", C, [b], o)
    with pytest.raises(ValueError, match="images do not match"):
        pil(rgba).alpha_composite(pil(la))
    refused(ValueError, "image 0: images do not match: modes RGBA and LA", C, [rgba], la)
    with pytest.raises(ValueError, match="images do not match"):
        pil(rgba).alpha_composite(pil(rgb))
    refused(ValueError, "image 0: images do not match: modes RGBA and RGB", C, [rgba], rgb)
    # ---- blend and composite
    refused(ValueError, "image 1: images do not match: sizes 7 x 6 and 3 x 2", A.blend_many, [rgb, rgb], [rgb, small], 0.5)
    refused(ValueError, "image 0: images do not match: modes RGB and RGBA", A.blend_many, [rgb], rgba, 0.5)
    with pytest.raises(ValueError, match="images do not match"):
        Image.blend(pil(rgb), pil(small), 0.5)
    refused(ValueError, "image 0: alpha inf is not finite as a float32", A.blend_many, [rgb], rgb, float("inf"))
    refused(ValueError, "image 0: alpha 1e+39 is not finite as a float32", A.blend_many, [rgb], rgb, 1e39)
    refused(ValueError, "image 0: alpha nan is not finite", A.blend_many, [rgb], rgb, float("nan"))
    refused(ValueError, "image 0: alpha 'x': a number required", A.blend_many, [rgb], rgb, "x")
    refused(ValueError, "alpha: 3 entries for 1 images", A.blend_many, [rgb], rgb, [0.1, 0.2, 0.3])
    big = np.zeros((8, 9, 3), np.uint8)
    refused(ValueError, "image 0: images do not match: sizes 7 x 6 and 9 x 8", A.composite_many, [rgb], big, np.zeros((6, 7), np.uint8))
    assert np.asarray(Image.composite(pil(rgb), pil(big), pil(np.zeros((6, 7), np.uint8)))).shape == (8, 9, 3)      # Pillow tolerates it
    assert "does not" in A.composite_many.__doc__ and "tolerates" in A.composite_many.__doc__
    refused(ValueError, "image 0: images do not match: a mask of 3 x 2", A.composite_many, [rgb], rgb, np.zeros((2, 3), np.uint8))
    refused(ValueError, "image 0: mask: a 3-channel image is no mask", A.composite_many, [rgb], rgb, rgb)
    refused(ValueError, "image 0: mask None", A.composite_many, [rgb], rgb, None)
    # ---- chops
    refused(ValueError, "image 0: images do not match: modes RGB and RGBA", A.chop_many, [rgb], rgba, "add")
    with pytest.raises(ValueError, match="images do not match"):
        ImageChops.add(pil(rgb), pil(rgba))
    for name in ("logical_and", "logical_or", "logical_xor", "offset", "invert"):
        refused(NotImplementedError, f"image 0: ImageChops.{name} is not built", A.chop_many, [rgb], rgb, name)
    refused(ValueError, "image 0: op 'blend'", A.chop_many, [rgb], rgb, "blend")
    refused(ValueError, "scale must be finite and not 0", A.chop_many, [rgb], rgb, A.ChopAdd(0.0))
    refused(ValueError, "scale must be finite and not 0", A.chop_many, [rgb], rgb, A.ChopSubtract(float("nan")))
    refused(ValueError, "offset: an int", A.chop_many, [rgb], rgb, A.ChopAdd(1.0, 2.5))
    refused(ValueError, "leaves the int range", A.chop_many, [rgb], rgb, A.ChopAdd(1e-8, 0))
    refused(ValueError, "op: 2 entries for 1 images", A.chop_many, [rgb], rgb, ["add", "add"])
