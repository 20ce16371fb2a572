"""CPU: the mode= keyword of standard_jpeg_decode_many / standard_jpeg_thumbnail_many / standard_jpeg_thumbnail_jpeg_many and the [H, W]
inputs of resize_many without a device -- validation before any device work, the C ABI's additions (include/aej.h against _lib.py),
and the fixtures tests/golden/jpeg_luma against live Pillow."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import jpeg_luma_reference as LR
from conftest import GOLDEN, ROOT

HERE = os.path.join(GOLDEN, "jpeg_luma")
NEW = ("aej_jpegdec_workspace_bytes_mode", "aej_jpegdec_batch_mode", "aej_jpegprog_workspace_bytes_mode", "aej_jpegprog_batch_mode",
       "aej_resample_workspace_bytes_ch", "aej_resample_batch_ch")


@pytest.fixture(scope="module")
def SJ():
    import adaptive_edge_aware_jpeg_amd.standard_jpeg as sj
    return sj


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "meta.json")) as f:
        return json.load(f), dict(np.load(os.path.join(HERE, "pixels.npz")))


def _file(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


@pytest.fixture()
def no_device(monkeypatch):
    """get_context raises: a call that reaches it has started device work"""
    import adaptive_edge_aware_jpeg_amd._lib as L
    import adaptive_edge_aware_jpeg_amd.resample as RS
    import adaptive_edge_aware_jpeg_amd.standard_jpeg as sj

    class Reached(Exception):
        pass

    def boom(*a, **k):
        raise Reached("get_context")
    for mod in (L, RS, sj):
        monkeypatch.setattr(mod, "get_context", boom)
    return Reached


def _calls(SJ, files):
    return {"decode": lambda m: SJ.standard_jpeg_decode_many(files, mode=m),
            "thumbnail": lambda m: SJ.standard_jpeg_thumbnail_many(files, (8, 8), mode=m),
            "thumbnail_jpeg": lambda m: SJ.standard_jpeg_thumbnail_jpeg_many(files, (8, 8), mode=m)}


def test_mode_is_checked_before_any_device_work(SJ, no_device):
    files = [_file("jpegdec/lena_64x64_420_q75"), _file("jpegdec/house_45x61_grey_q60")]
    for name, call in _calls(SJ, files).items():
        for bad in ("l", "LA", "YCbCr", "", "rgb", "Auto"):
            with pytest.raises(ValueError, match="every file: mode"):
                call(bad)
            with pytest.raises(ValueError, match="file 1: mode"):
                call(["L", bad])
        for bad in (None, 1, 1.0, True, b"L", {"L"}, np.array(["L", "L"])):
            with pytest.raises(TypeError, match="mode"):
                call(bad)
        with pytest.raises(TypeError, match="file 0: mode"):
            call([None, "L"])
        for wrong in (["L"], ("L", "L", "auto"), []):
            with pytest.raises(ValueError, match=rf"mode: {len(wrong)} values for 2 files"):
                call(wrong)
        for good in ("RGB", "L", "auto", ["RGB", "L"], ("auto", "auto")):      # a valid mode gets as far as the device and no further
            with pytest.raises(no_device):
                call(good)
    # the other keywords are still checked first, and a header that is refused names its file under every mode
    with pytest.raises(ValueError, match="scale"):
        SJ.standard_jpeg_decode_many(files, scale=3, mode="L")
    with pytest.raises(ValueError, match="file 1"):
        SJ.standard_jpeg_decode_many([files[0], files[1][:40]], mode="L")


def test_resize_many_ranks(no_device):
    import adaptive_edge_aware_jpeg_amd as A
    rgb, grey = np.zeros((8, 9, 3), np.uint8), np.zeros((8, 9), np.uint8)
    for bad in (np.zeros((8, 9, 4), np.uint8), np.zeros((8, 9, 1), np.uint8), np.zeros((8,), np.uint8), np.zeros((2, 8, 9, 3), np.uint8),
                np.zeros((0, 9), np.uint8)):
        with pytest.raises(ValueError, match=r"image 1: uint8 \[H, W\] or \[H, W, 3\] \(mode 'auto'\) required"):
            A.resize_many([grey, bad], (4, 4), mode="auto")
        with pytest.raises(ValueError, match=r"image 0: uint8 \[H, W\] \(mode 'L'\) required"):
            A.resize_many([bad], (4, 4), mode="L")
    # each mode takes its own ranks alone; without the keyword the call is as it was: [H, W] refused
    for images, mode, who in (([rgb, grey], "RGB", 1), ([grey, rgb], "L", 1), ([grey], None, 0)):
        with pytest.raises(ValueError, match=f"image {who}: uint8"):
            A.resize_many(images, (4, 4), **({} if mode is None else {"mode": mode}))
    for bad in ("l", "LA", None, 1):
        with pytest.raises(ValueError, match="mode"):
            A.resize_many([grey], (4, 4), mode=bad)
    with pytest.raises(TypeError, match="image 1: uint8"):
        A.resize_many([rgb, grey.astype(np.float32)], (4, 4), mode="auto")
    with pytest.raises(ValueError, match="image 1: box .*exceed"):
        A.resize_many([rgb, grey], (4, 4), box=[None, (0, 0, 10, 8)], mode="auto")
    for ok, mode in (([grey], "L"), ([grey, grey], "auto"), ([rgb, grey], "auto"), ([grey, rgb, grey], "auto"), ([rgb], "auto"), ([rgb], "RGB")):
        with pytest.raises(no_device):
            A.resize_many(ok, (4, 4), mode=mode)


def _params(header, name):
    """the parameter types of `name`'s prototype in the header, as _lib.py's letters"""
    m = re.search(r"AEJ_API\s+(\w+)\s+" + name + r"\(([^;]*)\);", header)
    assert m, name
    out = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        out.append("P" if "*" in p else "U64" if p.startswith("uint64_t") else "I64" if p.startswith("int64_t") else "I" if p.startswith("int ") else p)
    return m.group(1), out


def test_abi_additions():
    from adaptive_edge_aware_jpeg_amd import _lib as L
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "aej.h")) as f:
        header = f.read()
    letters = {L._P: "P", L._I: "I", L._I64: "I64", L._U64: "U64"}
    for name in NEW:
        assert getattr(lib, name) is not None
        res, args = L.SIGNATURES[name]
        hres, hargs = _params(header, name)
        assert [letters[a] for a in args] == hargs, name
        assert {"uint64_t": L._U64, "int": L._I}[hres] is res, name
    # each is its sibling plus one int array: after scales_host (decoders), after n (resample)
    for new, old, at in (("aej_jpegdec_batch_mode", "aej_jpegdec_batch_scaled", 4), ("aej_jpegdec_workspace_bytes_mode", "aej_jpegdec_workspace_bytes_scaled", 4),
                         ("aej_jpegprog_batch_mode", "aej_jpegprog_batch_scaled", 5), ("aej_jpegprog_workspace_bytes_mode", "aej_jpegprog_workspace_bytes_scaled", 5),
                         ("aej_resample_batch_ch", "aej_resample_batch", 3), ("aej_resample_workspace_bytes_ch", "aej_resample_workspace_bytes", 3)):
        a, b = list(L.SIGNATURES[new][1]), list(L.SIGNATURES[old][1])
        assert a[:at] + a[at + 1:] == b and a[at] is L._P and L.SIGNATURES[new][0] is L.SIGNATURES[old][0], new
        assert re.search(new + r"\([^;]*const int \*(components|channels)_host", header), new
    assert lib.aej_abi_version() == 3
    # no struct changed: the sizes of the parent commit
    assert ctypes.sizeof(L.ResampleDesc) == 80 and ctypes.sizeof(L.JpegDecDesc) == 9008
    assert re.search(r"int32_t reserved;\s*/\* 0 \*/\s*\} aej_resample_desc;", header)


def test_workspace_queries_refuse_other_counts():
    """host only: no context is needed to be refused"""
    from adaptive_edge_aware_jpeg_amd import _lib as L
    lib = L.load_library()
    two = (ctypes.c_int * 1)(2)
    assert lib.aej_jpegdec_workspace_bytes_mode(None, None, 1, None, ctypes.addressof(two)) == 0
    assert lib.aej_resample_workspace_bytes_ch(None, None, 1, ctypes.addressof(two)) == 0
    assert lib.aej_jpegdec_batch_mode(None, None, 1, None, None, None, 0, None, None, 0, None, None, None, 0) == -1      # AEJ_ERR_ARG
    assert lib.aej_resample_batch_ch(None, None, 1, None, None, 0, None, 0, None, 0) == -1


def test_fixtures_tell_the_two_meanings_of_L_apart(golden):
    """draft("L") -- the luma plane -- against convert("RGB").convert("L") -- ITU-R 601 over the clamped RGB: for every sampling at least one
    colour fixture where they differ, or the pixel tests could not tell which one the library returns"""
    meta, px = golden
    seen = {}
    for c in meta["cases"]:
        if c["sampling"] == "grey":
            continue
        Image = pytest.importorskip("PIL.Image")
        import io
        data = _file(c["name"])
        conv = np.asarray(Image.open(io.BytesIO(data)).convert("RGB").convert("L"))
        luma = px[c["name"] + "/L1"]
        assert luma.shape == conv.shape
        seen[c["sampling"]] = max(seen.get(c["sampling"], 0), int((luma != conv).sum()))
    for samp in ("4:4:4", "4:2:2", "4:2:0"):
        assert seen.get(samp, 0) >= 1, samp


def test_fixtures_are_complete_and_shaped(golden):
    meta, px = golden
    assert len(meta["cases"]) >= 30 and {c["sampling"] for c in meta["cases"]} >= {"grey", "4:4:4", "4:2:2", "4:2:0"}
    for c in meta["cases"]:
        W, H = c["size"]
        grey = c["sampling"] == "grey"
        for s in meta["scales"]:
            assert px[f"{c['name']}/L{s}"].shape == (-(-H // s), -(-W // s)) and px[f"{c['name']}/L{s}"].dtype == np.uint8
        assert px[c["name"] + "/auto"].shape == ((H, W) if grey else (H, W, 3))
        if grey:
            assert np.array_equal(px[c["name"] + "/auto"], px[c["name"] + "/L1"])
        for mode in ("L", "auto"):
            for size in meta["sizes"]:
                for r in meta["resample"]:
                    for g in meta["gaps"]:
                        t = px[f"{c['name']}/t{mode}_{size[0]}x{size[1]}_{r}_{g}"]
                        assert t.ndim == (2 if grey or mode == "L" else 3) and t.shape[0] <= max(size[1], H) and t.shape[1] <= max(size[0], W)


def test_fixtures_equal_live_pillow(golden, SJ):
    features = pytest.importorskip("PIL.features")
    meta, px = golden
    if features.version("libjpeg_turbo") != meta["libjpeg_turbo"]:
        pytest.skip(f"libjpeg-turbo {features.version('libjpeg_turbo')}: the fixtures were made by {meta['libjpeg_turbo']}")
    for c in meta["cases"]:
        data = _file(c["name"])
        assert LR.sampling(data) == c["sampling"]
        for s in meta["scales"]:
            assert np.array_equal(LR.draft_l(data, s), px[f"{c['name']}/L{s}"]), (c["name"], s)
            if c["sampling"] != "grey":              # the luma plane is channel 0 of the YCbCr decode, at every scale
                assert np.array_equal(np.asarray(LR.draft(data, "YCbCr", s))[..., 0], px[f"{c['name']}/L{s}"]), (c["name"], s)
        assert np.array_equal(LR.auto(data), px[c["name"] + "/auto"])
        for mode in ("L", "auto"):
            for size in meta["sizes"]:
                for r in meta["resample"]:
                    for g in meta["gaps"]:
                        key = f"{c['name']}/t{mode}_{size[0]}x{size[1]}_{r}_{g}"
                        assert np.array_equal(LR.thumbnail(data, tuple(size), r, g, mode, SJ.thumbnail_plan), px[key]), key


def test_mode_L_resize_is_one_channel_of_the_rgb_resize():
    """why tests/resample_reference.py serves as the one-channel model untouched"""
    Image = pytest.importorskip("PIL.Image")
    import resample_reference as M
    rng = np.random.default_rng(5)
    for it in range(40):
        H, W, w, h = (int(v) for v in rng.integers(1, 60, 4))
        a = rng.integers(0, 256, (H, W), dtype=np.uint8)
        f = tuple(M.FILTERS)[it % 5]
        gap = (None, 1.0, 2.0, 1.5)[it % 4]
        try:
            model = M.resize(np.stack([a] * 3, -1), (w, h), f, None, gap)[..., 0]
        except NotImplementedError:
            continue
        want = np.asarray(Image.fromarray(a).resize((w, h), M.FILTERS[f], reducing_gap=gap))
        assert want.ndim == 2 and np.array_equal(model, want), (it, H, W, w, h, f, gap)
