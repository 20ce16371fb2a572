"""Standard JPEG with Pillow's progressive=True on the host side: the Python restatement pinned to Pillow byte for byte, the coverage of
both cut rules of the end-of-band runs, the library's host core (aej_test_jfif_prog_scan_host, the text the kernels run) against the
restatement on synthetic coefficients, the fixtures, the ABI and the argument checks (no GPU needed)."""
import ctypes
import io
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_options_reference as O  # noqa: E402
import jfif_progressive_reference as P  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
from adaptive_edge_aware_jpeg_amd import standard_jpeg as S  # noqa: E402
from adaptive_edge_aware_jpeg_amd._lib import SIGNATURES, load_library  # noqa: E402

NEW = ("aej_jfif_workspace_bytes_prog", "aej_jfif_encode_batch_prog", "aej_jfif_recon_batch_prog")
NEW_TESTING = ("aej_test_jfif_prog_scan_host", "aej_test_jfif_prog_scan")
LAYOUTS = ("4:4:4", "4:2:2", "4:2:0")
SIZES = [(1, 1), (8, 8), (9, 4), (17, 33), (37, 53), (61, 90), (255, 257)]
FIXTURES = os.path.join(GOLDEN, "jfif_progressive")
NOISE_SEED = 1


def _pil(x, q, ss, **kw):
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * x.shape[0] * x.shape[1] + 4096)
    try:
        Image.fromarray(x).save(buf, "JPEG", quality=q, subsampling=ss, progressive=True, **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


def _lena():
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, "lena.png")).convert("RGB"))


def _images(H, W):
    """natural, noise, flat, primaries"""
    lena = _lena()
    nat = np.ascontiguousarray(np.tile(lena, (-(-H // lena.shape[0]), -(-W // lena.shape[1]), 1))[:H, :W])
    prim = np.zeros((H, W, 3), np.uint8)
    band = np.arange(W) * 3 // max(W, 1)
    for c in range(3):
        prim[:, :, c] = np.where(band == c, 255, 0)
    prim[H // 2:] = 255 - prim[H // 2:]
    return [nat, np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8), np.full((H, W, 3), (201, 17, 90), np.uint8), prim]


@pytest.mark.parametrize("ss", LAYOUTS)
@pytest.mark.parametrize("H,W", SIZES)
def test_restatement_equals_pillow(H, W, ss):
    for x in _images(H, W):
        for q in (1, 10, 50, 75, 95, 100):
            data, cuts = P.encode(x, q, ss)
            assert data == _pil(x, q, ss), (H, W, ss, q)
            assert len(cuts) == 10


def test_optimize_changes_nothing_in_pillow():
    x = _images(37, 53)[1]
    for ss in LAYOUTS:
        assert _pil(x, 75, ss) == _pil(x, 75, ss, optimize=True)


def test_both_cut_rules_are_covered():
    """the pixel-level set holds a file whose runs are cut at 0x7FFF blocks and one cut by the 937-bit rule (tests/test_gpu_jfif_progressive.py
    encodes the same two on the device)"""
    flat = np.full((1536, 1536, 3), (30, 140, 220), np.uint8)
    data, cuts = P.encode(flat, 75, "4:4:4")
    assert data == _pil(flat, 75, "4:4:4")
    assert sum(c[0] for c in cuts) >= 1 and [c[0] for c in cuts][1] == 1
    noise = np.random.default_rng(NOISE_SEED).integers(0, 2, (512, 512, 3), dtype=np.uint8) * 255
    data, cuts = P.encode(noise, 100, "4:4:4")
    assert data == _pil(noise, 100, "4:4:4")
    assert sum(c[1] for c in cuts) >= 1


def test_fixtures_are_what_the_restatement_writes():
    from PIL import Image
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        meta = json.load(f)
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    assert {c["subsampling"] for c in meta["cases"]} == set(LAYOUTS) and len(meta["cases"]) == 8
    for case in meta["cases"]:
        name = case["name"]
        with open(os.path.join(FIXTURES, name + ".jpg"), "rb") as f:
            want = f.read()
        assert P.encode(px[name + "_src"], case["quality"], case["subsampling"])[0] == want, name
        assert np.array_equal(O.decode(px[name + "_src"], case["quality"], case["subsampling"]), px[name + "_dec"]), name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(want)).convert("RGB")), px[name + "_dec"]), name


def test_scan_script_of_pillow_and_restatement():
    x = _images(37, 53)[0]
    for ss in LAYOUTS:
        data = P.encode(x, 75, ss)[0]
        frame, scans = S.parse_scans(data)
        assert (frame.height, frame.width, frame.n_scans, frame.sof) == (37, 53, 10, 0xC2)
        assert [(s.ss, s.se, s.ah, s.al) for s in scans] == [(c[1], c[2], c[3], c[4]) for c in P.SCRIPT]
        assert [[s.comp[k] for k in range(s.ncomp)] for s in scans] == [list(c[0]) for c in P.SCRIPT]
        # marker order: SOI APP0 DQT DQT SOF2, then DHT DHT SOS, then per scan [DHT] SOS (none before the DC refinement), then EOI
        markers, i = [], 2
        while data[i + 1] != 0xDA:
            markers.append(data[i + 1])
            i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
        assert markers == [0xE0, 0xDB, 0xDB, 0xC2, 0xC4, 0xC4]
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
        for k, s in enumerate(scans[1:], 1):
            sos = s.data_offset - (8 + 2 * s.ncomp)
            assert data[sos:sos + 2] == b"\xff\xda"
            prev = scans[k - 1]
            gap = data[prev.data_offset + prev.data_length:sos]
            if s.ss == 0:
                assert gap == b""
            else:
                assert gap[:2] == b"\xff\xc4" and gap[4] == (0x11 if s.comp[0] else 0x10) and len(gap) == 2 + int.from_bytes(gap[2:4], "big")


def _scan_host(c, ss, se, ah, al, cap=None):
    lib = load_library()
    c = np.ascontiguousarray(c, np.int16)
    cap = 64 + c.shape[0] * 8 * (se - ss + 2) if cap is None else cap
    out, n = (ctypes.c_uint8 * max(cap, 1))(), ctypes.c_uint64()
    counts, cuts = np.zeros(257, np.int64), np.zeros(2, np.int64)
    rc = lib.aej_test_jfif_prog_scan_host(c.ctypes.data, c.shape[0], ss, se, ah, al, ctypes.addressof(out), cap, ctypes.addressof(n),
                                          counts.ctypes.data, cuts.ctypes.data)
    return rc, bytes(out[:min(n.value, cap)]), counts, tuple(int(v) for v in cuts), n.value


def test_host_core_equals_restatement_on_synthetic_coefficients():
    seen = set()
    for name, c, ss, se, ah, al, want_cuts in P.synthetic_cases():
        rc, data, counts, cuts, _ = _scan_host(c, ss, se, ah, al)
        want = P.encode_scan(list(c.astype(np.int64)), ss, se, ah, al)
        assert rc == 0, name
        assert data == want[0], name
        assert np.array_equal(counts, want[1]), name
        assert cuts == tuple(want[2]), name
        if want_cuts is not None:
            assert cuts == want_cuts, name
        seen.add(name.split("_")[0])
    assert {"zrl", "deferred", "chain", "zero", "all", "only", "dense", "dc", "random"} <= seen


def test_host_core_on_a_file_s_own_scans():
    """every AC scan of a real image through the host core equals the scan data in Pillow's file"""
    x = _images(61, 90)[0]
    data = _pil(x, 50, "4:2:0")
    _, scans = S.parse_scans(data)
    _, comps = P.component_blocks(x, 50, "4:2:0")
    for (cs, ss, se, ah, al), s in zip(P.SCRIPT, scans):
        if ss == 0:
            continue
        rc, got, _, _, _ = _scan_host(np.array(comps[cs[0]], np.int16), ss, se, ah, al)
        assert rc == 0 and got == data[s.data_offset:s.data_offset + s.data_length], (cs, ss, se, ah, al)


def test_host_core_argument_errors():
    c = np.zeros((2, 64), np.int16)
    assert _scan_host(c, 1, 63, 1, 0, cap=0)[0] == -4 and _scan_host(c, 1, 63, 1, 0, cap=0)[4] == 1
    for bad in ((0, 5, 0, 0), (5, 4, 0, 0), (1, 64, 0, 0), (1, 63, 3, 1), (-1, 0, 0, 0), (1, 63, 0, 14)):
        assert _scan_host(c, *bad)[0] == -1, bad
    big = c.copy()
    big[1, 7] = 2048
    assert _scan_host(big, 1, 63, 0, 0)[0] == -1
    lib = load_library()
    assert lib.aej_test_jfif_prog_scan_host(None, 1, 1, 63, 0, 0, None, 0, None, None, None) == -1


def test_symbols_exported_and_declared():
    lib = load_library()
    root = os.path.join(os.path.dirname(GOLDEN), "..")
    with open(os.path.join(root, "include", "aej.h")) as f:
        h = f.read()
    with open(os.path.join(root, "include", "aej_testing.h")) as f:
        ht = f.read()
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in NEW + NEW_TESTING:
        assert name in SIGNATURES
        assert getattr(lib, name) is not None
        assert f" {name}(" in (h if name in NEW else ht)
    for name in NEW:
        assert name in doc
    assert lib.aej_abi_version() == 3


def test_c_argument_errors():
    lib = load_library()
    for ss in (-1, 3):
        assert lib.aej_jfif_workspace_bytes_prog(1, 8, 8, 1, ss) == 0
    assert lib.aej_jfif_workspace_bytes_prog(0, 8, 8, 1, 2) == 0
    assert lib.aej_jfif_workspace_bytes_prog(1, 8, 70000, 1, 2) == 0
    w = [lib.aej_jfif_workspace_bytes_prog(4, 256, 256, 2, ss) for ss in (2, 1, 0)]
    assert 0 < w[0] < w[1] < w[2]
    assert w[0] > lib.aej_jfif_workspace_bytes_opt(4, 256, 256, 2, 2, 1)          # ten scans need more room than one
    assert lib.aej_jfif_encode_batch_prog(None, None, 1, 8, 8, 1, None, 0, None, 0, None, None, None, None, 0) == -1
    assert lib.aej_jfif_recon_batch_prog(None, 1, 8, 8, 1, 0, None, None, 0) == -1


def test_python_argument_errors_need_no_device(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a context was requested before the arguments were checked")
    monkeypatch.setattr(S, "get_context", no_context)
    SW = sys.modules["adaptive_edge_aware_jpeg_amd.sweep"]
    monkeypatch.setattr(SW, "get_context", no_context)
    x = np.zeros((1, 8, 8, 3), np.uint8)
    for bad in (0, 1, "yes", None, 1.0):
        with pytest.raises(TypeError, match="progressive"):
            A.standard_jpeg_many(x, 50, progressive=bad)
        with pytest.raises(TypeError, match="progressive"):
            A.standard_jpeg_batch(x, [50], progressive=bad)
        with pytest.raises(TypeError, match="progressive"):
            A.sweep(x.astype(np.float32), metrics=0, sizes=None, standard_qualities=[50], standard_progressive=bad)
    with pytest.raises(ValueError, match="standard_qualities"):
        A.sweep(x.astype(np.float32), metrics=0, sizes=None, standard_progressive=True)
    with pytest.raises(TypeError, match="optimize"):
        A.standard_jpeg_many(x, 50, optimize=1, progressive=True)
    with pytest.raises(ValueError):
        A.standard_jpeg_batch(x, [0], progressive=True)


def test_standard_result_records_the_setting(tmp_path):
    from adaptive_edge_aware_jpeg_amd.sweep import StandardResult, SweepResult
    assert StandardResult([10, 90], 2).progressive is False
    st = StandardResult([10], 1, subsampling="4:4:4", progressive=True)
    assert (st.subsampling, st.optimize, st.progressive) == ("4:4:4", False, True)
    res = SweepResult([("YCbCr", (50, 50), (8, 8))], ["a"], [(8, 8)], 7, None)
    res.standard = st
    st.psnr[:], st.ssim[:], st.ms_ssim[:], st.compression_ratio[:] = 30, 0.5, 0.25, 10
    res.to_csv_standard(tmp_path / "s.csv")
    assert (tmp_path / "s.csv").read_text().splitlines()[0] == "image_name,quality,psnr,ssim,ms_ssim,compression_ratio"
