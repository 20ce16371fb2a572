"""Standard JPEG with Pillow's subsampling= and optimize= on the host side: the numpy restatement pinned to Pillow, the library's
optimal-table routine (aej_jfif_huffman_host, the code the device runs per table) and option-aware markers against Pillow's files, the
ABI and the argument checks (no GPU needed)."""
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
import jfif_reference as R  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
from adaptive_edge_aware_jpeg_amd import standard_jpeg as S  # noqa: E402
from adaptive_edge_aware_jpeg_amd._lib import SIGNATURES, load_library  # noqa: E402

NEW = ("aej_jfif_workspace_bytes_opt", "aej_jfif_headers_host_opt", "aej_jfif_huffman_host", "aej_jfif_encode_batch_opt",
       "aej_jfif_recon_batch_opt")
LAYOUTS = ("4:4:4", "4:2:2", "4:2:0")
FIXTURES = os.path.join(GOLDEN, "jfif_options")


def _pil(x, q, ss, opt):
    """Pillow's file.  With optimize=True libjpeg writes the whole scan in one piece and Pillow sizes that buffer as W * H (2 W * H from
    quality 95), which noise at 4:4:4 exceeds ("Suspension not allowed here"); a larger ImageFile.MAXBLOCK is Pillow's documented way
    round it and does not change the bytes."""
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * x.shape[0] * x.shape[1] + 4096)
    try:
        Image.fromarray(x).save(buf, "JPEG", quality=q, subsampling=ss, optimize=opt)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


def _pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _lena():
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, "lena.png")).convert("RGB"))


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _cases():
    lena = _lena()
    return [_noise(37, 53, 4), np.ascontiguousarray(lena[200:261, 230:320]), np.ascontiguousarray(lena[100:228, 90:250]),
            np.full((16, 24, 3), (30, 140, 220), np.uint8), _noise(1, 1, 5), _noise(9, 3, 6), _noise(17, 5, 7), _noise(16, 16, 8)]


def _dht_segments(data):
    """the (class/id byte, BITS, HUFFVAL) of every DHT segment before SOS, in file order"""
    out, i = [], 2
    while data[i + 1] != 0xDA:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] == 0xC4:
            body = data[i + 4:i + 2 + n]
            assert sum(body[1:17]) == len(body) - 17             # Pillow writes one table per segment
            out.append((body[0], list(body[1:17]), list(body[17:])))
        i += 2 + n
    return out


@pytest.mark.parametrize("q", [1, 10, 50, 90, 100])
@pytest.mark.parametrize("ss", LAYOUTS)
def test_restatement_equals_pillow_bytes_and_decode(ss, q):
    for x in _cases():
        for opt in (False, True):
            data = _pil(x, q, ss, opt)
            assert O.encode(x, q, ss, opt) == data, (x.shape, ss, opt, q)
            assert np.array_equal(O.decode(x, q, ss), _pil_decode(data)), (x.shape, ss, opt, q)


def test_restatement_default_is_the_existing_one():
    x = _noise(37, 53, 9)
    assert O.encode(x, 75) == R.encode(x, 75) and np.array_equal(O.decode(x, 75), R.decode(x, 75))
    assert O.encode(x, 75, 2) == R.encode(x, 75) and O.headers(75, 37, 53) == R.headers(75, 37, 53)


def test_restatement_narrow_images():
    """chroma at most 2 samples wide: the decoder replicates instead of the fancy filter (4:2:2, W <= 4); 4:4:4 never up-samples"""
    for ss in ("4:2:2", "4:4:4"):
        for W in (1, 2, 3, 4, 5):
            for H in (1, 2, 9, 16, 17):
                x = _noise(H, W, 10 * H + W)
                for q, opt in ((10, True), (100, False)):
                    data = _pil(x, q, ss, opt)
                    assert O.encode(x, q, ss, opt) == data, (H, W, ss, q)
                    assert np.array_equal(O.decode(x, q, ss), _pil_decode(data)), (H, W, ss, q)


@pytest.mark.parametrize("ss", LAYOUTS)
def test_host_tables_equal_pillow_dht(ss):
    """aej_jfif_huffman_host over the histogram of a file's own coefficients gives the four DHT segments Pillow wrote"""
    for x in _cases():
        for q in (1, 10, 50, 90, 100):
            dht = _dht_segments(_pil(x, q, ss, True))
            assert [d[0] for d in dht] == [0x00, 0x10, 0x01, 0x11]
            hist = O.histogram(O.coefficients(x, q, ss))
            for t in range(4):
                got = S.huffman_table(hist[t])
                assert got == (dht[t][1], dht[t][2]), (x.shape, ss, q, t)
                assert got == tuple(list(v) for v in O.optimal_table(hist[t]))


def test_host_tables_degenerate():
    # a flat image: every AC table holds EOB alone (one symbol of length 1), every DC table two symbols (the first diff and 0)
    flat = np.full((16, 24, 3), (30, 140, 220), np.uint8)
    for ss in LAYOUTS:
        hist = O.histogram(O.coefficients(flat, 50, ss))
        dht = _dht_segments(_pil(flat, 50, ss, True))
        for t in range(4):
            bits, vals = S.huffman_table(hist[t])
            assert (bits, vals) == (dht[t][1], dht[t][2])
            if t & 1:
                assert vals == [0] and bits == [1] + [0] * 15
            else:
                assert len(vals) == 2
    # one symbol, wherever it is
    for sym in (0, 7, 255):
        c = np.zeros(257, np.int64)
        c[sym] = 12345
        assert S.huffman_table(c) == ([1] + [0] * 15, [sym])
    # two equal counts: the tie goes to the larger index, so it is merged first and both get two bits next to the reserved code ...
    c = np.zeros(257, np.int64)
    c[3] = c[9] = 5
    assert S.huffman_table(c) == tuple(list(v) for v in O.optimal_table(c))
    # entry 256 is the reserved code whatever the caller put there
    c2 = c.copy()
    c2[256] = 99
    assert S.huffman_table(c2) == S.huffman_table(c)


def test_host_tables_length_limit():
    """Fibonacci-like counts give code lengths far beyond 16 bits before the K.3 adjustment"""
    fib = [1, 1]
    while len(fib) < 60:
        fib.append(fib[-1] + fib[-2])
    g = np.random.default_rng(3)
    for n, perm in ((20, False), (40, False), (60, True), (60, False)):
        c = np.zeros(257, np.int64)
        idx = g.permutation(256)[:n] if perm else np.arange(n)
        c[idx] = fib[:n]
        want = O.optimal_table(c)
        bits, vals = S.huffman_table(c)
        assert (bits, vals) == (list(want[0]), list(want[1])), n
        assert len(vals) == n and sum(bits) == n
        assert sum(b * 2 ** (16 - k) for k, b in enumerate(bits, 1)) < 2 ** 16      # Kraft, with room for the reserved code
    dense = g.integers(1, 1000, 257)
    want = O.optimal_table(dense)
    assert S.huffman_table(dense) == (list(want[0]), list(want[1]))


def test_host_table_argument_errors():
    lib = load_library()
    bits, vals = (ctypes.c_uint8 * 16)(), (ctypes.c_uint8 * 256)()
    b, v = ctypes.addressof(bits), ctypes.addressof(vals)
    zero = np.zeros(257, np.int64)
    assert lib.aej_jfif_huffman_host(zero.ctypes.data, b, v, 256) == -1
    neg = zero.copy()
    neg[5], neg[6] = 3, -1
    assert lib.aej_jfif_huffman_host(neg.ctypes.data, b, v, 256) == -1
    assert lib.aej_jfif_huffman_host(None, b, v, 256) == -1
    ok = zero.copy()
    ok[1], ok[2], ok[3] = 5, 6, 7
    assert lib.aej_jfif_huffman_host(ok.ctypes.data, b, v, 2) == -4
    assert lib.aej_jfif_huffman_host(ok.ctypes.data, b, v, 3) == 3
    for bad in (zero, neg, np.zeros(256, np.int64)):
        with pytest.raises(ValueError):
            S.huffman_table(bad)


@pytest.mark.parametrize("q,H,W", [(1, 1, 1), (10, 16, 16), (50, 37, 53), (90, 2160, 3840), (100, 3, 65500)])
def test_option_headers_equal_pillow(q, H, W):
    x = np.zeros((H, W, 3), np.uint8)
    for ss, code, sampling in (("4:4:4", 0, 0x11), ("4:2:2", 1, 0x21), ("4:2:0", 2, 0x22)):
        data = _pil(x, q, ss, False)
        hdr = S.headers(q, H, W, ss)
        assert hdr == S.headers(q, H, W, code) == O.headers(q, H, W, ss)
        assert len(hdr) == 623 and data[:623] == hdr and hdr[-14:-12] == b"\xff\xda"
        sof = hdr.index(b"\xff\xc0")
        assert hdr[sof + 11] == sampling
    assert S.headers(q, H, W) == S.headers(q, H, W, "4:2:0")


def test_fixtures_are_what_the_restatement_writes():
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        meta = json.load(f)
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    pairs = set()
    for case in meta["cases"]:
        name = case["name"]
        with open(os.path.join(FIXTURES, name + ".jpg"), "rb") as f:
            want = f.read()
        assert O.encode(px[name + "_src"], case["quality"], case["subsampling"], case["optimize"]) == want, name
        assert np.array_equal(O.decode(px[name + "_src"], case["quality"], case["subsampling"]), px[name + "_dec"]), name
        pairs.add((case["subsampling"], case["optimize"]))
    assert pairs == {(s, o) for s in LAYOUTS for o in (False, True)}


def test_symbols_exported_and_declared():
    lib = load_library()
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "aej.h")) as f:
        h = f.read()
    for name in NEW:
        assert name in SIGNATURES
        assert getattr(lib, name) is not None
        assert f" {name}(" in h
    assert lib.aej_abi_version() == 3


def test_c_argument_errors():
    lib = load_library()
    buf = ctypes.create_string_buffer(1024)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for ss in (-1, 3):
        assert lib.aej_jfif_headers_host_opt(50, 8, 8, ss, p, 1024) == -1
        assert lib.aej_jfif_workspace_bytes_opt(1, 8, 8, 1, ss, 0) == 0
    assert lib.aej_jfif_workspace_bytes_opt(1, 8, 8, 1, 2, 2) == 0
    assert lib.aej_jfif_headers_host_opt(50, 8, 8, 0, p, 100) == -4
    # the default options are the existing entry points
    assert lib.aej_jfif_workspace_bytes_opt(2, 37, 53, 3, 2, 0) == lib.aej_jfif_workspace_bytes(2, 37, 53, 3)
    # 4:4:4 holds twice the blocks of 4:2:0 (12 against 6 per 16 x 16 pixels), and per-file tables need room of their own
    w420, w422, w444 = (lib.aej_jfif_workspace_bytes_opt(4, 256, 256, 2, ss, 0) for ss in (2, 1, 0))
    assert w420 < w422 < w444 and w444 > 1.8 * w420
    assert lib.aej_jfif_workspace_bytes_opt(4, 256, 256, 2, 2, 1) > w420
    assert lib.aej_jfif_encode_batch_opt(None, None, 1, 8, 8, 1, None, 0, 1, None, 0, None, None, None, None, 0) == -1
    assert lib.aej_jfif_recon_batch_opt(None, 1, 8, 8, 1, 0, 1, None, None, 0) == -1


def test_python_argument_errors_need_no_device(monkeypatch):
    """bad options are refused before a context is created"""
    def no_context(*a, **k):
        raise AssertionError("a context was requested before the arguments were checked")
    monkeypatch.setattr(S, "get_context", no_context)
    SW = sys.modules["adaptive_edge_aware_jpeg_amd.sweep"]          # the package attribute `sweep` is the function
    monkeypatch.setattr(SW, "get_context", no_context)
    x = np.zeros((1, 8, 8, 3), np.uint8)
    for bad in ("4:1:1", "keep", -1, 3, True, False, None, 1.0, "420"):
        with pytest.raises(ValueError, match="subsampling") as e:
            A.standard_jpeg_many(x, 50, subsampling=bad)
        assert repr(bad) in str(e.value)
        with pytest.raises(ValueError, match="subsampling"):
            A.standard_jpeg_batch(x, [50], subsampling=bad)
        with pytest.raises(ValueError, match="subsampling"):
            A.sweep(x.astype(np.float32), metrics=0, sizes=None, standard_qualities=[50], standard_subsampling=bad)
        with pytest.raises(ValueError, match="subsampling"):
            A.sweep(x.astype(np.float32), metrics=0, sizes=None, standard_subsampling=bad)
        with pytest.raises(ValueError):
            S.headers(50, 8, 8, bad)
    for bad in (0, 1, "yes", None, 1.0):
        with pytest.raises(TypeError, match="optimize"):
            A.standard_jpeg_many(x, 50, optimize=bad)
        with pytest.raises(TypeError, match="optimize"):
            A.standard_jpeg_batch(x, [50], optimize=bad)
        with pytest.raises(TypeError, match="optimize"):
            A.sweep(x.astype(np.float32), metrics=0, sizes=None, standard_qualities=[50], standard_optimize=bad)
        with pytest.raises(TypeError, match="optimize"):
            A.sweep(x.astype(np.float32), metrics=0, sizes=None, standard_optimize=bad)
    # options that would be ignored are refused too
    with pytest.raises(ValueError, match="standard_qualities"):
        A.sweep(x.astype(np.float32), metrics=0, sizes=None, standard_subsampling="4:4:4")
    with pytest.raises(ValueError, match="standard_qualities"):
        A.sweep(x.astype(np.float32), metrics=0, sizes=None, standard_optimize=True)
    with pytest.raises(ValueError):
        A.standard_jpeg_batch(x, [0], subsampling="4:4:4")


def test_standard_result_records_the_setting(tmp_path):
    from adaptive_edge_aware_jpeg_amd.sweep import StandardResult, SweepResult
    st = StandardResult([10, 90], 2)
    assert (st.subsampling, st.optimize) == ("4:2:0", False)
    st = StandardResult([10], 1, subsampling="4:4:4", optimize=True)
    assert (st.subsampling, st.optimize) == ("4:4:4", True)
    res = SweepResult([("YCbCr", (50, 50), (8, 8))], ["a"], [(8, 8)], 7, None)
    res.standard = st
    st.psnr[:], st.ssim[:], st.ms_ssim[:], st.compression_ratio[:] = 30, 0.5, 0.25, 10
    res.to_csv_standard(tmp_path / "s.csv")
    assert (tmp_path / "s.csv").read_text().splitlines()[0] == "image_name,quality,psnr,ssim,ms_ssim,compression_ratio"
