"""GPU: standard JPEG with Pillow's progressive=True (csrc/jfifprog.hip) byte-identical to Pillow's files, its pixels unchanged, and the
kernels equal to the host core on the corners of the Annex G coder that pixels do not reach."""
import ctypes
import io
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_progressive_reference as P  # noqa: E402
import test_gpu_jfif as T  # noqa: E402  (its image helpers: _images, _fit, _png, _pil_decode)

pytestmark = pytest.mark.gpu
QUALITIES = (1, 10, 25, 50, 75, 90, 95, 100)
SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 53), (255, 257), (634, 505), (1080, 1920), (2160, 3840)]
LAYOUTS = ("4:4:4", "4:2:2", "4:2:0")
FIXTURES = os.path.join(GOLDEN, "jfif_progressive")
NOISE_SEED = 1                         # 0 / 255 noise of this seed takes a 937-bit cut (tests/test_jfif_progressive_host.py asserts it)


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _live_matches_fixtures():
    from PIL import features
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        return features.version("libjpeg_turbo") == json.load(f)["libjpeg_turbo"]


live = pytest.mark.skipif(not _live_matches_fixtures(), reason="this Pillow's libjpeg-turbo is not the one the fixtures pin")


def _pil(x, q, ss, **kw):
    """Pillow's progressive file; libjpeg writes it in one piece, so the buffer Pillow sizes from W * H is enlarged (ImageFile.MAXBLOCK
    is Pillow's documented way and does not change the bytes)."""
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * x.shape[0] * x.shape[1] + 4096)
    try:
        Image.fromarray(x).save(buf, "JPEG", quality=q, subsampling=ss, progressive=True, **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


def cut_inputs():
    """(image, quality, layout): one whose end-of-band runs reach 0x7FFF blocks, one that defers more than 937 correction bits"""
    flat = np.full((1536, 1536, 3), (30, 140, 220), np.uint8)
    noise = np.random.default_rng(NOISE_SEED).integers(0, 2, (512, 512, 3), dtype=np.uint8) * 255
    return [(flat, 75, "4:4:4"), (noise, 100, "4:4:4")]


def test_fixtures_bytes_and_pixels(A):
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        meta = json.load(f)
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    seen = set()
    for case in meta["cases"]:
        name, q, ss = case["name"], case["quality"], case["subsampling"]
        seen.add(ss)
        src = px[name + "_src"]
        with open(os.path.join(FIXTURES, name + ".jpg"), "rb") as f:
            want = f.read()
        f32 = src.astype(np.float32) / np.float32(255)
        for x in (src, f32):
            for opt in (False, True):
                assert A.standard_jpeg_many(x, q, subsampling=ss, optimize=opt, progressive=True) == [want], (name, opt)
                sizes, dec = A.standard_jpeg_batch(x[None], [q], subsampling=ss, optimize=opt, progressive=True)
                assert sizes.tolist() == [[len(want)]], name
                assert np.array_equal(dec[0, 0].cpu().numpy(), px[name + "_dec"]), name
    assert seen == set(LAYOUTS)


@live
@pytest.mark.parametrize("ss", LAYOUTS)
@pytest.mark.parametrize("H,W", SIZES)
def test_bytes_equal_pillow(A, H, W, ss):
    x = T._images(H, W, H * 7 + W)
    sizes, dec = A.standard_jpeg_batch(x, QUALITIES, subsampling=ss, progressive=True)
    base_sizes, base_dec = A.standard_jpeg_batch(x, QUALITIES, subsampling=ss)
    assert np.array_equal(dec.cpu().numpy(), base_dec.cpu().numpy())
    del base_dec
    dec = dec.cpu().numpy()
    for j, q in enumerate(QUALITIES):
        got = A.standard_jpeg_many(x, q, subsampling=ss, progressive=True)
        for i in range(x.shape[0]):
            want = _pil(x[i], q, ss)
            assert got[i] == want, f"image {i}, q={q}, {H}x{W}, {ss}: bytes differ"
            assert sizes[i, j] == len(want)
            assert np.array_equal(dec[j, i], T._pil_decode(want)), f"image {i}, q={q}, {H}x{W}, {ss}: pixels differ"


@live
def test_cut_inputs_equal_pillow(A):
    for x, q, ss in cut_inputs():
        want = _pil(x, q, ss)
        assert A.standard_jpeg_many(x, q, subsampling=ss, progressive=True) == [want], (x.shape, q)
        sizes, dec = A.standard_jpeg_batch(x[None], [q], subsampling=ss, progressive=True)
        assert sizes.tolist() == [[len(want)]]
        assert np.array_equal(dec[0, 0].cpu().numpy(), T._pil_decode(want))


@live
def test_mixed_batch_several_qualities(A):
    x = T._images(170, 181, 9)
    qs = (5, 35, 80, 98)
    for ss in LAYOUTS:
        sizes, dec = A.standard_jpeg_batch(x, qs, subsampling=ss, progressive=True)
        for j, q in enumerate(qs):
            files = A.standard_jpeg_many(x, q, subsampling=ss, progressive=True, optimize=True)
            for i in range(x.shape[0]):
                want = _pil(x[i], q, ss)
                assert files[i] == want and sizes[i, j] == len(want), (ss, q, i)
                assert np.array_equal(dec[j, i].cpu().numpy(), T._pil_decode(want)), (ss, q, i)


@pytest.mark.parametrize("ss", LAYOUTS)
def test_matches_cpu_restatement_and_batch_independence(A, ss):
    g = np.random.default_rng(11)
    for H, W in ((20, 20), (9, 41), (33, 5), (16, 3)):
        x = g.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        x[1] = x[1] // 64 * 64                                   # few levels: long zero runs and small tables
        for q in (10, 90):
            files = A.standard_jpeg_many(x, q, subsampling=ss, progressive=True)
            for i in range(2):
                assert files[i] == P.encode(x[i], q, ss)[0], (H, W, q, i)
                assert A.standard_jpeg_many(x[i], q, subsampling=ss, progressive=True) == [files[i]]


@pytest.mark.parametrize("ss", LAYOUTS)
def test_round_trip_through_the_file_decoder(A, ss):
    """two independently written paths: the encoder's reconstruction and the decoder of progressive .jpg files"""
    for H, W in ((37, 53), (64, 4), (255, 257)):
        x = T._images(H, W, 4)
        qs = (10, 75, 100)
        sizes, dec = A.standard_jpeg_batch(x, qs, subsampling=ss, progressive=True)
        for j, q in enumerate(qs):
            files = A.standard_jpeg_many(x, q, subsampling=ss, progressive=True)
            assert [len(f) for f in files] == sizes[:, j].tolist()
            back = A.standard_jpeg_decode_many(files, progressive=True)
            for i in range(x.shape[0]):
                assert np.array_equal(back[i].cpu().numpy(), dec[j, i].cpu().numpy()), (H, W, q, i)


def test_scan_script_of_the_library_file(A):
    from adaptive_edge_aware_jpeg_amd.standard_jpeg import parse_scans
    x = T._images(37, 53, 2)
    for ss in LAYOUTS:
        data = A.standard_jpeg_many(x[0], 75, subsampling=ss, progressive=True)[0]
        frame, scans = parse_scans(data)
        assert (frame.height, frame.width, frame.n_scans, frame.sof) == (37, 53, 10, 0xC2)
        assert [(s.ss, s.se, s.ah, s.al) for s in scans] == [(c[1], c[2], c[3], c[4]) for c in P.SCRIPT]
        assert [[s.comp[k] for k in range(s.ncomp)] for s in scans] == [list(c[0]) for c in P.SCRIPT]
        # marker order: SOI APP0 DQT DQT SOF2, DHT 0x00, DHT 0x01, SOS; then per scan [DHT of its AC table] SOS, none before the DC
        # refinement; EOI
        markers, i = [], 2
        while data[i + 1] != 0xDA:
            markers.append((data[i + 1], data[i + 4]))
            i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
        assert [m for m, _ in markers] == [0xE0, 0xDB, 0xDB, 0xC2, 0xC4, 0xC4] and [b for _, b in markers[4:]] == [0x00, 0x01]
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
        assert scans[-1].data_offset + scans[-1].data_length == len(data) - 2
        for k, s in enumerate(scans[1:], 1):
            sos = s.data_offset - (8 + 2 * s.ncomp)
            assert data[sos:sos + 2] == b"\xff\xda"
            gap = data[scans[k - 1].data_offset + scans[k - 1].data_length:sos]
            if s.ss == 0:
                assert gap == b"", k
            else:
                assert gap[:2] == b"\xff\xc4" and gap[4] == (0x11 if s.comp[0] else 0x10), k
                assert len(gap) == 2 + int.from_bytes(gap[2:4], "big"), k
            want_sel = [0, 0, 0] if s.ss == 0 else [1 if s.comp[0] else 0]
            assert [data[sos + 6 + 2 * c] for c in range(s.ncomp)] == want_sel, k


def _scan(lib, fn, ctx, c, ss, se, ah, al):
    c = np.ascontiguousarray(c, np.int16)
    cap = 64 + c.shape[0] * 8 * (se - ss + 2)
    out, n = (ctypes.c_uint8 * cap)(), ctypes.c_uint64()
    counts, cuts = np.zeros(257, np.int64), np.zeros(2, np.int64)
    args = (c.ctypes.data, c.shape[0], ss, se, ah, al, ctypes.addressof(out), cap, ctypes.addressof(n), counts.ctypes.data, cuts.ctypes.data)
    rc = fn(*((ctx.handle,) + args if ctx is not None else args))
    assert rc == 0, rc
    return bytes(out[:n.value]), counts, tuple(int(v) for v in cuts)


def test_device_testing_entry_equals_host_core(A):
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    ctx = get_context(0)
    lib = ctx.lib
    for name, c, ss, se, ah, al, want_cuts in P.synthetic_cases():
        host = _scan(lib, lib.aej_test_jfif_prog_scan_host, None, c, ss, se, ah, al)
        dev = _scan(lib, lib.aej_test_jfif_prog_scan, ctx, c, ss, se, ah, al)
        assert dev[0] == host[0], name
        assert np.array_equal(dev[1], host[1]), name
        assert dev[2] == host[2], name
        if want_cuts is not None:
            assert dev[2] == want_cuts, name


def test_defaults_untouched(A):
    x = T._images(37, 53, 3)
    for q in (10, 75):
        assert A.standard_jpeg_many(x, q, progressive=False) == A.standard_jpeg_many(x, q)
        assert A.standard_jpeg_many(x, q, optimize=True, progressive=False) == A.standard_jpeg_many(x, q, optimize=True)
        prog = A.standard_jpeg_many(x, q, progressive=True)
        assert all(b"\xff\xc2" in f[:700] and f != g for f, g in zip(prog, A.standard_jpeg_many(x, q)))
    with pytest.raises(TypeError):
        A.standard_jpeg_many(x, 75, progressive=1)


@live
def test_sweep_standard_progressive(A, tmp_path):
    x = T._images(170, 181, 2)[:3]
    xf = x.astype(np.float32) / np.float32(255)
    qs = (10, 50, 90)
    kw = dict(standard_qualities=qs, standard_subsampling="4:2:2", max_bytes=64 << 20)
    plain = A.sweep(xf, ("YCbCr",), [(50, 90)], [(8, 32)], **kw)
    res = A.sweep(xf, ("YCbCr",), [(50, 90)], [(8, 32)], standard_progressive=True, **kw)
    assert plain.standard.progressive is False and res.standard.progressive is True
    for k in ("psnr", "ssim", "ms_ssim"):
        assert np.array_equal(getattr(res.standard, k), getattr(plain.standard, k)), k
        assert np.array_equal(getattr(res, k), getattr(plain, k)), k
    for j, q in enumerate(qs):
        for i in range(x.shape[0]):
            n = len(_pil(x[i], q, "4:2:2"))
            assert res.standard.bytes[i, j] == n
            assert res.standard.compression_ratio[i, j] == 170 * 181 * 3 / n
    assert not np.array_equal(res.standard.bytes, plain.standard.bytes)
    p = tmp_path / "std.csv"
    res.to_csv_standard(p)
    assert p.read_text().splitlines()[0] == "image_name,quality,psnr,ssim,ms_ssim,compression_ratio"
