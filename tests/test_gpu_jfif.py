"""GPU: standard JPEG (csrc/jfif.hip) byte-identical to Pillow's files and pixel-identical to Pillow's decode of them."""
import io
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
QUALITIES = (1, 10, 25, 50, 75, 90, 95, 100)
SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 53), (255, 257), (768, 512), (634, 505), (1080, 1920), (2160, 3840)]
NATURAL = ["baboon", "bikes", "buildings", "house", "jelly_beans", "peppers"]
FIXTURES = os.path.join(GOLDEN, "jfif")


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


def _png(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, name + ".png")).convert("RGB"))


def _fit(img, H, W):
    """img tiled (mirrored) to cover H x W, cropped"""
    reps = (-(-H // img.shape[0]), -(-W // img.shape[1]))
    t = np.concatenate([np.concatenate([img if (j % 2 == 0) else img[:, ::-1] for j in range(reps[1])], 1) if i % 2 == 0 else
                        np.concatenate([img[::-1] if (j % 2 == 0) else img[::-1, ::-1] for j in range(reps[1])], 1) for i in range(reps[0])], 0)
    return np.ascontiguousarray(t[:H, :W])


def _images(H, W, seed):
    """[5, H, W, 3] uint8: lena, a natural image, uniform noise, a flat colour, saturated primaries"""
    g = np.random.default_rng(seed)
    prim = np.zeros((H, W, 3), np.uint8)
    band = np.arange(W) * 3 // max(W, 1)
    for c in range(3):
        prim[:, :, c] = np.where(band == c, 255, 0)
    prim[H // 2:] = 255 - prim[H // 2:]
    return np.stack([_fit(_png("lena"), H, W), _fit(_png("natural/" + NATURAL[seed % len(NATURAL)]), H, W),
                     g.integers(0, 256, (H, W, 3), dtype=np.uint8), np.full((H, W, 3), (201, 17, 90), np.uint8), prim])


def _pil(x, q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, "JPEG", quality=q)
    return buf.getvalue()


def _pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_fixtures_bytes_and_pixels(A):
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        meta = json.load(f)
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    for case in meta["cases"]:
        name, q = case["name"], case["quality"]
        src = px[name + "_src"]
        with open(os.path.join(FIXTURES, name + ".jpg"), "rb") as f:
            want = f.read()
        assert A.standard_jpeg_many(src, q) == [want], name
        sizes, dec = A.standard_jpeg_batch(src[None], [q])
        assert sizes.tolist() == [[len(want)]], name
        assert np.array_equal(dec[0, 0].cpu().numpy(), px[name + "_dec"]), name
        # the float32 path: Image.load's u8 / 255 maps back to the same levels
        assert A.standard_jpeg_many(src.astype(np.float32) / np.float32(255), q) == [want], name


@live
@pytest.mark.parametrize("H,W", SIZES)
def test_bytes_and_decode_equal_pillow(A, H, W):
    x = _images(H, W, H * 7 + W)
    sizes, dec = A.standard_jpeg_batch(x, QUALITIES)
    dec = dec.cpu().numpy()
    for j, q in enumerate(QUALITIES):
        got = A.standard_jpeg_many(x, q)
        for i in range(x.shape[0]):
            want = _pil(x[i], q)
            assert got[i] == want, f"image {i}, q={q}, {H}x{W}: bytes differ"
            assert sizes[i, j] == len(want)
            assert np.array_equal(dec[j, i], _pil_decode(want)), f"image {i}, q={q}, {H}x{W}: pixels differ"


@live
def test_narrow_images_decode_equal_pillow(A):
    g = np.random.default_rng(5)
    for W in (1, 2, 3, 4, 5):
        for H in (1, 2, 7, 9, 10, 16, 17, 33, 64):
            x = np.stack([g.integers(0, 256, (H, W, 3), dtype=np.uint8), _fit(_png("lena"), H, W)])
            sizes, dec = A.standard_jpeg_batch(x, (10, 75, 100))
            dec = dec.cpu().numpy()
            for j, q in enumerate((10, 75, 100)):
                for i in range(2):
                    want = _pil(x[i], q)
                    assert sizes[i, j] == len(want), (H, W, q)
                    assert np.array_equal(dec[j, i], _pil_decode(want)), (H, W, q, i)


def test_matches_cpu_restatement(A):
    g = np.random.default_rng(11)
    for H, W in ((20, 20), (9, 41), (33, 5)):
        x = g.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        sizes, dec = A.standard_jpeg_batch(x, (10, 90))
        for j, q in enumerate((10, 90)):
            files = A.standard_jpeg_many(x, q)
            for i in range(2):
                assert files[i] == R.encode(x[i], q)
                assert np.array_equal(dec[j, i].cpu().numpy(), R.decode(x[i], q))


def test_batch_independence(A):
    x = _images(37, 53, 3)
    alone = [A.standard_jpeg_many(x[i], 50)[0] for i in range(x.shape[0])]
    assert A.standard_jpeg_many(x, 50) == alone
    assert A.standard_jpeg_many(x[::-1].copy(), 50) == alone[::-1]
    s1, d1 = A.standard_jpeg_batch(x[1:2], (25, 90))
    s5, d5 = A.standard_jpeg_batch(x, (90, 25))
    assert s1[0].tolist() == s5[1][::-1].tolist()
    assert np.array_equal(d1[0, 0].cpu().numpy(), d5[1, 1].cpu().numpy())


def test_torch_input_and_errors(A):
    import torch
    x = _images(16, 16, 1)
    want = A.standard_jpeg_many(x, 75)
    assert A.standard_jpeg_many(torch.from_numpy(x).cuda(), 75) == want
    assert A.standard_jpeg_many(torch.from_numpy(x.astype(np.float32) / np.float32(255)).cuda(), 75) == want
    for q in (0, 101, 50.5):
        with pytest.raises(ValueError):
            A.standard_jpeg_many(x, q)
    with pytest.raises(ValueError):
        A.standard_jpeg_batch(x, [])
    with pytest.raises(ValueError):
        A.standard_jpeg_many(x.astype(np.float32) * 2, 75)
    with pytest.raises(TypeError):
        A.standard_jpeg_many(x.astype(np.int32), 75)


@live
def test_sweep_standard_equals_pillow_and_metrics(A, tmp_path):
    from adaptive_edge_aware_jpeg_amd.evaluation_metrics import PSNR, SSIM, MS_SSIM
    x = _images(170, 181, 2)[:3]
    xf = x.astype(np.float32) / np.float32(255)
    qs = (10, 25, 50, 75, 90)
    base = A.sweep(xf, ("YCbCr",), [(50, 90)], [(8, 32)])
    res = A.sweep(xf, ("YCbCr",), [(50, 90)], [(8, 32)], standard_qualities=qs, max_bytes=64 << 20)
    assert np.array_equal(res.psnr, base.psnr) and np.array_equal(res.bytes, base.bytes)
    st = res.standard
    for j, q in enumerate(qs):
        files = [_pil(x[i], q) for i in range(x.shape[0])]
        dec = np.stack([_pil_decode(f) for f in files]).astype(np.float32) / np.float32(255)
        m = A.EvaluationMetrics.batch(xf, dec, PSNR | SSIM | MS_SSIM).cpu().numpy()
        for i in range(x.shape[0]):
            assert st.bytes[i, j] == len(files[i])
            assert st.compression_ratio[i, j] == 170 * 181 * 3 / len(files[i])
            assert (st.psnr[i, j], st.ssim[i, j], st.ms_ssim[i, j]) == tuple(m[i])
    p = tmp_path / "std.csv"
    res.to_csv_standard(p)
    lines = p.read_text().splitlines()
    assert lines[0] == "image_name,quality,psnr,ssim,ms_ssim,compression_ratio"
    assert len(lines) == 1 + 3 * len(qs)
    assert lines[1].startswith("image_0,10,")


# ---- the pieces every stream writer shares (csrc/jfif_stream_core.h): noise through every coder ----------------------------------------
# 152 x 168 at 4:4:4 is 19 x 21 x 3 = 1197 blocks per file: more than one 1024-value tile of the prefix-sum kernel and no multiple of
# 64; noise at quality 95 puts 0xFF bytes across 64-byte chunk and 32-bit word boundaries, quality 30 gives short streams.
SHARED_KINDS = ({}, {"optimize": True}, {"progressive": True})
_shared_cache = {}


def _shared_noise():
    return np.random.default_rng(20261018).integers(0, 256, (2, 152, 168, 3), np.uint8)


def _shared_pillow(q, ss, grey):
    """Pillow's files of the two noise images (grey: of their channel 0) per kind, made once per case"""
    from PIL import Image
    key = (q, ss, grey)
    if key not in _shared_cache:
        files = []
        for kw in SHARED_KINDS:
            row = []
            for x in _shared_noise():
                buf = io.BytesIO()
                if grey:
                    Image.fromarray(np.ascontiguousarray(x[:, :, 0])).save(buf, "JPEG", quality=q, **kw)
                else:
                    Image.fromarray(x).save(buf, "JPEG", quality=q, subsampling=ss, **kw)
                assert buf.getvalue().count(b"\xff\x00") >= 5, (q, ss, grey, kw)      # the case cannot pass by never stuffing
                row.append(buf.getvalue())
            files.append(row)
        _shared_cache[key] = files
    return _shared_cache[key]


@live
@pytest.mark.parametrize("ss", ("4:4:4", "4:2:2", "4:2:0"))
@pytest.mark.parametrize("q", (95, 30))
def test_shared_stream_pieces_colour_equal_pillow(A, q, ss):
    x = _shared_noise()
    want = _shared_pillow(q, ss, False)
    for kw, files in zip(SHARED_KINDS, want):
        assert A.standard_jpeg_many(x, q, subsampling=ss, **kw) == files, (q, ss, kw)
        sizes, dec = A.standard_jpeg_batch(x, [q], subsampling=ss, **kw)
        assert sizes[:, 0].tolist() == [len(f) for f in files], (q, ss, kw)
        for i, f in enumerate(files):
            assert np.array_equal(dec[0, i].cpu().numpy(), _pil_decode(f)), (q, ss, kw, i)
    assert A.standard_jpeg_transcode_many(want[0], progressive=False, grey=True) == want[1], (q, ss)
    assert A.standard_jpeg_transcode_many(want[0], progressive=True, grey=True) == want[2], (q, ss)


@live
@pytest.mark.parametrize("q", (95, 30))
def test_shared_stream_pieces_grey_equal_pillow(A, q):
    g = [np.ascontiguousarray(x[:, :, 0]) for x in _shared_noise()]
    want = _shared_pillow(q, None, True)
    for kw, files in zip(SHARED_KINDS, want):
        assert A.standard_jpeg_encode_many(g, q, mode="L", **kw) == files, (q, kw)
        dec = A.standard_jpeg_decode_many(files, progressive=bool(kw.get("progressive")))
        for i, f in enumerate(files):
            assert np.array_equal(dec[i].cpu().numpy(), _pil_decode(f)), (q, kw, i)
    assert A.standard_jpeg_transcode_many(want[0], progressive=False, grey=True) == want[1], q
    assert A.standard_jpeg_transcode_many(want[0], progressive=True, grey=True) == want[2], q
