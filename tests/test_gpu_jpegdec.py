"""GPU: standard_jpeg_decode_many (csrc/jpegdec.hip) pixel-identical to Pillow's decode of baseline files of every supported layout,
the self-synchronising Huffman decode at its smallest subsequence length, and malformed scans reported per file."""
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FIXTURES = os.path.join(GOLDEN, "jpegdec")
NATURAL = ["baboon", "bikes", "buildings", "house", "jelly_beans", "peppers"]
JFIF_SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 53), (255, 257), (768, 512), (634, 505), (1080, 1920), (2160, 3840)]


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _meta():
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        return json.load(f)


def _live_matches_fixtures():
    from PIL import features
    return features.version("libjpeg_turbo") == _meta()["libjpeg_turbo"]


live = pytest.mark.skipif(not _live_matches_fixtures(), reason="this Pillow's libjpeg-turbo is not the one the fixtures pin")


def _file(name):
    with open(os.path.join(FIXTURES, name + ".jpg"), "rb") as f:
        return f.read()


def _png(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, name + ".png")).convert("RGB"))


def _fit(img, H, W):
    reps = (-(-H // img.shape[0]), -(-W // img.shape[1]))
    t = np.concatenate([np.concatenate([img if (j % 2 == 0) else img[:, ::-1] for j in range(reps[1])], 1) if i % 2 == 0 else
                        np.concatenate([img[::-1] if (j % 2 == 0) else img[::-1, ::-1] for j in range(reps[1])], 1) for i in range(reps[0])], 0)
    return np.ascontiguousarray(t[:H, :W])


def _pil(x, **opts):
    from PIL import Image
    img = Image.fromarray(x)
    if opts.pop("grey", False):
        img = img.convert("L")
    buf = io.BytesIO()
    img.save(buf, "JPEG", **opts)
    return buf.getvalue()


def _pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _decode(A, files):
    return [t.cpu().numpy() for t in A.standard_jpeg_decode_many(files)]


def _set_s(bits):
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    get_context(0).set_option("jpegdec_subseq_bits", bits)


def test_fixtures(A):
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    names = [c["name"] for c in _meta()["cases"]]
    got = _decode(A, [_file(n) for n in names])
    for n, g in zip(names, got):
        assert g.dtype == np.uint8 and np.array_equal(g, px[n]), n


def test_fixtures_one_by_one_and_views(A):
    import torch
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    names = [c["name"] for c in _meta()["cases"]]
    for n in names:
        (t,) = A.standard_jpeg_decode_many([_file(n)])
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
        assert np.array_equal(t.cpu().numpy(), px[n]), n
    ts = A.standard_jpeg_decode_many([bytearray(_file(n)) for n in names[:3]])
    assert len({t.untyped_storage().data_ptr() for t in ts}) == 1          # views into one packed allocation


OPTIONS = [dict(subsampling=2), dict(subsampling=1), dict(subsampling=0), dict(grey=True), dict(optimize=True),
           dict(restart_marker_blocks=3), dict(restart_marker_rows=1), dict(subsampling=1, restart_marker_rows=1),
           dict(subsampling=0, optimize=True, restart_marker_blocks=5), dict(grey=True, restart_marker_rows=1)]
QUALITIES = (1, 10, 50, 75, 95, 100)


@live
def test_live_mixed_call_equals_pillow(A):
    rng = np.random.default_rng(11)
    files = []
    ragged = [(1, 1), (3, 2), (9, 4), (17, 33), (37, 53), (64, 48), (121, 77), (255, 257)]
    for i, opts in enumerate(OPTIONS):
        for j, q in enumerate(QUALITIES):
            H, W = ragged[(i + j) % len(ragged)]
            y, x = rng.integers(0, 200, 2)
            src = _fit(_png("natural/" + NATURAL[(i + j) % len(NATURAL)])[y:, x:], H, W)
            files.append(_pil(src, quality=q, **opts))
    big = [((1080, 1920), dict(quality=75)), ((1080, 1920), dict(quality=95, subsampling=1, restart_marker_rows=1)),
           ((2160, 3840), dict(quality=75)), ((2160, 3840), dict(quality=50, subsampling=0, optimize=True)),
           ((2160, 3840), dict(quality=90, restart_marker_rows=1)), ((1080, 1920), dict(quality=30, grey=True))]
    for k, ((H, W), opts) in enumerate(big):
        files.append(_pil(_fit(_png("natural/" + NATURAL[k % len(NATURAL)]), H, W), **opts))
    order = rng.permutation(len(files))
    files = [files[i] for i in order]
    got = _decode(A, files)
    assert len(got) == len(files)
    for i, (f, g) in enumerate(zip(files, got)):
        ref = _pil_decode(f)
        assert g.shape == ref.shape and np.array_equal(g, ref), f"file {i} (case {order[i]})"


def test_round_trip_of_own_encoder(A):
    for k, (H, W) in enumerate(JFIF_SIZES):
        x = _fit(_png("natural/" + NATURAL[k % len(NATURAL)]), H, W)
        for q in (10, 75):
            files = A.standard_jpeg_many(x[None], q)
            (got,) = A.standard_jpeg_decode_many(files)
            ref = A.standard_jpeg_batch(x[None], [q])[1][0, 0]
            assert np.array_equal(got.cpu().numpy(), ref.cpu().numpy()), (H, W, q)


def test_smallest_subsequence_runs_the_sync(A):
    x = _fit(_png("natural/bikes"), 200, 264)
    files = [_pil(x, quality=75), _pil(x, quality=95, subsampling=0), _pil(x, quality=40, grey=True), _file("lena_64x64_420_q75"),
             _pil(x, quality=80, restart_marker_rows=1)]
    try:
        _set_s(32)
        small = _decode(A, files)
        rounds = A.standard_jpeg.decode_sync_rounds()
    finally:
        _set_s(2048)
    default = _decode(A, files)
    assert rounds > 1, rounds
    for s, d, f in zip(small, default, files):
        assert np.array_equal(s, d) and np.array_equal(d, _pil_decode(f))


def _scan_bounds(A, data):
    d = A.standard_jpeg.parse_header(data)
    return d.scan_offset, len(data) - 2                     # the scan, EOI excluded


def test_corrupt_files_raise_per_file(A):
    good = _file("buildings_50x66_rst3_q70")
    s0, s1 = _scan_bounds(A, good)
    truncated = good[:s0 + (s1 - s0) // 2] + b"\xff\xd9"
    i = good.index(b"\xff\xd0", s0)
    wrong_rst = good[:i] + b"\xff\xd3" + good[i + 2:]
    extra_rst = good[:s1] + b"\xff\xd7" + good[s1:]            # one restart marker more than the segments
    p = good.index(b"\xff\xc4")
    oversub = good[:p + 5] + bytes([3]) + good[p + 6:]
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    for k, bad in enumerate([truncated, wrong_rst, extra_rst, oversub]):
        with pytest.raises(ValueError, match="file 1"):
            A.standard_jpeg_decode_many([good, bad, _file("house_45x61_grey_q60")])
        # the good files of that call decode on their own
        got = _decode(A, [good, _file("house_45x61_grey_q60")])
        assert np.array_equal(got[0], px["buildings_50x66_rst3_q70"]) and np.array_equal(got[1], px["house_45x61_grey_q60"])
    no_rst = _file("lena_64x64_420_q75")
    t0, t1 = _scan_bounds(A, no_rst)
    with pytest.raises(ValueError, match="file 0"):
        A.standard_jpeg_decode_many([no_rst[:t0 + (t1 - t0) // 3] + b"\xff\xd9"])
    with pytest.raises(ValueError, match="file 0"):
        A.standard_jpeg_decode_many([no_rst[:t0 + 5]])


def test_bit_flips_raise_or_keep_the_shape(A):
    rng = np.random.default_rng(5)
    names = ["lena_64x64_420_q75", "jelly_40x70_rstrow_422_q80", "house_45x61_grey_q60", "peppers_40x56_444_q90"]
    for trial in range(40):
        name = names[trial % len(names)]
        data = bytearray(_file(name))
        s0, s1 = _scan_bounds(A, bytes(data))
        for _ in range(1 + trial % 4):
            pos = int(rng.integers(s0, s1))
            data[pos] ^= 1 << int(rng.integers(0, 8))
        d = A.standard_jpeg.parse_header(bytes(data))
        try:
            (g,) = A.standard_jpeg_decode_many([bytes(data)])
        except ValueError as e:
            assert "file 0" in str(e)
            continue
        assert tuple(g.shape) == (d.height, d.width, 3)


def test_empty_list_raises(A):
    with pytest.raises(ValueError):
        A.standard_jpeg_decode_many([])


def test_sweep_runs_on_decoded_files(A):
    names = ["lena_64x64_420_q75", "peppers_40x56_444_q90", "house_45x61_grey_q60"]
    files = [_file(n) for n in names]
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    from adaptive_edge_aware_jpeg_amd.sweep import PSNR, SSIM
    got = A.sweep(A.standard_jpeg_decode_many(files), metrics=PSNR | SSIM)
    ref = A.sweep([px[n] for n in names], metrics=PSNR | SSIM)
    assert len(got.rows()) == len(names) == len(ref.rows())
    for a, b in zip(got.rows(), ref.rows()):                # ms_ssim was not asked for: NaN in both
        assert a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a), (a, b)
