"""GPU: standard_jpeg_decode_many(..., progressive=True) (csrc/jpegprog.hip) pixel-identical to Pillow's decode of progressive files of
every supported layout, the coefficients after every dependency level against tests/progressive_reference.py, and malformed scans
reported per file.  Every comparison is np.array_equal with Pillow's ``convert("RGB")``."""
import ctypes
import io
import json
import os

import numpy as np
import pytest

import progressive_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FIXTURES = os.path.join(GOLDEN, "jpegprog")
BASELINE = os.path.join(GOLDEN, "jpegdec")
NATURAL = ["baboon", "bikes", "buildings", "house", "jelly_beans", "peppers"]


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _names():
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        return [c["name"] for c in json.load(f)["cases"]]


def _file(name, folder=FIXTURES):
    with open(os.path.join(folder, name + ".jpg"), "rb") as f:
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
    return [t.cpu().numpy() for t in A.standard_jpeg_decode_many(files, progressive=True)]


def test_fixtures_in_one_call(A):
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    names = _names()
    got = _decode(A, [_file(n) for n in names])
    for n, g in zip(names, got):
        assert np.array_equal(g, px[n]), n
        assert np.array_equal(g, _pil_decode(_file(n))), n


def test_fixtures_one_by_one_and_views(A):
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    names = _names()
    for n in names:
        (g,) = A.standard_jpeg_decode_many([_file(n)], progressive=True)
        assert g.dtype == A.standard_jpeg.get_context(0).torch.uint8 and np.array_equal(g.cpu().numpy(), px[n]), n
    outs = A.standard_jpeg_decode_many([_file(n) for n in names[:5]], progressive=True)
    base = outs[0].data_ptr()
    for o, n in zip(outs, names[:5]):                           # views of one packed allocation, in input order
        assert o.data_ptr() == base and o.is_contiguous() and tuple(o.shape) == px[n].shape
        base += o.numel()


def test_live_mixed_call_equals_pillow(A):
    rng = np.random.default_rng(23)
    files = []
    for k in range(36):
        H, W = (1, 1) if k == 0 else (int(rng.integers(1, 300)), int(rng.integers(1, 300)))
        x = _fit(_png("natural/" + NATURAL[k % len(NATURAL)]), H, W)
        opts = dict(quality=int(rng.integers(1, 101)), progressive=k % 3 != 0)
        layout = k % 4
        if layout == 3:
            opts["grey"] = True
        else:
            opts["subsampling"] = layout
        if k % 5 == 1:
            opts["restart_marker_blocks"] = int(rng.integers(1, 9))
        if k % 5 == 3:
            opts["restart_marker_rows"] = 1
        files.append(_pil(x, **opts))
    assert any(b"\xff\xc2" in f[:800] for f in files) and any(b"\xff\xc0" in f[:800] for f in files)
    got = _decode(A, files)
    for k, (f, g) in enumerate(zip(files, got)):
        assert np.array_equal(g, _pil_decode(f)), k


def test_full_size(A):
    nat = _fit(_png("natural/bikes"), 2160, 3840)
    flat = np.full((2160, 3840, 3), (70, 130, 190), np.uint8)
    files = [_pil(nat, quality=75, subsampling=2, progressive=True),
             _pil(nat, quality=95, subsampling=0, progressive=True),
             _pil(nat, quality=75, subsampling=2, progressive=True, restart_marker_rows=1),
             _pil(nat, quality=95, subsampling=0, progressive=True, restart_marker_rows=1),
             _pil(flat, quality=75, subsampling=2, progressive=True),                    # EOB runs of 32767 blocks, chained
             _pil(_fit(_png("natural/buildings"), 2157, 3839), quality=75, subsampling=2, progressive=True)]
    got = _decode(A, files)
    for k, (f, g) in enumerate(zip(files, got)):
        assert np.array_equal(g, _pil_decode(f)), k


def _device_coefficients(A, data, n_levels):
    from adaptive_edge_aware_jpeg_amd import _lib
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    ctx = _lib.get_context(0)
    t, lib = ctx.torch, ctx.lib
    frame, scans = SJ.parse_scans(data)
    arr = (_lib.JpegProgScan * len(scans))(*scans)
    dev, off = SJ._stage(ctx, [memoryview(data)], [(0, s.data_offset, s.data_length) for s in scans])
    nb = frame.mcux * frame.mcuy * frame.blocks_per_mcu
    coef = ctx.empty((nb, 64), t.int16)
    status = ctx.empty((1,), t.int32)
    nws = int(lib.aej_jpegprog_workspace_bytes(ctx.handle, ctypes.addressof(frame), ctypes.addressof(arr), 1))
    ws = ctx.workspace(nws)
    ctx.check(lib.aej_test_jpegprog_coefs(ctx.handle, ctypes.addressof(frame), ctypes.addressof(arr), 1, dev.data_ptr(),
                                          ctypes.c_uint64(dev.numel()), off.ctypes.data, n_levels, coef.data_ptr(), ctypes.c_uint64(nb),
                                          status.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws)))
    assert int(status.cpu()[0]) == 0
    return coef.cpu().numpy(), scans, frame


@pytest.mark.parametrize("name", ["bikes_53x37_420_rst3_q50", "noise_64x64_444_q100", "house_33x17_422_q50", "grey_33x47_rst3_q40"])
def test_coefficients_after_each_level(A, name):
    data = _file(name)
    frame, _ = A.standard_jpeg.parse_scans(data)
    assert frame.n_levels == 3
    for lv in range(1, frame.n_levels + 1):
        got, scans, _ = _device_coefficients(A, data, lv)
        ref = R.mcu_order(data, R.coefficients(data, only={i for i, s in enumerate(scans) if s.level < lv}))
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f"level {lv}: {len(bad)} coefficients differ, first (block, index) {bad[0]}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


def test_twins_hold_the_same_coefficients(A):
    x = _fit(_png("natural/peppers"), 150, 203)
    for opts in (dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(grey=True)):
        base, prog = _pil(x, quality=80, **opts), _pil(x, quality=80, progressive=True, **opts)
        gb, gp = _decode(A, [base, prog])
        assert np.array_equal(gb, gp) and np.array_equal(gp, _pil_decode(prog)) and np.array_equal(gb, _pil_decode(base)), opts


def _scan_ranges(A, data):
    _, scans = A.standard_jpeg.parse_scans(data)
    return [(s.data_offset, s.data_offset + s.data_length, (s.ss, s.ah)) for s in scans]


def test_corrupt_scans_raise_per_file(A):
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    good, other = _file("buildings_50x66_rst3_q70"), _file("house_45x61_grey_q60")
    ranges = _scan_ranges(A, good)
    bads = []
    for k in (0, 1, 4, 5, 6, 9):                                # a scan of every kind cut at a third and at two thirds
        a, b, _ = ranges[k]
        for cut in ((b - a) // 3, 2 * (b - a) // 3):
            bads.append(good[:a + cut] + good[b:])
    a, b, _ = ranges[4]
    i = good.index(b"\xff\xd0", a, b)
    bads.append(good[:i] + good[i + 2:])                        # a dropped restart marker
    bads.append(good[:i] + b"\xff\xd3" + good[i + 2:])          # ... and one out of sequence
    for k, bad in enumerate(bads):
        with pytest.raises(ValueError, match="file 1"):
            A.standard_jpeg_decode_many([good, bad, other], progressive=True)
        got = _decode(A, [good, other])
        assert np.array_equal(got[0], px["buildings_50x66_rst3_q70"]) and np.array_equal(got[1], px["house_45x61_grey_q60"]), k


def test_bit_flips_raise_or_keep_the_shape(A):
    """Flips inside each kind of scan that leave the marker structure alone (no 0xFF made, unmade or followed): the host parser accepts
    the file, so whatever happens is the device decoders' bounded loops at work."""
    rng = np.random.default_rng(5)
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    names = ["lena_64x64_420_q75", "jelly_40x70_rstrow_422_q80", "house_45x61_grey_q60", "peppers_40x56_444_q90", "noise_37x53_420_q100"]
    for trial in range(60):
        name = names[trial % len(names)]
        data = bytearray(_file(name))
        ranges = _scan_ranges(A, bytes(data))
        a, b, _ = ranges[trial % len(ranges)]
        for _ in range(1 + trial % 3):
            for _ in range(100):
                pos, bit = int(rng.integers(a, b)), 1 << int(rng.integers(0, 8))
                if data[pos] != 0xFF and data[pos] ^ bit != 0xFF and data[pos - 1] != 0xFF:
                    data[pos] ^= bit
                    break
        frame, _ = A.standard_jpeg.parse_scans(bytes(data))
        try:
            g, h = A.standard_jpeg_decode_many([bytes(data), _file(names[0])], progressive=True)
        except ValueError as e:
            assert "file 0" in str(e)
            continue
        assert tuple(g.shape) == (frame.height, frame.width, 3)
        assert np.array_equal(h.cpu().numpy(), px[names[0]])


def test_default_call_still_refuses(A):
    with pytest.raises(NotImplementedError, match="file 1"):
        A.standard_jpeg_decode_many([_file("lena_64x64_420_q75", BASELINE), _file("lena_64x64_420_q75")])


def test_sweep_runs_on_decoded_files(A):
    names = ["lena_64x64_420_q75", "peppers_40x56_444_q90", "house_45x61_grey_q60"]
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    from adaptive_edge_aware_jpeg_amd.sweep import PSNR, SSIM
    got = A.sweep(A.standard_jpeg_decode_many([_file(n) for n in names], progressive=True), metrics=PSNR | SSIM)
    ref = A.sweep([px[n] for n in names], metrics=PSNR | SSIM)
    assert len(got.rows()) == len(names) == len(ref.rows())
    for a, b in zip(got.rows(), ref.rows()):
        assert a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a), (a, b)
