"""GPU: standard_jpeg_decode_many(..., adobe=True) -- four-component (CMYK, YCCK) and RGB-coded files, baseline and progressive, and the C
entries behind it (aej_jpegdec_batch_adobe, aej_jpegprog_batch_adobe; csrc/jpegdec.hip k_jd_init4 / k_jd_sync4 / k_jd_write4, k_jd_idct4,
k_jd_adobe; csrc/jpegprog.hip k_jp_level4).  The reference is Pillow's own decode: as the fixtures tests/golden/jpeg_adobe record it,
always, and live where the libjpeg-turbo at hand is the one that made the fixtures.  Every comparison is exact."""
import ctypes
import json
import os

import numpy as np
import pytest

import jpeg_adobe_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
HERE = os.path.join(GOLDEN, "jpeg_adobe")


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "meta.json")) as f:
        return json.load(f), dict(np.load(os.path.join(HERE, "pixels.npz")))


@pytest.fixture(scope="module")
def live(golden):
    """live Pillow is asked only where its libjpeg-turbo is the one that made the fixtures; the fixtures are compared always"""
    from PIL import features
    return features.version("libjpeg_turbo") == golden[0]["libjpeg_turbo"]


def _file(name):
    with open(os.path.join(HERE, name + ".jpg"), "rb") as f:
        return f.read()


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), what


def _check(A, px, names, **kw):
    files = [_file(n) for n in names]
    for mode in ("auto", "RGB"):
        for n, g in zip(names, _np(A.standard_jpeg_decode_many(files, progressive=True, adobe=True, mode=mode, **kw))):
            _same(g, px[f"{n}/{mode}"], (n, mode))


# ---- 1. kinds x layouts x baseline / progressive, 83 x 61 -----------------------------------------------------------------------------------
def test_the_keyword_is_needed(A, golden):
    for n in ("cmyk_2x2", "rgb_1x1"):
        with pytest.raises(NotImplementedError, match="file 0"):
            A.standard_jpeg_decode_many([_file(n)])


def test_fixtures_every_kind_and_layout(A, golden):
    """every case of the fixtures in one call per mode, the 10-block Photoshop layout and the file without APP14 among them"""
    meta, px = golden
    names = [c["name"] for c in meta["cases"]]
    assert {"cmyk_2x2k", "plain_2x2", "cmyk_2x2_prog", "rgb_2x2_prog", "cmyk_2x2k_prog", "ycck_2x1k_prog"} <= set(names)
    _check(A, px, [names[(5 * i) % len(names)] for i in range(len(names))])


@pytest.mark.parametrize("name", ["cmyk_1x1", "cmyk_2x2", "ycck_2x1_prog", "cmyk_2x2k", "ycck_2x1k", "rgb_2x1", "rgb_1x1_prog", "plain_2x2",
                                  "cmyk_2x2k_prog", "ycck_2x1k_prog", "plain_2x2k_prog"])
def test_fixtures_one_file_per_call(A, golden, name):
    _check(A, golden[1], [name])


def test_live_pillow(A, golden, live):
    """files made now, against Pillow now: every kind x layout x baseline / progressive, other pictures than the fixtures'"""
    if not live:
        pytest.skip("another libjpeg-turbo than the fixtures': they are the reference")
    cases = [(k, l, p) for k in R.KINDS for l in R.LAYOUTS for p in (False, True)] + \
        [(k, l, p) for k in ("cmyk", "ycck", "plain") for l in R.LAYOUTS_K for p in (False, True)]
    files = [R.make_file(k, l, 83, 61, p, seed=17 + i) for i, (k, l, p) in enumerate(cases)]
    want = [R.pillow_pixels(f) for f in files]
    for j, mode in enumerate(("auto", "RGB")):
        for c, g, w in zip(cases, _np(A.standard_jpeg_decode_many(files, progressive=True, adobe=True, mode=mode)), want):
            _same(g, w[j], (c, mode))


# ---- 2. narrow planes: replication at most 2 samples wide, the fancy filters from 3 on, the K plane included -----------------------------
def test_narrow_planes(A, golden):
    meta, px = golden
    names = [c["name"] for c in meta["narrow"]]
    assert len(names) == 28 and {tuple(c["size"]) for c in meta["narrow"]} >= {(1, 20), (2, 20), (3, 20), (4, 20), (5, 20), (1, 1), (17, 33)}
    _check(A, px, names)


# ---- 3. restart intervals, and one segment over many subsequences ------------------------------------------------------------------------------
def test_restart_intervals(A, golden):
    meta, px = golden
    _check(A, px, meta["restart"])


def test_noise_spans_many_subsequences(A, golden):
    """96 x 80 quality-100 noise, 2 x 2 with K sub-sampled: an MCU of 7 blocks, one restart segment.  The synchronising decoder cuts the
    scan every "jpegdec_subseq_bits" bits; here that is over 70 subsequences, each entered with a fourth DC predictor to carry and a
    block slot up to 6 -- and in the 10-block file of the next call up to 9, which three bits do not hold."""
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    meta, px = golden
    data = _file(meta["noise"])
    d = A.standard_jpeg.parse_header(data, adobe=True)
    S = get_context(0).get_option("jpegdec_subseq_bits")
    assert (d.scan_length - 2) * 8 // S >= 70 and d.n_segments == 1 and d.blocks_per_mcu == 7
    _check(A, px, [meta["noise"]])
    rounds, n_sub = A.standard_jpeg.decode_sync_rounds(), (d.scan_length - 2) * 8 // S
    print(f"{n_sub} subsequences, {rounds} sync rounds")
    # Pillow gives all four components one DC and one AC table, so the bits never correct a wrong block slot: a decoder that waited for
    # the slot to arrive from the predecessor would need n_sub - 1 rounds.  It is taken from the block counts instead, and what is left
    # is the synchronisation of position and zigzag index -- slow in this file, whose blocks are a third of a subsequence long.
    assert 1 <= rounds <= n_sub * 2 // 3
    get_context(0).set_option("jpegdec_subseq_bits", 256)      # the 83 x 61 Photoshop files: a dozen subsequences each at 256 bits
    try:
        _check(A, px, ["cmyk_2x2k", "ycck_2x1k", "plain_2x1k"])
    finally:
        get_context(0).set_option("jpegdec_subseq_bits", S)


# ---- 4. one mixed call ----------------------------------------------------------------------------------------------------------------------------
def test_one_mixed_call(A, golden):
    meta, px = golden
    with open(os.path.join(GOLDEN, "jpeg_luma", "meta.json")) as f:
        old = [c["name"] for c in json.load(f)["cases"]]
    grey = next(n for n in old if "grey" in n and "prog" not in n)
    c420 = next(n for n in old if "420" in n and "prog" not in n)
    def old_file(n):
        with open(os.path.join(GOLDEN, n + ".jpg"), "rb") as f:
            return f.read()
    files = [old_file(grey), old_file(c420), _file("cmyk_2x2"), _file("ycck_1x1"), _file("rgb_1x1"), _file("cmyk_2x2_prog")]
    modes = ["L", "RGB", "auto", "RGB", "auto", "auto"]
    ts = A.standard_jpeg_decode_many(files, progressive=True, adobe=True, mode=modes)
    assert [tuple(t.shape[2:]) for t in ts] == [(), (3,), (4,), (3,), (3,), (4,)]
    assert len({t.untyped_storage().data_ptr() for t in ts}) == 1 and ts[0].untyped_storage().nbytes() == sum(t.numel() for t in ts)
    pos = ts[0].data_ptr()
    for t in ts:                                     # contiguous, in input order
        assert t.data_ptr() == pos and t.is_contiguous()
        pos += t.numel()
    for f, m, g in zip(files, modes, _np(ts)):
        (own,) = _np(A.standard_jpeg_decode_many([f], progressive=True, adobe=True, mode=m))
        _same(g, own, m)
    _same(_np(ts)[2], px["cmyk_2x2/auto"], "cmyk_2x2")
    _same(_np(ts)[3], px["ycck_1x1/RGB"], "ycck_1x1")
    # the two old files are what the call without the keyword gives
    plain = _np(A.standard_jpeg_decode_many(files[:2], mode=modes[:2]))
    _same(_np(ts)[0], plain[0], "grey")
    _same(_np(ts)[1], plain[1], "4:2:0")


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cmyk_2x2", "cmyk_2x2k", "cmyk_2x2_prog", "cmyk_2x2k_prog"])
def test_a_cut_file_names_itself(A, golden, name):
    """a file cut at 70 % of its scan -- of a progressive file its LAST scan, so that the script the parser sees stays complete and the
    error is the device's: the status word of k_jd_write4 / k_jp_level4, raised as ValueError naming the file"""
    data = _file(name)
    if name.endswith("prog"):
        last = A.standard_jpeg.parse_scans(data, adobe=True)[1][-1]
        cut = data[:last.data_offset + last.data_length * 7 // 10] + b"\xff\xd9"
        assert len(A.standard_jpeg.parse_scans(cut, adobe=True)[1]) == len(A.standard_jpeg.parse_scans(data, adobe=True)[1])
    else:
        d = A.standard_jpeg.parse_header(data, adobe=True)
        cut = data[:d.scan_offset + (len(data) - d.scan_offset) * 7 // 10]
    good = _file("ycck_2x2")
    with pytest.raises(ValueError, match="file 1: "):
        A.standard_jpeg_decode_many([good, cut], progressive=True, adobe=True, mode="auto")
    (g,) = _np(A.standard_jpeg_decode_many([good], adobe=True, mode="auto"))
    _same(g, golden[1]["ycck_2x2/auto"], "the good file on its own")


# ---- 6. the C entry: refusals before any device work ---------------------------------------------------------------------------------------------
def _c_call(A, data, scale, box, comps, out):
    from adaptive_edge_aware_jpeg_amd._lib import JpegAdobe, JpegDecDesc, get_context
    import torch
    ctx = get_context(0)
    lib = ctx.lib
    d = A.standard_jpeg.parse_header(data, adobe=True)
    descs, xs = (JpegDecDesc * 1)(d), (JpegAdobe * 1)(d.adobe)
    scan = torch.frombuffer(bytearray(data[d.scan_offset:d.scan_offset + d.scan_length]), dtype=torch.uint8).cuda()
    sc, bx, cc = (ctypes.c_int * 1)(scale), (ctypes.c_int32 * 4)(*box), (ctypes.c_int * 1)(comps)
    so, oo = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(0)
    status = torch.full((1,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")      # 0xA5 bytes: the entry clears its status words itself
    full = (ctypes.c_int * 1)(4 if d.ncomp == 4 else 3)
    nws = int(lib.aej_jpegdec_workspace_bytes_adobe(ctx.handle, ctypes.addressof(descs), 1, None, ctypes.addressof(full), None, ctypes.addressof(xs)))
    assert nws > 0
    assert (int(lib.aej_jpegdec_workspace_bytes_adobe(ctx.handle, ctypes.addressof(descs), 1, ctypes.addressof(sc), ctypes.addressof(cc),
                                                      ctypes.addressof(bx), ctypes.addressof(xs))) == 0) == (
        scale != 1 or comps == 1 or tuple(box) != (0, 0, d.width, d.height) or (comps == 4 and d.ncomp != 4))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    return lib.aej_jpegdec_batch_adobe(ctx.handle, ctypes.addressof(descs), 1, ctypes.addressof(sc), ctypes.addressof(cc), ctypes.addressof(bx),
                                       ctypes.addressof(xs), scan.data_ptr(), ctypes.c_uint64(scan.numel()), ctypes.addressof(so), out.data_ptr(),
                                       ctypes.c_uint64(out.numel()), ctypes.addressof(oo), status.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws))


def test_c_entry_refusals_leave_the_output_untouched(A, golden):
    import torch
    data = _file("cmyk_2x2")
    pattern = (torch.arange(83 * 61 * 4, device="cuda") % 251).to(torch.uint8)
    out = pattern.clone()
    whole = (0, 0, 83, 61)
    for scale, box, comps in ((2, whole, 3), (1, (0, 0, 8, 8), 3), (1, (3, 5, 30, 40), 4), (1, whole, 1), (8, whole, 4)):
        assert _c_call(A, data, scale, box, comps, out) == -5, (scale, box, comps)      # AEJ_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.equal(out, pattern)
    assert _c_call(A, _file("rgb_1x1"), 1, whole, 4, out) == -1                      # AEJ_ERR_ARG: four channels of three components
    torch.cuda.synchronize()
    assert torch.equal(out, pattern)
    assert _c_call(A, data, 1, whole, 4, out) == 0
    torch.cuda.synchronize()
    _same(out.view(61, 83, 4).cpu().numpy(), golden[1]["cmyk_2x2/auto"], "the C entry, four channels")
    out = pattern.clone()
    assert _c_call(A, data, 1, whole, 3, out) == 0
    torch.cuda.synchronize()
    _same(out[:83 * 61 * 3].view(61, 83, 3).cpu().numpy(), golden[1]["cmyk_2x2/RGB"], "the C entry, RGB")
    assert torch.equal(out[83 * 61 * 3:], pattern[83 * 61 * 3:])


def test_null_array_is_the_box_call(A):
    """aej_jpegdec_batch_adobe with NULL, or with an array that says YCbCr for every file, is aej_jpegdec_batch_box: the same workspace
    size, the same bytes"""
    from adaptive_edge_aware_jpeg_amd._lib import JpegAdobe, JpegDecDesc, get_context
    import torch
    ctx = get_context(0)
    lib = ctx.lib
    data = [R._save(R.picture(61, 83, 3, seed=s), "RGB", quality=85, subsampling=s) for s in (0, 1, 2)]
    ds = [A.standard_jpeg.parse_header(f, adobe=True) for f in data]
    n = len(ds)
    descs, xs = (JpegDecDesc * n)(*ds), (JpegAdobe * n)(*[d.adobe for d in ds])
    scans = torch.cat([torch.frombuffer(bytearray(f[d.scan_offset:d.scan_offset + d.scan_length]), dtype=torch.uint8) for f, d in zip(data, ds)]).cuda()
    so = (ctypes.c_int64 * n)(*np.cumsum([0] + [d.scan_length for d in ds[:-1]]).tolist())
    oo = (ctypes.c_int64 * n)(*[i * 83 * 61 * 3 for i in range(n)])
    head = (ctx.handle, ctypes.addressof(descs), n, None, None, None)
    nws = int(lib.aej_jpegdec_workspace_bytes_box(*head))
    assert nws > 0 and int(lib.aej_jpegdec_workspace_bytes_adobe(*head, None)) == nws
    assert int(lib.aej_jpegdec_workspace_bytes_adobe(*head, ctypes.addressof(xs))) == nws
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    outs = []
    for extra, fn in (((), lib.aej_jpegdec_batch_box), ((None,), lib.aej_jpegdec_batch_adobe), ((ctypes.addressof(xs),), lib.aej_jpegdec_batch_adobe)):
        out = torch.full((n * 83 * 61 * 3,), 7, dtype=torch.uint8, device="cuda")
        status = torch.full((n,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")      # 0xA5 bytes: the entry clears its status words itself
        assert fn(*head, *extra, scans.data_ptr(), ctypes.c_uint64(scans.numel()), ctypes.addressof(so), out.data_ptr(), ctypes.c_uint64(out.numel()),
                  ctypes.addressof(oo), status.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws)) == 0
        torch.cuda.synchronize()
        assert not status.any()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    for i, g in enumerate(_np(A.standard_jpeg_decode_many(data, adobe=True))):
        _same(outs[0][i * 83 * 61 * 3:(i + 1) * 83 * 61 * 3].view(61, 83, 3).cpu().numpy(), g, i)


def test_unaligned_images_in_the_packed_output(A, golden):
    """an image that starts at every offset modulo 4 in the packed output: the dword stores of k_jd_adobe and its byte-wise ends"""
    meta, px = golden
    for k in range(4):                               # k one-pixel RGB images in front: 3 k bytes
        names = ["cmyk_2x2_1x1"] * k + ["ycck_2x2", "cmyk_2x2k", "rgb_2x2"]
        files = [_file(n) for n in names]
        ts = A.standard_jpeg_decode_many(files, adobe=True, mode=["RGB"] * k + ["RGB", "auto", "RGB"])
        for n, g in zip(names[k:], _np(ts)[k:]):
            _same(g, px[n + ("/auto" if g.shape[-1] == 4 else "/RGB")], (k, n))
