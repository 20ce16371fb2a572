"""GPU: grey (one-component) JPEG in standard_jpeg_encode_many (mode="L" / "auto"), standard_jpeg_transcode_many and
standard_jpeg_transform_many (grey=True): the one-component entropy chains of csrc/jfif.hip and csrc/jfifprog.hip, the grey kind of
k_jm_coefs and the one-component mapping of k_jt_transform.  Every comparison is byte- or pixel-exact: against the fixtures under
tests/golden/jfif_grey (Pillow's files of mode-"L" images) always, and against live Pillow where its libjpeg-turbo is the one the
fixtures pin."""
import ctypes
import io
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_reference as JR  # noqa: E402
import jfif_transform_reference as R  # noqa: E402

from conftest import GOLDEN  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = os.path.join(GOLDEN, "jfif_grey")
SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (1, 40), (40, 1), (37, 53), (255, 257)]      # (H, W): the issue's
KINDS = {"baseline": ("", dict()), "optimize": ("_opt", dict(optimize=True)), "progressive": ("_prog", dict(progressive=True))}
AEJ_ERR_ARG, AEJ_ERR_CAPACITY = -1, -4


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


def _file(name):
    with open(os.path.join(FIXTURES, name + ".jpg"), "rb") as f:
        return f.read()


def _pil_save(x, q, **kw):
    """Pillow's file of an array (a larger ImageFile.MAXBLOCK lets one-piece scans through and does not change the bytes)"""
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * x.size + 4096)
    try:
        Image.fromarray(x).save(buf, "JPEG", quality=q, **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


def _pil_decode(data, mode=None):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    return np.asarray(im.convert(mode) if mode else im)


def _colour(h, w, seed):
    rng = np.random.default_rng(seed)
    ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5)[:, :, None] % 256
    return ((rng.integers(0, 256, (h, w, 3)) + ramp) // 2).astype(np.uint8)


@pytest.fixture(scope="module")
def cases():
    """[(name, source pixels, quality)] of the fixtures: noise over a ramp, every size of the issue"""
    with open(os.path.join(FIXTURES, "meta.json")) as f:
        meta = json.load(f)
    px = np.load(os.path.join(FIXTURES, "pixels.npz"))
    out = [(c["name"], px[c["name"] + "_src"], c["quality"]) for c in meta["cases"]]
    assert [x.shape for _, x, _ in out] == SIZES and {q for _, _, q in out} == {1, 10, 50, 75, 95, 100}
    return out


@pytest.fixture(scope="module")
def encoded(A, cases):
    """one ragged mode="L" call per kind, made once: {kind: (files, encode_groups())}"""
    cache = {}

    def get(kind):
        if kind not in cache:
            files = A.standard_jpeg_encode_many([x for _, x, _ in cases], [q for _, _, q in cases], mode="L", **KINDS[kind][1])
            cache[kind] = (files, A.encode_groups())
        return cache[kind]
    return get


# ---- 1. mode="L" files are Pillow's ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_mode_l_files_equal_the_fixtures(cases, encoded, kind):
    files, groups = encoded(kind)
    assert len(files) == len(cases) and groups == len(SIZES)
    for (name, _, _), f in zip(cases, files):
        assert f == _file(name + KINDS[kind][0]), f"{name}, {kind}: bytes differ from Pillow's file"


@live
@pytest.mark.parametrize("kind", list(KINDS))
def test_mode_l_files_equal_live_pillow(A, cases, encoded, kind):
    files, _ = encoded(kind)
    for (name, x, q), f in zip(cases, files):
        assert f == _pil_save(x, q, **KINDS[kind][1]), (name, kind)
    x = cases[4][1]                                                  # subsampling is validated and changes nothing
    for ss in ("4:4:4", "4:2:2", "4:2:0"):
        assert A.standard_jpeg_encode_many([x], 95, subsampling=ss, mode="L", **KINDS[kind][1]) == [files[4]]
        pil = _pil_save(x, 95, subsampling=ss, **KINDS[kind][1])    # Pillow: the factors in the frame header's sampling byte, nothing else
        at = pil.index(b"\xff\xc2" if kind == "progressive" else b"\xff\xc0") + 11
        assert pil[at] == {"4:4:4": 0x11, "4:2:2": 0x21, "4:2:0": 0x22}[ss] and pil[:at] + b"\x11" + pil[at + 1:] == files[4]


@pytest.fixture(scope="module")
def flat_progressive(A):
    """a constant 1032 x 2048 image: 33 024 blocks, more than 32 767, so every AC scan is one end-of-band run that must be split"""
    x = np.full((1032, 2048), 77, np.uint8)
    return x, A.standard_jpeg_encode_many([x], 75, progressive=True, mode="L")[0]


def test_long_end_of_band_runs_decode(A, flat_progressive):
    x, f = flat_progressive
    dec = _pil_decode(f)
    assert len(f) < 20000 and dec.shape == x.shape and (dec == dec[0, 0]).all() and abs(int(dec[0, 0]) - 77) <= 1      # flat, one quantiser step at most
    assert np.array_equal(A.standard_jpeg_decode_many([f], progressive=True)[0].cpu().numpy(), np.repeat(dec[:, :, None], 3, 2))


@live
def test_long_end_of_band_runs_equal_pillow(flat_progressive):
    x, f = flat_progressive
    assert f == _pil_save(x, 75, progressive=True)


# ---- 2. grey and colour in one call --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_auto_mixes_grey_and_colour(A, cases, kind):
    kw = KINDS[kind][1]
    g16, g17, g37 = cases[3][1], cases[4][1], cases[7][1]
    c16, c17 = _colour(16, 16, 5), _colour(17, 33, 6)
    images = [g16, c16, g17, c17, g37, g16, c17]
    qs = [10, 75, 95, 50, 100, 90, 1]
    got = A.standard_jpeg_encode_many(images, qs, mode="auto", **kw)
    assert A.encode_groups() == 5                                    # (16, 16) and (17, 33) once per component count, (37, 53) grey
    grey = [i for i, x in enumerate(images) if x.ndim == 2]
    rgb = [i for i, x in enumerate(images) if x.ndim == 3]
    want_g = A.standard_jpeg_encode_many([images[i] for i in grey], [qs[i] for i in grey], mode="L", **kw)
    assert A.encode_groups() == 3
    want_c = A.standard_jpeg_encode_many([images[i] for i in rgb], [qs[i] for i in rgb], **kw)
    assert [got[i] for i in grey] == want_g and [got[i] for i in rgb] == want_c
    assert got[0] == _file(cases[3][0] + KINDS[kind][0]) and got[4] == _file(cases[7][0] + KINDS[kind][0])
    assert got[0] != got[5] and got[3] != got[6]                     # one chain, two qualities: their own tables
    assert A.standard_jpeg_encode_many([c16, c17], [75, 50], mode="auto", **kw) == A.standard_jpeg_encode_many([c16, c17], [75, 50], **kw)


def test_input_forms_and_comment(A, cases, encoded):
    import torch
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as S
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    images, qs = [x for _, x, _ in cases], [q for _, _, q in cases]
    want, _ = encoded("baseline")
    enc = lambda xs: A.standard_jpeg_encode_many(xs, qs, mode="L")  # noqa: E731
    assert enc([x.astype(np.float32) / np.float32(255) for x in images]) == want
    dev = [torch.from_numpy(x).cuda() for x in images]
    assert enc(dev) == want
    assert enc([(d.float() / 255) if k % 2 else d for k, d in enumerate(dev)]) == want
    assert enc(tuple(images[:4]) + tuple(dev[4:])) == want           # host and device images in one call
    # views of one packed buffer with guard bytes between them: encoded where they lie, grey and colour side by side
    col = _colour(17, 33, 6)
    parts = [images[4], col, images[7]]
    guard, pos, offs = 37, 37, []
    for x in parts:
        offs.append(pos)
        pos += x.size + guard
    buf = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    views = []
    for x, o in zip(parts, offs):
        buf[o:o + x.size] = torch.from_numpy(x).cuda().reshape(-1)
        views.append(buf[o:o + x.size].view(*x.shape))
    before = buf.clone()
    keep, src, nbytes, off = S._packed_source(get_context(0), S._check_images(views, "auto"))
    assert src == buf.data_ptr() and nbytes == buf.numel() and off.tolist() == offs
    got = A.standard_jpeg_encode_many(views, [95, 50, 100], mode="auto")
    assert got == [want[4], A.standard_jpeg_encode_many([col], 50)[0], want[7]] and torch.equal(buf, before)
    # a comment the tensor carries: one COM segment after the JFIF APP0, as for colour
    t = torch.from_numpy(images[3]).cuda()
    t.jpeg_comment = b"hello"
    f = A.standard_jpeg_encode_many([t], 10, mode="L")[0]
    assert f == want[3][:20] + b"\xff\xfe\x00\x07hello" + want[3][20:]
    with pytest.raises(ValueError, match="image 1"):
        A.standard_jpeg_encode_many([images[0], np.full((3, 3), 1.5, np.float32)], mode="L")


# ---- 3. the device's coefficients are the host entry's --------------------------------------------------------------------------------------
def test_device_coefficients_equal_the_host_entry(A, cases, encoded):
    """our progressive files, read back by the library's host-stepped decoder, against aej_jfif_many_coefs_grey_host (which
    tests/test_jfif_grey_host.py pins to a NumPy restatement)"""
    from adaptive_edge_aware_jpeg_amd import _lib
    lib = _lib.load_library()
    files, _ = encoded("progressive")
    for (name, x, q), data in zip(cases, files):
        frame, scans = A.standard_jpeg.parse_scans(data)
        assert (frame.ncomp, frame.hs, frame.vs, frame.blocks_per_mcu, len(scans)) == (1, 1, 1, 1, 6)
        arr = (_lib.JpegProgScan * len(scans))(*scans)
        nb = frame.mcux * frame.mcuy
        got = np.zeros((nb, 64), np.int16)
        buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
        assert lib.aej_test_jpegprog_coefs_host(ctypes.addressof(frame), ctypes.addressof(arr), ctypes.addressof(buf), len(data), 1 << 30,
                                                got.ctypes.data, nb) == 0
        want = np.zeros((nb, 64), np.int16)
        xc = np.ascontiguousarray(x)
        assert lib.aej_jfif_many_coefs_grey_host(x.shape[1], x.shape[0], q, xc.ctypes.data, want.ctypes.data, nb) == nb
        assert np.array_equal(got[:, JR.ZIGZAG], want), name
    d = A.standard_jpeg.parse_header(encoded("optimize")[0][7])
    assert (d.ncomp, d.hs, d.vs, d.blocks_per_mcu, d.width, d.height) == (1, 1, 1, 1, 53, 37)


# ---- 4. our files through our decoder -------------------------------------------------------------------------------------------------------
def test_our_files_decode_to_pillows_pixels(A, cases, encoded):
    for kind in KINDS:
        files, _ = encoded(kind)
        got = A.standard_jpeg_decode_many(files, progressive=kind == "progressive")
        for (name, _, _), f, g in zip(cases, files, got):
            assert np.array_equal(g.cpu().numpy(), _pil_decode(f, "RGB")), (name, kind)


# ---- 5. the transcoder ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ("", "_prog"), ids=("baseline_source", "progressive_source"))
def test_transcode_gives_pillows_files(A, cases, src):
    files = [_file(name + src) for name, _, _ in cases]
    got = A.standard_jpeg_transcode_many(files, grey=True)
    assert A.standard_jpeg.transcode_groups() == len(SIZES)
    for (name, _, _), g in zip(cases, got):
        assert g == _file(name + "_opt"), (name, src)
    got = A.standard_jpeg_transcode_many(files, progressive=True, grey=True)
    for (name, _, _), g in zip(cases, got):
        assert g == _file(name + "_prog"), (name, src)


def test_transcode_mixes_grey_and_colour(A, cases):
    grey_b, grey_p = _file(cases[4][0]), _file(cases[7][0] + "_prog")
    col_b, col_p = _pil_save(_colour(17, 33, 6), 75, subsampling="4:2:0"), _pil_save(_colour(37, 53, 7), 90, subsampling="4:4:4", progressive=True)
    files = [grey_b, col_b, col_p, grey_p]
    for prog in (False, True):
        got = A.standard_jpeg_transcode_many(files, progressive=prog, grey=True)
        assert A.standard_jpeg.transcode_groups() == 4               # (17, 33) twice: the component count is part of the key
        for f, g in zip(files, got):
            assert [g] == A.standard_jpeg_transcode_many([f], progressive=prog, grey=True)
        assert got[1:3] == A.standard_jpeg_transcode_many(files[1:3], progressive=prog)      # the colour files: the call as it was
        assert got[0] == _file(cases[4][0] + ("_prog" if prog else "_opt")) and got[3] == _file(cases[7][0] + ("_prog" if prog else "_opt"))
    with pytest.raises(NotImplementedError, match=r"file 3.*grey=True"):
        A.standard_jpeg_transcode_many([col_b, col_p, col_b, grey_p])


# ---- 6. the transforms ----------------------------------------------------------------------------------------------------------------------
def _grey_noise(h, w, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _file_coefficients(A, data):
    """the quantised coefficients of one of our progressive grey files, [block rows][block columns][64] natural order, read by the
    library's host-stepped decoder"""
    from adaptive_edge_aware_jpeg_amd import _lib
    frame, scans = A.standard_jpeg.parse_scans(data)
    arr = (_lib.JpegProgScan * len(scans))(*scans)
    out = np.zeros((frame.mcuy * frame.mcux, 64), np.int16)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    assert _lib.load_library().aej_test_jpegprog_coefs_host(ctypes.addressof(frame), ctypes.addressof(arr), ctypes.addressof(buf), len(data), 1 << 30,
                                                            out.ctypes.data, out.shape[0]) == 0
    return out.reshape(frame.mcuy, frame.mcux, 64).astype(np.int64)


MIRRORS = ("none", "flip_h", "flip_v", "rot180")


@pytest.mark.parametrize("prog", (False, True))
def test_transforms_give_the_transformed_pixels(A, prog):
    """Sizes that are multiples of 8, all eight transforms, through Pillow's decoder.  Exactly the NumPy-transformed pixels of the
    source's decode: for the four mirrors on noise, and for all eight on constant 8 x 8 tiles (DC-only blocks).  For the four
    transposing transforms on noise that equality cannot hold for any lossless implementation: libjpeg's islow IDCT rounds between
    its column and its row pass, so it does not commute with a transposition -- the exactly transposed coefficients of these very
    sources, entropy-coded on the host, decode through Pillow to pixels that differ from the transposed decode by 1 level at 11 of 384
    (16 x 24) and 1 of 64 (8 x 8) pixels.  There the check is the stronger one on the coefficients themselves: the output's, read back
    from the file, against the NumPy mapping of the source's."""
    from PIL import Image
    tiles = np.random.default_rng(40).integers(0, 256, (2, 3), dtype=np.uint8)
    srcs = [_pil_save(_grey_noise(16, 24), 75), _pil_save(_grey_noise(8, 8, 4), 90, progressive=True),
            _pil_save(np.repeat(np.repeat(tiles, 8, 0), 8, 1), 100), _pil_save(np.full((8, 8), 201, np.uint8), 100)]
    files = [f for f in srcs for _ in R.NAMES]
    names = list(R.NAMES) * len(srcs)
    got = A.standard_jpeg_transform_many(files, names, progressive=prog, grey=True)
    as_prog = got if prog else A.standard_jpeg_transcode_many(got, progressive=True, grey=True)      # the same coefficients, in a file the host decoder reads
    assert as_prog == A.standard_jpeg_transform_many(files, names, progressive=True, grey=True)
    source_coef = [_file_coefficients(A, f) for f in A.standard_jpeg_transcode_many(srcs, progressive=True, grey=True)]
    for i, (f, name, g, p) in enumerate(zip(files, names, got, as_prog)):
        dec = _pil_decode(f)
        im = Image.open(io.BytesIO(g))
        assert im.mode == "L" and im.size == R.pixels(dec, name).shape[::-1] and im.info.get("progressive", 0) == int(prog)
        if name in MIRRORS or i >= 16:
            assert np.array_equal(_pil_decode(g), R.pixels(dec, name)), (i, name, prog)
        want = source_coef[i // 8]
        for step in R.STEPS[name]:
            want = R._step(want, step)
        assert np.array_equal(_file_coefficients(A, p), want), (i, name, prog)
    dec = _pil_decode(srcs[2])
    assert np.array_equal(dec, np.repeat(np.repeat(dec[::8, ::8], 8, 0), 8, 1)) and len(set(dec[::8, ::8].reshape(-1))) == 6      # the tiles decode as tiles
    srcs = srcs[:2]
    once = A.standard_jpeg_transcode_many(srcs, progressive=prog, grey=True)
    assert [got[0], got[8]] == once                                  # "none" is the transcode
    for f, want in zip(srcs, once):
        x = f
        for k in range(4):
            x = A.standard_jpeg_transform_many([x], "rot90", progressive=prog, grey=True)[0]
            assert k == 3 or x != want                               # noise is not its own rotation
        assert x == want
        assert A.standard_jpeg_transform_many(A.standard_jpeg_transform_many([f], "flip_h", progressive=prog, grey=True), "flip_h", progressive=prog, grey=True) == [want]


def test_trim_sampling_byte_and_exif(A):
    from PIL import Image
    x = _grey_noise(37, 53, 9)
    f = _pil_save(x, 75)
    with pytest.raises(ValueError, match="file 0"):
        A.standard_jpeg_transform_many([f], "flip_h", grey=True)
    g = A.standard_jpeg_transform_many([f], "flip_h", trim=True, grey=True)[0]
    assert _pil_decode(g).shape == (37, 48) and np.array_equal(_pil_decode(g), _pil_decode(f)[:, :48][:, ::-1])
    g = A.standard_jpeg_transform_many([f], "rot180", trim=True, grey=True)[0]     # both axes: 37 -> 32 rows, 53 -> 48 columns
    assert np.array_equal(_pil_decode(g), _pil_decode(f)[:32, :48][::-1, ::-1])
    assert _pil_decode(A.standard_jpeg_transform_many([f], "rot90", trim=True, grey=True)[0]).shape == (53, 32)      # rot90 mirrors the source's height
    # the frame header's sampling factors mean nothing for one component
    f = _pil_save(_grey_noise(16, 24), 75)
    at = f.index(b"\xff\xc0") + 11
    assert f[at - 1:at + 2] == bytes([1, 0x11, 0])
    patched = f[:at] + b"\x22" + f[at + 1:]
    for name in ("none", "rot90", "flip_v"):
        assert A.standard_jpeg_transform_many([patched], name, grey=True) == A.standard_jpeg_transform_many([f], name, grey=True)
    # "exif": Orientation 6 is rot90, and with keep_metadata=True the tag becomes 1
    e = Image.Exif()
    e[0x0112] = 6
    f = _pil_save(_grey_noise(16, 24), 75, exif=e.tobytes())
    plain = A.standard_jpeg_transform_many([f], "rot90", grey=True)[0]
    assert A.exif_orientation(f) == 6 and A.standard_jpeg_transform_many([f], "exif", grey=True) == [plain]
    kept = A.standard_jpeg_transform_many([f], "exif", keep_metadata=True, grey=True)[0]
    named = A.standard_jpeg_transform_many([f], "rot90", keep_metadata=True, grey=True)[0]
    im = Image.open(io.BytesIO(kept))
    assert im.mode == "L" and im.size == (16, 24) and im.getexif().get(0x0112) == 1 and Image.open(io.BytesIO(named)).getexif().get(0x0112) == 6
    assert len(kept) == len(named) and sum(a != b for a, b in zip(kept, named)) == 1      # the tag's low byte alone
    app1 = len(kept) - len(plain)
    assert kept[:20] + kept[20 + app1:] == plain


# ---- 7. the C entry: capacity retry and refusals of a grey descriptor --------------------------------------------------------------------------
def _abi_call(ctx, rows, src, src_bytes, out, cap, ss=2, opt=0, prog=0):
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import JfifManyDesc
    lib, n = ctx.lib, len(rows)
    descs = (JfifManyDesc * n)(*[JfifManyDesc(*r) for r in rows])
    nws = int(lib.aej_jfif_many_workspace_bytes(ctx.handle, ctypes.addressof(descs), n, ss, opt, prog))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device="cuda")
    # outputs the entry writes: they start as 0xA5 bytes, not as zeros it could lean on
    offsets, lengths = (torch.full((8 * n,), 0xA5, dtype=torch.uint8, device="cuda").view(torch.int64) for _ in range(2))
    total, groups = ctypes.c_uint64(), ctypes.c_int32()
    rc = lib.aej_jfif_many_encode(ctx.handle, ctypes.addressof(descs), n, src.data_ptr(), ctypes.c_uint64(src_bytes), ss, opt, prog,
                                  out.data_ptr() if out is not None else None, ctypes.c_uint64(cap), offsets.data_ptr(), lengths.data_ptr(),
                                  ctypes.addressof(total), ctypes.addressof(groups), ws.data_ptr(), ctypes.c_uint64(ws.numel()))
    torch.cuda.synchronize()
    return rc, int(total.value), offsets.cpu().tolist(), lengths.cpu().tolist(), nws


def _abi_source(cases, idx):
    import torch
    rows, pos = [], 0
    for i in idx:
        _, x, q = cases[i]
        rows.append((pos, x.shape[1], x.shape[0], q, 1))
        pos += x.size
    return rows, torch.from_numpy(np.concatenate([cases[i][1].reshape(-1) for i in idx])).cuda()


def test_abi_capacity_retry(A, cases, encoded):
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    ctx = get_context(0)
    idx = [4, 7, 3]
    rows, src = _abi_source(cases, idx)
    want = [encoded("baseline")[0][i] for i in idx]
    need = sum(len(f) for f in want)
    rc, total, _, lengths, _ = _abi_call(ctx, rows, src, src.numel(), None, 0)
    assert rc == 0 and total == need and lengths == [len(f) for f in want]
    out = torch.full((need + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    rc, total, _, _, _ = _abi_call(ctx, rows, src, src.numel(), out, need - 1)
    assert rc == AEJ_ERR_CAPACITY and total == need
    assert bool((out[need - 1:] == 0xCD).all()), "a call that does not fit must write nothing past the capacity"
    out.fill_(0xCD)
    rc, total, offsets, lengths, _ = _abi_call(ctx, rows, src, src.numel(), out, need)
    assert rc == 0 and total == need
    blob = out.cpu().numpy().tobytes()
    assert [blob[o:o + m] for o, m in zip(offsets, lengths)] == want and blob[need:] == b"\xcd" * 64


def test_abi_refusals_name_the_image(A, cases):
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    ctx = get_context(0)
    rows, src = _abi_source(cases, [4, 7, 3])
    out = torch.full((1 << 16,), 0xCD, dtype=torch.uint8, device="cuda")
    o1, w1, h1, q1, _ = rows[1]
    for bad, word in (((o1, 0, h1, q1, 1), b"width"), ((o1, w1, 65536, q1, 1), b"height"), ((o1, w1, h1, 0, 1), b"quality"),
                      ((o1, w1, h1, 101, 1), b"quality"), ((o1, w1, h1, q1, 2), b"components"), ((o1, w1, h1, q1, 4), b"components"),
                      ((o1, w1, h1, q1, -1), b"components"), ((-1, w1, h1, q1, 1), b"source"), ((src.numel() - w1 * h1 + 1, w1, h1, q1, 1), b"source"),
                      ((o1, w1, h1, q1, 3), b"source")):             # the same bytes taken as RGB end past the buffer
        r = list(rows)
        r[1] = bad
        rc, _, _, _, nws = _abi_call(ctx, r, src, src.numel(), out, out.numel())
        msg = ctx.lib.aej_last_error(ctx.handle)
        assert rc == AEJ_ERR_ARG and b"image 1" in msg and word in msg, (bad, msg)
        assert nws == 0 or word == b"source"
    rc, _, _, _, _ = _abi_call(ctx, rows, src, src.numel() - 1, out, out.numel())      # the last image ends one byte past the buffer
    assert rc == AEJ_ERR_ARG and b"image 2" in ctx.lib.aej_last_error(ctx.handle)
    assert bool((out == 0xCD).all())                                 # every refusal came before any device work
    rc, _, _, _, _ = _abi_call(ctx, rows, src, src.numel(), out, out.numel())
    assert rc == 0
