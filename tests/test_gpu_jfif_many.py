"""GPU: standard_jpeg_encode_many (csrc/jfifmany.hip: k_jm_coefs, then the transcoder's chains) and standard_jpeg_thumbnail_jpeg_many.
The unconditional oracle is standard_jpeg_many on each image alone -- another front-end kernel, pinned to Pillow by test_gpu_jfif*.py;
where this Pillow's libjpeg-turbo is the one the fixtures pin, Pillow itself is asked too."""
import ctypes
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
LAYOUTS = ("4:4:4", "4:2:2", "4:2:0")
MODES = [(s, o, False) for s in LAYOUTS for o in (False, True)] + [(s, False, True) for s in LAYOUTS]      # (layout, optimize, progressive)
SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (17, 33), (37, 53), (37, 53), (1, 40), (40, 1), (2, 3), (255, 257), (634, 505)]      # (H, W)
QUALITIES = [75, 1, 100, 10, 95, 50, 50, 75, 1, 100, 95, 10]          # the two 17 x 33 differ, the two 37 x 53 agree
AEJ_ERR_ARG, AEJ_ERR_CAPACITY = -1, -4


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _live_matches_fixtures():
    from PIL import features
    with open(os.path.join(GOLDEN, "jfif_options", "meta.json")) as f:
        return features.version("libjpeg_turbo") == json.load(f)["libjpeg_turbo"]


live = pytest.mark.skipif(not _live_matches_fixtures(), reason="this Pillow's libjpeg-turbo is not the one the fixtures pin")


def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5)[:, :, None] % 256
    return ((rng.integers(0, 256, (h, w, 3)) + ramp) // 2).astype(np.uint8)


def _pil_save(im, q, **kw):
    """Pillow's file (a larger ImageFile.MAXBLOCK lets optimised scans of noise through and does not change the bytes)"""
    from PIL import ImageFile
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * im.size[0] * im.size[1] + 4096)
    try:
        im.save(buf, "JPEG", quality=q, **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


@pytest.fixture(scope="module")
def images():
    return [_image(h, w, 11 * k + 1) for k, (h, w) in enumerate(SIZES)]


@pytest.fixture(scope="module")
def encoded(A, images):
    """the ragged call of every mode, made once: {mode: (files, encode_groups())}"""
    cache = {}

    def get(mode):
        if mode not in cache:
            ss, opt, prog = mode
            files = A.standard_jpeg_encode_many(images, QUALITIES, subsampling=ss, optimize=opt, progressive=prog)
            cache[mode] = (files, A.encode_groups())
        return cache[mode]
    return get


def test_the_call_is_the_one_the_issue_describes():
    assert len(SIZES) == len(QUALITIES) == 12 and set(QUALITIES) == {1, 10, 50, 75, 95, 100}
    assert QUALITIES[3] != QUALITIES[4] and QUALITIES[5] == QUALITIES[6]
    assert len(MODES) == 9


# ---- 1. against the same-size encoder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=lambda m: f"{m[0]}-opt{int(m[1])}-prog{int(m[2])}")
def test_files_equal_the_same_size_encoder(A, images, encoded, mode):
    ss, opt, prog = mode
    files, groups = encoded(mode)
    assert len(files) == len(images) and groups == len(set(SIZES)) == 10
    for i, (x, q) in enumerate(zip(images, QUALITIES)):
        want = A.standard_jpeg_many(x, q, subsampling=ss, optimize=opt, progressive=prog)[0]
        assert files[i] == want, f"image {i} ({SIZES[i]}, q={q}), {mode}: bytes differ"
    a, b = files[3], files[4]                                        # one chain, two qualities: their own tables
    assert a != b and a[:20] == b[:20] and a[20:158] != b[20:158]


# ---- 2. against live Pillow -------------------------------------------------------------------------------------------------------------
@live
@pytest.mark.parametrize("mode", MODES, ids=lambda m: f"{m[0]}-opt{int(m[1])}-prog{int(m[2])}")
def test_files_equal_pillow(images, encoded, mode):
    from PIL import Image
    ss, opt, prog = mode
    files, _ = encoded(mode)
    for i, (x, q) in enumerate(zip(images, QUALITIES)):
        assert files[i] == _pil_save(Image.fromarray(x), q, subsampling=ss, optimize=opt, progressive=prog), f"image {i} ({SIZES[i]}, q={q}), {mode}"


# ---- 3. input forms -----------------------------------------------------------------------------------------------------------------------
def test_input_forms_give_the_same_bytes(A, images, encoded):
    import torch
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as S
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    mode = ("4:2:0", False, False)
    want, _ = encoded(mode)
    enc = lambda xs: A.standard_jpeg_encode_many(xs, QUALITIES, subsampling=mode[0])  # noqa: E731
    assert enc([x.astype(np.float32) / np.float32(255) for x in images]) == want
    dev = [torch.from_numpy(x).cuda() for x in images]
    assert enc(dev) == want
    assert enc([(d.float() / 255) if k % 2 else d for k, d in enumerate(dev)]) == want        # float and uint8 tensors mixed
    strided = []
    for x in images:                                                 # every second row / column of a larger tensor
        big = torch.full((2 * x.shape[0], 2 * x.shape[1], 3), 0xA5, dtype=torch.uint8, device="cuda")      # what lies between the strides is not the image
        big[::2, ::2] = torch.from_numpy(x).cuda()
        strided.append(big[::2, ::2])
    assert not strided[-1].is_contiguous() and enc(strided) == want
    assert enc([np.asfortranarray(x) if k % 2 else x for k, x in enumerate(images)]) == want
    assert enc(tuple(images[:6]) + tuple(dev[6:])) == want           # host and device images in one call
    # views of one packed buffer, 37 guard bytes before, between and behind: encoded where they lie
    guard, pos, offs = 37, 37, []
    for x in images:
        offs.append(pos)
        pos += x.size + guard
    buf = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    views = []
    for x, o in zip(images, offs):
        buf[o:o + x.size] = torch.from_numpy(x).cuda().reshape(-1)
        views.append(buf[o:o + x.size].view(*x.shape))
    before, ptrs = buf.clone(), [v.data_ptr() for v in views]
    keep, src, nbytes, off = S._packed_source(get_context(0), S._check_images(views))
    assert src == buf.data_ptr() and nbytes == buf.numel() and off.tolist() == offs       # no copy: the buffer itself, by offset
    assert enc(views) == want
    assert [v.data_ptr() for v in views] == ptrs and torch.equal(buf, before)
    with pytest.raises(ValueError, match="image 1"):
        A.standard_jpeg_encode_many([images[0], np.full((3, 3, 3), 1.5, np.float32)])
    with pytest.raises(ValueError, match="image 1"):
        A.standard_jpeg_encode_many([dev[0], torch.full((3, 3, 3), -0.5, device="cuda")])


# ---- 4. order and boundaries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", LAYOUTS)
def test_order_and_single_image(A, images, ss):
    """one MCU first and thousands of blocks second, then the reverse: the binary search at both ends"""
    small, large = images[0], images[-1]
    fwd = A.standard_jpeg_encode_many([small, large], [50, 75], subsampling=ss)
    assert A.encode_groups() == 2
    rev = A.standard_jpeg_encode_many([large, small], [75, 50], subsampling=ss)
    assert fwd == rev[::-1]
    assert fwd[0] == A.standard_jpeg_many(small, 50, subsampling=ss)[0] and fwd[1] == A.standard_jpeg_many(large, 75, subsampling=ss)[0]
    for x in (small, images[3], large):
        assert A.standard_jpeg_encode_many([x], 75, subsampling=ss, optimize=True) == A.standard_jpeg_many(x, 75, subsampling=ss, optimize=True)
        assert A.encode_groups() == 1


# ---- 5. the C entry: capacity retry and refusals ------------------------------------------------------------------------------------------------
def _abi_call(ctx, rows, src, src_bytes, out, cap, ss=2, opt=0, prog=0):
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import JfifManyDesc
    lib, n = ctx.lib, len(rows)
    descs = (JfifManyDesc * n)(*[JfifManyDesc(o, w, h, q, 0) for o, w, h, q in rows])
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


def _abi_source(images, idx):
    import torch
    rows, pos = [], 0
    for i in idx:
        h, w = images[i].shape[:2]
        rows.append((pos, w, h, QUALITIES[i]))
        pos += images[i].size
    src = torch.from_numpy(np.concatenate([images[i].reshape(-1) for i in idx])).cuda()
    return rows, src


def test_capacity_retry(A, images, encoded):
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    ctx = get_context(0)
    idx = [3, 5, 10, 6]
    rows, src = _abi_source(images, idx)
    want = [encoded(("4:2:0", False, False))[0][i] for i in idx]
    need = sum(len(f) for f in want)
    rc, total, _, lengths, _ = _abi_call(ctx, rows, src, src.numel(), None, 0)      # no output: the sizes alone
    assert rc == 0 and total == need and lengths == [len(f) for f in want]
    out = torch.full((need + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    rc, total, _, _, _ = _abi_call(ctx, rows, src, src.numel(), out, need - 1)
    assert rc == AEJ_ERR_CAPACITY and total == need
    assert b"need" in ctx.lib.aej_last_error(ctx.handle)
    assert bool((out[need - 1:] == 0xCD).all()), "a call that does not fit must write nothing past the capacity"
    out.fill_(0xCD)
    rc, total, offsets, lengths, _ = _abi_call(ctx, rows, src, src.numel(), out, need)
    assert rc == 0 and total == need
    blob = out.cpu().numpy().tobytes()
    assert [blob[o:o + m] for o, m in zip(offsets, lengths)] == want and blob[need:] == b"\xcd" * 64


def test_abi_refusals_name_the_image(A, images):
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    ctx = get_context(0)
    rows, src = _abi_source(images, [3, 5, 1])
    import torch
    out = torch.full((1 << 16,), 0xCD, dtype=torch.uint8, device="cuda")
    o1, w1, h1, q1 = rows[1]
    for bad, word in (((o1, 0, h1, q1), b"width"), ((o1, w1, 65536, q1), b"height"), ((o1, w1, h1, 0), b"quality"), ((o1, w1, h1, 101), b"quality"),
                      ((-1, w1, h1, q1), b"source"), ((src.numel() - w1 * h1 * 3 + 1, w1, h1, q1), b"source")):
        r = list(rows)
        r[1] = bad
        rc, _, _, _, nws = _abi_call(ctx, r, src, src.numel(), out, out.numel())
        msg = ctx.lib.aej_last_error(ctx.handle)
        assert rc == AEJ_ERR_ARG and b"image 1" in msg and word in msg, (bad, msg)
        assert nws == 0 or word == b"source"                         # the size query refuses what it can see
    rc, _, _, _, _ = _abi_call(ctx, rows, src, src.numel() - 1, out, out.numel())      # the last image ends one byte past the buffer
    assert rc == AEJ_ERR_ARG and b"image 2" in ctx.lib.aej_last_error(ctx.handle)
    assert bool((out == 0xCD).all())                                 # every refusal came before any device work
    rc, _, _, _, _ = _abi_call(ctx, rows, src, src.numel(), out, out.numel())
    assert rc == 0


# ---- 6. JPEG to JPEG --------------------------------------------------------------------------------------------------------------------
def _thumbnailed_colour_files():
    """the colour files of tests/golden/jpegdec and jpegprog among the thumbnail fixtures of test_gpu_resample.py, each once"""
    with open(os.path.join(GOLDEN, "resample", "meta.json")) as f:
        cases = json.load(f)["cases"]
    seen, out = set(), []
    for c in cases:
        if c["kind"] == "thumb" and not c["grey"] and c["folder"] in ("jpegdec", "jpegprog") and (c["folder"], c["name"]) not in seen:
            seen.add((c["folder"], c["name"]))
            with open(os.path.join(GOLDEN, c["folder"], c["name"] + ".jpg"), "rb") as f:
                out.append((c["folder"], c["name"], f.read()))
    return out


def test_jpeg_to_jpeg(A):
    src = _thumbnailed_colour_files()
    assert len(src) >= 4 and {f for f, _, _ in src} == {"jpegdec", "jpegprog"}
    files = [d for _, _, d in src]
    got = A.standard_jpeg_thumbnail_jpeg_many(files, (64, 64), quality=80, progressive=True)
    thumbs = A.standard_jpeg_thumbnail_many(files, (64, 64), progressive=True)
    assert got == A.standard_jpeg_encode_many(thumbs, 80)
    assert A.encode_groups() == len({tuple(t.shape) for t in thumbs})
    for (folder, name, _), g, t in zip(src, got, thumbs):
        want, com = A.standard_jpeg_many(t, 80)[0], getattr(t, "jpeg_comment", None)
        assert (com is not None) == ("_com_" in name)
        if com is not None:                                          # the one thing carried over: a COM segment after the JFIF APP0
            want = want[:20] + b"\xff\xfe" + (len(com) + 2).to_bytes(2, "big") + com + want[20:]
        assert g == want, (folder, name)
        assert np.array_equal(A.standard_jpeg_decode_many([g])[0].shape, t.shape)
    qs = [10 + (7 * k) % 90 for k in range(len(files))]
    assert A.standard_jpeg_thumbnail_jpeg_many(files, (40, 30), quality=qs, subsampling="4:4:4", optimize=True, resample="lanczos", progressive=True) == \
        A.standard_jpeg_encode_many(A.standard_jpeg_thumbnail_many(files, (40, 30), resample="lanczos", progressive=True), qs, subsampling="4:4:4", optimize=True)


def _pil_thumbnail_jpeg(d, size, q, **kw):
    from PIL import Image
    im = Image.open(io.BytesIO(d))
    im.thumbnail(size, Image.BICUBIC, reducing_gap=2.0)
    assert im.mode == "RGB"
    return _pil_save(im, q, **kw)


@live
def test_jpeg_to_jpeg_equals_pillow(A):
    """The call against Pillow's thumbnail-then-save, every file.  Two of the files have a COM segment, which Pillow from 9.4 on writes
    again on save (im.info["comment"]): the thumbnails carry it as jpeg_comment and the encoder writes it."""
    import PIL
    src = _thumbnailed_colour_files()
    files = [d for _, _, d in src]
    assert sum(b"a COM segment" in d for d in files) >= 2
    assert tuple(int(v) for v in PIL.__version__.split(".")[:2]) >= (9, 4)
    got = A.standard_jpeg_thumbnail_jpeg_many(files, (64, 64), quality=80, progressive=True)
    differ = [(folder, name) for (folder, name, d), g in zip(src, got) if g != _pil_thumbnail_jpeg(d, (64, 64), 80)]
    assert differ == []
    got = A.standard_jpeg_thumbnail_jpeg_many(files, (50, 70), quality=60, progressive_out=True, progressive=True)
    differ = [(folder, name) for (folder, name, d), g in zip(src, got) if g != _pil_thumbnail_jpeg(d, (50, 70), 60, progressive=True)]
    assert differ == []


def test_truncated_source_raises_the_decoders_error(A):
    def _file(name):
        with open(os.path.join(GOLDEN, "jpegdec", name + ".jpg"), "rb") as f:
            return f.read()
    data, good = _file("buildings_96x128_crop_q95"), _file("lena_64x64_420_q75")
    d = A.standard_jpeg.parse_header(data)
    cut = data[:d.scan_offset + (len(data) - d.scan_offset) // 2]
    with pytest.raises(ValueError) as want:
        A.standard_jpeg_decode_many([good, cut])
    with pytest.raises(ValueError) as got:
        A.standard_jpeg_thumbnail_jpeg_many([good, cut], (20, 20), quality=80)
    assert str(got.value) == str(want.value) and str(got.value).startswith("file 1:")
