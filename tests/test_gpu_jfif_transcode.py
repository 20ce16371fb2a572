"""GPU: standard_jpeg_transcode_many (csrc/jfiftrans.hip) -- files Huffman-decoded to coefficients and entropy-coded again on the device.
A file Pillow wrote, transcoded, must equal Pillow's optimize=True / progressive=True file of the same pixels byte for byte, whatever
kind the source was (plain, optimised, progressive, with restart markers, with its own quantisation tables): the coefficients are the
same.  Then one mixed call, closure, pixels and tables of the other fixtures, metadata and the error returns."""
import io
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_options_reference as O  # noqa: E402
import jfif_transcode_helpers as H  # noqa: E402
import test_gpu_jfif as T  # noqa: E402  (its image helpers: _png, _fit)

pytestmark = pytest.mark.gpu
QUALITIES = (1, 10, 50, 75, 95, 100)
LAYOUTS = ("4:4:4", "4:2:2", "4:2:0")
KINDS = (dict(), dict(optimize=True), dict(progressive=True), dict(restart_marker_blocks=1), dict(restart_marker_rows=1))
QT = ([(3 * i) % 254 + 1 for i in range(64)], [(7 * i + 5) % 255 + 1 for i in range(64)])


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _pil(x, **opts):
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * x.shape[0] * x.shape[1] + (1 << 17))
    try:
        Image.fromarray(x).save(buf, "JPEG", **opts)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


def _pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _noise(H, W):
    return np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _primaries(H, W):
    prim = np.zeros((H, W, 3), np.uint8)
    band = np.arange(W) * 3 // W
    for c in range(3):
        prim[:, :, c] = np.where(band == c, 255, 0)
    prim[H // 2:] = 255 - prim[H // 2:]
    return prim


IMAGES = {"noise_1x1": lambda: _noise(1, 1), "noise_8x8": lambda: _noise(8, 8), "noise_9x3": lambda: _noise(3, 9),
          "primaries_17x33": lambda: _primaries(17, 33), "noise_37x53": lambda: _noise(37, 53),
          "lena_61x90": lambda: np.ascontiguousarray(T._png("lena")[200:261, 230:320])}


def _check_against_pillow(A, x, settings, kinds):
    """every source kind of every setting in one call per output kind; the expected files are Pillow's own"""
    sources, want_opt, want_prog, names = [], [], [], []
    for s in settings:
        wo, wp = _pil(x, optimize=True, **s), _pil(x, progressive=True, **s)
        for k in kinds:
            sources.append(_pil(x, **s, **k))
            want_opt.append(wo)
            want_prog.append(wp)
            names.append((sorted((a, b) for a, b in s.items() if a != "qtables"), k))
    got = A.standard_jpeg_transcode_many(sources, progressive=False)
    for g, w, nm in zip(got, want_opt, names):
        assert g == w, f"{nm}: baseline transcode differs from Pillow's optimize=True file"
    got = A.standard_jpeg_transcode_many(sources, progressive=True)
    for g, w, nm in zip(got, want_prog, names):
        assert g == w, f"{nm}: progressive transcode differs from Pillow's progressive=True file"


@pytest.mark.parametrize("name", list(IMAGES))
def test_bytes_equal_pillow_small(A, name):
    x = IMAGES[name]()
    settings = [dict(quality=q, subsampling=s) for q in QUALITIES for s in LAYOUTS]
    settings.append(dict(qtables=[list(QT[0]), list(QT[1])], subsampling="4:2:2"))
    _check_against_pillow(A, x, settings, KINDS)


def test_bytes_equal_pillow_256(A):
    """streams of many 64-byte chunks and several decoder subsequences"""
    x = _noise(256, 256)
    settings = [dict(quality=q, subsampling=s) for q, s in ((10, "4:2:0"), (75, "4:2:2"), (100, "4:4:4"), (95, "4:2:0"))]
    _check_against_pillow(A, x, settings, (dict(), dict(progressive=True), dict(restart_marker_rows=1)))
    A.standard_jpeg_transcode_many([_pil(x, quality=100, subsampling="4:4:4")])
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    assert SJ.decode_sync_rounds() > 0


def _mixed_sources():
    imgs = {k: f() for k, f in IMAGES.items()}
    big = _noise(256, 256)
    src = [_pil(imgs["noise_1x1"], quality=75, subsampling="4:2:0"),
           _pil(imgs["noise_8x8"], quality=10, subsampling="4:4:4", progressive=True),
           _pil(imgs["noise_8x8"], quality=95, subsampling="4:4:4"),                        # same group as the one before
           _pil(imgs["noise_9x3"], quality=100, subsampling="4:2:2", restart_marker_blocks=1),
           _pil(imgs["primaries_17x33"], quality=50, subsampling="4:2:0", optimize=True),
           _pil(imgs["primaries_17x33"], quality=50, subsampling="4:2:2"),                  # same size, another layout
           _pil(imgs["noise_37x53"], quality=1, subsampling="4:2:0", progressive=True),
           _pil(imgs["noise_37x53"], quality=100, subsampling="4:2:0", restart_marker_rows=1),
           _pil(imgs["lena_61x90"], quality=75, subsampling="4:4:4", progressive=True),
           _pil(imgs["lena_61x90"], qtables=[list(QT[0]), list(QT[1])], subsampling="4:2:2"),
           _pil(big, quality=75, subsampling="4:2:0"),
           _pil(big, quality=10, subsampling="4:2:0", progressive=True)]
    order = np.random.default_rng(12).permutation(len(src))
    return [src[i] for i in order], 9      # groups: 1x1, 8x8, 9x3, 17x33 twice, 37x53, 61x90 twice, 256x256


@pytest.mark.parametrize("prog", (False, True))
def test_mixed_call(A, prog):
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    src, groups = _mixed_sources()
    got = A.standard_jpeg_transcode_many(src, progressive=prog)
    assert SJ.transcode_groups() == groups
    assert len(got) == len(src)
    for i, s in enumerate(src):
        alone = A.standard_jpeg_transcode_many([s], progressive=prog)
        assert SJ.transcode_groups() == 1
        assert got[i] == alone[0], f"file {i}: the mixed call and the single call differ"
        assert np.array_equal(_pil_decode(got[i]), _pil_decode(s)), i


def test_closure(A):
    src, _ = _mixed_sources()
    base = A.standard_jpeg_transcode_many(src, progressive=False)
    prog = A.standard_jpeg_transcode_many(src, progressive=True)
    assert A.standard_jpeg_transcode_many(prog, progressive=False) == base
    assert A.standard_jpeg_transcode_many(base, progressive=True) == prog
    assert A.standard_jpeg_transcode_many(base, progressive=False) == base
    assert A.standard_jpeg_transcode_many(prog, progressive=True) == prog


def _fixture_files():
    out = []
    for folder in ("jpegdec", "jpegprog"):
        with open(os.path.join(GOLDEN, folder, "meta.json")) as f:
            cases = json.load(f)["cases"]
        for c in cases:
            with open(os.path.join(GOLDEN, folder, c["name"] + ".jpg"), "rb") as f:
                out.append((folder + "/" + c["name"], c["mode"], f.read()))
    return out


@pytest.mark.parametrize("prog", (False, True))
def test_fixture_pixels_and_tables(A, prog):
    from PIL import Image
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    files = _fixture_files()
    keep = [(n, d) for n, mode, d in files if mode == "RGB" and "qt16" not in n]
    assert len(keep) >= 25
    for n, mode, d in files:                                 # the rest is refused by name, before any device work
        if mode != "RGB" or "qt16" in n:
            with pytest.raises(NotImplementedError, match="file 1"):
                A.standard_jpeg_transcode_many([keep[0][1], d], progressive=prog)
    src = [d for _, d in keep]
    out = A.standard_jpeg_transcode_many(src, progressive=prog)
    ours_src = A.standard_jpeg_decode_many(src, progressive=True)
    ours_out = A.standard_jpeg_decode_many(out, progressive=True)
    for (n, s), o, a, b in zip(keep, out, ours_src, ours_out):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), n
        assert np.array_equal(_pil_decode(o), _pil_decode(s)), n
        io_, is_ = Image.open(io.BytesIO(o)), Image.open(io.BytesIO(s))
        assert {k: list(v) for k, v in io_.quantization.items()} == {k: list(v) for k, v in is_.quantization.items()}, n
        assert io_.info.get("progressive", 0) == (1 if prog else 0), n
        assert 0xDD not in [m for m, _, _ in SJ.marker_segments(o)], n      # no DRI: restart markers are dropped


def test_metadata(A):
    """Byte equality with Pillow's own file holds with the metadata too: Pillow writes APP0, EXIF, ICC (chunks of 65519 bytes), COM
    before the tables, which is where the splice puts the source's segments."""
    from PIL import Image
    exif = Image.Exif()
    exif[0x010E] = "a description"
    icc = bytes(range(256)) * 273 + bytes(112)
    x = IMAGES["lena_61x90"]()
    extra = dict(exif=exif.tobytes(), icc_profile=icc, comment=b"hello", dpi=(300, 72))
    src = _pil(x, quality=75, subsampling="4:2:0", **extra)
    for prog in (False, True):
        kind = dict(progressive=True) if prog else dict(optimize=True)
        with_meta = A.standard_jpeg_transcode_many([src], progressive=prog, keep_metadata=True)[0]
        assert with_meta == _pil(x, quality=75, subsampling="4:2:0", **extra, **kind)
        info = Image.open(io.BytesIO(with_meta)).info
        assert info["exif"] == exif.tobytes() and info["icc_profile"] == icc and info["comment"] == b"hello" and tuple(info["dpi"]) == (300, 72)
        without = A.standard_jpeg_transcode_many([src], progressive=prog)[0]
        assert without == _pil(x, quality=75, subsampling="4:2:0", dpi=(300, 72), **kind)


@pytest.mark.parametrize("prog", (False, True))
def test_foreign_component_ids(A, prog):
    """Sources whose component ids are not 1, 2, 3 (a baseline file with 0, 1, 2 and a progressive one with 'Y', 'C', 'c', both 4:2:0,
    beside an ordinary file of the same group): the output carries them in its frame header and in every scan header -- for the
    progressive output that is the one path on which the device rewrites the scan headers -- and is otherwise Pillow's own file."""
    x = IMAGES["noise_37x53"]()
    ids_b, ids_p = (0, 1, 2), (ord("Y"), ord("C"), ord("c"))
    kind = dict(progressive=True) if prog else dict(optimize=True)
    want = _pil(x, quality=75, subsampling="4:2:0", **kind)
    src = [H.with_ids(_pil(x, quality=75, subsampling="4:2:0"), ids_b), _pil(x, quality=75, subsampling="4:2:0"),
           H.with_ids(_pil(x, quality=75, subsampling="4:2:0", progressive=True), ids_p)]
    assert H.ids_of(src[0])[0] == list(ids_b) and H.ids_of(src[2])[0] == list(ids_p)
    out = A.standard_jpeg_transcode_many(src, progressive=prog)
    ours = A.standard_jpeg_decode_many(out, progressive=True)
    for o, s, ids, dec in zip(out, src, (ids_b, (1, 2, 3), ids_p), ours):
        frame, scans = H.ids_of(o)
        assert frame == list(ids)
        assert len(scans) == (10 if prog else 1)
        for sc in scans:
            assert sc == list(ids) if len(sc) == 3 else (len(sc) == 1 and sc[0] in ids), (ids, scans)
        assert o == H.with_ids(want, ids)                     # byte for byte Pillow's file, but for the ids
        assert np.array_equal(_pil_decode(o), _pil_decode(s)) and np.array_equal(_pil_decode(o), _pil_decode(want))
        assert np.array_equal(dec.cpu().numpy(), _pil_decode(s))


def _one_block_file(dc, ac, where=1):
    """8 x 8, 4:4:4, one MCU whose luma block holds the DC value `dc` and the AC coefficient `ac` at zigzag position `where`, coded by the
    tests' own restatement under tables built for exactly these symbols (no 8-bit encoder writes category 11)"""
    y = np.zeros(64, np.int64)
    y[0], y[where], y[5] = dc, ac, -2
    blocks = [(0, y), (1, np.zeros(64, np.int64)), (2, np.zeros(64, np.int64))]
    tabs = O.tables(blocks, True)
    return O.headers(50, 8, 8, 0, tabs) + O.entropy(blocks, tabs) + b"\xff\xd9"


def _ac_1024_file():
    return _one_block_file(3, 1024)


def test_coefficient_range_edges(A):
    """libjpeg's limits exactly: DC -1024 .. 1023 and AC -1023 .. 1023 pass (and survive: the output holds the same coefficients, so
    the transcode of the output is the output); one step outside fails the file."""
    inside = [_one_block_file(1023, 1023), _one_block_file(-1024, -1023), _one_block_file(1023, -1023, 63), _one_block_file(-1024, 1023, 63)]
    for prog in (False, True):
        out = A.standard_jpeg_transcode_many(inside, progressive=prog)
        assert A.standard_jpeg_transcode_many(out, progressive=prog) == out
        for o, s in zip(out, inside):
            assert np.array_equal(_pil_decode(o), _pil_decode(s))
        back = A.standard_jpeg_transcode_many(out, progressive=False)
        assert back == A.standard_jpeg_transcode_many(inside, progressive=False)
    for dc, ac, where in ((1024, 5, 1), (-1025, 5, 1), (0, -1024, 1), (0, 1024, 63), (0, -1024, 63)):
        bad = _one_block_file(dc, ac, where)
        for prog in (False, True):
            with pytest.raises(ValueError, match=r"file 1: coefficient out of range"):
                A.standard_jpeg_transcode_many([inside[0], bad], progressive=prog)


def test_errors(A):
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as SJ
    good = _pil(_noise(37, 53), quality=75, subsampling="4:2:0")
    other = _pil(_noise(8, 8), quality=75, subsampling="4:4:4", progressive=True)
    want = A.standard_jpeg_transcode_many([good, other])
    cut = good[:good.index(b"\xff\xda") + 14 + 40]           # the scan ends after 40 bytes
    with pytest.raises(ValueError, match=r"file 1: truncated scan"):
        A.standard_jpeg_transcode_many([good, cut, other])
    bad = _ac_1024_file()
    assert _pil_decode(bad).shape == (8, 8, 3)                # a file decoders read
    for prog in (False, True):
        with pytest.raises(ValueError, match=r"file 2: coefficient out of range"):
            A.standard_jpeg_transcode_many([good, other, bad], progressive=prog)
    assert A.standard_jpeg_transcode_many([good, other]) == want      # an ordinary error return: the device goes on working
    # a refused file: the call raises before any device work
    A.standard_jpeg_transcode_many([_pil(_noise(256, 256), quality=100, subsampling="4:4:4")])
    rounds, groups = SJ.decode_sync_rounds(), SJ.transcode_groups()
    assert rounds > 0
    grey = _pil(np.ascontiguousarray(_noise(9, 9)[:, :, 0]), quality=50)
    with pytest.raises(NotImplementedError, match="file 1"):
        A.standard_jpeg_transcode_many([good, grey])
    assert SJ.decode_sync_rounds() == rounds and SJ.transcode_groups() == groups
