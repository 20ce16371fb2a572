"""png_encode_many without a device: the numpy restatement of Pillow's PNG writer (tests/png_encode_reference.py) against Pillow itself
-- scanline stream and whole file, over modes, optimize and levels, and on the rows that decide the filter rule -- and the host-side
validation and declarations of the new entry."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import adaptive_edge_aware_jpeg_amd as A
from adaptive_edge_aware_jpeg_amd import _lib, png as P

import png_encode_cases as C
import png_encode_reference as R


def pil_save(x, **kw):
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, "PNG", **kw)
    return buf.getvalue()


MODE_CASES = C.mode_cases()
CRAFTED = C.crafted_cases()


def agrees_with_pillow(x, optimize, level):
    f = pil_save(x, optimize=optimize, compress_level=level)
    lines = R.scanlines(x, optimize)
    stream, _ = R.idat(f)
    assert zlib.decompress(stream) == lines
    assert R.make_file(x.shape, lines, 9 if optimize else level) == f
    assert R.encode(x, optimize, level) == f


@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("name", sorted(MODE_CASES))
def test_reference_equals_pillow(name, optimize, level):
    x = MODE_CASES[name]
    assert Image.fromarray(x).mode == name.split("-")[0]
    agrees_with_pillow(x, optimize, level)


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_rows_equal_pillow(name, optimize):
    agrees_with_pillow(CRAFTED[name], optimize, 6)


@pytest.mark.parametrize("name", sorted(C.TIES))
def test_a_tie_keeps_the_earlier_filter(name):
    up, row, costs, winner = C.TIES[name]
    got = tuple(R.cost(v) for v in R.filtered(np.array(row, np.uint8), np.array(up, np.uint8), 1))
    assert got == costs                                   # (None, Sub, Up, Average, Paeth)
    order = [R.NONE, R.UP, R.SUB, R.PAETH]                # the order of trial without optimize
    low = min(costs[t] for t in order)
    tied = [t for t in order if costs[t] == low]
    assert len(tied) == 2 and tied[0] == winner and costs[R.AVERAGE] > low      # the tie is real, and the earlier of the two is expected
    for optimize in (False, True):
        assert R.filter_types(C.tie_image(name), optimize)[1] == winner


def test_average_wins_only_with_optimize():
    up, row, costs, with_opt, without = C.AVERAGE
    got = tuple(R.cost(v) for v in R.filtered(np.array(row, np.uint8), np.array(up, np.uint8), 1))
    assert got == costs and costs[R.AVERAGE] < min(costs[t] for t in (R.NONE, R.SUB, R.UP, R.PAETH))
    assert R.filter_types(C.tie_image("average"), True)[1] == with_opt == R.AVERAGE
    assert R.filter_types(C.tie_image("average"), False)[1] == without


def test_zero_rows_and_first_row():
    x = MODE_CASES["RGB-zero-rows"]
    types = R.filter_types(x)
    assert types[0] == R.NONE and types[4] == R.NONE       # cost 0: nothing else is tried, although Up would cost more and Sub as little
    assert R.filter_types(MODE_CASES["L-same-rows"])[1:] == [R.UP] * 5
    # the row above the first row is all zeros: Up and None give the same bytes there, and None, tried first, stays
    first = R.filter_types(MODE_CASES["RGBA-noise"])[0]
    assert first != R.UP
    assert R.cost(np.array([127])) == 127 and R.cost(np.array([128])) == 128 and R.cost(np.array([129])) == 127
    assert R.filter_types(C.fold_image()) == [0, 1, 4]


def test_idat_split_at_65536():
    x = C.split_image()
    f = pil_save(x)
    stream, n = R.idat(f)
    assert len(stream) > R.IDAT_BYTES and n == 2
    assert R.encode(x) == f


@pytest.mark.parametrize("name", sorted(C.size_set()))
def test_size_set_needs_matches(name):
    """The GPU test asks the device deflate to beat Huffman-only coding on these images; Pillow's fastest level must do so too."""
    x = C.size_set()[name]
    lines = R.scanlines(x)
    f = pil_save(x, compress_level=1)
    assert R.encode(x, False, 1) == f
    assert len(f) < R.huffman_only(lines)
    assert 200 <= x.shape[0] <= 256 and x.shape[1] == 256


# ---- the package's host side
def test_validation_names_the_image_and_needs_no_device():
    good = np.zeros((4, 5, 3), np.uint8)
    bad = [
        (np.zeros((4, 5, 3), np.float32), "image 1: dtype"),
        (np.zeros((4, 5, 3, 1), np.uint8), "image 1: shape"),
        (np.zeros((4,), np.uint8), "image 1: shape"),
        (np.zeros((4, 5, 1), np.uint8), "image 1: 1 channels"),
        (np.zeros((4, 5, 5), np.uint8), "image 1: 5 channels"),
        (np.zeros((0, 5, 3), np.uint8), "image 1: shape (0, 5, 3) has no pixels"),
        (np.zeros((4, 0), np.uint8), "image 1: shape (4, 0) has no pixels"),
        ([[1, 2], [3, 4]], "image 1: list"),
    ]
    for x, text in bad:
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)")):
            A.png_encode_many([good, x])
    with pytest.raises(ValueError, match="image 0: .*mode RGB, not the mode 'L'"):
        A.png_encode_many([good], mode="L")
    with pytest.raises(ValueError, match="image 1: .*mode L, not the mode 'RGB'"):
        A.png_encode_many([good, np.zeros((4, 5), np.uint8)], mode="RGB")
    for kw, text in ((dict(mode="P"), "mode"), (dict(entropy="cpu"), "entropy"), (dict(compress_level=10), "compress_level"),
                     (dict(compress_level=-1), "compress_level"), (dict(compress_level=2.5), "compress_level"), (dict(optimize=1), "optimize"),
                     (dict(workers=0), "workers")):
        with pytest.raises(ValueError, match=text):
            A.png_encode_many([good], **kw)
    with pytest.raises(ValueError, match="a list of images"):
        A.png_encode_many(good)
    assert A.png_encode_many([]) == []


def test_host_tensors_are_validated_like_arrays():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="image 0: dtype torch.float32"):
        A.png_encode_many([torch.zeros(4, 5, 3)])
    with pytest.raises(ValueError, match="image 0: shape .* has no pixels"):
        A.png_encode_many([torch.zeros(4, 0, 3, dtype=torch.uint8)])


def test_symbols_and_abi():
    assert "png_encode_many" in A.__all__ and A.png_encode_many is P.png_encode_many
    lib = _lib.load_library()
    for name in ("aej_png_filter_batch", "aej_png_filter_bytes", "aej_deflate_bytes_workspace_bytes", "aej_deflate_bytes_histogram",
                 "aej_deflate_bytes_build_tables", "aej_deflate_bytes_batch"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.aej_abi_version() == 3
    assert lib.aej_png_filter_bytes(7, 12, 3) == 7 * 13
    for h, rb, bpp in ((0, 12, 3), (7, 0, 1), (7, 13, 3), (7, 12, 5), (7, (1 << 24) + 4, 4), ((1 << 24) + 1, 4, 4)):
        assert lib.aej_png_filter_bytes(h, rb, bpp) == 0
    descs = np.array([[0, 8193, 3, 100, 0, 0], [0, 1, 1, 2, 0, 0]], np.int64)
    assert lib.aej_deflate_bytes_workspace_bytes(descs.ctypes.data, 2) > 3 * 8192 * 4
    descs[1, 1] = 0                                        # an empty stream is refused
    assert lib.aej_deflate_bytes_workspace_bytes(descs.ctypes.data, 2) == 0
    assert lib.aej_deflate_bytes_workspace_bytes(None, 2) == 0


def test_build_tables_per_file():
    """aej_deflate_bytes_build_tables: one table per histogram, the construction of aej_deflate_build_tables with cover_all = 0."""
    lib = _lib.load_library()
    rng = np.random.default_rng(3)
    hist = np.zeros((3, 320), np.int32)
    hist[:, :256] = rng.integers(0, 50, (3, 256))
    hist[:, 256] = 1
    hist[1, 257:270] = 7
    hist[1, 286:300] = 3
    want = np.zeros((3, 448), np.uint32)
    cover = np.zeros(3, np.int32)
    assert lib.aej_deflate_build_tables(hist.ctypes.data, cover.ctypes.data, want.ctypes.data) == 0
    got = np.zeros((3, 448), np.uint32)
    assert lib.aej_deflate_bytes_build_tables(hist.ctypes.data, 3, got.ctypes.data) == 0
    assert (got == want).all()
    assert lib.aej_deflate_bytes_build_tables(None, 3, got.ctypes.data) != 0
