"""CPU: the premise of the rate-distortion sweep (requantising the stored DCT values gives the coefficients of another quality range),
its grid, the container length, argument checks and the result layout.  No device is needed."""
import csv
import importlib
import itertools
import os
import re

import numpy as np
import pytest

import adaptive_edge_aware_jpeg_amd as A
from adaptive_edge_aware_jpeg_amd.evaluation_metrics import PSNR
from conftest import GOLDEN, ROOT, golden_image

S = importlib.import_module("adaptive_edge_aware_jpeg_amd.sweep")      # (the package attribute `sweep` is the function)
CSRC = os.path.join(ROOT, "adaptive_edge_aware_jpeg_amd", "csrc")


def _requantise(Y, leaves, qm_by_size, zz_by_size):
    """numpy restatement of k_requant: coefficient i of a leaf = rint(float64(Y[zz[i]]) / q[zz[i]])"""
    out = np.empty(Y.size, np.int32)
    off = 0
    for s in leaves[:, 2]:
        s = int(s)
        zz = zz_by_size[s]
        y = Y[off:off + s * s].astype(np.float64)[zz]
        q = qm_by_size[s].ravel().astype(np.float64)[zz]
        out[off:off + s * s] = np.rint(y / q).astype(np.int32)
        off += s * s
    return out


@pytest.mark.parametrize("src, space, brange, qa, qb", [
    ("natural/house", "YCoCg-R", (2, 32), (40, 80), (10, 90)),
    ("lena", "YCbCr", (8, 8), (50, 50), (10, 25)),
    ("natural/peppers", "YCbCr", (4, 128), (90, 90), (10, 50)),
    ("natural/baboon", "OKLAB", (4, 64), (25, 75), (75, 90)),
])
def test_requantised_dct_equals_encode_under_other_quality(oracle, src, space, brange, qa, qb):
    img = golden_image(src)[:160, :224]
    img = np.ascontiguousarray(img)
    enc_a = oracle.encode_image(img, space, qa, brange, keep=True)
    enc_b = oracle.encode_image(img, space, qb, brange)
    _, zz, qm_a = oracle.tables(space, qa, brange)
    _, _, qm_b = oracle.tables(space, qb, brange)
    changed = 0
    for l in range(3):
        La, Lb = enc_a[l], enc_b[l]
        assert np.array_equal(La["leaves"], Lb["leaves"]) and np.array_equal(La["states"], Lb["states"]), f"layer {l}: quadtree depends on quality"
        coeffs_a, Y = oracle.blocks_encode(La["norm"], La["leaves"], qm_a[l], zz, want_dct=True)
        assert np.array_equal(coeffs_a, La["coeffs"])
        got = _requantise(Y, np.asarray(La["leaves"]).reshape(-1, 3), qm_b[l], zz)
        assert np.array_equal(got, Lb["coeffs"]), f"layer {l}"
        changed += int(np.count_nonzero(got != La["coeffs"]))
    assert changed > 0          # the two quality ranges quantise differently: the check is not vacuous


def test_reference_grid_is_the_reference_scripts():
    spaces, qrs, brs = A.reference_grid()
    assert tuple(spaces) == ("YCbCr",)
    qv, bv = (10, 25, 50, 75, 90), (4, 8, 16, 32, 64, 128)
    assert qrs == [(a, b) for a in qv for b in qv if a <= b] and len(qrs) == 15
    assert brs == [(a, b) for a in bv for b in bv if a <= b] and len(brs) == 21
    assert qrs[:3] == [(10, 10), (10, 25), (10, 50)] and brs[-2:] == [(64, 128), (128, 128)]
    assert len(list(itertools.product(spaces, qrs, brs))) == 315


@pytest.mark.parametrize("extension", [None, ".png", ".tiff"])
def test_container_length_equals_written_file(oracle, extension):
    img = np.ascontiguousarray(golden_image("natural/house")[:96, :136])
    H, W, _ = img.shape
    for space, qr, br in (("YCbCr", (10, 90), (4, 64)), ("YCoCg-R", (50, 50), (2, 32)), ("ICtCp", (25, 75), (8, 8))):
        layers = oracle.encode_image(img, space, qr, br)
        import zlib
        lens = [len(zlib.compress(np.ascontiguousarray(L["coeffs"], np.int32).tobytes(), level=9)) for L in layers]
        got = S.container_length(H, W, space, qr, br, extension, [len(L["states"]) for L in layers], lens)
        assert got == len(oracle.write_ajpg(layers, H, W, space, qr, br, extension))


def test_arguments_are_checked_before_any_device_work():
    x = np.zeros((1, 64, 64, 3), np.float32)
    with pytest.raises(ValueError, match="Unsupported color space: RGB"):
        A.sweep(x, color_spaces=("RGB",))
    with pytest.raises(ValueError, match="powers of two"):
        A.sweep(x, block_size_ranges=((4, 48),))
    with pytest.raises(ValueError, match="powers of two"):
        A.sweep(x, block_size_ranges=((64, 4),))
    with pytest.raises(NotImplementedError, match="above 1024"):
        A.sweep(x, block_size_ranges=((4, 2048),))
    with pytest.raises(ZeroDivisionError):                      # Jpeg._get_quantization_matrix of quality 0 (jpeg.py:716)
        A.sweep(x, quality_ranges=((0, 50),))
    with pytest.raises(ValueError, match="161x161"):            # MS-SSIM on a 64 x 64 image: refused up front
        A.sweep(x)
    with pytest.raises(ValueError, match="161x161"):
        A.sweep([np.zeros((200, 200, 3), np.float32), np.zeros((100, 300, 3), np.float32)])
    with pytest.raises(ValueError, match="sizes"):
        A.sweep(x, sizes="lzma")
    with pytest.raises(ValueError, match="names"):
        A.sweep(x, metrics=PSNR, names=["a", "b"])


def test_the_settings_errors_are_jpegs(oracle):
    """the block-range rule of the sweep is the library's (aej_set_settings), message for message"""
    src = open(os.path.join(CSRC, "api.hip")).read()
    assert "powers of two with 2 <= min <= max required" in src and "no kernel for blocks above" in src
    for br in ((128, 1024), (4, 4), (2, 256)):
        S.check_block_size_range(br)


def test_quantisation_blob_is_jpegs_layout():
    for cs, qr, br in (("YCbCr", (10, 90), (4, 128)), ("JzAzBz", (50, 50), (8, 8))):
        codec = A.Jpeg(A.JpegCompressionSettings(cs, qr, br))
        assert np.array_equal(S.qmats_blob(cs, qr, br), codec._qmats_blob())


def test_result_layout_and_csv(tmp_path):
    spaces, qrs, brs = ("YCbCr", "YCoCg"), [(10, 50), (75, 90)], [(4, 64), (8, 8), (2, 32)]
    cells = list(itertools.product(spaces, qrs, brs))
    res = S.SweepResult(cells, ["a.png", "b,c.png"], [(200, 300), (200, 300)], PSNR, "zlib")
    assert res.psnr.shape == res.ssim.shape == res.ms_ssim.shape == res.bytes.shape == res.compression_ratio.shape == (2, 12)
    assert res.psnr.dtype == np.float64 and res.bytes.dtype == np.int64 and res.compression_ratio.dtype == np.float64
    res.psnr[:] = np.arange(24).reshape(2, 12) + 0.123456
    res.bytes[:] = 1000
    res.compression_ratio[:] = 180000 / 1000
    rows = res.rows()
    assert len(rows) == 24 and list(rows[0]) == list(S.CSV_COLUMNS) and "lpips" not in rows[0]
    assert rows[12]["image_name"] == "b,c.png" and (rows[12]["color_space"], rows[12]["min_quality"], rows[12]["max_block_size"]) == ("YCbCr", 10, 64)
    p = tmp_path / "cr.csv"
    res.to_csv(p)
    text = p.read_text()
    lines = text.splitlines()
    assert lines[0] == "image_name,color_space,min_quality,max_quality,min_block_size,max_block_size,psnr,ssim,ms_ssim,compression_ratio"
    assert lines[1] == "a.png,YCbCr,10,50,4,64,0.1235,nan,nan,180.0000"
    back = list(csv.DictReader(open(p)))
    assert back[12]["image_name"] == "b,c.png" and back[12]["psnr"] == "12.1235"


def test_one_quantiser_for_encode_and_requantisation():
    """quantise_f64 / quantise_f32 / quantise are defined once (aej_quant.h) and used by the DCT epilogues and the requantisation alike"""
    defs = re.compile(r"__device__[^;{]*\bquantise(_f32|_f64)?\s*\(")
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h")) and f != "aej_quant.h":
            assert not defs.search(open(os.path.join(CSRC, f)).read()), f
    assert len(defs.findall(open(os.path.join(CSRC, "aej_quant.h")).read())) == 3
    for f in ("dct.hip", "requant.hip"):
        assert '#include "aej_quant.h"' in open(os.path.join(CSRC, f)).read()


def test_new_entry_points_are_declared_and_bound():
    from adaptive_edge_aware_jpeg_amd import _lib
    h = open(os.path.join(ROOT, "include", "aej.h")).read()
    for name in ("aej_requantise_batch", "aej_decode_batch_tables"):
        assert re.search(r"AEJ_API int " + name + r"\(", h) and name in _lib.SIGNATURES
        assert hasattr(_lib.load_library(), name)
