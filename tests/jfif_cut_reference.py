"""NumPy restatement of the lossless crop and chroma drop of standard_jpeg_transform_many (crop=, drop_chroma=), shared by the host and the
GPU tests.  Written from the rules of the interface alone: the transform (jfif_transform_reference.coefficients) first, on the whole
source; then the box, in the transformed image's coordinates, its corner moved up and left to the output's MCU grid; then a slice of
every component's real blocks.  A one-component output -- a grey source, or a colour one whose chroma is dropped -- has 8 x 8 MCUs and
is sampled 1 x 1, so for it every rule runs with hs = vs = 1 on the luma blocks alone."""
import numpy as np

import jfif_transform_reference as R

LAYOUTS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), "4:4:0": (1, 2)}


def check_box(box, h, w):
    """the refusals of a box against the h x w transformed image: four ints (no bool), 0 <= left < right <= w, 0 <= upper < lower <= h"""
    if len(box) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in box):
        raise ValueError("four ints")
    left, upper, right, lower = box
    if not (0 <= left < right <= w and 0 <= upper < lower <= h):
        raise ValueError("range")


def aligned(box, ohs, ovs):
    """(L, U, right, lower): the corner on the output's MCU grid (8 ohs x 8 ovs)"""
    left, upper, right, lower = box
    return left - left % (8 * ohs), upper - upper % (8 * ovs), right, lower


def geometry(H, W, hs, vs, name, trim, box=None, drop=False, grey=False):
    """-> (oH, oW, ohs, ovs) of the file written and (L, U, right, lower) kept of the transformed image; ValueError as
    jfif_transform_reference's for the transform, "range" for the box"""
    if drop or grey:
        hs = vs = 1
    tH, tW, ohs, ovs = R.out_geometry(H, W, hs, vs, name, trim)
    if box is None:
        return (tH, tW, ohs, ovs), (0, 0, tW, tH)
    check_box(box, tH, tW)
    L, U, right, lower = aligned(box, ohs, ovs)
    return (lower - U, right - L, ohs, ovs), (L, U, right, lower)


def source_planes(blocks, H, W, hs, vs, grey=False):
    """the decoder's layout of one file [block][64] -> per component a grid [rows][cols][64] (a grey file: its blocks in raster order)"""
    if grey:
        return [np.asarray(blocks).reshape(-(-H // 8), -(-W // 8), 64)]
    return R.to_planes(blocks, H, W, hs, vs)


def cut(planes, H, W, hs, vs, name, trim, box=None, drop=False):
    """planes: the source's components (one for a grey source) -> the output's real blocks per component, its (oH, oW, ohs, ovs) and
    the (L, U, right, lower) kept"""
    one = drop or len(planes) == 1
    if one:
        real, _ = R.coefficients(planes[:1], H, W, 1, 1, name, trim)      # the luma blocks alone, under the 8 x 8 rules
    else:
        real, _ = R.coefficients(planes, H, W, hs, vs, name, trim)
    geo, kept = geometry(H, W, hs, vs, name, trim, box, drop, one)
    oH, oW, ohs, ovs = geo
    L, U = kept[:2]
    out = []
    for c, t in enumerate(real):
        ch, cv = (ohs, ovs) if c == 0 else (1, 1)
        r0, c0 = U * cv // (8 * ovs), L * ch // (8 * ohs)
        rows, cols = -(-(-(-oH * cv // ovs)) // 8), -(-(-(-oW * ch // ohs)) // 8)
        part = t[r0:r0 + rows, c0:c0 + cols]
        assert part.shape[:2] == (rows, cols), "a real output block that is no real source block"
        out.append(part)
    return out, geo, kept


def to_output_order(real, oH, oW, ohs, ovs):
    """the real blocks -> [block][64] in the order the coders take: MCU order with the dummy rule, or raster order for one component"""
    if len(real) == 1:
        return np.asarray(real[0]).reshape(-1, 64).astype(np.int64)
    return R.to_mcu_order(real, oH, oW, ohs, ovs)


def check_padded(got, real, oH, oW, ohs, ovs, what=""):
    """jfif_transform_reference.check_padded, and its one-component analogue: the grid is the real blocks, nothing else"""
    if len(real) == 3:
        return R.check_padded(got, real, oH, oW, ohs, ovs, what)
    rows, cols = real[0].shape[:2]
    assert (rows, cols) == (-(-oH // 8), -(-oW // 8)), (what, rows, cols)
    assert len(got) == 1 and np.array_equal(np.asarray(got[0])[:rows, :cols], real[0]), f"{what}: blocks of the one component differ"
