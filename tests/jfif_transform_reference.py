"""NumPy restatement of the lossless JPEG transforms (standard_jpeg_transform_many), shared by the host and the GPU tests.  Written
from the definitions alone: flip_h, flip_v and transpose on pixels and on coefficient blocks, the other five as their compositions,
the trim as a crop of the source first.  Coefficients travel as progressive_reference.coefficients returns them: per component an
array [block rows][block columns][64] in natural order."""
import numpy as np

NAMES = ("none", "flip_h", "flip_v", "transpose", "transverse", "rot90", "rot180", "rot270")
TRANSPOSING = ("transpose", "transverse", "rot90", "rot270")
NEEDS_W = ("flip_h", "rot270", "rot180", "transverse")         # the source dimension a mirrored axis takes whole MCUs of
NEEDS_H = ("flip_v", "rot90", "rot180", "transverse")
STEPS = {"none": (), "flip_h": ("flip_h",), "flip_v": ("flip_v",), "transpose": ("transpose",), "rot180": ("flip_h", "flip_v"),
         "rot90": ("transpose", "flip_h"), "rot270": ("flip_h", "transpose"), "transverse": ("transpose", "flip_h", "flip_v")}
ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
LAYOUTS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}


def pixels(x, name):
    """the transform of an image array [H][W](...), by the table of the interface"""
    if name == "none":
        return x
    if name == "flip_h":
        return x[:, ::-1]
    if name == "flip_v":
        return x[::-1]
    if name == "transpose":
        return np.swapaxes(x, 0, 1)
    if name == "transverse":
        return np.swapaxes(x[::-1, ::-1], 0, 1)
    return np.rot90(x, {"rot90": -1, "rot180": 2, "rot270": 1}[name])


def trimmed_source(H, W, hs, vs, name, trim):
    """the source size the transform works on; ValueError when it is not perfect and trim is off, or nothing is left"""
    mw, mh = 8 * hs, 8 * vs
    h, w = H, W
    if name in NEEDS_W and W % mw:
        if not trim:
            raise ValueError("width")
        w = W // mw * mw
    if name in NEEDS_H and H % mh:
        if not trim:
            raise ValueError("height")
        h = H // mh * mh
    if h < 1 or w < 1:
        raise ValueError("nothing left")
    return h, w


def out_geometry(H, W, hs, vs, name, trim):
    h, w = trimmed_source(H, W, hs, vs, name, trim)
    return (w, h, vs, hs) if name in TRANSPOSING else (h, w, hs, vs)


def real_blocks(H, W, hs, vs):
    """[(block rows, block columns)] of the three components' real blocks"""
    out = []
    for h, v in ((hs, vs), (1, 1), (1, 1)):
        cw, ch = -(-W * h // hs), -(-H * v // vs)
        out.append((-(-ch // 8), -(-cw // 8)))
    return out


def _step(c, step):
    """one elementary transform of one component's real blocks [rows][cols][64]"""
    b = c.reshape(c.shape[0], c.shape[1], 8, 8)                # [by][bx][v][u]
    sign = np.where(np.arange(8) % 2 == 1, -1, 1)
    if step == "flip_h":
        b = b[:, ::-1] * sign[None, None, None, :]
    elif step == "flip_v":
        b = b[::-1] * sign[None, None, :, None]
    else:
        b = b.transpose(1, 0, 3, 2)
    return np.ascontiguousarray(b).reshape(b.shape[0], b.shape[1], 64)


def coefficients(coef, H, W, hs, vs, name, trim):
    """coef: the source's components (at least their real blocks) -> the output's real blocks per component, and its geometry"""
    h, w = trimmed_source(H, W, hs, vs, name, trim)
    out = []
    for c, (rows, cols) in zip(coef, real_blocks(h, w, hs, vs)):
        c = np.asarray(c)[:rows, :cols]
        for s in STEPS[name]:
            c = _step(c, s)
        out.append(c)
    return out, out_geometry(H, W, hs, vs, name, trim)


def to_planes(blocks, H, W, hs, vs):
    """[block][64] in MCU order -> per component the MCU-padded grid [rows][cols][64]"""
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    blocks = np.asarray(blocks).reshape(my, mx, hs * vs + 2, 64)
    luma = blocks[:, :, :hs * vs].reshape(my, mx, vs, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my * vs, mx * hs, 64)
    return [luma, blocks[:, :, hs * vs], blocks[:, :, hs * vs + 1]]


def to_mcu_order(real, H, W, hs, vs):
    """the real blocks per component -> [block][64] in MCU order with the dummy blocks of the rule: AC zero, DC of the block before in
    the MCU"""
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    out = np.zeros((my, mx, hs * vs + 2, 64), np.int64)
    for y in range(my):
        for x in range(mx):
            for k in range(hs * vs):
                by, bx = y * vs + k // hs, x * hs + k % hs
                if by < real[0].shape[0] and bx < real[0].shape[1]:
                    out[y, x, k] = real[0][by, bx]
                else:
                    out[y, x, k, 0] = out[y, x, k - 1, 0]
            out[y, x, hs * vs] = real[1][y, x]
            out[y, x, hs * vs + 1] = real[2][y, x]
    return out.reshape(-1, 64)


def check_padded(got, real, H, W, hs, vs, what=""):
    """got: the MCU-padded grids of a file (progressive_reference.coefficients); its real blocks must equal `real` exactly and its
    dummy blocks follow the rule"""
    want = to_planes(to_mcu_order(real, H, W, hs, vs), H, W, hs, vs)
    for c in range(3):
        assert got[c].shape == want[c].shape, (what, c, got[c].shape, want[c].shape)
        rows, cols = real[c].shape[:2]
        assert np.array_equal(got[c][:rows, :cols], real[c]), f"{what}: real blocks of component {c} differ"
        assert np.array_equal(got[c], want[c]), f"{what}: dummy blocks of component {c} do not follow the rule"
