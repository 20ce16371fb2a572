"""A NumPy model of Pillow's ``Image.convert`` between its 8-bit modes, of hue adjustment and of ``ImageOps.colorize`` (include/aej.h has
the formulas), without PIL, and the catalogue of cases the convert tests share.  test_convert_host.py pins this model to the installed
Pillow; test_gpu_convert.py compares the library with this model only."""
import numpy as np

MODES = ("L", "LA", "RGB", "RGBA", "YCbCr", "HSV", "CMYK")
BANDS = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4, "YCbCr": 3, "HSV": 3, "CMYK": 4}
DEFAULT_MODE = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
BASE = {"L": "L", "LA": "L", "RGB": "RGB", "RGBA": "RGB", "YCbCr": "RGB", "HSV": "RGB", "CMYK": "RGB"}
# the pairs Image.convert has a converter for (Pillow 12.2); a mode to itself is a copy
DIRECT = {"L": MODES, "LA": MODES, "RGB": MODES, "RGBA": MODES, "YCbCr": ("L", "LA", "RGB", "YCbCr"), "HSV": ("RGB", "HSV"),
          "CMYK": ("RGB", "RGBA", "HSV", "CMYK")}


def route(source, target):
    """the steps Image.convert takes: one where it has a converter, else through the source's base mode"""
    if target in DIRECT[source]:
        return ((source, target),)
    return ((source, BASE[source]), (BASE[source], target))


def _clip8(v):
    return np.clip(v, 0, 255)


def _tab(coef, offset=0):
    """(int)(coef * (i - offset) * 64 + 0.5), the C cast truncating towards zero"""
    return np.trunc(coef * (np.arange(256, dtype=np.float64) - offset) * 64 + 0.5).astype(np.int64)


_T = {c: _tab(c) for c in (.299, .587, .114, -.16874, -.33126, .5, -.41869, -.08131)}
_U = {c: _tab(c, 128) for c in (1.402, -.34414, -.71414, 1.772)}


def luma(r, g, b):
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16


def cmyk_to_rgb(p):
    nk = 255 - p[:, 3]
    out = []
    for c in range(3):
        t = p[:, c] * nk + 128
        out.append(_clip8(nk - (((t >> 8) + t) >> 8)))
    return out


def ycbcr_to_rgb(p):
    y, cb, cr = p[:, 0], p[:, 1], p[:, 2]
    return [_clip8(y + (_U[1.402][cr] >> 6)), _clip8(y + ((_U[-.34414][cb] + _U[-.71414][cr]) >> 6)), _clip8(y + (_U[1.772][cb] >> 6))]


def rgb_to_ycbcr(r, g, b):
    return [(_T[.299][r] + _T[.587][g] + _T[.114][b]) >> 6,
            _clip8(((_T[-.16874][r] + _T[-.33126][g] + _T[.5][b]) >> 6) + 128),
            _clip8(((_T[.5][r] + _T[-.41869][g] + _T[-.08131][b]) >> 6) + 128)]


def rgb_to_hsv(r, g, b):
    f32, f64 = np.float32, np.float64
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = mx == mn
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(f32)
        s = cr / mx.astype(f32)
        rc, gc, bc = ((mx - c).astype(f32) / cr for c in (r, g, b))
        rc, gc, bc = rc.astype(f64), gc.astype(f64), bc.astype(f64)
        h = np.where(r == mx, bc - gc, np.where(g == mx, 2.0 + rc - bc, 4.0 + gc - rc)).astype(f32)
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        H = _clip8(np.where(grey, 0, np.nan_to_num(h.astype(f64) * 255.0)).astype(np.int64))
        S = _clip8(np.where(grey, 0, np.nan_to_num(s.astype(f64) * 255.0)).astype(np.int64))
    return [H, S, mx]


def _round(x):
    """C's round: half away from zero"""
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb(p):
    f32, f64 = np.float32, np.float64
    h, s, v = p[:, 0], p[:, 1], p[:, 2]
    x = h.astype(f64) * 6.0 / 255.0
    i = np.floor(x)
    f = (x - i).astype(f32).astype(f64)
    fs = (s.astype(f64) / 255.0).astype(f32).astype(f64)
    vv = v.astype(f64)
    pp = _clip8(_round(vv * (1.0 - fs)).astype(np.int64))
    q = _clip8(_round(vv * (1.0 - fs * f)).astype(np.int64))
    t = _clip8(_round(vv * (1.0 - fs * (1.0 - f))).astype(np.int64))
    k = i.astype(np.int64) % 6
    sel = (((v, t, pp), (q, v, pp), (pp, v, t), (pp, q, v), (t, pp, v), (v, pp, q)))
    out = []
    for band in range(3):
        o = np.select([k == j for j in range(6)], [sel[j][band] for j in range(6)])
        out.append(np.where(s == 0, v, o))
    return out


def step(pixels, source, target):
    """one converter of Image.convert on [N, bands(source)] ints -> [N, bands(target)] ints"""
    p = pixels
    if source == target:
        return p.copy()
    alpha = p[:, -1] if source in ("LA", "RGBA") else np.full(len(p), 255, np.int64)
    grey = rgb = None
    if source in ("L", "LA") or (source == "YCbCr" and target in ("L", "LA")):
        grey = p[:, 0]
    elif source in ("RGB", "RGBA"):
        rgb = [p[:, 0], p[:, 1], p[:, 2]]
    elif source == "CMYK":
        rgb = cmyk_to_rgb(p)
    elif source == "YCbCr":
        rgb = ycbcr_to_rgb(p)
    else:
        rgb = hsv_to_rgb(p)
    zero = np.zeros(len(p), np.int64)
    if target in ("L", "LA"):
        out = [grey if rgb is None else luma(*rgb)]
    elif target in ("RGB", "RGBA"):
        out = [grey] * 3 if rgb is None else rgb
    elif target == "YCbCr":
        out = [grey, zero + 128, zero + 128] if rgb is None else rgb_to_ycbcr(*rgb)
    elif target == "HSV":
        out = [zero, zero, grey] if rgb is None else rgb_to_hsv(*rgb)
    else:
        out = [zero, zero, zero, 255 - grey] if rgb is None else [255 - rgb[0], 255 - rgb[1], 255 - rgb[2], zero]
    if target in ("LA", "RGBA"):
        out = out + [alpha]
    return np.stack(out, axis=1)


def _pixels(a, bands):
    a = np.asarray(a)
    return a.reshape(-1, bands).astype(np.int64), a.shape[:2]


def _image(p, shape):
    c = p.shape[1]
    return p.astype(np.uint8).reshape(shape + ((c,) if c > 1 else ()))


def convert(a, target, source_mode=None):
    """``Image.fromarray(a, source_mode).convert(target)`` as an array"""
    a = np.asarray(a)
    source = source_mode or DEFAULT_MODE[1 if a.ndim == 2 else a.shape[2]]
    p, shape = _pixels(a, BANDS[source])
    for s, t in route(source, target):
        p = step(p, s, t)
    return _image(p, shape)


def convert_matrix(a, target, matrix):
    """``Image.fromarray(a).convert(target, matrix)`` for an RGB image: target "L" with 4 entries, "RGB" with 12"""
    f32 = np.float32
    p, shape = _pixels(a, 3)
    m = np.asarray(matrix, np.float64).astype(f32).reshape(-1, 4)
    r, g, b = (p[:, k].astype(f32) for k in range(3))
    out = []
    for row in m:
        v = ((row[0] * r + row[1] * g) + row[2] * b) + row[3] + f32(0.5)
        assert v.dtype == f32
        out.append(np.where(v <= 0, 0, np.where(v >= 255, 255, np.trunc(np.clip(v, 0, 255)))).astype(np.int64))
    return _image(np.stack(out, axis=1), shape)


def hue_shift(factor):
    """the byte added to H: int(factor * 255), truncated towards zero, modulo 256"""
    return int(factor * 255) & 255


def hue(a, factor):
    """H of ``convert("HSV")`` moved by int(factor * 255) modulo 256 and back to RGB; alpha kept; grey modes unchanged"""
    a = np.asarray(a)
    if a.ndim == 2 or a.shape[2] == 2:
        return a.copy()
    p, shape = _pixels(a, a.shape[2])
    hsv = step(p[:, :3], "RGB", "HSV")
    hsv[:, 0] = (hsv[:, 0] + hue_shift(factor)) & 255
    rgb = step(hsv, "HSV", "RGB")
    return _image(np.concatenate([rgb, p[:, 3:]], axis=1), shape)


def colorize_table(black, white, mid=None, blackpoint=0, whitepoint=255, midpoint=127):
    """the 768 table entries of ``ImageOps.colorize``, restated: red, green, blue"""
    assert 0 <= blackpoint <= whitepoint <= 255
    if mid is not None:
        assert blackpoint <= midpoint <= whitepoint
    table = []
    for band in range(3):
        lo, hi = black[band], white[band]
        t = [lo] * blackpoint
        if mid is None:
            rng = range(0, whitepoint - blackpoint)
            t += [lo + i * (hi - lo) // len(rng) for i in rng]
        else:
            m = mid[band]
            r1, r2 = range(0, midpoint - blackpoint), range(0, whitepoint - midpoint)
            t += [lo + i * (m - lo) // len(r1) for i in r1]
            t += [m + i * (hi - m) // len(r2) for i in r2]
        t += [hi] * (256 - whitepoint)
        table += t
    return np.array(table, np.int64).astype(np.uint8)


def colorize(a, *args, **kwargs):
    t = colorize_table(*args, **kwargs).reshape(3, 256)
    a = np.asarray(a)
    return np.stack([t[b][a] for b in range(3)], axis=2)


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (3, 5), (17, 33), (64, 61))
HUE_FACTORS = (-0.5, -0.1, 0.0, 0.004, 0.1, 0.5)
XYZ = (0.412453, 0.357580, 0.180423, 0.0, 0.212671, 0.715160, 0.072169, 0.0, 0.019334, 0.119193, 0.950227, 0.0)
MATRICES = (
    ("RGB", (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)),
    ("RGB", XYZ),
    ("RGB", (-1.0, 0.5, 0.25, 100.0, 2.5, 2.5, 2.5, -300.0, 1e6, -1e6, 3.0, 0.0)),
    ("RGB", (0.5, 0.0, 0.0, 0.0, 0.25, 0.25, 0.0, 0.5, 0.0, 0.0, 0.5, -0.5)),      # ties: r / 2 + 0.5 sits on an integer for odd r
    ("L", (0.299, 0.587, 0.114, 0.0)),
    ("L", (0.5, 0.5, 0.0, 0.0)),
    ("L", (-1.0, 0.0, 2.0, 64.5)),
)
COLORIZE = (
    dict(black=(16, 32, 48), white=(250, 240, 230)),
    dict(black=(255, 0, 0), white=(0, 0, 255)),
    dict(black=(0, 0, 0), white=(255, 255, 255), mid=(200, 30, 90)),
    dict(black=(16, 32, 48), white=(250, 240, 230), blackpoint=40, whitepoint=200),
    dict(black=(10, 250, 5), white=(240, 3, 99), mid=(1, 2, 3), blackpoint=30, whitepoint=220, midpoint=100),
    dict(black=(10, 250, 5), white=(240, 3, 99), mid=(128, 128, 0), blackpoint=50, whitepoint=255, midpoint=50),      # blackpoint == midpoint
    dict(black=(0, 9, 0), white=(255, 255, 7), mid=(77, 0, 200), blackpoint=0, whitepoint=130, midpoint=130),         # midpoint == whitepoint
)


def random_image(rng, h, w, bands):
    return rng.integers(0, 256, (h, w) + ((bands,) if bands > 1 else ()), dtype=np.uint8)


def mode_cases(seed=20260):
    """all 49 pairs, each at one of SIZES in turn so that every size meets every band count: -> [(image, source, target)]"""
    rng = np.random.default_rng(seed)
    cases = []
    for i, s in enumerate(MODES):
        for j, t in enumerate(MODES):
            h, w = SIZES[(i + j) % len(SIZES)]
            cases.append((random_image(rng, h, w, BANDS[s]), s, t))
    for s in MODES:                                           # and every source at 1 x 1 to its most distant target
        cases.append((random_image(rng, 1, 1, BANDS[s]), s, "CMYK" if s != "CMYK" else "L"))
    return cases


def all_rgb():
    """4096 x 4096 x 3: every byte triple once"""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)


def all_cmyk():
    """every (c, k) pair in band 0 (a band's result depends on it and k alone; bands 1 and 2 hold other values), then a 64 x 64 x 64 x 4
    grid of the four bands together: [1088, 1024, 4]"""
    c, k = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    pairs = np.stack([c, (c * 7 + k) & 255, (k * 13 + c * 3) & 255, k], axis=-1).reshape(-1, 4)
    g = np.arange(0, 256, 4)
    grid = np.stack(np.meshgrid(g, g + 1, g + 3, np.array([0, 77, 200, 255]), indexing="ij"), axis=-1).reshape(-1, 4)
    return np.concatenate([pairs, grid]).astype(np.uint8).reshape(-1, 1024, 4)
