"""Pillow's ``Image.transform``, ``Image.rotate`` and ``Image.transpose`` restated in NumPy, and the case catalogue the warp tests share.

The model is IEEE float64, one operation at a time, in Pillow's order (DESIGN.md has the contract).  Its keyword switches turn on
the wrong variants that test_warp_host.py shows to differ from Pillow on the catalogue:

  half=False            coordinates without the half-pixel offset
  f32=True              coordinates in float32
  round_result=True     the interpolated value rounded, not truncated
  generic_nearest=True  AFFINE under NEAREST through the float64 path, not 16.16 fixed point / the tables
  direct_tables=True    the scale tables as a0 * (x + 0.5) + a2, not as running sums
  premultiply=False     interpolation of LA / RGBA without premultiplied alpha (also a public option: what Pillow does for CMYK)
  premul_fill=True      the fill colour premultiplied on its way in

Nothing here imports the package; `pillow()` is the only function that imports PIL."""
import math

import numpy as np

NEAREST, BILINEAR, BICUBIC = 0, 2, 3
AFFINE, EXTENT, PERSPECTIVE, QUAD = "affine", "extent", "perspective", "quad"
TRANSPOSE_NAMES = ("FLIP_LEFT_RIGHT", "FLIP_TOP_BOTTOM", "ROTATE_90", "ROTATE_180", "ROTATE_270", "TRANSPOSE", "TRANSVERSE")
FIXED_LIMIT = 32768.0


# ---- the host plan ----------------------------------------------------------------------------------------------------------------
def coefficients(method, data, w, h):
    """-> (kind, eight float64): Image.py's conversion of EXTENT to AFFINE and of QUAD's corners to its bilinear form"""
    data = [float(v) for v in data]
    if method == AFFINE:
        return AFFINE, data[:6] + [0.0, 0.0]
    if method == EXTENT:
        x0, y0, x1, y1 = data
        return AFFINE, [(x1 - x0) / w, 0.0, x0, 0.0, (y1 - y0) / h, y0, 0.0, 0.0]
    if method == PERSPECTIVE:
        return PERSPECTIVE, data[:8]
    nw, sw, se, ne = data[0:2], data[2:4], data[4:6], data[6:8]
    x0, y0 = nw
    As, At = 1.0 / w, 1.0 / h
    return QUAD, [x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
                  y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At]


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def fixed_constants(a):
    """A0 .. A5 of the 16.16 path"""
    return [fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]


def fixed_guard(a, w, h):
    return all(abs(x * a[0] + y * a[1] + a[2]) < FIXED_LIMIT and abs(x * a[3] + y * a[4] + a[5]) < FIXED_LIMIT
               for x, y in ((0, 0), (w, h), (0, h), (w, 0)))


def coord(v):
    """Pillow's COORD: -1 below zero, else truncation (beyond an int: outside, so -1 as well)"""
    return -1 if v < 0 or v >= 2147483648.0 else int(v)


def scale_tables(a, w, h, direct=False):
    """the two tables of the pure-scale path, by running sums as Pillow builds them"""
    out = []
    for n, step, off in ((w, a[0], a[2]), (h, a[4], a[5])):
        tab, o = np.empty(n, np.int32), off + step * 0.5
        for i in range(n):
            tab[i] = coord(step * (i + 0.5) + off) if direct else coord(o)
            o += step
        out.append(tab)
    return out


def nearest_path(kind, a, w, h):
    """which of Pillow's NEAREST loops an image takes: "tables", "fixed", "float" (the unbuilt fallback) or "generic" """
    if kind != AFFINE:
        return "generic"
    if a[1] == 0 and a[3] == 0:
        return "tables"
    return "fixed" if fixed_guard(a, w, h) else "float"


# ---- pixels -----------------------------------------------------------------------------------------------------------------------
def premultiply(a):
    """LA -> La, RGBA -> RGBa"""
    out = a.copy()
    alpha = a[..., -1].astype(np.int64)
    for c in range(a.shape[2] - 1):
        t = a[..., c].astype(np.int64) * alpha + 128
        out[..., c] = ((t >> 8) + t) >> 8
    return out


def unpremultiply(a):
    out = a.copy()
    alpha = a[..., -1].astype(np.int64)
    mid = (alpha != 0) & (alpha != 255)
    safe = np.where(alpha == 0, 1, alpha)
    for c in range(a.shape[2] - 1):
        v = np.minimum(255, (255 * a[..., c].astype(np.int64)) // safe)
        out[..., c] = np.where(mid, v, a[..., c])
    return out


def fill_bytes(fillcolor, channels):
    """what Image.new puts into every pixel: an int from 0 to 255 fills the first channel and leaves the others 0, alpha included"""
    if fillcolor is None:
        return [0] * channels
    if isinstance(fillcolor, (tuple, list)):
        return [int(v) for v in fillcolor]
    v = int(fillcolor)
    return [v] + [0] * (channels - 1)


def _coords(kind, a, w, h, half, f32):
    t = np.float32 if f32 else np.float64
    a = [t(v) for v in a]
    off = t(0.5) if half else t(0.0)
    xin = (np.arange(w, dtype=t) + off)[None, :] * np.ones((h, 1), t)
    yin = (np.arange(h, dtype=t) + off)[:, None] * np.ones((1, w), t)
    with np.errstate(all="ignore"):
        if kind == QUAD:
            xx = a[0] + a[1] * xin + a[2] * yin + a[3] * xin * yin
            yy = a[4] + a[5] * xin + a[6] * yin + a[7] * xin * yin
        else:
            xx = a[0] * xin + a[1] * yin + a[2]
            yy = a[3] * xin + a[4] * yin + a[5]
            if kind == PERSPECTIVE:
                den = a[6] * xin + a[7] * yin + t(1)
                xx, yy = xx / den, yy / den
    return xx.astype(np.float64), yy.astype(np.float64)


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def _interpolate(src, xx, yy, resample, round_result):
    """-> (values [h, w, C] uint8, inside [h, w]) for BILINEAR / BICUBIC"""
    H, W, C = src.shape
    with np.errstate(invalid="ignore"):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)          # a NaN coordinate is outside
    xs, ys = np.where(inside, xx, 0.0) - 0.5, np.where(inside, yy, 0.0) - 0.5
    x, y = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    dx, dy = (xs - x)[..., None], (ys - y)[..., None]
    p = src.astype(np.float64)
    cx = lambda v: np.clip(v, 0, W - 1)
    if resample == BILINEAR:
        def row(r):
            r = np.clip(r, 0, H - 1)
            lo, hi = p[r, cx(x)], p[r, cx(x + 1)]
            return lo + (hi - lo) * dx
        v1 = row(y)
        v2 = np.where(((y + 1 >= 0) & (y + 1 < H))[..., None], row(y + 1), v1)
        v = v1 + (v2 - v1) * dy
    else:
        x, y = x - 1, y - 1

        def row(r):
            r = np.clip(r, 0, H - 1)
            return _cubic(p[r, cx(x)], p[r, cx(x + 1)], p[r, cx(x + 2)], p[r, cx(x + 3)], dx)
        rows = [row(y)]
        for k in (1, 2, 3):
            rows.append(np.where(((y + k >= 0) & (y + k < H))[..., None], row(y + k), rows[-1]))
        v = _cubic(rows[0], rows[1], rows[2], rows[3], dy)
        v = np.clip(v, 0.0, 255.0)
    if round_result:
        v = np.floor(v + 0.5)
    return np.minimum(v, 255.0).astype(np.uint8), inside


def transform(a, size, method, data, resample=NEAREST, fillcolor=None, premultiply_alpha=True, *, half=True, f32=False,
              round_result=False, generic_nearest=False, direct_tables=False, premul_fill=False):
    """``Image.fromarray(a).transform(size, method, data, resample, fillcolor=fillcolor)`` as an array"""
    a = np.asarray(a)
    src = a if a.ndim == 3 else a[..., None]
    H, W, C = src.shape
    w, h = size
    kind, co = coefficients(method, data, w, h)
    fill = np.array(fill_bytes(fillcolor, C), np.uint8)
    alpha = C in (2, 4) and resample != NEAREST and premultiply_alpha
    if alpha:
        src = premultiply(src)
        if premul_fill:
            fill = premultiply(fill[None, None, :])[0, 0]
    if resample == NEAREST:
        path = "generic" if generic_nearest else nearest_path(kind, co, w, h)
        if path == "float":
            raise NotImplementedError("the float64 running-sum fallback beyond +-32768")
        if path == "tables":
            xtab, ytab = scale_tables(co, w, h, direct_tables)
            xi, yi = np.broadcast_to(xtab[None, :], (h, w)).astype(np.int64), np.broadcast_to(ytab[:, None], (h, w)).astype(np.int64)
        elif path == "fixed":
            A = fixed_constants(co)
            X, Y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
            xi, yi = (A[2] + X * A[0] + Y * A[1]) >> 16, (A[5] + X * A[3] + Y * A[4]) >> 16
        else:
            xx, yy = _coords(kind, co, w, h, half, f32)
            with np.errstate(invalid="ignore"):
                ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            xi, yi = np.where(ok, xx, -1.0).astype(np.int64), np.where(ok, yy, -1.0).astype(np.int64)
        inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        val = src[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]
    else:
        xx, yy = _coords(kind, co, w, h, half, f32)
        val, inside = _interpolate(src, xx, yy, resample, round_result)
    out = np.where(inside[..., None], val, fill[None, None, :]).astype(np.uint8)
    if alpha:
        out = unpremultiply(out)
    return out if a.ndim == 3 else out[..., 0]


def transpose(a, method):
    """``Image.transpose``; method 0 .. 6 or its name"""
    m = TRANSPOSE_NAMES.index(method) if isinstance(method, str) else int(method)
    t = lambda v: np.swapaxes(v, 0, 1)
    return np.ascontiguousarray((a[:, ::-1], a[::-1], t(a)[::-1], a[::-1, ::-1], t(a)[:, ::-1], t(a), t(a)[::-1, ::-1])[m])


def rotate_plan(W, H, angle, expand=False, center=None, translate=None):
    """``Image.rotate`` up to its last line: ("copy",), ("transpose", m) or ("affine", (w, h), matrix)"""
    angle = angle % 360.0
    if not (center or translate):
        if angle == 0:
            return ("copy",)
        if angle == 180:
            return ("transpose", 3)
        if angle in (90, 270) and (expand or W == H):
            return ("transpose", 2 if angle == 90 else 4)
    w, h = W, H
    post = (0, 0) if translate is None else translate
    if center is None:
        center = (w / 2, h / 2)
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]

    def tf(x, y, m):
        a, b, c, d, e, f = m
        return a * x + b * y + c, d * x + e * y + f
    m[2], m[5] = tf(-center[0] - post[0], -center[1] - post[1], m)
    m[2] += center[0]
    m[5] += center[1]
    if expand:
        xx, yy = zip(*(tf(x, y, m) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
        nw, nh = math.ceil(max(xx)) - math.floor(min(xx)), math.ceil(max(yy)) - math.floor(min(yy))
        m[2], m[5] = tf(-(nw - w) / 2.0, -(nh - h) / 2.0, m)
        w, h = nw, nh
    return ("affine", (w, h), m)


def rotate(a, angle, resample=NEAREST, expand=False, center=None, translate=None, fillcolor=None, premultiply_alpha=True, **switches):
    a = np.asarray(a)
    plan = rotate_plan(a.shape[1], a.shape[0], angle, expand, center, translate)
    if plan[0] == "copy":
        return a.copy()
    if plan[0] == "transpose":
        return transpose(a, plan[1])
    return transform(a, plan[1], AFFINE, plan[2], resample, fillcolor, premultiply_alpha, **switches)


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------
def image(h, w, c, seed=0):
    """a deterministic image with structure and noise; alpha (the last of 2 or 4 channels) takes 0, 255 and everything between"""
    rng = np.random.default_rng(1000 * h + 10 * w + c + seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * (7 + 3 * k) + y * (5 + 2 * k) + 31 * k) % 256 for k in range(c)], -1).astype(np.int64)
    a = (a + rng.integers(-40, 41, a.shape)) % 256
    if c in (2, 4):
        alpha = rng.integers(0, 256, (h, w))
        alpha[rng.random((h, w)) < 0.2] = 0
        alpha[rng.random((h, w)) < 0.2] = 255
        a[..., -1] = alpha
    a = a.astype(np.uint8)
    return a[..., 0] if c == 1 else a


def _rot(deg, scale, cx, cy, tx, ty):
    c, s = math.cos(math.radians(deg)) * scale, math.sin(math.radians(deg)) * scale
    return (c, s, cx - c * tx - s * ty, -s, c, cy + s * tx - c * ty)


FILLS = {1: (None, 77, (200,)), 2: (None, 90, (120, 60)), 3: (None, 255, (10, 200, 30)), 4: (None, 40, (250, 128, 7, 100))}


def catalogue():
    """-> list of (kind, image, kwargs): kind "transform", "rotate" or "transpose"; kwargs are the public call's, with `resample`
    0 / 2 / 3 and `method` a name.  Small on purpose: sources and outputs up to about 70 a side."""
    cases = []
    k = 0

    def add(kind, a, **kw):
        cases.append((kind, a, kw))

    def fill(c):
        nonlocal k
        k += 1
        return FILLS[c][k % 3]

    for c in (1, 2, 3, 4):
        big, small = image(37, 53, c), image(9, 6, c, 1)
        for f in (NEAREST, BILINEAR, BICUBIC):
            # AFFINE: a rotation with scale; entries 16.16 cannot hold, over a span of more than 60 pixels; a shear; an integer translation
            add("transform", big, size=(64, 41), method=AFFINE, data=_rot(23.0, 0.8, 26.0, 18.0, 32.0, 20.0), resample=f, fillcolor=fill(c))
            add("transform", big, size=(70, 66), method=AFFINE, data=(1 / 3, 0.7, -11.3, -0.7, 1 / 3, 41.9), resample=f, fillcolor=fill(c))
            add("transform", small, size=(13, 11), method=AFFINE, data=(1.0, 0.31, -2.0, 0.12, 0.9, -1.5), resample=f, fillcolor=fill(c))
            add("transform", big, size=(53, 37), method=AFFINE, data=(1, 0, 5, 0, 1, -3), resample=f, fillcolor=fill(c))
            # pure scales (the tables under NEAREST): the step of 0.1 from 0.25, a reduction, a mirror, and EXTENT
            add("transform", big, size=(70, 64), method=AFFINE, data=(0.1, 0, 0.25, 0, 0.1, 0.25), resample=f, fillcolor=fill(c))
            add("transform", big, size=(21, 17), method=AFFINE, data=(2.7, 0, -1.9, 0, 2.3, -0.4), resample=f, fillcolor=fill(c))
            add("transform", small, size=(9, 12), method=AFFINE, data=(-0.8, 0, 6.2, 0, 0.75, 0.1), resample=f, fillcolor=fill(c))
            add("transform", big, size=(31, 23), method=EXTENT, data=(-3.5, 2.25, 49.0, 40.0), resample=f, fillcolor=fill(c))
            # PERSPECTIVE: a mild one, and one whose denominator changes sign inside the output
            add("transform", big, size=(47, 33), method=PERSPECTIVE, data=(1.1, 0.12, -3.0, 0.05, 0.95, 1.5, 0.002, 0.004), resample=f, fillcolor=fill(c))
            add("transform", big, size=(40, 30), method=PERSPECTIVE, data=(0.9, 0.1, 2.0, -0.1, 1.0, 3.0, -0.05, 0.01), resample=f, fillcolor=fill(c))
            # QUAD: a convex one that leaves the source, and one with crossed corners
            add("transform", big, size=(33, 29), method=QUAD, data=(-4.0, 3.0, 2.5, 39.0, 55.5, 30.0, 47.0, -2.0), resample=f, fillcolor=fill(c))
            add("transform", small, size=(17, 15), method=QUAD, data=(5.0, 8.0, 0.5, 0.5, 5.5, 0.0, 0.0, 7.5), resample=f, fillcolor=fill(c))
            # rotate: plain, expanded, about a centre, with a translation, all of them
            add("rotate", big, angle=30.0, resample=f, fillcolor=fill(c))
            add("rotate", big, angle=-7.5, resample=f, expand=True, fillcolor=fill(c))
            add("rotate", small, angle=200, resample=f, expand=True, center=(1.5, 6.0), fillcolor=fill(c))
            add("rotate", big, angle=45, resample=f, translate=(4, -3), fillcolor=fill(c))
            add("rotate", small, angle=123.4, resample=f, expand=True, center=(2, 3), translate=(1.5, 2), fillcolor=fill(c))
            add("rotate", big, angle=90, resample=f, fillcolor=fill(c))                       # not square, not expanded: an AFFINE
            add("rotate", big, angle=180, resample=f, center=(20, 20), fillcolor=fill(c))      # a centre: no fast path
        sq = image(11, 11, c, 2)
        for angle, expand, a in ((0, False, big), (360, True, big), (180, False, big), (-180, True, small), (90, True, big), (270, True, small), (90, False, sq),
                                 (270, False, sq), (450, True, small)):
            add("rotate", a, angle=angle, resample=NEAREST if angle != 90 else BICUBIC, expand=expand, fillcolor=fill(c))
        for m in TRANSPOSE_NAMES:
            add("transpose", big, method=m)
            add("transpose", small, method=m)
    return cases


def model(case, **switches):
    kind, a, kw = case
    kw = dict(kw)
    if kind == "transpose":
        return transpose(a, kw["method"])
    if "premultiply" in kw:
        kw["premultiply_alpha"] = kw.pop("premultiply")
    if "premultiply" in switches:
        kw["premultiply_alpha"] = switches.pop("premultiply")
    return (transform if kind == "transform" else rotate)(a, **kw, **switches)


def pillow(case):
    """live Pillow's answer"""
    from PIL import Image
    kind, a, kw = case
    kw = dict(kw)
    im = Image.fromarray(a)
    if kind == "transpose":
        return np.asarray(im.transpose(getattr(Image.Transpose, kw["method"])))
    kw["resample"] = Image.Resampling(kw["resample"])
    if kind == "rotate":
        return np.asarray(im.rotate(**kw))
    kw["method"] = {AFFINE: Image.Transform.AFFINE, EXTENT: Image.Transform.EXTENT, PERSPECTIVE: Image.Transform.PERSPECTIVE,
                    QUAD: Image.Transform.QUAD}[kw["method"]]
    size, method, data = kw.pop("size"), kw.pop("method"), kw.pop("data")
    return np.asarray(im.transform(size, method, data, **kw))
