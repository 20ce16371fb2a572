"""NumPy model of Pillow's ImageEnhance (Brightness, Contrast, Color, Sharpness), ImageOps (autocontrast, equalize, posterize, solarize,
invert, grayscale), Image.point and Image.histogram for uint8 images of 1 to 4 channels (L, LA, RGB, RGBA), and the catalogue of cases
the host and GPU tests share.  Nothing here calls PIL: test_adjust_host.py pins the model to live Pillow, the GPU tests pin the library
to the model.

An op is a tuple: ("brightness", f), ("contrast", f), ("color", f), ("sharpness", f), ("autocontrast", cutoff, ignore, preserve_tone),
("equalize",), ("posterize", bits), ("solarize", threshold), ("invert",), ("grayscale",), ("point", lut).  A chain is a tuple of ops.
A case is (image, chain).

The wrong variants (keyword switches of `model`), each of which test_adjust_host.py shows to differ from Pillow on the catalogue:
fma (product and sum rounded once), f64 (the factor kept in float64), round_l (L as the rounded float sum 0.299 r + 0.587 g + 0.114 b),
mean_floor (Contrast's mean without + 0.5), eq_all_bins (equalize's step over all bins), alpha_zero (the degenerate's alpha 0 instead
of the image's own), sharp_border (Sharpness filters the border with replicated edges)."""
import numpy as np

ENHANCERS = ("brightness", "contrast", "color", "sharpness")
LUT_OPS = ("autocontrast", "equalize", "posterize", "solarize", "invert")
STATISTICS = ("contrast", "autocontrast", "equalize")


# ---- pieces ----------------------------------------------------------------------------------------------------------------------------
def _bands(a):
    return a[..., None] if a.ndim == 2 else a


def luma(a, round_l=False):
    """L of [H, W, C]: band 0 for 1 and 2 channels, else (r 19595 + g 38470 + b 7471 + 0x8000) >> 16"""
    if a.shape[2] < 3:
        return a[..., 0].copy()
    r, g, b = (a[..., k].astype(np.int64) for k in range(3))
    if round_l:
        return np.rint(0.299 * r + 0.587 * g + 0.114 * b).astype(np.uint8)
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, s, f, fma=False, f64=False):
    """Image.blend(d, s, f): float32 throughout, the product and the sum rounded separately"""
    diff = s.astype(np.int32) - d.astype(np.int32)
    a = np.float32(f)
    if f64:
        t = d.astype(np.float64) + float(f) * diff
        inside = 0 <= float(f) <= 1
    elif fma:
        t = (d.astype(np.float64) + np.float64(a) * diff).astype(np.float32)       # exact in float64, rounded once
        inside = 0 <= a <= 1
    else:
        t = d.astype(np.float32) + a * diff.astype(np.float32)
        inside = 0 <= a <= 1
    if inside:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def smooth(a, border=False):
    """filter(SMOOTH) of [H, W, C]: the 3 x 3 kernel (1 1 1, 1 5 1, 1 1 1) / 13 in float32, a row's products added left to right and
    the row's sum added to 0.5; samples within 1 of an edge are copies"""
    H, W, C = a.shape
    q = [np.float32(v) / np.float32(13) for v in (1, 1, 1, 1, 5, 1, 1, 1, 1)]
    p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge").astype(np.float32)
    ss = np.full((H, W, C), np.float32(0.5), np.float32)
    for j in range(3):
        rows = p[2 - j:2 - j + H]                              # kernel row 0 meets the image row below the sample
        rs = q[3 * j] * rows[:, 0:W]
        rs = rs + q[3 * j + 1] * rows[:, 1:W + 1]
        rs = rs + q[3 * j + 2] * rows[:, 2:W + 2]
        ss = ss + rs
    out = np.where(ss <= 0, 0, np.where(ss >= 255, 255, ss.astype(np.int32))).astype(np.uint8)
    if not border:
        keep = np.ones((H, W), bool)
        keep[1:H - 1, 1:W - 1] = False
        out[keep] = a[keep]
    return out


def histogram(a):
    """Image.histogram(): channels * 256 counts, band by band"""
    a = _bands(a)
    return np.concatenate([np.bincount(a[..., c].reshape(-1), minlength=256) for c in range(a.shape[2])]).astype(np.int64)


def _py_floordiv(vx, wx):
    return vx // wx                                            # Python's own: float64 floor division for floats, exact for ints


def autocontrast_lut(h, cutoff, ignore):
    """one band of ImageOps.autocontrast, loop for loop: 256 ints -> 256 ints"""
    h = [int(v) for v in h]
    if ignore is not None:
        for ix in ([ignore] if isinstance(ignore, (int, np.integer)) else ignore):
            h[ix] = 0
    if cutoff:
        if not isinstance(cutoff, tuple):
            cutoff = (cutoff, cutoff)
        n = sum(h)
        cut = int(_py_floordiv(n * cutoff[0], 100))
        for lo in range(256):
            if cut > h[lo]:
                cut = cut - h[lo]
                h[lo] = 0
            else:
                h[lo] -= cut
                cut = 0
            if cut <= 0:
                break
        cut = int(_py_floordiv(n * cutoff[1], 100))
        for hi in range(255, -1, -1):
            if cut > h[hi]:
                cut = cut - h[hi]
                h[hi] = 0
            else:
                h[hi] -= cut
                cut = 0
            if cut <= 0:
                break
    for lo in range(256):
        if h[lo]:
            break
    for hi in range(255, -1, -1):
        if h[hi]:
            break
    if hi <= lo:
        return list(range(256))
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(max(int(ix * scale + offset), 0), 255) for ix in range(256)]


def equalize_lut(h, all_bins=False):
    h = [int(v) for v in h]
    histo = [v for v in h if v]
    if len(histo) <= 1:
        return list(range(256))
    step = (sum(histo) - (h[-1] if all_bins else histo[-1])) // 255
    if not step:
        return list(range(256))
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))                        # Image.point clips a table entry to 8 bits
        n = n + h[i]
    return lut


def posterize_lut(bits):
    mask = ~(2 ** (8 - bits) - 1)
    return [i & mask for i in range(256)]


def solarize_lut(threshold):
    return [i if i < threshold else 255 - i for i in range(256)]


def _point(a, lut):
    """[H, W, C] through C tables of 256"""
    t = np.asarray(lut, np.int64).astype(np.uint8).reshape(-1, 256)
    return np.stack([t[c][a[..., c]] for c in range(a.shape[2])], axis=2)


# ---- one op ------------------------------------------------------------------------------------------------------------------------------
def apply_op(a, op, fma=False, f64=False, round_l=False, mean_floor=False, eq_all_bins=False, alpha_zero=False, sharp_border=False):
    """[H, W, C] uint8 -> [H, W, C'] uint8"""
    kind, C = op[0], a.shape[2]
    if kind in LUT_OPS and C not in (1, 3):
        raise ValueError(f"{kind}: not supported for {C} channels")
    if kind in ENHANCERS:
        f = op[1]
        nc = C - (C in (2, 4))                                  # colour bands
        if kind == "brightness":
            d = np.zeros_like(a)
        elif kind == "color":
            d = np.repeat(luma(a, round_l)[..., None], C, axis=2)
        elif kind == "contrast":
            h = np.bincount(luma(a, round_l).reshape(-1), minlength=256)
            mean = float(sum(i * int(h[i]) for i in range(256))) / (a.shape[0] * a.shape[1])
            d = np.full_like(a, int(mean) if mean_floor else int(mean + 0.5))
        else:
            d = smooth(a, sharp_border)
        if nc < C:
            d[..., nc] = 0 if alpha_zero else a[..., nc]
        return blend(d, a, f, fma, f64)
    if kind == "autocontrast":
        _, cutoff, ignore, tone = op
        if tone:
            lut = autocontrast_lut(np.bincount(luma(a, round_l).reshape(-1), minlength=256), cutoff, ignore) * C
        else:
            lut = sum((autocontrast_lut(np.bincount(a[..., c].reshape(-1), minlength=256), cutoff, ignore) for c in range(C)), [])
        return _point(a, lut)
    if kind == "equalize":
        return _point(a, sum((equalize_lut(np.bincount(a[..., c].reshape(-1), minlength=256), eq_all_bins) for c in range(C)), []))
    if kind == "posterize":
        return _point(a, posterize_lut(op[1]) * C)
    if kind == "solarize":
        return _point(a, solarize_lut(op[1]) * C)
    if kind == "invert":
        return _point(a, list(range(255, -1, -1)) * C)
    if kind == "grayscale":
        return luma(a, round_l)[..., None]
    if kind == "point":
        if len(op[1]) != 256 * C:
            raise ValueError("point: wrong table size")
        return _point(a, op[1])
    raise ValueError(f"unknown op {kind!r}")


def chain_of(ops):
    """an op or a tuple chain -> tuple of ops"""
    return (ops,) if isinstance(ops[0], str) else tuple(ops)


def model(case, **switch):
    """(image, op or chain) -> uint8 array, [H, W] for one channel"""
    a = _bands(case[0])
    for op in chain_of(case[1]):
        a = apply_op(a, op, **switch)
    return np.ascontiguousarray(a[..., 0] if a.shape[2] == 1 else a)


def channels_after(C, ops):
    """the channel count a chain leaves, or raise for an op that cannot take its image"""
    for op in chain_of(ops):
        if op[0] in LUT_OPS and C not in (1, 3):
            raise ValueError(op[0])
        if op[0] == "grayscale":
            C = 1
    return C


def plan_of(C, ops):
    """what adjust_plan must report: the segments (lists of op names), the histogram passes and the launches of one chain.  A
    Sharpness that is not first starts a new segment; each statistics op costs a histogram and a table launch; each Sharpness a
    SMOOTH launch; each segment an apply launch"""
    segments, passes, smooths = [[]], 0, 0
    for k, op in enumerate(chain_of(ops)):
        if op[0] == "sharpness":
            smooths += 1
            if k:
                segments.append([])
        passes += op[0] in STATISTICS
        segments[-1].append(op[0])
    return dict(segments=segments, passes=passes, launches=2 * passes + smooths + len(segments))


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 4), (16, 16), (16, 17), (67, 35))
FACTORS = (0, 1 / 3, 0.5, 1, 1.1, 1.9, 3.0, -0.3)


def image(h, w, c, seed=0):
    """random uint8 [h, w] or [h, w, c]; an alpha band holds 0, 255 and values between"""
    rng = np.random.default_rng(1000 * seed + 100 * c + 7 * h + w)
    a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if c in (2, 4) and h * w >= 4:
        al = a[..., -1].reshape(-1)
        al[0], al[1], al[2] = 0, 255, 128
    return a[..., 0].copy() if c == 1 else a


def _natural(h, w, c, seed):
    """smooth gradients plus noise: a histogram with empty ends, so that the cut-offs and Equalize have something to do"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 40 + 150 * (x + 2 * y) / max(1, w + 2 * h)
    a = np.stack([np.clip(base + 10 * k + rng.normal(0, 12, (h, w)), 0, 255) for k in range(c)], axis=2).astype(np.uint8)
    return a[..., 0].copy() if c == 1 else a


def point_table(c, seed=5):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 256, 256 * c)]


JITTER = (("brightness", 1.2), ("contrast", 0.8), ("color", 1.1), ("sharpness", 1.5))
CHAINS = (
    JITTER,
    (JITTER[3], JITTER[2], JITTER[1], JITTER[0]),
    (("contrast", 1.3), ("equalize",)),
    (("sharpness", 2.0), ("invert",)),
    (("solarize", 128), ("sharpness", 0.5), ("posterize", 4)),
    (("autocontrast", 5, None, False), ("sharpness", 1.9)),
    (("grayscale",), ("equalize",)),
    (("color", 0.5), ("grayscale",), ("autocontrast", 0, None, False), ("sharpness", 3.0)),
    (("brightness", 1.1), ("contrast", 1.9), ("sharpness", -0.3), ("equalize",), ("color", 1 / 3), ("sharpness", 3.0), ("autocontrast", (2, 10), 0, True), ("invert",)),
)


def catalogue():
    """-> [(image, op or chain)]; images up to 67 x 35"""
    cases, k = [], 0

    def add(op, channels, shapes=None, n=3):
        nonlocal k
        for c in channels:
            for s in (shapes or [SHAPES[(k + j * 4) % len(SHAPES)] for j in range(n)]):
                k += 1
                cases.append((image(s[0], s[1], c, k), op))

    for f in FACTORS:
        add(("brightness", f), (1, 2, 3, 4))
        add(("contrast", f), (1, 2, 3, 4))
        add(("color", f), (1, 2, 3, 4))
        add(("sharpness", f), (1, 2, 3, 4), SHAPES if f in (0, 1.9) else None)
    for cutoff in (0, 5, (2, 10), 49.9, 60):
        for ignore in (None, 0, (0, 255)):
            for tone in (False, True):
                op = ("autocontrast", cutoff, ignore, tone)
                add(op, (1, 3), n=2)
                for c in (1, 3):
                    cases.append((_natural(16, 17, c, len(cases)), op))
    flat = ("autocontrast", 0, None, False)
    for c in (1, 3):
        cases.append((np.full((5, 4, c), 77, np.uint8).reshape((5, 4) if c == 1 else (5, 4, 3)), flat))
        cases.append(((100 + image(16, 17, c, 3) % 4).astype(np.uint8), flat))
        cases.append(((100 + image(16, 17, c, 4) % 4).astype(np.uint8), ("autocontrast", 5, None, True)))
        cases.append((np.full((16, 17, c), 9, np.uint8).reshape((16, 17) if c == 1 else (16, 17, 3)), ("equalize",)))
        cases.append((_natural(67, 35, c, 11), ("equalize",)))
        cases.append((np.minimum(_natural(67, 35, c, 13), 150), ("equalize",)))      # a full last non-zero bin, bin 255 empty
        cases.append((_natural(67, 35, c, 12), ("contrast", 1.9)))
    add(("equalize",), (1, 3), SHAPES)
    for bits in (0, 1, 4, 8):
        add(("posterize", bits), (1, 3), n=2)
    for t in (0, 128, 100.5, 256):
        add(("solarize", t), (1, 3), n=2)
    add(("invert",), (1, 3))
    add(("grayscale",), (1, 2, 3, 4))
    for c in (1, 2, 3, 4):
        add(("point", point_table(c)), (c,))
    for ch in CHAINS:
        needs = [c for c in (1, 2, 3, 4) if _fits(c, ch)]
        add(ch, needs, [(16, 17), (67, 35), (3, 3)])
    return cases


def _fits(c, ops):
    try:
        channels_after(c, ops)
        return True
    except ValueError:
        return False


# ---- the same ops for the library and for the tests' Pillow side ---------------------------------------------------------------------
def library_ops(A, ops):
    """a model op or chain as the package's: an op stays an op, a chain becomes a tuple (A: the imported package)"""
    def one(op):
        k = op[0]
        if k in ENHANCERS:
            return getattr(A, k.capitalize())(op[1])
        if k == "autocontrast":
            return A.AutoContrast(op[1], op[2], op[3])
        if k in ("posterize", "solarize", "point"):
            return getattr(A, k.capitalize())(op[1])
        return {"equalize": A.Equalize, "invert": A.Invert, "grayscale": A.Grayscale}[k]()
    return one(ops) if isinstance(ops[0], str) else tuple(one(op) for op in ops)
