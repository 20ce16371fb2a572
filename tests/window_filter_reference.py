"""NumPy models of Pillow's Kernel (the ten built-ins among them), rank and mode filters on 8-bit images, and the case catalogue the
window-filter tests share.  Everything runs per channel.  float32 steps are np.float32 operations, which round one by one: a Kernel
is a float32 convolution whose order of operations decides the result.  test_window_filter_host.py pins the models to live Pillow."""
import numpy as np

F32 = np.float32


# ---- the three models -----------------------------------------------------------------------------------------------------------
def kernel_args(f):
    """a filter with .filterargs -> (k, q[k * k] float32, ss0 float32)"""
    (kw, kh), scale, offset, kernel = f.filterargs
    assert kw == kh and kw in (3, 5) and len(kernel) == kw * kw
    q = np.array([F32(F32(v) / F32(scale)) for v in kernel], F32)
    return kw, q, F32(F32(offset) + F32(0.5))


def kernel_model(a, f, flip=True, wide=False):
    """Image.filter(Kernel).  flip=False (kernel row 0 meets the row ABOVE) and wide=True (float64 accumulation) are the wrong variants
    the host test shows to differ from Pillow."""
    a = np.ascontiguousarray(a)
    k, q, ss0 = kernel_args(f)
    r, (h, w) = k // 2, a.shape[:2]
    out = a.copy()
    if w < k or h < k:
        return out
    T = np.float64 if wide else F32
    p = a.astype(T)
    ih, iw = h - 2 * r, w - 2 * r
    ss = np.full((ih, iw) + a.shape[2:], T(ss0), T)
    for j in range(k):
        top = 2 * r - j if flip else j                    # the image row of kernel row j, less (y - r)
        row = None
        for i in range(k):
            term = T(q[j * k + i]) * p[top:top + ih, i:i + iw]
            row = term if row is None else row + term
        ss = ss + row
    assert ss.dtype == T and np.isfinite(ss).all()
    res = np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.trunc(np.clip(ss, 0, 255)))).astype(np.uint8)
    out[r:h - r, r:w - r] = res
    return out


def _windows(a, r, mode):
    """[(2r + 1)^2, H, W(, C)] window samples of `a` padded by r in `mode`"""
    h, w = a.shape[:2]
    p = np.pad(a, ((r, r), (r, r)) + ((0, 0),) * (a.ndim - 2), mode=mode)
    return np.stack([p[dy:dy + h, dx:dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1)], 0)


def rank_model(a, f, copy_border=False):
    """Image.filter(RankFilter): window positions clamped to the image.  copy_border=True is the wrong variant (samples within r of an
    edge copied) the host test shows to differ."""
    a = np.ascontiguousarray(a)
    size, rank = int(f.size), int(f.rank)
    assert size % 2 == 1 and 0 <= rank < size * size
    r, (h, w) = size // 2, a.shape[:2]
    out = np.sort(_windows(a, r, "edge"), 0)[rank]
    if copy_border:
        keep = a.copy()
        if h > 2 * r and w > 2 * r:
            keep[r:h - r, r:w - r] = out[r:h - r, r:w - r]
        out = keep
    return np.ascontiguousarray(out)


def mode_model(a, f, clamp=False):
    """Image.filter(ModeFilter): the window clipped to the image; the most frequent value, the smallest on a tie, if it occurs more than
    twice.  clamp=True is the wrong variant (edge replication instead of clipping) the host test shows to differ."""
    a = np.ascontiguousarray(a)
    r = int(f.size) // 2
    win = _windows(a, r, "edge" if clamp else "constant").astype(np.int32)
    valid = _windows(np.ones(a.shape[:2], np.uint8), r, "edge" if clamp else "constant").astype(bool)
    valid = valid.reshape(valid.shape + (1,) * (a.ndim - 2))
    win = np.where(valid, win, -1)                        # -1 never equals a voter
    count = np.zeros(win.shape, np.int32)
    for j in range(win.shape[0]):
        count += (win == win[j]) & (win[j] >= 0)
    key = np.where(win >= 0, count * 256 + (255 - win), -1)      # most votes first, then the smaller value
    best = key.max(0)
    return np.where(best // 256 > 2, 255 - best % 256, a).astype(np.uint8)


def model(a, f):
    """what Image.fromarray(a).filter(f) gives for a Kernel, rank or mode filter object (ours, PIL.ImageFilter's or a Spec)"""
    if hasattr(f, "filterargs"):
        return kernel_model(a, f)
    if hasattr(f, "rank"):
        return rank_model(a, f)
    assert f.name == "Mode"
    return mode_model(a, f)


# ---- filters as plain data ------------------------------------------------------------------------------------------------------
class Spec:
    """a filter as plain data: what filter_many and PIL.ImageFilter's classes both carry"""

    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def __repr__(self):
        return f"{self.name}({', '.join(f'{k}={v!r}' for k, v in vars(self).items() if k != 'name')})"

    def pil(self):
        from PIL import ImageFilter
        if hasattr(self, "filterargs"):
            size, scale, offset, kernel = self.filterargs
            return ImageFilter.Kernel(size, kernel, scale, offset)
        if hasattr(self, "rank"):
            return ImageFilter.RankFilter(self.size, self.rank)
        return ImageFilter.ModeFilter(self.size)

    def ours(self, A):
        if hasattr(self, "filterargs"):
            size, scale, offset, kernel = self.filterargs
            return A.Kernel(size, kernel, scale, offset)
        if hasattr(self, "rank"):
            return A.RankFilter(self.size, self.rank)
        return A.ModeFilter(self.size)


def Kernel(k, kernel, scale=None, offset=0):
    kernel = [float(v) if isinstance(v, (float, np.floating)) else int(v) for v in kernel]
    return Spec("Kernel", filterargs=((k, k), sum(kernel) if scale is None else scale, offset, kernel))


def Rank(size, rank):
    return Spec("Rank", size=size, rank=rank)


def Mode(size):
    return Spec("Mode", size=size)


def delta(k, at):
    kernel = [0] * (k * k)
    kernel[at] = 1
    return Kernel(k, kernel)


BUILTIN_NAMES = ["SHARPEN", "SMOOTH", "SMOOTH_MORE", "DETAIL", "BLUR", "CONTOUR", "EDGE_ENHANCE", "EDGE_ENHANCE_MORE", "EMBOSS", "FIND_EDGES"]


def builtins():
    """the ten built-ins as Specs, the numbers read from PIL.ImageFilter"""
    from PIL import ImageFilter
    return [Spec(getattr(ImageFilter, n).name, filterargs=getattr(ImageFilter, n).filterargs) for n in BUILTIN_NAMES]


def kernel_filters():
    rng = np.random.default_rng(7)
    out = builtins()
    out += [Kernel(3, [1, 2, 1, 2, 4, 2, 1, 2, 1]), Kernel(3, [-1, 0, 2, 3, -2, 1, 0, 4, -3], 3, 10),
            Kernel(5, list(range(-5, 20)), 7, -30), Kernel(5, [(i * 7) % 11 - 3 for i in range(25)])]
    out += [Kernel(3, rng.standard_normal(9), 0.731, 3.25), Kernel(3, rng.standard_normal(9), -1.37, 140.6),
            Kernel(5, rng.standard_normal(25), 2.913, -7.75), Kernel(5, rng.standard_normal(25), -0.377, 99.125),
            Kernel(5, rng.standard_normal(25))]
    out += [delta(3, 4), delta(5, 12)] + [delta(3, at) for at in (0, 2, 6, 8)] + [delta(5, at) for at in (0, 4, 20, 24)]
    out += [Kernel(3, [-1] * 9, 1, 0), Kernel(5, [-2] * 25, 3, 100), Kernel(3, [0, 0, 0, 0, 10, 0, 0, 0, 0], 1), Kernel(5, [2] * 25, 5, -60)]
    return out


RANK_SIZES = [1, 3, 5, 7, 9, 15]
MODE_SIZES = [1, 2, 3, 4, 5, 7]


def rank_filters():
    out = []
    for s in RANK_SIZES:
        n = s * s
        for rank in sorted({0, min(1, n - 1), n // 3, n // 2, max(n - 2, 0), n - 1}):
            out.append(Rank(s, rank))
    return out


def mode_filters():
    return [Mode(s) for s in MODE_SIZES]


# ---- the catalogue --------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 6), (2, 7), (3, 3), (2, 3), (3, 2), (4, 5), (5, 5), (5, 4), (6, 5), (16, 17), (33, 64), (40, 130)]
CHANNELS = [1, 2, 3, 4]                      # L, LA, RGB, RGBA


def image(shape, channels, seed=0, levels=256):
    """256-level noise, or (levels=8) its eight-level quantisation, which gives the ties and majorities that decide modes"""
    rng = np.random.default_rng(1000 * seed + 17 * shape[0] + shape[1] + channels)
    a = rng.integers(0, 256, tuple(shape) + ((channels,) if channels > 1 else ()), dtype=np.uint8)
    return a if levels == 256 else (a // (256 // levels) * (256 // levels)).astype(np.uint8)


SMOOTH_MORE_CASE = (40, 64)                  # the noise image on which a float64-accumulating SMOOTH_MORE differs from Pillow


def catalogue():
    """[(image, Spec)]: every filter on every shape.  Mode filters see both images of every channel count; Kernel and rank filters
    see every shape with the channel count and the image (noise / eight levels) rotating with the filter, so that each filter meets
    each channel count and both images over the shapes.  Then SMOOTH_MORE on the 40 x 64 noise image."""
    cases = []
    filters = kernel_filters() + rank_filters()
    for si, shape in enumerate(SHAPES):
        images = {(ch, lv): image(shape, ch, levels=lv) for ch in CHANNELS for lv in (256, 8)}
        for fi, f in enumerate(filters):
            cases.append((images[CHANNELS[(fi + si) % 4], (256, 8)[(fi // 4 + si) % 2]], f))
        for f in mode_filters():
            for ch in CHANNELS:
                for lv in (256, 8):
                    cases.append((images[ch, lv], f))
    cases.append((image(SMOOTH_MORE_CASE, 1), builtins()[2]))
    return cases


def check_catalogue(cases, want):
    """the assertions on the models' own outputs: both clips occur, some mode sample is replaced and some kept, and some mode tie
    between two values is decided"""
    clip0 = clip255 = replaced = kept = tie = False
    for (a, f), w in zip(cases, want):
        if hasattr(f, "filterargs"):
            k, q, ss0 = kernel_args(f)
            r = k // 2
            if a.shape[0] >= k and a.shape[1] >= k:
                inner, src = w[r:-r, r:-r], a[r:-r, r:-r]
                clip0 = clip0 or bool(((inner == 0) & (src != 0)).any())
                clip255 = clip255 or bool(((inner == 255) & (src != 255)).any())
        elif f.name == "Mode":
            replaced = replaced or bool((w != a).any())
            kept = kept or (int(f.size) > 1 and bool((w == a).any()))
            if not tie and int(f.size) == 3 and a.ndim == 2 and a.shape[0] >= 3 and a.shape[1] >= 3:
                tie = _has_tie(a, w)
    assert clip0 and clip255, "both clips of a Kernel"
    assert replaced and kept, "a mode sample replaced and one kept"
    assert tie, "a mode tie between two values decided for the smaller"


def _has_tie(a, w):
    """some interior sample of a 3 x 3 mode whose two most frequent values have the same count above 2, the smaller one chosen"""
    for y in range(1, a.shape[0] - 1):
        for x in range(1, a.shape[1] - 1):
            v, c = np.unique(a[y - 1:y + 2, x - 1:x + 2], return_counts=True)
            top = v[c == c.max()]
            if c.max() > 2 and len(top) > 1 and w[y, x] == top.min():
                return True
    return False
