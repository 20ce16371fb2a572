"""Pillow's Color3DLUT restated in NumPy, and the catalogue of cases the CPU and GPU tests share.

`prepare` is the float -> INT16 rule of the table (a float32 product, +-0.5 added in double, truncation, two clamps), `apply` the
per-pixel rule: every byte times a 18-bit scale picks a cell and a 15-bit position, and the eight corners are interpolated in int32,
axis 1 (R) first.  test_lut3d_host.py holds both against live Pillow over the whole catalogue; the GPU tests compare with `model`.
"""
import functools

import numpy as np

K = 255 << 6                                   # 16320: table value 1.0
HI, LO = (32767 - 0.5) / K, (-32768 + 0.5) / K  # the clamp thresholds, doubles
SHAPES = [(1, 1), (1, 2), (2, 1), (1, 7), (5, 3), (3, 63), (3, 64), (2, 65), (4, 255), (3, 257), (17, 13)]
RAMP = (256, 256)
SIZES = [2, 3, (2, 3, 65), (65, 2, 3), (3, 65, 2), 16, 17, 33, 65, 20, 21]      # (20 and 21: an even and an odd size between the usual ones)
KINDS = ["identity", "mild", "wild", "constant", "ties", "thresholds"]
COMBOS = [(3, 3, 3), (4, 3, 3), (4, 3, 4), (3, 4, 4), (4, 4, 4)]      # (image channels, table channels, output channels)
MODES = {(3, 3, 3): None, (4, 3, 3): "RGB", (4, 3, 4): None, (3, 4, 4): "RGBA", (4, 4, 4): None}


def size3(size):
    return (size,) * 3 if isinstance(size, int) else tuple(size)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def prepare(table):
    """floats (any dtype, a list) -> INT16, as Pillow reads a table: every item a C float"""
    with np.errstate(over="ignore"):
        t = np.asarray(table, np.float32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (t * np.float32(K)).astype(np.float64)             # the product is rounded to float32
        r = np.trunc(np.where(t < 0, p - 0.5, p + 0.5))
    r = np.where(t.astype(np.float64) >= HI, 32767, np.where(t.astype(np.float64) <= LO, -32768, r))
    return r.astype(np.int16)


def apply(image, size, channels, prepared, channels_out):
    """image uint8 [H, W, 3 or 4]; prepared: INT16 of s3 * s2 * s1 * channels -> uint8 [H, W, channels_out]"""
    s1, s2, s3 = size3(size)
    tab = prepared.reshape(s3 * s2 * s1, channels).astype(np.int64)
    px = image.reshape(-1, image.shape[2]).astype(np.int64)
    idx, shift = [], []
    for d, s in enumerate((s1, s2, s3)):
        scale = int((s - 1) / 255.0 * (1 << 18))
        i = px[:, d] * scale
        idx.append(i >> 18)
        shift.append(((i & 0x3FFFF) >> 3)[:, None])
    base = idx[0] + idx[1] * s1 + idx[2] * s1 * s2

    def lerp(a, b, s):
        return (a * (32768 - s) + b * s) >> 15
    left = lerp(lerp(tab[base], tab[base + 1], shift[0]), lerp(tab[base + s1], tab[base + s1 + 1], shift[0]), shift[1])
    up = base + s1 * s2
    right = lerp(lerp(tab[up], tab[up + 1], shift[0]), lerp(tab[up + s1], tab[up + s1 + 1], shift[0]), shift[1])
    v = np.clip((lerp(left, right, shift[2]) + 32) >> 6, 0, 255)
    if channels_out == 4 and channels == 3:
        v = np.concatenate([v, px[:, 3:4]], axis=1)            # a 3-channel table copies the source's alpha
    assert v.shape[1] == channels_out
    return v.astype(np.uint8).reshape(image.shape[:2] + (channels_out,))


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
class Lut:
    """one table of the catalogue: `size`, `channels`, `mode` (the target mode) and `table`, and the filter objects made from it"""

    def __init__(self, size, kind, channels, mode, table):
        self.size, self.kind, self.channels, self.mode, self.table = size3(size), kind, channels, mode, table
        self.prepared = prepare(table)

    def pil(self):
        from PIL import ImageFilter
        return ImageFilter.Color3DLUT(self.size, self.table, self.channels, self.mode)

    def ours(self, A):
        return A.Color3DLUT(self.size, self.table, self.channels, self.mode)

    def bands(self, channels_in):
        return {None: channels_in, "RGB": 3, "RGBA": 4}[self.mode]

    def __repr__(self):
        return f"Lut({self.size}, {self.kind}, channels={self.channels}, mode={self.mode})"


def _ulp(v, steps):
    v = np.float32(v)
    for _ in range(abs(steps)):
        v = np.nextafter(v, np.float32(np.inf if steps > 0 else -np.inf), dtype=np.float32)
    return v


def table_values(kind, n, seed):
    """n table values of one kind: a float32 array (float64, float16 and a list for some seeds: Pillow reads each as a C float)"""
    rng = np.random.default_rng(seed)
    if kind == "mild":
        t = rng.uniform(-0.3, 1.3, n)
    elif kind == "wild":
        t = rng.uniform(-3, 3, n)                              # both clamps of the table and of the output
    elif kind == "constant":
        t = np.full(n, 0.4321)
    elif kind == "ties":
        t = (rng.integers(-20000, 20000, n) + 0.5) / K         # p +- 0.5 lands on or beside an integer
    elif kind == "thresholds":
        edge = np.array([_ulp(HI, k) for k in (-1, 0, 1)] + [_ulp(LO, k) for k in (-1, 0, 1)] + [np.inf, -np.inf, 0.0, -0.0], np.float32)
        t = np.where(rng.random(n) < 0.5, edge[rng.integers(0, len(edge), n)], rng.uniform(-2.1, 2.1, n).astype(np.float32))
        return t.astype(np.float32)
    else:
        raise KeyError(kind)
    if seed % 4 == 1:
        return t.astype(np.float64)
    if seed % 4 == 2:
        return t.astype(np.float16)
    if seed % 4 == 3 and n <= 20000:
        return [float(v) for v in t]
    return t.astype(np.float32)


@functools.lru_cache(maxsize=None)
def lut(size, kind, channels, mode):
    """the catalogue's table of this size, kind, channels and target mode: one object per key, so that a table used by several cases
    is one object"""
    s1, s2, s3 = size3(size)
    n = s1 * s2 * s3 * channels
    if kind == "identity":                                     # what Color3DLUT.generate makes of the identity: b outermost, r innermost
        g = np.stack(np.meshgrid(np.arange(s3) / (s3 - 1), np.arange(s2) / (s2 - 1), np.arange(s1) / (s1 - 1), indexing="ij")[::-1], axis=-1)
        if channels == 4:
            g = np.concatenate([g, np.full(g.shape[:3] + (1,), 0.5)], axis=-1)
        return Lut(size, kind, channels, mode, g.reshape(-1))
    return Lut(size, kind, channels, mode, table_values(kind, n, seed=n % 1000 + KINDS.index(kind) + (0 if mode is None else 5)))


# ---- images ---------------------------------------------------------------------------------------------------------------------------
def image(shape, channels, seed=0):
    """random bytes with the eight corners of {0, 255}^3 planted where the image has room"""
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + channels + seed)
    a = rng.integers(0, 256, shape + (channels,), dtype=np.uint8)
    flat = a.reshape(-1, channels)
    for k in range(min(8, len(flat))):
        flat[(k * 7) % len(flat), :3] = [255 * (k & 1), 255 * (k >> 1 & 1), 255 * (k >> 2 & 1)]
    return a


@functools.lru_cache(maxsize=None)
def ramp(channels):
    """every (R, G) pair once: R = x, G = y, B = (37 x + 101 y) mod 256; a fourth channel of (x + 3 y) mod 256"""
    y, x = np.mgrid[0:256, 0:256]
    planes = [x, y, (37 * x + 101 * y) % 256] + ([(x + 3 * y) % 256] if channels == 4 else [])
    a = np.stack(planes, axis=-1).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def catalogue():
    """[(image, Lut)]: every shape under every combination, every size class on the ramp, every kind of table under every combination"""
    cases, k = [], 0
    for combo in COMBOS:                                       # (a) the small shapes: sizes and kinds cycle through them
        ci, tc, _ = combo
        for shape in SHAPES:
            cases.append((image(shape, ci, k), lut(SIZES[k % len(SIZES)], KINDS[k % len(KINDS)], tc, MODES[combo])))
            k += 1
    for j, size in enumerate(SIZES):                           # (b) one ramp per size class
        combo = COMBOS[j % len(COMBOS)]
        cases.append((ramp(combo[0]), lut(size, KINDS[1 + j % 2], combo[1], MODES[combo])))
    for kind in KINDS:                                         # (c) every kind of table under every combination, at two sizes
        for combo in COMBOS:
            for size in (5, 17):
                cases.append((image((17, 13), combo[0], len(cases)), lut(size, kind, combo[1], MODES[combo])))
    return cases


def model(image_, lut_):
    return apply(image_, lut_.size, lut_.channels, lut_.prepared, lut_.bands(image_.shape[2]))


def check_catalogue(cases):
    """what the catalogue must hold"""
    assert {a.shape[:2] for a, _ in cases} == set(SHAPES) | {RAMP}
    assert {(a.shape[:2], a.shape[2]) for a, _ in cases} >= {(s, c) for s in SHAPES for c in (3, 4)}
    assert {f.size for _, f in cases} >= {size3(s) for s in SIZES}
    assert {f.size for a, f in cases if a.shape[:2] == RAMP} == {size3(s) for s in SIZES}
    assert {f.kind for _, f in cases} == set(KINDS)
    assert {(a.shape[2], f.channels, f.bands(a.shape[2])) for a, f in cases} == set(COMBOS)
    assert {(f.kind, a.shape[2], f.channels, f.bands(a.shape[2])) for a, f in cases} == {(k,) + c for k in KINDS for c in COMBOS}
