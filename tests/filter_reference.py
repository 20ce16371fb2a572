"""NumPy model of Pillow's BoxBlur, GaussianBlur and UnsharpMask on 8-bit images (the arithmetic of libImaging/BoxBlur.c and
UnsharpMask.c), and the case catalogue the filter tests share.  Everything runs per channel: n passes of one extended box blur per
axis, each rounded to uint8, then the integer unsharp epilogue.  float32 steps are np.float32 operations, which round one by one."""
import math

import numpy as np

F32 = np.float32
PASSES = {"BoxBlur": 1, "GaussianBlur": 3, "UnsharpMask": 3}


def gaussian_box(radius):
    """the float32 box radius three box passes stand for a Gaussian of `radius` with (libImaging's _gaussian_blur_radius)"""
    radius = F32(radius)
    sigma2 = F32(F32(radius * radius) / F32(3))
    L = F32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = F32(math.floor((float(L) - 1.0) / 2.0))
    a = F32(F32(F32(2) * l + F32(1)) * F32(F32(l * F32(l + F32(1))) - F32(F32(3) * sigma2)))
    a = F32(a / F32(F32(6) * F32(sigma2 - F32(F32(l + F32(1)) * F32(l + F32(1))))))
    return F32(l + a)


def box_weights(fr):
    """float32 box radius -> (r, ww, fw)"""
    fr = F32(fr)
    r = int(fr)
    ww = int(F32(F32(1 << 24) / F32(fr * F32(2) + F32(1))))
    fw = (((1 << 24) - (2 * r + 1) * ww) & 0xFFFFFFFF) // 2
    return r, ww, fw


def box_pass(a, axis, r, ww, fw):
    """one pass along `axis` of a uint8 array, indices clamped to the line"""
    p = np.moveaxis(a, axis, 0).astype(np.int64)
    n = p.shape[0]
    p = np.concatenate([np.repeat(p[:1], r + 1, 0), p, np.repeat(p[-1:], r + 1, 0)], 0)      # p[j] = line[clamp(j - r - 1)]
    c = np.concatenate([np.zeros_like(p[:1]), np.cumsum(p, 0)], 0)                            # c[m] = sum of p[:m]
    acc = c[2 * r + 2:2 * r + 2 + n] - c[1:1 + n]
    far = p[0:n] + p[2 * r + 2:2 * r + 2 + n]
    out = (acc * ww + far * fw + (1 << 23)) >> 24
    assert out.min() >= 0 and out.max() <= 255
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def radii_of(radius):
    xy = tuple(radius) if isinstance(radius, (tuple, list)) else (radius, radius)
    return F32(xy[0]), F32(xy[1])


def blur(a, boxes, n):
    """n horizontal passes of box radius boxes[0], then n vertical ones of boxes[1]; a zero radius skips its axis"""
    out = a
    for axis, box in ((1, boxes[0]), (0, boxes[1])):
        if box != 0:
            for _ in range(n):
                out = box_pass(out, axis, *box_weights(box))
    return out.copy()


def plan_of(name, radius):
    """-> (passes, (box x, box y)) as float32"""
    xy = radii_of(radius)
    return PASSES[name], (xy if name == "BoxBlur" else (gaussian_box(xy[0]), gaussian_box(xy[1])))


def model(a, f):
    """what Image.fromarray(a).filter(f) gives, for a filter object with .name, .radius (and .percent, .threshold)"""
    a = np.ascontiguousarray(a)
    n, boxes = plan_of(f.name, f.radius)
    out = blur(a, boxes, n)
    if f.name != "UnsharpMask":
        return out
    src, diff = a.astype(np.int64), a.astype(np.int64) - out.astype(np.int64)
    x = diff * int(f.percent)
    sharp = np.clip(src + np.sign(x) * (np.abs(x) // 100), 0, 255)
    return np.where(np.abs(diff) > int(f.threshold), sharp, src).astype(np.uint8)


# ---- the catalogue ------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 5), (16, 17), (33, 64), (64, 65), (40, 130)]
CHANNELS = [1, 2, 3, 4]                      # L, LA, RGB, RGBA
RADII = [0, 0.3, 0.5, 1, 1.5, 2, 2.7, 3, 5, 9.25, 20, 70, 200]
UNSHARP = [(2, 150, 3), (1, 50, 0), (0.5, 500, 10), (3, 1, 0), (2, -50, 3), (2, 150, -1), (2, 150, 300), (3, 100000, 1)]
SWEEP = [k / 97 for k in range(1, 4000)]


class Spec:
    """a filter as plain data: what filter_many and PIL.ImageFilter's classes both read"""

    def __init__(self, name, radius, percent=None, threshold=None):
        self.name, self.radius, self.percent, self.threshold = name, radius, percent, threshold

    def __repr__(self):
        return f"{self.name}({self.radius}" + (f", {self.percent}, {self.threshold})" if self.name == "UnsharpMask" else ")")

    def pil(self):
        from PIL import ImageFilter
        if self.name == "UnsharpMask":
            return ImageFilter.UnsharpMask(self.radius, self.percent, self.threshold)
        return getattr(ImageFilter, self.name)(self.radius)


def image(shape, channels, seed=0):
    """a test image: noise over a ramp, so that blurs move values and the unsharp mask meets both clips"""
    rng = np.random.default_rng(1000 * seed + 17 * shape[0] + shape[1] + channels)
    full = tuple(shape) + ((channels,) if channels > 1 else ())
    a = rng.integers(0, 256, full, dtype=np.uint8)
    a[rng.random(full) < 0.15] = 255
    a[rng.random(full) < 0.15] = 0
    return a


def catalogue():
    """[(image, Spec)]: every shape in every mode with every radius -- as a number for both filters, with 0 on either axis, and in an
    (x, y) pair with another radius -- and with every set of unsharp parameters"""
    cases = []
    for shape in SHAPES:
        for ch in CHANNELS:
            a = image(shape, ch)
            for k, r in enumerate(RADII):
                other = RADII[(k + 5) % len(RADII)]
                cases.append((a, Spec("BoxBlur", r)))
                cases.append((a, Spec("GaussianBlur", r)))
                cases.append((a, Spec("GaussianBlur", (r, 0))))
                cases.append((a, Spec("GaussianBlur", (0, r))))
                cases.append((a, Spec("BoxBlur" if k % 2 else "GaussianBlur", (r, other))))
            for u in UNSHARP:
                cases.append((a, Spec("UnsharpMask", *u)))
    return cases
