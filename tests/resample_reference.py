"""An independent NumPy model of Pillow's 8-bit resampling (resize_many, standard_jpeg_thumbnail_many): Image.resize for the five
convolution filters, Image.reduce, resize's reducing_gap step and Image.thumbnail on a JPEG file.  Written from the arithmetic, not
from the library's C++:

    xmin, n, taps = taps_for(in_size, in0, in1, out_size, filter)     # per output index: first source index, tap count, int32 taps
    out = resize(a, (w, h), filter, box=None, reducing_gap=None)      # uint8 [H][W][C] -> uint8 [h][w][C]
    out = reduce(a, (fx, fy), box=None)
    plan = thumbnail_plan(W, H, size, reducing_gap)                   # (scale, (fx, fy), final_size, box) or None
    out = thumbnail(data, size, filter, reducing_gap)                 # a JPEG file's bytes -> what Image.thumbnail leaves

  * the box crosses into Pillow's C code as four float32; scale = double(in1 - in0) / out_size with the subtraction in float32;
    everything after that is double.  support = filter support * max(scale, 1); per output index xx: center = in0 + (xx + 0.5) * scale,
    xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in_size) - xmin,
    k[x] = filter((x + xmin - center + 0.5) / max(scale, 1)), normalised by their sum in index order (when it is not 0), then
    int(k * 2^22 +- 0.5) truncated.
  * one pass: clip((2^21 + sum(pixel * tap)) >> 22, 0, 255), int32; horizontal first, rounded to uint8, then vertical.
  * reduce: ((sum + n // 2) * (2^32 // (256 * n))) >> 24 in uint32, n the source pixels really in the cell.

Filters by Pillow's integer: 4 box, 2 bilinear, 5 hamming, 3 bicubic, 1 lanczos."""
import math

import numpy as np

FILTERS = {"box": 4, "bilinear": 2, "hamming": 5, "bicubic": 3, "lanczos": 1}
SUPPORT = {4: 0.5, 2: 1.0, 5: 1.0, 3: 2.0, 1: 3.0}
PRECISION_BITS = 22


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


KERNEL = {4: _box, 2: _bilinear, 5: _hamming, 3: _bicubic, 1: _lanczos}


def filter_id(f):
    return FILTERS[f] if isinstance(f, str) else int(f)


def taps_for(in_size, in0, in1, out_size, filt):
    """-> (xmin [out_size], n [out_size], taps: list of int lists)"""
    f = filter_id(filt)
    in0, in1 = np.float32(in0), np.float32(in1)
    scale = float(np.float32(in1 - in0)) / out_size
    in0 = float(in0)
    fs = max(scale, 1.0)
    support = SUPPORT[f] * fs
    kern = KERNEL[f]
    xmins, ns, taps = [], [], []
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [kern((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        taps.append([int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in k])
        xmins.append(xmin)
        ns.append(max(xmax, 0))
    return np.array(xmins, np.int64), np.array(ns, np.int64), taps


def one_pass(a, axis, xmin, n, taps):
    """the pass along `axis` (0 vertical, 1 horizontal) of uint8 [H][W][C]"""
    a = np.moveaxis(np.asarray(a, np.int64), axis, 0)
    out = np.empty((len(xmin),) + a.shape[1:], np.int64)
    for i in range(len(xmin)):
        t = np.array(taps[i][:n[i]], np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (a[xmin[i]:xmin[i] + n[i]] * t).sum(0)
        assert np.abs(acc).max(initial=0) < 2 ** 31
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def reduce(a, factors, box=None):
    a = np.asarray(a)
    fx, fy = factors
    H, W = a.shape[:2]
    x0, y0, x1, y1 = box if box is not None else (0, 0, W, H)
    a = a[y0:y1, x0:x1].astype(np.uint64)
    h, w = a.shape[:2]
    oh, ow = -(-h // fy), -(-w // fx)
    out = np.empty((oh, ow) + a.shape[2:], np.uint8)
    for y in range(oh):
        for x in range(ow):
            cell = a[y * fy:(y + 1) * fy, x * fx:(x + 1) * fx]
            n = cell.shape[0] * cell.shape[1]
            s = cell.reshape((n,) + a.shape[2:]).sum(0)
            v = ((s + n // 2) * ((1 << 32) // (256 * n))) & 0xFFFFFFFF
            out[y, x] = v >> 24
    return out


def safe_box(size_img, size, filt, box):
    """Image._get_safe_box for an image of size_img (w, h)"""
    fsup = SUPPORT[filter_id(filt)] - 0.5
    sx, sy = (box[2] - box[0]) / size[0], (box[3] - box[1]) / size[1]
    return (max(0, int(box[0] - fsup * sx)), max(0, int(box[1] - fsup * sy)),
            min(size_img[0], math.ceil(box[2] + fsup * sx)), min(size_img[1], math.ceil(box[3] + fsup * sy)))


def reduce_factors(box, size, gap):
    if gap is None:
        return 1, 1
    return int((box[2] - box[0]) / size[0] / gap) or 1, int((box[3] - box[1]) / size[1] / gap) or 1


def resize(a, size, filt="bicubic", box=None, reducing_gap=None):
    a = np.asarray(a)
    f = filter_id(filt)
    H, W = a.shape[:2]
    w, h = size
    if box is None:
        box = (0, 0, W, H)
    if (W, H) == (w, h) and tuple(box) == (0, 0, W, H):
        return a.copy()
    fx, fy = reduce_factors(box, size, reducing_gap)
    if fx > 1 or fy > 1:
        rb = safe_box((W, H), size, f, box)
        a = reduce(a, (fx, fy), rb)
        box = ((box[0] - rb[0]) / fx, (box[1] - rb[1]) / fy, (box[2] - rb[0]) / fx, (box[3] - rb[1]) / fy)
        H, W = a.shape[:2]
    if H > W * 100 and h < H:
        raise NotImplementedError("tall image: Pillow resizes vertically first")
    b = [float(np.float32(v)) for v in box]
    need_h = w != W or b[0] != 0 or b[2] != w
    need_v = h != H or b[1] != 0 or b[3] != h
    if need_v:
        ymin, yn, ytaps = taps_for(H, box[1], box[3], h, f)
        first, last = int(ymin[0]), int(ymin[-1] + yn[-1])
    if need_h:
        xmin, xn, xtaps = taps_for(W, box[0], box[2], w, f)
        if need_v:
            a = a[first:last]
            ymin = ymin - first
        a = one_pass(a, 1, xmin, xn, xtaps)
    if need_v:
        a = one_pass(a, 0, ymin, yn, ytaps)
    return a.copy() if not (need_h or need_v) else a


def thumbnail_size(W, H, size):
    """Image.thumbnail's preserve_aspect_ratio: the final (w, h), or None when the request covers the image"""
    x, y = math.floor(size[0]), math.floor(size[1])
    if x >= W and y >= H:
        return None

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = W / H
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def draft_scale(W, H, size):
    if size[0] < 1 or size[1] < 1:
        return 1
    ratio = min(W // size[0], H // size[1])
    return next((s for s in (8, 4, 2) if s <= ratio), 1)


def thumbnail_plan(W, H, size, reducing_gap=2.0):
    final = thumbnail_size(W, H, size)
    if final is None:
        return None
    s = 1 if reducing_gap is None else draft_scale(W, H, (int(size[0] * reducing_gap), int(size[1] * reducing_gap)))
    box = (0, 0, W / s, H / s)
    dw, dh = -(-W // s), -(-H // s)
    if (dw, dh) == final:
        return s, (1, 1), final, box
    return s, reduce_factors(box, final, reducing_gap), final, box


def thumbnail(data, size, filt="bicubic", reducing_gap=2.0):
    import progressive_reference as P
    import scaled_decode_reference as R
    frame, _ = P.walk(bytes(data))
    plan = thumbnail_plan(frame["width"], frame["height"], size, reducing_gap)
    if plan is None:
        return R.decode(data, 1)
    s, _, final, box = plan
    a = R.decode(data, s)
    if (a.shape[1], a.shape[0]) == final:
        return a
    return resize(a, final, filt, box=box, reducing_gap=reducing_gap)
