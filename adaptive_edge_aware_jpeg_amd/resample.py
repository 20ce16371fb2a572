"""Pillow's ``Image.resize`` for 8-bit RGB and mode-"L" images on the GPU, pixel for pixel: ``resize_many`` takes [H, W, 3] and (with
``mode="L"`` / ``"auto"``) [H, W] images of mixed sizes, in one call, and returns
what ``Image.fromarray(a).resize(size, filter, box=box, reducing_gap=g)`` returns for each, for the five convolution filters
("box", "bilinear", "hamming", "bicubic", "lanczos", or Pillow's integers 4, 2, 5, 3, 1), down- and up-scaling alike, with Pillow's
fractional ``box`` and its ``reducing_gap`` step (``Image.reduce`` over ``Image._get_safe_box`` first).  ``standard_jpeg_thumbnail_many``
(standard_jpeg.py) is ``Image.thumbnail`` on JPEG files built from the scaled decode and this.

The arithmetic is Pillow's (csrc/resample.hip, ``aej_resample_*`` in include/aej.h): per axis a table of int32 taps -- the filter
evaluated on the host, in double, normalised and rounded to 22 fractional bits -- and on the device one horizontal and one vertical
pass, each ``clip((2^21 + sum(pixel * tap)) >> 22, 0, 255)`` with the horizontal result rounded to uint8 in between; ``reduce`` is the
integer cell mean ``((sum + n // 2) * (2^32 // (256 n))) >> 24``.  A one-channel image runs the same plan, tables and arithmetic on its
one channel (Pillow's mode-"L" resize equals one channel of its RGB resize of three copies), through one-channel instantiations of
the three kernels.  One call is at most three kernel launches per channel count present (three for RGB images alone, six for a mix)
and one upload however many images it has, and nothing is read back.

Not built (NotImplementedError): ``nearest`` (Pillow takes another path for it), an image more than 100 times as tall as wide that
is made shorter (Pillow resizes that one vertically first), and modes other than 8-bit RGB and 8-bit L (no RGBA, LA, 16-bit or
float images).  There is no CPU fallback.
"""
import ctypes
import math

import numpy as np

from ._images import gather_u8, image_list, is_int, is_number, one_or_each, packed_views, run_entry
from ._lib import get_context

FILTERS = {"box": 4, "bilinear": 2, "hamming": 5, "bicubic": 3, "lanczos": 1}      # Pillow's Image.Resampling integers
_SUPPORT = {4: 0.5, 2: 1.0, 5: 1.0, 3: 2.0, 1: 3.0}


def _check_filter(resample, what="resample") -> int:
    """one filter -> Pillow's integer.  `what` names the image (or "every image") in a refusal."""
    if isinstance(resample, str):
        if resample == "nearest":
            raise NotImplementedError(f"{what}: resample 'nearest': Pillow takes another path for it, which is not built")
        if resample in FILTERS:
            return FILTERS[resample]
    elif is_int(resample):
        if int(resample) == 0:
            raise NotImplementedError(f"{what}: resample 0 (nearest): Pillow takes another path for it, which is not built")
        if int(resample) in _SUPPORT:
            return int(resample)
    raise ValueError(f"{what}: resample {resample!r}: 'box', 'bilinear', 'hamming', 'bicubic', 'lanczos' or Pillow's 4, 2, 5, 3, 1 required")


def _check_gap(gap, what="reducing_gap"):
    """reducing_gap, which all images of a call share: `what` says so in a refusal ("every image")"""
    if gap is None:
        return None
    if not is_number(gap) or not gap >= 1.0:
        raise ValueError(f"{what}: reducing_gap must be 1.0 or greater (got {gap!r})")
    return float(gap)


def _check_size(size, what, integers=True):
    """one (w, h): positive integers (or, for a thumbnail request, positive numbers whose floor is at least 1)"""
    ok = not isinstance(size, (str, bytes)) and hasattr(size, "__len__") and len(size) == 2 and all(is_number(v) for v in size)
    if ok and integers:
        ok = all(int(v) == v and v >= 1 for v in size)
    elif ok:
        ok = all(math.isfinite(v) and v >= 1 for v in size)
    if not ok:
        raise ValueError(f"{what}: size {size!r}: (width, height), positive {'integers' if integers else 'numbers'} (no bools) required")
    return (int(size[0]), int(size[1])) if integers else (size[0], size[1])


def _per_item(value, n, width, name, what):
    """one value (a sequence of `width` numbers) or a sequence of n such values -> list of n"""
    if value is None:
        return [None] * n
    if isinstance(value, (str, bytes)) or not hasattr(value, "__len__"):
        raise ValueError(f"{name} {value!r}: {width} numbers, or one such entry per {what}, required")
    if len(value) == width and all(is_number(v) or isinstance(v, (bool, np.bool_)) for v in value):
        return [tuple(value)] * n
    if len(value) != n:
        raise ValueError(f"{name}: {len(value)} entries for {n} {what}s")
    return list(value)


def _safe_box(size_img, size, f, box):
    """Image._get_safe_box: the box grown by the pixels the filter may read, clipped to the image"""
    fsup = _SUPPORT[f] - 0.5
    sx, sy = (box[2] - box[0]) / size[0], (box[3] - box[1]) / size[1]
    return (max(0, int(box[0] - fsup * sx)), max(0, int(box[1] - fsup * sy)),
            min(size_img[0], math.ceil(box[2] + fsup * sx)), min(size_img[1], math.ceil(box[3] + fsup * sy)))


def _tap_hull(in_size, in0, in1, out_size, f):
    """(first, end) source indices one axis of a resize reads: the first tap of output 0 to the end of the last output's taps -- the
    window arithmetic of aej_resample_taps_host's bounds (rs_window, csrc/resample.hip: float32 box edges and their float32
    difference, the rest in double) for those two outputs alone, without the tables"""
    a, b = np.float32(in0), np.float32(in1)
    scale = float(b - a) / out_size
    support = _SUPPORT[f] * (1.0 if scale < 1.0 else scale)

    def window(xx):
        center = float(a) + (xx + 0.5) * scale
        lo, hi = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in_size)
        return lo, max(hi - lo, 0)

    first, (lo, cnt) = window(0)[0], window(out_size - 1)
    return first, lo + cnt


def reduce_factors(box, size, gap):
    """the integer factors Image.resize reduces by first under reducing_gap=gap"""
    if gap is None:
        return 1, 1
    return int((box[2] - box[0]) / size[0] / gap) or 1, int((box[3] - box[1]) / size[1] / gap) or 1


def _steps(what, W, H, size, box, f, gap):
    """Image.resize's choices for one W x H image, on the host: -> dict(src=(W, H), dst=size, box, factors, reduce_box) for
    aej_resample_desc.  `what` names the image in a refusal."""
    w, h = size
    whole = (0, 0, W, H)
    if box is None:
        box = whole
    else:
        if len(box) != 4 or not all(is_number(v) and math.isfinite(v) for v in box):
            raise ValueError(f"{what}: box {box!r}: four numbers (x0, y0, x1, y1) required")
        b = [float(np.float32(v)) for v in box]       # as Pillow's C code sees it
        if b[0] < 0 or b[1] < 0:
            raise ValueError(f"{what}: box {tuple(box)!r}: box offset can't be negative")
        if b[2] > W or b[3] > H:
            raise ValueError(f"{what}: box {tuple(box)!r}: box can't exceed original image size ({W} x {H})")
        if not (b[2] - b[0] > 0 and b[3] - b[1] > 0):
            raise ValueError(f"{what}: box {tuple(box)!r}: box can't be empty")
        box = tuple(box)
    step = dict(src=(W, H), dst=(w, h), box=tuple(box), factors=(1, 1), reduce_box=(0, 0, 0, 0))
    if (W, H) == (w, h) and tuple(box) == whole:
        return step
    fx, fy = reduce_factors(box, size, gap)
    if fx > 1 or fy > 1:
        rb = _safe_box((W, H), size, f, box)
        step.update(factors=(fx, fy), reduce_box=rb,
                    box=((box[0] - rb[0]) / fx, (box[1] - rb[1]) / fy, (box[2] - rb[0]) / fx, (box[3] - rb[1]) / fy))
        W, H = -(-(rb[2] - rb[0]) // fx), -(-(rb[3] - rb[1]) // fy)
    if H > W * 100 and h < H:
        raise NotImplementedError(f"{what}: a {W} x {H} image, more than 100 times as tall as wide, made shorter: Pillow resizes it "
                                  "vertically first, which is not built")
    return step


def _run(ctx, src, src_bytes, src_off, steps, f, channels=None, windows=None, packed=False):
    """aej_resample_batch_win over the images at src + src_off[i] -> list of uint8 [h, w, 3] views into one packed allocation.
    f: one filter per image.  channels (None: every image 3): 3 or 1 per image; an image with 1 comes back as [h, w].  windows (int32
    [n, 4] x0, y0, vw, vh; None: none): step i's src is the stored rectangle at (x0, y0) of a virtual vw x vh image in whose
    coordinates its boxes are.  The entry takes NULL channels when every image has 3 and NULL windows when there are none, and is then
    aej_resample_batch_ch / aej_resample_batch (include/aej.h).  packed: -> the packed allocation itself."""
    from ._lib import ResampleDesc
    t, lib, n = ctx.torch, ctx.lib, len(steps)
    descs = (ResampleDesc * n)()
    ch = [3] * n if channels is None else [int(c) for c in channels]
    pos = 0
    dst_off = []
    for i, s in enumerate(steps):
        d = descs[i]
        d.src_offset, d.dst_offset = int(src_off[i]), pos
        (d.src_w, d.src_h), (d.dst_w, d.dst_h) = s["src"], s["dst"]
        d.box = (ctypes.c_float * 4)(*s["box"])
        d.filter = f[i]
        d.reduce_x, d.reduce_y = s["factors"]
        d.reduce_box = (ctypes.c_int32 * 4)(*s["reduce_box"])
        dst_off.append(pos)
        pos += d.dst_w * d.dst_h * ch[i]
    out = ctx.empty((pos,), t.uint8)
    cc = np.array(ch, np.int32) if any(c != 3 for c in ch) else None
    ww = None if windows is None else np.ascontiguousarray(windows, np.int32)
    run_entry(ctx, lib.aej_resample_workspace_bytes_win, lib.aej_resample_batch_win, descs, n, src, src_bytes, out,
              args=(None if cc is None else cc.ctypes.data, None if ww is None else ww.ctypes.data))
    if packed:
        return out
    return packed_views(out, dst_off, [(s["dst"][1], s["dst"][0]) + ((3,) if c == 3 else ()) for s, c in zip(steps, ch)])


def resample_taps(in_size: int, in0: float, in1: float, out_size: int, resample="bicubic"):
    """aej_resample_taps_host (host only): the table of one axis -> (xmin int32 [out_size], count int32 [out_size], taps int32
    [out_size, ksize], zero past each row's count)."""
    from ._lib import load_library
    lib, f = load_library(), _check_filter(resample, "resample_taps")
    k = lib.aej_resample_taps_host(int(in_size), float(in0), float(in1), int(out_size), f, None, None, 0)
    if k < 0:
        raise ValueError(f"taps of {in_size} -> {out_size} over [{in0}, {in1}]: sizes of at least 1 and 0 <= in0 < in1 <= in_size required")
    bounds, taps = np.zeros((out_size, 2), np.int32), np.zeros((out_size, k), np.int32)
    rc = lib.aej_resample_taps_host(int(in_size), float(in0), float(in1), int(out_size), f, bounds.ctypes.data, taps.ctypes.data, taps.size)
    assert rc == k
    return bounds[:, 0].copy(), bounds[:, 1].copy(), taps


def resize_many(images, size, resample="bicubic", box=None, reducing_gap=None, device: int = 0, mode: str = "RGB") -> list:
    """Resize uint8 [H_i, W_i, 3] (RGB) and, with mode=, [H_i, W_i] (mode "L") images (device tensors, host tensors or NumPy arrays, of mixed sizes) on
    the device: -> list of uint8 [h_i, w_i, 3] / [h_i, w_i] tensors -- output i has the rank of input i --, views into one packed
    allocation; element i equals ``np.asarray(Image.fromarray(a_i).resize(size_i, F, box=box_i, reducing_gap=reducing_gap))``.
    mode, as standard_jpeg_encode_many's: "RGB" (the default: the call as it always was, every image [H, W, 3], an [H, W] image refused
    as before); "L": every image [H, W]; "auto": [H, W] and [H, W, 3] images mixed freely in one call.  Other ranks, and a last axis
    other than 3, are refused under every mode; a mode other than the three raises ValueError.
    size: one (w, h), or one per image.  box: None (the whole image), one (x0, y0, x1, y1) -- fractions allowed, as in Pillow -- or
    one (or None) per image.  resample (one, or a list of one per image): "box", "bilinear", "hamming", "bicubic", "lanczos" or Pillow's 4, 2, 5, 3, 1; "nearest" / 0
    raises NotImplementedError.  reducing_gap: None, or a number >= 1.0 (ValueError otherwise): images whose box is more than that
    many times the size are first reduced by whole factors, as Pillow does.  Up-scaling is the same path.  Every argument is checked
    on the host before any device work and a refusal names the image; an image more than 100 times as tall as wide that is made
    shorter raises NotImplementedError."""
    images = image_list(images, "resize_many")
    n = len(images)
    f, gap = one_or_each(resample, n, _check_filter, "resample", "image"), _check_gap(reducing_gap, "every image")
    if not isinstance(mode, str) or mode not in ("RGB", "L", "auto"):
        raise ValueError(f"mode {mode!r}: 'RGB', 'L' or 'auto' required")
    if not isinstance(size, (str, bytes)) and hasattr(size, "__len__") and len(size) == 2 and all(is_number(v) or isinstance(v, (bool, np.bool_)) for v in size):
        sizes = [_check_size(size, "resize_many")] * n
    else:
        if isinstance(size, (str, bytes)) or not hasattr(size, "__len__") or len(size) != n:
            raise ValueError(f"size {size!r}: one (width, height), or one per image ({n}), required")
        sizes = [_check_size(s, f"image {i}") for i, s in enumerate(size)]
    boxes = _per_item(box, n, 4, "box", "image")
    steps, shapes = [], []
    for i, a in enumerate(images):
        shape, dt = tuple(a.shape), str(a.dtype)
        colour, grey = len(shape) == 3 and shape[2] == 3, len(shape) == 2
        if not ((colour and mode != "L") or (grey and mode != "RGB")) or shape[0] < 1 or shape[1] < 1:
            want = {"RGB": "[H, W, 3]", "L": "[H, W] (mode 'L')", "auto": "[H, W] or [H, W, 3] (mode 'auto')"}[mode]
            raise ValueError(f"image {i}: uint8 {want} required, got shape {shape}")
        if dt not in ("uint8", "torch.uint8"):
            raise TypeError(f"image {i}: uint8 required, got {dt}")
        if max(shape[:2]) > 65535 or max(sizes[i]) > 65535:
            raise ValueError(f"image {i}: sizes up to 65535 a side")
        steps.append(_steps(f"image {i}", shape[1], shape[0], sizes[i], boxes[i], f[i], gap))
        shapes.append(shape)
    ctx = get_context(device)
    # the sources: device tensors are read where they are; NumPy arrays and host tensors cross in one pinned copy
    src = gather_u8(ctx, images)              # (held until _run's entry has synchronised)
    base, span, src_off = src.span()
    return _run(ctx, base, span, src_off, steps, f, [3 if len(s) == 3 else 1 for s in shapes])
