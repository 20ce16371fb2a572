"""Pillow's ``ImageEnhance`` and the point operations of ``ImageOps`` on the GPU, pixel for pixel (csrc/adjust.hip, ``aej_adjust_*``):
``adjust_many`` applies one op, or a chain of up to 8, to each of a list of uint8 images of mixed sizes and one to four channels in one
call; ``histogram_many`` is ``Image.histogram()``; ``adjust_plan`` says, without a device, what the library makes of one chain.

    out  = adjust_many(images, Contrast(1.3))                                  # one op for all images
    out  = adjust_many(images, (Brightness(1.2), Contrast(0.8), Color(1.1)))   # a TUPLE is a chain, applied left to right
    out  = adjust_many(images, [Equalize(), (Solarize(128), Sharpness(2.0))])  # a LIST is one entry (an op or a tuple chain) per image

The ops are small value classes; nothing is refused when one is made, so that ``adjust_many``'s refusal can name the image.

==============================================================  ===========================================  =====================
op                                                              equals in Pillow                             images
==============================================================  ===========================================  =====================
``Brightness(f)``, ``Contrast(f)``, ``Color(f)``, ``Sharpness(f)``  ``ImageEnhance.X(im).enhance(f)``            1 to 4 channels; alpha unchanged
``AutoContrast(cutoff=0, ignore=None, preserve_tone=False)``     ``ImageOps.autocontrast``                    1 and 3 channels
``Equalize()``, ``Posterize(bits)``, ``Solarize(threshold=128)``, ``Invert()``  ``ImageOps.*``                   1 and 3 channels
``Grayscale()``                                                  ``im.convert("L")``; the output is [H, W]    1 to 4 channels
``Point(lut)``                                                   ``im.point(lut)``, 256 * channels ints 0-255  1 to 4 channels
==============================================================  ===========================================  =====================

The arithmetic is Pillow's, restated (include/aej.h has every formula): ``enhance`` is ``Image.blend`` in float32 with the product and
the sum rounded separately; ``autocontrast`` and ``equalize`` restate ``ImageOps.py`` loop for loop in int64 and float64 on the device,
from histograms counted there.  A chain is evaluated per pixel in registers; only a ``Sharpness`` that is not first makes the library
write an intermediate image (to its workspace).

Not built, refused by name with NotImplementedError: ``mask=`` arguments, images of mode "P" and "1", ``ImageOps.colorize``
(``Colorize``) and hue adjustment (``Hue``) as ops of a chain -- ``colorize_many`` and ``hue_many`` (convert.py) are calls of their own."""
import ctypes
import math

import numpy as np

from ._images import (gather_u8, image_shape, intake, is_int, is_number, one_or_each, packed_out, packed_results, packed_shape,
                      refuse_pil_and_bool, run_entry)

MAX_OPS = 8
TABLE_BYTES = 1024
KINDS = ("brightness", "contrast", "color", "sharpness", "autocontrast", "equalize", "lut", "grayscale")      # AEJ_ADJUST_* (include/aej.h)
_MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


class _Op:
    name = None
    kind = None

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in vars(self).items())})"


class _Enhance(_Op):
    def __init__(self, factor):
        self.factor = factor


class Brightness(_Enhance):
    """``ImageEnhance.Brightness(im).enhance(factor)``"""
    name = kind = "brightness"


class Contrast(_Enhance):
    """``ImageEnhance.Contrast(im).enhance(factor)``"""
    name = kind = "contrast"


class Color(_Enhance):
    """``ImageEnhance.Color(im).enhance(factor)``"""
    name = kind = "color"


class Sharpness(_Enhance):
    """``ImageEnhance.Sharpness(im).enhance(factor)``"""
    name = kind = "sharpness"


class AutoContrast(_Op):
    """``ImageOps.autocontrast(im, cutoff, ignore, preserve_tone=preserve_tone)``: cutoff a number or a (low, high) pair, ignore None,
    an int or ints"""
    name = kind = "autocontrast"

    def __init__(self, cutoff=0, ignore=None, preserve_tone=False, mask=None):
        self.cutoff, self.ignore, self.preserve_tone, self.mask = cutoff, ignore, preserve_tone, mask


class Equalize(_Op):
    """``ImageOps.equalize(im)``"""
    name = kind = "equalize"

    def __init__(self, mask=None):
        self.mask = mask


class Posterize(_Op):
    """``ImageOps.posterize(im, bits)``, bits 0 to 8"""
    name, kind = "posterize", "lut"

    def __init__(self, bits):
        self.bits = bits


class Solarize(_Op):
    """``ImageOps.solarize(im, threshold)``"""
    name, kind = "solarize", "lut"

    def __init__(self, threshold=128):
        self.threshold = threshold


class Invert(_Op):
    """``ImageOps.invert(im)``"""
    name, kind = "invert", "lut"


class Grayscale(_Op):
    """``ImageOps.grayscale(im)``, that is ``im.convert("L")``: the output has one channel"""
    name = kind = "grayscale"


class Point(_Op):
    """``im.point(lut)``: exactly 256 * channels ints from 0 to 255, band by band"""
    name, kind = "point", "lut"

    def __init__(self, lut):
        self.lut = lut


class Colorize(_Op):
    """``ImageOps.colorize``: not built as an op of a chain; ``colorize_many`` (convert.py) is the call"""
    name = "colorize"

    def __init__(self, *args, **kwargs):
        pass


class Hue(_Op):
    """hue adjustment (``convert("HSV")``): not built as an op of a chain; ``hue_many`` (convert.py) is the call"""
    name = "hue"

    def __init__(self, *args, **kwargs):
        pass


_ONLY_L_RGB = ("autocontrast", "equalize", "posterize", "solarize", "invert")      # what goes through ImageOps._lut


# ---- argument checks (host only) ---------------------------------------------------------------------------------------------------
def _image(a, who):
    refuse_pil_and_bool(a, who)
    return image_shape(a, who)


def _check_chain(v, who):
    """an op or a tuple of ops -> tuple of ops"""
    chain = v if isinstance(v, tuple) else (v,)
    if len(chain) < 1:
        raise ValueError(f"{who}: an empty chain")
    for op in chain:
        if not isinstance(op, _Op):
            raise TypeError(f"{who}: {op!r}: an op of adjust.py (Brightness, Contrast, ..., Point) or a tuple of them required")
    if len(chain) > MAX_OPS:
        raise ValueError(f"{who}: a chain of {len(chain)} ops: at most {MAX_OPS}")
    return chain


def _lut_of(op, C, who):
    """the 256 * C table entries of a table op on a C-channel image"""
    if op.name == "posterize":
        if not (is_int(op.bits) and 0 <= int(op.bits) <= 8):
            raise ValueError(f"{who}: Posterize: bits {op.bits!r}: an int from 0 to 8 required")
        mask = ~(2 ** (8 - int(op.bits)) - 1)
        return [i & mask for i in range(256)] * C
    if op.name == "solarize":
        if not is_number(op.threshold) or math.isnan(op.threshold):
            raise ValueError(f"{who}: Solarize: threshold {op.threshold!r}: a number required")
        return [i if i < op.threshold else 255 - i for i in range(256)] * C
    if op.name == "invert":
        return list(range(255, -1, -1)) * C
    try:
        lut = list(op.lut)
    except TypeError:
        raise ValueError(f"{who}: Point: a table of {256 * C} ints required") from None
    if len(lut) != 256 * C:
        raise ValueError(f"{who}: Point: a table of {len(lut)} entries: exactly {256 * C} (256 for each of {C} channels)")
    if not all(is_int(x) and 0 <= int(x) <= 255 for x in lut):
        raise ValueError(f"{who}: Point: table entries must be ints from 0 to 255")
    return [int(x) for x in lut]


def _describe(chain, C, who, tables):
    """fill the ops of one image's descriptor: -> (list of AdjustOp fields as dicts, the channels left).  `tables`: dict bytes -> index,
    the call's 1024-byte tables"""
    ops = []
    for op in chain:
        if op.name in ("colorize", "hue"):
            raise NotImplementedError(f"{who}: {type(op).__name__} is not built as an op of adjust_many: {op.name}_many (convert.py) is the call")
        if getattr(op, "mask", None) is not None:
            raise NotImplementedError(f"{who}: {type(op).__name__}: mask= is not built")
        if op.name in _ONLY_L_RGB and C not in (1, 3):
            raise ValueError(f"{who}: {type(op).__name__}: not supported for mode {_MODES[C]} ({C} channels): Pillow's ImageOps takes L and RGB here")
        o = dict(kind=KINDS.index(op.kind), table=0, factor=0.0, preserve_tone=0, cutoff=(0.0, 0.0), ignore=[0] * 8)
        if isinstance(op, _Enhance):
            f = op.factor
            if not is_number(f):
                raise ValueError(f"{who}: {type(op).__name__}: factor {f!r}: a number required")
            with np.errstate(over="ignore"):
                f32 = float(np.float32(f))
            if not math.isfinite(f32):
                raise ValueError(f"{who}: {type(op).__name__}: factor {f!r} is not finite as a float32")
            o["factor"] = f32
        elif op.name == "autocontrast":
            cut = op.cutoff if isinstance(op.cutoff, (tuple, list)) else (op.cutoff, op.cutoff)
            if len(cut) != 2 or not all(is_number(x) and math.isfinite(x) and x >= 0 for x in cut):
                raise ValueError(f"{who}: AutoContrast: cutoff {op.cutoff!r}: a number or a pair of numbers, finite and not negative, required")
            ign = [] if op.ignore is None else list(op.ignore) if isinstance(op.ignore, (tuple, list)) else [op.ignore]
            if not all(is_int(x) and 0 <= int(x) <= 255 for x in ign):
                raise ValueError(f"{who}: AutoContrast: ignore {op.ignore!r}: None, an int or ints from 0 to 255 required")
            for x in ign:
                o["ignore"][int(x) >> 5] |= 1 << (int(x) & 31)
            o["cutoff"] = (float(cut[0]), float(cut[1]))
            o["preserve_tone"] = 1 if op.preserve_tone else 0
        elif op.kind == "lut":
            t = np.zeros(TABLE_BYTES, np.uint8)
            t[:256 * C] = _lut_of(op, C, who)
            o["table"] = tables.setdefault(t.tobytes(), len(tables))
        if op.name == "grayscale":
            C = 1
        ops.append(o)
    return ops, C


def _fill(d, shape, ops):
    from ._lib import AdjustDesc  # noqa: F401
    d.height, d.width, d.channels, d.n_ops = *shape, len(ops)
    for k, o in enumerate(ops):
        p = d.ops[k]
        p.kind, p.table, p.factor, p.preserve_tone = o["kind"], o["table"], o["factor"], o["preserve_tone"]
        p.cutoff[:] = o["cutoff"]
        p.ignore[:] = o["ignore"]


def _each_chain(ops, n):
    """a list is one entry per image; anything else is one value for all"""
    if isinstance(ops, list):
        return one_or_each(ops, n, _check_chain, "ops", "image")
    return [_check_chain(ops, "every image")] * n


def adjust_geometry():
    """aej_adjust_geometry_host (host only): -> dict(chunk, threads, max_grid, table_bytes): the pixels of one image a workgroup of the
    histogram and apply kernels takes at a time, its threads, the largest grid, and the bytes of a table"""
    from ._lib import load_library
    g = (ctypes.c_int32 * 4)()
    load_library().aej_adjust_geometry_host(ctypes.addressof(g))
    return dict(zip(("chunk", "threads", "max_grid", "table_bytes"), (int(v) for v in g)))


def adjust_plan(channels, ops):
    """What the library makes of one chain on a `channels`-channel image, without a device (aej_adjust_plan_host): ->
    dict(segments, passes, launches, out_channels).  segments: the op names, segment by segment -- a segment is evaluated per pixel in
    registers, and a ``Sharpness`` that is not first starts a new one; passes: the histogram passes (one per ``Contrast``,
    ``AutoContrast`` and ``Equalize``); launches: 2 * passes (histogram and tables) + one SMOOTH per ``Sharpness`` + one apply per
    segment.  The refusals are adjust_many's."""
    from ._lib import AdjustDesc, AdjustPlan, load_library
    if not (is_int(channels) and 1 <= channels <= 4):
        raise ValueError(f"adjust_plan: {channels!r} channels: 1 to 4")
    who = "adjust_plan"
    chain = _check_chain(ops, who)
    described, out_c = _describe(chain, int(channels), who, {})
    d, p = AdjustDesc(), AdjustPlan()
    _fill(d, (1, 1, int(channels)), described)
    rc = load_library().aej_adjust_plan_host(ctypes.addressof(d), ctypes.addressof(p))
    if rc:
        raise ValueError(f"{who}: the chain was refused (code {rc})")
    firsts = [int(p.segment_first[k]) for k in range(p.n_segments)] + [len(chain)]
    names = [op.name for op in chain]
    return dict(segments=[names[a:b] for a, b in zip(firsts, firsts[1:])], passes=int(p.n_passes), launches=int(p.n_launches),
                out_channels=int(p.out_channels))


def adjust_many(images, ops, device: int = 0) -> list:
    """Pillow's enhancers and point operations for uint8 [H_i, W_i], [H_i, W_i, 2], [H_i, W_i, 3] and [H_i, W_i, 4] images (Pillow's L,
    LA, RGB and RGBA; device tensors, host tensors or NumPy arrays, of mixed sizes, up to 32767 a side) on the device: -> list of uint8
    device tensors in input order, views into one packed allocation that never alias an input, so that ``standard_jpeg_encode_many``
    and ``png_encode_many`` read them in place; element i equals the ops of its chain applied one after another to
    ``Image.fromarray(a_i)``.  ops: an op for all images, a TUPLE of ops (a chain, applied left to right) for all images, or a LIST
    with one entry -- an op or a tuple chain -- per image.  The module docstring lists the ops.  ``Grayscale`` leaves an [H, W] image
    and the ops after it see one channel.  An input tensor's ``jpeg_comment`` goes to its output.  Everything is checked on the host
    before any device work and a refusal names the image: ValueError for a wrong shape, a side above 32767, a list of another length,
    an empty chain or one of more than 8 ops, a factor whose float32 value is not finite, ``AutoContrast``, ``Equalize``,
    ``Posterize``, ``Solarize`` or ``Invert`` on a 2- or 4-channel image (Pillow raises OSError there; the count is taken after the
    earlier ops of the chain), a ``Point`` table that does not have exactly 256 entries per channel or holds anything but ints 0 to
    255, a cutoff that is negative or not finite, bits outside 0 to 8; TypeError for a dtype other than uint8 and for something that
    is not an op; NotImplementedError for ``mask=``, images of mode "P" and "1", ``Colorize`` and ``Hue``."""
    from ._lib import AdjustDesc, get_context
    images, shapes = intake(images, "adjust_many", _image)
    n = len(images)
    chains = _each_chain(ops, n)
    tables, jobs, seen = {}, [], {}
    for i, (h, w, C) in enumerate(shapes):
        key = (id(chains[i]), C)                              # one chain for all images is described once per channel count
        if key not in seen:
            seen[key] = _describe(chains[i], C, f"image {i}", tables)
        described, out_c = seen[key]
        jobs.append((described, packed_shape(h, w, out_c)))
    ctx = get_context(device)
    src = gather_u8(ctx, images)
    base, span, src_off = src.span()
    out_shapes = [j[1] for j in jobs]
    out, offsets = packed_out(ctx, out_shapes)
    descs = (AdjustDesc * n)()
    filled = {}
    for i, (described, _) in enumerate(jobs):
        key = (id(described), shapes[i][2])
        if key in filled:
            ctypes.memmove(ctypes.addressof(descs[i]), ctypes.addressof(descs[filled[key]]), ctypes.sizeof(AdjustDesc))
            descs[i].height, descs[i].width = shapes[i][:2]
        else:
            _fill(descs[i], shapes[i], described)
            filled[key] = i
        descs[i].src_offset, descs[i].dst_offset = src_off[i], offsets[i]
    blob = b"".join(tables)                                   # (dicts keep insertion order: table k is the k-th key)
    host_tables = (ctypes.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
    run_entry(ctx, ctx.lib.aej_adjust_workspace_bytes, ctx.lib.aej_adjust_batch, descs, n, base, span, out,
              args=(ctypes.addressof(host_tables), len(tables)), query_args=())      # synchronises: src's staging is free again
    return packed_results(out, offsets, out_shapes, images)


def histogram_many(images, device: int = 0) -> list:
    """``Image.histogram()`` for a list of images as adjust_many takes them: -> list of int64 device tensors [channels_i * 256], band
    by band, views into one packed allocation in input order.  Counted on the device as uint32 (32767 x 32767 fits) and widened
    there.  The image checks are adjust_many's."""
    from ._lib import AdjustDesc, get_context
    images, shapes = intake(images, "histogram_many", _image)
    n = len(images)
    ctx = get_context(device)
    src = gather_u8(ctx, images)
    base, span, src_off = src.span()
    out_shapes = [(256 * c,) for _, _, c in shapes]
    out, offsets = packed_out(ctx, out_shapes, ctx.torch.int64)
    descs = (AdjustDesc * n)()
    for i, s in enumerate(shapes):
        _fill(descs[i], s, [])
        descs[i].src_offset, descs[i].dst_offset = src_off[i], offsets[i]
    run_entry(ctx, ctx.lib.aej_adjust_workspace_bytes, ctx.lib.aej_histogram_batch, descs, n, base, span, out)      # synchronises: src's staging is free again
    return packed_results(out, offsets, out_shapes)
