"""Pillow's ``Image.filter`` on the GPU, pixel for pixel -- ``ImageFilter.BoxBlur``, ``GaussianBlur`` and ``UnsharpMask``, and the window
filters ``Kernel`` (with the ten built-ins), ``RankFilter`` / ``MedianFilter`` / ``MinFilter`` / ``MaxFilter`` and ``ModeFilter``:
``filter_many`` takes 8-bit [H, W] (L), [H, W, 2] (LA), [H, W, 3] (RGB) and [H, W, 4] (RGBA) images of mixed sizes, each with its own
filter if wanted, in one call, and returns what ``Image.fromarray(a).filter(F)`` returns for each -- the step between
``standard_jpeg_thumbnail_many`` and ``standard_jpeg_encode_many`` of a preview service.

The arithmetic is Pillow's (csrc/filter.hip, ``aej_filter_*`` in include/aej.h).  The three blurs are one family: n passes of one
extended box blur per axis -- ``(ww * sum(p[x - r .. x + r]) + fw * (p[x - r - 1] + p[x + r + 1]) + 2^23) >> 24`` in uint32, indices
clamped to the line, every pass rounded to uint8 --, horizontal passes first, then an integer epilogue for the unsharp mask.  BoxBlur
is one pass with the radius as given; GaussianBlur three passes with a box radius computed from the Gaussian one in float32 steps
(``filter_plan`` shows it); UnsharpMask is ``in + (in - blur) * percent / 100`` (C division, clipped) where ``|in - blur| >
threshold``.  Channels are filtered independently, as Pillow does: no alpha pre-multiplication.

Two kernel paths, both exact: a fused tile kernel for small radii (the whole filter in LDS, one read and one write of the image), and
one launch per pass for any box radius up to 1024.  One call is one upload however many images it has, and nothing is read back.

The window filters are three more families (csrc/window.hip, ``aej_window_*``), each one kernel that stages a tile and its halo in
LDS: ``Kernel`` -- and the ten built-ins ``SHARPEN``, ``SMOOTH``, ``SMOOTH_MORE``, ``DETAIL``, ``BLUR``, ``CONTOUR``, ``EDGE_ENHANCE``,
``EDGE_ENHANCE_MORE``, ``EMBOSS``, ``FIND_EDGES``, which are Kernels -- is a 3 x 3 or 5 x 5 float32 convolution in exactly Pillow's
order of operations (kernel row 0 meets the row below the sample; samples within r of an edge are copies); ``RankFilter``,
``MedianFilter``, ``MinFilter`` and ``MaxFilter`` pick the rank-th smallest of a window clamped to the image; ``ModeFilter`` takes the
most frequent value of a window clipped to the image if it occurs more than twice.  With them ``filter_many`` takes every
``PIL.ImageFilter`` filter except ``Color3DLUT``, blurs and window filters mixed freely in one call.

Departures from Pillow: a negative radius is refused for all three blurs (Pillow refuses it for BoxBlur only and returns garbage for
the other two); a Kernel scale of 0 -- ``scale=None`` over a zero-sum kernel included -- is refused (Pillow divides by zero and returns
zeros); a mode size below 1 is refused (Pillow accepts it).  Not built (NotImplementedError): a box radius above 1024, ``|percent|``
above 1,000,000, a rank size above 15, a mode size above 7 and a ``|kernel[i] / scale|`` or ``|offset|`` above 2^100.  There is no
CPU fallback.
"""
import ctypes
import math

import numpy as np

from ._images import gather_u8, image_list, image_shape, is_int, is_number, one_or_each, packed_out, packed_results, packed_shape, run_entry

KINDS = {"BoxBlur": 0, "GaussianBlur": 1, "UnsharpMask": 2}      # AEJ_FILTER_*
PATHS = {"auto": 0, "fused": 1, "passes": 2}                     # AEJ_FILTER_AUTO / _FUSED / _PASSES
MAX_BOX_RADIUS = 1024
MAX_PERCENT = 1000000
MAX_RANK_SIZE = 15
MAX_MODE_SIZE = 7
MAX_KERNEL_VALUE = 2.0 ** 100                                    # of |kernel[i] / scale| and |offset|: no partial sum overflows float32


class BoxBlur:
    """``PIL.ImageFilter.BoxBlur``: radius is a number, or an (x, y) pair"""
    name = "BoxBlur"

    def __init__(self, radius):
        self.radius = radius


class GaussianBlur:
    """``PIL.ImageFilter.GaussianBlur``: radius is a number, or an (x, y) pair"""
    name = "GaussianBlur"

    def __init__(self, radius=2):
        self.radius = radius


class UnsharpMask:
    """``PIL.ImageFilter.UnsharpMask``"""
    name = "UnsharpMask"

    def __init__(self, radius=2, percent=150, threshold=3):
        self.radius = radius
        self.percent = percent
        self.threshold = threshold


class Kernel:
    """``PIL.ImageFilter.Kernel``: a 3 x 3 or 5 x 5 convolution; scale None is the sum of the kernel.  Nothing is refused here:
    ``filter_many`` checks the arguments, so that its refusal can name the image."""
    name = "Kernel"

    def __init__(self, size, kernel, scale=None, offset=0):
        if scale is None:
            try:
                scale = sum(kernel)
            except TypeError:
                scale = None                           # not numbers: filter_many says so
        self.filterargs = size, scale, offset, kernel


class _Builtin(Kernel):
    """a built-in of PIL.ImageFilter: a Kernel whose ``filterargs`` are its class's, constructed without arguments"""

    def __init__(self):
        pass


class BLUR(_Builtin):
    name = "Blur"
    filterargs = (5, 5), 16, 0, (1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1)


class CONTOUR(_Builtin):
    name = "Contour"
    filterargs = (3, 3), 1, 255, (-1, -1, -1, -1, 8, -1, -1, -1, -1)


class DETAIL(_Builtin):
    name = "Detail"
    filterargs = (3, 3), 6, 0, (0, -1, 0, -1, 10, -1, 0, -1, 0)


class EDGE_ENHANCE(_Builtin):
    name = "Edge-enhance"
    filterargs = (3, 3), 2, 0, (-1, -1, -1, -1, 10, -1, -1, -1, -1)


class EDGE_ENHANCE_MORE(_Builtin):
    name = "Edge-enhance More"
    filterargs = (3, 3), 1, 0, (-1, -1, -1, -1, 9, -1, -1, -1, -1)


class EMBOSS(_Builtin):
    name = "Emboss"
    filterargs = (3, 3), 1, 128, (-1, 0, 0, 0, 1, 0, 0, 0, 0)


class FIND_EDGES(_Builtin):
    name = "Find Edges"
    filterargs = (3, 3), 1, 0, (-1, -1, -1, -1, 8, -1, -1, -1, -1)


class SHARPEN(_Builtin):
    name = "Sharpen"
    filterargs = (3, 3), 16, 0, (-2, -2, -2, -2, 32, -2, -2, -2, -2)


class SMOOTH(_Builtin):
    name = "Smooth"
    filterargs = (3, 3), 13, 0, (1, 1, 1, 1, 5, 1, 1, 1, 1)


class SMOOTH_MORE(_Builtin):
    name = "Smooth More"
    filterargs = (5, 5), 100, 0, (1, 1, 1, 1, 1, 1, 5, 5, 5, 1, 1, 5, 44, 5, 1, 1, 5, 5, 5, 1, 1, 1, 1, 1, 1)


BUILTINS = ("BLUR", "CONTOUR", "DETAIL", "EDGE_ENHANCE", "EDGE_ENHANCE_MORE", "EMBOSS", "FIND_EDGES", "SHARPEN", "SMOOTH", "SMOOTH_MORE")


class RankFilter:
    """``PIL.ImageFilter.RankFilter``: the rank-th smallest (from 0) of the size x size window, size odd"""
    name = "Rank"

    def __init__(self, size, rank):
        self.size = size
        self.rank = rank


class MedianFilter(RankFilter):
    """``PIL.ImageFilter.MedianFilter``"""
    name = "Median"

    def __init__(self, size=3):
        self.size = size
        self.rank = size * size // 2 if is_int(size) else None


class MinFilter(RankFilter):
    """``PIL.ImageFilter.MinFilter``"""
    name = "Min"

    def __init__(self, size=3):
        self.size = size
        self.rank = 0


class MaxFilter(RankFilter):
    """``PIL.ImageFilter.MaxFilter``"""
    name = "Max"

    def __init__(self, size=3):
        self.size = size
        self.rank = size * size - 1 if is_int(size) else None


class ModeFilter:
    """``PIL.ImageFilter.ModeFilter``: the most frequent value of the window if it occurs more than twice"""
    name = "Mode"

    def __init__(self, size=3):
        self.size = size


def filter_plan(kind, xradius, yradius):
    """aej_filter_plan_host (host only, no device): -> dict(passes, box=(x, y), r=(x, y), ww=(x, y), fw=(x, y)), the passes of a
    filter kind ("BoxBlur", "GaussianBlur", "UnsharpMask") and per axis the float32 box radius and the integer weights of a pass.
    ValueError for a radius that is negative or not finite, NotImplementedError for a box radius above 1024."""
    from ._lib import FilterPlan, load_library
    p = FilterPlan()
    rc = load_library().aej_filter_plan_host(KINDS[kind], float(xradius), float(yradius), ctypes.addressof(p))
    if rc == -5:
        raise NotImplementedError(f"{kind}({xradius}, {yradius}): a box radius above {MAX_BOX_RADIUS}")
    if rc:
        raise ValueError(f"{kind}({xradius}, {yradius}): radii must be finite and not negative")
    return dict(passes=int(p.passes), box=(float(p.box[0]), float(p.box[1])), r=(int(p.r[0]), int(p.r[1])),
                ww=(int(p.ww[0]), int(p.ww[1])), fw=(int(p.fw[0]), int(p.fw[1])))


def filter_geometry():
    """aej_filter_geometry_host (host only): -> dict(tile_w, tile_h, max_halo, row_span, col_band, col_bytes): the fused kernel's tile
    and the largest passes * (r + 1) it takes on an axis, and the spans and bands of the pass kernels."""
    from ._lib import load_library
    g = (ctypes.c_int32 * 6)()
    load_library().aej_filter_geometry_host(ctypes.addressof(g))
    return dict(zip(("tile_w", "tile_h", "max_halo", "row_span", "col_band", "col_bytes"), (int(v) for v in g)))


def window_geometry():
    """aej_window_geometry_host (host only): -> dict(tile_w, tile_h, kernel_halo, rank_halo, mode_halo): the window kernels' tile and
    the largest halo (size // 2) of a Kernel, a rank and a mode filter."""
    from ._lib import load_library
    g = (ctypes.c_int32 * 5)()
    load_library().aej_window_geometry_host(ctypes.addressof(g))
    return dict(zip(("tile_w", "tile_h", "kernel_halo", "rank_halo", "mode_halo"), (int(v) for v in g)))


def _f32(v):
    """a checked number as float32, an overflow quietly infinite"""
    try:
        with np.errstate(over="ignore"):
            return np.float32(v)
    except OverflowError:                              # an int beyond a double
        return np.float32(math.inf if v > 0 else -math.inf)


def _check_kernel(f, what):
    """an object with ``filterargs`` -> ("window", AEJ_WINDOW_KERNEL, k, 0, scale, offset, kernel)"""
    args = f.filterargs
    if not isinstance(args, (tuple, list)) or len(args) != 4:
        raise ValueError(f"{what}: Kernel filterargs {args!r}: (size, scale, offset, kernel) required")
    size, scale, offset, kernel = args
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(is_int(v) for v in size) or tuple(size) not in ((3, 3), (5, 5)):
        raise ValueError(f"{what}: Kernel size {size!r}: (3, 3) or (5, 5) required")
    k = int(size[0])
    try:
        kernel = list(kernel)
    except TypeError:
        raise ValueError(f"{what}: Kernel kernel {kernel!r}: a sequence of {k * k} numbers required") from None
    if len(kernel) != k * k or not all(is_number(v) for v in kernel):
        raise ValueError(f"{what}: Kernel kernel {kernel!r}: a sequence of {k * k} numbers required")
    if scale is None:
        scale = sum(kernel)                            # as Pillow: the sum of the kernel
    if not is_number(scale) or not is_number(offset):
        raise ValueError(f"{what}: Kernel scale {scale!r} and offset {offset!r}: numbers required")
    fs, fo, fk = _f32(scale), _f32(offset), [_f32(v) for v in kernel]
    if not all(np.isfinite(v) for v in [fs, fo] + fk):
        raise ValueError(f"{what}: Kernel values, scale and offset must be finite in float32")
    if fs == 0:
        raise ValueError(f"{what}: Kernel scale {scale!r}: a scale of 0 (scale=None over a zero-sum kernel included) is refused")
    with np.errstate(over="ignore"):
        quot = [v / fs for v in fk]
    if not all(np.isfinite(v) for v in quot):
        raise ValueError(f"{what}: Kernel kernel / scale must be finite in float32")
    if max(abs(float(v)) for v in quot + [fo]) > MAX_KERNEL_VALUE:
        raise NotImplementedError(f"{what}: Kernel |kernel / scale| or |offset| above 2^100 is not built")
    return "window", 0, k, 0, float(fs), float(fo), [float(v) for v in fk]


def _check_size(f, what, kind):
    size = f.size
    if not is_int(size):
        raise TypeError(f"{what}: {kind} size {size!r}: an int required (no bools)")
    return int(size)


def _check_rank(f, what):
    """an object with ``size`` and ``rank`` -> ("window", AEJ_WINDOW_RANK, size, rank, 0, 0, [])"""
    size = _check_size(f, what, "rank filter")
    if not is_int(f.rank):
        raise TypeError(f"{what}: rank filter rank {f.rank!r}: an int required (no bools)")
    rank = int(f.rank)
    if size < 1 or size % 2 == 0:
        raise ValueError(f"{what}: rank filter size {size}: an odd size from 1 on required, as in Pillow")
    if not 0 <= rank < size * size:
        raise ValueError(f"{what}: rank filter rank {rank}: a rank in [0, {size * size}) required, as in Pillow")
    if size > MAX_RANK_SIZE:
        raise NotImplementedError(f"{what}: rank filter size {size}: a size above {MAX_RANK_SIZE} is not built")
    return "window", 1, size, rank, 0.0, 0.0, []


def _check_mode(f, what):
    """an object named "Mode" with ``size`` -> ("window", AEJ_WINDOW_MODE, size, 0, 0, 0, [])"""
    size = _check_size(f, what, "ModeFilter")
    if size < 1:
        raise ValueError(f"{what}: ModeFilter size {size}: a size from 1 on required")
    if size > MAX_MODE_SIZE:
        raise NotImplementedError(f"{what}: ModeFilter size {size}: a size above {MAX_MODE_SIZE} is not built")
    return "window", 2, size, 0, 0.0, 0.0, []


def _halo(plan):
    """the halo the fused kernel needs per axis: passes * (r + 1) where the axis is blurred at all"""
    return tuple(plan["passes"] * (plan["r"][a] + 1) if plan["box"][a] != 0 else 0 for a in (0, 1))


def _check_filter(f, what):
    """one filter object -> (kind, xradius, yradius, percent, threshold, plan) for a blur, ("window", kind, size, rank, scale, offset,
    kernel) for a window filter.  `what` names the image (or "every image") in a refusal.  A class -- ``ImageFilter.SHARPEN`` is one --
    or any other callable is called for its instance; the filters are told by their attributes, as Pillow's own objects carry them."""
    if callable(f):
        try:
            f = f()
        except Exception as e:
            raise ValueError(f"{what}: filter {f!r}: calling it for a filter object failed: {e}") from None
    name = getattr(f, "name", None)
    if hasattr(f, "filterargs"):
        return _check_kernel(f, what)
    if hasattr(f, "size") and hasattr(f, "rank"):
        return _check_rank(f, what)
    if name == "Mode" and hasattr(f, "size"):
        return _check_mode(f, what)
    if not isinstance(name, str) or name not in KINDS or not hasattr(f, "radius"):
        raise ValueError(f"{what}: filter {f!r}: a BoxBlur, GaussianBlur, UnsharpMask, Kernel, rank or mode filter (or an object with its name and "
                         f"parameters) required")
    radius = f.radius
    if name != "UnsharpMask" and isinstance(radius, (tuple, list)):
        if len(radius) != 2 or not all(is_number(v) for v in radius):
            raise ValueError(f"{what}: {name} radius {radius!r}: a number or an (x, y) pair of numbers required")
        xy = (float(radius[0]), float(radius[1]))
    elif is_number(radius):
        xy = (float(radius), float(radius))
    else:
        raise ValueError(f"{what}: {name} radius {radius!r}: a number{'' if name == 'UnsharpMask' else ' or an (x, y) pair of numbers'} required")
    if not all(math.isfinite(v) for v in xy):
        raise ValueError(f"{what}: {name} radius {radius!r}: finite numbers required")
    if min(xy) < 0:
        raise ValueError(f"{what}: {name} radius {radius!r}: radius must be >= 0")
    percent = threshold = 0
    if name == "UnsharpMask":
        percent, threshold = getattr(f, "percent", None), getattr(f, "threshold", None)
        for k, v in (("percent", percent), ("threshold", threshold)):
            if not is_int(v):
                raise TypeError(f"{what}: UnsharpMask {k} {v!r}: an int required (no bools), as in Pillow")
        percent, threshold = int(percent), int(threshold)
        if abs(percent) > MAX_PERCENT:
            raise NotImplementedError(f"{what}: UnsharpMask percent {percent}: |percent| above {MAX_PERCENT} is not built")
        threshold = min(max(threshold, -1), 255)      # below 0 every sample is sharpened, from 255 on none: the same for all such values
    xy = tuple(float(np.float32(v)) for v in xy)      # as Pillow's C code sees them
    if not all(math.isfinite(v) for v in xy):
        raise NotImplementedError(f"{what}: {name} radius {radius!r}: a box radius above {MAX_BOX_RADIUS} is not built")
    try:
        plan = filter_plan(name, xy[0], xy[1])
    except NotImplementedError:
        raise NotImplementedError(f"{what}: {name} radius {radius!r}: a box radius above {MAX_BOX_RADIUS} is not built") from None
    return KINDS[name], xy[0], xy[1], percent, threshold, plan


def filter_many(images, filter, device: int = 0, _path: str = "auto") -> list:
    """Filter uint8 [H_i, W_i], [H_i, W_i, 2], [H_i, W_i, 3] and [H_i, W_i, 4] images (Pillow's L, LA, RGB and RGBA; device tensors,
    host tensors or NumPy arrays, of mixed sizes) on the device: -> list of uint8 device tensors with the shapes of the inputs, views
    into one packed allocation that never alias an input; element i equals ``np.asarray(Image.fromarray(a_i).filter(F_i))``.
    filter: one filter for all images, or a list of one per image, blurs and window filters mixed freely: BoxBlur, GaussianBlur,
    UnsharpMask, Kernel and the ten built-ins (SHARPEN ...), RankFilter, MedianFilter, MinFilter, MaxFilter, ModeFilter.
    ``PIL.ImageFilter``'s own objects are taken as well -- any object with a blur's ``name`` and ``radius`` (``percent``, ``threshold``),
    with ``filterargs``, with ``size`` and ``rank``, or named "Mode" with a ``size`` --, and so is a class or another callable that
    returns one: ``ImageFilter.SHARPEN`` is a class.  An input tensor's ``jpeg_comment`` goes to its output, as Pillow's ``filter``
    keeps ``im.info``.  Every argument is checked on the host before any device work and a refusal names the image: ValueError for a
    wrong shape, a side above 65535, a filter list of another length, an unknown filter, a radius that is negative or not finite, a
    kernel size other than (3, 3) and (5, 5), a kernel of the wrong length or with non-numbers, a kernel value, scale, offset or
    quotient not finite in float32, a scale of 0, a rank size that is even or below 1, a rank outside [0, size^2), a mode size below
    1; TypeError for a dtype other than uint8 and a percent, threshold, size or rank that is not an int; NotImplementedError for a box
    radius above 1024, |percent| above 1,000,000, a rank size above 15, a mode size above 7 and a |kernel / scale| or |offset| above
    2^100.  _path ("auto", "fused", "passes") picks the blurs' kernel path for tests and A/B runs; "fused" raises ValueError for a
    blur beyond its halo; images with a window filter ignore it."""
    from ._lib import FilterDesc, WindowDesc, get_context
    images = image_list(images, "filter_many")
    n = len(images)
    if not isinstance(_path, str) or _path not in PATHS:
        raise ValueError(f"_path {_path!r}: 'auto', 'fused' or 'passes' required")
    filters = one_or_each(filter, n, _check_filter, "filter", "image")
    if _path == "fused":
        limit = filter_geometry()["max_halo"]
        for i, f in enumerate(filters):
            if f[0] != "window" and max(_halo(f[5])) > limit:
                raise ValueError(f"image {i}: _path 'fused': the filter needs a halo of {max(_halo(f[5]))}, the fused kernel takes {limit}")
    shapes = [image_shape(a, f"image {i}", 65535) for i, a in enumerate(images)]      # (after the filters: a call with both wrong names the filter)
    ctx = get_context(device)
    lib = ctx.lib
    # the sources: device tensors are read where they are; NumPy arrays and host tensors cross in one pinned copy
    src = gather_u8(ctx, images)
    base, span, src_off = src.span()
    # one packed output in input order; the blurs' entry and the window filters' entry each write their own images' bytes into it
    window = [f[0] == "window" for f in filters]
    nw = sum(window)
    descs, wdescs = (FilterDesc * max(n - nw, 1))(), (WindowDesc * max(nw, 1))()
    out_shapes = [packed_shape(*s) for s in shapes]
    out, offsets = packed_out(ctx, out_shapes)
    kb, kw = 0, 0
    for i, f in enumerate(filters):
        if window[i]:
            d, kw = wdescs[kw], kw + 1
            d.kind, d.size, d.rank, d.scale, d.offset = f[1:6]
            d.kernel[:len(f[6])] = f[6]
        else:
            d, kb = descs[kb], kb + 1
            d.kind, d.xradius, d.yradius, d.percent, d.threshold = f[:5]
        d.src_offset, d.dst_offset = src_off[i], offsets[i]
        d.height, d.width, d.channels = shapes[i]
    if n > nw:
        run_entry(ctx, lib.aej_filter_workspace_bytes, lib.aej_filter_batch, descs, n - nw, base, span, out, args=(PATHS[_path],))
    if nw:
        run_entry(ctx, lib.aej_window_workspace_bytes, lib.aej_window_batch, wdescs, nw, base, span, out)      # (either synchronises: src's staging is free again)
    return packed_results(out, offsets, out_shapes, images)
