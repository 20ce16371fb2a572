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
most frequent value of a window clipped to the image if it occurs more than twice.

``Color3DLUT`` is the one filter that works on a pixel, not on its neighbourhood (csrc/lut3d.hip, ``aej_lut3d_*``): the R, G and B
bytes of an [H, W, 3] or [H, W, 4] image are the coordinates in a table of size 2 .. 65 per axis and 3 or 4 channels, whose eight
entries around the point are interpolated in integers (include/aej.h has the rule); the output has the channels of the filter's
``target_mode`` where it names one, else the input's.  The floats of a table become INT16 once per call and distinct table object
(``aej_lut3d_prepare_host``).  With it ``filter_many`` takes every ``PIL.ImageFilter`` filter, blurs, window filters and tables mixed
freely in one call.

Departures from Pillow: a negative radius is refused for all three blurs (Pillow refuses it for BoxBlur only and returns garbage for
the other two); a Kernel scale of 0 -- ``scale=None`` over a zero-sum kernel included -- is refused (Pillow divides by zero and returns
zeros); a mode size below 1 is refused (Pillow accepts it).  Not built (NotImplementedError): a box radius above 1024, ``|percent|``
above 1,000,000, a rank size above 15, a mode size above 7 and a ``|kernel[i] / scale|`` or ``|offset|`` above 2^100.  A table with a
NaN is refused (Pillow's result for one is undefined).  There is no CPU fallback.
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
MODE_BANDS = {"RGB": 3, "YCbCr": 3, "HSV": 3, "LAB": 3, "RGBA": 4, "RGBX": 4, "CMYK": 4, "RGBa": 4}      # the 8-bit modes a Color3DLUT may target


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


class Color3DLUT:
    """``PIL.ImageFilter.Color3DLUT``: a table of ``channels`` (3 or 4) values per point of a size[0] x size[1] x size[2] grid over the
    colour cube (2 .. 65 points an axis), the first axis -- R -- changing fastest; 0.0 is the lowest output value, 1.0 the highest.
    table: ``channels * size**3`` numbers, or ``size**3`` tuples of ``channels``, or a NumPy array of shape (n * channels,),
    (n, channels) or (size[2], size[1], size[0], channels).  target_mode: the mode of the result where it differs from the image's
    (``filter_many`` reads its number of bands).  The checks and their messages are Pillow's."""
    name = "Color 3D LUT"

    def __init__(self, size, table, channels=3, target_mode=None, _copy_table=True):
        if channels not in (3, 4):
            raise ValueError("Only 3 or 4 output channels are supported")
        self.size = size = self._check_size(size)
        self.channels = channels
        self.mode = target_mode
        items = size[0] * size[1] * size[2]
        wrong_size = False
        if isinstance(table, np.ndarray):
            if table.shape in ((items * channels,), (items, channels), (size[2], size[1], size[0], channels)):
                table = (table.copy() if _copy_table else table).reshape(items * channels)
            else:
                wrong_size = True
        else:
            if _copy_table:
                table = list(table)
            if table and isinstance(table[0], (list, tuple)):
                flat = []
                for pixel in table:
                    if len(pixel) != channels:
                        raise ValueError(f"The elements of the table should have a length of {channels}.")
                    flat.extend(pixel)
                table = flat
        if wrong_size or len(table) != items * channels:
            raise ValueError("The table should have either channels * size**3 float items or size**3 items of channels-sized tuples with floats. "
                             f"Table should be: {channels}x{size[0]}x{size[1]}x{size[2]}. Actual length: {len(table)}")
        self.table = table

    @staticmethod
    def _check_size(size):
        try:
            _, _, _ = size
        except ValueError as e:
            raise ValueError("Size should be either an integer or a tuple of three integers.") from e
        except TypeError:
            size = (size, size, size)
        size = tuple(int(x) for x in size)
        if not all(2 <= s <= 65 for s in size):
            raise ValueError("Size should be in [2, 65] range.")
        return size

    @classmethod
    def generate(cls, size, callback, channels=3, target_mode=None):
        """the table of ``callback(r, g, b)`` -> ``channels`` values at every grid point, the coordinates from 0.0 to 1.0; b is the
        outermost loop, r the innermost"""
        s1, s2, s3 = cls._check_size(size)
        if channels not in (3, 4):
            raise ValueError("Only 3 or 4 output channels are supported")
        table = [0] * (s1 * s2 * s3 * channels)
        at = 0
        for b in range(s3):
            for g in range(s2):
                for r in range(s1):
                    table[at:at + channels] = callback(r / (s1 - 1), g / (s2 - 1), b / (s3 - 1))
                    at += channels
        return cls((s1, s2, s3), table, channels=channels, target_mode=target_mode, _copy_table=False)

    def transform(self, callback, with_normals=False, channels=None, target_mode=None):
        """a new table of ``callback(*values)`` -- ``callback(r, g, b, *values)`` with_normals -- at every grid point; channels: those
        of the new table where they change"""
        if channels not in (None, 3, 4):
            raise ValueError("Only 3 or 4 output channels are supported")
        ch_in, ch_out = self.channels, channels or self.channels
        s1, s2, s3 = self.size
        table = [0] * (s1 * s2 * s3 * ch_out)
        at_in = at_out = 0
        for b in range(s3):
            for g in range(s2):
                for r in range(s1):
                    values = self.table[at_in:at_in + ch_in]
                    values = callback(r / (s1 - 1), g / (s2 - 1), b / (s3 - 1), *values) if with_normals else callback(*values)
                    table[at_out:at_out + ch_out] = values
                    at_in += ch_in
                    at_out += ch_out
        return type(self)(self.size, table, channels=ch_out, target_mode=target_mode or self.mode, _copy_table=False)

    def __repr__(self):
        mode = f" target_mode={self.mode}" if self.mode else ""
        return "<{} from {} size={:d}x{:d}x{:d} channels={:d}{}>".format(type(self).__name__, type(self.table).__name__, *self.size, self.channels, mode)


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


def lut3d_geometry():
    """aej_lut3d_geometry_host (host only): -> dict(threads, run, tile): the lanes of a workgroup, the adjacent pixels a lane takes at
    a time and the pixels of a workgroup."""
    from ._lib import load_library
    g = (ctypes.c_int32 * 3)()
    load_library().aej_lut3d_geometry_host(ctypes.addressof(g))
    return dict(zip(("threads", "run", "tile"), (int(v) for v in g)))


def _check_lut(f, what, cache=None):
    """an object with ``table``, ``channels`` and ``size`` -> ("lut", size, channels, bands of its target mode or None, its table as
    INT16).  cache: {id(object): (object, result)} of one call, so that an object given for many images is prepared once and is one
    table of the call."""
    if cache is not None and id(f) in cache:
        return cache[id(f)][1]
    from ._lib import load_library
    channels, size, mode = f.channels, f.size, getattr(f, "mode", None)
    if not is_int(channels) or channels not in (3, 4):
        raise ValueError(f"{what}: Color3DLUT channels {channels!r}: 3 or 4 required")
    if is_int(size):
        size = (size,) * 3
    if not isinstance(size, (tuple, list)) or len(size) != 3 or not all(is_int(v) and 2 <= v <= 65 for v in size):
        raise ValueError(f"{what}: Color3DLUT size {size!r}: an int or three ints in [2, 65] required")
    size = tuple(int(v) for v in size)
    if mode is not None and (not isinstance(mode, str) or mode not in MODE_BANDS):
        raise ValueError(f"{what}: Color3DLUT target mode {mode!r}: one of {', '.join(MODE_BANDS)} (8-bit, 3 or 4 bands) or None required")
    try:
        table = np.asarray(f.table)
        if table.dtype.kind not in "fiub":
            raise TypeError
        with np.errstate(over="ignore"):
            table = np.ascontiguousarray(table, np.float32).reshape(-1)      # as Pillow reads every item: a C float
    except (TypeError, ValueError):
        raise TypeError(f"{what}: Color3DLUT table: numbers required") from None
    items = size[0] * size[1] * size[2] * int(channels)
    if table.size != items:
        raise ValueError(f"{what}: Color3DLUT table of {table.size} values: {channels}x{size[0]}x{size[1]}x{size[2]} = {items} required")
    if np.isnan(table).any():
        raise ValueError(f"{what}: Color3DLUT table holds a NaN")
    prepared = np.empty(items, np.int16)
    if load_library().aej_lut3d_prepare_host(table.ctypes.data, items, prepared.ctypes.data):
        raise ValueError(f"{what}: Color3DLUT table refused")
    res = ("lut", size, int(channels), None if mode is None else MODE_BANDS[mode], prepared)
    if cache is not None:
        cache[id(f)] = (f, res)                        # (holds the object: its id stays its own for the call)
    return res


def _lut_channels_out(channels_in, lut, who):
    """Pillow's rule by bands alone: the output has the bands of the target mode, else the source's"""
    _, _, tc, bands, _ = lut
    if channels_in not in (3, 4):
        raise ValueError(f"{who}: Color3DLUT takes [H, W, 3] and [H, W, 4] images, got {channels_in} channel{'s' if channels_in > 1 else ''} "
                         f"(Pillow: image has wrong mode)")
    co = bands or channels_in
    if tc == 4 and co == 3:
        raise ValueError(f"{who}: Color3DLUT with a 4-channel table needs a 4-band result, the {'target mode' if bands else 'image'} has 3 (as Pillow)")
    if co == 4 and tc == 3 and channels_in == 3:
        raise ValueError(f"{who}: Color3DLUT with a 3-channel table on a 3-channel image cannot fill a 4-band target mode (as Pillow)")
    return co


def lut3d_plan(channels_in, lut):
    """What ``filter_many`` does with a Color3DLUT on an image of channels_in channels (host only, no device): -> (channels of the
    output, bytes of the table as staged on the device -- 8 an entry --, the kernel path: "global", the only one, which reads the
    table through the caches).  The refusals are ``filter_many``'s, naming "the image"."""
    res = _check_lut(lut, "the image")
    co = _lut_channels_out(channels_in, res, "the image")
    return co, 8 * res[1][0] * res[1][1] * res[1][2], "global"


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


def _check_filter(f, what, luts=None):
    """one filter object -> (kind, xradius, yradius, percent, threshold, plan) for a blur, ("window", kind, size, rank, scale, offset,
    kernel) for a window filter, ("lut", ...) for a Color3DLUT (_check_lut, with its cache `luts`).  `what` names the image (or "every
    image") in a refusal.  A class -- ``ImageFilter.SHARPEN`` is one -- or any other callable is called for its instance; the filters
    are told by their attributes, as Pillow's own objects carry them."""
    if callable(f):
        try:
            f = f()
        except Exception as e:
            raise ValueError(f"{what}: filter {f!r}: calling it for a filter object failed: {e}") from None
    if hasattr(f, "table") and hasattr(f, "channels") and hasattr(f, "size"):
        return _check_lut(f, what, luts)
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
    host tensors or NumPy arrays, of mixed sizes) on the device: -> list of uint8 device tensors with the shapes of the inputs -- but
    for an image under a Color3DLUT whose target mode has another number of bands, which is [H_i, W_i, bands] --, views into one
    packed allocation that never alias an input; element i equals ``np.asarray(Image.fromarray(a_i).filter(F_i))``.
    filter: one filter for all images, or a list of one per image, blurs, window filters and tables mixed freely: BoxBlur,
    GaussianBlur, UnsharpMask, Kernel and the ten built-ins (SHARPEN ...), RankFilter, MedianFilter, MinFilter, MaxFilter, ModeFilter,
    Color3DLUT.  ``PIL.ImageFilter``'s own objects are taken as well -- any object with ``table``, ``channels`` and ``size`` (and
    ``mode``), with a blur's ``name`` and ``radius`` (``percent``, ``threshold``), with ``filterargs``, with ``size`` and ``rank``, or
    named "Mode" with a ``size`` --, and so is a class or another callable that returns one: ``ImageFilter.SHARPEN`` is a class.  A
    Color3DLUT takes [H, W, 3] and [H, W, 4] images; its output has the bands of its target mode (RGB, YCbCr, HSV, LAB: 3; RGBA, RGBX,
    CMYK, RGBa: 4), else the input's: a 3-channel table drops the alpha of a 4-channel image for a 3-band target and copies it
    otherwise, a 4-channel table writes all four bytes.  One table object given for many images is prepared and uploaded once.
    An input tensor's ``jpeg_comment`` goes to its output, as Pillow's ``filter`` keeps ``im.info``.  Every argument is checked on the
    host before any device work and a refusal names the image: ValueError for a wrong shape, a side above 65535, a filter list of
    another length, an unknown filter, a radius that is negative or not finite, a kernel size other than (3, 3) and (5, 5), a kernel
    of the wrong length or with non-numbers, a kernel value, scale, offset or quotient not finite in float32, a scale of 0, a rank
    size that is even or below 1, a rank outside [0, size^2), a mode size below 1, a table size outside [2, 65], table channels other
    than 3 and 4, a table of the wrong length or with a NaN, a target mode that is not one of the eight, an image of 1 or 2 channels
    under a table, a 4-channel table for a 3-band result, a 3-channel table on a 3-channel image for a 4-band result; TypeError for a
    dtype other than uint8, a percent, threshold, size or rank that is not an int and a table with non-numbers; NotImplementedError
    for a box radius above 1024, |percent| above 1,000,000, a rank size above 15, a mode size above 7 and a |kernel / scale| or
    |offset| above 2^100.  _path ("auto", "fused", "passes") picks the blurs' kernel path for tests and A/B runs; "fused" raises
    ValueError for a blur beyond its halo; images with a window filter or a table ignore it."""
    from ._lib import FilterDesc, Lut3dDesc, WindowDesc, get_context
    images = image_list(images, "filter_many")
    n = len(images)
    if not isinstance(_path, str) or _path not in PATHS:
        raise ValueError(f"_path {_path!r}: 'auto', 'fused' or 'passes' required")
    luts = {}
    filters = one_or_each(filter, n, lambda f, what: _check_filter(f, what, luts), "filter", "image")
    if _path == "fused":
        limit = filter_geometry()["max_halo"]
        for i, f in enumerate(filters):
            if f[0] not in ("window", "lut") and max(_halo(f[5])) > limit:
                raise ValueError(f"image {i}: _path 'fused': the filter needs a halo of {max(_halo(f[5]))}, the fused kernel takes {limit}")
    shapes = [image_shape(a, f"image {i}", 65535) for i, a in enumerate(images)]      # (after the filters: a call with both wrong names the filter)
    out_shapes = [packed_shape(h, w, _lut_channels_out(c, f, f"image {i}") if f[0] == "lut" else c) for i, ((h, w, c), f) in enumerate(zip(shapes, filters))]
    ctx = get_context(device)
    lib = ctx.lib
    # the sources: device tensors are read where they are; NumPy arrays and host tensors cross in one pinned copy
    src = gather_u8(ctx, images)
    base, span, src_off = src.span()
    # one packed output in input order; the blurs' entry, the window filters' entry and the tables' entry each write their own images' bytes into it
    nw, nl = sum(f[0] == "window" for f in filters), sum(f[0] == "lut" for f in filters)
    descs, wdescs, ldescs = (FilterDesc * max(n - nw - nl, 1))(), (WindowDesc * max(nw, 1))(), (Lut3dDesc * max(nl, 1))()
    out, offsets = packed_out(ctx, out_shapes)
    kb, kw, kl = 0, 0, 0
    tables = {}                                        # the call's distinct tables by identity: id -> (index, INT16 array)
    for i, f in enumerate(filters):
        if f[0] == "lut":
            d, kl = ldescs[kl], kl + 1
            d.size[:], d.table_channels, d.channels_out = f[1], f[2], out_shapes[i][2]
            d.table = tables.setdefault(id(f[4]), (len(tables), f[4]))[0]
            d.src_offset, d.dst_offset = src_off[i], offsets[i]
            d.height, d.width, d.channels_in = shapes[i]
            continue
        if f[0] == "window":
            d, kw = wdescs[kw], kw + 1
            d.kind, d.size, d.rank, d.scale, d.offset = f[1:6]
            d.kernel[:len(f[6])] = f[6]
        else:
            d, kb = descs[kb], kb + 1
            d.kind, d.xradius, d.yradius, d.percent, d.threshold = f[:5]
        d.src_offset, d.dst_offset = src_off[i], offsets[i]
        d.height, d.width, d.channels = shapes[i]
    if n > nw + nl:
        run_entry(ctx, lib.aej_filter_workspace_bytes, lib.aej_filter_batch, descs, n - nw - nl, base, span, out, args=(PATHS[_path],))
    if nw:
        run_entry(ctx, lib.aej_window_workspace_bytes, lib.aej_window_batch, wdescs, nw, base, span, out)      # (each synchronises: src's staging is free again)
    if nl:
        flat = [t for _, t in tables.values()]
        table_offsets = np.cumsum([0] + [t.size for t in flat], dtype=np.int64)
        every = np.ascontiguousarray(np.concatenate(flat) if len(flat) > 1 else flat[0])
        run_entry(ctx, lib.aej_lut3d_workspace_bytes, lib.aej_lut3d_batch, ldescs, nl, base, span, out,
                  args=(every.ctypes.data, table_offsets.ctypes.data, len(flat)), query_args=())
    return packed_results(out, offsets, out_shapes, images)
