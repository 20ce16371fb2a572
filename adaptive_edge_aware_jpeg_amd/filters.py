"""Pillow's ``Image.filter`` with ``ImageFilter.BoxBlur``, ``GaussianBlur`` and ``UnsharpMask`` on the GPU, pixel for pixel:
``filter_many`` takes 8-bit [H, W] (L), [H, W, 2] (LA), [H, W, 3] (RGB) and [H, W, 4] (RGBA) images of mixed sizes, each with its own
filter if wanted, in one call, and returns what ``Image.fromarray(a).filter(F)`` returns for each -- the step between
``standard_jpeg_thumbnail_many`` and ``standard_jpeg_encode_many`` of a preview service.

The arithmetic is Pillow's (csrc/filter.hip, ``aej_filter_*`` in include/aej.h).  The three filters are one family: n passes of one
extended box blur per axis -- ``(ww * sum(p[x - r .. x + r]) + fw * (p[x - r - 1] + p[x + r + 1]) + 2^23) >> 24`` in uint32, indices
clamped to the line, every pass rounded to uint8 --, horizontal passes first, then an integer epilogue for the unsharp mask.  BoxBlur
is one pass with the radius as given; GaussianBlur three passes with a box radius computed from the Gaussian one in float32 steps
(``filter_plan`` shows it); UnsharpMask is ``in + (in - blur) * percent / 100`` (C division, clipped) where ``|in - blur| >
threshold``.  Channels are filtered independently, as Pillow does: no alpha pre-multiplication.

Two kernel paths, both exact: a fused tile kernel for small radii (the whole filter in LDS, one read and one write of the image), and
one launch per pass for any box radius up to 1024.  One call is one upload however many images it has, and nothing is read back.

Departure from Pillow: a negative radius is refused for all three filters (Pillow refuses it for BoxBlur only and returns garbage for
the other two).  Not built (NotImplementedError): a box radius above 1024 and ``|percent|`` above 1,000,000.  There is no CPU fallback.
"""
import ctypes
import math

import numpy as np

from ._images import gather_u8, is_int, is_number, one_or_each, packed_views

KINDS = {"BoxBlur": 0, "GaussianBlur": 1, "UnsharpMask": 2}      # AEJ_FILTER_*
PATHS = {"auto": 0, "fused": 1, "passes": 2}                     # AEJ_FILTER_AUTO / _FUSED / _PASSES
MAX_BOX_RADIUS = 1024
MAX_PERCENT = 1000000


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


def _halo(plan):
    """the halo the fused kernel needs per axis: passes * (r + 1) where the axis is blurred at all"""
    return tuple(plan["passes"] * (plan["r"][a] + 1) if plan["box"][a] != 0 else 0 for a in (0, 1))


def _check_filter(f, what):
    """one filter object -> (kind, xradius, yradius, percent, threshold, plan).  `what` names the image (or "every image") in a refusal."""
    name = getattr(f, "name", None)
    if not isinstance(name, str) or name not in KINDS or not hasattr(f, "radius"):
        raise ValueError(f"{what}: filter {f!r}: a BoxBlur, GaussianBlur or UnsharpMask (or an object with that name and its parameters) required")
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
    filter: one BoxBlur, GaussianBlur or UnsharpMask for all images, or a list of one per image; ``PIL.ImageFilter``'s own instances
    are taken as well (any object with that ``name`` and ``radius``, ``percent``, ``threshold``).  An input tensor's ``jpeg_comment``
    goes to its output, as Pillow's ``filter`` keeps ``im.info``.  Every argument is checked on the host before any device work and a
    refusal names the image: ValueError for a wrong shape, a side above 65535, a filter list of another length, an unknown filter, a
    radius that is negative or not finite; TypeError for a dtype other than uint8 and a percent or threshold that is not an int;
    NotImplementedError for a box radius above 1024 and |percent| above 1,000,000.  _path ("auto", "fused", "passes") picks the kernel
    path for tests and A/B runs; "fused" raises ValueError for a filter beyond its halo."""
    from ._lib import FilterDesc, get_context
    images = list(images)
    n = len(images)
    if n < 1:
        raise ValueError("filter_many needs at least one image")
    if not isinstance(_path, str) or _path not in PATHS:
        raise ValueError(f"_path {_path!r}: 'auto', 'fused' or 'passes' required")
    filters = one_or_each(filter, n, _check_filter, "filter", "image")
    if _path == "fused":
        limit = filter_geometry()["max_halo"]
        for i, f in enumerate(filters):
            if max(_halo(f[5])) > limit:
                raise ValueError(f"image {i}: _path 'fused': the filter needs a halo of {max(_halo(f[5]))}, the fused kernel takes {limit}")
    shapes = []
    for i, a in enumerate(images):
        shape, dt = tuple(getattr(a, "shape", ())), str(getattr(a, "dtype", None))
        if not (len(shape) == 2 or (len(shape) == 3 and shape[2] in (2, 3, 4))) or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"image {i}: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape {shape}")
        if dt not in ("uint8", "torch.uint8"):
            raise TypeError(f"image {i}: uint8 required, got {dt}")
        if max(shape[:2]) > 65535:
            raise ValueError(f"image {i}: sizes up to 65535 a side")
        shapes.append(shape)
    ctx = get_context(device)
    t, lib = ctx.torch, ctx.lib
    # the sources: device tensors are read where they are; NumPy arrays and host tensors cross in one pinned copy
    src = gather_u8(ctx, images)
    base, span, src_off = src.span()
    descs = (FilterDesc * n)()
    pos = 0
    for i, (shape, f) in enumerate(zip(shapes, filters)):
        d = descs[i]
        d.src_offset, d.dst_offset = src_off[i], pos
        d.height, d.width, d.channels = shape[0], shape[1], shape[2] if len(shape) == 3 else 1
        d.kind, d.xradius, d.yradius, d.percent, d.threshold = f[:5]
        pos += src.nbytes[i]
    out = ctx.empty((pos,), t.uint8)
    path = PATHS[_path]
    ws = ctx.workspace(max(int(lib.aej_filter_workspace_bytes(ctx.handle, ctypes.addressof(descs), n, path)), 256))
    ctx.check(lib.aej_filter_batch(ctx.handle, ctypes.addressof(descs), n, path, ctypes.c_void_p(base), ctypes.c_uint64(span),
                                   out.data_ptr(), ctypes.c_uint64(pos), ws.data_ptr(), ctypes.c_uint64(ws.numel())))
    res = packed_views(out, [d.dst_offset for d in descs], shapes)
    for o, a in zip(res, images):
        com = getattr(a, "jpeg_comment", None)
        if com is not None:
            o.jpeg_comment = com
    return res
