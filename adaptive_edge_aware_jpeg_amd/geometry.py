"""Pillow's ``Image.transform``, ``Image.rotate`` and ``Image.transpose`` on the GPU, pixel for pixel (csrc/warp.hip, ``aej_warp_*``):
``transform_many`` (AFFINE, EXTENT, PERSPECTIVE and QUAD under NEAREST, BILINEAR and BICUBIC), ``rotate_many`` and
``transpose_many``, each over a list of uint8 images of mixed sizes and one to four channels in one call, and ``transform_plan``, what
the host decided for one image.

The arithmetic is Pillow's, restated: IEEE float64, one rounded operation at a time (include/aej.h has every formula).  What
``Image.py`` does in Python -- EXTENT to AFFINE, QUAD's corners to its bilinear form, all of ``rotate`` -- is restated here in Python
floats, operation for operation; nothing calls into PIL.  Under NEAREST an AFFINE image takes one of Pillow's two integer paths, picked
by the library's host code: the running-sum tables when ``a1 == a3 == 0`` (every EXTENT), 16.16 fixed point otherwise.

One departure: a coordinate that is NaN (a PERSPECTIVE with 0 / 0 at a pixel centre) is undefined behaviour in Pillow; here that pixel
is an outside pixel and takes the fill.

Sequence-valued arguments (``size``, ``data``, ``fillcolor``, ``center``, ``translate``): a flat sequence of numbers is ONE value for
all images -- except that a *list* given as ``fillcolor`` is always one entry per image (write one colour as a tuple) --, a list or
tuple with an entry that is itself a sequence (or None) is one value per image."""
import ctypes
import math

import numpy as np

from ._images import MAX_SIDE, gather_u8, intake, is_int, is_number, one_or_each, packed_out, packed_results, packed_shape, run_entry

RESAMPLE = {"nearest": 0, "lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}      # Pillow's Image.Resampling
TRANSFORMS = ("affine", "extent", "perspective", "quad", "mesh")                                 # Pillow's Image.Transform, by value
TRANSPOSES = ("flip_left_right", "flip_top_bottom", "rotate_90", "rotate_180", "rotate_270", "transpose", "transverse")      # Image.Transpose
DATA_LENGTH = {"affine": 6, "extent": 4, "perspective": 8, "quad": 8}
PATHS = ("transpose", "tables", "fixed", "affine", "perspective", "quad")      # AEJ_WARP_* (include/aej.h)
_USE = "Use Image.Resampling.NEAREST (0), Image.Resampling.BILINEAR (2) or Image.Resampling.BICUBIC (3)"
_AEJ_ERR_UNSUPPORTED = -5


# ---- argument checks (host only) ---------------------------------------------------------------------------------------------------
def _flat(v):
    return isinstance(v, (list, tuple)) and all(is_number(x) for x in v)


def _each(value, n, check, name, one):
    """one_or_each for an argument whose single value may be a sequence: `one(value)` tells a single value"""
    if one(value):
        return [check(value, "every image")] * n
    return one_or_each(value, n, check, name, "image")


def _check_resample(v, who):
    if isinstance(v, str) and v.lower() in RESAMPLE:
        v = RESAMPLE[v.lower()]
    if not is_int(v):
        raise ValueError(f"{who}: Unknown resampling filter ({v}). {_USE}")
    v = int(v)
    if v in (0, 2, 3):
        return v
    unusable = {4: "Image.Resampling.BOX", 5: "Image.Resampling.HAMMING", 1: "Image.Resampling.LANCZOS"}
    if v in unusable:
        raise ValueError(f"{who}: {unusable[v]} ({v}) cannot be used. {_USE}")
    raise ValueError(f"{who}: Unknown resampling filter ({v}). {_USE}")


def _check_method(v, who):
    if hasattr(v, "getdata") or hasattr(v, "transform"):
        raise NotImplementedError(f"{who}: method {v!r}: ImageTransformHandler and transform objects are not built")
    name = None
    if isinstance(v, str) and v.lower() in TRANSFORMS:
        name = v.lower()
    elif is_int(v) and 0 <= int(v) < len(TRANSFORMS):
        name = TRANSFORMS[int(v)]
    if name is None:
        raise ValueError(f"{who}: unknown transformation method {v!r}: 'affine', 'extent', 'perspective', 'quad' or Pillow's Image.Transform value required")
    if name == "mesh":
        raise NotImplementedError(f"{who}: MESH transforms are not built")
    return name


def _check_transpose(v, who):
    if isinstance(v, str) and v.lower() in TRANSPOSES:
        return TRANSPOSES.index(v.lower())
    if is_int(v) and 0 <= int(v) < len(TRANSPOSES):
        return int(v)
    raise ValueError(f"{who}: unknown transpose method {v!r}: one of Pillow's seven Image.Transpose methods, by name or value, required")


def _check_size(v, who):
    if not (isinstance(v, (list, tuple)) and len(v) == 2 and all(is_int(x) for x in v)):
        raise ValueError(f"{who}: size {v!r}: (width, height) as two ints required")
    w, h = int(v[0]), int(v[1])
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise ValueError(f"{who}: size {v!r}: sizes from 1 to {MAX_SIDE} a side")
    return w, h


def _check_data(v, who):
    if not _flat(v) or len(v) < 1:
        raise ValueError(f"{who}: data {v!r}: a sequence of numbers required")
    out = tuple(float(x) for x in v)
    if not all(math.isfinite(x) for x in out):
        raise ValueError(f"{who}: data {v!r}: finite numbers required")
    return out


def _check_fill(v, who):
    if v is None:
        return None
    if isinstance(v, str):
        raise ValueError(f"{who}: fillcolor {v!r}: colour names are refused; None, an int or one int per channel required")
    vals = list(v) if isinstance(v, (list, tuple)) else [v]
    if not vals or not all(is_int(x) and 0 <= int(x) <= 255 for x in vals):
        raise ValueError(f"{who}: fillcolor {v!r}: None, an int or one int per channel, each 0 to 255, required")
    return tuple(int(x) for x in vals) if isinstance(v, (list, tuple)) else int(v)


def _check_pair(name):
    def check(v, who):
        if v is None:
            return None
        if not (_flat(v) and len(v) == 2 and all(math.isfinite(x) for x in v)):
            raise ValueError(f"{who}: {name} {v!r}: None or two finite numbers required")
        return tuple(x if isinstance(x, (int, float)) else (int(x) if is_int(x) else float(x)) for x in v)
    return check


def _check_angle(v, who):
    if not is_number(v) or not math.isfinite(v):
        raise ValueError(f"{who}: angle {v!r}: a finite number required")
    return v if isinstance(v, (int, float)) else (int(v) if is_int(v) else float(v))


def _check_flag(name):
    def check(v, who):
        if not isinstance(v, (bool, np.bool_)) and not is_int(v):
            raise TypeError(f"{who}: {name} {v!r}: a bool required")
        return bool(v)
    return check


def _one_fill(v):
    """a list is one entry per image, and so is a tuple with an entry that is not a number"""
    return not isinstance(v, list) and not (isinstance(v, tuple) and not _flat(v))


def _scalar(v):
    return not isinstance(v, (list, tuple))


def _fill_bytes(fill, channels, who):
    """what ``Image.new`` puts into every pixel: an int fills the first channel and leaves the others 0, alpha included"""
    if fill is None:
        return (0,) * channels
    if isinstance(fill, tuple):
        if len(fill) != channels:
            raise ValueError(f"{who}: fillcolor {fill!r}: {len(fill)} values for {channels} channel{'s' if channels > 1 else ''}")
        return fill
    return (fill,) + (0,) * (channels - 1)


# ---- Image.py, restated --------------------------------------------------------------------------------------------------------------
def _coefficients(method, data, w, h, who):
    """-> (path name, eight floats): EXTENT becomes AFFINE and QUAD's corners its bilinear form, as ``Image.__transformer`` does"""
    if len(data) != DATA_LENGTH[method]:
        raise ValueError(f"{who}: data of {len(data)} values: '{method}' takes {DATA_LENGTH[method]}")
    if method == "affine":
        return "affine", list(data) + [0.0, 0.0]
    if method == "extent":
        x0, y0, x1, y1 = data
        xs = (x1 - x0) / w
        ys = (y1 - y0) / h
        return "affine", [xs, 0.0, x0, 0.0, ys, y0, 0.0, 0.0]
    if method == "perspective":
        return "perspective", list(data)
    nw, sw, se, ne = data[:2], data[2:4], data[4:6], data[6:8]
    x0, y0 = nw
    As = 1.0 / w
    At = 1.0 / h
    return "quad", [x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
                    y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At]


def _rotate(W, H, angle, expand, center, translate):
    """``Image.rotate`` up to its last line: ("copy",), ("transpose", method) or ("affine", (w, h), matrix)"""
    angle = angle % 360.0
    if not (center or translate):
        if angle == 0:
            return ("copy",)
        if angle == 180:
            return ("transpose", 3)
        if angle in (90, 270) and (expand or W == H):
            return ("transpose", 2 if angle == 90 else 4)
    w, h = W, H
    post_trans = (0, 0) if translate is None else translate
    if center is None:
        center = (w / 2, h / 2)
    angle = -math.radians(angle)
    matrix = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]

    def transform(x, y, matrix):
        a, b, c, d, e, f = matrix
        return a * x + b * y + c, d * x + e * y + f

    matrix[2], matrix[5] = transform(-center[0] - post_trans[0], -center[1] - post_trans[1], matrix)
    matrix[2] += center[0]
    matrix[5] += center[1]
    if expand:
        xx, yy = [], []
        for x, y in ((0, 0), (w, 0), (w, h), (0, h)):
            tx, ty = transform(x, y, matrix)
            xx.append(tx)
            yy.append(ty)
        nw = math.ceil(max(xx)) - math.floor(min(xx))
        nh = math.ceil(max(yy)) - math.floor(min(yy))
        matrix[2], matrix[5] = transform(-(nw - w) / 2.0, -(nh - h) / 2.0, matrix)
        w, h = nw, nh
    return ("affine", (w, h), matrix)


# ---- one image's job -------------------------------------------------------------------------------------------------------------------
def _job(shape, size, path, coef, resample, fill, premultiply, who, method=0):
    """the descriptor fields of one image, resolved by the library's host plan (aej_warp_plan_host): -> dict"""
    from ._lib import WarpDesc, WarpPlan, load_library
    H, W, C = shape
    w, h = size
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise ValueError(f"{who}: an output of {w} x {h}: sizes from 1 to {MAX_SIDE} a side")
    if not all(math.isfinite(v) for v in coef):
        raise ValueError(f"{who}: a coefficient that is not finite: {coef!r}")
    d = WarpDesc()
    d.src_w, d.src_h, d.dst_w, d.dst_h, d.channels = W, H, w, h, C
    d.path, d.method, d.filter, d.premultiply = PATHS.index(path), method, resample, 1 if premultiply else 0
    d.coef[:] = coef
    d.fill[:C] = _fill_bytes(fill, C, who)
    p = WarpPlan()
    tables = (ctypes.c_int32 * (w + h))()
    rc = load_library().aej_warp_plan_host(ctypes.addressof(d), ctypes.addressof(p), ctypes.addressof(tables), w + h)
    if rc == _AEJ_ERR_UNSUPPORTED:
        raise NotImplementedError(f"{who}: an affine transform under 'nearest' beyond 16.16 fixed point (a coordinate of 32768 or more at a corner "
                                  f"of the output): Pillow's float64 fallback is not built")
    if rc:
        raise ValueError(f"{who}: the transform was refused (code {rc})")
    return dict(desc=d, plan=p, tables=tables, out_shape=packed_shape(h, w, C))


def transform_plan(W, H, size, method, data, resample="nearest", channels=3, premultiply=True):
    """What the host decides for one W x H image under ``transform_many(..., size, method, data, resample)``, without a device: ->
    dict(path, coefficients, fixed, xtab, ytab, premultiply).  path: "tables", "fixed", "affine", "perspective" or "quad" (include/aej.h);
    coefficients: the eight float64 the kernel reads (an EXTENT as its AFFINE, a QUAD as its bilinear form); fixed: A0 .. A5 of the 16.16
    path, else None; xtab, ytab: the int32 running-sum tables of the pure-scale path, else None; premultiply: whether alpha is
    premultiplied (2 and 4 channels under "bilinear" and "bicubic", unless premultiply=False).  The refusals are transform_many's."""
    if not (is_int(W) and is_int(H) and 1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f"transform_plan: a {W} x {H} image: sizes from 1 to {MAX_SIDE} a side")
    if not (is_int(channels) and 1 <= channels <= 4):
        raise ValueError(f"transform_plan: {channels!r} channels: 1 to 4")
    who = "transform_plan"
    size, method, data, resample = _check_size(size, who), _check_method(method, who), _check_data(data, who), _check_resample(resample, who)
    path, coef = _coefficients(method, data, size[0], size[1], who)
    j = _job((int(H), int(W), int(channels)), size, path, coef, resample, None, premultiply, who)
    p, w = j["plan"], size[0]
    tab = np.frombuffer(j["tables"], np.int32).copy()
    tables = PATHS[p.path] == "tables"
    return dict(path=PATHS[p.path], coefficients=[float(v) for v in coef], fixed=[int(v) for v in p.fixed] if PATHS[p.path] == "fixed" else None,
                xtab=tab[:w] if tables else None, ytab=tab[w:] if tables else None, premultiply=bool(p.premultiply))


def warp_geometry():
    """aej_warp_geometry_host (host only): -> dict(tile_w, tile_h, flip_bytes, flip_rows, swap_w, swap_h): the output tile of the warp
    kernel in pixels, of the mirrored copy in bytes of a row and rows, and of the transposing kernel in pixels"""
    from ._lib import load_library
    g = (ctypes.c_int32 * 6)()
    load_library().aej_warp_geometry_host(ctypes.addressof(g))
    return dict(zip(("tile_w", "tile_h", "flip_bytes", "flip_rows", "swap_w", "swap_h"), (int(v) for v in g)))


def _run(images, jobs, device):
    """the device part of the three calls: one gather, one packed output, one aej_warp_batch"""
    from ._lib import WarpDesc, get_context
    n = len(images)
    ctx = get_context(device)
    src = gather_u8(ctx, images)
    base, span, src_off = src.span()
    shapes = [j["out_shape"] for j in jobs]
    out, offsets = packed_out(ctx, shapes)
    descs = (WarpDesc * n)()
    for i, j in enumerate(jobs):
        ctypes.memmove(ctypes.addressof(descs[i]), ctypes.addressof(j["desc"]), ctypes.sizeof(WarpDesc))
        descs[i].src_offset, descs[i].dst_offset = src_off[i], offsets[i]
    run_entry(ctx, ctx.lib.aej_warp_workspace_bytes, ctx.lib.aej_warp_batch, descs, n, base, span, out)      # synchronises: src's staging is free again
    return packed_results(out, offsets, shapes, images)


def transform_many(images, size, method, data, resample="nearest", fillcolor=None, premultiply=True, device: int = 0) -> list:
    """``Image.transform`` for uint8 [H_i, W_i], [H_i, W_i, 2], [H_i, W_i, 3] and [H_i, W_i, 4] images (Pillow's L, LA, RGB and RGBA;
    device tensors, host tensors or NumPy arrays, of mixed sizes, up to 32767 a side) on the device: -> list of uint8 device tensors,
    image i with its own channel layout and size[i], views into one packed allocation in input order that never alias an input;
    element i equals ``np.asarray(Image.fromarray(a_i).transform(size_i, method_i, data_i, resample_i, fillcolor=fillcolor_i))``.
    size, method, data, resample and fillcolor: one for all images or one per image (the module docstring says how a sequence is
    read); methods, filters and channel counts mix freely in one call.  method: "affine" (data: 6 numbers), "extent" (4),
    "perspective" (8), "quad" (8: the NW, SW, SE and NE corners), or Pillow's ``Image.Transform`` value.  resample: "nearest",
    "bilinear", "bicubic" or 0, 2, 3.  fillcolor: None (0 in every channel), an int (as ``Image.new``: the first channel, the others
    0) or one int per channel, each 0 to 255.  Images with alpha (2 and 4 channels) are interpolated premultiplied, as Pillow's LA and
    RGBA are; premultiply=False treats their channels independently under every filter -- what Pillow does for CMYK, and what the
    [H, W, 4] images of ``standard_jpeg_decode_many(..., adobe=True, mode="auto")`` need.  A NaN coordinate (undefined in Pillow) makes
    an outside pixel.  An input tensor's ``jpeg_comment`` goes to its output.  Everything is checked on the host before any device
    work and a refusal names the image: ValueError for a wrong shape, a side above 32767, a list of another length, an unknown method
    or filter (Pillow's text), a data of the wrong length or with a value that is not a finite number, a fillcolor that is a name, out
    of range or of another length than the channels; TypeError for a dtype other than uint8; NotImplementedError for "mesh", an
    ``ImageTransformHandler`` and an affine transform under "nearest" whose coordinates reach 32768 at a corner of the output
    (Pillow's float64 fallback is not built)."""
    images, shapes = intake(images, "transform_many")
    n = len(images)
    sizes = _each(size, n, _check_size, "size", lambda v: _flat(v) and len(v) == 2)
    methods = _each(method, n, _check_method, "method", _scalar)
    datas = _each(data, n, _check_data, "data", _flat)
    filters = _each(resample, n, _check_resample, "resample", _scalar)
    fills = _each(fillcolor, n, _check_fill, "fillcolor", _one_fill)
    pre = _check_flag("premultiply")(premultiply, "every image")
    jobs = []
    for i in range(n):
        who = f"image {i}"
        path, coef = _coefficients(methods[i], datas[i], sizes[i][0], sizes[i][1], who)
        jobs.append(_job(shapes[i], sizes[i], path, coef, filters[i], fills[i], pre, who))
    return _run(images, jobs, device)


def rotate_many(images, angle, resample="nearest", expand=False, center=None, translate=None, fillcolor=None, premultiply=True,
                device: int = 0) -> list:
    """``Image.rotate`` for a list of images as transform_many takes them: element i equals ``np.asarray(Image.fromarray(a_i).rotate(
    angle_i, resample_i, expand_i, center_i, translate_i, fillcolor=fillcolor_i))``.  ``Image.rotate`` is restated in Python floats,
    operation for operation: ``angle % 360.0``; without center and translate 0 is a copy, 180 is ROTATE_180, and 90 and 270 are
    ROTATE_90 / ROTATE_270 when expand is set or the image is square; otherwise the matrix comes from ``round(cos, 15)`` and
    ``round(sin, 15)`` about the centre (default (w / 2, h / 2)), expand sizes the output by ``ceil(max) - floor(min)`` of the
    transformed corners, and the result is an AFFINE transform.  Every argument is one for all images or one per image.  The checks,
    the refusals and premultiply are transform_many's; ValueError also for an angle, center or translate that is not finite."""
    images, shapes = intake(images, "rotate_many")
    n = len(images)
    angles = _each(angle, n, _check_angle, "angle", _scalar)
    filters = _each(resample, n, _check_resample, "resample", _scalar)
    expands = _each(expand, n, _check_flag("expand"), "expand", _scalar)
    centers = _each(center, n, _check_pair("center"), "center", lambda v: v is None or _flat(v))
    translates = _each(translate, n, _check_pair("translate"), "translate", lambda v: v is None or _flat(v))
    fills = _each(fillcolor, n, _check_fill, "fillcolor", _one_fill)
    pre = _check_flag("premultiply")(premultiply, "every image")
    jobs = []
    for i in range(n):
        who = f"image {i}"
        H, W = shapes[i][:2]
        plan = _rotate(W, H, angles[i], expands[i], centers[i], translates[i])
        if plan[0] == "copy":                              # the identity under NEAREST: the tables path, a plain copy
            jobs.append(_job(shapes[i], (W, H), "affine", [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], 0, None, pre, who))
        elif plan[0] == "transpose":
            jobs.append(_job(shapes[i], (H, W) if plan[1] != 3 else (W, H), "transpose", [0.0] * 8, 0, None, pre, who, method=plan[1]))
        else:
            jobs.append(_job(shapes[i], plan[1], "affine", [float(v) for v in plan[2]] + [0.0, 0.0], filters[i], fills[i], pre, who))
    return _run(images, jobs, device)


def transpose_many(images, method, device: int = 0) -> list:
    """``Image.transpose`` for a list of images as transform_many takes them: element i equals ``np.asarray(Image.fromarray(a_i)
    .transpose(method_i))``.  method: one for all images or one per image, any of Pillow's seven ``Image.Transpose`` methods by name
    ("FLIP_LEFT_RIGHT", "FLIP_TOP_BOTTOM", "ROTATE_90", "ROTATE_180", "ROTATE_270", "TRANSPOSE", "TRANSVERSE"; any case) or value
    (0 .. 6).  The flips and ROTATE_180 are mirrored copies, the five others go through an LDS tile.  ValueError for an unknown method."""
    images, shapes = intake(images, "transpose_many")
    n = len(images)
    methods = _each(method, n, _check_transpose, "method", _scalar)
    jobs = []
    for i in range(n):
        H, W = shapes[i][:2]
        swap = methods[i] in (2, 4, 5, 6)
        jobs.append(_job(shapes[i], (H, W) if swap else (W, H), "transpose", [0.0] * 8, 0, None, False, f"image {i}", method=methods[i]))
    return _run(images, jobs, device)
