"""Pillow's ``Image.convert`` between its 8-bit modes, hue adjustment and ``ImageOps.colorize`` on the GPU, pixel for pixel
(csrc/convert.hip, ``aej_convert_*``), for lists of uint8 images of mixed sizes and one to four channels in one call.

    rgb  = convert_many(images, "RGB")                       # im.convert("RGB") of every image
    hsv  = convert_many(images, ["HSV", "L", ...])           # one target for all, or a list of one per image
    rgb  = convert_many(cmyk, "RGB", source_mode="CMYK")     # source_mode: what the channels MEAN
    xyz  = convert_many(images, "RGB", matrix=(0.412453, 0.357580, 0.180423, 0, ...))   # im.convert("RGB", matrix12) / ("L", matrix4)
    out  = hue_many(images, 0.1)                             # torchvision's adjust_hue on PIL images
    tone = colorize_many(greys, (16, 32, 48), (250, 240, 230))      # ImageOps.colorize
    plan = convert_plan(4, "L", source_mode="CMYK")          # host only: {"steps": ("CMYK>RGB", "RGB>L"), "out_channels": 1}

The modes are "L", "LA", "RGB", "RGBA", "YCbCr", "HSV" and "CMYK"; a source's mode defaults from its channel count (1 L, 2 LA, 3 RGB,
4 RGBA).  Where ``Image.convert`` has no converter for a pair it goes through the source's base mode (RGB for YCbCr, HSV and CMYK);
the library takes the same route -- ``convert_plan`` reports it -- with both steps in registers.  include/aej.h has every formula.

This module shares its name with the package's ``convert`` function (the reference's colour-space conversion): the package attribute
``convert`` stays that function, so import from here by name: ``from adaptive_edge_aware_jpeg_amd.convert import convert_geometry``.

Not built, refused by name with NotImplementedError: the targets "1", "P", "PA", "I", "I;16", "F", "LAB", "RGBa", "La" and "RGBX",
and ``dither=``, ``palette=`` and ``colors=``."""
import ctypes
import math

import numpy as np

from ._images import gather_u8, image_shape, intake, is_int, is_number, one_or_each, packed_out, packed_results, packed_shape, refuse_pil_and_bool, run_entry

MODES = ("L", "LA", "RGB", "RGBA", "YCbCr", "HSV", "CMYK")      # AEJ_MODE_* (include/aej.h)
BANDS = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4, "YCbCr": 3, "HSV": 3, "CMYK": 4}
KINDS = ("mode", "matrix", "hue", "table")                      # AEJ_CONVERT_*
TABLE_BYTES = 768
_DEFAULT = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
_NOT_BUILT = ("1", "P", "PA", "I", "I;16", "I;16L", "I;16B", "I;16N", "F", "LAB", "RGBa", "La", "RGBX")
_BASE = {"L": "L", "LA": "L", "RGB": "RGB", "RGBA": "RGB", "YCbCr": "RGB", "HSV": "RGB", "CMYK": "RGB"}
# the pairs Image.convert (Pillow 12.2) has a converter for; a mode to itself is a copy
_DIRECT = {"L": MODES, "LA": MODES, "RGB": MODES, "RGBA": MODES, "YCbCr": ("L", "LA", "RGB", "YCbCr"), "HSV": ("RGB", "HSV"),
           "CMYK": ("RGB", "RGBA", "HSV", "CMYK")}


def _image(a, who):
    refuse_pil_and_bool(a, who)
    return image_shape(a, who)


def _check_target(m, who):
    if isinstance(m, str) and m in _NOT_BUILT:
        raise NotImplementedError(f"{who}: mode {m!r} is not built")
    if not (isinstance(m, str) and m in MODES):
        raise ValueError(f"{who}: unknown mode {m!r}: one of {', '.join(MODES)}")
    return m


def _check_source(m, who):
    return None if m is None else _check_target(m, who)


def _source_of(m, channels, who):
    if m is None:
        return _DEFAULT[channels]
    if BANDS[m] != channels:
        raise ValueError(f"{who}: source_mode {m!r} has {BANDS[m]} bands, the image {channels} channels")
    return m


def _route(source, target):
    """the steps Image.convert takes: one where it has a converter, else through the source's base mode"""
    if target in _DIRECT[source]:
        return ((source, target),)
    return ((source, _BASE[source]), (_BASE[source], target))


def _check_matrix(m, who):
    if m is None:
        return None
    try:
        m = tuple(m)
    except TypeError:
        raise ValueError(f"{who}: matrix: a sequence of 4 or 12 numbers required") from None
    if len(m) not in (4, 12):
        raise ValueError(f"{who}: a matrix of {len(m)} entries: 4 (target \"L\") or 12 (target \"RGB\")")
    if not all(is_number(x) for x in m):
        raise ValueError(f"{who}: matrix entries must be numbers")
    with np.errstate(over="ignore"):
        f = tuple(float(np.float32(x)) for x in m)
    if not all(math.isfinite(x) for x in f):
        raise ValueError(f"{who}: a matrix entry that is not finite as a float32")
    return f


def _each(value, n, check, name):
    """a list is one entry per image; anything else is one value for all"""
    if isinstance(value, list):
        return one_or_each(value, n, check, name, "image")
    return [check(value, "every image")] * n


def _each_matrix(matrix, n):
    if matrix is None:
        return [None] * n
    if isinstance(matrix, list) and len(matrix) > 0 and (matrix[0] is None or isinstance(matrix[0], (tuple, list, np.ndarray))):
        return one_or_each(matrix, n, _check_matrix, "matrix", "image")
    return [_check_matrix(matrix, "every image")] * n


def _fill(d, shape, source, target, kind="mode", hue=0, table=0, matrix=None):
    d.height, d.width, d.channels = shape
    d.source_mode, d.target_mode, d.kind, d.hue_shift, d.table = MODES.index(source), MODES.index(target), KINDS.index(kind), hue, table
    if matrix is not None:
        d.matrix[:len(matrix)] = matrix


def _run(images, shapes, jobs, tables=(), device=0):
    """the tail of the three calls: jobs[i] = _fill's arguments after the shape, for image i"""
    from ._lib import ConvertDesc, get_context
    n = len(images)
    ctx = get_context(device)
    src = gather_u8(ctx, images)
    base, span, src_off = src.span()
    out_shapes = [packed_shape(h, w, BANDS[j["target"]]) for (h, w, _), j in zip(shapes, jobs)]
    out, offsets = packed_out(ctx, out_shapes)
    descs = (ConvertDesc * n)()
    for i, j in enumerate(jobs):
        _fill(descs[i], shapes[i], **j)
        descs[i].src_offset, descs[i].dst_offset = src_off[i], offsets[i]
    blob = b"".join(tables)
    host_tables = (ctypes.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
    run_entry(ctx, ctx.lib.aej_convert_workspace_bytes, ctx.lib.aej_convert_batch, descs, n, base, span, out,
              args=(ctypes.addressof(host_tables), len(tables)), query_args=())      # synchronises: src's staging is free again
    return packed_results(out, offsets, out_shapes, images)


def convert_geometry():
    """aej_convert_geometry_host (host only): -> dict(chunk, threads, max_grid): the pixels of one image a workgroup takes at a time,
    its threads, and the largest grid"""
    from ._lib import load_library
    g = (ctypes.c_int32 * 3)()
    load_library().aej_convert_geometry_host(ctypes.addressof(g))
    return dict(zip(("chunk", "threads", "max_grid"), (int(v) for v in g)))


def convert_plan(channels, mode, source_mode=None):
    """The route ``Image.convert`` takes from a `channels`-channel image (taken as `source_mode`, default from the channel count) to
    `mode`, without a device (aej_convert_plan_host): -> dict(steps, out_channels); steps is a tuple of "FROM>TO" strings, one per
    converter, e.g. ("CMYK>RGB", "RGB>L").  The refusals are convert_many's."""
    from ._lib import ConvertDesc, ConvertPlan, load_library
    if not (is_int(channels) and 1 <= channels <= 4):
        raise ValueError(f"convert_plan: {channels!r} channels: 1 to 4")
    who = "convert_plan"
    target = _check_target(mode, who)
    source = _source_of(_check_source(source_mode, who), int(channels), who)
    d, p = ConvertDesc(), ConvertPlan()
    _fill(d, (1, 1, int(channels)), source, target)
    rc = load_library().aej_convert_plan_host(ctypes.addressof(d), ctypes.addressof(p))
    if rc:
        raise ValueError(f"{who}: the conversion was refused (code {rc})")
    steps = tuple(f"{MODES[p.step_from[k]]}>{MODES[p.step_to[k]]}" for k in range(p.n_steps))
    if steps != tuple(f"{a}>{b}" for a, b in _route(source, target)):
        raise RuntimeError(f"{who}: the library's route {steps} is not {_route(source, target)}")
    return dict(steps=steps, out_channels=int(p.out_channels))


def convert_many(images, mode, source_mode=None, matrix=None, dither=None, palette=None, colors=None, device: int = 0) -> list:
    """``Image.convert(mode)`` for uint8 [H_i, W_i], [H_i, W_i, 2], [H_i, W_i, 3] and [H_i, W_i, 4] images (device tensors, host tensors
    or NumPy arrays, of mixed sizes, up to 32767 a side) on the device: -> list of uint8 device tensors in input order with the channel
    count of the target mode, views into one packed allocation that never alias an input, so that the encoders and the other ``_many``
    calls read them in place.  mode: one of "L", "LA", "RGB", "RGBA", "YCbCr", "HSV", "CMYK" for all images, or a LIST of one per
    image.  source_mode: what the channels of an image mean -- None (1 channel L, 2 LA, 3 RGB, 4 RGBA) or a mode with as many bands as
    the image has channels; one value for all or a LIST with a mode or None per image.  matrix: ``im.convert("L", matrix4)`` or
    ``im.convert("RGB", matrix12)`` of a 3-channel image taken as RGB; one matrix (a tuple) for all or a LIST of one per image.  An
    input tensor's ``jpeg_comment`` goes to its output.  Everything is checked on the host before any device work and a refusal names
    the image: ValueError for a wrong shape, a side above 32767, a list of another length, an unknown mode, a source_mode whose bands
    do not match, a matrix of the wrong length, on a source that is not RGB or with an entry that is not finite; TypeError for a dtype
    other than uint8; NotImplementedError for the targets and arguments the module docstring lists."""
    for name, v in (("dither", dither), ("palette", palette), ("colors", colors)):
        if v is not None:
            raise NotImplementedError(f"every image: {name}= is not built")
    images, shapes = intake(images, "convert_many", _image)
    n = len(images)
    targets = _each(mode, n, _check_target, "mode")
    sources = _each(source_mode, n, _check_source, "source_mode")
    matrices = _each_matrix(matrix, n)
    jobs = []
    for i, (h, w, c) in enumerate(shapes):
        who = f"image {i}"
        source = _source_of(sources[i], c, who)
        job = dict(source=source, target=targets[i])
        if matrices[i] is not None:
            if source != "RGB":
                raise ValueError(f"{who}: a matrix takes an RGB source, not {source}")
            want = {"L": 4, "RGB": 12}.get(targets[i])
            if want is None:
                raise ValueError(f"{who}: a matrix takes the target \"L\" or \"RGB\", not {targets[i]!r}")
            if len(matrices[i]) != want:
                raise ValueError(f"{who}: a matrix of {len(matrices[i])} entries for target {targets[i]!r}: {want} required")
            job.update(kind="matrix", matrix=matrices[i])
        jobs.append(job)
    return _run(images, shapes, jobs, device=device)


def hue_many(images, factor, device: int = 0) -> list:
    """torchvision's ``adjust_hue`` on PIL images, for images as convert_many takes them: on 3 channels ``h, s, v =
    im.convert("HSV").split()``, h replaced by ``(h + int(factor * 255)) & 255`` and ``Image.merge("HSV", (h, s, v)).convert("RGB")``;
    a 4-channel image gets that on its colour bands and keeps its alpha; 1- and 2-channel images come back unchanged.  factor: a
    number in [-0.5, 0.5] for all images or a list of one per image (ValueError otherwise).  One read and one write per pixel."""
    images, shapes = intake(images, "hue_many", _image)

    def check(f, who):
        if not is_number(f) or not -0.5 <= f <= 0.5:
            raise ValueError(f"{who}: hue factor {f!r}: a number in [-0.5, 0.5] required")
        return int(f * 255) & 255

    shifts = one_or_each(factor, len(images), check, "factor", "image")
    jobs = []
    for (h, w, c), s in zip(shapes, shifts):
        m = _DEFAULT[c]
        jobs.append(dict(source=m, target=m, kind="hue", hue=s) if c >= 3 else dict(source=m, target=m))
    return _run(images, shapes, jobs, device=device)


def _colour(v, name, who):
    if isinstance(v, str):
        raise TypeError(f"{who}: {name} {v!r}: a sequence of 3 ints required; resolving colour names (ImageColor.getrgb) is the caller's job")
    try:
        v = tuple(v)
    except TypeError:
        raise ValueError(f"{who}: {name} {v!r}: a sequence of 3 ints from 0 to 255 required") from None
    if len(v) != 3 or not all(is_int(x) and 0 <= int(x) <= 255 for x in v):
        raise ValueError(f"{who}: {name} {v!r}: a sequence of 3 ints from 0 to 255 required")
    return tuple(int(x) for x in v)


def colorize_table(black, white, mid=None, blackpoint=0, whitepoint=255, midpoint=127, who="colorize_table"):
    """the table of ``ImageOps.colorize``, restated in its integer arithmetic: -> 768 bytes, red, green, blue"""
    black, white = _colour(black, "black", who), _colour(white, "white", who)
    mid = None if mid is None else _colour(mid, "mid", who)
    points = (blackpoint, whitepoint) if mid is None else (blackpoint, midpoint, whitepoint)
    if not all(is_int(p) for p in points) or not all(a <= b for a, b in zip((0,) + points, points + (255,))):
        raise ValueError(f"{who}: 0 <= blackpoint <= {'' if mid is None else 'midpoint <= '}whitepoint <= 255 required, got {points}")
    table = []
    for band in range(3):
        lo, hi = black[band], white[band]
        t = [lo] * blackpoint
        if mid is None:
            span = whitepoint - blackpoint
            t += [lo + i * (hi - lo) // span for i in range(span)]
        else:
            m, s1, s2 = mid[band], midpoint - blackpoint, whitepoint - midpoint
            t += [lo + i * (m - lo) // s1 for i in range(s1)]
            t += [m + i * (hi - m) // s2 for i in range(s2)]
        t += [hi] * (256 - whitepoint)
        table += t
    return bytes(table)


def colorize_many(images, black, white, mid=None, blackpoint=0, whitepoint=255, midpoint=127, device: int = 0) -> list:
    """``ImageOps.colorize(im, black, white, mid, blackpoint, whitepoint, midpoint)`` for 1-channel images as convert_many takes them:
    -> [H, W, 3] images.  The colours are 3-sequences of ints 0 to 255 (a string: TypeError -- ``ImageColor.getrgb`` is the caller's
    job).  The 768-byte table is built on the host as ImageOps.py builds it and the device maps L through it."""
    images, shapes = intake(images, "colorize_many", _image)
    for i, (h, w, c) in enumerate(shapes):
        if c != 1:
            raise ValueError(f"image {i}: colorize takes 1-channel (L) images, got {c} channels")
    table = colorize_table(black, white, mid, blackpoint, whitepoint, midpoint, who="every image")
    jobs = [dict(source="L", target="RGB", kind="table", table=0)] * len(images)
    return _run(images, shapes, jobs, tables=(table,), device=device)
