"""Pillow's two-image operations on the GPU, pixel for pixel (csrc/compose.hip, ``aej_compose_*``): ``paste_many`` is ``Image.paste``
with every mask Pillow takes, ``alpha_composite_many`` is ``Image.alpha_composite``, ``blend_many`` is ``Image.blend``,
``composite_many`` is ``Image.composite`` and ``chop_many`` is ``ImageChops``; ``compose_plan`` says, without a device, what the library
makes of one element.

    out = paste_many(bases, logo, at=(-3, 20), mask="alpha")                  # b = base.copy(); b.paste(logo, (-3, 20), logo)
    out = alpha_composite_many(rgba, white_rgba_backgrounds)                  # Image.alpha_composite(base, overlay)
    out = blend_many(images1, images2, [0.3, 0.5])                            # Image.blend, one alpha per image
    out = composite_many(images1, images2, masks)                             # Image.composite(im1, im2, mask)
    out = chop_many(images1, images2, ChopAdd(scale=2.0, offset=-10))         # ImageChops.add(im1, im2, 2.0, -10)

All take lists of uint8 [H, W], [H, W, 2], [H, W, 3] and [H, W, 4] images (Pillow's L, LA, RGB and RGBA; device tensors, host tensors
or NumPy arrays, of mixed sizes up to 32767 a side) and return a list of uint8 device tensors in input order, views of one packed
allocation that never aliases an input; an input is never written, so Pillow's in-place calls are "copy, then do it".  A second-image
or mask argument is ONE value for all images or a LIST with one value per image.  An object that occurs several times in a call -- one
logo for 64 thumbnails, an overlay that is its own mask -- is staged once.  The arithmetic is Pillow's, restated in include/aej.h.

Not built, refused by name with NotImplementedError: pastes between channel counts other than equal ones, 4 onto 3 and 2 onto 1;
``ImageChops.logical_and`` / ``logical_or`` / ``logical_xor`` / ``offset`` / ``invert``; images of mode "P" and "1" (a bool array is a
mask only)."""
import ctypes
import math

import numpy as np

from ._images import (MAX_SIDE, gather_u8, image_list, image_shape, is_int, is_number, is_pil, packed_out, packed_results, packed_shape,
                      refuse_pil_and_bool, run_entry)

KINDS = ("paste", "alpha_composite", "blend", "chop")          # AEJ_COMPOSE_* (include/aej.h); "composite" is a paste
MASK_KINDS = ("none", "bit", "byte", "overlay")                # AEJ_COMPOSE_MASK_*
CHOPS = ("add", "subtract", "add_modulo", "subtract_modulo", "multiply", "screen", "lighter", "darker", "difference", "soft_light",
         "hard_light", "overlay")                              # AEJ_CHOP_*
CHOPS_NOT_BUILT = ("logical_and", "logical_or", "logical_xor", "offset", "invert")
_MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
_PASTE_PAIRS = ((1, 1), (2, 2), (3, 3), (4, 4), (3, 4), (1, 2))      # (base channels, overlay channels)


class _Chop:
    name = None

    def __init__(self, scale=1.0, offset=0):
        self.scale, self.offset = scale, offset

    def __repr__(self):
        return f"{type(self).__name__}(scale={self.scale!r}, offset={self.offset!r})"


class ChopAdd(_Chop):
    """``ImageChops.add(im1, im2, scale, offset)``: scale a number other than 0, offset an int (as Pillow's C entry takes it)"""
    name = "add"


class ChopSubtract(_Chop):
    """``ImageChops.subtract(im1, im2, scale, offset)``"""
    name = "subtract"


# ---- argument checks (host only) ---------------------------------------------------------------------------------------------------
def _dtype(a):
    return str(getattr(a, "dtype", None)).replace("torch.", "")


def _is_image(a):
    return hasattr(a, "shape") and hasattr(a, "dtype")


def _shape(a, who, what="image"):
    """a uint8 image -> (h, w, channels)"""
    if not _is_image(a) and not is_pil(a):
        raise TypeError(f"{who}: {what}: a uint8 array or tensor required, got {type(a).__name__}")
    refuse_pil_and_bool(a, who, what, f"{who}: {what}")
    try:
        return image_shape(a, f"{who}: {what}")
    except TypeError:                                  # (this module names a tensor's dtype without its "torch.")
        raise TypeError(f"{who}: {what}: uint8 required, got {_dtype(a)}") from None


def _mask_shape(m, who):
    """a mask -> (mask kind, h, w, channels): a bool array is Pillow's mode "1", uint8 [h, w] is "L", [h, w, 2] and [h, w, 4] give their
    last band"""
    if not _is_image(m):
        raise TypeError(f"{who}: mask: None, 'alpha', a bool array or a uint8 image required, got {m!r}")
    shape = tuple(m.shape)
    if _dtype(m) == "bool":
        if len(shape) != 2 or min(shape) < 1 or max(shape) > MAX_SIDE:
            raise ValueError(f"{who}: mask: a bool mask is [h, w] with sizes from 1 to {MAX_SIDE}, got shape {shape}")
        return "bit", int(shape[0]), int(shape[1]), 1
    h, w, c = _shape(m, who, "mask")
    if c == 3:
        raise ValueError(f"{who}: mask: a 3-channel image is no mask (Pillow: bad transparency mask)")
    return "byte", h, w, c


def _ints(v, lengths):
    return isinstance(v, (tuple, list)) and len(v) in lengths and all(is_int(x) for x in v)


def _each(value, n, name, single):
    """one value for all n images, or a list with one per image -> list of n.  `single(v)`: v is ONE value even though it is a list"""
    if isinstance(value, list) and not single(value):
        if len(value) != n:
            raise ValueError(f"{name}: {len(value)} entries for {n} images")
        return value
    return [value] * n


def _element(kind, base, who, **kw):
    """the fields every element has; `over` and `mask` are the objects read (or None)"""
    h, w, c = _shape(base, who)
    e = dict(kind=kind, op=0, base=base, over=None, mask=None, size=(w, h), channels=c, over_size=(w, h), over_channels=c, mask_size=(0, 0),
             mask_channels=0, mask_kind="none", at=(0, 0), box=None, alpha=0.0, scale=1.0, offset=0.0, colour=(0, 0, 0, 0), name=kind)
    e.update(kw)
    if e["box"] is None:
        e["box"] = (0, 0) + tuple(e["over_size"])
    return e


def _paste_element(base, overlay, at, mask, who, name="paste"):
    h, w, c = _shape(base, who)
    # ---- the mask
    mk, msize, mc, mobj = "none", (0, 0), 0, None
    if isinstance(mask, str):
        if mask != "alpha":
            raise ValueError(f"{who}: mask {mask!r}: None, 'alpha', a bool array or a uint8 image required")
        mk = "overlay"
    elif mask is not None:
        mk, mh, mw, mc = _mask_shape(mask, who)
        msize, mobj = (mw, mh), mask
    # ---- the box
    if at is None:
        at = (0, 0)
    if not _ints(at, (2, 4)):
        raise ValueError(f"{who}: at {at!r}: a tuple of 2 or 4 ints required")
    at = tuple(int(v) for v in at)
    if max(abs(v) for v in at) > 2 * MAX_SIDE:
        raise ValueError(f"{who}: at {at!r}: coordinates within +-{2 * MAX_SIDE}")
    # ---- the overlay
    if _is_image(overlay):
        oh, ow, oc = _shape(overlay, who, "overlay")
        if (c, oc) not in _PASTE_PAIRS:
            raise NotImplementedError(f"{who}: a paste of mode {_MODES[oc]} onto mode {_MODES[c]} is not built")
        if mk == "overlay" and oc not in (2, 4):
            raise ValueError(f"{who}: mask 'alpha' needs an overlay with an alpha band, got mode {_MODES[oc]}")
        if mobj is not None and msize != (ow, oh):
            raise ValueError(f"{who}: images do not match: a mask of {msize[0]} x {msize[1]} for an overlay of {ow} x {oh}")
        osize, oobj, colour = (ow, oh), overlay, (0, 0, 0, 0)
    else:
        colour = (overlay,) if is_int(overlay) else overlay
        if not (isinstance(colour, tuple) and len(colour) == c and all(is_int(v) and 0 <= int(v) <= 255 for v in colour)):
            raise ValueError(f"{who}: overlay {overlay!r}: an image, or a colour of mode {_MODES[c]}: "
                             + ("an int from 0 to 255" if c == 1 else f"a tuple of {c} ints from 0 to 255"))
        if mk == "overlay":
            raise ValueError(f"{who}: mask 'alpha' needs an overlay image, not a colour")
        if mobj is not None and mc == 2:
            raise ValueError(f"{who}: bad transparency mask: Pillow fills a colour through masks of mode 1, L and RGBA, not LA")
        if mobj is not None:
            osize = msize
        elif len(at) == 4:
            osize = (at[2] - at[0], at[3] - at[1])
            if min(osize) < 1 or max(osize) > MAX_SIDE:
                raise ValueError(f"{who}: at {at!r}: a colour needs a box of 1 to {MAX_SIDE} pixels a side")
        else:
            raise ValueError(f"{who}: cannot determine region size; use 4-item box (a colour needs a mask or a 4-tuple at)")
        oc, oobj, colour = 0, None, tuple(int(v) for v in colour) + (0,) * (4 - c)
    if len(at) == 4 and (at[2] - at[0], at[3] - at[1]) != osize:
        raise ValueError(f"{who}: images do not match: at {at!r} is {at[2] - at[0]} x {at[3] - at[1]}, the overlay {osize[0]} x {osize[1]}")
    return _element("paste", base, who, over=oobj, mask=mobj, over_size=osize, over_channels=oc, mask_size=msize, mask_channels=mc, mask_kind=mk,
                    at=at[:2], colour=colour, name=name)


def _alpha_element(base, overlay, dest, source, who):
    if not isinstance(source, (list, tuple)):
        raise ValueError(f"{who}: Source must be a list or tuple")
    if not isinstance(dest, (list, tuple)):
        raise ValueError(f"{who}: Destination must be a list or tuple")
    if len(source) not in (2, 4):
        raise ValueError(f"{who}: Source must be a sequence of length 2 or 4")
    if len(dest) != 2:
        raise ValueError(f"{who}: Destination must be a sequence of length 2")
    if not all(is_int(v) for v in tuple(source) + tuple(dest)):
        raise ValueError(f"{who}: dest and source must hold ints")
    if max(abs(int(v)) for v in tuple(source) + tuple(dest)) > 2 * MAX_SIDE:
        raise ValueError(f"{who}: dest and source: coordinates within +-{2 * MAX_SIDE}")
    if min(source) < 0:
        raise ValueError(f"{who}: Source must be non-negative")
    h, w, c = _shape(base, who)
    oh, ow, oc = _shape(overlay, who, "overlay")
    box = tuple(int(v) for v in source) + ((ow, oh) if len(source) == 2 else ())
    if box[2] < box[0]:
        raise ValueError(f"{who}: Coordinate 'right' is less than 'left'")
    if box[3] < box[1]:
        raise ValueError(f"{who}: Coordinate 'lower' is less than 'upper'")
    if c not in (2, 4):
        raise ValueError(f"{who}: image has wrong mode: alpha_composite takes RGBA and LA, got {_MODES[c]}")
    if c != oc:
        raise ValueError(f"{who}: images do not match: modes {_MODES[c]} and {_MODES[oc]}")
    return _element("alpha_composite", base, who, over=overlay, over_size=(ow, oh), over_channels=oc, at=(int(dest[0]) - box[0], int(dest[1]) - box[1]),
                    box=box)


def _same(base, other, who, what):
    h, w, c = _shape(base, who)
    oh, ow, oc = _shape(other, who, what)
    if c != oc:
        raise ValueError(f"{who}: images do not match: modes {_MODES[c]} and {_MODES[oc]}")
    if (h, w) != (oh, ow):
        raise ValueError(f"{who}: images do not match: sizes {w} x {h} and {ow} x {oh}")


def _blend_element(im1, im2, alpha, who):
    _same(im1, im2, who, "second image")
    if not is_number(alpha):
        raise ValueError(f"{who}: alpha {alpha!r}: a number required")
    with np.errstate(over="ignore"):
        a32 = float(np.float32(alpha))
    if not math.isfinite(a32):
        raise ValueError(f"{who}: alpha {alpha!r} is not finite as a float32")
    return _element("blend", im1, who, over=im2, alpha=a32)


def _composite_element(im1, im2, mask, who):
    _same(im1, im2, who, "second image")
    if mask is None or isinstance(mask, str):
        raise ValueError(f"{who}: mask {mask!r}: a bool array or a uint8 image required")
    return _paste_element(im2, im1, (0, 0), mask, who, name="composite")      # image = image2.copy(); image.paste(image1, None, mask)


def _chop_element(im1, im2, op, who):
    h, w, c = _shape(im1, who)
    oh, ow, oc = _shape(im2, who, "second image")
    name = op.name if isinstance(op, _Chop) else op
    if name in CHOPS_NOT_BUILT:
        raise NotImplementedError(f"{who}: ImageChops.{name} is not built")
    if not isinstance(name, str) or name not in CHOPS:
        raise ValueError(f"{who}: op {op!r}: one of {', '.join(CHOPS)}, ChopAdd(scale, offset) or ChopSubtract(scale, offset) required")
    if c != oc:
        raise ValueError(f"{who}: images do not match: modes {_MODES[c]} and {_MODES[oc]}")
    scale, offset = (op.scale, op.offset) if isinstance(op, _Chop) else (1.0, 0)
    if not is_number(scale):
        raise ValueError(f"{who}: {op!r}: scale: a number required")
    with np.errstate(over="ignore"):
        s32 = float(np.float32(scale))
    if not math.isfinite(s32) or s32 == 0.0:
        raise ValueError(f"{who}: {op!r}: scale must be finite and not 0 as a float32")
    if not (is_int(offset) and abs(int(offset)) < 2 ** 24):
        raise ValueError(f"{who}: {op!r}: offset: an int below 2^24 required (Pillow's C entry takes an int)")
    if 510.0 / abs(s32) + abs(int(offset)) >= 2.0 ** 31:
        raise ValueError(f"{who}: {op!r}: (a + b) / scale + offset leaves the int range, where Pillow's conversion is undefined")
    return _element("chop", im1, who, op=CHOPS.index(name), over=im2, over_size=(ow, oh), over_channels=oc, scale=s32, offset=float(int(offset)),
                    name=name)


def _fill(d, e):
    d.kind, d.op = KINDS.index(e["kind"]), e["op"]
    d.width, d.height, d.channels = e["size"][0], e["size"][1], e["channels"]
    d.over_width, d.over_height, d.over_channels = e["over_size"][0], e["over_size"][1], e["over_channels"]
    d.mask_width, d.mask_height, d.mask_channels = e["mask_size"][0], e["mask_size"][1], e["mask_channels"]
    d.mask_kind = MASK_KINDS.index(e["mask_kind"])
    d.x, d.y = e["at"]
    d.box[:] = e["box"]
    d.alpha, d.scale, d.offset = e["alpha"], e["scale"], e["offset"]
    d.colour[:] = e["colour"]


def _resolve(lib, d, who):
    from ._lib import ComposePlan
    p = ComposePlan()
    rc = lib.aej_compose_plan_host(ctypes.addressof(d), ctypes.addressof(p))
    if rc:
        raise ValueError(f"{who}: the element was refused (code {rc})")
    return p


def compose_geometry():
    """aej_compose_geometry_host (host only): -> dict(chunk, threads, max_grid): the pixels of one output image a workgroup takes at a
    time, its threads, and the largest grid"""
    from ._lib import load_library
    g = (ctypes.c_int32 * 3)()
    load_library().aej_compose_geometry_host(ctypes.addressof(g))
    return dict(zip(("chunk", "threads", "max_grid"), (int(v) for v in g)))


_ELEMENTS = {"paste": _paste_element, "alpha_composite": _alpha_element, "blend": _blend_element, "composite": _composite_element,
             "chop": _chop_element}


def compose_plan(kind, base, second, *args, **kwargs):
    """What the library makes of ONE element, without a device (aej_compose_plan_host).  kind: "paste", "alpha_composite", "blend",
    "composite" or "chop"; the other arguments are that call's for one image, by position or by its keywords: ``compose_plan("paste",
    base, logo, at=(-3, 20), mask="alpha")``, ``compose_plan("chop", a, b, "multiply")``.  -> dict(kind, size (w, h), channels, region
    (left, top, right, bottom in the output: the pixels the second image can change, or None when it lies wholly outside), reads (the
    sources a kernel reads: "base", "overlay", "mask")).  "composite" is the paste of images1 over images2, so its base is the
    SECOND image.  The refusals are the calls'."""
    from ._lib import ComposeDesc, load_library
    if kind not in _ELEMENTS:
        raise ValueError(f"compose_plan: kind {kind!r}: one of {', '.join(_ELEMENTS)}")
    names = {"paste": ("at", "mask"), "alpha_composite": ("dest", "source"), "blend": ("alpha",), "composite": ("masks",), "chop": ("op",)}[kind]
    defaults = {"at": (0, 0), "mask": None, "dest": (0, 0), "source": (0, 0)}
    vals = dict(zip(names, args))
    if len(args) > len(names) or set(kwargs) - set(names) or set(kwargs) & set(vals):
        raise TypeError(f"compose_plan: {kind}: takes {', '.join(names)}")
    vals.update(kwargs)
    for k in names:
        if k not in vals:
            if k not in defaults:
                raise TypeError(f"compose_plan: {kind}: {k} is missing")
            vals[k] = defaults[k]
    e = _ELEMENTS[kind](base, second, *[vals[k] for k in names], "compose_plan")
    d = ComposeDesc()
    _fill(d, e)
    p = _resolve(load_library(), d, "compose_plan")
    region = tuple(int(v) for v in p.region)
    reads = ["base"] + (["overlay"] if p.reads_overlay else []) + (["mask"] if p.reads_mask else [])
    return dict(kind="composite" if e["name"] == "composite" else e["kind"], op=e["name"] if e["kind"] == "chop" else None, size=(int(p.out_width), int(p.out_height)), channels=int(p.out_channels),
                region=region if region[2] > region[0] else None, reads=tuple(reads))


def _run(elements, firsts, device):
    """the device half of every call: stage each distinct object once, describe, launch, view"""
    from ._lib import ComposeDesc, get_context
    n = len(elements)
    ctx = get_context(device)
    lib = ctx.lib
    objs, where = [], {}
    for e in elements:
        for k in ("base", "over", "mask"):
            if e[k] is not None and id(e[k]) not in where:
                where[id(e[k])] = len(objs)
                objs.append(e[k])
    src = gather_u8(ctx, objs)
    base, span, src_off = src.span()
    descs = (ComposeDesc * n)()
    shapes = []
    for i, e in enumerate(elements):
        d = descs[i]
        _fill(d, e)
        d.base_offset = src_off[where[id(e["base"])]]
        d.over_offset = src_off[where[id(e["over"])]] if e["over"] is not None else 0
        d.mask_offset = src_off[where[id(e["mask"])]] if e["mask"] is not None else 0
        p = _resolve(lib, d, f"image {i}")
        shapes.append(packed_shape(int(p.out_height), int(p.out_width), int(p.out_channels)))
    out, offsets = packed_out(ctx, shapes)
    for d, o in zip(descs, offsets):
        d.dst_offset = o
    run_entry(ctx, lib.aej_compose_workspace_bytes, lib.aej_compose_batch, descs, n, base, span, out)      # synchronises: src's staging is free again
    return packed_results(out, offsets, shapes, firsts)


def _is_box(v):
    return all(is_int(x) for x in v)


def paste_many(bases, overlays, at=(0, 0), mask=None, device: int = 0) -> list:
    """``b = base.copy(); b.paste(overlay, at, mask)`` for every base: -> list of uint8 device tensors of the bases' shapes.

    overlays: an image or a colour for all bases, or a LIST with one per base.  A colour is an int for a 1-channel base or a TUPLE with
    the base's channel count; it needs a mask, whose size is then the region, or a 4-tuple `at`.  at: Pillow's box, a tuple (x, y) or
    (left, top, right, bottom) -- the size of a 4-tuple must equal the overlay's --, or a list of them; offsets may be negative and the
    region may stick out of the base on any side or lie wholly outside it: it is clipped as Pillow clips it.  mask: None (replace), a
    bool array (Pillow's mode "1": select where true), uint8 [h, w] (mode "L"), uint8 [h, w, 2] or [h, w, 4] (the last band is the
    mask, as Pillow's LA and RGBA masks), or the string "alpha": the overlay's own last band, ``paste(logo, at, logo)``; or a list of
    them.  With 2 or 4 channels on both sides the alpha band is pasted like any other band, as Pillow does; a 4-channel overlay on a
    3-channel base and a 2-channel one on a 1-channel base lose their alpha.  ValueError: a wrong shape, a side above 32767, a list of
    another length, a 3-channel mask, a mask whose size is not the overlay's, a 4-tuple `at` of another size than the overlay
    ("images do not match"), "alpha" with an overlay of 1 or 3 channels or a colour, a colour that does not fit the base's mode or
    has neither a mask nor a 4-tuple `at` of at least one pixel.  TypeError: a dtype other than uint8.  NotImplementedError: every
    other pair of modes, naming both."""
    bases = image_list(bases, "paste_many")
    n = len(bases)
    ov = _each(overlays, n, "overlays", lambda v: False)
    ats = _each(at, n, "at", _is_box)
    masks = _each(mask, n, "mask", lambda v: False)
    return _run([_paste_element(bases[i], ov[i], ats[i], masks[i], f"image {i}") for i in range(n)], bases, device)


def alpha_composite_many(bases, overlays, dest=(0, 0), source=(0, 0), device: int = 0) -> list:
    """``b = base.copy(); b.alpha_composite(overlay, dest, source)`` for every base; with the defaults and equal sizes this is
    ``Image.alpha_composite(base, overlay)``.  Bases and overlays have 4 or 2 channels (RGBA and LA), both alike.  overlays: one image
    for all bases or a list.  dest: (x, y) in the base; source: (left, top) or (left, top, right, bottom) in the overlay; each one
    value or a list of them.  The part of the source box outside the overlay is transparent and the part of the destination outside
    the base is dropped, as in Pillow.  ValueError, with Pillow's words: "Source must be a sequence of length 2 or 4", "Destination
    must be a sequence of length 2", "Source must be non-negative", "Coordinate 'right' is less than 'left'", "Coordinate 'lower' is
    less than 'upper'", "image has wrong mode" for anything but 2 and 4 channels, "images do not match" for 2 against 4."""
    bases = image_list(bases, "alpha_composite_many")
    n = len(bases)
    ov = _each(overlays, n, "overlays", lambda v: False)
    dests = _each(dest, n, "dest", _is_box)
    sources = _each(source, n, "source", _is_box)
    return _run([_alpha_element(bases[i], ov[i], dests[i], sources[i], f"image {i}") for i in range(n)], bases, device)


def blend_many(images1, images2, alpha, device: int = 0) -> list:
    """``Image.blend(im1, im2, alpha)``: im1 + alpha (im2 - im1) in float32 on every band, alpha included.  images2: one image for all
    or a list; alpha: one number or a list.  Values outside 0 to 1 extrapolate and clip, as Pillow's.  ValueError: images of one
    element whose sizes or channel counts differ ("images do not match"), an alpha whose float32 value is not finite."""
    images1 = image_list(images1, "blend_many")
    n = len(images1)
    second = _each(images2, n, "images2", lambda v: False)
    alphas = _each(alpha, n, "alpha", lambda v: False)
    return _run([_blend_element(images1[i], second[i], alphas[i], f"image {i}") for i in range(n)], images1, device)


def composite_many(images1, images2, masks, device: int = 0) -> list:
    """``Image.composite(im1, im2, mask)``: im1 where the mask is 255, im2 where it is 0, Pillow's masked-paste mix in between.  masks
    as paste_many's (a bool array, uint8 [h, w], or the last band of [h, w, 2] and [h, w, 4]); images2 and masks: one for all or a
    list.  The two images and the mask of one element must have EQUAL sizes and the images equal channel counts (ValueError "images
    do not match"); Pillow tolerates a second image larger than the first and the mask, this call does not."""
    images1 = image_list(images1, "composite_many")
    n = len(images1)
    second = _each(images2, n, "images2", lambda v: False)
    ms = _each(masks, n, "masks", lambda v: False)
    return _run([_composite_element(images1[i], second[i], ms[i], f"image {i}") for i in range(n)], images1, device)


def chop_many(images1, images2, op, device: int = 0) -> list:
    """``ImageChops.<op>(im1, im2)``.  op: one of "add", "subtract", "add_modulo", "subtract_modulo", "multiply", "screen", "lighter",
    "darker", "difference", "soft_light", "hard_light", "overlay", or ``ChopAdd(scale, offset)`` / ``ChopSubtract(scale, offset)``
    (the names alone mean scale 1 and offset 0); one for all images or a list.  The channel counts of an element must be equal
    (ValueError "images do not match"); the sizes may differ and the output is the common top-left rectangle, the minimum of each
    side, as Pillow's.  Every band is treated alike, alpha included.  ValueError: an unknown op, a scale that is 0 or not finite,
    an offset that is not an int, a scale and offset that take the result out of the int range.  NotImplementedError:
    "logical_and", "logical_or", "logical_xor", "offset" and "invert"."""
    images1 = image_list(images1, "chop_many")
    n = len(images1)
    second = _each(images2, n, "images2", lambda v: False)
    ops = _each(op, n, "op", lambda v: False)
    return _run([_chop_element(images1[i], second[i], ops[i], f"image {i}") for i in range(n)], images1, device)
