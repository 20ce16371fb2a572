"""The intake the image-list calls share (``filter_many``, ``transform_many``, ``adjust_many``, ``paste_many`` and their siblings,
``resize_many``, ``png_encode_many``, ``standard_jpeg_encode_many``): the argument predicates, "one value or one per image", the check
of one packed uint8 image, the staging of a list of uint8 images of mixed sizes, part on the host and part on the device, into device
memory with one upload, and the tail of a packed-image call -- one packed output, one library entry, its views.  Imports without torch
and without a device."""
import ctypes
import math

import numpy as np

MAX_SIDE = 32767                     # of the images of the warp, adjust and compose calls (filter_many takes 65535)


def is_tensor(x):
    """a torch tensor, told without importing torch (which may not see a device yet)"""
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def one_or_each(value, n, check, name, what):
    """one value for all n `what`s ("image", "file"), or a list / tuple of one per `what` -> list of n checked values.  `check(v, who)`
    checks one and names `who` in a refusal: "`what` i" for entry i, "every `what`" for the one value all of them share."""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{name}: {len(value)} entries for {n} {what}s")
        return [check(v, f"{what} {i}") for i, v in enumerate(value)]
    return [check(value, f"every {what}")] * n


def image_list(images, name):
    """the images of call `name` as a list of at least one"""
    images = list(images)
    if len(images) < 1:
        raise ValueError(f"{name} needs at least one image")
    return images


def image_shape(a, who, max_side=MAX_SIDE):
    """one packed uint8 image -- [H, W], [H, W, 2], [H, W, 3] or [H, W, 4], device tensor, host tensor or NumPy array -> (h, w, channels).
    `who` names it in a refusal.  The checks, in order: the shape, the dtype, the sides."""
    shape, dt = tuple(getattr(a, "shape", ())), str(getattr(a, "dtype", None))
    if not (len(shape) == 2 or (len(shape) == 3 and shape[2] in (2, 3, 4))) or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape {shape}")
    if dt not in ("uint8", "torch.uint8"):
        raise TypeError(f"{who}: uint8 required, got {dt}")
    if max(shape[:2]) > max_side:
        raise ValueError(f"{who}: sizes up to {max_side} a side")
    return int(shape[0]), int(shape[1]), int(shape[2]) if len(shape) == 3 else 1


def is_pil(a):
    return isinstance(getattr(a, "mode", None), str) and hasattr(a, "getbands")


def refuse_pil_and_bool(a, who, what="image", label=None):
    """what the calls that name them say to a PIL image and to a bool array (Pillow's mode "1"), before image_shape sees either.
    `label` (default `who`) is what the TypeError for a PIL image starts with."""
    if is_pil(a):
        if a.mode in ("P", "1"):
            raise NotImplementedError(f"{who}: {what}s of mode {a.mode!r} are not built")
        raise TypeError(f"{label or who}: a uint8 array or tensor required, got a PIL image")
    if str(getattr(a, "dtype", None)) in ("bool", "torch.bool"):
        raise NotImplementedError(f"{who}: {what}s of mode '1' (bool) are not built")


def intake(images, name, check=image_shape):
    """the images of call `name` -> (list, [check(image, "image i")]): at least one image, each a packed uint8 image"""
    images = image_list(images, name)
    return images, [check(a, f"image {i}") for i, a in enumerate(images)]


def packed_shape(h, w, channels):
    """the shape of a packed image: [h, w] for one channel, else [h, w, channels]"""
    return (h, w) + ((channels,) if channels > 1 else ())


def stage_layout(nbytes, on_host, align=1):
    """Where the host items of a list lie in its staging buffer: -> (offsets, total).  offsets[i] is a multiple of `align` for a host
    item, in input order and back to back but for the alignment, and None for a device item; total, a multiple of `align` too, is the
    size of the buffer."""
    offsets, pos = [], 0
    for nb, h in zip(nbytes, on_host):
        offsets.append(pos if h else None)
        if h:
            pos = -(-(pos + nb) // align) * align
    return offsets, pos


class Sources:
    """what gather_u8 returns: `keep` (one device tensor per image, which holds its pixels), `ptrs` (their absolute device addresses)
    and `nbytes`"""
    __slots__ = ("keep", "ptrs", "nbytes")

    def __init__(self, keep, ptrs, nbytes):
        self.keep, self.ptrs, self.nbytes = keep, ptrs, nbytes

    def span(self):
        """-> (base, span_bytes, offsets): the lowest address, the bytes from it to the end of the last image, and every image's
        offset from it -- the (src, src_bytes, src_offset) of the entries that take one source pointer"""
        base = min(self.ptrs)
        end = max(p + nb for p, nb in zip(self.ptrs, self.nbytes))
        return base, end - base, [p - base for p in self.ptrs]


def gather_u8(ctx, arrays, align=1):
    """A list of checked uint8 images (NumPy arrays, host tensors, device tensors; any shapes) -> Sources on ctx's device.

    Host items -- NumPy arrays and CPU tensors, made dense by np.ascontiguousarray -- all cross in one ``ctx.pinned`` buffer and one
    ``copy_(non_blocking=True)`` into one device buffer, at stage_layout's offsets.  A device tensor is used where it lies after
    ``.to(ctx.device).contiguous()``: a contiguous tensor on the right device is not copied and keeps its address.

    The staging contract: the pinned buffer belongs to the context and is valid until the next use of ``ctx.pinned``, and the upload
    from it is only enqueued here.  So the caller follows with a library entry that synchronises the context's stream before it
    returns, or with a stream-ordered blocking copy, before anything uses ``ctx.pinned`` again; and it holds `keep` until then.
    (DESIGN.md names the line that does so for each caller.)"""
    t, n = ctx.torch, len(arrays)
    nbytes = [int(math.prod(a.shape)) for a in arrays]
    on_host = [not (is_tensor(a) and a.is_cuda) for a in arrays]
    offsets, total = stage_layout(nbytes, on_host, align)
    keep = [None] * n
    if any(on_host):
        stage = ctx.pinned(total)
        host = stage.numpy()
        for a, o, nb in zip(arrays, offsets, nbytes):
            if o is not None:
                host[o:o + nb] = np.ascontiguousarray(a.numpy() if is_tensor(a) else a).reshape(-1)
        up = ctx.empty((total,), t.uint8)
        up.copy_(stage[:total], non_blocking=True)
    for i, (a, o, nb) in enumerate(zip(arrays, offsets, nbytes)):
        keep[i] = a.to(device=ctx.device).contiguous() if o is None else up[o:o + nb]
    return Sources(keep, [k.data_ptr() for k in keep], nbytes)


def packed_views(out, offsets, shapes):
    """the images of one packed allocation: out[o:o + prod(shape)] as `shape`, for every offset and shape"""
    return [out[int(o):int(o) + int(math.prod(s))].view(*s) for o, s in zip(offsets, shapes)]


# ---- the tail of a packed-image call: one packed output, one or more library entries into it, its views --------------------------------
def packed_out(ctx, shapes, dtype=None):
    """one allocation of `dtype` (default uint8) that holds arrays of `shapes` back to back in input order: -> (out, offsets), the
    offsets in elements"""
    offsets, pos = [], 0
    for s in shapes:
        offsets.append(pos)
        pos += int(math.prod(s))
    return ctx.empty((pos,), ctx.torch.uint8 if dtype is None else dtype), offsets


def run_entry(ctx, query, batch, descs, n, base, span, out, args=(), query_args=None):
    """One packed-image entry of the library over the n descriptors `descs`: `query` sizes its workspace (never below 256 bytes) and
    `batch` runs it, reading the span bytes at address `base` and writing the whole of `out`.  args: what `batch` takes between n and
    the source; query_args: what `query` takes after n (default: args).  The entry synchronises the context's stream before it
    returns, which ends the use of gather_u8's staging buffer."""
    d = ctypes.addressof(descs)
    ws = ctx.workspace(max(int(query(ctx.handle, d, n, *(args if query_args is None else query_args))), 256))
    ctx.check(batch(ctx.handle, d, n, *args, ctypes.c_void_p(base), ctypes.c_uint64(span), out.data_ptr(), ctypes.c_uint64(out.numel()),
                    ws.data_ptr(), ctypes.c_uint64(ws.numel())))


def packed_results(out, offsets, shapes, inputs=()):
    """packed_views, with the ``jpeg_comment`` of input i carried to result i"""
    res = packed_views(out, offsets, shapes)
    for o, a in zip(res, inputs):
        com = getattr(a, "jpeg_comment", None)
        if com is not None:
            o.jpeg_comment = com
    return res
