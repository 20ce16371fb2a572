"""The intake the image-list calls share (``filter_many``, ``adjust_many``, ``resize_many``, ``png_encode_many``, ``standard_jpeg_encode_many``): the
argument predicates, "one value or one per image", and the staging of a list of uint8 images of mixed sizes, part on the host and part
on the device, into device memory with one upload.  Imports without torch and without a device."""
import math

import numpy as np


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
