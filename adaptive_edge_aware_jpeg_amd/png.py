"""PNG files decoded on the GPU, pixel-identical to Pillow (``png_decode_many``), the host chunk walk (``png_parse_header``), and PNG
files written on the GPU with Pillow's scanline filtering (``png_encode_many``, at the end of this module).

The host reads only the chunk framing (``aej_png_parse_host``).  The zlib stream of every file -- its IDAT chunks joined -- is inflated
by ``aej_inflate_batch`` (csrc/inflate.hip, one wave per file) or, as the A / B partner, by ``zlib.decompress`` on a thread pool; the
scanline un-filter and the expansion of grey, palette and alpha layouts run on the device either way (csrc/png.hip).

Adam7-interlaced files (``interlaced=True``) and 16-bit files (``depth16=True``) are opt-in keywords of both calls; without them such a
file is refused as it always was.  Neither touches the inflate: an interlaced file is seven smaller un-filter problems (the work item
of the un-filter kernel is a pass, ``png_adam7_passes``) whose packed pass images a second kernel interleaves, and a 16-bit file is the
same walk with units of 2, 4, 6 or 8 bytes."""
import ctypes
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional

import numpy as np

from ._images import gather_u8, is_int, is_tensor, packed_views, stage_layout
from ._lib import get_context
from .jpeg import usable_cpus
from .standard_jpeg import _buffer, _refuse

MODES = ("RGB", "auto")      # AEJ_PNG_RGB, AEJ_PNG_AUTO
MAX_HOST_WORKERS = 16
ACCEPT_ADAM7, ACCEPT_16BIT = 1, 2      # AEJ_PNG_ACCEPT_*
_HINTS = (("Adam7 interlace is not built", "interlaced=True"), ("16-bit samples are not built", "depth16=True"))


def _accept(interlaced, depth16) -> int:
    for name, v in (("interlaced", interlaced), ("depth16", depth16)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError(f"{name}: {v!r} is not a bool")
    return (ACCEPT_ADAM7 if interlaced else 0) | (ACCEPT_16BIT if depth16 else 0)


def png_adam7_passes(width: int, height: int):
    """The seven Adam7 passes of a ``width`` x ``height`` image (PNG specification, section 8.2; aej_png_adam7_passes_host, host only):
    a list of ``(x0, y0, dx, dy, w_p, h_p)`` -- pass p holds the pixels ``(x0 + i dx, y0 + j dy)``, ``w_p`` x ``h_p`` of them, both 0
    for a pass without pixels (such a pass has no bytes in the file, not even filter bytes).  Each non-empty pass is one work item of the
    un-filter kernel.  ValueError for a side that is no positive integer."""
    from ._lib import load_library
    if not is_int(width) or not is_int(height) or width < 1 or height < 1 or width >= 1 << 31 or height >= 1 << 31:
        raise ValueError(f"width and height must be positive integers, not {width!r} and {height!r}")
    t = np.zeros((7, 6), np.int32)
    if load_library().aej_png_adam7_passes_host(int(width), int(height), t.ctypes.data):
        raise ValueError(f"width {width} and height {height} are refused")
    return [tuple(int(v) for v in row) for row in t]


def png_parse_header(data, index: int = 0, interlaced: bool = False, depth16: bool = False):
    """aej_png_parse_host: the PngDesc of one file's chunks (host only, no device needed).  Attributes: ``width``, ``height``,
    ``bit_depth``, ``colour_type``, ``channels`` (samples per pixel in the file), ``row_bytes`` (a scanline without its filter byte),
    ``mode`` (Pillow's mode of the opened file: "1", "L", "P", "RGB", "LA", "RGBA"), ``n_idat`` and ``idat_bytes`` (number and total data
    bytes of the IDAT chunks, empty ones included), ``palette_len`` (entries of PLTE), ``has_trns``, ``interlace``, ``raw_bytes`` (the
    inflated size the file must have: height x (1 + row_bytes), or for an interlaced file the sum over its non-empty passes of
    h_p x (1 + row_bytes_p)) and ``idat_spans``: an int64 array [n_idat, 2] of (offset in the file, length) of each IDAT chunk's data.
    ``interlaced=True`` takes Adam7 files (``interlace`` is 1, ``row_bytes`` stays the full-width scanline), ``depth16=True`` files of bit
    depth 16 (``mode`` is Pillow's: "I;16" for colour type 0, "RGB" for 2, "RGBA" for 4 and for 6); a value that is not a bool raises
    TypeError.  Raises NotImplementedError for a valid file outside the supported set (without its keyword 16-bit samples and Adam7
    interlace, the message naming the keyword; APNG frames) and ValueError for a malformed one (bad signature, missing IHDR, PLTE or
    IDAT, a bad CRC on IHDR, PLTE or tRNS, zero width or height, a chunk length that runs past the file), both naming the file index."""
    from ._lib import AEJ_ERR_CAPACITY, AEJ_ERR_UNSUPPORTED, PngDesc, load_library
    accept = _accept(interlaced, depth16)
    lib = load_library()
    buf, n = _buffer(data)
    d, msg = PngDesc(), ctypes.create_string_buffer(256)
    spans = np.zeros((8, 2), np.int64)

    def parse():
        return lib.aej_png_parse_host_accept(ctypes.addressof(buf), n, accept, ctypes.addressof(d), spans.ctypes.data, len(spans), ctypes.addressof(msg), 256)

    rc = parse()
    if rc == AEJ_ERR_CAPACITY:                           # more IDAT chunks than the first guess: the count is known now
        spans = np.zeros((d.n_idat, 2), np.int64)
        rc = parse()
    if rc == AEJ_ERR_UNSUPPORTED:
        for text, keyword in _HINTS:
            if msg.value.decode() == text:
                raise NotImplementedError(f"file {index}: {text}; pass {keyword} to png_decode_many or png_parse_header")
    _refuse(rc, msg, index)
    d.idat_spans = spans[:d.n_idat]
    return d


def _check_modes(mode, n):
    try:
        modes = [mode] * n if isinstance(mode, str) else list(mode)
    except TypeError:
        raise ValueError(f"mode: {mode!r} is neither one of {MODES} nor a sequence of them") from None
    if len(modes) != n:
        raise ValueError(f"mode: {len(modes)} values for {n} files")
    for i, m in enumerate(modes):
        if m not in MODES:
            raise ValueError(f"mode of file {i}: {m!r} is not one of {MODES}")
    return modes


def _out_channels(d, mode) -> int:
    """bytes per pixel of the image written (png_out_channels of csrc/api_png.hip)"""
    if mode == "RGB" or d.colour_type == 3:
        return 3
    if d.bit_depth == 16:
        return {0: 2, 2: 3, 4: 4, 6: 4}[d.colour_type]
    return d.channels


def _inflate_on_host(ctx, streams, raw, in_off, sizes, interlaced, workers):
    """inflate="host": zlib.decompress of every file's stream on a thread pool, each result through a page-locked buffer into its slot of
    ``raw``.  Raises ValueError naming the file for a stream zlib refuses or that inflates to another size than the header's."""
    t = ctx.torch
    chunk = 256 << 20
    buf = getattr(ctx, "_png_pinned", None)
    need = min(chunk, max(max(sizes), 1 << 20))
    if buf is None or buf.numel() < need:
        buf = ctx._png_pinned = t.empty(need, dtype=t.uint8, pin_memory=True)
    cap = buf.numel()
    hb = buf.numpy()
    used = 0

    def one(s):
        try:
            return zlib.decompress(s)
        except zlib.error as e:
            return e

    with ThreadPoolExecutor(max_workers=min(workers or usable_cpus(), MAX_HOST_WORKERS)) as ex:
        for i, data in enumerate(ex.map(one, streams)):
            if isinstance(data, zlib.error):
                raise ValueError(f"file {i}: the zlib stream of its IDAT chunks does not inflate ({data})")
            if len(data) != sizes[i]:
                raise ValueError(f"file {i}: inflated size {len(data)} is not height x (1 + row bytes) = {sizes[i]}" if not interlaced[i] else
                                 f"file {i}: inflated size {len(data)} is not the sum of its passes' height x (1 + row bytes) = {sizes[i]}")
            done = 0
            while done < sizes[i]:
                if used == cap:                          # the buffer is full: wait for its copies before refilling it
                    t.cuda.current_stream(ctx.device).synchronize()
                    used = 0
                k = min(sizes[i] - done, cap - used)
                hb[used:used + k] = np.frombuffer(data, np.uint8, k, done)
                raw[in_off[i] + done:in_off[i] + done + k].copy_(buf[used:used + k], non_blocking=True)
                used += k
                done += k
    t.cuda.current_stream(ctx.device).synchronize()      # the buffer is reused by the next call


def png_decode_many(files, mode="RGB", inflate: str = "gpu", device: int = 0, workers: Optional[int] = None, interlaced: bool = False,
                    depth16: bool = False) -> List:
    """Decode PNG files (bytes-like, of mixed sizes and kinds) on the GPU -> a list of device uint8 tensors, one per file, in file order.

    ``mode`` is one value for all files or one per file.  "RGB": [H, W, 3], equal to ``np.asarray(Image.open(f).convert("RGB"))`` --
    alpha is dropped (not composited: ``alpha_composite_many`` over a background does that from mode="auto"), tRNS is ignored, grey is replicated, palette indices go through PLTE and an index past the
    palette's end reads black.  "auto": the layout of Pillow's own mode -- colour type 0 gives [H, W] (bit depth 1 becomes 0 / 255, depth
    2 is multiplied by 85, depth 4 by 17: what Pillow's modes "1" and "L" convert to), colour type 4 [H, W, 2], 2 [H, W, 3], 6 [H, W, 4];
    colour type 3 gives [H, W, 3] through the palette, the one place where "auto" is ``convert("RGB")`` and not Pillow's mode "P".  Any
    other mode raises ValueError.

    Supported: non-interlaced files of colour type 0 (1, 2, 4, 8 bits), 2 (8), 3 (1, 2, 4, 8), 4 (8) and 6 (8), any number of IDAT chunks
    (empty ones and ones that split the zlib header included); unknown ancillary chunks are skipped; no gamma, ICC or sRGB handling, as
    Pillow applies none on open.  Without their keywords 16-bit samples and Adam7 interlace raise NotImplementedError("file i: ...",
    naming the keyword), as APNG frames always do; a malformed file (``png_parse_header``) raises ValueError("file i: ..."), both
    before any device work.

    ``interlaced=True`` also takes Adam7-interlaced files of every supported kind, mixed freely with the others: such a file gives, in
    either mode, exactly what the non-interlaced file of the same samples gives.  ``depth16=True`` also takes files of bit depth 16
    (colour types 0, 2, 4, 6), interlaced or not.  Pillow keeps the HIGH BYTE of a 16-bit sample, except for grey: "RGB" gives the high
    bytes of R, G, B (colour types 2, 6) or of the grey sample three times (4), but for colour type 0 the sample CLIPPED to 255 --
    ``min(v, 255)`` three times, not a shift: that is what Pillow's ``convert("RGB")`` of its mode "I;16" does, however odd.  "auto":
    colour type 2 gives uint8 [H, W, 3], 4 and 6 uint8 [H, W, 4] (Pillow opens 16-bit grey + alpha as "RGBA": grey, grey, grey, alpha),
    and colour type 0 a ``torch.uint16`` [H, W] tensor of the whole samples in host byte order (mode "I;16"), equal to
    ``np.asarray(Image.open(f))`` -- a view of the same packed allocation as the other images, its offset rounded up to 2 bytes.  A
    value of either keyword that is not a bool raises TypeError.

    ``inflate="gpu"`` (default): the joined IDAT bytes of all files cross in one page-locked copy and ``aej_inflate_batch`` decodes them,
    one wave per file.  ``inflate="host"``: ``zlib.decompress`` per file on a thread pool (``workers``, at most 16) and the filtered
    scanlines are uploaded.  With either, the un-filter and the layout conversion run on the device and nothing is read back but the
    status words, once per call: a stream that does not inflate, an inflated size other than H x (1 + row bytes) (of an interlaced file:
    other than the sum of that over its non-empty passes) and a filter byte above 4 raise ValueError naming the file (the first such file of the call); the other files of the call are not affected.

    DEPARTURE FROM PILLOW: IDAT chunk CRCs are not checked; the Adler-32 of the inflated data is, on the device (by zlib with
    ``inflate="host"``).  A file whose only damage is an IDAT CRC therefore decodes here, where Pillow raises."""
    if inflate not in ("gpu", "host"):
        raise ValueError("inflate must be 'gpu' or 'host'")
    _accept(interlaced, depth16)
    files = list(files)
    n = len(files)
    modes = _check_modes(mode, n)
    if n == 0:
        return []
    parsed = [png_parse_header(f, i, interlaced, depth16) for i, f in enumerate(files)]
    return _decode_parsed(get_context(device), parsed, [memoryview(f).cast("B") for f in files], modes, inflate, workers)


def _decode_parsed(ctx, parsed, views, modes, inflate, workers, events=None):
    """png_decode_many after the host parse.  events (tools/profiling/bench_png_decode.py): a dict that gets torch events around the two
    enqueues, "inflate" (inflate="gpu" alone) and "unfilter": (start, end) each."""
    from ._lib import INFLATE_STATUS, PNG_STATUS, PngDesc
    t, lib, n = ctx.torch, ctx.lib, len(parsed)

    def mark(name, at):
        if events is not None:
            events.setdefault(name, [t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)])[at].record()

    def align(v, a=4):
        return (v + a - 1) // a * a

    sizes = [d.raw_bytes for d in parsed]
    in_off, out_off, shapes, wide = np.zeros(n, np.int64), np.zeros(n, np.int64), [], []
    ipos = opos = 0
    for i, d in enumerate(parsed):
        in_off[i], out_off[i] = ipos, opos
        ipos += align(sizes[i])
        c = _out_channels(d, modes[i])
        wide.append(d.bit_depth == 16 and d.colour_type == 0 and modes[i] == "auto")      # "I;16": two bytes a pixel, one uint16
        if wide[i]:
            out_off[i] = opos = align(opos, 2)
        shapes.append((d.height, d.width) if modes[i] == "auto" and (c == 1 or wide[i]) else (d.height, d.width, c))
        opos += d.height * d.width * c
    raw = ctx.empty((ipos,), t.uint8)
    out = ctx.empty((opos,), t.uint8)
    stat = ctx.empty((2, n), t.int32)

    # one page-locked staging buffer, one host-to-device copy: the palettes, the stream descriptors and (inflate="gpu") the streams
    off_pal = 0
    off_sd = off_pal + align(n * 768, 16)
    pos = off_sd + align(n * 32, 16)
    st_off = []
    if inflate == "gpu":
        for d in parsed:
            st_off.append(pos)
            pos = align(pos + d.idat_bytes)
    total = align(pos, 16)
    host = ctx.pinned(total)[:total].numpy()
    sd = host[off_sd:off_sd + n * 32].view(np.int64).reshape(n, 4)
    streams = []
    for i, d in enumerate(parsed):
        host[off_pal + 768 * i:off_pal + 768 * (i + 1)] = np.frombuffer(d.palette, np.uint8)
        pieces = [views[i][o:o + k] for o, k in d.idat_spans if k]
        if inflate == "gpu":
            p = st_off[i]
            for piece in pieces:
                host[p:p + len(piece)] = np.frombuffer(piece, np.uint8)
                p += len(piece)
            sd[i] = (st_off[i], d.idat_bytes, in_off[i], sizes[i])
        else:
            streams.append(b"".join(pieces))
    if inflate == "host":
        _inflate_on_host(ctx, streams, raw, in_off, sizes, [d.interlace for d in parsed], workers)
    dev = ctx.empty((total,), t.uint8)
    dev.copy_(ctx.pinned(total)[:total], non_blocking=True)
    base = dev.data_ptr()
    if inflate == "gpu":
        inflated = ctx.empty((n,), t.int64)
        mark("inflate", 0)
        ctx.check(lib.aej_inflate_batch(ctx.handle, base, base + off_sd, n, raw.data_ptr(), ctypes.c_uint64(raw.numel()), inflated.data_ptr(),
                                        stat[0].data_ptr()))
        mark("inflate", 1)
        vouch = (inflated.data_ptr(), stat[0].data_ptr())
    else:
        stat[0].zero_()
        vouch = (None, None)
    descs = (PngDesc * n)(*parsed)
    layouts = np.array([MODES.index(m) for m in modes], np.int32)
    nws = int(lib.aej_png_workspace_bytes(ctx.handle, ctypes.addressof(descs), n))
    if nws == 0:
        raise ValueError("descriptors the library refuses")
    ws = ctx.workspace(nws)
    mark("unfilter", 0)
    ctx.check(lib.aej_png_unfilter_batch(ctx.handle, ctypes.addressof(descs), n, raw.data_ptr(), ctypes.c_uint64(raw.numel()), in_off.ctypes.data,
                                         *vouch, base + off_pal, layouts.ctypes.data, out.data_ptr(), ctypes.c_uint64(out.numel()),
                                         out_off.ctypes.data, stat[1].data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws)))
    mark("unfilter", 1)
    s = stat.cpu().numpy()                               # the one read-back; it also ends the staging buffer's use
    for i in range(n):
        if s[0, i]:
            code = int(s[0, i])
            raise ValueError(f"file {i}: {PNG_STATUS[1]} ({INFLATE_STATUS[code] if 0 <= code < len(INFLATE_STATUS) else f'status {code}'})")
        if s[1, i]:
            code = int(s[1, i])
            raise ValueError(f"file {i}: {PNG_STATUS[code] if 0 <= code < len(PNG_STATUS) else f'status {code}'}")
    if not any(wide):
        return packed_views(out, out_off, shapes)
    return [out[int(o):int(o) + 2 * s[0] * s[1]].view(t.uint16).view(*s) if w else packed_views(out, [o], [s])[0]
            for o, s, w in zip(out_off, shapes, wide)]


# ---- encode -------------------------------------------------------------------------------------------------------------------------
ENCODE_MODES = ("auto", "L", "LA", "RGB", "RGBA")
_MODE_OF_CHANNELS = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
_COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
IDAT_BYTES = 65536           # Pillow cuts the zlib stream into IDAT chunks of this size
MAX_ENCODE_SIDE = 1 << 24    # rows, and bytes per row, of one image (aej_png_filter_bytes)


def _check_images(images, mode, optimize, compress_level, entropy, workers):
    """The host-side validation of png_encode_many (no device is touched): -> [(image, H, W, bytes per pixel)]."""
    if entropy not in ("gpu", "host"):
        raise ValueError("entropy must be 'gpu' or 'host'")
    if mode not in ENCODE_MODES:
        raise ValueError(f"mode: {mode!r} is not one of {ENCODE_MODES}")
    if not isinstance(optimize, (bool, np.bool_)):
        raise ValueError(f"optimize: {optimize!r} is not a bool")
    if not is_int(compress_level) or not 0 <= compress_level <= 9:
        raise ValueError(f"compress_level: {compress_level!r} is not an integer in 0 .. 9")
    if workers is not None and (not is_int(workers) or workers < 1):
        raise ValueError(f"workers: {workers!r} is neither None nor a positive integer")
    if isinstance(images, np.ndarray) or is_tensor(images):
        raise ValueError("images: a list of images is expected, not one array (mixed sizes have no common array)")
    items = []
    for i, x in enumerate(list(images)):
        if not (isinstance(x, np.ndarray) or is_tensor(x)):
            raise ValueError(f"image {i}: {type(x).__name__} is neither a numpy array nor a torch tensor")
        if str(x.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"image {i}: dtype {x.dtype} is not uint8")
        shape = tuple(int(v) for v in x.shape)
        if len(shape) not in (2, 3):
            raise ValueError(f"image {i}: shape {shape} is neither [H, W] nor [H, W, C]")
        if len(shape) == 3 and shape[2] not in (2, 3, 4):
            raise ValueError(f"image {i}: {shape[2]} channels; the layouts are [H, W] (L), [H, W, 2] (LA), [H, W, 3] (RGB) and [H, W, 4] (RGBA)")
        bpp = 1 if len(shape) == 2 else shape[2]
        if mode != "auto" and _MODE_OF_CHANNELS[bpp] != mode:
            raise ValueError(f"image {i}: shape {shape} is mode {_MODE_OF_CHANNELS[bpp]}, not the mode {mode!r} asked for")
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"image {i}: shape {shape} has no pixels")
        if shape[0] > MAX_ENCODE_SIDE or shape[1] * bpp > MAX_ENCODE_SIDE:
            raise NotImplementedError(f"image {i}: shape {shape}: more than 2^24 rows or bytes per row are not built")
        items.append((x, shape[0], shape[1], bpp))
    return items


def _chunk(name, body):
    return struct.pack(">I", len(body)) + name + bytes(body) + struct.pack(">I", zlib.crc32(body, zlib.crc32(name)))


def _frame(H, W, bpp, stream):
    """The file Pillow writes around a zlib stream: signature, IHDR, IDAT chunks of 65536 bytes, IEND."""
    stream = memoryview(stream)
    parts = [_SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, _COLOUR_TYPE[bpp], 0, 0, 0))]
    parts += [_chunk(b"IDAT", stream[k:k + IDAT_BYTES]) for k in range(0, len(stream), IDAT_BYTES)]
    parts.append(_chunk(b"IEND", b""))
    return b"".join(parts)


def _align4(v):
    return (v + 3) // 4 * 4


def _filter_on_device(ctx, items, optimize, events=None):
    """aej_png_filter_batch over all images -> (device uint8 buffer, offsets, sizes) of their scanline streams (offsets are multiples of
    4).  Images that are not on the device cross in one page-locked copy; a tensor that is not contiguous is made so first."""
    t, lib, n = ctx.torch, ctx.lib, len(items)
    sizes = [H * (1 + W * bpp) for _, H, W, bpp in items]
    offs, pos = stage_layout(sizes, [True] * n, align=4)
    raw = ctx.empty((pos + 4,), t.uint8)
    src = gather_u8(ctx, [x for x, _, _, _ in items], align=4)       # (the caller's read-back ends the staging buffer's use)
    descs = np.array([(src.ptrs[i], H, W * bpp, bpp, offs[i]) for i, (_, H, W, bpp) in enumerate(items)], np.int64).reshape(n, 5)
    if events is not None:
        events["filter"] = [t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)]
        events["filter"][0].record()
    ctx.check(lib.aej_png_filter_batch(ctx.handle, descs.ctypes.data, n, 1 if optimize else 0, raw.data_ptr(), ctypes.c_uint64(raw.numel())))
    if events is not None:
        events["filter"][1].record()
    return raw, offs, sizes, src.keep


def _deflate_on_device(ctx, raw, items, offs, sizes):
    """aej_deflate_bytes_*: -> (page-locked uint8 numpy view of the streams back to back, their sizes)."""
    from ._lib import AejError
    t, lib, n = ctx.torch, ctx.lib, len(items)
    caps = [_align4(int(lib.aej_deflate_stream_bound(ctypes.c_uint64(k)))) for k in sizes]
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    descs = np.array([(offs[i], sizes[i], bpp, 1 + W * bpp, out_off[i], caps[i]) for i, (_, H, W, bpp) in enumerate(items)], np.int64).reshape(n, 6)
    nws = int(lib.aej_deflate_bytes_workspace_bytes(descs.ctypes.data, n))
    if nws == 0:
        raise ValueError("stream sizes the library refuses")
    ws = ctx.workspace(nws)
    out = ctx.empty((int(out_off[n]),), t.uint8)
    hist = ctx.empty((n, 320), t.int32)
    dsizes = ctx.empty((n,), t.int64)
    common = (ctx.handle, raw.data_ptr(), ctypes.c_uint64(raw.numel()), descs.ctypes.data, n)
    ctx.check(lib.aej_deflate_bytes_histogram(*common, hist.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws)))
    h = np.ascontiguousarray(hist.cpu().numpy())
    tab = np.zeros((n, 448), np.uint32)
    if lib.aej_deflate_bytes_build_tables(h.ctypes.data, n, tab.ctypes.data):
        raise AejError("aej_deflate_bytes_build_tables failed")
    tabs = t.from_numpy(tab.view(np.int32)).to(ctx.device)
    ctx.check(lib.aej_deflate_bytes_batch(*common, tabs.data_ptr(), 1, out.data_ptr(), ctypes.c_uint64(out.numel()), dsizes.data_ptr(),
                                          ws.data_ptr(), ctypes.c_uint64(nws)))
    got = [int(v) for v in dsizes.cpu().numpy()]
    packed = t.cat([out[int(out_off[i]):int(out_off[i]) + got[i]] for i in range(n)])      # compacted on the device: one copy of what was written
    host = ctx.pinned(packed.numel())[:packed.numel()]
    host.copy_(packed)
    return host.numpy(), got


def png_encode_many(images, mode="auto", optimize: bool = False, compress_level: int = 6, entropy: str = "gpu", device: int = 0,
                    workers: Optional[int] = None) -> List[bytes]:
    """Write PNG files on the GPU -> a list of ``bytes``, one file per image, in order.  The scanline filtering is Pillow's, so the
    filter bytes and the filtered scanlines (``zlib.decompress`` of the joined IDAT chunks) equal those of
    ``Image.fromarray(x).save(f, "PNG", optimize=optimize)`` byte for byte, and the files decode to the input pixels.

    ``images``: uint8 device tensors, host tensors or numpy arrays, of mixed sizes and kinds: [H, W] (L), [H, W, 2] (LA), [H, W, 3]
    (RGB), [H, W, 4] (RGBA) -- the layouts ``png_decode_many(mode="auto")`` returns.  ``mode="auto"`` takes each image's own layout;
    "L", "LA", "RGB" or "RGBA" insist on that one.  A tensor that is not contiguous is accepted and made contiguous first (the filter
    kernel reads whole rows back to back).  Wrong dtype, rank, channel count, an image without pixels and bad option values raise
    ValueError("image i: ...") on the host before any device work; more than 2^24 rows or bytes per row raise NotImplementedError.
    Files carry IHDR, IDAT and IEND only: no palette, 16-bit, interlace, pnginfo, ICC or dpi.

    ``optimize`` is Pillow's: the Average filter joins the candidates (and, with ``entropy="host"``, zlib runs at level 9).

    ``entropy="gpu"`` (default): the scanlines are deflated on the device (csrc/deflate.hip, matches at byte positions, one deflate
    block per file under the file's own Huffman code) and only the finished streams are read back; the host adds the chunk framing.
    The files are larger than Pillow's (README) and ``compress_level`` is IGNORED: there is one effort level.  The same input gives the
    same bytes, alone or in a batch.  ``entropy="host"``: the scanlines are read back once and
    ``zlib.compressobj(compress_level, DEFLATED, 15, 9, Z_FILTERED)`` runs on a thread pool (``workers``, at most 16): the file equals
    Pillow's byte for byte."""
    items = _check_images(images, mode, optimize, compress_level, entropy, workers)
    if not items:
        return []
    return _encode_checked(get_context(device), items, bool(optimize), int(compress_level), entropy, workers)


def _encode_checked(ctx, items, optimize, compress_level, entropy, workers, events=None):
    raw, offs, sizes, keep = _filter_on_device(ctx, items, optimize, events)
    pool = ThreadPoolExecutor(max_workers=min(workers or MAX_HOST_WORKERS, MAX_HOST_WORKERS))
    try:
        if entropy == "host":
            host = ctx.pinned(raw.numel())[:raw.numel()]
            host.copy_(raw)                                  # the one read-back (it also ends the use of the inputs)
            hb = host.numpy()
            level = 9 if optimize else compress_level

            def one(i):
                z = zlib.compressobj(level, zlib.DEFLATED, 15, 9, zlib.Z_FILTERED)
                stream = z.compress(hb[offs[i]:offs[i] + sizes[i]]) + z.flush()
                return _frame(items[i][1], items[i][2], items[i][3], stream)
        else:
            hb, got = _deflate_on_device(ctx, raw, items, offs, sizes)
            starts = np.concatenate([[0], np.cumsum(got)])

            def one(i):
                return _frame(items[i][1], items[i][2], items[i][3], hb[int(starts[i]):int(starts[i]) + got[i]])
        files = list(pool.map(one, range(len(items))))
    finally:
        pool.shutdown()
    del keep
    return files
