"""Standard (baseline) JPEG on the GPU: the files Pillow writes with ``Image.save(buf, "JPEG", quality=q)`` and the pixels its decoder
returns for them -- the standard-JPEG side of the reference's comparison (test/analysis/metrics_comparison.py: YCbCr, 4:2:0, 8 x 8
blocks, quality 10/25/50/75/90).  ``subsampling=`` ("4:4:4", "4:2:2", "4:2:0" or Pillow's 0, 1, 2) and ``optimize=True`` are Pillow's
keywords of the same call: the chroma layout, and per file the Huffman tables libjpeg builds from that file's own symbols (built on the
device: histogram, tables, table-driven emit) instead of the Annex K ones.  ``progressive=True`` is Pillow's keyword too: the SOF2 file
of libjpeg's ten-scan simple progression, its Annex G entropy coder run on the device (csrc/jfifprog.hip, ``aej_jfif_*_prog``); the
coefficients, and so the decoded pixels, are those of the baseline file.  The defaults are Pillow's: 4:2:0, not optimised, baseline.

``standard_jpeg_decode_many`` reads such files back -- any baseline file, not only this library's, and with ``progressive=True`` any
complete progressive file -- on the device, pixel-identical to ``Image.open(file).convert("RGB")`` (csrc/jpegdec.hip, ``aej_jpegdec_*``;
csrc/jpegprog.hip, ``aej_jpegprog_*``).  With ``scale=2``, ``4`` or ``8`` (one value, or one per file) a file is decoded at that fraction of
its size straight from its coefficients, through libjpeg's reduced inverse DCTs: the ``[ceil(H / s), ceil(W / s), 3]`` pixels Pillow
returns once ``Image.draft()`` has chosen scale ``s`` -- what ``Image.thumbnail()`` starts from (the ``scales_host`` of
``aej_jpegdec_batch_adobe`` / ``aej_jpegprog_batch_adobe``, the one decoder entry per kind that every keyword here goes through; one
fused kernel, csrc/jpegdec.hip ``k_jd_scaled``).  ``draft_scale`` is ``draft()``'s choice of that
scale for a requested size.

``standard_jpeg_thumbnail_many`` finishes that line: ``Image.thumbnail`` on JPEG files, on the device, pixel-identical to Pillow -- the
aspect-preserving final size, the decode at the scale ``draft()`` picks for ``size * reducing_gap``, then Pillow's ``resize`` of the
decoded image over the fractional box ``draft()`` returns: its integer box reduce and its two-pass fixed-point resample (resample.py,
csrc/resample.hip, ``aej_resample_*``), with nothing read back but the decoder's status words.  ``thumbnail_plan`` is that choice for one
file size, on the host.  ``resize_many`` (resample.py) is ``Image.resize`` itself for device images.

``mode="L"`` / ``"auto"`` (one value, or one per file) on the decode and on both thumbnail calls is Pillow's mode "L" on the pixel side:
a one-component file comes back as ``[h, w]``, and under ``"L"`` so does a colour file, as its luma plane alone -- what Pillow gives after
``im.draft("L", size)`` makes libjpeg set ``out_color_space = JCS_GRAYSCALE``: no chroma IDCT, no up-sampling, no colour conversion, and
not ``convert("L")``, from which it differs by several levels (the same entries' ``components_host``; one kernel at
every scale, csrc/jpegdec.hip ``k_jd_luma``).  ``resize_many(mode="L" / "auto")`` takes ``[H, W]`` images, alone or beside ``[H, W, 3]`` ones
(the ``channels_host`` of ``aej_resample_batch_win``), and ``standard_jpeg_thumbnail_jpeg_many(mode="auto")`` writes a grey source's thumbnail as the
one-component file Pillow saves.  ``"RGB"``, the default, is every call as it always was.

``standard_jpeg_transcode_many`` joins the two without touching a pixel: it Huffman-decodes existing files to their quantised
coefficients on the device and entropy-codes the same coefficients again, as a baseline file under the file's own optimal Huffman
tables or as the ten-scan progressive file (csrc/jfiftrans.hip; ``aej_jfif_transform_*_cut`` with no transform, crop or chroma
drop) -- what ``jpegtran -optimize`` and ``jpegtran -progressive`` do.  The output keeps the source's quantisation tables, component ids, sampling and JFIF density, drops its
restart markers, and with ``keep_metadata=True`` carries its APP1..APP13, APP15 and COM segments over (spliced on the host).  A
Pillow file transcoded this way equals Pillow's own ``optimize=True`` / ``progressive=True`` file of the same pixels byte for byte.
``standard_jpeg_transform_many`` is the same call with a lossless flip, rotation or transposition of every file on the way, by name or
from the EXIF Orientation tag (``jpegtran -flip / -rotate / -transpose``, ``exiftran -a``; ``aej_jfif_transform_*_cut``).  Both take
one-component (grey) files too when ``grey=True`` is passed.

``standard_jpeg_encode_many`` is the encoder for images of mixed sizes, each with its own quality, in one call: one front-end kernel over
every block of every image, then one entropy chain per distinct size (csrc/jfifmany.hip, ``aej_jfif_many_*_rst``); the files are those
``standard_jpeg_many`` writes for each image alone; with ``mode="L"`` / ``"auto"`` it also writes the one-component files Pillow saves
for mode-"L" images, from ``[H, W]`` planes.  ``standard_jpeg_thumbnail_jpeg_many`` puts it behind
``standard_jpeg_thumbnail_many``: JPEG bytes in, smaller JPEG bytes out, the pixels never leaving the device.

The files are byte-identical to Pillow's with libjpeg-turbo (JFIF 1.01, Annex K quantisation and Huffman tables, islow DCT, no restart
markers) and the decoded pixels equal ``np.asarray(Image.open(file).convert("RGB"))``.  Colour, down-sampling and DCT run once per image
and every requested quality reuses them (csrc/jfif.hip, ``aej_jfif_*`` in include/aej.h).  Images are uint8, or float32 in [0, 1]
taken as ``rint(x * 255)`` -- the exact inverse of ``Image.load``'s ``uint8 / 255``.
"""
import ctypes
import math
from typing import List, Sequence, Tuple

import numpy as np

from ._images import gather_u8, is_int, is_number, is_tensor, one_or_each, packed_views
from ._lib import get_context

HEADER_CAPACITY = 1024       # SOI .. SOS are 623 bytes with the Annex K Huffman tables; optimised tables are never longer
PROGRESSIVE_HEADER_CAPACITY = 4096   # SOI .. SOF2, ten SOS and eleven DHT, each of them no longer than 5 + 16 + 256 bytes at its largest
SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
SUBSAMPLING_NAMES = ("4:4:4", "4:2:2", "4:2:0")
_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def _check_quality(q):
    if isinstance(q, bool) or int(q) != q or not 1 <= int(q) <= 100:
        raise ValueError(f"quality {q!r}: an integer in 1..100 required")
    return int(q)


def _check_subsampling(s) -> int:
    """"4:4:4" / "4:2:2" / "4:2:0" or Pillow's 0 / 1 / 2 -> 0 / 1 / 2"""
    if isinstance(s, str) and s in SUBSAMPLING:
        return SUBSAMPLING[s]
    if is_int(s) and 0 <= int(s) <= 2:
        return int(s)
    raise ValueError(f"subsampling {s!r}: '4:4:4', '4:2:2', '4:2:0' or 0, 1, 2 required")


def _check_bool(name, v) -> bool:
    if not isinstance(v, (bool, np.bool_)):
        raise TypeError(f"{name} {v!r}: a bool required")
    return bool(v)


def _check_restart(blocks, rows):
    """restart_marker_blocks= / restart_marker_rows= -> two ints in 0..65535 (TypeError for anything but an int, a bool included;
    ValueError outside the range a DRI segment holds)"""
    for name, v in (("restart_marker_blocks", blocks), ("restart_marker_rows", rows)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
        if not 0 <= v <= 65535:
            raise ValueError(f"{name} {v}: 0..65535 required")
    return blocks, rows


def headers(quality: int, H: int, W: int, subsampling="4:2:0", mode: str = "RGB") -> bytes:
    """The markers SOI .. SOS of the file of one (quality, H, W, subsampling) with the Annex K Huffman tables
    (aej_jfif_headers_host_opt); mode="L": those of the grey file (aej_jfif_headers_grey_host; subsampling does not bear on it)."""
    from ._lib import load_library
    ss = _check_subsampling(subsampling)
    if mode not in ("RGB", "L"):
        raise ValueError(f"mode {mode!r}: 'RGB' or 'L' required")
    lib = load_library()
    buf = ctypes.create_string_buffer(HEADER_CAPACITY)
    if mode == "L":
        n = lib.aej_jfif_headers_grey_host(int(quality), int(H), int(W), ctypes.cast(buf, ctypes.c_void_p), HEADER_CAPACITY)
    else:
        n = lib.aej_jfif_headers_host_opt(int(quality), int(H), int(W), ss, ctypes.cast(buf, ctypes.c_void_p), HEADER_CAPACITY)
    if n < 0:
        raise ValueError(f"quality {quality}, {H}x{W}: quality must be in 1..100 and H, W in 1..65535")
    return buf.raw[:n]


def quant_tables(quality: int) -> Tuple[List[int], List[int]]:
    """(luma, chroma) quantisation tables of a quality in natural (row-major) order -- ``Image.open(file).quantization[0 / 1]``."""
    h = headers(_check_quality(quality), 8, 8)
    out, i = [], 2
    while len(out) < 2:                         # walk the marker segments after SOI (table bytes may look like markers)
        n = int.from_bytes(h[i + 2:i + 4], "big")
        if h[i + 1] == 0xDB:
            nat = np.empty(64, np.int64)
            nat[_ZIGZAG] = np.frombuffer(h[i + 5:i + 69], np.uint8)
            out.append([int(v) for v in nat])
        i += 2 + n
    return out[0], out[1]


def huffman_table(counts) -> Tuple[List[int], List[int]]:
    """(BITS[1..16], HUFFVAL) of the optimal table libjpeg builds from 257 symbol counts (aej_jfif_huffman_host, host only: the routine
    the device runs per table).  Entry 256, the reserved all-ones code, is taken as 1."""
    from ._lib import load_library
    c = np.ascontiguousarray(np.asarray(counts, np.int64))
    if c.shape != (257,):
        raise ValueError(f"257 counts required, got shape {c.shape}")
    bits, vals = (ctypes.c_uint8 * 16)(), (ctypes.c_uint8 * 256)()
    n = load_library().aej_jfif_huffman_host(c.ctypes.data, ctypes.addressof(bits), ctypes.addressof(vals), 256)
    if n < 0:
        raise ValueError("counts must be >= 0 and not all zero")
    return list(bits), list(vals[:n])


def _to_u8(ctx, x):
    """[B, H, W, 3] or [H, W, 3] uint8 / float32 (numpy or torch) -> device uint8 [B, H, W, 3]"""
    t = ctx.torch
    is_torch = isinstance(x, t.Tensor)
    if not is_torch:
        x = np.asarray(x)
    if x.ndim == 3:
        x = x[None]
    if x.ndim != 4 or x.shape[3] != 3:
        raise ValueError(f"images must be [B, H, W, 3] (or one [H, W, 3]), got {tuple(x.shape)}")
    if x.shape[0] < 1:
        raise ValueError("at least one image required")
    return _values_u8(ctx, x)


def _values_u8(ctx, x):
    """uint8 / float32 in [0, 1] (numpy or torch, any shape) -> device uint8 of that shape: float values as rint(x * 255)"""
    t = ctx.torch
    dt = str(x.dtype)
    if dt in ("uint8", "torch.uint8"):
        return ctx.to_device(x, t.uint8)
    if dt not in ("float32", "torch.float32"):
        raise TypeError(f"images must be uint8 or float32 in [0, 1], got {dt}")
    xf = ctx.to_device(x, t.float32)
    lo, hi = t.aminmax(xf)
    if not (float(lo) >= 0.0 and float(hi) <= 1.0):
        raise ValueError("float32 images must lie in [0, 1]")
    return t.round(xf * t.full((), 255.0, dtype=t.float32, device=ctx.device)).to(t.uint8)


def _sized_call(ctx, call, cap, total, offsets, lengths):
    """The capacity retry of the entries that write files: call(out, cap) with `out` a device uint8 buffer of the guessed capacity `cap`
    (None for cap 0: the sizes alone); on AEJ_ERR_CAPACITY with the entry's `total` above cap once more with exactly that many bytes; then
    ctx.check.  -> (out, the files' offsets in it, their lengths), the two on the host as int64 arrays"""
    from ._lib import AEJ_ERR_CAPACITY
    out = ctx.empty((cap,), ctx.torch.uint8) if cap else None
    rc = call(out, cap)
    if rc == AEJ_ERR_CAPACITY and total.value > cap:
        cap = int(total.value)
        out = ctx.empty((cap,), ctx.torch.uint8)
        rc = call(out, cap)
    ctx.check(rc)
    return out, offsets.cpu().numpy(), lengths.cpu().numpy()


def _file_bytes(out, offsets, lengths) -> List[bytes]:
    """_sized_call's result read back in one copy -> the files, in the order of `offsets`"""
    blob = out[:int((offsets + lengths).max())].cpu().numpy().tobytes()
    return [blob[o:o + n] for o, n in zip(offsets.tolist(), lengths.tolist())]


class _Encoded:
    """One aej_jfif_encode_batch: the workspace (it holds the coefficients the reconstruction reads), lengths [Q, B], optional bytes."""

    def __init__(self, ctx, x_u8, qualities, want_bytes, subsampling=2, optimize=False, progressive=False):
        t, lib = ctx.torch, ctx.lib
        self.ctx, self.qualities = ctx, [_check_quality(q) for q in qualities]
        self.ss, self.opt = ss, opt = _check_subsampling(subsampling), int(_check_bool("optimize", optimize))
        self.prog = prog = _check_bool("progressive", progressive)      # a progressive file's tables are always its own: optimize changes nothing
        if not self.qualities:
            raise ValueError("at least one quality required")
        B, H, W = (int(v) for v in x_u8.shape[:3])
        self.B, self.H, self.W, Q = B, H, W, len(self.qualities)
        if not (1 <= H <= 65535 and 1 <= W <= 65535):
            raise ValueError(f"{H}x{W}: baseline JPEG needs 1 <= H, W <= 65535")
        nbytes = int(lib.aej_jfif_workspace_bytes_prog(B, H, W, Q, ss) if prog else lib.aej_jfif_workspace_bytes_opt(B, H, W, Q, ss, opt))
        self.ws = ctx.empty((nbytes,), t.uint8)
        q = np.array(self.qualities, np.int32)
        offsets, lengths = ctx.empty((Q * B,), t.int64), ctx.empty((Q * B,), t.int64)
        total = ctypes.c_uint64()
        cap = 0
        if want_bytes:
            hdr = PROGRESSIVE_HEADER_CAPACITY if prog else HEADER_CAPACITY
            cap = Q * B * (hdr + H * W * 3 // (4 if ss == 2 else 2))      # most files are far smaller; a miss costs one more call
        encode = lib.aej_jfif_encode_batch_prog if prog else lib.aej_jfif_encode_batch_opt
        call = lambda o, c: encode(ctx.handle, x_u8.data_ptr(), B, H, W, Q, q.ctypes.data, ss, *(() if prog else (opt,)),  # noqa: E731
                                   o.data_ptr() if o is not None else None,
                                   ctypes.c_uint64(c), offsets.data_ptr(), lengths.data_ptr(), ctypes.addressof(total), self.ws.data_ptr(),
                                   ctypes.c_uint64(nbytes))
        self.out, host_off, host_len = _sized_call(ctx, call, cap, total, offsets, lengths)
        self.lengths, self.offsets = host_len.reshape(Q, B), host_off.reshape(Q, B)

    def files(self) -> List[List[bytes]]:
        """[quality][image] bytes"""
        B = self.B
        flat = _file_bytes(self.out, self.offsets.reshape(-1), self.lengths.reshape(-1))
        return [flat[k:k + B] for k in range(0, len(flat), B)]

    def decoded(self):
        """device uint8 [Q, B, H, W, 3]: what Pillow's decoder returns for every file"""
        ctx = self.ctx
        rgb = ctx.empty((len(self.qualities), self.B, self.H, self.W, 3), ctx.torch.uint8)
        if self.prog:
            ctx.check(ctx.lib.aej_jfif_recon_batch_prog(ctx.handle, self.B, self.H, self.W, len(self.qualities), self.ss, rgb.data_ptr(),
                                                        self.ws.data_ptr(), ctypes.c_uint64(self.ws.numel())))
            return rgb
        ctx.check(ctx.lib.aej_jfif_recon_batch_opt(ctx.handle, self.B, self.H, self.W, len(self.qualities), self.ss, self.opt, rgb.data_ptr(),
                                                   self.ws.data_ptr(), ctypes.c_uint64(self.ws.numel())))
        return rgb


def encode_decode(ctx, x_u8, qualities, want_bytes=False, subsampling=2, optimize=False, progressive=False) -> _Encoded:
    """The sweep's entry: one encode of device uint8 [B, H, W, 3] for every quality (on ctx's stream)."""
    return _Encoded(ctx, x_u8, qualities, want_bytes, subsampling, optimize, progressive)


def workspace_bytes(ctx, B, H, W, n_q, subsampling=2, optimize=False, progressive=False) -> int:
    if _check_bool("progressive", progressive):
        return int(ctx.lib.aej_jfif_workspace_bytes_prog(B, H, W, n_q, _check_subsampling(subsampling)))
    return int(ctx.lib.aej_jfif_workspace_bytes_opt(B, H, W, n_q, _check_subsampling(subsampling), int(_check_bool("optimize", optimize))))


def standard_jpeg_many(x, quality: int, device: int = 0, subsampling="4:2:0", optimize: bool = False, progressive: bool = False) -> List[bytes]:
    """Every image's file, equal to ``PIL.Image.fromarray(u8).save(buf, "JPEG", quality=quality, subsampling=subsampling,
    optimize=optimize, progressive=progressive)``.  x: uint8 or float32 in [0, 1], [B, H, W, 3] or [H, W, 3], numpy or torch.  subsampling: "4:4:4", "4:2:2",
    "4:2:0" or 0, 1, 2 (ValueError otherwise); optimize: a bool (TypeError otherwise) -- per file the Huffman tables built from its
    own symbols; progressive: a bool (TypeError otherwise) -- the progressive (SOF2) file of libjpeg's ten scans, whose tables are
    always its own, so optimize does not change its bytes.  This call, standard_jpeg_batch and sweep write no restart markers (their
    Annex K bit count is fused into the quantisation kernel); standard_jpeg_encode_many and the transcoder take restart_marker_blocks=
    and restart_marker_rows=."""
    q, ss, opt, prog = _check_quality(quality), _check_subsampling(subsampling), _check_bool("optimize", optimize), _check_bool("progressive", progressive)
    ctx = get_context(device)
    return _Encoded(ctx, _to_u8(ctx, x), [q], True, ss, opt, prog).files()[0]


def standard_jpeg_batch(x, qualities: Sequence[int], device: int = 0, subsampling="4:2:0", optimize: bool = False, progressive: bool = False):
    """-> (sizes int64 [B, Q]: len() of every file, decoded uint8 [Q, B, H, W, 3] on the device: Pillow's decode of every file).
    Colour, down-sampling and DCT run once per image for all the qualities.  subsampling, optimize, progressive: as standard_jpeg_many
    (with progressive the sizes are those of the progressive files; the pixels do not change)."""
    qualities = [_check_quality(q) for q in qualities]
    ss, opt, prog = _check_subsampling(subsampling), _check_bool("optimize", optimize), _check_bool("progressive", progressive)
    ctx = get_context(device)
    enc = _Encoded(ctx, _to_u8(ctx, x), qualities, False, ss, opt, prog)
    return np.ascontiguousarray(enc.lengths.T.astype(np.int64)), enc.decoded()


def _buffer(data):
    """bytes-like -> (a ctypes copy of it, its length); an empty input still gets an address"""
    mv = memoryview(data).cast("B")
    return ((ctypes.c_uint8 * len(mv)).from_buffer_copy(mv) if len(mv) else (ctypes.c_uint8 * 1)()), len(mv)


def _refuse(rc, msg, index):
    """a parser's return code and message -> NotImplementedError (AEJ_ERR_UNSUPPORTED) or ValueError naming the file; nothing for 0"""
    from ._lib import AEJ_ERR_UNSUPPORTED
    if rc == AEJ_ERR_UNSUPPORTED:
        raise NotImplementedError(f"file {index}: {msg.value.decode()}")
    if rc != 0:
        raise ValueError(f"file {index}: {msg.value.decode()}")


def _raise_status(bad):
    """bad: [(file index, non-zero AEJ_JPEGDEC_* status word)] in file order -> ValueError for the first; nothing when empty"""
    from ._lib import JPEGDEC_STATUS
    for i, code in bad:
        raise ValueError(f"file {i}: {JPEGDEC_STATUS[code] if 0 <= code < len(JPEGDEC_STATUS) else f'status {code}'}")


def parse_header(data, index: int = 0, layout_440: bool = False, adobe: bool = False):
    """aej_jpegdec_parse_host_440: the JpegDecDesc of one file's markers (host only).  Raises NotImplementedError for a valid file
    outside the supported set and ValueError for a malformed header, both naming the file index.  layout_440=True (the entry's
    layout_440 = 1) also takes a three-component file whose luma is sampled 1 x 2 over 1 x 1 chroma (4:4:0: hs = 1, vs = 2); without it
    such a file is refused.  adobe=True (aej_jpegdec_parse_host_adobe, whose parser accepts files the other refuses) also takes
    four-component (CMYK, YCCK) and RGB-coded files, refused without it; the descriptor then carries two more attributes: ``adobe``,
    the file's JpegAdobe (component 3's factors and tables), and ``colour``, one of "YCbCr", "RGB", "CMYK", "YCCK"."""
    from ._lib import JPEG_COLOURS, JpegAdobe, JpegDecDesc, load_library
    buf, n = _buffer(data)
    d, msg = JpegDecDesc(), ctypes.create_string_buffer(256)
    head = (ctypes.addressof(buf), n, ctypes.addressof(d), ctypes.addressof(msg), 256)
    lib = load_library()
    adobe, l440 = _check_bool("adobe", adobe), int(_check_bool("layout_440", layout_440))
    if adobe:
        x = JpegAdobe()
        _refuse(lib.aej_jpegdec_parse_host_adobe(*head[:3], ctypes.addressof(x), *head[3:], l440), msg, index)
        d.adobe, d.colour = x, JPEG_COLOURS[x.colour]
        return d
    _refuse(lib.aej_jpegdec_parse_host_440(*head, l440), msg, index)
    return d


def parse_scans(data, index: int = 0, layout_440: bool = False, adobe: bool = False):
    """aej_jpegprog_parse_host_440: (JpegProgFrame, [JpegProgScan, ...]) of one progressive (SOF2) file, every marker SOI .. EOI walked
    on the host.  Raises ValueError for a malformed file or a scan script that violates T.81 G.1.1.1 and NotImplementedError for a valid
    file outside the supported set (an incomplete progression, arithmetic coding, a file that is not progressive, ...), both naming the
    file index.  layout_440: as parse_header (the entry's layout_440).  adobe: as parse_header (aej_jpegprog_parse_host_adobe); the
    frame then carries ``adobe`` and ``colour``."""
    from ._lib import JPEG_COLOURS, JpegAdobe, JpegProgFrame, JpegProgScan, load_library
    lib = load_library()
    buf, n = _buffer(data)
    frame, msg = JpegProgFrame(), ctypes.create_string_buffer(256)
    adobe, l440 = _check_bool("adobe", adobe), int(_check_bool("layout_440", layout_440))
    if adobe:
        x = JpegAdobe()
        parse = lambda d, m, f, sc, cap, ms, mc: lib.aej_jpegprog_parse_host_adobe(d, m, f, sc, cap, ctypes.addressof(x), ms, mc, l440)  # noqa: E731
    else:
        parse = lambda *a: lib.aej_jpegprog_parse_host_440(*a, l440)  # noqa: E731
    _refuse(parse(ctypes.addressof(buf), n, ctypes.addressof(frame), None, 0, ctypes.addressof(msg), 256), msg, index)
    scans = (JpegProgScan * max(frame.n_scans, 1))()
    _refuse(parse(ctypes.addressof(buf), n, ctypes.addressof(frame), ctypes.addressof(scans), frame.n_scans, ctypes.addressof(msg), 256), msg, index)
    if adobe:
        frame.adobe, frame.colour = x, JPEG_COLOURS[x.colour]
    return frame, list(scans)


def _parse_sources(files, progressive=True, transcoder=False, start=0, grey=False, layout_440=False, adobe=False):
    """Parse every file once, telling baseline from progressive: yields (i, is_progressive, JpegDecDesc | (JpegProgFrame, scans), the
    frame -- that descriptor, or that JpegProgFrame --, view) file by file, i counting from start.  progressive=False refuses
    progressive files the way standard_jpeg_decode_many does without
    its keyword; transcoder=True refuses what the transcoder does not take, which without grey=True includes one-component files.
    layout_440=True, adobe=True: the parsers' keywords of those names, for every file.  Every refusal names the file."""
    for i, f in enumerate(files, start):
        try:
            d, is_prog = parse_header(f, i, layout_440, adobe), False
        except NotImplementedError as e:
            if "progressive JPEG (SOF2)" not in str(e):
                raise
            if not progressive:
                raise NotImplementedError(f"{e}; pass progressive=True to standard_jpeg_decode_many") from None
            d, is_prog = parse_scans(f, i, layout_440, adobe), True
        frame = d[0] if is_prog else d
        if transcoder and frame.ncomp != 3 and not (grey and frame.ncomp == 1):
            raise NotImplementedError(f"file {i}: a single-component (grey) file: the transcoder takes three-component files unless grey=True is passed")
        if transcoder and frame.precision16:
            raise NotImplementedError(f"file {i}: a 16-bit quantisation table: the transcoder writes 8-bit tables")
        yield i, is_prog, d, frame, memoryview(f).cast("B")


class _Sources:
    """The parsed files of one call, marshalled once for the decoders and the transcoder: parsed[i] is file i's JpegDecDesc or
    (JpegProgFrame, scans), frames[i] its frame either way, views[i] its bytes; base_idx and prog_idx are the baseline and the
    progressive files, each in file order."""

    def __init__(self):
        self.parsed, self.frames, self.views, self.base_idx, self.prog_idx = [], [], [], [], []

    def parse(self, files, *args, **kw):
        """_parse_sources(files, ...) with every file entered here before it is yielded as (i, frame, view): what the caller checks
        between two files is reported before the next file's header is"""
        for i, is_prog, d, frame, mv in _parse_sources(files, *args, **kw):
            self.parsed.append(d)
            self.frames.append(frame)
            self.views.append(mv)
            (self.prog_idx if is_prog else self.base_idx).append(i)
            yield i, frame, mv

    def baseline(self, idx):
        """-> (JpegDecDesc [n], n, the staging pieces (file, scan offset, scan length)) of the baseline files idx"""
        from ._lib import JpegDecDesc
        descs = (JpegDecDesc * max(len(idx), 1))(*[self.parsed[i] for i in idx])
        return descs, len(idx), [(i, self.parsed[i].scan_offset, self.parsed[i].scan_length) for i in idx]

    def progressive(self, idx):
        """-> (JpegProgFrame [n], the files' JpegProgScan in one flat array, n, the staging pieces (file, data offset, data length) of
        those scans) of the progressive files idx"""
        from ._lib import JpegProgFrame, JpegProgScan
        flat = [(i, s) for i in idx for s in self.parsed[i][1]]
        frames = (JpegProgFrame * max(len(idx), 1))(*[self.frames[i] for i in idx])
        scans = (JpegProgScan * max(len(flat), 1))(*[s for _, s in flat])
        return frames, scans, len(idx), [(i, s.data_offset, s.data_length) for i, s in flat]


def _stage(ctx, views, pieces):
    """pieces: [(file, offset, length)] -> (device uint8 buffer holding them 16-byte aligned, int64 offsets), in one pinned copy"""
    t = ctx.torch
    off = np.zeros(max(len(pieces), 1), np.int64)
    pos = 0
    for k, (_, _, length) in enumerate(pieces):
        off[k] = pos
        pos += (length + 15) // 16 * 16
    stage = ctx.pinned(max(pos, 1))
    host = stage.numpy()
    for k, (i, o, length) in enumerate(pieces):
        host[off[k]:off[k] + length] = np.frombuffer(views[i], np.uint8, length, o)
    dev = ctx.empty((max(pos, 1),), t.uint8)
    dev.copy_(stage[:max(pos, 1)], non_blocking=True)
    return dev, off


def _adobe_array(frames):
    """the JpegAdobe [n] of a call's frames when one of them is a four-component or RGB-coded file (the _adobe entries), else None"""
    from ._lib import JpegAdobe
    xs = [getattr(f, "adobe", None) for f in frames]
    if not any(x is not None and x.colour != 0 for x in xs):
        return None
    return (JpegAdobe * len(xs))(*[x if x is not None else JpegAdobe() for x in xs])


def _decode_kind(ctx, src, prog, out, out_off, scales=None, comps=None, boxes=None, sbox=False):
    """aej_jpegdec_batch_adobe over the call's baseline files or (prog) aej_jpegprog_batch_adobe over its progressive ones -> their
    status words (device int32).  The package binds the widest entry: an option that no file of the call uses goes as NULL -- scales
    (int32 [n]), comps (3, 1 or, for a four-component file that leaves in mode "CMYK", 4 per file), boxes (int32 [n, 4]), the JpegAdobe
    array (_adobe_array) -- and the entry is then the narrower one byte for byte, launches included (include/aej.h).  sbox: the boxes are
    in pixels of each file's scaled image, which is the _sbox entries' reading of the same arguments."""
    idx = src.prog_idx if prog else src.base_idx
    if prog:
        frames, pscans, n, pieces = src.progressive(idx)
        lead = (ctx.handle, ctypes.addressof(frames), ctypes.addressof(pscans), n)
    else:
        descs, n, pieces = src.baseline(idx)
        lead = (ctx.handle, ctypes.addressof(descs), n)
    data, data_off = _stage(ctx, src.views, pieces)
    oo = np.ascontiguousarray(out_off[idx])
    status = ctx.empty((n,), ctx.torch.int32)
    arrays = [None if a is None else np.ascontiguousarray(a[idx], np.int32) for a in (scales, comps, boxes)]
    how = [None if a is None else a.ctypes.data for a in arrays]
    xs = _adobe_array([src.frames[i] for i in idx])
    # _adobe wins over _sbox: its files are refused at any scale but 1, where a scaled box is the full-size box (another file's at 2, 4, 8: refused)
    sfx = "_sbox" if sbox and xs is None else "_adobe"
    if sfx == "_adobe":
        how.append(None if xs is None else ctypes.addressof(xs))
    family = "aej_jpegprog_" if prog else "aej_jpegdec_"
    nws = int(getattr(ctx.lib, family + "workspace_bytes" + sfx)(*lead, *how))
    if nws == 0:
        raise ValueError("descriptors the library refuses")
    ws = ctx.workspace(nws)
    ctx.check(getattr(ctx.lib, family + "batch" + sfx)(*lead, *how, data.data_ptr(), ctypes.c_uint64(data.numel()), data_off.ctypes.data,
                                                       out.data_ptr(), ctypes.c_uint64(out.numel()), oo.ctypes.data, status.data_ptr(),
                                                       ws.data_ptr(), ctypes.c_uint64(nws)))
    return status


SCALES = (1, 2, 4, 8)


def _check_scale(s) -> int:
    if not is_int(s) or int(s) not in SCALES:
        raise ValueError(f"scale {s!r}: 1, 2, 4 or 8 required")
    return int(s)


def _check_scales(scale, n):
    """scale= of standard_jpeg_decode_many -> int32 [n], one of SCALES per file"""
    if isinstance(scale, (str, bytes)) or not hasattr(scale, "__len__"):
        return np.full(n, _check_scale(scale), np.int32)
    if len(scale) != n:
        raise ValueError(f"scale: {len(scale)} values for {n} files")
    return np.array([_check_scale(s) for s in scale], np.int32).reshape(n)


def _check_modes(mode, n, what="file"):
    """mode= of the decoders and thumbnail calls -> list of n of "RGB", "L", "auto": one string for every file, or a list / tuple of
    one per file.  ValueError for another string (in a sequence naming the file) or a sequence of another length; TypeError for
    anything that is neither a string nor a list / tuple (in a sequence naming the file)."""
    def one(m, who):
        if not isinstance(m, str):
            raise TypeError(f"{who}: mode {m!r}: a string ('RGB', 'L' or 'auto') required")
        if m not in ("RGB", "L", "auto"):
            raise ValueError(f"{who}: mode {m!r}: 'RGB', 'L' or 'auto' required")
        return m
    if isinstance(mode, str):
        return [one(mode, f"every {what}")] * n
    if not isinstance(mode, (list, tuple)):
        raise TypeError(f"mode {mode!r}: 'RGB', 'L' or 'auto', or a list of one per {what}, required")
    if len(mode) != n:
        raise ValueError(f"mode: {len(mode)} values for {n} {what}s")
    return [one(m, f"{what} {i}") for i, m in enumerate(mode)]


def _check_decode_box(b, who):
    """one box -> (left, top, right, bottom) of ints; TypeError for anything that is not a list / tuple of four integers"""
    if not isinstance(b, (list, tuple)) or len(b) != 4:
        raise TypeError(f"{who}: box {b!r}: (left, top, right, bottom) required")
    for v in b:
        if not is_int(v):
            raise TypeError(f"{who}: box {tuple(b)!r}: four integers required")
    return tuple(int(v) for v in b)


def _check_boxes(box, n):
    """box= of standard_jpeg_decode_many -> None, or a list of n of None / (left, top, right, bottom).  One box for every file, or a
    list / tuple with one entry per file, each a box or None (told apart by an entry that is None, a list or a tuple).  TypeError for a
    value or an entry that is not a box of four integers (a bool, a float, a tuple of another length); ValueError for a sequence of
    another length than files.  Whether a box fits its image is checked once the header is parsed (_box_in_image)."""
    if box is None:
        return None
    if not isinstance(box, (list, tuple)):
        raise TypeError(f"box {box!r}: (left, top, right, bottom), or a list of one such tuple or None per file, required")
    if len(box) == 0 or any(b is None or isinstance(b, (list, tuple)) for b in box):
        if len(box) != n:
            raise ValueError(f"box: {len(box)} entries for {n} files")
        return [None if b is None else _check_decode_box(b, f"file {i}") for i, b in enumerate(box)]
    return [_check_decode_box(box, "every file")] * n


def _box_in_image(box, width, height, index):
    """ValueError naming the file unless 0 <= left < right <= width and 0 <= top < bottom <= height"""
    l, t, r, b = box
    if not (0 <= l < r <= width and 0 <= t < b <= height):
        raise ValueError(f"file {index}: box {box!r} is empty, inverted or leaves the {width} x {height} image (nothing is padded)")


def decode_box_window(width: int, height: int, hs: int, vs: int, ncomp: int, box, luma: bool = False, scale: int = 1):
    """The MCU window of a boxed decode (host only): (mx0, my0, mx1, my1), the half-open rectangle of MCUs -- 8 hs x 8 vs pixels each,
    8 x 8 for a one-component file -- whose blocks the pixels of box = (left, top, right, bottom) read in a width x height file with
    luma sampling factors hs x vs (1 x 1, 2 x 1, 2 x 2, 1 x 2) and ncomp components.  That is the MCUs of the luma samples of those
    pixels and, per chroma component of a three-component file, of the samples libjpeg's up-sampling reads for them: the co-sited one
    plus one neighbour in each up-sampled direction (h2v2: the far row and columns j +- 1; h2v1: columns; h1v2: rows), after the edge
    rules of the FILE's chroma plane (no neighbour past its first or last sample; a plane at most 2 wide is replicated: no neighbour
    at all).  The bounding rectangle is exact.  luma=True: the window of a mode "L" decode, the luma samples' alone.  The C twin is
    aej_jpegdec_box_window_host.  ValueError for a box that is empty or leaves the image, TypeError for one that is not four integers.
    scale (1, 2, 4 or 8; 1: all of the above): the window of scaled_box=, a box in pixels of the image decoded at that scale,
    ceil(width / scale) x ceil(height / scale), whose MCUs cover 8 hs / scale x 8 vs / scale scaled pixels.  The chroma follows libjpeg
    at that scale: 4:4:4 and 4:2:0 chroma comes out of its inverse DCT at luma resolution (the pixel's own MCU alone); 4:2:2 chroma is
    up-sampled h2v1 fancy at scales 2 and 4 when the scaled chroma plane is more than 2 wide (one neighbour column after the clamps)
    and replicated otherwise; 4:4:0 chroma is up-sampled h1v2 fancy at scales 2 and 4 (one neighbour row) and replicated at scale 8.
    The C twin is aej_jpegdec_sbox_window_host."""
    box = _check_decode_box(box, "decode_box_window")
    width, height, hs, vs, ncomp = int(width), int(height), int(hs), int(vs), int(ncomp)
    if width < 1 or height < 1 or ncomp not in (1, 3) or (ncomp == 3 and (hs not in (1, 2) or vs not in (1, 2))):
        raise ValueError(f"decode_box_window: a {width} x {height} file of {ncomp} components sampled {hs} x {vs}")
    scale = _check_scale(scale)
    if scale != 1:
        ow, oh, m = -(-width // scale), -(-height // scale), 8 // scale
        _box_in_image(box, ow, oh, 0)
        if ncomp == 1:
            hs = vs = 1
        l, t, r, b = box
        mx0, mx1, my0, my1 = l // (hs * m), (r - 1) // (hs * m) + 1, t // (vs * m), (b - 1) // (vs * m) + 1
        if ncomp == 3 and not luma and hs != vs and scale != 8:
            def reach(a0, a1, nc):                   # first and last chroma sample the fancy filter reads for luma samples a0 .. a1
                j0, j1 = a0 >> 1, a1 >> 1
                return j0 - (1 if a0 % 2 == 0 and j0 > 0 else 0), j1 + (1 if a1 % 2 == 1 and j1 < nc - 1 else 0)
            if hs == 2 and (ow + 1) // 2 > 2:
                j0, j1 = reach(l, r - 1, (ow + 1) // 2)
                mx0, mx1 = min(mx0, j0 // m), max(mx1, j1 // m + 1)
            elif vs == 2:
                i0, i1 = reach(t, b - 1, (oh + 1) // 2)
                my0, my1 = min(my0, i0 // m), max(my1, i1 // m + 1)
        return mx0, my0, mx1, my1
    _box_in_image(box, width, height, 0)
    if ncomp == 1:
        hs = vs = 1
    l, t, r, b = box
    mx0, mx1, my0, my1 = l // (8 * hs), (r - 1) // (8 * hs) + 1, t // (8 * vs), (b - 1) // (8 * vs) + 1
    if ncomp == 3 and not luma:
        wc, hc = -(-width // hs), -(-height // vs)
        fancy = not (hs == 2 and wc <= 2)

        def span(a0, a1, f, nc):                     # first and last chroma sample read for luma samples a0 .. a1 of one axis
            if f == 1:
                return a0, a1
            j0, j1 = a0 >> 1, a1 >> 1
            if fancy:
                j0 -= 1 if a0 % 2 == 0 and j0 > 0 else 0
                j1 += 1 if a1 % 2 == 1 and j1 < nc - 1 else 0
            return j0, j1

        j0, j1 = span(l, r - 1, hs, wc)
        i0, i1 = span(t, b - 1, vs, hc)
        mx0, mx1, my0, my1 = min(mx0, j0 // 8), max(mx1, j1 // 8 + 1), min(my0, i0 // 8), max(my1, i1 // 8 + 1)
    return mx0, my0, mx1, my1


def decode_box_stats(device: int = 0):
    """(segments_total, segments_decoded, coef_blocks) of the last standard_jpeg_decode_many with a box or a scaled_box (or
    standard_jpeg_resized_crop_many, whose decode is one) on this device's current
    stream that had baseline files (aej_jpegdec_box_stats), summed over those files: their restart segments, the ones that were
    Huffman-decoded (those holding an MCU of the window's MCU rows; every one of a file without a box) and the coefficient blocks
    stored.  Computed on the host from the headers and the windows: nothing is read back."""
    ctx = get_context(device)
    out = (ctypes.c_int64 * 3)()
    ctx.check(ctx.lib.aej_jpegdec_box_stats(ctx.handle, ctypes.addressof(out)))
    return int(out[0]), int(out[1]), int(out[2])


def _views(out, out_off, shapes, comps):
    """the images of a packed decode: [h, w, 3], [h, w] where comps says 1, or [h, w, 4] where it says 4"""
    return packed_views(out, out_off, [(h, w) if c == 1 else (h, w, c) for (h, w), c in zip(shapes, comps)])


def draft_scale(width: int, height: int, size) -> int:
    """The scale ``Image.draft(None, size)`` picks for a width x height JPEG file (host only): the largest of 8, 4, 2, 1 that is not above
    ``min(width // size[0], height // size[1])`` -- the smallest decode that is still at least ``size`` (width, height) large, which is
    how ``Image.thumbnail()`` chooses.  Pass it as ``scale=`` of standard_jpeg_decode_many.  ValueError for a size that is not positive."""
    w, h = int(size[0]), int(size[1])
    if w < 1 or h < 1 or int(width) < 1 or int(height) < 1:
        raise ValueError(f"draft_scale: {width} x {height} file, size {tuple(size)!r}: positive sizes required")
    ratio = min(int(width) // w, int(height) // h)
    return next((s for s in (8, 4, 2) if s <= ratio), 1)


def standard_jpeg_decode_many(files, device: int = 0, progressive: bool = False, scale=1, layout_440: bool = False, mode="RGB", box=None,
                              adobe: bool = False, scaled_box=None) -> list:
    """Decode JPEG files on the device: -> list of uint8 [H_i, W_i, 3] tensors (views into one packed allocation), in input
    order, on the context of the current stream; element i equals ``np.asarray(Image.open(io.BytesIO(files[i])).convert("RGB"))``.
    scale: 1, 2, 4 or 8, or a sequence of one such value per file (ValueError naming the value otherwise; a bool is refused): file i
    is decoded at 1 / scale of its size from its coefficients (reduced inverse DCTs, no full-size image in between) and element i is
    the [ceil(H_i / s), ceil(W_i / s), 3] image Pillow gives after ``im.draft("RGB", (W_i // s, H_i // s))`` has chosen scale s
    (draft_scale is that choice).  scale=1 is the call as it always was.
    files: a sequence of bytes-like .jpg contents, of any sizes and of the supported layouts mixed (4:2:0, 4:2:2, 4:4:4, grey).
    Baseline files always; with ``progressive=True`` also progressive (SOF2) files whose scans complete every coefficient, mixed
    freely with baseline ones (csrc/jpegprog.hip, ``aej_jpegprog_*``) -- without it a progressive file is refused as before.  Every
    header -- of a progressive file every marker up to EOI -- is read on the host before any device work (NotImplementedError /
    ValueError naming the file); the scans cross in one copy per kind and are un-stuffed, Huffman-decoded and reconstructed on the
    device.  A file whose scan is malformed raises ValueError naming its index and the reason (the per-file status words are read back
    once per kind).  There is no CPU fallback.
    layout_440=True (TypeError for a value that is not a bool) also takes 4:4:0 files -- three components, luma sampled 1 x 2 over 1 x 1
    chroma, what ``jpegtran -rotate 90`` makes of a 4:2:2 photo -- baseline or progressive, at every scale, mixed freely with the other
    layouts; without it such a file is refused as before (NotImplementedError, "sampling factors 1x2,...").
    mode: "RGB" (the default: the call as it always was), "L", "auto", or a list / tuple of one of them per file.  "L": element i is
    uint8 [h, w] -- a one-component file's samples, a colour file's LUMA PLANE: what Pillow gives after ``im.draft("L", (W_i // s,
    H_i // s))`` (libjpeg's out_color_space = JCS_GRAYSCALE), at every scale, for every layout, baseline and progressive.  This is NOT
    ``im.convert("L")``: no ITU-R 601 weighting of the clamped R, G, B -- the two differ by several levels where the chroma is strong.
    The chroma blocks of such a file are entropy-decoded (the scan interleaves them) and then never touched: no chroma IDCT, no
    up-sampling, no colour conversion, a third of the output bytes.  "auto": each file in Pillow's own mode, ``np.asarray(Image.open(f))``
    -- [h, w] for a one-component file, [h, w, 3] for a colour one.  The images stay views into one packed allocation (h * w bytes of an
    L image, h * w * 3 of an RGB one).  A string that is not one of the three, or a sequence of another length than files, raises
    ValueError (naming the file of a bad entry); a value that is neither a string nor a list / tuple TypeError -- before any device
    work, like every keyword here.
    box: None (the default: the call as it always was -- NULL boxes, the same launches), one (left, top, right, bottom)
    for every file, or a list with one entry per file, each such a tuple or None (the whole image).  Pillow's crop() coordinates, in
    pixels of the decoded image, 0 <= left < right <= W_i and 0 <= top < bottom <= H_i.  Element i is then uint8 [bottom - top,
    right - left, 3] -- [bottom - top, right - left] where mode makes it one-channel -- and equals ``np.asarray(Image.open(f)
    .convert("RGB").crop(box))`` (for "L": the ``draft("L", None)`` image cropped), i.e. ``[top:bottom, left:right]`` of what the call
    returns without box=: a box edge inside the picture is filtered with its real neighbours from outside the box.  Only what the box
    needs is done (csrc/jpegdec.hip, ``k_jd_sbox<0>``; ``decode_box_window`` is the MCU window, ``decode_box_stats`` what the last call
    skipped): of a baseline file only the restart segments that hold MCUs of the window's MCU rows are Huffman-decoded and only those
    rows' coefficients are stored; one kernel reconstructs the box's tiles from the coefficients, with no sample planes.  A progressive
    file keeps its whole entropy decode and gets the boxed reconstruction.  Works with progressive=True, layout_440=True and every
    mode; boxed and unboxed files, every kind and layout mix in one call.  Refusals, before any device work: a box that is empty,
    inverted or leaves the image ValueError naming the file (Pillow would pad with black; that is not built); a bool, a float or a
    tuple of another length TypeError; a list of another length than files ValueError; a box on a file whose scale is not 1
    NotImplementedError ("a box at scale 2, 4 or 8 is not built").  ERRORS IN SKIPPED DATA: a boxed decode reports scan errors only
    for the data it reads -- a malformed restart segment that the box does not need is not noticed, where the call without box=
    raises.
    adobe=True (TypeError for a value that is not a bool; without it every call is as it always was, every refusal included) also
    takes the files libjpeg reads under another colour model, baseline or -- with progressive=True -- progressive, mixed freely with
    the others: four components as CMYK (no Adobe APP14 marker, or one with transform 0) or YCCK (transform 2; any other transform
    NotImplementedError), and three components coded as RGB (no JFIF marker, and APP14 transform 0 or the component ids 'R','G','B':
    what ``save(..., keep_rgb=True)`` writes).  Components 1 and 2 sampled 1 x 1, component 0 as for YCbCr files, component 3 as
    component 0 (Photoshop: K at full resolution, up to 10 blocks per MCU) or 1 x 1 (Pillow's subsampling=1 / 2: K is up-sampled with
    the chroma, by the same rules).  mode="auto" gives such a file in Pillow's own mode: uint8 [H, W, 4] equal to
    ``np.asarray(Image.open(f))`` (mode "CMYK": 255 - sample; for YCCK libjpeg's YCbCr -> RGB of components 0..2 and 255 - K) for
    four components, [H, W, 3] (the samples) for an RGB-coded one.  mode="RGB" gives [H, W, 3] for every file: of a four-component one
    Pillow's ``.convert("RGB")`` of that CMYK image, in its integer arithmetic.  Not built, NotImplementedError naming the file before
    any device work: mode="L", a scale other than 1 or a box for one of these files ("... of a four-component / RGB-coded file is
    not built").  The thumbnail, transcode, transform and encode calls have no such keyword and refuse these files as before.
    scaled_box: box= in pixels of each file's SCALED image, [ceil(H_i / s_i), ceil(W_i / s_i)] -- Pillow's crop() box of the drafted
    image -- so that it works at scale 2, 4 and 8: one box for every file, or one box or None per file.  Element i equals
    ``[top:bottom, left:right]`` of the same call without the keyword.  Only the box's tiles are reconstructed, from the reduced inverse
    DCTs (csrc/jpegdec.hip, ``k_jd_sbox``; ``decode_box_window(..., scale=s)`` is the MCU window), and the restart-segment skip and the
    coefficient window of box= apply to baseline files as they do there.  At scale 1 it is box=.  The checks and error words are
    those of box=, against the scaled image's size; giving both box= and scaled_box= raises ValueError; box= at scale 2, 4 or 8 still
    raises NotImplementedError."""
    files = list(files)
    if not files:
        raise ValueError("standard_jpeg_decode_many needs at least one file")
    modes = _check_modes(mode, len(files))
    if box is not None and scaled_box is not None:
        raise ValueError("box= and scaled_box= are both given: one of them (box= is in full-size pixels, scaled_box= in pixels of the scaled image)")
    _, out, out_off, shapes, comps = _decode_files(files, device, progressive, _check_scales(scale, len(files)),
                                                   layout_440=_check_bool("layout_440", layout_440), modes=modes,
                                                   boxes=_check_boxes(box, len(files)), adobe=_check_bool("adobe", adobe),
                                                   sboxes=_check_boxes(scaled_box, len(files)))
    return _views(out, out_off, shapes, comps)


def _decode_files(files, device, progressive, scales, choose=None, layout_440=False, modes=None, boxes=None, adobe=False, sboxes=None):
    """The decode of standard_jpeg_decode_many -> (context, the packed uint8 output, int64 offsets, [(h, w)], [3 or 1: the channels of
    each image]).  scales: int32 [n]; with `choose`, file i's scale is choose(i, width, height) instead, asked once its header
    is parsed and before any device work.  modes: _check_modes' list (None: every file "RGB").  boxes: _check_boxes' list (None: no
    file has one); the shape of a boxed file is its box's.  adobe: the parsers' keyword; a four-component file that leaves in mode
    "CMYK" has 4 channels.  sboxes (not together with boxes): the same list with every box in pixels of its file's scaled image; an
    entry may be set by `choose`, which is asked first."""
    n = len(files)
    src, shapes, comps, box_arr = _Sources(), [], [], None
    sbox = sboxes is not None
    if sbox:
        boxes = sboxes
    for i, frame, _ in src.parse(files, progressive, layout_440=layout_440, adobe=adobe):
        m = "RGB" if modes is None else modes[i]
        comps.append(1 if m == "L" or (m == "auto" and frame.ncomp == 1) else 4 if m == "auto" and frame.ncomp == 4 else 3)
        if choose is not None:
            scales[i] = choose(i, frame.width, frame.height)
        s = int(scales[i])
        if adobe and frame.colour != "YCbCr":            # the new kinds: full size, whole, in colour
            whole = boxes is None or boxes[i] is None or boxes[i] == ((0, 0, -(-frame.width // s), -(-frame.height // s)) if sbox else (0, 0, frame.width, frame.height))
            what = "mode 'L'" if m == "L" else "a scale other than 1" if s != 1 else None if whole else "a box"
            if what:
                raise NotImplementedError(f"file {i}: {what} of a four-component / RGB-coded file is not built")
        shapes.append((-(-frame.height // s), -(-frame.width // s)))
        if boxes is not None and boxes[i] is not None:
            bw, bh = (shapes[-1][1], shapes[-1][0]) if sbox else (frame.width, frame.height)      # the image the box is a box of
            _box_in_image(boxes[i], bw, bh, i)
            if boxes[i] == (0, 0, bw, bh):
                continue                                 # the whole image: no box
            if s != 1 and not sbox:
                raise NotImplementedError(f"file {i}: a box at scale 2, 4 or 8 is not built")
            box_arr = np.zeros((n, 4), np.int32) if box_arr is None else box_arr
            box_arr[i] = boxes[i]
            shapes[-1] = (boxes[i][3] - boxes[i][1], boxes[i][2] - boxes[i][0])
    if box_arr is not None:                          # a call with boxes: every other file's is its whole image
        for i, frame in enumerate(src.frames):
            if not box_arr[i].any():
                s = int(scales[i]) if sbox else 1
                box_arr[i] = (0, 0, -(-frame.width // s), -(-frame.height // s))
    if (scales == 1).all():
        scales = None                                # every file at full size: NULL
    comps_arr = None if all(c == 3 for c in comps) else np.array(comps, np.int32)      # every image RGB: NULL
    ctx = get_context(device)
    t = ctx.torch
    out_off = np.zeros(n, np.int64)
    opos = 0
    for i, (h, w) in enumerate(shapes):
        out_off[i] = opos
        opos += h * w * comps[i]
    out = ctx.empty((max(opos, 1),), t.uint8)
    st = np.zeros(n, np.int64)
    for idx, prog in ((src.base_idx, False), (src.prog_idx, True)):      # one staging copy and one entry per kind
        if idx:
            st[idx] = _decode_kind(ctx, src, prog, out, out_off, scales, comps_arr, box_arr,
                                   sbox and box_arr is not None).cpu().numpy()      # the one read-back of the per-file status words
    _raise_status((int(i), int(st[i])) for i in np.flatnonzero(st))
    return ctx, out, out_off, shapes, comps


def _thumbnail_size(width, height, size):
    """Image.thumbnail's preserve_aspect_ratio: the final (w, h), or None when the request covers the image"""
    import math
    x, y = math.floor(size[0]), math.floor(size[1])
    if x >= width and y >= height:
        return None

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = width / height
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def thumbnail_plan(width: int, height: int, size, reducing_gap=2.0):
    """What ``Image.thumbnail(size, reducing_gap=reducing_gap)`` does to a width x height JPEG file (host only): None when the request
    covers the image (it stays as it is), otherwise ``(scale, (fx, fy), final_size, box)``: the scale ``draft()`` decodes at (1 without
    a reducing_gap), the whole factors ``resize`` reduces the decoded image by first, the aspect-preserving final (w, h), and the box
    (0, 0, width / scale, height / scale) -- fractional -- that the decoded image is resampled over.  When the decoded size already
    equals final_size nothing follows the decode and the factors are (1, 1)."""
    from .resample import _check_gap, _check_size, reduce_factors
    size, gap = _check_size(size, "thumbnail_plan", integers=False), _check_gap(reducing_gap, "thumbnail_plan")
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f"thumbnail_plan: a {width} x {height} file: positive sizes required")
    final = _thumbnail_size(width, height, size)
    if final is None:
        return None
    s = 1
    if gap is not None:
        want = (int(size[0] * gap), int(size[1] * gap))
        ratio = min(width // want[0], height // want[1]) if want[0] > 0 and want[1] > 0 else 0
        s = next((v for v in (8, 4, 2) if v <= ratio), 1)
    box = (0, 0, width / s, height / s)
    if (-(-width // s), -(-height // s)) == final:
        return s, (1, 1), final, box
    return s, reduce_factors(box, final, gap), final, box


def _check_crop_box(b, who):
    """one crop box of the resized-crop calls -> (l, t, r, b) of numbers; TypeError for anything that is not a list / tuple of four
    finite numbers (a bool is none)"""
    if not isinstance(b, (list, tuple)) or len(b) != 4:
        raise TypeError(f"{who}: box {b!r}: (left, top, right, bottom) required")
    if not all(is_number(v) and math.isfinite(v) for v in b):
        raise TypeError(f"{who}: box {tuple(b)!r}: four finite numbers required")
    return tuple(v.item() if isinstance(v, np.generic) else v for v in b)


def resized_crop_plan(width: int, height: int, box, size, resample="bilinear", reducing_gap=None, what: str = "resized_crop_plan"):
    """What standard_jpeg_resized_crop_many does with one width x height file (host only).  box = (l, t, r, b) in full-size pixels,
    fractions allowed, 0 <= l < r <= width and 0 <= t < b <= height (ValueError otherwise; TypeError for anything but four numbers);
    size = (w, h).  -> dict with
    scale: 1 when reducing_gap is None, otherwise the largest of 8, 4, 2, 1 that does not exceed ``min(int(r - l) // int(w * g),
        int(b - t) // int(h * g))`` (1 when a divisor is 0) -- thumbnail_plan's rule with the box's size in the place of the image's;
    box: (l / s, t / s, r / s, b / s), the box resize() is given on the image decoded at that scale, ceil(width / s) x ceil(height / s);
    factors, reduce_box: the whole factors resize() reduces by first under reducing_gap and the region it reduces ((1, 1): none);
    window: (x0, y0, x1, y1), the integer rectangle of the scaled image that is read: the reduce box where there is a reduce, else
        per axis from the first tap of the first output pixel to the end of the last output pixel's taps (resample_taps' bounds);
    step: resize_many's own description of the resize (box in the coordinates the reduce leaves)."""
    from . import resample as RS
    f, gap, (w, h) = RS._check_filter(resample, what), RS._check_gap(reducing_gap, what), RS._check_size(size, what)
    l, t, r, b = box = _check_crop_box(box, what)
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f"{what}: a {width} x {height} file: positive sizes required")
    if not (0 <= l < r <= width and 0 <= t < b <= height):
        raise ValueError(f"{what}: box {box!r} is empty, inverted or leaves the {width} x {height} image (nothing is padded)")
    s = 1
    if gap is not None:
        dw, dh = int(w * gap), int(h * gap)
        ratio = min(int(r - l) // dw, int(b - t) // dh) if dw > 0 and dh > 0 else 0
        s = next((v for v in (8, 4, 2) if v <= ratio), 1)
    ow, oh = -(-width // s), -(-height // s)
    sbox = (l / s, t / s, r / s, b / s)
    step = RS._steps(what, ow, oh, (w, h), sbox, f, gap)
    if step["factors"] != (1, 1):
        window = tuple(int(v) for v in step["reduce_box"])
    else:
        (x0, x1), (y0, y1) = RS._tap_hull(ow, step["box"][0], step["box"][2], w, f), RS._tap_hull(oh, step["box"][1], step["box"][3], h, f)
        window = (x0, y0, x1, y1)
    return dict(scale=s, box=sbox, factors=step["factors"], reduce_box=step["reduce_box"], window=window, step=step)


def standard_jpeg_resized_crop_many(files, box, size, resample="bilinear", reducing_gap=None, progressive: bool = False,
                                    layout_440: bool = False, mode: str = "RGB", device: int = 0):
    """Decode a box of each JPEG file and resize it to one size, on the device -- RandomResizedCrop's decode, a tile pyramid's, a region
    preview's: -> ONE uint8 tensor [N, h, w, 3] ([N, h, w] under mode="L").  box: one (l, t, r, b) for every file or a list of one per
    file, in full-size pixels, fractions allowed, inside the image (nothing is padded).  size: one (w, h).  resample: one of the five
    filters of resize_many ("nearest" is not built).  Per file (resized_crop_plan): the scale s_i the reducing_gap allows for the
    box's size (1 without one), then element i equals ``resize_many([standard_jpeg_decode_many([f_i], scale=s_i, ...)[0]], size,
    resample, box=box_i / s_i, reducing_gap=reducing_gap)[0]`` -- in Pillow's words the image drafted at scale s_i, then
    ``.convert("RGB").resize(size, F, box=box_i / s_i, reducing_gap=g)``; with the defaults ``Image.open(f).convert("RGB")
    .resize(size, F, box=box)``.  Only the window of the scaled image that the resize reads is ever reconstructed: one decode with
    scaled_box= each file's plan window, then one resample that reads those windows in place under the whole image's tap tables
    (``aej_resample_batch_win``; at most three launches).  Nothing is read back except the decoder's status words.
    progressive / layout_440: as standard_jpeg_decode_many.  mode: "RGB" or "L" (the luma plane, as there); "auto" is refused
    (ValueError): one tensor has one channel count.  TypeError for a box that is not four numbers, ValueError naming the file for a
    list of another length than files or a box outside its image, before any device work."""
    from . import resample as RS
    layout_440 = _check_bool("layout_440", layout_440)
    files = list(files)
    n = len(files)
    if n < 1:
        raise ValueError("standard_jpeg_resized_crop_many needs at least one file")
    if not isinstance(mode, str):
        raise TypeError(f"mode {mode!r}: 'RGB' or 'L' required")
    if mode not in ("RGB", "L"):
        raise ValueError(f"mode {mode!r}: 'RGB' or 'L' required" + (" ('auto' would mix channel counts in the one tensor returned)" if mode == "auto" else ""))
    f, gap = RS._check_filter(resample, "every file"), RS._check_gap(reducing_gap, "every file")
    w, h = RS._check_size(size, "standard_jpeg_resized_crop_many")
    if not isinstance(box, (list, tuple)):
        raise TypeError(f"box {box!r}: (left, top, right, bottom), or a list of one such tuple per file, required")
    if len(box) > 0 and all(isinstance(b, (list, tuple)) for b in box):
        if len(box) != n:
            raise ValueError(f"box: {len(box)} entries for {n} files")
        boxes = [_check_crop_box(b, f"file {i}") for i, b in enumerate(box)]
    else:
        boxes = [_check_crop_box(box, "every file")] * n
    plans, sboxes = [None] * n, [None] * n

    def choose(i, width, height):
        plans[i] = p = resized_crop_plan(width, height, boxes[i], (w, h), f, gap, f"file {i}")
        sboxes[i] = p["window"]
        return p["scale"]

    ctx, out, out_off, shapes, comps = _decode_files(files, device, progressive, np.ones(n, np.int32), choose, layout_440, [mode] * n, sboxes=sboxes)
    steps, windows = [], np.zeros((n, 4), np.int32)
    for i, p in enumerate(plans):
        x0, y0, x1, y1 = p["window"]
        steps.append(dict(p["step"], src=(x1 - x0, y1 - y0)))      # the stored rectangle; the virtual image is the whole scaled one
        windows[i] = (x0, y0) + p["step"]["src"]
    res = RS._run(ctx, out.data_ptr(), out.numel(), out_off, steps, [f] * n, comps, windows=windows, packed=True)
    return res.view(*((n, h, w) + ((3,) if mode == "RGB" else ())))


def standard_jpeg_thumbnail_many(files, size, resample="bicubic", reducing_gap=2.0, progressive: bool = False, device: int = 0,
                                 layout_440: bool = False, mode="RGB") -> list:
    """``Image.thumbnail`` on JPEG files, on the device: -> list of uint8 [h_i, w_i, 3] tensors, views into one packed allocation;
    element i equals ``im = Image.open(io.BytesIO(files[i])); im.thumbnail(size_i, F, reducing_gap=reducing_gap);
    np.asarray(im.convert("RGB"))``.  Per file (thumbnail_plan): the aspect-preserving final size; the decode at the scale ``draft()``
    picks for ``size * reducing_gap`` (standard_jpeg_decode_many's scaled decode); then ``resize`` to the final size over the fractional
    box draft() returns, with its own reducing_gap step (resample.py, csrc/resample.hip).  A file the request covers comes back at
    full size.  Nothing but the decoder's status words is read back.  A tensor whose file has a COM segment carries its text as the
    attribute ``jpeg_comment`` (bytes), as Pillow keeps ``im.info["comment"]``; standard_jpeg_encode_many writes it again, as Pillow's save does.
    size: one (w, h), or one per file.  resample (one, or a list of one per file) / reducing_gap: as resize_many (reducing_gap=None: full-size decode, one resize).
    files / progressive / layout_440: as standard_jpeg_decode_many, which refuses what this refuses, with the same words.
    mode: standard_jpeg_decode_many's ("RGB", the default: the call as it always was).  An image that "L" or "auto" makes one-channel
    is uint8 [h_i, w_i]: the same plan -- scale, factors, box, final size -- run on the one-channel decode and the one-channel resize.
    For a one-component file that is ``im.thumbnail(size_i, F, reducing_gap=reducing_gap); np.asarray(im)``, a mode-"L" image.  For a
    colour file under "L" it is the thumbnail Pillow makes when the file's ONE draft() call asks for mode "L" (thumbnail()'s own draft
    does nothing after a first one): with ``plan = thumbnail_plan(W, H, size, g)``, the full-size ``im.draft("L", None)`` image when
    plan is None, otherwise ``res = im.draft("L", (int(size[0] * g), int(size[1] * g)))`` (``im.draft("L", None)`` when g is None) and
    then, if ``im.size != plan[2]``, ``im.resize(plan[2], F, box=res[1], reducing_gap=g)``.  Luma, not ``convert("L")``."""
    from . import resample as RS
    layout_440 = _check_bool("layout_440", layout_440)
    files = list(files)
    n = len(files)
    if n < 1:
        raise ValueError("standard_jpeg_thumbnail_many needs at least one file")
    modes = _check_modes(mode, n)
    f, gap = one_or_each(resample, n, RS._check_filter, "resample", "file"), RS._check_gap(reducing_gap, "every file")
    if not isinstance(size, (str, bytes)) and hasattr(size, "__len__") and len(size) == 2 and not any(hasattr(v, "__len__") for v in size):
        sizes = [RS._check_size(size, "standard_jpeg_thumbnail_many", integers=False)] * n
    else:
        if isinstance(size, (str, bytes)) or not hasattr(size, "__len__") or len(size) != n:
            raise ValueError(f"size {size!r}: one (width, height), or one per file ({n}), required")
        sizes = [RS._check_size(v, f"file {i}", integers=False) for i, v in enumerate(size)]
    steps = [None] * n

    def choose(i, width, height):
        plan = thumbnail_plan(width, height, sizes[i], gap)
        s, final, box = (1, (width, height), None) if plan is None else (plan[0], plan[2], plan[3])
        dw, dh = -(-width // s), -(-height // s)
        if (dw, dh) == final:
            box = None                               # unchanged, or the drafted size is the final one: a copy
        steps[i] = RS._steps(f"file {i}", dw, dh, final, box, f[i], gap)
        return s

    ctx, out, out_off, shapes, comps = _decode_files(files, device, progressive, np.ones(n, np.int32), choose, layout_440, modes)
    if all(st["src"] == st["dst"] and st["box"] == (0, 0) + st["src"] for st in steps):
        res = _views(out, out_off, shapes, comps)
    else:
        res = RS._run(ctx, out.data_ptr(), out.numel(), out_off, steps, f, comps)
    for i, t in enumerate(res):                      # what Pillow keeps in im.info["comment"] over thumbnail(): see standard_jpeg_encode_many
        com = _jpeg_comment(files[i], i)
        if com is not None:
            t.jpeg_comment = com
    return res


def _jpeg_comment(data, index):
    """the payload of the last COM segment before the first scan of one file (Pillow's ``im.info["comment"]``), or None"""
    mv = memoryview(data).cast("B")
    try:
        com = [bytes(mv[a + 4:b]) for m, a, b in marker_segments(mv, index) if m == 0xFE]
    except ValueError:
        return None
    return com[-1] if com else None


def decode_sync_rounds(device: int = 0) -> int:
    """Sync rounds of the Huffman decode that the last standard_jpeg_decode_many on this device's current stream ran
    (aej_jpegdec_sync_rounds): 0 when every segment fit one subsequence."""
    ctx = get_context(device)
    return int(ctx.lib.aej_jpegdec_sync_rounds(ctx.handle))


# ---- lossless transcode -------------------------------------------------------------------------------------------------------------
def marker_segments(data, index: int = 0):
    """[(marker, start, end)] of the marker segments between SOI and the first SOS of one file: data[start:end] is the whole segment,
    FF xx and its length included (host only).  ValueError naming the file for bytes that are not such a sequence."""
    mv = memoryview(data).cast("B")
    n, i, out = len(mv), 2, []
    if n < 4 or mv[0] != 0xFF or mv[1] != 0xD8:
        raise ValueError(f"file {index}: no SOI marker")
    while True:
        if i + 4 > n or mv[i] != 0xFF:
            raise ValueError(f"file {index}: marker expected at byte {i}")
        m = mv[i + 1]
        if m == 0xFF:                              # fill byte
            i += 1
            continue
        if m == 0xDA:
            return out
        if m == 0x01 or 0xD0 <= m <= 0xD9:
            raise ValueError(f"file {index}: marker FF{m:02X} before SOS")
        length = (mv[i + 2] << 8) | mv[i + 3]
        if length < 2 or i + 2 + length > n:
            raise ValueError(f"file {index}: truncated segment FF{m:02X}")
        out.append((m, i, i + 2 + length))
        i += 2 + length


def _jfif_density(mv, segs):
    """(units, Xdensity, Ydensity) of the source's JFIF APP0; (0, 1, 1) -- what Pillow writes without dpi= -- when it has none"""
    for m, a, b in segs:
        if m == 0xE0 and b - a >= 16 and bytes(mv[a + 4:a + 9]) == b"JFIF\0":
            return mv[a + 11], (mv[a + 12] << 8) | mv[a + 13], (mv[a + 14] << 8) | mv[a + 15]
    return 0, 1, 1


def _is_metadata(m) -> bool:
    return 0xE1 <= m <= 0xED or m == 0xEF or m == 0xFE


def metadata_segments(data, index: int = 0) -> bytes:
    """What keep_metadata=True carries over: the file's APP1 .. APP13, APP15 and COM segments, verbatim and in order.  APP0 (JFIF,
    JFXX: the output has its own) and APP14 (Adobe: the output is a JFIF file) never are."""
    mv = memoryview(data).cast("B")
    return b"".join(bytes(mv[a:b]) for m, a, b in marker_segments(mv, index) if _is_metadata(m))


def _prefix(data, index, progressive, transform, trim, grey, layout_440, box=None, drop=False):
    """transcode_prefix (the transform "none", whose geometry refuses no file the parsers took) and transform_prefix, both through
    aej_jfif_transform_headers_host_cut; box (or None) and drop: transform_prefix's crop and drop_chroma"""
    from ._lib import load_library
    (_, is_prog, _, frame, mv), = _parse_sources([data], transcoder=True, start=index, grey=_check_bool("grey", grey), layout_440=layout_440)
    _transform_geometry(index, frame, _check_transform(transform, index), trim, layout_440, box, drop)
    dens = (ctypes.c_uint16 * 3)(*_jfif_density(mv, marker_segments(mv, index)))
    buf = (ctypes.c_uint8 * 512)()
    b4 = None if box is None else (ctypes.c_int32 * 4)(*box)
    n = load_library().aej_jfif_transform_headers_host_cut(
        None if is_prog else ctypes.addressof(frame), ctypes.addressof(frame) if is_prog else None, ctypes.addressof(dens), int(progressive),
        TRANSFORMS.index(transform), int(trim), int(layout_440), None if b4 is None else ctypes.addressof(b4), int(drop),
        ctypes.addressof(buf), 512)
    if n < 0:
        raise ValueError(f"file {index}: the library refuses its descriptor ({n})")
    return bytes(buf[:n])


def transcode_prefix(data, progressive: bool = False, index: int = 0, grey: bool = False, layout_440: bool = False) -> bytes:
    """The bytes SOI .. end of SOF0 / SOF2 that standard_jpeg_transcode_many writes for one file (aej_jfif_transform_headers_host_cut
    with the code 0, no crop and no chroma drop, host only): JFIF APP0 with the source's density, its quantisation tables, its frame
    header.  grey, layout_440: as standard_jpeg_transcode_many."""
    progressive = _check_bool("progressive", progressive)
    return _prefix(data, index, progressive, "none", False, grey, _check_bool("layout_440", layout_440))


def splice_metadata(out: bytes, meta: bytes) -> bytes:
    """`meta` (metadata_segments) right after the JFIF APP0 of a file this library wrote: SOI (2 bytes) and APP0 (18) come first"""
    return out[:20] + meta + out[20:] if meta else out


_last_transcode_groups = 0


def transcode_groups() -> int:
    """Entropy-encode chains the last successful standard_jpeg_transcode_many of this process ran: one per distinct (height, width,
    sampling, components) among its files.  A diagnostic for tests and tools, nothing to build on: one module-level value for every device and
    thread, which a call that raises leaves as it was."""
    return _last_transcode_groups


TRANSFORMS = ("none", "flip_h", "flip_v", "transpose", "transverse", "rot90", "rot180", "rot270")      # codes 0..7: jpegtran's JXFORM order
_EXIF_TRANSFORM = (None, "none", "flip_h", "rot180", "flip_v", "transpose", "rot90", "transverse", "rot270")      # by Orientation value
_TRANSPOSING = ("transpose", "transverse", "rot90", "rot270")


def _exif_orientation_at(mv, segs):
    """(value, offset of its two bytes in the file, byte order) of the Orientation tag (0x0112, one SHORT) in IFD0 of the first EXIF
    APP1 segment; None when there is no such segment or tag or the block is malformed"""
    for m, a, b in segs:
        if m != 0xE1 or b - a < 10 or bytes(mv[a + 4:a + 10]) != b"Exif\0\0":
            continue
        t = a + 10                                  # the TIFF header; offsets count from here and must stay inside the segment
        if b - t < 8:
            return None
        order = {b"II*\0": "little", b"MM\0*": "big"}.get(bytes(mv[t:t + 4]))
        if order is None:
            return None
        num = lambda o, k: int.from_bytes(bytes(mv[o:o + k]), order)  # noqa: E731
        ifd = t + num(t + 4, 4)
        if ifd + 2 > b:
            return None
        for e in range(ifd + 2, ifd + 2 + 12 * num(ifd, 2), 12):
            if e + 12 > b:
                return None
            if num(e, 2) == 0x0112:
                return (num(e + 8, 2), e + 8, order) if num(e + 2, 2) == 3 and num(e + 4, 4) == 1 else None
        return None
    return None


def exif_orientation(data, index: int = 0) -> int:
    """The EXIF Orientation tag of one file (host only): 1..8 as ``Image.open(f).getexif().get(0x0112, 1)`` gives it; 1 when the file
    has no EXIF APP1 segment, no such tag in IFD0, a malformed EXIF block or a value outside 1..8."""
    mv = memoryview(data).cast("B")
    try:
        at = _exif_orientation_at(mv, marker_segments(mv, index))
    except ValueError:
        return 1
    return at[0] if at and 1 <= at[0] <= 8 else 1


def _check_box(box, i):
    """one crop entry -> None or four ints; bool, float and anything that is not four values are refused, naming the file"""
    if box is None:
        return None
    ok = not isinstance(box, (str, bytes)) and hasattr(box, "__len__") and len(box) == 4 and \
        all(is_int(v) for v in box)
    if not ok:
        raise ValueError(f"file {i}: crop {box!r}: (left, upper, right, lower) as four ints, or None, required")
    return tuple(int(v) for v in box)


def _check_crop(crop, n):
    """crop= -> [n] boxes or None: None, one box for every file, or a sequence of one entry (a box or None) per file"""
    if crop is None:
        return [None] * n
    if isinstance(crop, (str, bytes)) or not hasattr(crop, "__len__"):
        raise ValueError(f"file 0: crop {crop!r}: (left, upper, right, lower) as four ints, a sequence of one such box or None per file, or None required")
    entries = list(crop)
    if entries and not any(e is None or hasattr(e, "__len__") for e in entries):      # plain values: one box
        return [_check_box(entries, 0)] * n
    if len(entries) != n:
        raise ValueError(f"file {min(len(entries), n)}: {len(entries)} crop boxes for {n} files")
    return [_check_box(e, i) for i, e in enumerate(entries)]


def _transform_geometry(i, frame, name, trim, layout_440, box=None, drop=False):
    """The geometry of one file's transform, with its crop box (or None) and drop_chroma (aej_jfif_transform_geometry_host_cut) -> the
    output's (height, width, hs, vs) and the crop's aligned corner (L, U); every refusal names the file and comes before any device
    work.  The frame's own component count goes to the entry: a parsed one-component frame carries hs = vs = 1."""
    from ._lib import load_library
    nc = 1 if frame.ncomp == 1 else 3
    one = drop or nc == 1                           # a one-component output: 8 x 8 MCUs, no layout
    if name in _TRANSPOSING and frame.hs != frame.vs and not layout_440 and not one:
        raise NotImplementedError(f"file {i}: {name} of a 4:2:2 file would be a 4:4:0 file, which neither the coders nor the decoders here have")
    out = (ctypes.c_int32 * 6)()
    entry = lambda b: load_library().aej_jfif_transform_geometry_host_cut(  # noqa: E731
        frame.height, frame.width, frame.hs, frame.vs, nc, TRANSFORMS.index(name), int(trim), int(layout_440), b, int(drop), ctypes.addressof(out))
    rc = entry(None)
    mcu = "8 x 8" if one else f"{8 * frame.hs} x {8 * frame.vs}"
    if rc == 1:
        raise ValueError(f"file {i}: {name} of a {frame.width} x {frame.height} file mirrors an axis that is not a whole number of its {mcu} MCUs; "
                         "trim=True drops the partial MCUs at that edge first")
    if rc == 2:
        raise ValueError(f"file {i}: {name} with trim=True leaves nothing of a {frame.width} x {frame.height} file with {mcu} MCUs")
    if rc:
        raise ValueError(f"file {i}: the library refuses the transform ({rc})")
    if box is None:
        return tuple(out)
    h, w = out[0], out[1]
    if not (0 <= box[0] < box[2] <= w and 0 <= box[1] < box[3] <= h):
        raise ValueError(f"file {i}: crop {box} does not lie inside the {w} x {h} image that {name}{' with trim=True' if trim else ''} leaves: "
                         f"0 <= left < right <= {w} and 0 <= upper < lower <= {h} required (boxes are not clamped)")
    cut = (ctypes.c_int32 * 4)(*box)                # (held by a name: an unnamed array is freed as soon as addressof returns, before the entry reads it)
    rc = entry(ctypes.addressof(cut))
    if rc:
        raise ValueError(f"file {i}: the library refuses the crop {box} ({rc})")
    return tuple(out)


def transform_crop_box(data, transform, crop, trim: bool = False, index: int = 0, grey: bool = False, layout_440: bool = False,
                       drop_chroma: bool = False):
    """-> (left, upper, right, lower) that standard_jpeg_transform_many really keeps of one file under one transform name and one crop
    box, in the coordinates of the transformed (and trimmed) image (host only): the box with its upper-left corner moved up and left to
    the output's MCU grid -- 8 hs x 8 vs of the output, 8 x 8 for a one-component one -- as jpegtran -crop moves it.  The file written is
    right - left wide and lower - upper high; an annotation at (x, y) of the transformed image is at (x - left, y - upper) of it.  The
    refusals are standard_jpeg_transform_many's."""
    trim, grey, layout_440 = _check_bool("trim", trim), _check_bool("grey", grey), _check_bool("layout_440", layout_440)
    drop_chroma = _check_bool("drop_chroma", drop_chroma)
    box = _check_box(crop, index)
    if box is None:
        raise ValueError(f"file {index}: crop None: a box required")
    (_, _, _, frame, _), = _parse_sources([data], transcoder=True, start=index, grey=grey, layout_440=layout_440)
    g = _transform_geometry(index, frame, _check_transform(transform, index), trim, layout_440, box, drop_chroma)
    return (g[4], g[5], box[2], box[3])


def _check_transform(name, i):
    if not isinstance(name, str) or name not in TRANSFORMS:
        raise ValueError(f"file {i}: unknown transform {name!r}: one of {', '.join(TRANSFORMS)} required" +
                         (" ('exif' is a setting of the whole call)" if name == "exif" else ""))
    return name


def transform_prefix(data, transform, progressive: bool = False, trim: bool = False, index: int = 0, grey: bool = False,
                     layout_440: bool = False, crop=None, drop_chroma: bool = False) -> bytes:
    """The bytes SOI .. end of SOF0 / SOF2 that standard_jpeg_transform_many writes for one file under one transform name
    (aej_jfif_transform_headers_host_cut, host only): transcode_prefix with the output's size and sampling and, for a transposing
    transform, every quantisation table transposed.  grey, layout_440: as standard_jpeg_transform_many (with layout_440 a transposed
    4:2:2 frame carries the sampling byte 0x12).  crop (one box, or None), drop_chroma: as standard_jpeg_transform_many: the cropped
    size; for a dropped chroma one DQT and the one-component frame header."""
    progressive, trim = _check_bool("progressive", progressive), _check_bool("trim", trim)
    box = _check_box(crop, index)
    drop_chroma, layout_440 = _check_bool("drop_chroma", drop_chroma), _check_bool("layout_440", layout_440)
    return _prefix(data, index, progressive, transform, trim, grey, layout_440, box, drop_chroma)


def standard_jpeg_transform_many(files, transform, progressive: bool = False, trim: bool = False, device: int = 0,
                                 keep_metadata: bool = False, grey: bool = False, restart_marker_blocks: int = 0,
                                 restart_marker_rows: int = 0, layout_440: bool = False, crop=None, drop_chroma: bool = False) -> List[bytes]:
    """Lossless flip, rotation or transposition on the device: standard_jpeg_transcode_many with the files' quantised coefficients
    rearranged between the Huffman decode and the entropy coders (one kernel in the place of the transcoder's bridge), so that no
    sample is quantised a second time -- ``jpegtran -flip / -rotate / -transpose / -transverse``.  files, progressive, device and
    keep_metadata are the transcoder's, and so is what is accepted and refused.

    transform: one name for every file, a sequence of one name per file, or "exif".  With W, H the source size, rotations clockwise:
    "none" out = in; "flip_h" out[y, x] = in[y, W-1-x]; "flip_v" in[H-1-y, x]; "transpose" in[x, y]; "transverse" in[H-1-x, W-1-y];
    "rot90" np.rot90(in, -1); "rot180" in[::-1, ::-1]; "rot270" np.rot90(in, 1).  "exif" takes each file's transform from the
    Orientation tag of its EXIF APP1 segment (exif_orientation; 1..8: none, flip_h, rot180, flip_v, transpose, rot90, transverse,
    rot270 -- PIL.ImageOps.exif_transpose), "none" for a file without a usable tag; with keep_metadata=True it then sets the tag's
    two bytes to 1 in the carried-over segment and changes nothing else in it.  EXIF thumbnails and pixel-dimension tags
    (PixelXDimension, ImageWidth, ...) are NOT rewritten, in no mode; explicit names leave the metadata untouched, as jpegtran does.

    A transposing transform swaps width, height and the luma sampling factors and writes the quantisation tables transposed.  A
    mirrored axis has to be a whole number of the source's MCUs (8 hs x 8 vs): flip_h and rot270 need it of the width, flip_v and
    rot90 of the height, rot180 and transverse of both.  Otherwise trim=False raises ValueError (jpegtran -perfect) and trim=True
    drops the partial MCU column / row at the right / bottom edge first (jpegtran -trim); a dimension that trims to 0 raises
    ValueError.  The padding samples of real edge blocks travel with their block; the dummy blocks of edge MCUs are written as
    libjpeg writes them.  "none" is exactly the transcode.

    grey=True also takes one-component (grey) files, mixed freely with colour ones, "exif" included (TypeError for a value that is not a
    bool; without it such a file is refused as before).  A grey file's MCU is one 8 x 8 block whatever sampling factors its frame header
    carries, so every transform is allowed, a mirrored axis has to be a multiple of 8 and trim=True drops the partial 8-pixel column /
    row; it has no dummy blocks.  Its output is the transcoder's grey file with its one table transposed by a transposing transform.

    restart_marker_blocks, restart_marker_rows: the transcoder's (``jpegtran -restart NB`` / ``-restart N``), counted on the OUTPUT's
    MCU grid; with both 0 the output has no restart markers whatever the source carries.

    layout_440=True (TypeError for a value that is not a bool) takes the 4:4:0 layout on both sides: a transposing transform of a
    4:2:2 source -- "exif" with Orientation 5..8 on a camera's portrait shot -- writes a 4:4:0 file (luma 1 x 2, frame sampling byte
    0x12), one of a 4:4:0 source a 4:2:2 file, and 4:4:0 sources are accepted under every transform; the MCU rules above hold with
    hs, vs = 1, 2.  Such outputs need layout_440=True again to be read back by this library; Pillow and libjpeg read them as they are.

    crop: None, one box for every file, or a sequence of one entry per file, an entry being a box or None -- ``jpegtran -crop``, with
    no second quantisation.  A box is (left, upper, right, lower) as Image.crop takes it, four ints (bool refused), in the coordinates
    of the image AFTER the transform and its trim: the upright image for "exif".  With H', W' that image's size 0 <= left < right <= W'
    and 0 <= upper < lower <= H' are required (ValueError naming the file; boxes are not clamped, and a box reaching into the strip a
    trim dropped is refused).  The upper-left corner moves up and left to the output's MCU grid, as jpegtran moves it: with mw, mh the
    output's MCU size, L = left - left % mw, U = upper - upper % mh, and the file is right - L wide, lower - U high and holds
    [U:lower, L:right] of the transformed image (transform_crop_box gives L, U, right, lower).  trim / perfect are decided on the whole
    source first; the new right and bottom edges may cut an MCU, whose dummy blocks are then libjpeg's.  The box of the whole image
    writes the bytes of the call without it; restart intervals count on the cropped output's MCU grid.

    drop_chroma=True (TypeError for a value that is not a bool): ``jpegtran -grayscale``: a three-component source is written as a
    one-component file, exactly as the transcoder writes a grey source -- one DQT (the luma table as table 0, transposed by a transposing
    transform), the frame sampling byte 0x11, the luma component's id, one non-interleaved scan or libjpeg's six-scan progression --
    whose blocks are the source's real luma blocks.  For such a file the MCU of every rule above is 8 x 8: a mirrored axis has to be a
    multiple of 8, trim=True drops the partial 8-pixel strip, the crop aligns to 8, and a transposing transform of a 4:2:2 source needs
    no layout_440.  One-component sources still need grey=True and pass through unchanged.  Both keywords combine freely with each
    other and with every keyword above.

    Not built: without layout_440 a transposing transform of a 4:2:2 file that keeps its chroma (it would be 4:4:0; NotImplementedError);
    jpegtran's -drop and -wipe, the forced-size "f" suffix of -crop and offsets from the right or bottom edge.  EXIF pixel-dimension tags
    are not rewritten after a crop either.  Every refusal names the file and comes before any device work; there is no CPU fallback."""
    progressive, keep_metadata = _check_bool("progressive", progressive), _check_bool("keep_metadata", keep_metadata)
    trim, grey, layout_440 = _check_bool("trim", trim), _check_bool("grey", grey), _check_bool("layout_440", layout_440)
    drop_chroma = _check_bool("drop_chroma", drop_chroma)
    rst = _check_restart(restart_marker_blocks, restart_marker_rows)
    files = list(files)
    if not files:
        raise ValueError("standard_jpeg_transform_many needs at least one file")
    n = len(files)
    boxes = _check_crop(crop, n)
    if isinstance(transform, str):
        names = None if transform == "exif" else [_check_transform(transform, 0)] * n
    else:
        names = list(transform)
        if len(names) != n:
            raise ValueError(f"file {min(len(names), n)}: {len(names)} transforms for {n} files")
        names = [_check_transform(t, i) for i, t in enumerate(names)]
    return _transcode_many(files, progressive, device, keep_metadata, names, trim, names is None, grey, rst, layout_440, boxes, drop_chroma)


def standard_jpeg_transcode_many(files, progressive: bool = False, device: int = 0, keep_metadata: bool = False, grey: bool = False,
                                 restart_marker_blocks: int = 0, restart_marker_rows: int = 0, layout_440: bool = False) -> List[bytes]:
    """Lossless transcode on the device: -> every file entropy-coded again, in input order.  files: a non-empty sequence of bytes-like
    JPEG contents, baseline / extended-sequential (SOF0 / SOF1) and complete progressive (SOF2) files of any sizes and of the 4:4:4,
    4:2:2 and 4:2:0 layouts mixed freely.  progressive=False: a baseline file under the file's own optimal Huffman tables (what
    optimize=True writes); progressive=True: libjpeg's ten-scan progressive file (what progressive=True writes).  Every quantised
    coefficient of the output equals the source's, so both decode to the same pixels, and a file Pillow wrote gives Pillow's own
    optimize=True / progressive=True file byte for byte.  The output: SOI, JFIF 1.01 APP0 with the source's density, with
    keep_metadata=True the source's APP1 .. APP13, APP15 and COM segments (host work; never APP0 or Adobe APP14), the source's
    quantisation tables (8-bit, one DQT per table), its frame header, then tables and scans as the encoders lay them out.

    restart_marker_blocks, restart_marker_rows: Pillow's save options of those names, here ``jpegtran -restart NB`` / ``-restart N``
    (standard_jpeg_encode_many documents them): the output carries a DRI and an RSTn marker every N MCUs / MCU rows, which is what lets
    a decoder -- this library's among them -- work on the file's restart segments in parallel, and equals Pillow's optimize=True /
    progressive=True file with the same option byte for byte.  A source's own restart markers are never carried over: the two keywords
    alone decide, and with both 0 (the default) the output has none.

    grey=True also takes one-component (grey) files, baseline or progressive, mixed freely with colour ones (TypeError for a value
    that is not a bool).  Such a file is sampled 1 x 1 whatever its frame header says; its output has one DQT (its table, as table 0),
    a one-component frame header, the file's own DC and AC table and one non-interleaved scan -- with progressive=True libjpeg's six
    scans for one component -- so that a grey file Pillow wrote gives Pillow's optimize=True / progressive=True file of the mode-"L"
    image byte for byte.

    layout_440=True (TypeError for a value that is not a bool) also takes 4:4:0 files (three components, luma sampled 1 x 2 over
    1 x 1 chroma), mixed freely with the rest; the output keeps the layout (frame sampling byte 0x12).  Without it such a file is
    refused as before.

    Refused before any device work, naming the file: what the decoders' parsers refuse, 16-bit quantisation tables and, without
    grey=True, grey files (NotImplementedError), malformed headers (ValueError).  A file whose scan is corrupt, or that decodes to a
    coefficient an 8-bit JPEG cannot hold, raises ValueError naming its index and the reason; nothing is returned then.  There is no
    CPU fallback."""
    progressive, keep_metadata = _check_bool("progressive", progressive), _check_bool("keep_metadata", keep_metadata)
    grey, layout_440 = _check_bool("grey", grey), _check_bool("layout_440", layout_440)
    rst = _check_restart(restart_marker_blocks, restart_marker_rows)
    files = list(files)
    if not files:
        raise ValueError("standard_jpeg_transcode_many needs at least one file")
    return _transcode_many(files, progressive, device, keep_metadata, None, False, False, grey, rst, layout_440)


def _transcode_many(files, progressive, device, keep_metadata, names, trim, exif, grey=False, rst=(0, 0), layout_440=False, boxes=None,
                    drop=False):
    """the transcode (names None and not exif) and the transform, both through the aej_jfif_transform_*_cut entries: names[i] is file
    i's transform, exif takes it from the file; rst: (restart_marker_blocks, restart_marker_rows); boxes: None, or [n] crop boxes or
    None; drop: drop_chroma.  What no file of the call uses goes as the entry's neutral value -- NULL transforms when every file is
    "none", NULL boxes when no file has one, 0 for the rest -- which is the narrower entry byte for byte (include/aej.h)."""
    global _last_transcode_groups
    n = len(files)
    names = ["none"] * n if names is None else names
    boxes = [None] * n if boxes is None else boxes
    src, density, meta = _Sources(), [None] * n, [b""] * n
    for i, frame, mv in src.parse(files, transcoder=True, grey=grey, layout_440=layout_440):
        segs = marker_segments(mv, i)
        density[i] = _jfif_density(mv, segs)
        at = _exif_orientation_at(mv, segs) if exif else None
        if at and 1 <= at[0] <= 8:
            names[i] = _EXIF_TRANSFORM[at[0]]
        _transform_geometry(i, frame, names[i], trim, layout_440, boxes[i], drop)
        if keep_metadata:
            meta[i] = metadata_segments(mv, i)
            if at and 1 < at[0] <= 8:                # the tag's value becomes 1, in the TIFF block's byte order; nothing else changes
                k = sum(min(b, at[1]) - a for m, a, b in segs if a < at[1] and _is_metadata(m))      # its place among the carried bytes
                meta[i] = meta[i][:k] + (1).to_bytes(2, at[2]) + meta[i][k + 2:]
    order = src.base_idx + src.prog_idx             # the call's file order: baseline sources first
    ctx = get_context(device)
    t, lib = ctx.torch, ctx.lib
    descs, nb, base_pieces = src.baseline(src.base_idx)
    frames, pscans, npg, prog_pieces = src.progressive(src.prog_idx)
    # one staging copy for both kinds (the pinned buffer behind _stage is only valid until its next use)
    scans, off = _stage(ctx, src.views, base_pieces + prog_pieces)
    data, scan_off, data_off = scans, np.ascontiguousarray(off[:max(nb, 1)]), np.ascontiguousarray(off[nb:nb + max(len(prog_pieces), 1)])
    dens = np.ascontiguousarray(np.array([density[i] for i in order], np.uint16))
    codes = np.ascontiguousarray(np.array([TRANSFORMS.index(names[i]) for i in order], np.int32))
    box_arr = np.ascontiguousarray(np.array([boxes[i] or (0, 0, 0, 0) for i in order], np.int32))      # right == 0: no crop
    how = (int(progressive), codes.ctypes.data if codes.any() else None, int(trim), int(rst[0]), int(rst[1]), int(layout_440),
           box_arr.ctypes.data if box_arr.any() else None, int(drop))
    nws = int(lib.aej_jfif_transform_workspace_bytes_cut(ctx.handle, ctypes.addressof(descs), nb, ctypes.addressof(frames), ctypes.addressof(pscans),
                                                         npg, *how))
    if nws == 0:
        raise ValueError("descriptors the library refuses")
    ws = ctx.workspace(nws)
    status, offsets, lengths = ctx.empty((n,), t.int32), ctx.empty((n,), t.int64), ctx.empty((n,), t.int64)
    total, groups = ctypes.c_uint64(), ctypes.c_int32()
    cap = sum(len(v) for v in src.views) * 5 // 4 + (PROGRESSIVE_HEADER_CAPACITY if progressive else HEADER_CAPACITY) * n      # (a miss costs one more call)
    call = lambda o, c: lib.aej_jfif_transform_batch_cut(  # noqa: E731
        ctx.handle, ctypes.addressof(descs), nb, scans.data_ptr(), ctypes.c_uint64(scans.numel()), scan_off.ctypes.data, ctypes.addressof(frames),
        ctypes.addressof(pscans), npg, data.data_ptr(), ctypes.c_uint64(data.numel()), data_off.ctypes.data, dens.ctypes.data, *how,
        o.data_ptr(), ctypes.c_uint64(c), offsets.data_ptr(), lengths.data_ptr(), ctypes.addressof(total), status.data_ptr(),
        ctypes.addressof(groups), ws.data_ptr(), ctypes.c_uint64(nws))
    sized = _sized_call(ctx, call, cap, total, offsets, lengths)
    _last_transcode_groups = int(groups.value)
    st = status.cpu().numpy()                       # the one read-back of the per-file status words
    _raise_status(sorted((order[int(k)], int(st[k])) for k in np.flatnonzero(st)))
    res = [None] * n
    for k, f in enumerate(_file_bytes(*sized)):
        res[order[k]] = splice_metadata(f, meta[order[k]])
    return res


# ---- images of mixed sizes in one call ------------------------------------------------------------------------------------------------
_last_encode_groups = 0


def encode_groups() -> int:
    """Entropy-encode chains the last successful standard_jpeg_encode_many of this process ran: one per distinct (height, width,
    components) among its images.  The twin of transcode_groups, and like it a diagnostic: one module-level value, which a call that raises leaves as
    it was."""
    return _last_encode_groups


def _check_qualities(quality, n, what="image"):
    """quality= of the many-image calls -> [n] ints: one value for all, or one per image (ValueError naming the image otherwise)"""
    if isinstance(quality, (str, bytes)) or not hasattr(quality, "__len__"):
        return [_check_quality(quality)] * n
    if len(quality) != n:
        raise ValueError(f"quality: {len(quality)} values for {n} {what}s")
    out = []
    for i, q in enumerate(quality):
        try:
            out.append(_check_quality(q))
        except (ValueError, TypeError):
            raise ValueError(f"{what} {i}: quality {q!r}: an integer in 1..100 required") from None
    return out


MODES = ("RGB", "L", "auto")


def _check_mode(mode) -> str:
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode {mode!r}: 'RGB', 'L' or 'auto' required")
    return mode


def _check_images(images, mode="RGB"):
    """The host-side checks of standard_jpeg_encode_many, before any device context exists -> [(image, is_torch, is_float)]; a grey
    image is the one with two dimensions"""
    if isinstance(images, (str, bytes)) or not hasattr(images, "__len__") or (hasattr(images, "ndim") and not isinstance(images, (list, tuple))):
        raise ValueError("standard_jpeg_encode_many needs a sequence of [H, W, 3] images (one [B, H, W, 3] array is standard_jpeg_many's input)")
    if len(images) < 1:
        raise ValueError("standard_jpeg_encode_many needs at least one image")
    if len(images) > 65535:
        raise ValueError(f"{len(images)} images: at most 65535 in one call")
    out = []
    for i, x in enumerate(images):
        is_torch = is_tensor(x)
        if not is_torch:
            x = np.asarray(x)
        dt = str(x.dtype)
        if dt not in ("uint8", "torch.uint8", "float32", "torch.float32"):
            raise TypeError(f"image {i}: uint8 or float32 in [0, 1] required, got {dt}")
        colour, grey = x.ndim == 3 and x.shape[2] == 3, x.ndim == 2
        if not ((colour and mode != "L") or (grey and mode != "RGB")):
            want = {"RGB": "[H, W, 3]", "L": "[H, W] (mode 'L')", "auto": "[H, W] or [H, W, 3] (mode 'auto')"}[mode]
            raise ValueError(f"image {i}: {want} required, got {tuple(x.shape)}")
        if not (1 <= x.shape[0] <= 65535 and 1 <= x.shape[1] <= 65535):
            raise ValueError(f"image {i}: {x.shape[0]}x{x.shape[1]}: JPEG needs 1 <= H, W <= 65535")
        com = getattr(x, "jpeg_comment", None)
        if com is not None and (not isinstance(com, (bytes, bytearray)) or len(com) > 65533):
            raise TypeError(f"image {i}: jpeg_comment must be at most 65533 bytes, got {type(com).__name__}")
        out.append((x, is_torch, dt.endswith("float32")))
    return out


def _packed_source(ctx, imgs):
    """-> (what keeps the pixels alive on the device, the source's address, its bytes, int64 offsets of the images in it).  Device uint8
    tensors that are contiguous views of one allocation on this device are used where they lie; anything else is packed into a new buffer
    (images that are all on the host by _images.gather_u8, whose staging contract aej_jfif_many_encode's synchronise meets)."""
    t, n = ctx.torch, len(imgs)
    if all(is_t and not is_f and x.is_cuda and x.device == ctx.device and x.is_contiguous() for x, is_t, is_f in imgs):
        st = imgs[0][0].untyped_storage()
        if all(x.untyped_storage().data_ptr() == st.data_ptr() for x, _, _ in imgs):
            off = np.array([x.data_ptr() - st.data_ptr() for x, _, _ in imgs], np.int64)
            return [x for x, _, _ in imgs], st.data_ptr(), st.nbytes(), off
    if not any(is_t for _, is_t, _ in imgs):                 # every image on the host: one pinned copy
        arrays = []
        for i, (x, _, is_f) in enumerate(imgs):
            if is_f:
                if not (x.min() >= 0.0 and x.max() <= 1.0):
                    raise ValueError(f"image {i}: float32 images must lie in [0, 1]")
                x = np.rint(x * np.float32(255)).astype(np.uint8)
            arrays.append(x)
        src = gather_u8(ctx, arrays)
        base, total, off = src.span()
        return src.keep, base, total, np.array(off, np.int64)
    sizes = np.array([int(np.prod(x.shape)) for x, _, _ in imgs], np.int64)      # 3 H W, or H W of a grey image
    off = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    total = int(sizes.sum())
    buf = ctx.empty((total,), t.uint8)
    for i, (x, _, _) in enumerate(imgs):
        try:
            u8 = _to_u8(ctx, x) if x.ndim == 3 else _values_u8(ctx, x)
        except ValueError as e:
            raise ValueError(f"image {i}: {e}") from None
        buf[int(off[i]):int(off[i] + sizes[i])].copy_(u8.reshape(-1))
    return buf, buf.data_ptr(), total, off


def _encode_many(ctx, imgs, qualities, ss, opt, prog, rst=(0, 0)):
    """aej_jfif_many_encode_rst over the checked images (_check_images' list); rst: (restart_marker_blocks, restart_marker_rows), (0, 0)
    being aej_jfif_many_encode"""
    global _last_encode_groups
    from ._lib import JfifManyDesc
    t, lib, n = ctx.torch, ctx.lib, len(imgs)
    keep, src, src_bytes, off = _packed_source(ctx, imgs)
    descs = (JfifManyDesc * n)(*[JfifManyDesc(int(off[i]), int(x.shape[1]), int(x.shape[0]), qualities[i], 1 if x.ndim == 2 else 3) for i, (x, _, _) in enumerate(imgs)])
    nws = int(lib.aej_jfif_many_workspace_bytes_rst(ctx.handle, ctypes.addressof(descs), n, ss, int(opt), int(prog), int(rst[0]), int(rst[1])))
    if nws == 0:
        raise ValueError("descriptors the library refuses")
    ws = ctx.workspace(nws)
    offsets, lengths = ctx.empty((n,), t.int64), ctx.empty((n,), t.int64)
    total, groups = ctypes.c_uint64(), ctypes.c_int32()
    hdr = PROGRESSIVE_HEADER_CAPACITY if prog else HEADER_CAPACITY
    cap = sum(hdr + x.shape[0] * x.shape[1] * 3 // (4 if ss == 2 else 2) for x, _, _ in imgs)      # most files are far smaller; a miss costs one more call
    call = lambda o, c: lib.aej_jfif_many_encode_rst(  # noqa: E731
        ctx.handle, ctypes.addressof(descs), n, src, ctypes.c_uint64(src_bytes), ss, int(opt), int(prog), int(rst[0]), int(rst[1]), o.data_ptr(),
        ctypes.c_uint64(c), offsets.data_ptr(), lengths.data_ptr(), ctypes.addressof(total), ctypes.addressof(groups), ws.data_ptr(),
        ctypes.c_uint64(nws))
    sized = _sized_call(ctx, call, cap, total, offsets, lengths)      # (`keep` has held the pixels until here)
    _last_encode_groups = int(groups.value)
    res = _file_bytes(*sized)
    for i, (x, _, _) in enumerate(imgs):             # a comment the image carries: one COM segment after the JFIF APP0, where libjpeg puts it
        com = getattr(x, "jpeg_comment", None)
        if com is not None:
            res[i] = splice_metadata(res[i], b"\xff\xfe" + (len(com) + 2).to_bytes(2, "big") + bytes(com))
    return res


def standard_jpeg_encode_many(images, quality=75, subsampling="4:2:0", optimize: bool = False, progressive: bool = False, device: int = 0,
                              mode: str = "RGB", restart_marker_blocks: int = 0, restart_marker_rows: int = 0) -> List[bytes]:
    """Images of mixed sizes encoded in one call: -> every image's file, in input order; file i equals
    ``Image.fromarray(u8_i).save(buf, "JPEG", quality=q_i, subsampling=subsampling, optimize=optimize, progressive=progressive)`` byte
    for byte, and ``standard_jpeg_many(images[i], q_i, ...)[0]``.  images: a non-empty sequence of [H_i, W_i, 3] images, each uint8 or
    float32 in [0, 1] taken as ``rint(x * 255)``, numpy or torch, sizes mixed freely.  quality: one int for all, or one per image.
    subsampling, optimize, progressive: as standard_jpeg_many, one setting for the call.

    mode: "RGB" (the call as it always was); "L": every image is [H_i, W_i], uint8 or float32 by the same rule, and file i is the
    one-component file ``Image.fromarray(u8_i).save(buf, "JPEG", quality=q_i, optimize=optimize, progressive=progressive)`` writes for
    that mode-"L" image, byte for byte; "auto": [H, W] images are grey and [H, W, 3] images colour, mixed freely, each file that of its
    own single-mode call.  subsampling is checked but does not bear on a grey image: its one component is sampled 1 x 1, which is also
    what Pillow codes -- given an explicit subsampling= for a mode-"L" image Pillow writes those factors into the frame header's
    sampling byte and changes nothing else (a decoder ignores them for one component); this library always writes 1 x 1 there, the
    file of a save without that keyword.

    One kernel converts, down-samples, transforms and quantises every block of every image (csrc/jfifmany.hip); the images are then
    grouped by (size, components) and each group runs one entropy chain (encode_groups() tells how many), so launches grow with the
    number of distinct sizes.  Device uint8 tensors that are contiguous views of one allocation -- what standard_jpeg_thumbnail_many and
    resize_many return -- are read where they lie, by offset; anything else is packed into one device buffer first.

    A torch image that carries the attribute ``jpeg_comment`` (bytes; standard_jpeg_thumbnail_many sets it from its file's COM segment)
    gets that text as a COM segment right after the JFIF APP0 -- what Pillow from 9.4 on does with ``im.info["comment"]`` on save, and
    the only thing its save carries over from a file.  Without the attribute (every NumPy image) no such segment is written.

    restart_marker_blocks=N, restart_marker_rows=N: Pillow's save options of those names (libjpeg's restart_interval and
    restart_in_rows), one setting for the call, for colour and grey images and with optimize= and progressive=; file i equals Pillow's
    save with the same keywords.  A scan's restart interval R counts MCUs of that scan: blocks=N gives R = N for every scan; rows=N > 0
    overrides it with R = min(N x the scan's MCUs per row, 65535), per scan (an interleaved scan has ceil(W / (8 hs)) MCUs per row, a
    grey file's scan or a progressive AC scan the component's blocks per row).  The file carries ``FF DD 00 04 Rhi Rlo`` before the SOS
    of every scan whose R differs from the last one written, and before MCU k R (k >= 1) the coder flushes, pads the byte with 1-bits,
    writes ``FF D0+((k-1) & 7)`` and resets the DC predictors (a progressive scan its end-of-band run too); optimised tables are built
    under the same resets.  Such a file decodes restart segment by restart segment in parallel (standard_jpeg_decode_many).  Both 0 (the
    default): the file as it always was.  A value that is not an int (a bool or a float included) raises TypeError, one outside 0..65535
    ValueError -- a deliberate departure from Pillow, which wraps or reinterprets such values silently.  standard_jpeg_many,
    standard_jpeg_batch and sweep write no restart markers (their Annex K bit count is fused into quantisation): this call, the
    thumbnail call below, standard_jpeg_transcode_many and standard_jpeg_transform_many do.

    Checked before any device work, naming the image: a quality outside 1..100, a shape that is not the mode's ([H, W, 3], [H, W])
    with 1 <= H, W <= 65535, a quality sequence of another length, a mode other than the three (ValueError); a dtype other than uint8 / float32, optimize / progressive that are not bools
    (TypeError).  float32 values outside [0, 1] raise ValueError once the image is looked at.  There is no CPU fallback."""
    ss, opt, prog = _check_subsampling(subsampling), _check_bool("optimize", optimize), _check_bool("progressive", progressive)
    rst = _check_restart(restart_marker_blocks, restart_marker_rows)
    imgs = _check_images(images, _check_mode(mode))
    qualities = _check_qualities(quality, len(imgs))
    return _encode_many(get_context(device), imgs, qualities, ss, opt, prog, rst)


def standard_jpeg_thumbnail_jpeg_many(files, size, quality=75, subsampling="4:2:0", optimize: bool = False, progressive_out: bool = False,
                                      resample="bicubic", reducing_gap=2.0, progressive: bool = False, device: int = 0,
                                      restart_marker_blocks: int = 0, restart_marker_rows: int = 0, layout_440: bool = False,
                                      mode="RGB") -> List[bytes]:
    """JPEG files in, their thumbnails out as JPEG files: ``standard_jpeg_encode_many(standard_jpeg_thumbnail_many(files, size, resample,
    reducing_gap, progressive, device), quality, subsampling, optimize, progressive_out, device)`` -- for a three-component source file
    i equals ``im = Image.open(io.BytesIO(files[i])); im.thumbnail(size, resample, reducing_gap=reducing_gap); im.save(buf, "JPEG",
    quality=q_i, subsampling=subsampling, optimize=optimize, progressive=progressive_out)`` byte for byte.  The thumbnails never leave
    the device: only the decoder's status words and the finished files are read back.  Like Pillow's save it carries no metadata
    over (no EXIF, ICC profile or density) but a source's COM segment, which Pillow from 9.4 on writes again from
    ``im.info["comment"]``: the thumbnails carry it as ``jpeg_comment`` and the encoder writes it (both documented there).
    mode: standard_jpeg_thumbnail_many's, handed to it, and the matching mode to standard_jpeg_encode_many.  "RGB" (the default, the
    call as it always was): a grey (single-component) source comes out as a three-component file with neutral chroma.  "auto": every
    file in Pillow's own mode -- a grey source leaves as the ONE-component file of Pillow's ``im.thumbnail(size); im.save(...)``, byte
    for byte, a third of the pixel traffic on the way; colour sources as without the keyword.  "L": colour sources leave grey too,
    from their luma plane (standard_jpeg_thumbnail_many's recipe, then ``save``; not ``convert("L")``).  A list gives one mode per file.
    files, size, resample, reducing_gap, progressive (whether progressive SOURCES are accepted): standard_jpeg_thumbnail_many's.
    quality (one, or one per file), subsampling, optimize, progressive_out: standard_jpeg_encode_many's quality, subsampling, optimize
    and progressive; restart_marker_blocks, restart_marker_rows: passed through to it (Pillow's save options).  Every argument is checked, and every header parsed, before any device work; a file whose scan is corrupt raises
    the decoder's ValueError naming it and nothing is returned.  layout_440: standard_jpeg_thumbnail_many's, for the SOURCES (the
    thumbnails are written in `subsampling`, which has no 4:4:0)."""
    ss, opt, prog = _check_subsampling(subsampling), _check_bool("optimize", optimize), _check_bool("progressive_out", progressive_out)
    rst = _check_restart(restart_marker_blocks, restart_marker_rows)
    files = list(files)
    if not files:
        raise ValueError("standard_jpeg_thumbnail_jpeg_many needs at least one file")
    qualities = _check_qualities(quality, len(files), "file")
    modes = _check_modes(mode, len(files))
    thumbs = standard_jpeg_thumbnail_many(files, size, resample, reducing_gap, progressive, device, layout_440, modes)
    enc_mode = modes[0] if all(m == modes[0] for m in modes) else "auto"      # a per-file mix: each thumbnail's rank says what it is
    return _encode_many(get_context(device), _check_images(thumbs, enc_mode), qualities, ss, opt, prog, rst)
