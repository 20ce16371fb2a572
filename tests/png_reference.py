"""Plain Python / numpy PNG writer and reader for the PNG tests (no part of the package is imported here).

The writer exists because a file made by Pillow never lets a test choose the filter of a row: ``make_png`` filters each row with the
REQUESTED filter type, compresses with zlib at the requested level and frames the chunks with ``zlib.crc32``.  The reader is the first
reference: the specification's un-filter (section 9: Sub, Up, Average with a 9-bit sum, Paeth with the tie order a, b, c) and Pillow's
expansions, written independently of the package.  Live Pillow on the same bytes is the second (PNG decode is lossless, so no version is
pinned); ``expected`` makes the two agree before anybody asks the GPU."""
import functools
import io
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
KINDS = ((0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8))      # (colour type, bit depth): the supported set
BAND = 64                                                # rows per band of csrc/png.hip (kRows): the heights below straddle it


def chunk(kind: bytes, data: bytes = b"") -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def pack_rows(w, h, depth, colour_type, samples):
    """samples [h, w, channels] (values below 2^depth) -> the scanlines [h, row_bytes] as the file stores them before filtering"""
    ch = CHANNELS[colour_type]
    s = np.asarray(samples, np.uint8).reshape(h, w * ch)
    if depth == 8:
        return s.copy()
    per = 8 // depth
    pad = (-s.shape[1]) % per
    s = np.concatenate([s, np.zeros((h, pad), np.uint8)], 1).reshape(h, -1, per)
    out = np.zeros(s.shape[:2], np.uint8)
    for k in range(per):                                 # the leftmost pixel in the high-order bits
        out |= (s[:, :, k] & ((1 << depth) - 1)) << (8 - depth * (k + 1))
    return out


def filter_rows(rows, bpp, filters):
    """the filtered scanlines, each behind its filter byte: row r filtered with type filters[r] (a byte above 4 is written as it is, over
    an unfiltered row: what a broken writer would leave)"""
    h, rb = rows.shape
    out = bytearray()
    prev = [0] * rb
    for r in range(h):
        cur = rows[r].tolist()
        f = filters[r]
        line = []
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[f] if f <= 4 else 0
            line.append((cur[i] - pred) & 255)
        out.append(f)
        out += bytes(line)
        prev = cur
    return bytes(out)


def make_png(w, h, depth, colour_type, samples, filters, level=6, idat_split=None, extra_chunks=(), rows=None, stream_edit=None):
    """One PNG file.  filters: one type for every row, or one per row.  idat_split: None (one IDAT), k (IDAT chunks of k bytes) or
    (k, True) (the same with an empty IDAT between any two).  extra_chunks: (type, data) pairs written between IHDR and the first IDAT
    in the order given (PLTE and tRNS come this way).  rows: scanlines actually written (the header keeps h).  stream_edit: a function
    the finished zlib stream goes through (for the corrupt files of the error tests)."""
    filters = [filters] * h if isinstance(filters, int) else list(filters)
    bpp = CHANNELS[colour_type] if depth == 8 else 1
    raw = pack_rows(w, h, depth, colour_type, samples)
    n = h if rows is None else rows
    z = zlib.compress(filter_rows(raw[:n], bpp, filters[:n]), level)
    if stream_edit is not None:
        z = stream_edit(z)
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour_type, 0, 0, 0))]
    out += [chunk(k, d) for k, d in extra_chunks]
    if idat_split is None:
        out.append(chunk(b"IDAT", z))
    else:
        k, empties = idat_split if isinstance(idat_split, tuple) else (idat_split, False)
        for i in range(0, len(z), k):
            if empties and i:
                out.append(chunk(b"IDAT"))
            out.append(chunk(b"IDAT", z[i:i + k]))
    out.append(chunk(b"IEND"))
    return b"".join(out)


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
def read_chunks(data):
    """-> [(type, data, offset of the data in the file)]; no CRC is looked at"""
    assert data[:8] == SIGNATURE
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        out.append((bytes(data[pos + 4:pos + 8]), bytes(data[pos + 8:pos + 8 + n]), pos + 8))
        pos += 12 + n
        if out[-1][0] == b"IEND":
            break
    return out


def read_png(data):
    """-> (header dict, un-filtered scanlines [h, row_bytes] uint8) by the specification's reconstruction"""
    chunks = read_chunks(data)
    w, h, depth, ct, _, _, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert chunks[0][0] == b"IHDR" and interlace == 0
    ch = CHANNELS[ct]
    rb = (w * ch * depth + 7) // 8
    bpp = ch if depth == 8 else 1
    plte = b"".join(d for k, d, _ in chunks if k == b"PLTE")
    raw = zlib.decompress(b"".join(d for k, d, _ in chunks if k == b"IDAT"))
    assert len(raw) == h * (1 + rb)
    rows = np.zeros((h, rb), np.uint8)
    prev = [0] * rb
    for r in range(h):
        f = raw[r * (1 + rb)]
        line = list(raw[r * (1 + rb) + 1:(r + 1) * (1 + rb)])
        for i in range(rb):
            a = line[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            line[i] = (line[i] + (0, a, b, (a + b) >> 1, _paeth(a, b, c))[f]) & 255
        rows[r] = line
        prev = line
    head = dict(width=w, height=h, bit_depth=depth, colour_type=ct, channels=ch, row_bytes=rb, palette=plte,
                has_trns=any(k == b"tRNS" for k, _, _ in chunks),
                idat=[(o, len(d)) for k, d, o in chunks if k == b"IDAT"],
                mode={0: "1" if depth == 1 else "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}[ct])
    return head, rows


def expand(head, rows, mode):
    """the image png_decode_many promises for `mode` ("RGB" or "auto"), from the un-filtered scanlines"""
    w, h, depth, ct, ch = head["width"], head["height"], head["bit_depth"], head["colour_type"], head["channels"]
    if depth == 8:
        s = rows.reshape(h, w, ch)
    else:
        bits = np.unpackbits(rows, axis=1).reshape(h, -1, depth)
        s = np.zeros(bits.shape[:2], np.uint8)
        for k in range(depth):
            s = (s << 1) | bits[:, :, k]
        s = s[:, :w].reshape(h, w, 1)
        if ct == 0:
            s = s * np.uint8(255 // ((1 << depth) - 1))
    if ct == 3:
        pal = np.zeros((256, 3), np.uint8)
        pal[:len(head["palette"]) // 3] = np.frombuffer(head["palette"], np.uint8).reshape(-1, 3)
        return pal[s[:, :, 0]]
    if mode == "RGB":
        return np.ascontiguousarray(np.repeat(s[:, :, :1], 3, 2) if ct in (0, 4) else s[:, :, :3])
    return np.ascontiguousarray(s[:, :, 0] if ct == 0 else s)


def reference(data, mode):
    head, rows = read_png(data)
    return expand(head, rows, mode)


def pillow(data, mode):
    """live Pillow on the same bytes: convert("RGB"), or the image in Pillow's own mode ("1" as "L", "P" through its palette)"""
    import warnings
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # (Pillow advises RGBA for a palette with tRNS; the promise here is convert("RGB"))
        if mode == "RGB" or im.mode == "P":
            return np.asarray(im.convert("RGB"))
        return np.asarray(im.convert("L") if im.mode == "1" else im)


# ---- the files of the tests -------------------------------------------------------------------------------------------------------------
def random_samples(rng, w, h, depth, colour_type):
    """seeded samples with smooth stretches (so that matches and every Paeth branch occur) and noise"""
    ch = CHANNELS[colour_type]
    s = rng.integers(0, 1 << depth, (h, w, ch))
    ramp = (np.arange(w)[None, :, None] * 3 + np.arange(h)[:, None, None] * 5 + np.arange(ch)[None, None, :] * 40) % (1 << depth)
    return np.where(rng.random((h, w, 1)) < 0.5, s, ramp).astype(np.uint8)


def palette_chunk(rng, entries):
    return (b"PLTE", rng.integers(0, 256, 3 * entries).astype(np.uint8).tobytes())


def kind_file(rng, w, h, colour_type, depth, filters, **kw):
    """a file of one supported kind; a palette file gets a PLTE of as many entries as its depth can index (256 at depth 8)"""
    extra = list(kw.pop("extra_chunks", ()))
    if colour_type == 3 and not any(k == b"PLTE" for k, _ in extra):
        extra.insert(0, palette_chunk(rng, 1 << depth))
    return make_png(w, h, depth, colour_type, random_samples(rng, w, h, depth, colour_type), filters, extra_chunks=extra, **kw)


PATTERNS = {"cycle": lambda h: [r % 5 for r in range(h)], "reverse": lambda h: [(4 - r) % 5 for r in range(h)],
            **{f"all{f}": (lambda f: lambda h: [f] * h)(f) for f in range(5)}}
HEIGHTS = (1, BAND - 1, BAND, BAND + 1, 2 * BAND + 2)


@functools.lru_cache(maxsize=None)
def suite():
    """name -> file bytes: every well-formed file the GPU tests decode (seeded; built once per process)"""
    rng = np.random.default_rng(20260719)
    files = {}
    for pat, fn in PATTERNS.items():                     # filters and geometry: 13 x 7 of every kind, every pattern
        for ct, depth in KINDS:
            files[f"f13x7_{pat}_ct{ct}d{depth}"] = kind_file(rng, 13, 7, ct, depth, fn(7))
    for w in (1, 2, 3):                                  # no left neighbour, a short row
        for ct, depth in KINDS:
            files[f"w{w}_ct{ct}d{depth}"] = kind_file(rng, w, 6, ct, depth, PATTERNS["cycle"](6))
    for hgt in HEIGHTS:                                  # the carry across band boundaries
        for f in (4, 3):
            files[f"h{hgt}_all{f}"] = kind_file(rng, 70, hgt, 2, 8, f)
    files["wide_rgba"] = kind_file(rng, 700, 9, 6, 8, PATTERNS["cycle"](9))      # a row wider than any LDS tile
    # rows wider than a tile AND more than one band, at the other unit sizes
    files["wide_rgb"] = kind_file(rng, 300, BAND + 6, 2, 8, PATTERNS["reverse"](BAND + 6))
    files["wide_grey"] = kind_file(rng, 600, BAND + 2, 0, 8, PATTERNS["cycle"](BAND + 2))
    files["wide_ga"] = kind_file(rng, 300, BAND + 3, 4, 8, PATTERNS["cycle"](BAND + 3))
    files["wide_bits"] = kind_file(rng, 2501, 3, 0, 1, [4, 3, 1])
    files["wide_pal4"] = kind_file(rng, 777, BAND + 1, 3, 4, PATTERNS["reverse"](BAND + 1))
    s = random_samples(rng, 97, 41, 8, 2)                # streams: stored, fixed / short dynamic, dynamic blocks; split IDAT
    for level in (0, 1, 9):
        files[f"level{level}"] = make_png(97, 41, 8, 2, s, PATTERNS["cycle"](41), level=level)
    files["idat_1"] = make_png(97, 41, 8, 2, s, PATTERNS["cycle"](41), idat_split=1)
    files["idat_7_empty"] = make_png(97, 41, 8, 2, s, PATTERNS["cycle"](41), idat_split=(7, True))
    with open(os.path.join(GOLDEN, "lena.png"), "rb") as fh:
        files["lena"] = fh.read()
    # layouts
    idx = rng.integers(0, 256, (9, 31, 1)).astype(np.uint8)
    idx[0, :4, 0] = (255, 10, 9, 0)
    files["short_palette"] = make_png(31, 9, 8, 3, idx, PATTERNS["cycle"](9), extra_chunks=[palette_chunk(rng, 10)])
    files["trns_palette"] = kind_file(rng, 31, 9, 3, 4, PATTERNS["cycle"](9), extra_chunks=[palette_chunk(rng, 16), (b"tRNS", bytes(range(0, 160, 10)))])
    files["trns_grey"] = kind_file(rng, 31, 9, 0, 8, PATTERNS["cycle"](9), extra_chunks=[(b"tRNS", b"\x00\x07")])
    files["trns_rgb"] = kind_file(rng, 31, 9, 2, 8, PATTERNS["cycle"](9), extra_chunks=[(b"tRNS", b"\x00\x01\x00\x02\x00\x03")])
    files["ancillary"] = kind_file(rng, 31, 9, 2, 8, PATTERNS["reverse"](9), extra_chunks=[(b"tEXt", b"Comment\0hello"), (b"zzZz", b"\1\2\3")])
    files["ga"] = kind_file(rng, 45, 33, 4, 8, PATTERNS["cycle"](33))
    files["rgba"] = kind_file(rng, 45, 33, 6, 8, PATTERNS["reverse"](33))
    return files


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """the reference image of suite()[name] in `mode`: the reader's, after live Pillow has agreed with it (computed once, read-only)"""
    data = suite()[name]
    want = reference(data, mode)
    got = pillow(data, mode)
    assert want.dtype == np.uint8 and want.shape == got.shape and np.array_equal(want, got), f"{name} ({mode}): the reader and Pillow differ"
    want.setflags(write=False)
    return want


def corrupt_files():
    """name -> (file bytes, what zlib says of its stream): the data errors of the error tests, each built with the writer"""
    rng = np.random.default_rng(7)
    s = random_samples(rng, 40, 20, 8, 2)
    filt = PATTERNS["cycle"](20)

    def flip(z):
        k = len(z) // 2
        return z[:k] + bytes([z[k] ^ 0x5A]) + z[k + 1:]

    return {
        "flipped": make_png(40, 20, 8, 2, s, filt, level=9, stream_edit=flip),
        "truncated": make_png(40, 20, 8, 2, s, filt, level=9, stream_edit=lambda z: z[:len(z) - 11]),
        "short": make_png(40, 20, 8, 2, s, filt, rows=19),
        "filter5": make_png(40, 20, 8, 2, s, [0, 1, 2, 5] + filt[4:]),
    }
