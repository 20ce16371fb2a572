"""What Pillow's PNG writer produces for modes L, LA, RGB and RGBA, restated in numpy: the per-row filter choice (Pillow's own rule, not
libpng's), the zlib stream and the chunk framing.  The reference of ``png_encode_many`` (tests/test_png_encode_host.py checks it against
Pillow itself, tests/test_gpu_png_encode.py checks the library against it).

Filter choice of a row (``bpp`` bytes per pixel, the row above the first row all zeros): cost(f) = sum of (v if v < 128 else 256 - v)
over the row's filtered bytes v.  Start with None (0).  If its cost is 0, keep it.  Otherwise try Up (2), Sub (1), Average (3, only with
``optimize``) and Paeth (4) in that order and switch only to a strictly smaller cost.

The zlib stream is ``zlib.compressobj(level, DEFLATED, 15, 9, Z_FILTERED)`` over the scanlines (level 9 with ``optimize``), cut into IDAT
chunks of 65536 bytes; the file is the signature, IHDR, the IDATs and IEND."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
IDAT_BYTES = 65536
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}      # bytes per pixel -> IHDR colour type
NONE, SUB, UP, AVERAGE, PAETH = 0, 1, 2, 3, 4


def as_rows(image):
    """[H, W] or [H, W, C] uint8 -> ([H, W * C] rows, bpp)"""
    x = np.ascontiguousarray(image, np.uint8)
    bpp = 1 if x.ndim == 2 else x.shape[2]
    return x.reshape(x.shape[0], -1), bpp


def filtered(row, up, bpp):
    """The five filtered versions of one row (int arrays of bytes 0 .. 255), indexed by filter type."""
    x, b = row.astype(np.int32), up.astype(np.int32)
    a, c = np.zeros_like(x), np.zeros_like(x)
    a[bpp:], c[bpp:] = x[:-bpp] if bpp < len(x) else 0, b[:-bpp] if bpp < len(x) else 0
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return [x, (x - a) & 255, (x - b) & 255, (x - ((a + b) >> 1)) & 255, (x - paeth) & 255]


def cost(v):
    return int(np.where(v < 128, v, 256 - v).sum())


def choose(row, up, bpp, optimize=False):
    """(filter type, filtered bytes) Pillow writes for `row` under `up`."""
    f = filtered(row, up, bpp)
    best, best_cost = NONE, cost(f[NONE])
    if best_cost == 0:
        return NONE, f[NONE].astype(np.uint8)
    for t in (UP, SUB, AVERAGE, PAETH):
        if t == AVERAGE and not optimize:
            continue
        c = cost(f[t])
        if c < best_cost:
            best, best_cost = t, c
    return best, f[best].astype(np.uint8)


def scanlines(image, optimize=False):
    """The bytes Pillow deflates: per row the filter byte, then the filtered row."""
    rows, bpp = as_rows(image)
    out = np.empty((rows.shape[0], 1 + rows.shape[1]), np.uint8)
    up = np.zeros(rows.shape[1], np.uint8)
    for y, row in enumerate(rows):
        out[y, 0], out[y, 1:] = choose(row, up, bpp, optimize)
        up = row
    return out.tobytes()


def filter_types(image, optimize=False):
    rows, _ = as_rows(image)
    return list(np.frombuffer(scanlines(image, optimize), np.uint8).reshape(rows.shape[0], -1)[:, 0])


def chunk(name, body):
    return struct.pack(">I", len(body)) + name + body + struct.pack(">I", zlib.crc32(name + body))


def frame(shape, stream):
    """The PNG file of a finished zlib stream: signature, IHDR, IDATs of 65536 bytes, IEND.  shape: [H, W] or [H, W, C]."""
    bpp = 1 if len(shape) == 2 else shape[2]
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", shape[1], shape[0], 8, COLOUR_TYPE[bpp], 0, 0, 0))]
    out += [chunk(b"IDAT", stream[i:i + IDAT_BYTES]) for i in range(0, len(stream), IDAT_BYTES)]
    return b"".join(out + [chunk(b"IEND", b"")])


def pillow_zlib(data, level):
    z = zlib.compressobj(level, zlib.DEFLATED, 15, 9, zlib.Z_FILTERED)
    return z.compress(data) + z.flush()


def make_file(shape, data, level=6):
    """Pillow's file for the scanline bytes `data` of an image of `shape` at compress_level `level` (optimize=True: level 9)."""
    return frame(shape, pillow_zlib(data, level))


def encode(image, optimize=False, compress_level=6):
    x = np.asarray(image)
    return make_file(x.shape, scanlines(x, optimize), 9 if optimize else compress_level)


def idat(data):
    """The joined IDAT bodies of a PNG file, and the number of IDAT chunks."""
    pos, parts = 8, []
    while pos < len(data):
        n, name = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if name == b"IDAT":
            parts.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    return b"".join(parts), len(parts)


def huffman_only(data):
    """Bytes of `data` under zlib's best Huffman-only coding: what a deflate that finds no match costs."""
    z = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    return len(z.compress(data) + z.flush())
