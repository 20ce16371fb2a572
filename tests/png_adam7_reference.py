"""Plain Python / numpy writer and reader of Adam7-interlaced and 16-bit PNG files for the PNG tests (no part of the package is imported
here; chunk framing, the row filter and the seeded samples come from tests/png_reference.py).

Pillow cannot WRITE interlaced files and never lets a test choose a row's filter, so ``make_png`` here packs 16-bit samples big-endian,
splits an image into the seven Adam7 passes (PNG specification, section 8.2: the 8 x 8 pattern ``ADAM7`` below), filters every non-empty
pass as an image of its own with the REQUESTED filter per row, and joins the passes into one zlib stream; a pass without pixels
contributes nothing, not even filter bytes.  The reader is the first reference -- the specification's un-filter per pass, the scatter
of every pass to its pixels, Pillow's expansions of 16-bit samples -- and live Pillow on the same bytes the second; ``expected`` makes
the two agree before anybody asks the GPU."""
import functools
import io
import struct
import zlib

import numpy as np

import png_reference as R

# the specification's pattern: the pass (1 .. 7) of pixel (x & 7, y & 7), row by row
ADAM7 = ((1, 6, 4, 6, 2, 6, 4, 6),
         (7, 7, 7, 7, 7, 7, 7, 7),
         (5, 6, 5, 6, 5, 6, 5, 6),
         (7, 7, 7, 7, 7, 7, 7, 7),
         (3, 6, 4, 6, 3, 6, 4, 6),
         (7, 7, 7, 7, 7, 7, 7, 7),
         (5, 6, 5, 6, 5, 6, 5, 6),
         (7, 7, 7, 7, 7, 7, 7, 7))
KINDS16 = ((0, 16), (2, 16), (4, 16), (6, 16))
KINDS = R.KINDS + KINDS16                               # every kind, each also interlaced
MODE16 = {0: "I;16", 2: "RGB", 4: "RGBA", 6: "RGBA"}


def pass_pixels(w, h, p):
    """-> (ys, xs): the rows and columns of pass p (1 .. 7) in a w x h image, from the pattern alone"""
    ys = [y for y in range(h) if p in ADAM7[y & 7]]
    xs = [x for x in range(w) if ys and ADAM7[ys[0] & 7][x & 7] == p]
    return (ys, xs) if xs else ([], [])


def bpp_of(colour_type, depth):
    return max(1, R.CHANNELS[colour_type] * depth // 8)


def pack_rows(w, h, depth, colour_type, samples):
    """samples [h, w, channels] -> scanlines [h, row_bytes]; 16-bit samples big-endian"""
    if depth != 16:
        return R.pack_rows(w, h, depth, colour_type, samples)
    return np.asarray(samples, np.uint16).reshape(h, -1).astype(">u2").view(np.uint8).reshape(h, -1).copy()


def scanlines(w, h, depth, colour_type, samples, filters, interlace):
    """the bytes the zlib stream holds.  filters: one type, one per image row (a pass row takes the filter of the image row it comes from
    unless `filters` is a dict {pass: one type or a list per pass row}), for a non-interlaced file one per row"""
    bpp = bpp_of(colour_type, depth)
    samples = np.asarray(samples).reshape(h, w, R.CHANNELS[colour_type])
    if not interlace:
        f = [filters] * h if isinstance(filters, int) else list(filters)
        return R.filter_rows(pack_rows(w, h, depth, colour_type, samples), bpp, f)
    out = b""
    for p in range(1, 8):
        ys, xs = pass_pixels(w, h, p)
        if not ys:
            continue
        if isinstance(filters, dict):
            f = filters.get(p, 0)
            f = [f] * len(ys) if isinstance(f, int) else list(f)
        else:
            f = [filters] * len(ys) if isinstance(filters, int) else [filters[y] for y in ys]
        sub = samples[np.ix_(ys, xs)]
        out += R.filter_rows(pack_rows(len(xs), len(ys), depth, colour_type, sub), bpp, f)
    return out


def make_png(w, h, depth, colour_type, samples, filters, interlace=0, level=6, extra_chunks=(), stream_edit=None, raw_edit=None):
    """One PNG file.  raw_edit: a function the scanline bytes go through before zlib (short or foreign streams of the error tests)."""
    raw = scanlines(w, h, depth, colour_type, samples, filters, interlace)
    if raw_edit is not None:
        raw = raw_edit(raw)
    z = zlib.compress(raw, level)
    if stream_edit is not None:
        z = stream_edit(z)
    out = [R.SIGNATURE, R.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour_type, 0, 0, interlace))]
    out += [R.chunk(k, d) for k, d in extra_chunks]
    out += [R.chunk(b"IDAT", z), R.chunk(b"IEND")]
    return b"".join(out)


def raw_bytes(w, h, depth, colour_type, interlace):
    """the length of the writer's scanline stream"""
    return len(scanlines(w, h, depth, colour_type, np.zeros((h, w, R.CHANNELS[colour_type]), np.uint16), 0, interlace))


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
def _unfilter(raw, pos, h, rb, bpp):
    rows = np.zeros((h, rb), np.uint8)
    prev = [0] * rb
    for r in range(h):
        f = raw[pos]
        line = list(raw[pos + 1:pos + 1 + rb])
        assert len(line) == rb and f <= 4
        for i in range(rb):
            a = line[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            line[i] = (line[i] + (0, a, b, (a + b) >> 1, R._paeth(a, b, c))[f]) & 255
        rows[r] = line
        prev = line
        pos += 1 + rb
    return rows, pos


def _samples(rows, w, depth, ch):
    """un-filtered scanlines [h, rb] -> the samples [h, w, ch] (uint16 for depth 16, unscaled for the packed depths)"""
    h = rows.shape[0]
    if depth == 16:
        return rows.reshape(h, -1).view(">u2").astype(np.uint16).reshape(h, w, ch)
    if depth == 8:
        return rows.reshape(h, w, ch)
    bits = np.unpackbits(rows, axis=1).reshape(h, -1, depth)
    s = np.zeros(bits.shape[:2], np.uint8)
    for k in range(depth):
        s = (s << 1) | bits[:, :, k]
    return s[:, :w].reshape(h, w, 1)


def read_png(data):
    """-> (header dict, samples [h, w, channels]): the specification's reconstruction, pass by pass for an interlaced file"""
    chunks = R.read_chunks(data)
    w, h, depth, ct, _, _, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    ch = R.CHANNELS[ct]
    bpp = bpp_of(ct, depth)
    raw = zlib.decompress(b"".join(d for k, d, _ in chunks if k == b"IDAT"))
    samples = np.zeros((h, w, ch), np.uint16 if depth == 16 else np.uint8)
    pos = 0
    if interlace:
        for p in range(1, 8):
            ys, xs = pass_pixels(w, h, p)
            if ys:
                rows, pos = _unfilter(raw, pos, len(ys), (len(xs) * ch * depth + 7) // 8, bpp)
                samples[np.ix_(ys, xs)] = _samples(rows, len(xs), depth, ch)
    else:
        rows, pos = _unfilter(raw, pos, h, (w * ch * depth + 7) // 8, bpp)
        samples[:] = _samples(rows, w, depth, ch)
    assert pos == len(raw)
    mode = MODE16[ct] if depth == 16 else {0: "1" if depth == 1 else "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}[ct]
    head = dict(width=w, height=h, bit_depth=depth, colour_type=ct, channels=ch, row_bytes=(w * ch * depth + 7) // 8, interlace=interlace,
                raw_bytes=len(raw), mode=mode, palette=b"".join(d for k, d, _ in chunks if k == b"PLTE"))
    return head, samples


def expand(head, s, mode):
    """the image png_decode_many promises for `mode` from the samples"""
    depth, ct = head["bit_depth"], head["colour_type"]
    if depth == 16:
        hi = (s >> 8).astype(np.uint8)
        if ct == 0:                                      # Pillow's "I;16": the samples; convert("RGB") CLIPS them
            return np.ascontiguousarray(s[:, :, 0]) if mode == "auto" else np.repeat(np.minimum(s, 255).astype(np.uint8), 3, 2)
        if ct == 4:                                      # opened as RGBA
            rgba = np.concatenate([np.repeat(hi[:, :, :1], 3, 2), hi[:, :, 1:]], 2)
            return np.ascontiguousarray(rgba if mode == "auto" else rgba[:, :, :3])
        return np.ascontiguousarray(hi if mode == "auto" else hi[:, :, :3])
    if depth < 8 and ct == 0:
        s = s * np.uint8(255 // ((1 << depth) - 1))
    if ct == 3:
        pal = np.zeros((256, 3), np.uint8)
        pal[:len(head["palette"]) // 3] = np.frombuffer(head["palette"], np.uint8).reshape(-1, 3)
        return pal[s[:, :, 0]]
    if mode == "RGB":
        return np.ascontiguousarray(np.repeat(s[:, :, :1], 3, 2) if ct in (0, 4) else s[:, :, :3])
    return np.ascontiguousarray(s[:, :, 0] if ct == 0 else s)


def reference(data, mode):
    head, s = read_png(data)
    return expand(head, s, mode)


def pillow(data, mode):
    """live Pillow on the same bytes: convert("RGB"), or np.asarray of the opened image ("1" as "L", "P" through its palette)"""
    import warnings
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if mode == "RGB" or im.mode == "P":
            return np.asarray(im.convert("RGB"))
        return np.asarray(im.convert("L") if im.mode == "1" else im)


# ---- the files of the tests -------------------------------------------------------------------------------------------------------------
def random_samples(rng, w, h, depth, colour_type):
    """seeded samples; 16-bit ones with high and low bytes that differ, and (grey) values on both sides of 255 so that the clip shows"""
    if depth != 16:
        return R.random_samples(rng, w, h, depth, colour_type)
    ch = R.CHANNELS[colour_type]
    s = rng.integers(0, 1 << 16, (h, w, ch))
    ramp = (np.arange(w)[None, :, None] * 771 + np.arange(h)[:, None, None] * 1285 + np.arange(ch)[None, None, :] * 10280 + 3) % (1 << 16)
    s = np.where(rng.random((h, w, 1)) < 0.5, s, ramp)
    small = rng.integers(0, 512, (h, w, ch))             # 0 .. 511: around the clip
    s = np.where(rng.random((h, w, 1)) < 0.3, small, s)
    s = np.ascontiguousarray(s)
    k = min(4, s.size)
    s.reshape(-1)[:k] = (255, 256, 0, 65535)[:k]
    return s.astype(np.uint16)


def kind_file(rng, w, h, colour_type, depth, filters, interlace=0, **kw):
    extra = list(kw.pop("extra_chunks", ()))
    if colour_type == 3:
        extra.insert(0, R.palette_chunk(rng, 1 << depth))
    return make_png(w, h, depth, colour_type, random_samples(rng, w, h, depth, colour_type), filters, interlace, extra_chunks=extra, **kw)


SMALL_KINDS = ((2, 8), (0, 1), (3, 4), (6, 16))          # the 81 sizes W, H in 1 .. 9 of each
BANDS = ((11, 131, 2, 8), (11, 257, 2, 8), (9, 513, 0, 8))      # pass 7 with 65 and 128 rows, pass 6 with 129, pass 1 with 65


def _k(ct, depth):
    return f"ct{ct}d{depth}"


@functools.lru_cache(maxsize=None)
def suite():
    """name -> file bytes: every well-formed file the GPU tests decode (seeded; built once per process)"""
    rng = np.random.default_rng(20261021)
    files = {}
    for ct, depth in SMALL_KINDS:                        # empty and partial passes
        for h in range(1, 10):
            for w in range(1, 10):
                files[f"s{w}x{h}_{_k(ct, depth)}_i"] = kind_file(rng, w, h, ct, depth, [(r + w) % 5 for r in range(h)], 1)
    for pat, fn in R.PATTERNS.items():
        for ct, depth in KINDS:                          # every kind interlaced at 13 x 7 and 9 x 9; every 16-bit kind plain at 13 x 7
            files[f"f13x7_{pat}_{_k(ct, depth)}_i"] = kind_file(rng, 13, 7, ct, depth, fn(7), 1)
            files[f"f9x9_{pat}_{_k(ct, depth)}_i"] = kind_file(rng, 9, 9, ct, depth, fn(9), 1)
        for ct, depth in KINDS16:
            files[f"f13x7_{pat}_{_k(ct, depth)}"] = kind_file(rng, 13, 7, ct, depth, fn(7))
    for w, h, ct, depth in BANDS:                        # the carry across bands inside a pass
        for f in (4, 3):
            files[f"band{w}x{h}_all{f}_i"] = kind_file(rng, w, h, ct, depth, f, 1)
    files["wide_rgba8_i"] = kind_file(rng, 700, 9, 6, 8, R.PATTERNS["cycle"](9), 1)           # pass 7 wider than a tile
    files["wide_grey8_i"] = kind_file(rng, 300, 9, 0, 8, R.PATTERNS["reverse"](9), 1)
    for i in (0, 1):                                     # 16-bit RGBA: 32 units a tile; 16-bit RGB: 42
        tag = "_i" if i else ""
        files[f"rgba16_40x70{tag}"] = kind_file(rng, 40, 70, 6, 16, R.PATTERNS["cycle"](70), i)
        files[f"rgba16_700x9{tag}"] = kind_file(rng, 700, 9, 6, 16, R.PATTERNS["reverse"](9), i)
    files["rgb16_90x70"] = kind_file(rng, 90, 70, 2, 16, R.PATTERNS["cycle"](70))
    files["odd_grey8"] = kind_file(rng, 5, 3, 0, 8, R.PATTERNS["cycle"](3))                   # 15 bytes: the uint16 image behind it starts odd
    files["grey16_7x5"] = kind_file(rng, 7, 5, 0, 16, R.PATTERNS["cycle"](5))
    return files


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """the reference image of suite()[name] in `mode`: the reader's, after live Pillow has agreed with it (computed once, read-only)"""
    data = suite()[name]
    want = reference(data, mode)
    got = pillow(data, mode)
    assert want.dtype == got.dtype and want.shape == got.shape and np.array_equal(want, got), f"{name} ({mode}): the reader and Pillow differ"
    want.setflags(write=False)
    return want


def mixed():
    """-> (names, modes): more than 80 tiny files of both suites' kinds -- interlaced and not, 8-bit, packed and 16-bit -- shuffled, a
    mode per file; names of tests/png_reference.py's suite carry the prefix "R:" """
    S = suite()
    names = [n for n in sorted(S) if n.startswith(("f13x7_cycle", "f9x9_reverse", "s5x4", "s9x2", "s3x8", "s1x1", "s8x8", "s2x9"))]
    names += ["R:" + n for n in sorted(R.suite()) if n.startswith(("f13x7_reverse", "w2_"))]
    names += ["odd_grey8", "grey16_7x5"]
    order = np.random.default_rng(9).permutation(len(names))
    names = [names[i] for i in order]
    modes = [("RGB", "auto")[(i * 7 + 3) % 5 % 2] for i in range(len(names))]
    return names, modes


def lookup(name):
    return R.suite()[name[2:]] if name.startswith("R:") else suite()[name]


def lookup_expected(name, mode):
    return R.expected(name[2:], mode) if name.startswith("R:") else expected(name, mode)


def corrupt_files():
    """name -> file bytes: interlaced files whose data is wrong (11 x 10 RGB8: every pass has pixels)"""
    rng = np.random.default_rng(8)
    w, h = 11, 10
    s = R.random_samples(rng, w, h, 8, 2)
    plain = len(scanlines(w, h, 8, 2, s, 0, 0))
    last_row = 1 + 3 * len(pass_pixels(w, h, 7)[1])
    return {
        "filter5": make_png(w, h, 8, 2, s, {1: 1, 2: 2, 3: [5], 4: 4, 5: 3, 6: 1, 7: 4}, 1),                 # a filter byte 5 in pass 3
        "short": make_png(w, h, 8, 2, s, 1, 1, raw_edit=lambda raw: raw[:len(raw) - last_row]),                # one row of pass 7 too few
        "plain_size": make_png(w, h, 8, 2, s, 0, 1, raw_edit=lambda raw: (raw + bytes(plain))[:plain]),      # the non-interlaced size
    }
