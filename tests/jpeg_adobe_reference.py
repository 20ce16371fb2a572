"""Test files and pixel rules for the colour models that are not YCbCr: four-component files (CMYK, YCCK) and RGB-coded ones, as
``standard_jpeg_decode_many(..., adobe=True)`` takes them.  Pillow's decode of a file is always the expected result; what is here makes
the files -- through Pillow where Pillow can write the layout, through a small baseline writer where it cannot (component 3 at
component 0's sampling factors: what Photoshop writes, an MCU of 6 or 10 blocks) -- and states the per-pixel rules in numpy, which the
host tests check against Pillow so that the reference is itself checked on the CPU.
"""
import io

import numpy as np

from jfif_reference import AC_CHROMA, AC_LUMA, DC_CHROMA, DC_LUMA, ZIGZAG, _Bits, _category, huff_codes, quant_tables

KINDS = ("cmyk", "ycck", "plain", "rgb")             # plain: four components without an APP14 marker, which libjpeg reads as CMYK
LAYOUTS = ("1x1", "2x1", "2x2")                      # component 0's factors, every other component 1 x 1 (what Pillow writes)
LAYOUTS_K = ("2x1k", "2x2k")                         # component 3 at component 0's factors: K at full resolution (the writer below)


# ---- the pixel rules ----------------------------------------------------------------------------------------------------------------------
def muldiv255(a, b):
    """Pillow's MULDIV255 (ImagingUtils.h)"""
    t = a.astype(np.int64) * b + 128
    return ((t >> 8) + t) >> 8


def cmyk_to_rgb(cmyk):
    """Pillow's cmyk2rgb (Convert.c): uint8 [..., 4] mode "CMYK" pixels -> uint8 [..., 3]"""
    c = cmyk.astype(np.int64)
    nk = 255 - c[..., 3:4]
    return np.clip(nk - muldiv255(c[..., :3], nk), 0, 255).astype(np.uint8)


def ycc_to_rgb(y, cb, cr):
    """libjpeg's YCbCr -> RGB (jdcolor.c, 16-bit fixed point), clamped: int arrays -> uint8 [..., 3]"""
    y, cb, cr = (np.asarray(v, np.int64) for v in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def cmyk_pixels(samples):
    """decoded samples uint8 [..., 4] of a CMYK file -> Pillow's mode "CMYK" pixels: the "CMYK;I" unpacker inverts every channel"""
    return (255 - samples.astype(np.int64)).astype(np.uint8)


def ycck_pixels(samples):
    """decoded samples uint8 [..., 4] of a YCCK file -> Pillow's mode "CMYK" pixels: libjpeg's ycck_cmyk_convert writes 255 - R,
    255 - G, 255 - B and K, and Pillow inverts all four"""
    s = samples.astype(np.int64)
    return np.concatenate([ycc_to_rgb(s[..., 0], s[..., 1], s[..., 2]), (255 - s[..., 3:4]).astype(np.uint8)], -1)


# ---- pictures and Pillow ---------------------------------------------------------------------------------------------------------------------
def picture(H, W, channels, seed=5, noise=40):
    """smooth ramps of different periods per channel under noise: every channel, K included, has structure the up-sampling filters see"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 9 + y * 3) % 256, 255 - (x * 5 + y * 11) % 256, (x * 2 + y * 7 + 90) % 256, (x * 13 + y * 4 + 30) % 256], -1)[..., :channels]
    return np.clip(base + rng.integers(-noise, noise + 1, (H, W, channels)), 0, 255).astype(np.uint8)


def noise_picture(H, W, channels, seed=9):
    return np.random.default_rng(seed).integers(0, 256, (H, W, channels), dtype=np.uint8)


def pillow_pixels(data):
    """-> (np.asarray(Image.open(f)), np.asarray(Image.open(f).convert("RGB")))"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im).copy(), np.asarray(im.convert("RGB")).copy()


def _save(a, mode, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


# ---- marker surgery ----------------------------------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, start, end)] of the marker segments in front of the first SOS (start: the 0xFF, end: past the payload)"""
    out, p = [], 2
    while data[p + 1] != 0xDA:
        n = data[p + 2] << 8 | data[p + 3]
        out.append((data[p + 1], p, p + 2 + n))
        p += 2 + n
    return out


def app14(transform):
    return b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])


def set_transform(data, transform):
    """the APP14 transform byte -- the 12th byte after 'Adobe' starts -- set to `transform`"""
    (s,) = [s for m, s, e in segments(data) if m == 0xEE and data[s + 4:s + 9] == b"Adobe"]
    return data[:s + 15] + bytes([transform]) + data[s + 16:]


def drop_segments(data, marker):
    for m, s, e in reversed(segments(data)):
        if m == marker:
            data = data[:s] + data[e:]
    return data


def replace_app0_by_app14(data, transform=0):
    """a JFIF file -> the same scan without JFIF and with an Adobe marker: three components that libjpeg reads as RGB"""
    (s, e), = [(s, e) for m, s, e in segments(data) if m == 0xE0]
    return data[:s] + app14(transform) + data[e:]


# ---- a writer for any sampling factors, baseline or spectral-selection progressive -----------------------------------------------------------
def _put_dc(bits, codes, diff):
    n = _category(diff)
    bits.put(*codes[n])
    if n:
        bits.put(diff if diff >= 0 else diff - 1, n)


def _put_ac(bits, codes, blk):
    """coefficients 1..63 of one block: (run, size) symbols, ZRL, EOB -- a baseline block's, and equally a progressive AC first scan's of
    the whole band with Al = 0 and every end-of-band run of length 1"""
    run = 0
    for k in range(1, 64):
        val = int(blk[k])
        if val == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*codes[0xF0])
            run -= 16
        n = _category(val)
        bits.put(*codes[run << 4 | n])
        bits.put(val if val >= 0 else val - 1, n)
        run = 0
    if run:
        bits.put(*codes[0x00])


def write_baseline(W, H, comps, quality=90, transform=None, restart_interval=0, ids=None, progressive=False):
    """A file from quantised blocks.  comps: [(h, v, blocks)] per component, blocks int [mcuy * v][mcux * h][64] in zigzag order --
    every block of the MCU grid, dummy ones included.  Component 0 takes quantisation table 0 and the Annex K luminance Huffman tables,
    the others table 1 and the chrominance ones (libjpeg's defaults for every colour space but that is no concern of a decoder).
    transform: the APP14 marker's, None for no marker.  progressive=False: one interleaved sequential scan (SOF0), with restart markers
    every restart_interval MCUs.  progressive=True: SOF2 with the shape of libjpeg's script and no successive approximation -- one
    interleaved DC scan of all components (Ss = Se = 0, Al = 0), then one AC scan per component over the whole band (Ss = 1, Se = 63,
    Al = 0), which walks the component's OWN block grid: ceil(ceil(W h / hmax) / 8) columns, not the MCU grid's (T.81 A.2.2).  A complete
    progression, so libjpeg does not smooth.  -> bytes"""
    assert not (progressive and restart_interval)
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    out = bytearray(b"\xff\xd8")
    if transform is not None:
        out += app14(transform)
    for t, q in enumerate(quant_tables(quality)):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(v) for v in q[ZIGZAG])
    out += (b"\xff\xc2" if progressive else b"\xff\xc0") + (8 + 3 * len(comps)).to_bytes(2, "big") + b"\x08" + H.to_bytes(2, "big") + \
        W.to_bytes(2, "big") + bytes([len(comps)])
    ids = ids or list(range(1, len(comps) + 1))
    for i, (h, v, _) in enumerate(comps):
        out += bytes([ids[i], h << 4 | v, 0 if i == 0 else 1])
    tables = {0x00: DC_LUMA, 0x01: DC_CHROMA, 0x10: AC_LUMA, 0x11: AC_CHROMA}
    for tc, (bits, vals) in tables.items():
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc]) + bytes(bits) + bytes(vals)
    if restart_interval:
        out += b"\xff\xdd\x00\x04" + restart_interval.to_bytes(2, "big")
    out += b"\xff\xda" + (6 + 2 * len(comps)).to_bytes(2, "big") + bytes([len(comps)])
    for i in range(len(comps)):
        out += bytes([ids[i], 0x00 if i == 0 else 0x11])
    out += b"\x00\x00\x00" if progressive else b"\x00\x3f\x00"
    dc = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
    ac = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]
    bits, pred, rst = _Bits(), [0] * len(comps), 0
    for mcu in range(mcux * mcuy):
        if restart_interval and mcu and mcu % restart_interval == 0:
            out += bits.flush() + bytes([0xFF, 0xD0 + rst % 8])
            bits, pred, rst = _Bits(), [0] * len(comps), rst + 1
        my, mx = divmod(mcu, mcux)
        for i, (h, v, blocks) in enumerate(comps):
            t = 0 if i == 0 else 1
            for dy in range(v):
                for dx in range(h):
                    blk = blocks[my * v + dy][mx * h + dx]
                    _put_dc(bits, dc[t], int(blk[0]) - pred[i])
                    pred[i] = int(blk[0])
                    if not progressive:
                        _put_ac(bits, ac[t], blk)
    out += bits.flush()
    for i, (h, v, blocks) in enumerate(comps if progressive else []):
        out += b"\xff\xda\x00\x08\x01" + bytes([ids[i], 0x00 if i == 0 else 0x11]) + b"\x01\x3f\x00"
        bits = _Bits()
        for by in range(-(-(-(-H * v // vmax)) // 8)):
            for bx in range(-(-(-(-W * h // hmax)) // 8)):
                _put_ac(bits, ac[0 if i == 0 else 1], blocks[by][bx])
        out += bits.flush()
    return bytes(out + b"\xff\xd9")


def random_blocks(rng, rows, cols, amplitude=250):
    """quantised blocks [rows][cols][64], zigzag order: a DC that wanders and a dozen low-frequency AC terms: under the quality-90 tables the samples
    fill 0..255 and some leave it (the range limit), and every up-sampling neighbour matters"""
    b = np.zeros((rows, cols, 64), np.int64)
    b[..., 0] = rng.integers(-amplitude, amplitude + 1, (rows, cols))
    b[..., 1:13] = rng.integers(-15, 16, (rows, cols, 12)) * (rng.random((rows, cols, 12)) < 0.6)
    b[..., 40] = rng.integers(-1, 2, (rows, cols))       # a long zero run (a ZRL symbol) in most blocks
    return b


def photoshop_file(kind, layout, W, H, seed=21, restart_interval=0, progressive=False):
    """four components with component 3 at component 0's factors (layout "2x1k" / "2x2k"): an MCU of 6 / 10 blocks"""
    h, v = (2, 1) if layout == "2x1k" else (2, 2)
    rng = np.random.default_rng(seed)
    mcux, mcuy = -(-W // (8 * h)), -(-H // (8 * v))
    comps = [(h, v, random_blocks(rng, mcuy * v, mcux * h)), (1, 1, random_blocks(rng, mcuy, mcux)), (1, 1, random_blocks(rng, mcuy, mcux)),
             (h, v, random_blocks(rng, mcuy * v, mcux * h))]
    return write_baseline(W, H, comps, transform={"cmyk": 0, "ycck": 2, "plain": None}[kind], restart_interval=restart_interval,
                          progressive=progressive)


def make_file(kind, layout, W, H, progressive=False, quality=88, seed=5, noise=40, **kw):
    """One test file.  kind: KINDS; layout: LAYOUTS (through Pillow) or, for the four-component kinds, LAYOUTS_K (the writer above,
    progressive: its spectral-selection script).  kw goes to Pillow's save (restart_marker_rows=, restart_marker_blocks=, ...)."""
    assert kind in KINDS and layout in LAYOUTS + LAYOUTS_K
    if layout in LAYOUTS_K:
        assert kind != "rgb"
        return photoshop_file(kind, layout, W, H, seed, progressive=progressive, **kw)
    ss = LAYOUTS.index(layout)
    if kind == "rgb":
        a = picture(H, W, 3, seed, noise)
        if ss == 0:                                      # ids 'R','G','B', APP14 transform 0, no JFIF; Pillow refuses keep_rgb with subsampling
            return _save(a, "RGB", quality=quality, keep_rgb=True, progressive=progressive, **kw)
        return replace_app0_by_app14(_save(a, "RGB", quality=quality, subsampling=ss, progressive=progressive, **kw))
    data = _save(picture(H, W, 4, seed, noise), "CMYK", quality=quality, subsampling=ss, progressive=progressive, **kw)      # APP14 transform 0
    if kind == "ycck":
        return set_transform(data, 2)
    if kind == "plain":
        return drop_segments(data, 0xEE)
    return data
