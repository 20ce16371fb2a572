"""A numpy restatement of baseline JPEG as libjpeg(-turbo) writes and reads it with Pillow's defaults (4:2:0, Annex K tables, islow DCT,
fancy up-sampling), from the published algorithm.  ``encode`` returns the .jpg bytes, ``decode`` the RGB pixels Pillow's decoder returns
for them, and ``quant_tables`` / ``headers`` the pieces on their own.  The GPU kernels (csrc/jfif.hip) are compared against it.
"""
import numpy as np

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                  + [99] * 32, np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# Annex K.3 Huffman tables: (BITS[1..16], HUFFVAL)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8"
    "c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def huff_codes(table):
    """symbol -> (code, length) of a (BITS, HUFFVAL) table (Annex C)"""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_tables(q):
    """(luma, chroma) int64 [64] in natural order, Pillow's quality scaling with baseline clamping"""
    q = min(max(int(q), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (LUMA, CHROMA))


def _fix(x):
    return int(x * 65536 + 0.5)


def _rgb_to_ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    half = 1 << 15
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + half) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + half - 1) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + half - 1) >> 16
    return y, cb, cr


def planes(rgb):
    """-> (Y [8 ceil(H/8)][8 ceil(W/8)], Cb, Cr [8 ceil(H/16)][8 ceil(W/16)]) int64 sample planes, edges padded as libjpeg does"""
    H, W = rgb.shape[:2]
    y, cb, cr = _rgb_to_ycc(rgb)
    by, bx = -(-H // 8), -(-W // 8)
    Y = np.pad(y, ((0, 8 * by - H), (0, 8 * bx - W)), mode="edge")
    cy, cx = -(-H // 16), -(-W // 16)
    out = []
    for c in (cb, cr):
        c = np.pad(c, ((0, H % 2), (0, 16 * cx - W)), mode="edge")
        s = c[0::2, 0::2] + c[1::2, 0::2] + c[0::2, 1::2] + c[1::2, 1::2]
        bias = np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2)
        d = (s + bias) >> 2
        out.append(np.pad(d, ((0, 8 * cy - d.shape[0]), (0, 0)), mode="edge"))
    return Y, out[0], out[1]


F = {k: v for k, v in dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069,
                            f2053=16819, f2562=20995, f3072=25172).items()}


def _desc(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, shift_even, shift_odd, pass1):
    """one pass of jfdctint over axis -1 of d (int64 [..., 8])"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = np.empty_like(d)
    if pass1:
        o[..., 0], o[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[..., 0], o[..., 4] = _desc(t10 + t11, 2), _desc(t10 - t11, 2)
    z1 = (t12 + t13) * F["f0541"]
    o[..., 2] = _desc(z1 + t13 * F["f0765"], shift_even)
    o[..., 6] = _desc(z1 - t12 * F["f1847"], shift_even)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F["f1175"]
    t4, t5, t6, t7 = t4 * F["f0298"], t5 * F["f2053"], t6 * F["f3072"], t7 * F["f1501"]
    z1, z2, z3, z4 = z1 * -F["f0899"], z2 * -F["f2562"], z3 * -F["f1961"] + z5, z4 * -F["f0390"] + z5
    o[..., 7] = _desc(t4 + z1 + z3, shift_odd)
    o[..., 5] = _desc(t5 + z2 + z4, shift_odd)
    o[..., 3] = _desc(t6 + z2 + z3, shift_odd)
    o[..., 1] = _desc(t7 + z1 + z4, shift_odd)
    return o


def fdct(blocks):
    """jfdctint (islow) of int64 [..., 8, 8] samples after the -128 level shift; output scaled by 8 as libjpeg leaves it"""
    d = _fdct_1d(blocks - 128, 11, 11, True)
    return np.swapaxes(_fdct_1d(np.swapaxes(d, -1, -2), 15, 15, False), -1, -2)


def quantise(c, qtab):
    q = (8 * qtab).reshape(8, 8)
    a = (np.abs(c) + (q >> 1)) // q
    return np.where(c < 0, -a, a)


def _blocks(p):
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)      # [by][bx][8][8]


def coefficients(rgb, q):
    """-> list of (component, [64] int64 zigzag) in scan order, dummy blocks included"""
    H, W = rgb.shape[:2]
    Y, Cb, Cr = planes(rgb)
    lq, cq = quant_tables(q)
    qy = quantise(fdct(_blocks(Y)), lq)
    qc = [quantise(fdct(_blocks(c)), cq) for c in (Cb, Cr)]
    by, bx = qy.shape[:2]
    out = []
    for my in range(-(-H // 16)):
        for mx in range(-(-W // 16)):
            prev = None
            for dy in range(2):
                for dx in range(2):
                    yy, xx = 2 * my + dy, 2 * mx + dx
                    if yy < by and xx < bx:
                        blk = qy[yy, xx].reshape(64)[ZIGZAG]
                    else:
                        blk = np.zeros(64, np.int64)
                        blk[0] = prev[0]
                    out.append((0, blk))
                    prev = blk
            out.append((1, qc[0][my, mx].reshape(64)[ZIGZAG]))
            out.append((2, qc[1][my, mx].reshape(64)[ZIGZAG]))
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _category(v):
    return int(abs(int(v))).bit_length()


def entropy(blocks):
    """Huffman-coded scan data (byte-stuffed, padded with 1-bits) of coefficients(...)"""
    dc = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
    ac = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]
    pred = [0, 0, 0]
    bits = _Bits()
    for comp, blk in blocks:
        t = 1 if comp else 0
        diff = int(blk[0]) - pred[comp]
        pred[comp] = int(blk[0])
        n = _category(diff)
        bits.put(*dc[t][n])
        if n:
            bits.put(diff if diff >= 0 else diff - 1, n)
        run = 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                bits.put(*ac[t][0xF0])
                run -= 16
            n = _category(v)
            bits.put(*ac[t][(run << 4) | n])
            bits.put(v if v >= 0 else v - 1, n)
            run = 0
        if run:
            bits.put(*ac[t][0x00])
    return bits.flush()


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def headers(q, H, W):
    """SOI .. SOS (everything before the scan data)"""
    lq, cq = quant_tables(q)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate((lq, cq)):
        out += _seg(0xDB, bytes([i]) + bytes(int(v) for v in t[ZIGZAG]))
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_id, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _seg(0xC4, bytes([cls_id]) + bytes(bits) + bytes(vals))
    return out + _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(rgb, q):
    """uint8 [H, W, 3] -> the bytes of PIL.Image.fromarray(rgb).save(buf, "JPEG", quality=q)"""
    H, W = rgb.shape[:2]
    return headers(q, H, W) + entropy(coefficients(rgb, q)) + b"\xff\xd9"


# ---- reconstruction: what libjpeg's decoder returns for those coefficients ----------------------------------------------------------
def _idct_1d(d, pass1):
    """one pass of jidctint over axis -1 (pass1 on dequantised coefficients, pass 2 on the workspace)"""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * F["f0541"]
    t2, t3 = z1 - z3 * F["f1847"], z1 + z2 * F["f0765"]
    t0, t1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F["f1175"]
    t0, t1, t2, t3 = t0 * F["f0298"], t1 * F["f2053"], t2 * F["f3072"], t3 * F["f1501"]
    z1, z2, z3, z4 = z1 * -F["f0899"], z2 * -F["f2562"], z3 * -F["f1961"] + z5, z4 * -F["f0390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 11 if pass1 else 18
    o = np.empty_like(d)
    o[..., 0], o[..., 7] = _desc(t10 + t3, n), _desc(t10 - t3, n)
    o[..., 1], o[..., 6] = _desc(t11 + t2, n), _desc(t11 - t2, n)
    o[..., 2], o[..., 5] = _desc(t12 + t1, n), _desc(t12 - t1, n)
    o[..., 3], o[..., 4] = _desc(t13 + t0, n), _desc(t13 - t0, n)
    return o


def range_limit(x):
    """libjpeg's masked IDCT range limit of the output before the +128 shift"""
    m = x & 1023
    return np.where(m < 128, m + 128, np.where(m < 512, 255, np.where(m < 896, 0, m - 896)))


def idct(coef, qtab):
    """[..., 8, 8] quantised coefficients (natural order) -> samples"""
    d = coef * qtab.reshape(8, 8)
    ws = np.swapaxes(_idct_1d(np.swapaxes(d, -1, -2), True), -1, -2)      # columns first
    return range_limit(_idct_1d(ws, False))


def _upsample(c, H, W):
    """h2v2 fancy up-sampling of the real ceil(H/2) x ceil(W/2) chroma samples -> [H][W].  libjpeg-turbo turns it off when the chroma
    is at most 2 samples wide (W <= 4) and replicates each sample 2 x 2 instead."""
    h, w = -(-H // 2), -(-W // 2)
    c = c[:h, :w]
    if w <= 2:
        return np.repeat(np.repeat(c, 2, 0), 2, 1)[:H, :W]
    above = np.concatenate([c[:1], c[:-1]])
    below = np.concatenate([c[1:], c[-1:]])
    rows = np.empty((2 * h, w), np.int64)
    rows[0::2] = 3 * c + above
    rows[1::2] = 3 * c + below
    left = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
    out = np.empty((2 * h, 2 * w), np.int64)
    out[:, 0::2] = (3 * rows + left + 8) >> 4
    out[:, 1::2] = (3 * rows + right + 7) >> 4
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr):
    half = 1 << 15
    cbx, crx = cb - 128, cr - 128
    r = y + ((_fix(1.402) * crx + half) >> 16)
    g = y + ((-_fix(0.34414) * cbx + half - _fix(0.71414) * crx) >> 16)
    b = y + ((_fix(1.772) * cbx + half) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(rgb, q):
    """uint8 [H, W, 3] -> np.asarray(Image.open(<its file>).convert("RGB"))"""
    H, W = rgb.shape[:2]
    Y, Cb, Cr = planes(rgb)
    lq, cq = quant_tables(q)
    pl = []
    for p, t in ((Y, lq), (Cb, cq), (Cr, cq)):
        b = idct(quantise(fdct(_blocks(p)), t), t)
        pl.append(b.swapaxes(1, 2).reshape(p.shape))
    return ycc_to_rgb(pl[0][:H, :W], _upsample(pl[1], H, W), _upsample(pl[2], H, W))
