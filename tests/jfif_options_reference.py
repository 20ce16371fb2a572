"""The numpy restatement of tests/jfif_reference.py extended to Pillow's ``subsampling=`` (4:4:4, 4:2:2, 4:2:0) and ``optimize=True``:
the MCU geometry and the h2v1 / full-size chroma paths of libjpeg's published algorithm, the symbol histogram of a scan, and T.81
Annex K.2 as libjpeg builds optimal Huffman tables from it.  ``encode`` returns the .jpg bytes, ``decode`` the pixels Pillow's decoder
returns for them.  tests/test_jfif_options_host.py pins it to Pillow; the GPU kernels (csrc/jfif.hip) are compared against it.
"""
import numpy as np

import jfif_reference as R

FACTORS = {0: (1, 1), 1: (2, 1), 2: (2, 2), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}      # luma (h, v) sampling factors


def planes(rgb, hs, vs):
    """-> (Y [8 ceil(H/8)][8 ceil(W/8)], Cb, Cr [8 ceil(H/(8 vs))][8 ceil(W/(8 hs))]) int64, edges padded as libjpeg does"""
    H, W = rgb.shape[:2]
    y, cb, cr = R._rgb_to_ycc(rgb)
    Y = np.pad(y, ((0, -H % 8), (0, -W % 8)), mode="edge")
    my, mx = -(-H // (8 * vs)), -(-W // (8 * hs))
    out = []
    for c in (cb, cr):
        c = np.pad(c, ((0, -H % vs), (0, 8 * hs * mx - W)), mode="edge")
        if (hs, vs) == (2, 2):
            s = c[0::2, 0::2] + c[1::2, 0::2] + c[0::2, 1::2] + c[1::2, 1::2]
            d = (s + np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2)) >> 2
        elif (hs, vs) == (2, 1):
            s = c[:, 0::2] + c[:, 1::2]
            d = (s + np.arange(s.shape[1]) % 2) >> 1
        else:
            d = c
        out.append(np.pad(d, ((0, 8 * my - d.shape[0]), (0, 0)), mode="edge"))
    return Y, out[0], out[1]


def coefficients(rgb, q, subsampling=2):
    """-> list of (component, [64] int64 zigzag) in scan order, dummy luma blocks included (DC of the block before, no AC)"""
    hs, vs = FACTORS[subsampling]
    H, W = rgb.shape[:2]
    Y, Cb, Cr = planes(rgb, hs, vs)
    lq, cq = R.quant_tables(q)
    qy = R.quantise(R.fdct(R._blocks(Y)), lq)
    qc = [R.quantise(R.fdct(R._blocks(c)), cq) for c in (Cb, Cr)]
    by, bx = qy.shape[:2]
    out = []
    for my in range(-(-H // (8 * vs))):
        for mx in range(-(-W // (8 * hs))):
            prev = None
            for dy in range(vs):
                for dx in range(hs):
                    yy, xx = vs * my + dy, hs * mx + dx
                    if yy < by and xx < bx:
                        blk = qy[yy, xx].reshape(64)[R.ZIGZAG]
                    else:
                        blk = np.zeros(64, np.int64)
                        blk[0] = prev[0]
                    out.append((0, blk))
                    prev = blk
            out.append((1, qc[0][my, mx].reshape(64)[R.ZIGZAG]))
            out.append((2, qc[1][my, mx].reshape(64)[R.ZIGZAG]))
    return out


def _walk(blocks):
    """the scan as (table class 0 DC / 1 AC, table id 0 luma / 1 chroma, symbol, extra bits value, extra bits count)"""
    pred = [0, 0, 0]
    for comp, blk in blocks:
        t = 1 if comp else 0
        diff = int(blk[0]) - pred[comp]
        pred[comp] = int(blk[0])
        n = R._category(diff)
        yield 0, t, n, diff if diff >= 0 else diff - 1, n
        run = 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                yield 1, t, 0xF0, 0, 0
                run -= 16
            n = R._category(v)
            yield 1, t, (run << 4) | n, v if v >= 0 else v - 1, n
            run = 0
        if run:
            yield 1, t, 0x00, 0, 0


def histogram(blocks):
    """-> int64 [4][257]: counts of the symbols the scan writes, in DHT order (DC luma, AC luma, DC chroma, AC chroma)"""
    h = np.zeros((4, 257), np.int64)
    for cls, t, sym, _, _ in _walk(blocks):
        h[2 * t + cls, sym] += 1
    return h


def optimal_table(counts):
    """T.81 K.2 as libjpeg's jpeg_gen_optimal_table does it: 257 counts (entry 256 is the reserved all-ones code and is set to 1)
    -> (BITS[1..16], HUFFVAL).  Ties between equal counts go to the larger symbol index."""
    freq = [int(v) for v in counts[:256]] + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        v = None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        v = None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1                                         # every symbol of both trees moves one level down
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2                                           # and c2's chain is appended to c1's
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    longest = max(codesize)
    bits = [0] * (max(longest, 16) + 1)
    for n in codesize:
        if n:
            bits[n] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                  # the reserved code leaves the longest length in use
    vals = [j for n in range(1, longest + 1) for j in range(256) if codesize[j] == n]
    return bits[1:17], vals


def tables(blocks, optimize):
    """the four (BITS, HUFFVAL) tables of a file in DHT order"""
    if not optimize:
        return [R.DC_LUMA, R.AC_LUMA, R.DC_CHROMA, R.AC_CHROMA]
    return [optimal_table(h) for h in histogram(blocks)]


def entropy(blocks, tabs):
    codes = [R.huff_codes(t) for t in tabs]
    bits = R._Bits()
    for cls, t, sym, extra, n in _walk(blocks):
        bits.put(*codes[2 * t + cls][sym])
        if n:
            bits.put(extra, n)
    return bits.flush()


def headers(q, H, W, subsampling=2, tabs=None):
    """SOI .. SOS with the layout's sampling factors and the given tables (Annex K by default)"""
    hs, vs = FACTORS[subsampling]
    tabs = tables(None, False) if tabs is None else tabs
    lq, cq = R.quant_tables(q)
    out = b"\xff\xd8" + R._seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate((lq, cq)):
        out += R._seg(0xDB, bytes([i]) + bytes(int(v) for v in t[R.ZIGZAG]))
    out += R._seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_id, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), tabs):
        out += R._seg(0xC4, bytes([cls_id]) + bytes(bits) + bytes(vals))
    return out + R._seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(rgb, q, subsampling=2, optimize=False):
    """uint8 [H, W, 3] -> the bytes of PIL.Image.fromarray(rgb).save(buf, "JPEG", quality=q, subsampling=subsampling, optimize=optimize)"""
    H, W = rgb.shape[:2]
    blocks = coefficients(rgb, q, subsampling)
    tabs = tables(blocks, optimize)
    return headers(q, H, W, subsampling, tabs) + entropy(blocks, tabs) + b"\xff\xd9"


def _upsample(c, H, W, hs, vs):
    if (hs, vs) == (2, 2):
        return R._upsample(c, H, W)
    if hs == 1:
        return c[:H, :W]
    w = -(-W // 2)                                               # h2v1: fancy, or replication when the chroma is at most 2 wide
    c = c[:H, :w]
    if w <= 2:
        return np.repeat(c, 2, 1)[:, :W]
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((H, 2 * w), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out[:, :W]


def decode(rgb, q, subsampling=2):
    """uint8 [H, W, 3] -> np.asarray(Image.open(<its file>).convert("RGB")) (the Huffman tables do not change the pixels)"""
    hs, vs = FACTORS[subsampling]
    H, W = rgb.shape[:2]
    lq, cq = R.quant_tables(q)
    pl = []
    for p, t in zip(planes(rgb, hs, vs), (lq, cq, cq)):
        b = R.idct(R.quantise(R.fdct(R._blocks(p)), t), t)
        pl.append(b.swapaxes(1, 2).reshape(p.shape))
    return R.ycc_to_rgb(pl[0][:H, :W], _upsample(pl[1], H, W, hs, vs), _upsample(pl[2], H, W, hs, vs))
