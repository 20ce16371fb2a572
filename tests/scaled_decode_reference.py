"""An independent NumPy model of the scaled JPEG decode (standard_jpeg_decode_many(..., scale=2 / 4 / 8)): what libjpeg returns for
scale_num / scale_denom = 1 / s, which is what Pillow returns once ``Image.draft()`` has chosen scale s.  Integer arithmetic on int64
arrays, written from libjpeg's rules (jidctred.c, jdmaster.c, jdsample.c), not from the library's HIP functions:

  * m = 8 / s is the luma IDCT size.  A component starts at n = m and doubles while n < 8 and both (hmax * m) % (h * n * 2) and
    (vmax * m) % (v * n * 2) are 0: 4:2:0 chroma gets 2m and comes out at luma resolution, 4:2:2 chroma stays at m.
  * the 4 x 4, 2 x 2 and 1 x 1 inverse DCTs below; the 8 x 8 one (4:2:0 chroma at scale 2) is tests/jfif_reference.py's.
  * 4:2:2 chroma is up-sampled with the h2v1 "fancy" filter at scales 2 and 4 (plain replication for a plane at most 2 samples wide)
    and with plain replication at scale 8, where the smallest IDCT is 1 x 1 and libjpeg switches fancy up-sampling off.

    rgb = decode(data, scale)                   # uint8 [ceil(H / s)][ceil(W / s)][3]; every layout the library takes, 4:4:0 included
    luma = decode(data, scale, "L")             # uint8 [ceil(H / s)][ceil(W / s)]: the luma plane, what Pillow's draft("L", ...) gives
    rgb = decode(data, 1, simd=True)            # the 8 x 8 IDCT as libjpeg-turbo's SIMD code computes it outside the range of real samples
    samples = idct_reduced(coef, qt, n)         # [..., 8, 8] quantised coefficients -> [..., n, n] samples, n in (1, 2, 4)

Coefficients come from tests/progressive_reference.py (progressive files) or from the sequential Huffman decode below (baseline
files), both plain Python."""
import numpy as np

import jfif_reference as J
import progressive_reference as P


def _descale(x, k):
    return (x + (1 << (k - 1))) >> k


def _pass4(d, k):
    """the 4-point pass over axis -1 of [..., 8]: index 4 is never read"""
    t0 = d[..., 0] << 14
    t2 = d[..., 2] * 15137 - d[..., 6] * 6270
    t10, t12 = t0 + t2, t0 - t2
    o0 = -d[..., 7] * 1730 + d[..., 5] * 11893 - d[..., 3] * 17799 + d[..., 1] * 8697
    o2 = -d[..., 7] * 4176 - d[..., 5] * 4926 + d[..., 3] * 7373 + d[..., 1] * 20995
    return np.stack([_descale(t10 + o2, k), _descale(t12 + o0, k), _descale(t12 - o0, k), _descale(t10 - o2, k)], -1)


def _pass2(d, k):
    """the 2-point pass over axis -1 of [..., 8]: only 0, 1, 3, 5, 7 are read"""
    t10 = d[..., 0] << 15
    t0 = -d[..., 7] * 5906 + d[..., 5] * 6967 - d[..., 3] * 10426 + d[..., 1] * 29692
    return np.stack([_descale(t10 + t0, k), _descale(t10 - t0, k)], -1)


def idct_reduced(coef, qt, n):
    """[..., 8, 8] quantised coefficients (natural order: [row][column]) and 64 quantisers -> [..., n, n] samples"""
    d = np.asarray(coef, np.int64) * np.asarray(qt, np.int64).reshape(8, 8)
    if n == 8:
        return J.idct(np.asarray(coef, np.int64), np.asarray(qt, np.int64))
    if n == 1:
        return J.range_limit(_descale(d[..., :1, :1], 3))
    one, k1, k2 = (_pass4, 12, 19) if n == 4 else (_pass2, 13, 20)
    ws = np.swapaxes(one(np.swapaxes(d, -1, -2), k1), -1, -2)      # pass 1 down every column: [..., n rows, 8 columns]
    return J.range_limit(one(ws, k2))                              # pass 2 along every row (the unused columns are not read)


def idct_size(h, v, hmax, vmax, m):
    n = m
    while n < 8 and (hmax * m) % (h * n * 2) == 0 and (vmax * m) % (v * n * 2) == 0:
        n *= 2
    return n


def baseline_coefficients(data):
    """Quantised coefficients of a baseline (SOF0 / SOF1, one interleaved scan) file, laid out as progressive_reference.coefficients"""
    frame, scans = P.walk(data)
    (sc,) = scans
    mx, my, geo = P._geometry(frame)
    coef = [np.zeros((g["ah"], g["aw"], 64), np.int64) for g in geo]
    units = [[(c, y * geo[c]["v"] + j, x * geo[c]["h"] + i) for (c, _, _) in sc["comps"] for j in range(geo[c]["v"])
              for i in range(geo[c]["h"])] for y in range(my) for x in range(mx)]
    ri = sc["ri"] or len(units)
    dct = {c: P._codes(sc["dc"][td]) for (c, td, _) in sc["comps"]}
    act = {c: P._codes(sc["ac"][ta]) for (c, _, ta) in sc["comps"]}
    for k, raw in enumerate(P._intervals(data, sc)):
        br = P._Bits(raw)
        pred = {c: 0 for (c, _, _) in sc["comps"]}
        for unit in units[k * ri:(k + 1) * ri]:
            for (c, by, bx) in unit:
                blk = coef[c][by, bx]
                t = br.symbol(dct[c])
                pred[c] += P._extend(br.bits(t), t)
                blk[0] = pred[c]
                z = 1
                while z < 64:
                    rs = br.symbol(act[c])
                    r, s = rs >> 4, rs & 15
                    if s:
                        z += r
                        blk[P.ZZ[z]] = P._extend(br.bits(s), s)
                        z += 1
                    elif r == 15:
                        z += 16
                    else:
                        break
    return coef


# ---- the 8 x 8 inverse DCT as libjpeg-turbo's x86 SIMD code computes it (jidctint-sse2 / -avx2: the published algorithm of jidctint.c on
# 16-bit lanes).  Inside the range real samples give it equals jfif_reference.idct; outside it differs in three places: the dequantised
# products and the 16-bit sums (in0 +- in4, the odd part's z3 and z4) wrap at 16 bits, each pass's results are packed to int16 with
# saturation, and the last step is a saturating pack to int8 plus 128 -- not the masked table of the C code.
def _wrap16(x):
    return ((x + 32768) & 65535) - 32768


def _wrap32(x):
    return ((x + (1 << 31)) & ((1 << 32) - 1)) - (1 << 31)


def _simd_pass(d, n):
    """one pass over axis -1 of int16-valued [..., 8] -> int16-valued [..., 8]"""
    F = J.F
    t2 = d[..., 2] * F["f0541"] + d[..., 6] * (F["f0541"] - F["f1847"])
    t3 = d[..., 2] * (F["f0541"] + F["f0765"]) + d[..., 6] * F["f0541"]
    t0, t1 = _wrap16(d[..., 0] + d[..., 4]) << 13, _wrap16(d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    d7, d5, d3, d1 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z3, z4 = _wrap16(d7 + d3), _wrap16(d5 + d1)
    z3, z4 = z3 * (F["f1175"] - F["f1961"]) + z4 * F["f1175"], z3 * F["f1175"] + z4 * (F["f1175"] - F["f0390"])
    o0 = d7 * (F["f0298"] - F["f0899"]) - d1 * F["f0899"] + z3
    o3 = -d7 * F["f0899"] + d1 * (F["f1501"] - F["f0899"]) + z4
    o1 = d5 * (F["f2053"] - F["f2562"]) - d3 * F["f2562"] + z4
    o2 = -d5 * F["f2562"] + d3 * (F["f3072"] - F["f2562"]) + z3
    out = np.empty_like(d)
    for k, (a, b) in enumerate(((t10, o3), (t11, o2), (t12, o1), (t13, o0))):
        a, b = _wrap32(a), _wrap32(b)
        out[..., k] = np.clip(_wrap32(_wrap32(a + b) + (1 << (n - 1))) >> n, -32768, 32767)
        out[..., 7 - k] = np.clip(_wrap32(_wrap32(a - b) + (1 << (n - 1))) >> n, -32768, 32767)
    return out


def idct_simd(coef, qt):
    """[..., 8, 8] quantised coefficients (natural order) and 64 quantisers -> [..., 8, 8] samples"""
    coef = np.asarray(coef, np.int64)
    d = _wrap16(coef * np.asarray(qt, np.int64).reshape(8, 8))
    ws = np.swapaxes(_simd_pass(np.swapaxes(d, -1, -2), 11), -1, -2)
    flat = (coef[..., 1:, :] == 0).all((-1, -2))                    # no AC term below row 0: every row is the first, shifted left in 16 bits
    ws = np.where(flat[..., None, None], _wrap16(d[..., :1, :] << 2) + np.zeros_like(d), ws)
    return np.clip(_simd_pass(ws, 18), -128, 127) + 128


_COEF = {}


def upsample_h1v2(c, H):
    """libjpeg's h1v2 "fancy" up-sampling of ceil(H / 2) real chroma rows -> [H] rows: 3/4 of the nearer row and 1/4 of the further,
    the edge rows standing in for the rows outside.  No narrow-plane exception (jdsample.c has none for this layout)."""
    h = -(-H // 2)
    c = c[:h]
    above = np.concatenate([c[:1], c[:-1]])
    below = np.concatenate([c[1:], c[-1:]])
    out = np.empty((2 * h, c.shape[1]), np.int64)
    out[0::2] = (3 * c + above + 1) >> 2
    out[1::2] = (3 * c + below + 2) >> 2
    return out[:H]


def decode(data, scale=1, mode="RGB", simd=False):
    """uint8 [ceil(H / scale)][ceil(W / scale)][3] of a baseline or complete progressive file of any layout the library takes (4:4:4,
    4:2:2, 4:2:0, 4:4:0, grey); mode "L": [ceil(H / scale)][ceil(W / scale)], the luma plane (a grey file's samples).  simd (full size
    only): the 8 x 8 inverse DCT with the semantics of libjpeg-turbo's SIMD code (idct_simd), which matters only outside the range of real samples"""
    assert scale in (1, 2, 4, 8) and mode in ("RGB", "L") and not (simd and scale != 1)
    data = bytes(data)
    frame, scans = P.walk(data)
    if data not in _COEF:                                          # the slow part, shared by the scales of one file
        _COEF[data] = P.coefficients(data) if frame["sof"] == 0xC2 else baseline_coefficients(data)
    coef = _COEF[data]
    mx, my, geo = P._geometry(frame)
    H, W = frame["height"], frame["width"]
    qts = {}
    for sc in scans:                                               # a component's table is the one in force at its first scan
        for c, q in sc["qts"].items():
            qts.setdefault(c, q)
    m = 8 // scale
    hmax, vmax = geo[0]["h"], geo[0]["v"]                          # chroma is sampled 1 x 1: the luma factors are the maxima
    planes = []
    for c, g in enumerate(geo):
        n = idct_size(g["h"], g["v"], hmax, vmax, m)
        blocks = coef[c].reshape(g["ah"], g["aw"], 8, 8)
        b = idct_simd(blocks, qts[c]) if simd else idct_reduced(blocks, qts[c], n)
        p = b.swapaxes(1, 2).reshape(g["ah"] * n, g["aw"] * n)
        planes.append(p[:-(-H * g["v"] * n // (vmax * 8)), :-(-W * g["h"] * n // (hmax * 8))])      # the component's real size
    y = planes[0]
    oh, ow = y.shape
    assert (oh, ow) == (-(-H // scale), -(-W // scale))
    if mode == "L":
        return y.astype(np.uint8)
    if len(planes) == 1:
        return np.stack([y, y, y], -1).astype(np.uint8)
    cb, cr = planes[1], planes[2]
    if (hmax, vmax) == (1, 2):                                     # 4:4:0: h1v2 fancy, replication at scale 8 (the smallest IDCT is 1 x 1)
        assert cb.shape == (-(-oh // 2), ow)
        if scale == 8:
            cb, cr = np.repeat(cb, 2, 0)[:oh], np.repeat(cr, 2, 0)[:oh]
        else:
            cb, cr = upsample_h1v2(cb, oh), upsample_h1v2(cr, oh)
    elif (hmax, vmax) == (2, 2) and scale == 1:                      # full size: h2v2 fancy, as tests/jfif_reference.py has it
        cb, cr = J._upsample(cb, H, W), J._upsample(cr, H, W)
    elif cb.shape != y.shape:                                      # 4:2:2: the one layout still up-sampled below full size
        assert (hmax, vmax) == (2, 1) and cb.shape == (oh, -(-ow // 2))
        if scale == 8:
            cb, cr = np.repeat(cb, 2, 1)[:, :ow], np.repeat(cr, 2, 1)[:, :ow]
        else:
            cb, cr = P._upsample_h2v1(cb, ow), P._upsample_h2v1(cr, ow)
    return J.ycc_to_rgb(y, cb, cr)
