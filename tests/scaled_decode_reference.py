"""An independent NumPy model of the scaled JPEG decode (standard_jpeg_decode_many(..., scale=2 / 4 / 8)): what libjpeg returns for
scale_num / scale_denom = 1 / s, which is what Pillow returns once ``Image.draft()`` has chosen scale s.  Integer arithmetic on int64
arrays, written from libjpeg's rules (jidctred.c, jdmaster.c, jdsample.c), not from the library's HIP functions:

  * m = 8 / s is the luma IDCT size.  A component starts at n = m and doubles while n < 8 and both (hmax * m) % (h * n * 2) and
    (vmax * m) % (v * n * 2) are 0: 4:2:0 chroma gets 2m and comes out at luma resolution, 4:2:2 chroma stays at m.
  * the 4 x 4, 2 x 2 and 1 x 1 inverse DCTs below; the 8 x 8 one (4:2:0 chroma at scale 2) is tests/jfif_reference.py's.
  * 4:2:2 chroma is up-sampled with the h2v1 "fancy" filter at scales 2 and 4 (plain replication for a plane at most 2 samples wide)
    and with plain replication at scale 8, where the smallest IDCT is 1 x 1 and libjpeg switches fancy up-sampling off.

    rgb = decode(data, scale)                   # uint8 [ceil(H / s)][ceil(W / s)][3]
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


_COEF = {}


def decode(data, scale):
    """uint8 [ceil(H / scale)][ceil(W / scale)][3] of a baseline or complete progressive file"""
    assert scale in (1, 2, 4, 8)
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
        b = idct_reduced(coef[c].reshape(g["ah"], g["aw"], 8, 8), qts[c], n)
        p = b.swapaxes(1, 2).reshape(g["ah"] * n, g["aw"] * n)
        planes.append(p[:-(-H * g["v"] * n // (vmax * 8)), :-(-W * g["h"] * n // (hmax * 8))])      # the component's real size
    y = planes[0]
    oh, ow = y.shape
    assert (oh, ow) == (-(-H // scale), -(-W // scale))
    if len(planes) == 1:
        return np.stack([y, y, y], -1).astype(np.uint8)
    cb, cr = planes[1], planes[2]
    if (hmax, vmax) == (2, 2) and scale == 1:                      # full size: h2v2 fancy, as tests/jfif_reference.py has it
        cb, cr = J._upsample(cb, H, W), J._upsample(cr, H, W)
    elif cb.shape != y.shape:                                      # 4:2:2: the one layout still up-sampled below full size
        assert (hmax, vmax) == (2, 1) and cb.shape == (oh, -(-ow // 2))
        if scale == 8:
            cb, cr = np.repeat(cb, 2, 1)[:, :ow], np.repeat(cr, 2, 1)[:, :ow]
        else:
            cb, cr = P._upsample_h2v1(cb, ow), P._upsample_h2v1(cr, ow)
    return J.ycc_to_rgb(y, cb, cr)
