"""An independent progressive-JPEG decoder in plain Python / NumPy for the tests of standard_jpeg_decode_many(..., progressive=True):
T.81 Annex G (Figures G.3 - G.7 restated) down to the quantised coefficients, then tests/jfif_reference.py's IDCT, up-sampling and
colour conversion for the pixels.  It shares nothing with the library: its own marker walk, Huffman tables, bit reader and block
addressing.  Slow by design (one Python step per symbol); meant for images of a few thousand blocks.

    frame, scans = walk(data)                   # the marker walk: frame, and every scan with the tables in force at its SOS
    coef = coefficients(data, n_scans=None)     # {component: int array [blocks_y][blocks_x][64] natural order} after the first n scans
    rgb = decode(data)                          # uint8 [H][W][3], equal to np.asarray(Image.open(file).convert("RGB"))
"""
import numpy as np

import jfif_reference as J

ZZ = [int(v) for v in J.ZIGZAG]


def walk(data):
    """-> (frame dict, [scan dict]).  A scan: components [(index, td, ta)], ss, se, ah, al, ri, dc / ac tables {selector: (counts,
    symbols)} as in force at its SOS, start / end byte offsets of its entropy-coded data, and the DHT payloads seen since the last scan."""
    assert data[:2] == b"\xff\xd8"
    p, frame, scans, ri = 2, None, [], 0
    tables = {0: {}, 1: {}}
    qts, dht_since = {}, []
    while True:
        assert data[p] == 0xFF, f"no marker at {p}"
        while data[p + 1] == 0xFF:
            p += 1
        m = data[p + 1]
        if m == 0xD9:
            break
        n = int.from_bytes(data[p + 2:p + 4], "big")
        body = data[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xC4:
            dht_since.append(bytes(body))
            i = 0
            while i < len(body):
                counts = list(body[i + 1:i + 17])
                tables[body[i] >> 4][body[i] & 15] = (counts, list(body[i + 17:i + 17 + sum(counts)]))
                i += 17 + sum(counts)
        elif m == 0xDB:
            i = 0
            while i < len(body):
                pq, tq = body[i] >> 4, body[i] & 15
                raw = body[i + 1:i + 1 + 64 * (pq + 1)]
                vals = [int.from_bytes(raw[2 * k:2 * k + 2], "big") for k in range(64)] if pq else list(raw)
                nat = [0] * 64
                for z in range(64):
                    nat[ZZ[z]] = vals[z]
                qts[tq] = nat
                i += 1 + 64 * (pq + 1)
        elif m == 0xDD:
            ri = int.from_bytes(body, "big")
        elif m in (0xC0, 0xC1, 0xC2):
            comps = [dict(id=body[6 + 3 * i], h=body[7 + 3 * i] >> 4, v=body[7 + 3 * i] & 15, tq=body[8 + 3 * i]) for i in range(body[5])]
            frame = dict(sof=m, height=int.from_bytes(body[1:3], "big"), width=int.from_bytes(body[3:5], "big"), comps=comps)
        elif m == 0xDA:
            ns = body[0]
            ids = [c["id"] for c in frame["comps"]]
            comps = [(ids.index(body[1 + 2 * i]), body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
            q = _scan_end(data, p)
            scans.append(dict(comps=comps, ss=body[1 + 2 * ns], se=body[2 + 2 * ns], ah=body[3 + 2 * ns] >> 4, al=body[3 + 2 * ns] & 15,
                              ri=ri, dc={k: v for k, v in tables[0].items()}, ac={k: v for k, v in tables[1].items()},
                              start=p, end=q, dht=dht_since, qts={c[0]: qts.get(frame["comps"][c[0]]["tq"]) for c in comps}))
            dht_since = []
            p = q
    return frame, scans


def _ff_run(data, i):
    """data[i] is 0xFF: (offset of the byte after the run of 0xFF that starts there, that byte; None at the end of the data)"""
    while i < len(data) and data[i] == 0xFF:
        i += 1
    return i, (data[i] if i < len(data) else None)


def _scan_end(data, p):
    """offset of the marker that ends the entropy-coded data starting at p, by libjpeg's rule: a run of 0xFF followed by 0x00 is one
    data 0xFF, followed by RSTn one restart marker, followed by anything else the end of the scan (the run's first byte is returned)"""
    while True:
        if data[p] != 0xFF:
            p += 1
            continue
        q, c = _ff_run(data, p)
        if c is None or not (c == 0 or 0xD0 <= c <= 0xD7):
            return p
        p = q + 1


class _Bits:
    """MSB-first reader over one restart interval's bytes (stuffing removed by _intervals)"""

    def __init__(self, raw):
        self.b, self.pos = raw, 0

    def bit(self):
        assert self.pos < 8 * len(self.b), "ran out of bits"
        v = (self.b[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return v

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, tab):
        code, length = 0, 0
        while True:
            code = (code << 1) | self.bit()
            length += 1
            if (length, code) in tab:
                return tab[(length, code)]
            assert length < 16, "no such Huffman code"


def _codes(table):
    """(counts, symbols) -> {(length, code): symbol}, canonical order (T.81 C.2)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(table[0][length - 1]):
            out[(length, code)] = table[1][k]
            code += 1
            k += 1
        code <<= 1
    return out


def _extend(v, t):
    return v if t == 0 or v >= (1 << (t - 1)) else v - (1 << t) + 1


def _intervals(data, scan):
    """the scan's restart intervals, un-stuffed, by the rule of _scan_end.  Bytes between an interval's last needed bit and the next
    marker stay at its end, where the decode of a known number of units never looks: libjpeg drops them too (with a warning)"""
    raw, out, cur, i = data[scan["start"]:scan["end"]], [], bytearray(), 0
    while i < len(raw):
        if raw[i] != 0xFF:
            cur.append(raw[i])
            i += 1
            continue
        i, c = _ff_run(raw, i)
        if c is None:                                              # fill bytes in front of the marker that ends the scan
            break
        if c == 0:
            cur.append(0xFF)
        else:
            assert 0xD0 <= c <= 0xD7
            out.append(bytes(cur))
            cur = bytearray()
        i += 1
    out.append(bytes(cur))
    return out


def _geometry(frame):
    hmax = max(c["h"] for c in frame["comps"])
    vmax = max(c["v"] for c in frame["comps"])
    if len(frame["comps"]) == 1:
        hmax = vmax = 1
    W, H = frame["width"], frame["height"]
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    g = []
    for c in frame["comps"]:
        h, v = (1, 1) if len(frame["comps"]) == 1 else (c["h"], c["v"])
        g.append(dict(h=h, v=v, bw=-(-(-(-W * h // hmax)) // 8), bh=-(-(-(-H * v // vmax)) // 8), aw=mx * h, ah=my * v))
    return mx, my, g


def coefficients(data, n_scans=None, only=None):
    """Quantised coefficients after the first n_scans scans (all by default; `only`: a set of scan indices instead):
    [component] -> int64 [allocated blocks_y][allocated blocks_x][64], natural order, the MCU-padded grid."""
    frame, scans = walk(data)
    mx, my, geo = _geometry(frame)
    coef = [np.zeros((g["ah"], g["aw"], 64), np.int64) for g in geo]
    for si, sc in enumerate(scans):
        if (only is not None and si not in only) or (only is None and n_scans is not None and si >= n_scans):
            continue
        ss, se, ah, al = sc["ss"], sc["se"], sc["ah"], sc["al"]
        if len(sc["comps"]) > 1:                                   # interleaved: MCUs, padded blocks included
            units = [[(c, y * geo[c]["v"] + j, x * geo[c]["h"] + i) for (c, _, _) in sc["comps"] for j in range(geo[c]["v"])
                      for i in range(geo[c]["h"])] for y in range(my) for x in range(mx)]
        else:                                                      # the component's own ceil(w / 8) x ceil(h / 8) blocks, raster order
            c = sc["comps"][0][0]
            units = [[(c, y, x)] for y in range(geo[c]["bh"]) for x in range(geo[c]["bw"])]
        ri = sc["ri"] or len(units)
        parts = _intervals(data, sc)
        assert len(parts) == -(-len(units) // ri), "restart marker count"
        dct = {c: _codes(sc["dc"][td]) for (c, td, _) in sc["comps"] if ss == 0 and ah == 0}
        act = {c: _codes(sc["ac"][ta]) for (c, _, ta) in sc["comps"] if ss > 0}
        for k, raw in enumerate(parts):
            br = _Bits(raw)
            pred = {c: 0 for (c, _, _) in sc["comps"]}
            eobrun = 0
            for unit in units[k * ri:(k + 1) * ri]:
                for (c, by, bx) in unit:
                    blk = coef[c][by, bx]
                    if ss == 0 and ah == 0:                        # G.1.2.1, first pass
                        t = br.symbol(dct[c])
                        pred[c] += _extend(br.bits(t), t)
                        blk[0] = pred[c] * (1 << al)
                    elif ss == 0:                                  # G.1.2.1, refinement: one bit
                        if br.bit():
                            blk[0] |= 1 << al
                    elif ah == 0:                                  # G.1.2.2 (Figure G.3 inverted)
                        if eobrun:
                            eobrun -= 1
                            continue
                        z = ss
                        while z <= se:
                            rs = br.symbol(act[c])
                            r, s = rs >> 4, rs & 15
                            if s:
                                z += r
                                blk[ZZ[z]] = _extend(br.bits(s), s) * (1 << al)
                                z += 1
                            elif r == 15:
                                z += 16
                            else:
                                eobrun = (1 << r) + br.bits(r) - 1
                                break
                    else:                                          # G.1.2.3 (Figure G.7 inverted)
                        eobrun = _refine_ac(br, act[c], blk, ss, se, al, eobrun)
    return coef


def _refine_ac(br, tab, blk, ss, se, al, eobrun):
    def correct(z):
        if br.bit() and not (int(blk[ZZ[z]]) & (1 << al)):
            blk[ZZ[z]] += (1 << al) if blk[ZZ[z]] > 0 else -(1 << al)

    z = ss
    if eobrun == 0:
        while z <= se:
            rs = br.symbol(tab)
            r, s = rs >> 4, rs & 15
            new = 0
            if s:
                assert s == 1
                new = (1 << al) if br.bit() else -(1 << al)
            elif r < 15:
                eobrun = (1 << r) + br.bits(r)
                break
            while z <= se:                                         # pass r zero-history coefficients; the others take a correction bit
                if blk[ZZ[z]] != 0:
                    correct(z)
                else:
                    if r == 0:
                        break
                    r -= 1
                z += 1
            if new:
                blk[ZZ[z]] = new
            z += 1
    if eobrun:
        while z <= se:
            if blk[ZZ[z]] != 0:
                correct(z)
            z += 1
        eobrun -= 1
    return eobrun


def mcu_order(data, coef):
    """The coefficients as the library lays them out: [block][64], MCU after MCU, luma blocks in raster order inside the MCU, then chroma."""
    frame, _ = walk(data)
    mx, my, geo = _geometry(frame)
    out = []
    for y in range(my):
        for x in range(mx):
            for c, g in enumerate(geo):
                for j in range(g["v"]):
                    for i in range(g["h"]):
                        out.append(coef[c][y * g["v"] + j, x * g["h"] + i])
    return np.array(out, np.int64)


def _upsample_h2v1(c, W):
    w = -(-W // 2)
    c = c[:, :w]
    if w <= 2:
        return np.repeat(c, 2, 1)[:, :W]
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((c.shape[0], 2 * w), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    out[:, 0], out[:, 2 * w - 1] = c[:, 0], c[:, w - 1]
    return out[:, :W]


def decode(data):
    """uint8 [H][W][3]: what Pillow's ``Image.open(file).convert("RGB")`` returns for a complete progressive file"""
    frame, scans = walk(data)
    coef = coefficients(data)
    mx, my, geo = _geometry(frame)
    H, W = frame["height"], frame["width"]
    qts = {}
    for sc in scans:                                               # a component's table is the one in force at its first scan
        for c, q in sc["qts"].items():
            qts.setdefault(c, q)
    planes = []
    for c, g in enumerate(geo):
        b = J.idct(coef[c].reshape(g["ah"], g["aw"], 8, 8), np.array(qts[c], np.int64))
        planes.append(b.swapaxes(1, 2).reshape(g["ah"] * 8, g["aw"] * 8))
    y = planes[0][:H, :W]
    if len(planes) == 1:
        return np.stack([y, y, y], -1).astype(np.uint8)
    h, v = geo[0]["h"], geo[0]["v"]
    if (h, v) == (1, 1):
        cb, cr = planes[1][:H, :W], planes[2][:H, :W]
    elif (h, v) == (2, 1):
        cb, cr = _upsample_h2v1(planes[1][:H], W), _upsample_h2v1(planes[2][:H], W)
    else:
        cb, cr = J._upsample(planes[1], H, W), J._upsample(planes[2], H, W)
    return J.ycc_to_rgb(y, cb, cr)
