"""A plain Python / numpy restatement of the progressive file Pillow writes with ``save(..., "JPEG", quality=q, subsampling=s,
progressive=True)``: libjpeg's ten-scan simple progression, the Annex G entropy coder with its end-of-band runs and deferred
correction bits written as the serial state machine it is, one optimal Huffman table per scan.  The quantised coefficients come from
tests/jfif_options_reference.py.  ``encode`` returns the .jpg bytes and, per scan, how many end-of-band runs were cut because the run
reached 0x7FFF blocks and how many because more than 937 correction bits were pending.  tests/test_jfif_progressive_host.py pins it to
Pillow; the library's host core and kernels (csrc/jfif_prog_core.h, csrc/jfifprog.hip) are compared against it.
"""
import numpy as np

import jfif_options_reference as O
import jfif_reference as R

# (components, Ss, Se, Ah, Al): component 0 Y, 1 Cb, 2 Cr; the chroma scans come Cr first
SCRIPT = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
          ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
MAX_EOBRUN = 0x7FFF
MAX_DEFERRED = 937                     # MAX_CORR_BITS - DCTSIZE2 + 1


class Scan:
    """the events of one scan: ("s", table, symbol) and ("b", value, count)"""

    def __init__(self):
        self.ev, self.eobrun, self.be, self.cuts_run, self.cuts_bits = [], 0, [], 0, 0

    def sym(self, table, s):
        self.ev.append(("s", table, s))

    def bits(self, v, n):
        if n:
            self.ev.append(("b", v & ((1 << n) - 1), n))

    def flush(self, table):
        if self.eobrun:
            n = self.eobrun.bit_length() - 1
            self.sym(table, n << 4)
            self.bits(self.eobrun, n)
            for b in self.be:
                self.bits(b, 1)
            self.eobrun, self.be = 0, []


def dc_first(sc, blocks, al):
    pred = [0, 0, 0]
    for comp, blk in blocks:
        v = int(blk[0]) >> al
        diff, pred[comp] = v - pred[comp], v
        n = R._category(diff)
        sc.sym(1 if comp else 0, n)
        sc.bits(diff if diff >= 0 else diff - 1, n)


def dc_refine(sc, blocks, al):
    for _, blk in blocks:
        sc.bits(int(blk[0]) >> al, 1)


def ac_first(sc, table, blocks, ss, se, al):
    for blk in blocks:
        r = 0
        if np.any(blk[ss:se + 1]):
            for k in range(ss, se + 1):
                v = int(blk[k])
                t = abs(v) >> al
                if t == 0:
                    r += 1
                    continue
                sc.flush(table)
                while r > 15:
                    sc.sym(table, 0xF0)
                    r -= 16
                n = t.bit_length()
                sc.sym(table, (r << 4) | n)
                sc.bits(t if v >= 0 else ~t, n)
                r = 0
        else:
            r = se - ss + 1
        if r > 0:
            sc.eobrun += 1
            if sc.eobrun == MAX_EOBRUN:
                sc.flush(table)
                sc.cuts_run += 1


def ac_refine(sc, table, blocks, ss, se, al):
    for blk in blocks:
        r, br = 0, []
        if np.any(blk[ss:se + 1]):
            a = [abs(int(v)) >> al for v in blk]
            eob = max([k for k in range(ss, se + 1) if a[k] == 1], default=-1)
            for k in range(ss, se + 1):
                if a[k] == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    sc.flush(table)
                    sc.sym(table, 0xF0)
                    r -= 16
                    for b in br:
                        sc.bits(b, 1)
                    br = []
                if a[k] > 1:
                    br.append(a[k] & 1)
                    continue
                sc.flush(table)
                sc.sym(table, (r << 4) | 1)
                sc.bits(0 if blk[k] < 0 else 1, 1)
                for b in br:
                    sc.bits(b, 1)
                br, r = [], 0
        else:
            r = se - ss + 1
        if r > 0 or br:
            sc.eobrun += 1
            sc.be += br
            if sc.eobrun == MAX_EOBRUN or len(sc.be) > MAX_DEFERRED:
                sc.cuts_run += sc.eobrun == MAX_EOBRUN
                sc.cuts_bits += sc.eobrun != MAX_EOBRUN
                sc.flush(table)


def scan_events(blocks, ss, se, ah, al, table=0):
    """the events of one scan.  blocks: [(component, [64] zigzag)] for a DC scan, a list of [64] zigzag arrays for an AC scan"""
    sc = Scan()
    if ss == 0:
        (dc_refine if ah else dc_first)(sc, blocks, al)
    else:
        (ac_refine if ah else ac_first)(sc, table, blocks, ss, se, al)
        sc.flush(table)
    return sc


def histogram(sc, n_tables=2):
    h = np.zeros((n_tables, 257), np.int64)
    for e in sc.ev:
        if e[0] == "s":
            h[e[1], e[2]] += 1
    return h


def scan_bytes(sc, tabs):
    """the events under the (BITS, HUFFVAL) tables tabs[table] -> padded, stuffed bytes"""
    codes = [R.huff_codes(t) if t is not None else None for t in tabs]
    bits = R._Bits()
    for e in sc.ev:
        if e[0] == "s":
            bits.put(*codes[e[1]][e[2]])
        else:
            bits.put(e[1], e[2])
    return bits.flush()


def encode_scan(blocks, ss, se, ah, al):
    """one single-table scan over given coefficients -> (bytes, counts [257], (cuts by 0x7FFF, cuts by the 937-bit rule))"""
    sc = scan_events([(0, b) for b in blocks] if ss == 0 else blocks, ss, se, ah, al)
    h = histogram(sc, 1)[0]
    tab = O.optimal_table(h) if h.any() else None
    return scan_bytes(sc, [tab]), h, (sc.cuts_run, sc.cuts_bits)


def component_blocks(rgb, q, subsampling):
    """-> (MCU-order [(component, blk)], {component: its own ceil(w_c/8) x ceil(h_c/8) blocks in raster order})"""
    hs, vs = O.FACTORS[subsampling]
    H, W = rgb.shape[:2]
    mcu = O.coefficients(rgb, q, subsampling)
    by, bx = -(-H // 8), -(-W // 8)
    my, mx = -(-H // (8 * vs)), -(-W // (8 * hs))
    per = hs * vs + 2
    luma = {}
    comps = {1: [], 2: []}
    for m in range(my * mx):
        for k in range(hs * vs):
            yy, xx = vs * (m // mx) + k // hs, hs * (m % mx) + k % hs
            if yy < by and xx < bx:
                luma[yy * bx + xx] = mcu[m * per + k][1]
        comps[1].append(mcu[m * per + hs * vs][1])
        comps[2].append(mcu[m * per + hs * vs + 1][1])
    comps[0] = [luma[i] for i in range(by * bx)]
    return mcu, comps


def headers(q, H, W, subsampling):
    """SOI .. SOF2"""
    h = O.headers(q, H, W, subsampling)
    i = h.index(b"\xff\xc0")
    return h[:i] + b"\xff\xc2" + h[i + 2:i + 19]


def encode(rgb, q, subsampling=2):
    """uint8 [H, W, 3] -> (the bytes of PIL.Image.fromarray(rgb).save(buf, "JPEG", quality=q, subsampling=subsampling,
    progressive=True), [(cuts by 0x7FFF, cuts by the 937-bit rule) per scan])"""
    H, W = rgb.shape[:2]
    mcu, comps = component_blocks(rgb, q, subsampling)
    out, cuts = headers(q, H, W, subsampling), []
    for cs, ss, se, ah, al in SCRIPT:
        if ss == 0:
            sc = scan_events(mcu, 0, 0, ah, al)
            tabs = [None, None]
            if ah == 0:
                tabs = [O.optimal_table(h) for h in histogram(sc)]
                for i, t in enumerate(tabs):
                    out += R._seg(0xC4, bytes([i]) + bytes(t[0]) + bytes(t[1]))
            td = 0 if ah else 0x10                               # libjpeg zeroes the selector of a table the scan does not use
            out += R._seg(0xDA, bytes([3, 1, 0x00, 2, td, 3, td, 0, 0, ah << 4 | al]))
        else:
            t = 1 if cs[0] else 0
            sc = scan_events(comps[cs[0]], ss, se, ah, al, t)
            tabs = [None, None]
            tabs[t] = O.optimal_table(histogram(sc)[t])
            out += R._seg(0xC4, bytes([0x10 | t]) + bytes(tabs[t][0]) + bytes(tabs[t][1]))
            out += R._seg(0xDA, bytes([1, cs[0] + 1, t, ss, se, ah << 4 | al]))
        out += scan_bytes(sc, tabs)
        cuts.append((sc.cuts_run, sc.cuts_bits))
    return out + b"\xff\xd9", cuts


def synthetic_cases():
    """(name, int16 [n][64] zigzag coefficients, Ss, Se, Ah, Al, expected (cuts by 0x7FFF, cuts by the 937-bit rule) or None): the
    corners of the coder that pixels do not reach, for the library's host core and kernels"""
    g = np.random.default_rng(2024)
    out = []

    def blocks(n):
        return np.zeros((n, 64), np.int16)

    c = blocks(6)                                                # ZRL against the end of band in a refinement scan
    c[0, 1], c[0, 40] = 1, 2                                     # 38 zeros before a coefficient past the last new one: no ZRL, folded into EOB
    c[1, 1], c[1, 30], c[1, 63] = 3, 1, -2                       # 28 zeros before a new one: ZRL takes the buffered bit
    c[2, 2], c[2, 20], c[2, 40], c[2, 60] = -5, 2, -1, 7         # ZRL twice with bits buffered between
    c[3, 63] = 1                                                 # three ZRL, then the last coefficient
    c[4, 17], c[4, 18] = 6, -1
    c[5, 1:64] = 1
    out.append(("zrl_eob_refine", c, 1, 63, 1, 0, (0, 0)))
    out.append(("zrl_first", c, 1, 63, 0, 0, (0, 0)))
    for total in (937, 938, 939):                                # deferred bits: 14 blocks of 63, then one that lands on the sum
        c = blocks(20)
        c[0, 1] = 1                                              # opens the chain with nothing deferred
        c[1:15, 1:64] = 2
        c[15, 1:total - 882 + 1] = 3
        c[16, 5] = 2                                             # one more bit: over the limit when the sum stood at 937
        c[18, 9] = -1
        out.append((f"deferred_{total}", c, 1, 63, 1, 0, (0, 1)))
    for n in (0x7FFE, 0x7FFF, 0x8000, 0x8001):
        c = blocks(n + 2)
        c[0, 3], c[n + 1, 7] = 1, -1                             # block 0 emits and joins: a chain of n + 1 blocks
        out.append((f"chain_{n + 1:#x}_refine", c, 1, 63, 1, 0, (1 if n + 1 >= 0x7FFF else 0, 0)))
        out.append((f"chain_{n + 1:#x}_first", c, 1, 63, 0, 0, (1 if n + 1 >= 0x7FFF else 0, 0)))
    for n in (0x7FFF, 0x8000):
        out.append((f"zero_{n:#x}", blocks(n), 1, 63, 1, 0, (1, 0)))
    out.append(("all_zero_first", blocks(7), 6, 63, 0, 2, (0, 0)))
    out.append(("all_zero_refine", blocks(1), 1, 63, 2, 1, (0, 0)))
    c = blocks(5)
    c[1, 10], c[1, 33], c[3, 63] = 2, -3, 6                      # blocks whose only content is correction bits
    out.append(("only_correction_bits", c, 1, 63, 1, 0, (0, 0)))
    c = blocks(40)
    c[:, 1:64] = g.integers(2, 200, (40, 63)) * g.choice([-1, 1], (40, 63))      # nothing new anywhere: cuts every 15 blocks
    out.append(("dense_correction", c, 1, 63, 1, 0, (0, 2)))
    dc = blocks(300)
    dc[:, 0] = g.integers(-1024, 1025, 300)
    out.append(("dc_first", dc, 0, 0, 0, 1, (0, 0)))
    out.append(("dc_refine", dc, 0, 0, 1, 0, (0, 0)))
    for k, dens in enumerate((0.02, 0.2, 0.7)):
        c = (g.integers(-40, 41, (700, 64)) * (g.random((700, 64)) < dens)).astype(np.int16)
        c[200:400] = np.clip(c[200:400], -3, 3)
        for ss, se, ah, al in ((1, 5, 0, 2), (6, 63, 0, 2), (1, 63, 0, 1), (1, 63, 2, 1), (1, 63, 1, 0)):
            out.append((f"random_{k}_{ss}_{se}_{ah}_{al}", c, ss, se, ah, al, None))
    return out
