"""A JPEG writer from quantised coefficients with every choice of the stream left to the caller, written from T.81: the files that
conform to the standard but that no libjpeg encoder writes -- odd Huffman code shapes, table ids 2 and 3, 16-bit quantisation tables,
0-bit padding, fill bytes and stray bytes before markers, any restart interval, any complete progressive scan script with end-of-band
runs of a chosen length.  It shares nothing with the library; the decoders under test and the tests' Python references read what it
writes, and live Pillow says what the pixels are.

    data = write(W, H, comps, ...)              # comps: [(h, v, blocks)], blocks int [rows][cols][64] in zigzag order (the MCU grid)
    table = chain(symbols) / long_tail(symbols, hot) / flat16(symbols) / single(symbol) / from_length(symbols, 3) / lengths(symbols, [...])
    comps = from_pixels(rgb, qtables, layout) / random_comps(rng, W, H, layout) / extreme(rng, W, H, amplitude)
"""
import numpy as np

import jfif_reference as J
from jpeg_adobe_reference import random_blocks

LAYOUTS = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2), "grey": None}
DC_SYMBOLS = list(range(12))
AC_SYMBOLS = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)]      # EOB, ZRL and every (run, size) of 8-bit samples
EOBRUN_SYMBOLS = [r << 4 for r in range(1, 15)]                                         # progressive AC scans: EOB1 .. EOB14 (EOB0 is EOB)
PROG_AC_SYMBOLS = AC_SYMBOLS + EOBRUN_SYMBOLS                                           # what any progressive AC scan of 8-bit samples can use


# ---- Huffman tables (BITS, HUFFVAL) ----------------------------------------------------------------------------------------------------
def lengths(symbols, lens):
    """the table that gives symbols[i] a code of lens[i] bits (lens ascending).  Checked as libjpeg's jpeg_make_d_derived_tbl checks it:
    the codes of every length fit, and the all-ones code of the longest length stays unused"""
    symbols, lens = list(symbols), list(lens)
    assert len(symbols) == len(lens) <= 256 and lens == sorted(lens) and 1 <= lens[0] and lens[-1] <= 16 and len(set(symbols)) == len(symbols)
    code, prev = 0, lens[0]
    for n in lens:
        code <<= n - prev
        prev = n
        assert code < (1 << n) - 1, "over-subscribed, or the all-ones code is used"
        code += 1
    bits = [lens.count(n) for n in range(1, 17)]
    return bits, symbols


def chain(symbols):
    """code lengths 1, 2, 3, ...: 0, 10, 110, ..."""
    return lengths(symbols, range(1, len(symbols) + 1))


def long_tail(symbols, hot=()):
    """eight short codes (1 .. 8 bits) and every other symbol at 16 bits, the `hot` ones last: up to 255 codes below the unused all-ones"""
    rest = [s for s in symbols if s not in hot] + list(hot)
    return lengths(rest, list(range(1, 9)) + [16] * (len(rest) - 8))


def flat16(symbols):
    return lengths(symbols, [16] * len(symbols))


def single(symbol):
    """one code of one bit: 0"""
    return lengths([symbol], [1])


def from_length(symbols, first=3):
    """no code shorter than `first` bits: 2^first - 1 codes of that length, every further symbol at 16 bits under the last prefix"""
    n = min(len(symbols), (1 << first) - 1)
    return lengths(symbols, [first] * n + [16] * (len(symbols) - n))


def lut_edge(symbols):
    """codes of 8, 9 and 10 bits side by side (and 11, 12 for the many): both sides of the edge of a 9-bit lookup table"""
    many = [2] * 3 + [8] * 30 + [9] * 20 + [10] * 30 + [11] * 40 + [12] * 133
    return lengths(symbols, (many if len(symbols) > 12 else [1, 2, 3, 4, 5, 6, 9, 9, 10, 10, 10, 10])[:len(symbols)])


def spread(symbols):
    """a table for up to 256 symbols with codes of 3, 6, 9 and 12 bits: short and long codes, both sides of a 9-bit lookup table"""
    return lengths(symbols, ([3] * 4 + [6] * 16 + [9] * 60 + [12] * 176)[:len(symbols)])


def codes(table):
    """symbol -> (code, length): T.81 C.2.  A symbol listed twice keeps its first code"""
    bits, vals = table
    out, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            out.setdefault(vals[k], (code, n))
            code += 1
            k += 1
        code <<= 1
    return out


# ---- block sources -----------------------------------------------------------------------------------------------------------------------
def grid(W, H, layout):
    """(hmax, vmax, mcux, mcuy) of a layout's MCU grid"""
    h, v = LAYOUTS[layout] or (1, 1)
    return h, v, -(-W // (8 * h)), -(-H // (8 * v))


def random_comps(rng, W, H, layout, amplitude=250):
    """jpeg_adobe_reference.random_blocks for every component of a layout"""
    h, v, mx, my = grid(W, H, layout)
    comps = [(h, v, random_blocks(rng, my * v, mx * h, amplitude))]
    if layout != "grey":
        comps += [(1, 1, random_blocks(rng, my, mx, amplitude)) for _ in range(2)]
    return comps


def _pad(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def from_pixels(rgb, qtables, layout):
    """real 8-bit samples through jfif_reference.fdct and quantise: rgb uint8 [H][W][3] (grey: [H][W]); qtables: one natural-order table
    per component.  Chroma is sub-sampled by a plain box mean -- a decoder never learns how -- and every plane is edge-padded to whole MCUs"""
    H, W = rgb.shape[:2]
    h, v, mx, my = grid(W, H, layout)
    if layout == "grey":
        planes = [np.asarray(rgb, np.int64).reshape(H, W)]
    else:
        planes = list(J._rgb_to_ycc(rgb))
    comps = []
    for c, p in enumerate(planes):
        ch, cv = (h, v) if c == 0 else (1, 1)
        if c and (h, v) != (1, 1):
            p = _pad(p, -(-H // v) * v, -(-W // h) * h)
            p = (p.reshape(p.shape[0] // v, v, p.shape[1] // h, h).sum((1, 3)) + h * v // 2) // (h * v)
        p = _pad(p, my * cv * 8, mx * ch * 8)
        q = J.quantise(J.fdct(J._blocks(p)), np.asarray(qtables[c], np.int64))
        comps.append((ch, cv, q.reshape(q.shape[0], q.shape[1], 64)[..., J.ZIGZAG]))
    return comps


def extreme(rng, W, H, amplitude=1023):
    """grey blocks with every coefficient drawn from +-amplitude: under a 16-bit quantisation table far outside what samples can give"""
    _, _, mx, my = grid(W, H, "grey")
    return [(1, 1, rng.integers(-amplitude, amplitude + 1, (my, mx, 64)))]


# ---- bits ----------------------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, pad):
        self.acc, self.n, self.out, self.pad = 0, 0, bytearray(), pad

    def put(self, code, length):
        if not length:
            return
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
            k = 8 - self.n
            self.put(((1 << k) - 1) if self.pad else 0, k)
        return bytes(self.out)


def _cat(v):
    return int(abs(int(v))).bit_length()


def _put_value(bits, v, n):
    bits.put(v if v >= 0 else v - 1, n)


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def _dqt(tables, split):
    out, body = b"", b""
    for t, (vals, pq) in enumerate(tables):
        z = [int(vals[J.ZIGZAG[k]]) for k in range(64)]
        one = bytes([pq << 4 | t]) + (b"".join(x.to_bytes(2, "big") for x in z) if pq else bytes(z))
        if split:
            out += _seg(0xDB, one)
        else:
            body += one
    return out if split else _seg(0xDB, body)


def _dht(tables, how):
    """tables: [(class, id, (BITS, HUFFVAL))].  how: "each" one segment per table, "one" a single segment, "twice" every table defined
    first with its symbols reversed and then again as given: the later definition wins"""
    if how == "twice":
        return _dht([(c, i, (b, list(v)[::-1])) for c, i, (b, v) in tables], "one") + _dht(tables, "each")
    parts = [bytes([c << 4 | i]) + bytes(b) + bytes(v) for c, i, (b, v) in tables]
    return b"".join(_seg(0xC4, p) for p in parts) if how == "each" else _seg(0xC4, b"".join(parts))


# ---- one scan's entropy-coded data -----------------------------------------------------------------------------------------------------------
class _Scan:
    """the units of one scan cut into restart intervals; between them `junk`, `fill` fill bytes (plus `shift` before the first) and RSTn"""

    def __init__(self, pad, dri, fill, junk, shift):
        self.pad, self.dri, self.fill, self.junk, self.shift = pad, dri, fill, junk, shift
        self.out, self.bits, self.units, self.rst = bytearray(), _Bits(pad), 0, 0

    def unit(self, reset):
        """call before each unit (an MCU, or a block of a non-interleaved scan); reset(): the coder's state at a restart"""
        if self.dri and self.units and self.units % self.dri == 0:
            reset()
            self.out += self.bits.flush() + self.junk + b"\xff" * (self.fill + (self.shift if self.rst == 0 else 0)) + bytes([0xFF, 0xD0 + self.rst % 8])
            self.bits, self.rst = _Bits(self.pad), self.rst + 1
        self.units += 1

    def end(self, reset):
        reset()
        return bytes(self.out + self.bits.flush() + self.junk + b"\xff" * self.fill)


def _sequential_ac(bits, ac, blk):
    run = 0
    for k in range(1, 64):
        val = int(blk[k])
        if val == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])
            run -= 16
        n = _cat(val)
        bits.put(*ac[run << 4 | n])
        _put_value(bits, val, n)
        run = 0
    if run:
        bits.put(*ac[0x00])


def _units(comps, members, W, H):
    """the scan's units as lists of (component, block row, block column): MCUs of an interleaved scan, else the component's own blocks"""
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    if len(members) > 1:
        mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
        return [[(c, y * comps[c][1] + j, x * comps[c][0] + i) for c in members for j in range(comps[c][1]) for i in range(comps[c][0])]
                for y in range(my) for x in range(mx)]
    c = members[0]
    h, v = (1, 1) if len(comps) == 1 else comps[c][:2]
    bw, bh = -(-(-(-W * h // hmax)) // 8), -(-(-(-H * v // vmax)) // 8)
    return [[(c, y, x)] for y in range(bh) for x in range(bw)]


class _Eob:
    """the pending end-of-band run of a progressive AC scan, with the correction bits that wait behind it (T.81 G.1.2.2, G.1.2.3)"""

    def __init__(self, cap):
        self.run, self.bits, self.cap = 0, [], cap

    def emit(self, out, ac):
        if self.run:
            n = self.run.bit_length() - 1
            out.put(*ac[n << 4])
            out.put(self.run - (1 << n), n)
            self.run = 0
        for b in self.bits:
            out.put(b, 1)
        self.bits = []


def _ac_first(out, ac, blk, ss, se, al, eob):
    run = 0
    for k in range(ss, se + 1):
        val = int(blk[k])
        mag = abs(val) >> al
        if mag == 0:
            run += 1
            continue
        eob.emit(out, ac)
        while run > 15:
            out.put(*ac[0xF0])
            run -= 16
        n = mag.bit_length()
        out.put(*ac[run << 4 | n])
        _put_value(out, mag if val > 0 else -mag, n)
        run = 0
    if run:
        eob.run += 1
        if eob.run == eob.cap:
            eob.emit(out, ac)


def _ac_refine(out, ac, blk, ss, se, al, eob):
    mags = [abs(int(blk[k])) >> al for k in range(64)]
    last = max([k for k in range(ss, se + 1) if mags[k] == 1], default=-1)      # the last newly non-zero coefficient
    run, pending = 0, []
    for k in range(ss, se + 1):
        m = mags[k]
        if m == 0:
            run += 1
            continue
        while run > 15 and k <= last:
            eob.emit(out, ac)
            out.put(*ac[0xF0])
            run -= 16
            for b in pending:
                out.put(b, 1)
            pending = []
        if m > 1:                                      # already non-zero: its next bit waits for the next symbol
            pending.append(m & 1)
            continue
        eob.emit(out, ac)
        out.put(*ac[run << 4 | 1])
        out.put(0 if blk[k] < 0 else 1, 1)
        for b in pending:
            out.put(b, 1)
        pending, run = [], 0
    if run or pending:
        eob.run += 1
        eob.bits += pending
        if eob.run == eob.cap or len(eob.bits) > 937:
            eob.emit(out, ac)


def write(W, H, comps, qtables=None, dqt_split=True, dc_tables=None, ac_tables=None, dht="each", selectors=None, ids=None, sof=0xC0, dri=0,
          pad=1, fill=0, junk=b"", shift=0, script=None, eob_cap=0x7FFF, scan_tables=None, final=None):
    """The file of the quantised blocks `comps` ([(h, v, blocks)], blocks int [rows][cols][64] in zigzag order over the whole MCU grid).
    qtables: [(64 values in natural order, Pq)] for ids 0, 1, ...; default the quality-90 pair, 8-bit.  dqt_split: one DQT segment per table.
    dc_tables / ac_tables: {id: (BITS, HUFFVAL)}; default the Annex K pairs under ids 0 and 1.  dht: "each", "one" or "twice" (see _dht).
    selectors: (Tq, Td, Ta) per component; default (0, 0, 0) for component 0 and (1, 1, 1) for the others.  ids: component ids.
    sof: 0xC0, 0xC1, or 0xC2 with a `script` [(components, Ss, Se, Ah, Al)] of a complete progression.  dri: the restart interval in
    units of each scan (MCUs; blocks in a one-component scan).  pad: the bit that fills a segment's last byte.  junk, fill: `junk` bytes
    and then `fill` 0xFF bytes in front of every RSTn, of every later SOS and of EOI; shift: that many more 0xFF in front of each scan's
    first RSTn (a list: one count per scan), which moves every later byte of the scan.  eob_cap: the length at which an end-of-band run is written out.  scan_tables: {scan index: (dc_tables, ac_tables)}
    defined in front of that scan (a redefinition between scans).  final: (junk, fill) in front of EOI alone, in the place of junk and fill.
    -> bytes"""
    n = len(comps)
    qtables = qtables or [(q, 0) for q in J.quant_tables(90)]
    dc_tables = dc_tables if dc_tables is not None else {0: J.DC_LUMA, 1: J.DC_CHROMA}
    ac_tables = ac_tables if ac_tables is not None else {0: J.AC_LUMA, 1: J.AC_CHROMA}
    selectors = selectors or [(0, 0, 0)] + [(1, 1, 1)] * (n - 1)
    ids = ids or list(range(1, n + 1))
    progressive = sof == 0xC2
    assert progressive == (script is not None) and len(qtables) <= 4
    out = bytearray(b"\xff\xd8") + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00") + _dqt(qtables, dqt_split)
    out += _seg(sof, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([n]) +
                b"".join(bytes([ids[i], comps[i][0] << 4 | comps[i][1], selectors[i][0]]) for i in range(n)))
    out += _dht([(0, i, t) for i, t in sorted(dc_tables.items())] + [(1, i, t) for i, t in sorted(ac_tables.items())], dht)
    if dri:
        out += _seg(0xDD, dri.to_bytes(2, "big"))
    script = script if progressive else [(list(range(n)), 0, 63, 0, 0)]
    blocks = [np.asarray(c[2], np.int64) for c in comps]
    geo = [list(c[:2]) for c in comps]
    for si, (members, ss, se, ah, al) in enumerate(script):
        if scan_tables and si in scan_tables:
            dc_tables, ac_tables = {**dc_tables, **scan_tables[si][0]}, {**ac_tables, **scan_tables[si][1]}
            out += _dht([(0, i, t) for i, t in sorted(scan_tables[si][0].items())] + [(1, i, t) for i, t in sorted(scan_tables[si][1].items())], "each")
        out += _seg(0xDA, bytes([len(members)]) + b"".join(bytes([ids[c], selectors[c][1] << 4 | selectors[c][2]]) for c in members) +
                    bytes([ss, se, ah << 4 | al]))
        dc = {c: codes(dc_tables[selectors[c][1]]) for c in members if ss == 0 and ah == 0}
        ac = {c: codes(ac_tables[selectors[c][2]]) for c in members if se > 0}
        last = si == len(script) - 1
        j, f = final if (final is not None and last) else (junk, fill)
        sc = _Scan(pad, dri, fill, junk, shift[si] if isinstance(shift, (list, tuple)) else shift)
        pred, eob = [0] * n, _Eob(eob_cap)

        def reset():
            for c in members:
                pred[c] = 0
            if ss > 0:
                eob.emit(sc.bits, ac[members[0]])

        for unit in _units(geo, members, W, H):
            sc.unit(reset)
            for c, by, bx in unit:
                blk = blocks[c][by, bx]
                if not progressive:
                    _put_dc(sc.bits, dc[c], int(blk[0]) - pred[c])
                    pred[c] = int(blk[0])
                    _sequential_ac(sc.bits, ac[c], blk)
                elif ss == 0 and ah == 0:
                    v = int(blk[0]) >> al
                    _put_dc(sc.bits, dc[c], v - pred[c])
                    pred[c] = v
                elif ss == 0:
                    sc.bits.put((int(blk[0]) >> al) & 1, 1)
                elif ah == 0:
                    _ac_first(sc.bits, ac[c], blk, ss, se, al, eob)
                else:
                    _ac_refine(sc.bits, ac[c], blk, ss, se, al, eob)
        sc.junk, sc.fill = j, f
        out += sc.end(reset)
    return bytes(out + b"\xff\xd9")


def _put_dc(bits, dc, diff):
    n = _cat(diff)
    bits.put(*dc[n])
    _put_value(bits, diff, n)
