"""A plain Python zlib (RFC 1950) / deflate (RFC 1951) reader -- TEST INFRASTRUCTURE, the reference of the inflate tests.  Written from
the two RFCs, one bit at a time; it shares nothing with csrc/inflate.hip and imports neither the package nor ``zlib``.

    data, status = inflate(stream)
    data, status, trace = inflate_traced(stream)

``status`` is one of the AEJ_INFLATE_* values of include/aej.h.  On an error ``data`` is what had been decoded before it.

The RFCs leave open what a decoder does with a code that is not complete; this reader follows zlib (inflate.c / inftrees.c, checked
against zlib 1.2.11): an over-subscribed code is an error; an incomplete code is an error unless it is a literal / length or distance
code whose longest code has one bit; a distance code without any code is accepted and fails where a distance is needed; a block without
an end-of-block code, more than 286 literal / length or more than 30 distance code lengths are errors; bytes after the Adler-32 are not
looked at.  A stream that ends before a bit that is needed has status TRUNCATED, whatever else may be wrong further on.

``trace`` records what the stream made the reader do, so that a catalogue can assert that it reaches what it was built to reach."""

OK, BAD_HEADER, BAD_BLOCK_TYPE, BAD_CODE_LENGTHS, BAD_SYMBOL, TOO_FAR, STORED_LEN, TRUNCATED, OVER_CAPACITY, ADLER = range(10)

_LEN = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1), (19, 2), (23, 2), (27, 2),
        (31, 2), (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4), (115, 4), (131, 5), (163, 5), (195, 5), (227, 5), (258, 0)]
_DIST = [(1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (7, 1), (9, 2), (13, 2), (17, 3), (25, 3), (33, 4), (49, 4), (65, 5), (97, 5), (129, 6),
         (193, 6), (257, 7), (385, 7), (513, 8), (769, 8), (1025, 9), (1537, 9), (2049, 10), (3073, 10), (4097, 11), (6145, 11),
         (8193, 12), (12289, 12), (16385, 13), (24577, 13)]
_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class Trace:
    """What one stream exercised (see the module text)."""

    def __init__(self):
        self.cinfo = self.flevel = None
        self.blocks = []             # "stored" / "fixed" / "dynamic", in order
        self.len_pairs = set()       # (length code 257 .. 285, extra value)
        self.dist_pairs = set()      # (distance code 0 .. 29, extra value)
        self.lit_lengths = []        # per dynamic block: the literal / length code lengths, by symbol
        self.dist_lengths = []       # per dynamic block: the distance code lengths, by symbol
        self.cl_lengths = []         # per dynamic block: (HCLEN, the 19 code-length code lengths by symbol)
        self.repeats = []            # (symbol 16 / 17 / 18, count, index of the first length written, HLIT, previous code-length symbol)
        self.stored = []             # (LEN, bit offset 0 .. 7 of the block header's first bit, input byte offset of the first data byte,
        #                               output position)
        self.matches = []            # (distance, length, output position of its first byte)
        self.lit_code_bits = set()   # lengths of the literal / length codes actually read
        self.dist_code_bits = set()  # lengths of the distance codes actually read
        self.lit_counts = [0] * 286  # how often each literal / length symbol was read (256: once per coded block)
        self.dist_counts = [0] * 30  # how often each distance symbol was read

    def crossing(self):
        """the repeat symbols with a run that starts among the literal lengths and ends among the distance lengths"""
        return {s for s, count, at, hlit, _ in self.repeats if at < hlit < at + count}


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _In:
    def __init__(self, data):
        self.data, self.at, self.end = bytes(data), 0, 8 * len(data)

    def bit(self):
        if self.at >= self.end:
            raise _Stop(TRUNCATED)
        v = (self.data[self.at >> 3] >> (self.at & 7)) & 1
        self.at += 1
        return v

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= self.bit() << i
        return v


class _Code:
    """a canonical Huffman code (RFC 1951 3.2.2) as a map (number of bits, code value) -> symbol"""

    def __init__(self, lengths, may_be_partial):
        self.map = {}
        self.longest = max(lengths) if lengths else 0
        if self.longest == 0:
            if not may_be_partial:
                raise _Stop(BAD_CODE_LENGTHS)
            return
        space = 1 << self.longest                     # Kraft: every code of l bits takes 2^(longest - l) of it
        used = sum(1 << (self.longest - l) for l in lengths if l)
        if used > space:
            raise _Stop(BAD_CODE_LENGTHS)
        if used < space and not (may_be_partial and self.longest == 1):
            raise _Stop(BAD_CODE_LENGTHS)
        code = 0
        for n in range(1, self.longest + 1):
            for s, l in enumerate(lengths):
                if l == n:
                    self.map[(n, code)] = s
                    code += 1
            code <<= 1

    def read(self, src):
        """-> (symbol, bits read), or (None, 0) as soon as the bits read so far cannot begin any code"""
        if not self.map:
            src.bit()                                  # zlib's table holds one-bit entries that say "invalid": a bit is needed to hit one
            return None, 0
        code = 0
        for n in range(1, self.longest + 1):
            code = (code << 1) | src.bit()
            s = self.map.get((n, code))
            if s is not None:
                return s, n
        return None, 0


_FIXED_LIT = _Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False)
_FIXED_DIST = _Code([5] * 32, False)


def _adler(data):
    a, b = 1, 0
    for i in range(0, len(data), 3800):               # 3800 * 255 * 3800 / 2 stays far below 2^63; Python's ints do not care anyway
        for c in data[i:i + 3800]:
            a += c
            b += a
        a %= 65521
        b %= 65521
    return (b << 16) | a


def _dynamic_codes(src, tr):
    hlit, hdist, hclen = src.bits(5) + 257, src.bits(5) + 1, src.bits(4) + 4
    if hlit > 286 or hdist > 30:
        raise _Stop(BAD_CODE_LENGTHS)
    cl = [0] * 19
    for k in range(hclen):
        cl[_ORDER[k]] = src.bits(3)
    tr.cl_lengths.append((hclen, cl))
    clc = _Code(cl, False)
    lengths, last = [], None
    while len(lengths) < hlit + hdist:
        s, _ = clc.read(src)
        if s is None:
            raise _Stop(BAD_CODE_LENGTHS)
        if s < 16:
            lengths.append(s)
        else:
            if s == 16:
                if not lengths:
                    raise _Stop(BAD_CODE_LENGTHS)
                value, count = lengths[-1], 3 + src.bits(2)
            elif s == 17:
                value, count = 0, 3 + src.bits(3)
            else:
                value, count = 0, 11 + src.bits(7)
            if len(lengths) + count > hlit + hdist:
                raise _Stop(BAD_CODE_LENGTHS)
            tr.repeats.append((s, count, len(lengths), hlit, last))
            lengths += [value] * count
        last = s
    if lengths[256] == 0:
        raise _Stop(BAD_CODE_LENGTHS)
    tr.lit_lengths.append(lengths[:hlit])
    tr.dist_lengths.append(lengths[hlit:])
    return _Code(lengths[:hlit], True), _Code(lengths[hlit:], True)


def _run(src, out, tr):
    if len(src.data) < 2:
        raise _Stop(TRUNCATED)
    cmf, flg = src.bits(8), src.bits(8)
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf * 256 + flg) % 31 or flg & 0x20:
        raise _Stop(BAD_HEADER)
    tr.cinfo, tr.flevel = cmf >> 4, flg >> 6
    final = 0
    while not final:
        header_at = src.at
        final, kind = src.bit(), src.bits(2)
        if kind == 3:
            raise _Stop(BAD_BLOCK_TYPE)
        if kind == 0:
            src.bits(-src.at % 8)
            n, check = src.bits(16), src.bits(16)
            if n ^ check != 0xFFFF:
                raise _Stop(STORED_LEN)
            first = src.at >> 3
            if first + n > len(src.data):
                raise _Stop(TRUNCATED)
            tr.blocks.append("stored")
            tr.stored.append((n, header_at & 7, first, len(out)))
            out += src.data[first:first + n]
            src.at += 8 * n
            continue
        if kind == 1:
            tr.blocks.append("fixed")
            lit, dist = _FIXED_LIT, _FIXED_DIST
        else:
            lit, dist = _dynamic_codes(src, tr)
            tr.blocks.append("dynamic")
        while True:
            s, n = lit.read(src)
            if s is None or s > 285:
                raise _Stop(BAD_SYMBOL)
            tr.lit_code_bits.add(n)
            tr.lit_counts[s] += 1
            if s < 256:
                out.append(s)
                continue
            if s == 256:
                break
            base, extra = _LEN[s - 257]
            e = src.bits(extra)
            length = base + e
            d, n = dist.read(src)
            if d is None or d > 29:
                raise _Stop(BAD_SYMBOL)
            tr.dist_code_bits.add(n)
            tr.dist_counts[d] += 1
            base, extra = _DIST[d]
            f = src.bits(extra)
            distance = base + f
            if distance > len(out):
                raise _Stop(TOO_FAR)
            tr.len_pairs.add((s, e))
            tr.dist_pairs.add((d, f))
            tr.matches.append((distance, length, len(out)))
            if distance >= length:
                out += out[len(out) - distance:len(out) - distance + length]
            else:
                for _ in range(length):
                    out.append(out[-distance])
    src.bits(-src.at % 8)
    want = 0
    for _ in range(4):
        want = (want << 8) | src.bits(8)
    if want != _adler(out):
        raise _Stop(ADLER)


def inflate_traced(stream):
    src, out, tr = _In(stream), bytearray(), Trace()
    try:
        _run(src, out, tr)
        status = OK
    except _Stop as stop:
        status = stop.status
    return bytes(out), status, tr


def inflate(stream):
    return inflate_traced(stream)[:2]
