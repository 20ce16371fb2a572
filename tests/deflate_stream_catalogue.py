"""The catalogue of conforming zlib streams that zlib never writes, and of malformed ones, shared by tests/test_inflate_streams_host.py
(every case against ``zlib.decompress`` and tests/inflate_reference.py, and the coverage the catalogue claims, asserted from the
reference's trace) and tests/test_gpu_inflate_streams.py (csrc/inflate.hip).  Every stream is built at run time from seeds by
tests/deflate_stream_writer.py; nothing here reads the library or calls ``zlib``.

    for case in catalogue(): case.name ("group/case"), case.data, case.payload
    for bad in malformed():  bad.name, bad.data, bad.status
    restream(payload, style) -> a stream of `payload` in one of STYLES (what the PNG and .ajpg tests wrap)

Two things the RFC rules out and the catalogue therefore holds in another form.  (1) A valid dynamic block has HCLEN >= 5: the first
four code-length symbols in transmission order are 16, 17, 18 and 0, which can only spell lengths of zero, and a block without an
end-of-block code is invalid.  ``clcode/hclen5`` is the least valid header, ``hclen4_all_zero`` is among the malformed.  (2) No valid
zlib stream is shorter than 8 bytes (2 header, 10 bits of an empty fixed block, 4 trailer): ``input/bytes8`` .. ``bytes16`` are the
whole streams, lengths 6 and 7 occur among the prefixes of PREFIX_CASES (status TRUNCATED)."""
import functools
from collections import namedtuple

import numpy as np

import deflate_stream_writer as W
from deflate_reference import huffman_lengths
from deflate_stream_writer import bits, dynamic, fixed, lit, match, match_value, stored, sym

Case = namedtuple("Case", "name data payload")
Bad = namedtuple("Bad", "name data status")
MAX_STREAM_OUT = 256 << 10
MAX_TOTAL_OUT = 8 << 20
OVERLAP_DISTANCES = tuple(range(1, 66)) + (127, 128)
OVERLAP_LENGTHS = (3, 63, 64, 65, 128, 129, 258)
STORED_LENS = (0, 1, 63, 64, 65, 255, 256, 257, 65535)
OUTPUT_SIZES = (0, 1, 255, 256, 257, 511, 512, 32767, 32768, 32769, 65537)
MATCH_STARTS = (255, 256, 257, 32767, 32768, 32769, 65535, 65536, 65537)
PREFIX_CASES = ("prefix/stored", "prefix/fixed", "prefix/dynamic", "prefix/dynamic_long")      # every strict prefix of these is run


def _rng(*key):
    return np.random.default_rng([ord(c) for c in "/".join(str(k) for k in key)])


def noise(r, n):
    return r.integers(0, 256, n, dtype=np.uint8).tobytes()


def lits(data):
    return [lit(b) for b in data]


def stored_run(data):
    """`data` as stored blocks of at most 65535 bytes, none final"""
    return [stored(data[i:i + 65535], final=False) for i in range(0, len(data), 65535)]


def random_tokens(r, n_out, pos=0, window=32768, p_match=0.5):
    """tokens that expand to exactly n_out bytes when the output stands at `pos`: runs of 1 .. 8 random literals and matches of any
    length at any distance inside min(pos, window)"""
    out, left = [], n_out
    while left:
        if pos and left >= 3 and r.random() < p_match:
            length = int(min(left, r.integers(3, 259)))
            out.append(match_value(length, int(r.integers(1, min(pos, window) + 1))))
        else:
            length = int(min(left, r.integers(1, 9)))
            out += lits(noise(r, length))
        pos += length
        left -= length
    return out


# ---- code lengths and their spelling ----------------------------------------------------------------------------------------------------
def rle(lengths):
    """the code-length symbols an ordinary encoder would write for `lengths`: 18 / 17 for runs of zeros, 16 for repeats"""
    out, i, seq = [], 0, list(lengths)
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, k - 11)); run -= k
            if run >= 3:
                out.append((17, run - 3)); run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, k - 3)); run -= k
            out += [(v, 0)] * run
    return out


class Spell:
    """code lengths written down symbol by symbol: the lengths and the code-length symbols that spell them grow together"""

    def __init__(self):
        self.lengths, self.symbols = [], []

    def v(self, length, n=1):
        self.lengths += [length] * n
        self.symbols += [(length, 0)] * n
        return self

    def r16(self, n):
        self.lengths += [self.lengths[-1]] * n
        self.symbols.append((16, n - 3))
        return self

    def r17(self, n):
        self.lengths += [0] * n
        self.symbols.append((17, n - 3))
        return self

    def r18(self, n):
        self.lengths += [0] * n
        self.symbols.append((18, n - 11))
        return self

    def block(self, tokens, hlit, **kw):
        assert W.kraft(self.lengths[:hlit]) == 1 << 15 or max(self.lengths[:hlit]) == 1, "literal code not complete"
        return dynamic(tokens, self.lengths[:hlit], self.lengths[hlit:], cl_symbols=self.symbols, **kw)


def _hist(tokens):
    """how often the tokens use each literal / length symbol (end-of-block once) and each distance symbol"""
    ll, dd = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if t[0] != "bits":
            ll[t[1]] += 1
        if t[0] == "match":
            dd[t[3]] += 1
    return ll, dd


def lengths_of(tokens, hlit=None, hdist=None):
    """Huffman code lengths for what `tokens` use (and end-of-block), trimmed to the last used symbol unless hlit / hdist say otherwise"""
    ll, dd = _hist(tokens)
    ll, dd = huffman_lengths(ll, 15), huffman_lengths(dd, 15)
    hlit = hlit or max(257, max(s + 1 for s in range(286) if ll[s]))
    hdist = hdist or max([1] + [s + 1 for s in range(30) if dd[s]])
    return ll[:hlit], dd[:hdist]


def dyn(tokens, hlit=None, hdist=None, **kw):
    """a dynamic block with Huffman lengths for its own tokens and an ordinary header"""
    ll, dd = lengths_of(tokens, hlit, hdist)
    return dynamic(tokens, ll, dd, cl_symbols=rle(ll + dd), **kw)


def place(pairs, n):
    """n code lengths, zero but for the (symbol, length) pairs"""
    out = [0] * n
    for s, l in pairs:
        out[s] = l
    return out


SLOW_SHAPE = [11] + [12] * 2 + [13] * 4 + [14] * 4 + [15] * 8           # 19 codes that fill 2^-9 exactly
DIST30 = [4] * 15 + list(range(5, 13)) + [14] + [15] * 6                # a complete 30-symbol code with 15-bit members


def slow_lit_lengths(symbols):
    """a complete literal code whose 19 used `symbols` (end-of-block among them) have 11 .. 15 bits; the codes of 1 .. 9 bits go to
    literals 0 .. 8, which nothing uses"""
    assert len(symbols) == 19 and 256 in symbols and min(symbols) > 8
    return place([(s, s + 1) for s in range(9)] + list(zip(sorted(symbols), SLOW_SHAPE)), max(257, max(symbols) + 1))


def tail_lengths(counts, ladder=6):
    """code lengths for the used symbols of `counts` with a long tail: the `ladder` most frequent symbols get 1, 2, .. bits and the rest
    shares the last 2^-ladder evenly, so that with more than 2^(14 - ladder) symbols the tail has 15-bit codes"""
    used = sorted((s for s, c in enumerate(counts) if c), key=lambda s: -counts[s])
    out = [0] * len(counts)
    assert len(used) >= ladder + 2
    for k in range(ladder):
        out[used[k]] = k + 1
    rest = used[ladder:]
    for s, l in zip(rest, W.balanced_lengths(len(rest), 15 - ladder)):
        out[s] = ladder + l
    return out


# ---- a parse for the streams that carry a given payload -------------------------------------------------------------------------------
def lz_parse(data, window=32768, chain=12, only_distance=None, overlap_first=False):
    """A greedy LZ77 parse -> [("lit", b) | ("copy", length, distance)].  only_distance: matches at that distance alone;
    overlap_first: a match at a distance of at most 65 that is longer than its distance wins over a longer plain one."""
    data = bytes(data)
    out, p, n, seen = [], 0, len(data), {}

    def run(q):
        k = 0
        while p + k < n and k < 258 and data[q + k] == data[p + k]:
            k += 1
        return k

    def note(i):
        if i + 3 <= n:
            seen.setdefault(data[i:i + 3], []).append(i)

    while p < n:
        best = (0, 0)
        if only_distance is not None:
            if p >= only_distance:
                best = (run(p - only_distance), only_distance)
        else:
            if overlap_first:
                for d in range(1, min(p, 65) + 1):
                    k = run(p - d)
                    if k > d and k > best[0]:
                        best = (k, d)
            if best[0] < 3:
                for q in reversed(seen.get(data[p:p + 3], [])[-chain:]):
                    if p - q <= window:
                        k = run(q)
                        if k > best[0]:
                            best = (k, p - q)
        if best[0] >= 3:
            out.append(("copy",) + best)
            for i in range(p, p + best[0]):
                note(i)
            p += best[0]
        else:
            out.append(("lit", data[p]))
            note(p)
            p += 1
    return out


def _tokens(parse, alt258=False):
    out = []
    for t in parse:
        if t[0] == "lit":
            out.append(lit(t[1]))
        else:
            m = match_value(t[1], t[2])
            out.append(match(284, 31, m[3], m[4]) if alt258 and t[1] == 258 else m)
    return out


def _style_stored(p):
    return [stored(p[i:i + 65535]) for i in range(0, len(p), 65535)] or [stored(b"")]


def _style_stored_chunks(p):
    sizes, out, i, k = (1, 63, 64, 65, 0, 255, 256, 257, 3), [], 0, 0
    while i < len(p):
        out.append(stored(p[i:i + sizes[k % len(sizes)]]))
        i += sizes[k % len(sizes)]
        k += 1
    return out or [stored(b"")]


def _style_one_code_distance(p):
    t = _tokens(lz_parse(p, only_distance=1))
    ll, _ = lengths_of(t)
    return [dynamic(t, ll, [1], cl_symbols=rle(ll + [1]))]


def _style_literal_only(p):
    t = lits(p)
    ll, _ = lengths_of(t)
    return [dynamic(t, ll, [0], cl_symbols=rle(ll + [0]))]


def _style_long_literal_codes(p):
    t = _tokens(lz_parse(p))
    ll, dd = _hist(t)
    for s in range(286):                                  # every symbol gets a code, so that the tail is long whatever the payload holds
        ll[s] = ll[s] * 300 + 1
    ll, dd = tail_lengths(ll), huffman_lengths([c + 1 for c in dd], 15)
    return [dynamic(t, ll, dd, cl_symbols=rle(ll + dd))]


def _style_long_distance_codes(p):
    t = _tokens(lz_parse(p))
    ll, dd = _hist(t)
    order = sorted(range(30), key=lambda s: -dd[s])
    dl = place(zip(order, sorted(DIST30, reverse=True)), 30)      # the longest codes for the most frequent: they are sure to be read
    ll = huffman_lengths(ll, 15)
    return [dynamic(t, ll, dl, cl_symbols=W.plain_cl_symbols(ll + dl))]


def _style_block_mix(p):
    """a new block every few tokens, stored / fixed / dynamic in turn; matches reach back into earlier blocks"""
    t, out, i, k = lz_parse(p), [], 0, 0
    while i < len(t):
        part = t[i:i + 5 + k % 7]
        if k % 3 == 0:
            j = 0
            while j < len(part) and part[j][0] == "lit":
                j += 1
            out.append(stored(bytes(x[1] for x in part[:j])))
            if j < len(part):
                out.append(fixed(_tokens(part[j:])))
        elif k % 3 == 1:
            out.append(fixed(_tokens(part)))
        else:
            out.append(dyn(_tokens(part)))
        i += 5 + k % 7
        k += 1
    return out or [fixed([])]


def _style_overlap(p):
    return [fixed(_tokens(lz_parse(p, overlap_first=True)))]


def _style_alt258(p):
    t = _tokens(lz_parse(p), alt258=True)
    return [dyn(t, hlit=286)]


def _style_cl_repeats(p):
    """HLIT 286 and HDIST 30 with the unused symbols at zero, so that the header is full of 16 / 17 / 18; the code-length code has 7-bit
    members"""
    t = _tokens(lz_parse(p))
    ll, dd = lengths_of(t, 286, 30)
    cs = rle(ll + dd)
    used = sorted({s for s, _ in cs}, key=lambda s: -sum(1 for x, _ in cs if x == s))
    while len(used) < 8:
        used.append(next(s for s in range(19) if s not in used))
    j = max(j for j in range(1, 6) if 2 <= len(used) - j <= 1 << (7 - j))      # a ladder of j codes, the rest shares 2^-j
    cl = place(zip(used, list(range(1, j + 1)) + [j + l for l in W.balanced_lengths(len(used) - j, 7 - j)]), 19)
    return [dynamic(t, ll, dd, cl_symbols=cs, cl_lengths=cl)]


def _style_small_window(p):
    return [dyn(_tokens(lz_parse(p, window=256)))]


STYLES = {"stored": _style_stored, "stored_chunks": _style_stored_chunks, "fixed": lambda p: [fixed(_tokens(lz_parse(p)))],
          "one_code_distance": _style_one_code_distance, "literal_only": _style_literal_only,
          "long_literal_codes": _style_long_literal_codes, "long_distance_codes": _style_long_distance_codes,
          "block_mix": _style_block_mix, "overlap": _style_overlap, "alt258": _style_alt258, "cl_repeats": _style_cl_repeats,
          "small_window": _style_small_window}


def restream(payload, style):
    """a zlib stream of `payload` written in `style` (a key of STYLES)"""
    payload = bytes(payload)
    data, got = W.write(STYLES[style](payload), cinfo=0 if style == "small_window" else 7)
    assert got == payload, style
    return data


def scanline_like(r, rows=24, row_bytes=96):
    """what the filtered scanlines of a small picture look like: a small filter byte, then periodic stretches of every period up to the
    row, noise, ramps, and rows of zeros long enough for matches of 258"""
    out = bytearray()
    for y in range(rows):
        out.append(y % 5)
        if y % 4 == 3:
            out += bytes(row_bytes)
        elif y % 4 == 2:
            out += noise(r, row_bytes)
        else:
            unit = noise(r, 1 + (7 * y) % 66)
            out += (unit * (row_bytes // len(unit) + 1))[:row_bytes]
    return bytes(out) + bytes(600)


# ---- the valid streams ----------------------------------------------------------------------------------------------------------------
def _header(add):
    for cinfo in range(8):
        for flevel in range(4):
            r = _rng("header", cinfo, flevel)
            window = 256 << cinfo
            t = random_tokens(r, window, window=window) + [match_value(258, window)] + random_tokens(r, 40, pos=window + 258, window=window)
            add(f"header/cinfo{cinfo}_flevel{flevel}", [fixed(t) if flevel % 2 else dyn(t)], cinfo=cinfo, flevel=flevel)


def _stored(add):
    for n in STORED_LENS:
        add(f"stored/len{n}", [stored(noise(_rng("stored", n), n))])
    for b in range(8):                                    # 3 + 9 b + 8 + 7 bits of a fixed block: the stored header starts at (2 + b) & 7
        add(f"stored/after_fixed_{b}", [fixed([lit(200 + b)] * b + [lit(65)], final=False), stored(noise(_rng("after", b), 70 + b))])
    add("stored/empty_x300", [fixed(lits(b"ab"), final=False)] + [stored(b"")] * 300)
    r = _rng("across")
    add("stored/across_32768", [stored(noise(r, 32000), final=False), stored(noise(r, 1000), final=False),
                                fixed([match_value(258, 32768), lit(7), match_value(130, 32768)])])
    for k in range(4):                                    # the first data byte sits at input offset 7 + 5 k
        add(f"stored/in_pos_{k}", [stored(b"")] * k + [stored(noise(_rng("inpos", k), 67 + k))])


def _blocks(add):
    eob_only = lambda **kw: dynamic([], [0] * 256 + [1], [0], **kw)      # noqa: E731
    add("blocks/empty_fixed_final", [fixed(lits(b"xy"), final=False), fixed([])])
    add("blocks/empty_fixed_first", [fixed([], final=False), fixed([], final=False), fixed(lits(b"xy"))])
    add("blocks/empty_dynamic_final", [fixed(lits(b"xy"), final=False), eob_only()])
    add("blocks/empty_dynamic_first", [eob_only(final=False), dyn([], final=False), fixed(lits(b"xy"))])
    add("blocks/empty_only", [fixed([], final=False), eob_only(final=False), stored(b"", final=False), dyn([])])
    r = _rng("forty")
    blocks, pos = [], 0
    for k in range(40):
        n = int(r.integers(3, 13))
        if k % 3 == 0:
            blocks.append(stored(noise(r, n)))
        else:
            t = random_tokens(r, n, pos=pos, p_match=0.7)
            blocks.append(fixed(t) if k % 3 == 1 else dyn(t))
        pos += n
    add("blocks/forty_mixed", blocks)


def _litcode(add):
    r = _rng("litcode")
    ladder = place([(97 + k, k + 1) for k in range(15)] + [(256, 15)], 257)
    add("litcode/ladder_1_to_15", [dynamic(lits(bytes(97 + int(k) for k in r.integers(0, 15, 200)) + bytes(range(97, 112))), ladder, [0])])
    used = list(range(65, 80)) + [256, 257, 260, 285]
    dl = place([(20 + k, k + 1) for k in range(9)] + list(zip(range(19), SLOW_SHAPE)), 29)
    t = lits(bytes(range(65, 80)) * 2)
    for k in range(19):
        t += [match((257, 260, 285)[k % 3], 0, k, 0), lit(65 + k % 15)]
    add("litcode/all_slow", [dynamic(t, slow_lit_lengths(used), dl, cl_symbols=rle(slow_lit_lengths(used) + dl))])
    ten = place([(s, s + 1) for s in range(8)] + [(65, 10), (66, 10), (67, 11), (68, 11), (69, 11), (256, 11)], 257)
    add("litcode/ten_and_eleven", [dynamic(lits(bytes(65 + int(k) for k in r.integers(0, 5, 300))), ten, [0])])
    add("litcode/eob_only", [dynamic([], [0] * 256 + [1], [0])])
    add("litcode/two_symbols", [dynamic(lits(b"x" * 37), place([(120, 1), (256, 1)], 257), [0])])
    t = random_tokens(r, 500)
    add("litcode/hlit257", [dyn(lits(noise(r, 300)), hlit=257)])
    add("litcode/hlit286", [dyn(t + [match(285, 0, 0, 0)], hlit=286)])


def _distcode(add):
    r = _rng("distcode")
    add("distcode/empty", [dyn(lits(noise(r, 100)), hdist=1)])
    t = lits(noise(r, 9))
    for n in (3, 70, 258):
        t += [match_value(n, 1)] + lits(noise(r, 3))
    ll, _ = lengths_of(t)
    add("distcode/one_code_0", [dynamic(t, ll, [1])])
    t = [match(257, 0, 29, 0), lit(1), match_value(258, 32768), match(270, 1, 29, 4000)]
    ll, _ = lengths_of(t)
    add("distcode/one_code_29", stored_run(noise(r, 32768)) + [dynamic(t, ll, [0] * 29 + [1], cl_symbols=rle(ll + [0] * 29 + [1]))])
    t = []
    for d in range(30):
        t += [match(257 + d % 29, 0, d, (1 << W.DIST_EXTRA[d]) - 1), lit(d)]
    ll, _ = lengths_of(t)
    order = [int(k) for k in r.permutation(30)]
    add("distcode/thirty_15bit", stored_run(noise(r, 32768)) + [dynamic(t, ll, place(zip(order, DIST30), 30))])
    add("distcode/hdist30", [dyn(random_tokens(r, 400), hdist=30)])


def _clcode(add):
    r = _rng("clcode")
    # HCLEN 5: only 16, 17, 18, 0 and 8 have codes; literals 1 .. 255 and end-of-block at 8 bits are a complete code
    s = Spell().v(0).v(8).r16(6)
    while len(s.lengths) < 257:
        s.r16(min(6, 257 - len(s.lengths))) if 257 - len(s.lengths) >= 3 else s.v(8)
    s.v(0)
    add("clcode/hclen5", [s.block(lits(noise(r, 64).replace(b"\0", b"\1")), 257, cl_lengths=place([(16, 1), (8, 2), (0, 3), (17, 4), (18, 4)], 19))])
    # HCLEN 19: length 15 is the last in the transmission order
    ladder = place([(97 + k, k + 1) for k in range(15)] + [(256, 15)], 257)
    add("clcode/hclen19", [dynamic(lits(b"abcdefghijklmno"), ladder, [0], cl_symbols=rle(ladder + [0]))])
    # 7-bit members, used: 16 and 10
    s = Spell().v(0).v(8)
    while len(s.lengths) < 255:
        s.r16(min(6, 255 - len(s.lengths))) if 255 - len(s.lengths) >= 3 else s.v(8)
    s.v(9, 2).v(10, 4).v(0, 2).v(1, 2)                    # 254 of 8 bits, two of 9, four of 10: complete; HLIT 261, distance codes 2 and 3
    add("clcode/seven_bit", [s.block(lits(noise(r, 64).translate(bytes(min(max(b, 1), 254) for b in range(256)))) + [match(257, 0, 2, 0)], 261,
                                     cl_lengths=place([(8, 1), (0, 2), (9, 3), (1, 4), (18, 5), (17, 6), (10, 7), (16, 7)], 19))])
    # every repeat symbol at both ends of its range: 162 zeros, then 4 of 6 bits and 120 of 7 (symbols 162 .. 285), two distance codes
    s = Spell().r18(138).r18(11).r17(10).r17(3).v(6).r16(3).v(7)
    for _ in range(19):
        s.r16(6)
    s.r16(3).v(7, 2).v(1, 2)
    t = lits(bytes(162 + int(k) for k in r.integers(0, 94, 120)))
    t += [match(285, 0, 0, 0), match(257, 0, 1, 0), match(284, 31, 0, 0)]
    add("clcode/repeat_extremes", [s.block(t, 286)])
    # a 16 from the literal lengths into the distance lengths: literals 0 .. 126 and end-of-block at 8 bits, length codes 257 and 258
    # at 2, four distance codes at 2
    low = bytes(b % 127 for b in range(256))
    s = Spell().v(8, 127).r18(129).v(8).v(2).r16(5)
    add("clcode/cross_16", [s.block(lits(noise(r, 50).translate(low)) + [match(257, 0, 2, 0), match(258, 0, 3, 0)], 259)])
    # a 17 and an 18 across the boundary (zeros); 16 right after 17 and after 18 repeats the zero
    high = bytes(max(b, 23) for b in range(256))
    s = Spell().r17(3).r16(3).r18(11).r16(6)              # literals 0 .. 22 unused
    for l in W.balanced_lengths(258 - 23, 15):            # 23 .. 257
        s.v(l)
    s.r17(3 + 4).v(1, 2)                                  # 258 .. 260 and distance codes 0 .. 3 at zero, 4 and 5 at one bit
    add("clcode/cross_17", [s.block(lits(noise(r, 60).translate(high)) + [match(257, 0, 4, 0), match(257, 0, 5, 1)], 261)])
    s = Spell().v(0, 23)
    for l in W.balanced_lengths(258 - 23, 15):
        s.v(l)
    s.r18(13 + 5).v(2, 4)                                 # 258 .. 270 and distance codes 0 .. 4 at zero, 5 .. 8 at two bits
    add("clcode/cross_18", [s.block(lits(noise(r, 60).translate(high)) + [match(257, 0, 5 + k, k & 1) for k in range(4)], 271)])
    # a 16 as the first distance length: it copies the two bits of length code 258
    s = Spell().v(8, 127).r18(129).v(8).v(2, 2).r16(3).v(2)
    add("clcode/sixteen_first_distance", [s.block(lits(noise(r, 50).translate(low)) + [match(257, 0, 3, 0), match(258, 0, 0, 0)], 259)])


def _symbols(add):
    for kind in ("fixed", "dynamic"):
        r = _rng("symbols", kind)
        dist = [(d, e) for d in range(30) for e in (0, (1 << W.DIST_EXTRA[d]) - 1)]
        t = []
        for k, (c, e) in enumerate([(c, e) for c in range(257, 286) for e in (0, (1 << W.LEN_EXTRA[c - 257]) - 1)] + [(285, 0), (284, 31)]):
            t += [match(c, e, *dist[k % 60])] + lits(noise(r, 2))
        add(f"symbols/{kind}_all", stored_run(noise(r, 32768)) + [fixed(t) if kind == "fixed" else dyn(t)])
    r = _rng("eqpos")
    add("symbols/distance_equals_position", [fixed(lits(noise(r, 5)) + [match_value(11, 5), match_value(16, 16), match_value(3, 32)])])


def _overlap(add):
    for n in OVERLAP_LENGTHS:
        r = _rng("overlap", n)
        t = []
        for d in OVERLAP_DISTANCES:
            t += lits(noise(r, 130)) + [match_value(n, d)]
        add(f"overlap/len{n}", [fixed(t + lits(noise(r, 5))) if n % 2 else dyn(t + lits(noise(r, 5)))])


def _boundary(add):
    for p in MATCH_STARTS:
        for n, d in ((258, min(p, 32768)), (64, 1), (129, 63)):
            r = _rng("start", p, n)
            add(f"boundary/start{p}_len{n}", stored_run(noise(r, p)) + [fixed([match_value(n, d)] + lits(noise(r, 3)) + [match_value(n, d)])])
    for k, n in enumerate(OUTPUT_SIZES):
        r = _rng("size", n)
        t = random_tokens(r, n)
        add(f"boundary/size{n}", [(fixed, dyn)[k % 2](t)])


def _input(add):
    for k in range(9):                                    # 8 + k bytes: k literals below 144 in a fixed block
        add(f"input/bytes{8 + k}", [fixed(lits(noise(_rng("bytes", k), k).translate(bytes(b & 127 for b in range(256)))))])
    for k in range(6):
        add(f"input/stored_bytes{11 + k}", [stored(noise(_rng("sbytes", k), k))])
    for n in (1, 3, 9):
        add(f"input/tail{n}", [dyn(random_tokens(_rng("tail", n), 300))], tail=b"\xff" * n)


def _prefix(add):
    r = _rng("prefix")
    add("prefix/stored", [fixed(lits(b"ab"), final=False), stored(noise(r, 40), final=False), stored(noise(r, 30))])
    add("prefix/fixed", [fixed(random_tokens(r, 400))])
    add("prefix/dynamic", [dyn(random_tokens(r, 300, p_match=0.3))])
    used = list(range(65, 80)) + [256, 257, 260, 285]
    t = lits(bytes(range(65, 80)))
    for k in range(12):
        t += [match((257, 260, 285)[k % 3], 0, k % 4, 0), lit(65 + k)]
    ll = slow_lit_lengths(used)
    add("prefix/dynamic_long", [dynamic(t, ll, [2] * 4, cl_symbols=rle(ll + [2] * 4))])


def _restream(add):
    p = scanline_like(_rng("restream"))
    for style in STYLES:
        add(f"restream/{style}", STYLES[style](p), cinfo=0 if style == "small_window" else 7)


@functools.lru_cache(maxsize=None)
def catalogue():
    """-> tuple of Case, in a fixed order; built once per process"""
    cases = []

    def add(name, blocks, **kw):
        data, payload = W.write(blocks, **kw)
        cases.append(Case(name, data, payload))

    for group in (_header, _stored, _blocks, _litcode, _distcode, _clcode, _symbols, _overlap, _boundary, _input, _prefix, _restream):
        group(add)
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def by_name(name):
    return next(c for c in catalogue() if c.name == name)


# ---- the malformed streams ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def malformed():
    """-> tuple of Bad: one fault each, with the status it must end in.  Every stream is followed by eight zero bytes, so that none of
    them is also truncated."""
    out = []

    def add(name, blocks, status):
        out.append(Bad("malformed/" + name, W.write(blocks)[0] + bytes(8), status))

    two = place([(65, 1), (256, 1)], 257)
    cl = place([(0, 2), (1, 2), (2, 2), (16, 3), (18, 3)], 19)
    add("hlit287", [dynamic([], place([(65, 1), (256, 1)], 287), [0])], 3)
    add("hdist31", [dynamic([], two, [0] * 31)], 3)
    add("sixteen_first", [dynamic([], two, [0], cl_symbols=[(16, 0)] + W.plain_cl_symbols(two[3:] + [0]), cl_lengths=cl)], 3)
    add("repeat_past_end", [dynamic([], two, [0], cl_symbols=W.plain_cl_symbols(two[:250]) + [(18, 0)], cl_lengths=cl, eob=False)], 3)
    add("no_end_of_block", [dynamic([lit(65)], place([(65, 1), (66, 1)], 257), [0], eob=False)], 3)
    add("hclen4_all_zero", [dynamic([], [0] * 257, [0], cl_symbols=[(18, 127), (18, 109)], cl_lengths=place([(18, 1), (0, 1)], 19), hclen=4, eob=False)], 3)
    add("cl_incomplete", [dynamic([], two, [0], cl_lengths=place([(0, 1), (1, 2)], 19))], 3)
    add("cl_oversubscribed", [dynamic([], two, [0], cl_lengths=place([(0, 1), (1, 1), (2, 1)], 19))], 3)
    add("lit_incomplete_2bit", [dynamic([lit(65)], place([(65, 2), (66, 2), (256, 2)], 257), [0])], 3)
    add("dist_incomplete_2bit", [dynamic([lit(65)], two, [2, 2, 2])], 3)
    one = place([(65, 2), (256, 2), (257, 1)], 258)
    add("one_code_distance_other_code", [dynamic([lit(65), sym(257), bits(1, 1)], one, [1], eob=False)], 4)
    add("empty_distance_code_used", [dynamic([lit(65), sym(257), bits(0, 4)], one, [0], eob=False)], 4)
    add("one_code_literal_other_code", [dynamic([bits(1, 1)], [0] * 256 + [1], [0], eob=False)], 4)
    add("fixed_literal_286", [fixed([lit(65), sym(286)], eob=False)], 4)
    add("fixed_distance_30", [fixed(lits(b"abcdef") + [match(257, 0, 30, 0)], eob=False)], 4)
    add("too_far_at_1", [fixed([lit(65), match_value(3, 2)])], 5)
    add("too_far_at_32767", stored_run(noise(_rng("far"), 32767)) + [fixed([match_value(3, 32768)])], 5)
    add("nlen_wrong", [stored(b"hello", nlen=5 ^ 0xFFFE)], 6)
    add("nlen_wrong_after_fixed", [fixed(lits(b"ab"), final=False), stored(b"", nlen=0xFFFE)], 6)
    return tuple(out)
