"""A zlib (RFC 1950 / 1951) stream writer driven by an explicit description -- TEST INFRASTRUCTURE for the inflate tests.  Nothing here
compresses: the caller says which blocks the stream has, which code lengths a dynamic block declares and with which code-length symbols
its header spells them, and gives every token as code plus extra bits, so that streams no encoder writes (length 258 as code 284 with
extra 31, a 16 that repeats a zero, a one-code distance code) can be written, and malformed ones too.

    stream, payload = write([stored(b"abc"), fixed([lit(65), match(257, 0, 0, 0)])], cinfo=7, flevel=2)

Tokens: ``lit(b)``, ``match(length_code, length_extra, dist_code, dist_extra)`` and, for the malformed streams, ``sym(s)`` (the bare
literal / length code of symbol s) and ``bits(value, n)`` (raw bits, LSB first).  The last block is final unless a block says otherwise.
The Adler-32 is computed here from what the tokens expand to."""
import numpy as np

from deflate_reference import CL_ORDER, _Bits, canonical_codes

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class _Out(_Bits):
    """_Bits that moves finished bytes out of the accumulator, so that a long stream is not one growing integer"""

    def __init__(self):
        super().__init__()
        self.done = bytearray()

    def put(self, value, nbits):
        super().put(value, nbits)
        if self.n >= 512:
            k = self.n // 8
            self.done += (self.v & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.v >>= 8 * k
            self.n -= 8 * k

    def bytes(self):
        return bytes(self.done) + self.v.to_bytes((self.n + 7) // 8, "little")


def lit(b):
    return ("lit", int(b))


def match(length_code, length_extra, dist_code, dist_extra):
    return ("match", int(length_code), int(length_extra), int(dist_code), int(dist_extra))


def sym(s):
    return ("sym", int(s))


def bits(value, n):
    return ("bits", int(value), int(n))


def match_value(length, distance):
    """the token of a match given by value, in the usual (least) code: 258 is code 285"""
    lc = max(c for c in range(29) if LEN_BASE[c] <= length) if length < 258 else 28
    dc = max(c for c in range(30) if DIST_BASE[c] <= distance)
    return match(257 + lc, length - LEN_BASE[lc], dc, distance - DIST_BASE[dc])


def stored(data, nlen=None, final=None):
    return dict(kind="stored", data=bytes(data), nlen=nlen, final=final)


def fixed(tokens, eob=True, final=None):
    return dict(kind="fixed", tokens=list(tokens), eob=eob, final=final)


def plain_cl_symbols(lengths):
    """every code length spelled as itself: no 16 / 17 / 18"""
    return [(int(l), 0) for l in lengths]


def dynamic(tokens, lit_lengths, dist_lengths, cl_lengths=None, hclen=None, cl_symbols=None, eob=True, final=None):
    """lit_lengths: HLIT code lengths (257 .. 286 of them for a valid block), dist_lengths: HDIST of them.  cl_symbols: the header's
    code-length symbols as (symbol, extra value) pairs -- they are written as given, whether or not they spell the two lists.
    cl_lengths: the 19 lengths of the code-length code by symbol; by default a complete code over the symbols used.  hclen: how many of
    them are written; by default up to the last non-zero one in the transmission order."""
    if cl_symbols is None:
        cl_symbols = plain_cl_symbols(list(lit_lengths) + list(dist_lengths))
    if cl_lengths is None:
        cl_lengths = default_cl_lengths(cl_symbols)
    if hclen is None:
        hclen = max([4] + [k + 1 for k in range(19) if cl_lengths[CL_ORDER[k]]])
    return dict(kind="dynamic", tokens=list(tokens), lit=list(lit_lengths), dist=list(dist_lengths), cl=list(cl_lengths), hclen=hclen,
                cl_symbols=list(cl_symbols), eob=eob, final=final)


def default_cl_lengths(cl_symbols):
    """a complete, balanced code over the code-length symbols used (the more frequent ones get the shorter codes); a lone symbol gets
    an unused partner, since a code-length code of one code is incomplete"""
    used = sorted({s for s, _ in cl_symbols}, key=lambda s: -sum(1 for t, _ in cl_symbols if t == s))
    if len(used) < 2:
        used.append(next(s for s in (0, 8, 7) if s not in used))
    out = [0] * 19
    for l in balanced_lengths(len(used), 7):
        out[used.pop(0)] = l
    return out


def balanced_lengths(n, limit):
    """n code lengths of a complete code (Kraft sum exactly 1), ascending, none above `limit`"""
    assert 2 <= n <= 1 << limit
    k = (n - 1).bit_length()                    # 2^(k-1) < n <= 2^k: 2^k - n codes of k - 1 bits, the rest of k bits
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def kraft(lengths, limit=15):
    return sum(1 << (limit - l) for l in lengths if l)


def adler32(data):
    a, b = 1, 0
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    for i in range(0, len(d), 4096):
        c = d[i:i + 4096]
        n = len(c)
        b = (b + n * a + int((np.arange(n, 0, -1, dtype=np.int64) * c).sum())) % 65521
        a = (a + int(c.sum())) % 65521
    return (b << 16) | a


def _expand(out, tok):
    """append what a token stands for to the bytearray `out`; False where it stands for nothing (the malformed streams)"""
    if tok[0] == "lit":
        if tok[1] > 255:
            return False
        out.append(tok[1])
        return True
    if tok[0] != "match":
        return False
    _, lc, le, dc, de = tok
    if not (257 <= lc <= 285 and dc < 30):
        return False
    length, dist = LEN_BASE[lc - 257] + le, DIST_BASE[dc] + de
    if dist > len(out) or length > 258:
        return False
    for _ in range(length):
        out.append(out[-dist])
    return True


def _put_tokens(b, blk, lit_len, dist_len, out):
    lit_code, dist_code = canonical_codes(lit_len), canonical_codes(dist_len)

    def put_lit(s):
        assert lit_len[s], f"no code for literal / length symbol {s}"
        b.put_code(lit_code[s], lit_len[s])

    for tok in blk["tokens"]:
        if tok[0] == "bits":
            b.put(tok[1], tok[2])
            continue
        put_lit(tok[1])
        if tok[0] == "match":
            _, lc, le, dc, de = tok
            b.put(le, LEN_EXTRA[lc - 257] if lc <= 285 else 0)
            assert dist_len[dc], f"no code for distance symbol {dc}"
            b.put_code(dist_code[dc], dist_len[dc])
            b.put(de, DIST_EXTRA[dc] if dc < 30 else 0)
        if out is not None and not _expand(out, tok):
            out = None
    if blk["eob"]:
        put_lit(256)
    return out


def deflate(blocks):
    """-> (the raw deflate bytes, what they inflate to as far as the tokens are valid)"""
    b = _Out()
    out = bytearray()
    alive = out
    for k, blk in enumerate(blocks):
        final = blk["final"] if blk["final"] is not None else k == len(blocks) - 1
        b.put(1 if final else 0, 1)
        if blk["kind"] == "stored":
            b.put(0, 2)
            b.put(0, -b.n % 8)
            n = len(blk["data"])
            assert n <= 65535
            b.put(n, 16)
            b.put((n ^ 0xFFFF) if blk["nlen"] is None else blk["nlen"], 16)
            b.put(int.from_bytes(blk["data"], "little"), 8 * n)
            if alive is not None:
                alive += blk["data"]
        elif blk["kind"] == "fixed":
            b.put(1, 2)
            alive = _put_tokens(b, blk, FIXED_LIT, FIXED_DIST, alive)
        else:
            b.put(2, 2)
            b.put(len(blk["lit"]) - 257, 5)
            b.put(len(blk["dist"]) - 1, 5)
            b.put(blk["hclen"] - 4, 4)
            for i in range(blk["hclen"]):
                b.put(blk["cl"][CL_ORDER[i]], 3)
            cl_code = canonical_codes(blk["cl"])
            for s, extra in blk["cl_symbols"]:
                assert blk["cl"][s], f"no code for code-length symbol {s}"
                b.put_code(cl_code[s], blk["cl"][s])
                b.put(extra, CL_EXTRA.get(s, 0))
            alive = _put_tokens(b, blk, blk["lit"], blk["dist"], alive)
    return b.bytes(), bytes(out)


def zlib_header(cinfo=7, flevel=2, fdict=0):
    cmf = (cinfo << 4) | 8
    flg = (flevel << 6) | (fdict << 5)
    flg |= (31 - (cmf * 256 + flg) % 31) % 31
    return bytes([cmf, flg])


def write(blocks, cinfo=7, flevel=2, tail=b""):
    """-> (zlib stream, payload).  tail: bytes appended after the Adler-32 trailer."""
    body, payload = deflate(blocks)
    return zlib_header(cinfo, flevel) + body + adler32(payload).to_bytes(4, "big") + bytes(tail), payload
