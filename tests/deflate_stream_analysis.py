"""What a zlib stream's trace (tests/inflate_reference.py) says about the encoder that wrote it -- TEST INFRASTRUCTURE for the tests of
csrc/deflate.hip.  From the trace and the decoded bytes: the token list, the exact number of bits those tokens cost under RFC 1951's fixed
code and under a table in the layout of include/aej.h (``table[316]`` header bits + code lengths + extra bits + end of block), and the
symbol counts.  Matches are costed in the usual (least) code: length 258 is symbol 285."""
import numpy as np

from deflate_reference import HDR_BITS_AT, HIST_BINS, N_LITLEN, distance_symbol, length_symbol
from deflate_stream_writer import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA

FIXED_LIT_BITS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8      # RFC 1951 3.2.6


def tokens_of(trace, out):
    """[('lit', byte) | ('match', length, distance)] in stream order: the bytes no match produced are the literals"""
    toks, p = [], 0
    for dist, length, at in trace.matches:
        assert p <= at, "matches are recorded in output order"
        toks += [("lit", b) for b in out[p:at]]
        toks.append(("match", length, dist))
        p = at + length
    assert p <= len(out)
    toks += [("lit", b) for b in out[p:]]
    return toks


def fixed_bits(tokens):
    """bits of the one final fixed block that holds `tokens`: 3 header bits, the tokens, 7 bits of end of block"""
    n = 3 + 7
    for t in tokens:
        if t[0] == "lit":
            n += FIXED_LIT_BITS[t[1]]
        else:
            ls, _, le = length_symbol(t[1])
            n += FIXED_LIT_BITS[ls] + le + 5 + distance_symbol(t[2])[2]
    return n


def table_bits(tokens, table):
    """bits of the one block `table` opens that holds `tokens`, or None where the table has no code for a symbol they need (end of
    block included)"""
    bits = lambda s: int(table[s]) >> 16
    if bits(256) == 0:
        return None
    n = int(table[HDR_BITS_AT]) + bits(256)
    for t in tokens:
        if t[0] == "lit":
            k = bits(t[1])
            if k == 0:
                return None
            n += k
        else:
            ls, _, le = length_symbol(t[1])
            ds, _, de = distance_symbol(t[2])
            k, kd = bits(ls), bits(N_LITLEN + ds)
            if k == 0 or kd == 0:
                return None
            n += k + le + kd + de
    return n


def stream_bytes(block_bits):
    """zlib header, the block padded to a byte, Adler-32"""
    return 2 + (block_bits + 7) // 8 + 4


def symbol_counts(trace):
    """the trace's counts in the layout of the kernels' histogram: [0 .. 285] literal / length symbols, [286 .. 315] distance symbols"""
    h = np.zeros(HIST_BINS, np.int64)
    h[:N_LITLEN] = trace.lit_counts
    h[N_LITLEN:N_LITLEN + 30] = trace.dist_counts
    return h


def expected_kind(tokens, table):
    """which code an encoder that takes the cheaper one -- the fixed code on a tie, or where the table lacks a code -- uses, and the
    stream's size: -> ("fixed" | "dynamic", bytes)"""
    f = fixed_bits(tokens)
    d = table_bits(tokens, table) if table is not None else None
    if d is None or f <= d:
        return "fixed", stream_bytes(f)
    return "dynamic", stream_bytes(d)


def reachable_symbols(d_max=8191):
    """from RFC 1951's tables (held by the stream writer): the length symbols of 4 L (L = 1 .. 64) and 3 + 4 L (L = 0 .. 63) bytes and the
    distance symbols of 4 d bytes (d = 1 .. d_max), each with the least and the greatest extra value such a number gives it"""
    def of(values, base, extra, first):
        out = {}
        for v in values:
            s = max(k for k in range(len(base)) if base[k] <= v)
            x = v - base[s]
            assert 0 <= x < (1 << extra[s]) or (extra[s] == 0 and x == 0)
            lo, hi = out.get(first + s, (x, x))
            out[first + s] = (min(lo, x), max(hi, x))
        return out
    lens = of([4 * L for L in range(1, 65)] + [3 + 4 * L for L in range(64)], LEN_BASE, LEN_EXTRA, 257)
    dists = of([4 * d for d in range(1, d_max + 1)], DIST_BASE, DIST_EXTRA, 0)
    return lens, dists
