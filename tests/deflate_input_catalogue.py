"""Seeded int32 arrays for the GPU deflate (csrc/deflate.hip) -- TEST INFRASTRUCTURE.  Plain numpy; nothing from the package.

    for name, array, claims in catalogue(capacities=(65536, 61440)): ...

The codec's coefficient arrays are mostly zeros and small magnitudes; these arrays are what it never writes.  Every entry says in ``claims``
what it was built to reach, and tests/test_deflate_inputs_host.py checks each claim by brute force:

    plants      [Plant]: a repeat put there on purpose (see Plant)
    distinct    True: the upper three bytes of the coefficients are pairwise distinct (outside the plants' copies), so that neither of
                the parser's two match shapes exists anywhere else
    no_match    True: distinct, and no plant: the stream can only be literals
    bytes       (lo, hi): every byte of the array lies in lo .. hi
    window      (pos, L, d): what an unrestricted LZ77 search finds at `pos` (borders/: more than the chunked parser can take)

What the parser can take (restated from csrc/deflate.hip's header and cost model, so that a plant can say whether it is meant to be taken):
a stream is cut into chunks of 8192 coefficients and sub-blocks of 64; a token is an "A" match of L coefficients (4 L bytes, L = 1 .. 64) or
a "B" match -- a literal low byte, then 3 + 4 L bytes (L = 0 .. 63) -- at a distance of d coefficients; destination and source lie in one
chunk and the destination in one sub-block.  Distances 1 .. 8 (`kLzNear`) are always tried; farther sources are found through a hash of
(upper three bytes of coefficient i, coefficient i + 1), so a far A match of one coefficient and a far B match of L = 0 are never seen, and
neither is anything at the last coefficient of a sub-block.  An A candidate must score above zero: 64 L > dist_cost(4 d)."""
from collections import namedtuple

import numpy as np

CHUNK, SUB, NEAR = 8192, 64, 8
SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 8191, 8192, 8193, 8192 + 63, 8192 + 64, 8192 + 65, 2 * 8192)
GROUPS = ("lengths", "distances", "literals", "runs", "ends", "adler", "borders")

Entry = namedtuple("Entry", "name array claims")
# kind "A": array[pos : pos + L] == array[pos - d : pos - d + L] and the next coefficient differs (or the sub-block ends)
# kind "B": array[pos] and array[pos - d] agree in their upper three bytes and differ in the low one, then L equal coefficients
# taken: the parser is expected to write exactly this match; why: the reason when it is not
Plant = namedtuple("Plant", "kind pos L d taken why", defaults=(True, ""))


def dist_cost(D):
    """lz_dist_cost of csrc/deflate.hip, in eighths of a bit (D: distance in bytes)"""
    x = D - 1
    if x < 2:
        return 16
    if x < 4:
        return 28
    e = x.bit_length() - 2
    return (28 if e <= 1 else 40) + 8 * e


def token_bytes(plant):
    """-> (match length in bytes, distance in bytes, output position of the match's first byte)"""
    if plant.kind == "A":
        return 4 * plant.L, 4 * plant.d, 4 * plant.pos
    return 3 + 4 * plant.L, 4 * plant.d, 4 * plant.pos + 1


def distinct_fill(rng, n, lo=0, hi=255):
    """n coefficients with bytes in lo .. hi whose upper three bytes are pairwise distinct"""
    span = hi - lo + 1
    assert n <= span ** 3
    upper = rng.choice(span ** 3, size=n, replace=False).astype(np.int64)
    b = np.empty((n, 4), np.uint8)
    b[:, 0] = rng.integers(lo, hi + 1, n)
    for k in (1, 2, 3):
        b[:, k] = lo + upper % span
        upper //= span
    return b.reshape(-1).view("<i4").copy() if n else np.zeros(0, np.int32)


def _copy(a, pos, L, d, kind):
    """plant a repeat at pos (sequentially, so that a distance below the length gives a periodic run)"""
    if kind == "B":
        a[pos] = (a[pos - d] & ~0xFF) | ((a[pos - d] ^ 0x55) & 0xFF)
        pos += 1
    for k in range(L):
        a[pos + k] = a[pos + k - d]


# ---- lengths/ ---------------------------------------------------------------------------------------------------------------------------
def _lengths(kind, far):
    """one plant per unit of 2 (near) or 4 (far) sub-blocks; the destination starts the unit's last sub-block"""
    rng = np.random.default_rng(100 + 2 * (kind == "B") + far)
    unit = 4 * SUB if far else 2 * SUB
    Ls = range(1, 65) if kind == "A" else range(0, 64)
    a = distinct_fill(rng, unit * 64 + (0 if far else SUB)).view(np.uint32).astype(np.int64)      # (far: two whole chunks)
    plants = []
    for k, L in enumerate(Ls):
        pos = unit * k + unit - SUB
        if far:
            d = 9 + (37 * L) % 92                       # 9 .. 100, below and above the length
            seen = L >= (2 if kind == "A" else 1)
            why = "" if seen else "the hash of a far source covers the next coefficient, which differs"
        else:
            d = 2 if (kind == "A" and L == 1) else 1 + (L + 2 * (kind == "B")) % NEAR      # (an A match of one coefficient scores 64 - dist_cost: positive up to d = 4)
            seen, why = True, ""
        _copy(a, pos, L, d, kind)
        plants.append(Plant(kind, pos, L, d, seen, why))
    return Entry(f"lengths/{kind}_{'far' if far else 'near'}", (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32), dict(plants=plants, distinct=True))


# ---- distances/ -------------------------------------------------------------------------------------------------------------------------
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
             24577]                                        # RFC 1951 3.2.5


def distance_grid():
    """coefficient distances that give every distance symbol a multiple of four bytes can have, at its lowest and highest such value,
    plus 9 (the first beyond kLzNear) and two values with bit 12 of a 13-bit extra set.  8191 is not among them: see _distances."""
    ds = {9}
    for s, base in enumerate(DIST_BASE):
        top = (DIST_BASE[s + 1] - 1) if s + 1 < len(DIST_BASE) else 32768
        multiples = [D for D in range(base, top + 1) if D % 4 == 0 and D // 4 <= CHUNK - 2]
        if multiples:
            ds.update((multiples[0] // 4, multiples[-1] // 4))
    ds.update(((16385 + 4096 + 3) // 4, (24577 + 4096 + 3) // 4))
    return sorted(ds)


def _distances():
    """repeats of 16 coefficients, placed greedily into chunks: source at q, copy at q + d inside one sub-block, a differing coefficient
    behind it.  The two largest distances leave no room for 16: d = 8190 is a B match of one coefficient at the chunk's last but one
    position (an A match of two scores 128 - dist_cost(32760) = -16 and is refused); d = 8191 could only end at the chunk's last
    coefficient, where a match can be one coefficient long and the chain is not walked -- planted, and expected to stay literals."""
    rng = np.random.default_rng(7)
    grid = [d for d in distance_grid() if d <= CHUNK - 16]
    chunks, plants, busy = [], [], None
    for d in grid:
        for attempt in (0, 1):
            if busy is None:
                busy = np.zeros(CHUNK, bool)
                busy[:2] = busy[-2:] = True               # (kept for the two largest distances in the first chunk)
                chunks.append(busy)
            found = None
            for q in range(0, CHUNK - d - 17):
                i = q + d
                if i % SUB + 17 <= SUB and not busy[q:q + min(d, 16)].any() and not busy[i:i + 17].any() and not (d < 16 and busy[q:i].any()):
                    found = (q, i)
                    break
            if found:
                break
            busy = None
        assert found, d
        q, i = found
        busy[q:q + min(d, 16)] = True
        busy[i:i + 17] = True
        plants.append(Plant("A", (len(chunks) - 1) * CHUNK + i, 16, d))
    a = distinct_fill(rng, len(chunks) * CHUNK).view(np.uint32).astype(np.int64)
    for p in plants:
        _copy(a, p.pos, p.L, p.d, "A")
    a[CHUNK - 2] = a[0] ^ 0x55                             # d = 8190: B, L = 1
    a[CHUNK - 1] = a[1]
    plants.append(Plant("B", CHUNK - 2, 1, CHUNK - 2))
    far = [Plant("A", CHUNK - 1, 1, CHUNK - 1, False, "a match at a sub-block's last coefficient is one coefficient long: only kLzNear is tried there")]
    out = [Entry("distances/grid", (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32), dict(plants=plants, distinct=True))]
    b = distinct_fill(np.random.default_rng(8), CHUNK)
    b[CHUNK - 1] = b[0]
    out.append(Entry("distances/d8191", b, dict(plants=far, distinct=True)))
    return out


# ---- literals/ --------------------------------------------------------------------------------------------------------------------------
def _literals(capacities):
    v = np.arange(256, dtype=np.int64)
    lanes = (v | ((v + 64) % 256) << 8 | ((v + 128) % 256) << 16 | ((v + 192) % 256) << 24).astype(np.uint32).view(np.int32)
    n = 2 * CHUNK + 65
    out = [Entry("literals/every_byte_every_lane", lanes, dict(no_match=True, distinct=True)),
           Entry("literals/high", distinct_fill(np.random.default_rng(21), n, 144, 255), dict(no_match=True, distinct=True, bytes=(144, 255))),
           Entry("literals/low", distinct_fill(np.random.default_rng(22), n, 0, 143), dict(no_match=True, distinct=True, bytes=(0, 143)))]
    cap = max(capacities)
    out.append(Entry("literals/high_capacity", distinct_fill(np.random.default_rng(23), cap, 144, 255),
                     dict(no_match=True, distinct=True, bytes=(144, 255), large=True)))
    return out


def literal_only_size(n, bits_per_byte=9):
    """bytes of the one-block fixed-code stream of n coefficients that are all literals of `bits_per_byte` bits"""
    return 2 + (3 + 4 * bits_per_byte * n + 7 + 7) // 8 + 4


# ---- runs/ ------------------------------------------------------------------------------------------------------------------------------
def _runs():
    n = CHUNK + 65
    out = []
    for v in (0, -1, 0x01020304, -0x80000000):
        out.append(Entry(f"runs/constant_{v & 0xFFFFFFFF:08x}", np.full(n, v, np.int32), dict(constant=v)))
    for p in (2, 3, 7, 63, 64, 65):
        base = ((np.arange(p, dtype=np.int64) + 1) * 0x00010001).astype(np.int32)      # p distinct values over a small byte alphabet
        out.append(Entry(f"runs/period_{p}", np.resize(base, n), dict(period=p)))
    rng = np.random.default_rng(31)
    body = rng.integers(-3, 4, n - 5000).astype(np.int32)
    body[0] = body[-1] = 3
    out.append(Entry("runs/leading_zeros", np.concatenate([np.zeros(5000, np.int32), body]), dict(zeros=(0, 5000))))
    out.append(Entry("runs/trailing_zeros", np.concatenate([body, np.zeros(5000, np.int32)]), dict(zeros=(n - 5000, n))))
    return out


# ---- ends/ and adler/ -------------------------------------------------------------------------------------------------------------------
def filling(kind, n, seed=0):
    if kind == "zeros":
        return np.zeros(n, np.int32)
    if kind == "ones":
        return np.full(n, -1, np.int32)                    # every byte 0xFF
    if kind == "random":
        return np.random.default_rng(40 + seed).integers(-4, 5, n).astype(np.int32)
    if kind == "nomatch":
        return distinct_fill(np.random.default_rng(50 + seed), n)
    if kind == "top5":                                     # bytes 251 .. 255: the largest Adler-32 partial sums short of all-0xFF
        return np.random.default_rng(60 + seed).integers(251, 256, 4 * n).astype(np.uint8).view("<i4").copy() if n else np.zeros(0, np.int32)
    raise ValueError(kind)


def _ends(capacities):
    out = []
    for kind in ("zeros", "ones", "random", "nomatch"):
        for k, n in enumerate(SIZES):
            out.append(Entry(f"ends/{kind}_{n}", filling(kind, n, k), dict(n=n, **({"no_match": True, "distinct": True} if kind == "nomatch" else {}))))
        for cap in capacities:
            out.append(Entry(f"ends/{kind}_capacity_{cap}", filling(kind, cap, cap % 97),
                             dict(n=cap, capacity=cap, large=True, **({"no_match": True, "distinct": True} if kind == "nomatch" else {}))))
    return out


def _adler(capacities):
    out = []
    for kind in ("ones", "top5"):
        for n in (CHUNK - 1, CHUNK + 1, 2 * CHUNK):
            out.append(Entry(f"adler/{kind}_{n}", filling(kind, n, n % 89), dict(n=n, bytes=(255, 255) if kind == "ones" else (251, 255))))
        for cap in capacities:
            out.append(Entry(f"adler/{kind}_capacity_{cap}", filling(kind, cap, 3), dict(n=cap, capacity=cap, large=True,
                                                                                         bytes=(255, 255) if kind == "ones" else (251, 255))))
    return out


# ---- borders/ ---------------------------------------------------------------------------------------------------------------------------
def _borders():
    """24 coefficients that straddle a border, repeated later: a source may not leave the destination's chunk and a token may not leave
    its sub-block, so the parser can take less than an unrestricted search finds (claims["window"])"""
    a = distinct_fill(np.random.default_rng(71), 2 * CHUNK)
    src, dst = CHUNK - 12, CHUNK + 1024 - 12               # the copy's second half starts a sub-block of the second chunk
    a[dst:dst + 24] = a[src:src + 24]
    chunk = Entry("borders/chunk", a, dict(distinct=True, window=(dst, 24, 1024), plants=[Plant("A", dst + 12, 12, 1024)]))
    b = distinct_fill(np.random.default_rng(72), CHUNK)
    src, dst = 2 * SUB - 12, 8 * SUB - 12                  # source and copy both straddle a sub-block border
    b[dst:dst + 24] = b[src:src + 24]
    sub = Entry("borders/sub_block", b, dict(distinct=True, window=(dst, 24, 6 * SUB), plants=[Plant("A", dst, 12, 6 * SUB), Plant("A", dst + 12, 12, 6 * SUB)]))
    return [chunk, sub]


def catalogue(capacities=(65536, 61440), groups=GROUPS):
    """-> [Entry].  capacities: the coefficient capacities of the layers the capacity-sized entries are made for."""
    out = []
    if "lengths" in groups:
        out += [_lengths(kind, far) for kind in "AB" for far in (False, True)]
    if "distances" in groups:
        out += _distances()
    if "literals" in groups:
        out += _literals(capacities)
    if "runs" in groups:
        out += _runs()
    if "ends" in groups:
        out += _ends(capacities)
    if "adler" in groups:
        out += _adler(capacities)
    if "borders" in groups:
        out += _borders()
    return out


# ---- tables/ : inputs plus foreign tables ---------------------------------------------------------------------------------------------------
def tables_catalogue(adaptive_table):
    """-> [(name, array, table, expect)] with expect "fixed" / "dynamic" / None (None: whichever is cheaper for the stream's own tokens).
    `adaptive_table` is deflate_reference.adaptive_table (handed in: this module imports nothing).  A table is one layer's [448] words."""
    N_LITLEN, N_DIST = 286, 30
    every = np.ones(N_LITLEN, np.int64), np.ones(N_DIST, np.int64)
    out = []
    # exactly one length symbol missing (270: lengths 23 .. 26, the A match of 6 coefficients), everything else coded; the counts favour
    # what a run of zeros needs, so that the table wins where the missing symbol is not needed
    ll = every[0].copy()
    ll[270] = 0
    ll[0], ll[284], every[1][3] = 100, 1000, 1000
    a_near = _lengths("A", False).array
    out.append(("tables/no_length_270", a_near, adaptive_table(ll, every[1], cover_all=False), "fixed"))
    # exactly one distance symbol missing (10: distances 33 .. 48 bytes, d = 9 .. 12 coefficients)
    dd = every[1].copy()
    dd[10] = 0
    grid = _distances()[0].array
    out.append(("tables/no_distance_10", grid, adaptive_table(every[0], dd, cover_all=False), "fixed"))
    # the same two tables on data that does not need the missing symbol: usable
    zeros = np.zeros(CHUNK + 65, np.int32)
    out.append(("tables/no_length_270_unneeded", zeros, adaptive_table(ll, every[1], cover_all=False), None))
    # the same on data the table would win on by far if the missing symbol were free: a run of zeros needs length symbol 284 (252 and
    # 256 bytes) and distance symbol 3 (4 bytes) and little else
    ll = np.ones(N_LITLEN, np.int64)
    ll[0], ll[284] = 100, 0
    dd = np.ones(N_DIST, np.int64)
    dd[3] = 1000
    out.append(("tables/no_length_284_on_zeros", zeros, adaptive_table(ll, dd, cover_all=False), "fixed"))
    ll[284], dd[3] = 1000, 0
    out.append(("tables/no_distance_3_on_zeros", zeros, adaptive_table(ll, dd, cover_all=False), "fixed"))
    # end of block without a code: adaptive_table always codes it, so the entry is blanked in a complete table
    t = adaptive_table(*every, cover_all=False).copy()
    t[256] = 0
    out.append(("tables/no_end_of_block", zeros, t, "fixed"))
    # literals rarest: 15-bit literal codes; on incompressible data the fixed code must win
    ll = np.ones(N_LITLEN, np.int64)
    ll[256:] = [1 << (12 + k) for k in range(30)]
    t15 = adaptive_table(ll, np.full(N_DIST, 1 << 20, np.int64), cover_all=False)
    assert max(int(t15[s]) >> 16 for s in range(256)) == 15
    out.append(("tables/literals_15_bits", filling("nomatch", 3000, 5), t15, "fixed"))
    # a tie, and one bit either side of it: see tie_case
    for k, (arr, tab, expect) in enumerate(tie_case(adaptive_table)):
        out.append((f"tables/tie_{('below', 'equal', 'above')[k]}", arr, tab, expect))
    # a complete table counted on another array
    other = filling("random", 5000, 9)
    hist = np.bincount(other.view(np.uint8), minlength=N_LITLEN)[:N_LITLEN]
    out.append(("tables/complete_from_other_array", grid, adaptive_table(hist, np.zeros(N_DIST, np.int64), cover_all=True), None))
    out.append(("tables/complete_on_codec_like", filling("random", CHUNK + 65, 2), adaptive_table(hist, np.zeros(N_DIST, np.int64), cover_all=True), None))
    return out


def tie_case(adaptive_table):
    """Arrays without any match (so their tokens are their bytes) whose stream costs, under one table, one bit less than / exactly as
    much as / one bit more than under the fixed code.  The table gives literals 0 .. 31 seven bits (the fixed code: eight) and some other
    literals below 144 eight bits (as the fixed code does); with `a` seven-bit bytes among otherwise eight-bit bytes
    dynamic - fixed = header + end-of-block - 10 - a.  -> [(array, table, expected kind)]"""
    ll = np.ones(286, np.int64)
    ll[:32] = 8
    ll[32:144] = 3
    table = adaptive_table(ll, np.ones(30, np.int64), cover_all=False)
    bits = [int(table[s]) >> 16 for s in range(286)]
    seven = [s for s in range(144) if bits[s] == 7]
    eight = [s for s in range(144) if bits[s] == 8]
    assert len(seven) >= 8 and len(eight) >= 32, (len(seven), len(eight))
    need = int(table[316]) + bits[256] - 10                # seven-bit bytes for a tie
    out = []
    for delta, expect in ((1, "dynamic"), (0, "fixed"), (-1, "fixed")):
        rng = np.random.default_rng(90)
        a, n = need + delta, need + 40
        e = np.array(eight[:32])
        upper = rng.choice(len(e) ** 3, size=n, replace=False)
        b = np.empty((n, 4), np.uint8)
        b[:, 0] = e[rng.integers(0, len(e), n)]
        b[:a, 0] = np.array(seven)[rng.integers(0, len(seven), a)]
        for k in (1, 2, 3):
            b[:, k] = e[upper % len(e)]
            upper //= len(e)
        out.append((b.reshape(-1).view("<i4").copy(), table, expect))
    return out
