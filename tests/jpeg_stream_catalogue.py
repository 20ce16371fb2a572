"""The catalogue of conforming JPEG streams that no libjpeg encoder writes, shared by tests/test_jpeg_streams_host.py (every case against
live Pillow, the parsers and the host-stepped decoders) and tests/test_gpu_jpeg_streams.py (the kernels).  Every file is built at run
time from seeds by tests/jpeg_stream_writer.py; nothing here reads the library.

    for case in catalogue(): case.name, case.data, case.progressive, case.layout, case.tags
    pixels = reference(case.data, scale, mode)      # tests/scaled_decode_reference.decode, computed once per (file, scale, mode)
"""
import functools
from collections import namedtuple

import numpy as np

import jfif_reference as J
import jpeg_stream_writer as Wr
import scaled_decode_reference as R

Case = namedtuple("Case", "name data progressive layout tags")
LAYOUTS = ("444", "422", "420", "440", "grey")
W0, H0 = 52, 40                                        # the small shape: ragged in both directions under every layout, more than one MCU row
ONES = [(np.ones(64, np.int64), 0)]
NEVER_DC = {3: Wr.lengths([0, 2], [1, 2]), 4: Wr.lengths([0, 3], [1, 2])}      # by the flat DC value: '0' for category 0, '10' for its own (2 or 3)
NEVER_AC = Wr.single(0x00)
HOT = [0x00, 0x01, 0x11, 0xF0]


@functools.lru_cache(maxsize=None)
def reference(data, scale=1, mode="RGB"):
    out = R.decode(data, scale, mode)
    out.setflags(write=False)
    return out


def _rng(*key):
    return np.random.default_rng([ord(c) for c in "/".join(str(k) for k in key)])


def _ncomp(layout):
    return 1 if layout == "grey" else 3


def script_simple(n):
    """three kinds of scan: all DC, each component's low band, each component's high band"""
    return [(list(range(n)), 0, 0, 0, 0)] + [([c], 1, 5, 0, 0) for c in range(n)] + [([c], 6, 63, 0, 0) for c in range(n)]


def script_refine(n):
    """successive approximation in both DC and AC, with refinement scans whose correction bits meet open end-of-band runs"""
    return ([(list(range(n)), 0, 0, 0, 1)] + [([c], 1, 5, 0, 2) for c in range(n)] + [([c], 6, 63, 0, 2) for c in range(n)] +
            [([c], 1, 63, 2, 1) for c in range(n)] + [(list(range(n)), 0, 0, 1, 0)] + [([c], 1, 63, 1, 0) for c in range(n)])


def script_steps(n):
    """Al 3 -> 0 in single steps, DC and AC"""
    out = [(list(range(n)), 0, 0, 0, 3)] + [([c], 1, 63, 0, 3) for c in range(n)]
    for al in (2, 1, 0):
        out += [(list(range(n)), 0, 0, al + 1, al)] + [([c], 1, 63, al + 1, al) for c in range(n)]
    return out


PROG_AC = {0: Wr.spread(Wr.PROG_AC_SYMBOLS), 1: Wr.long_tail(Wr.PROG_AC_SYMBOLS, [0x00, 0x10, 0x01, 0x11])}


def flat(W, H, layout, dc, **kw):
    """a flat picture (dc: 3 or 4) under a one-code AC table and a two-code DC table: after the first block (2 + category + 1 bits: 5 for
    DC value 3, 6 for 4) every block is '00', and so is every guessed entry state's reading of the bits"""
    h, v, mx, my = Wr.grid(W, H, layout)
    comps = [(h, v, np.zeros((my * v, mx * h, 64), np.int64))] + [(1, 1, np.zeros((my, mx, 64), np.int64)) for _ in range(_ncomp(layout) - 1)]
    for c in comps:
        c[2][..., 0] = dc
    n = len(comps)
    return Wr.write(W, H, comps, qtables=ONES, dc_tables={0: NEVER_DC[dc]}, ac_tables={0: NEVER_AC}, selectors=[(0, 0, 0)] * n, **kw)


def _ff_blocks(rows, cols):
    """grey blocks whose bits hold long runs of ones under CHAIN_DC / CHAIN_AC: every third block a DC of 2047 (category 11 behind an
    eleven-ones code), the next one coefficients 1 and 2 at 1023 (ten ones behind a twelve-ones code), the third coefficients 6 and 7"""
    b = np.zeros((rows, cols, 64), np.int64)
    flat_ = b.reshape(-1, 64)
    flat_[0::3, 0] = 2047
    flat_[1::3, 1:3] = 1023
    flat_[2::3, 6:8] = 1023
    return b


CHAIN_DC = Wr.chain([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])
CHAIN_AC = Wr.chain([0x00, 0x01, 0x11, 0x02, 0x10, 0x20, 0x03, 0x04, 0x05, 0x30, 0x40, 0x50, 0x0A, 0x5A])


def ff_file(W, H, progressive=False, dri=2, shift=0, fill=0):
    """a grey file full of stuffed 0xFF bytes, with restart markers: the subject of the chunk-boundary placements"""
    _, _, mx, my = Wr.grid(W, H, "grey")
    kw = dict(sof=0xC2, script=script_simple(1)) if progressive else {}
    return Wr.write(W, H, [(1, 1, _ff_blocks(my, mx))], qtables=ONES, dc_tables={0: CHAIN_DC}, ac_tables={0: CHAIN_AC}, selectors=[(0, 0, 0)],
                    dri=dri, shift=shift, fill=fill, **kw)


def scan_bytes(data):
    """[(start, end)] of every scan's entropy-coded data, end at the marker that ends it"""
    _, scans = R.P.walk(data)
    return [(s["start"], s["end"]) for s in scans]


def placements(progressive):
    """[(name, data, check)]: ff_file with its bytes moved so that a stuffed pair, a restart marker, a fill run or EOI meets a 64-byte
    chunk boundary of (every) scan; check(data) asserts the positions"""
    out = []
    W, H = 48, 40

    def first_rst(d, a, b):
        p = a
        while not (d[p] == 0xFF and 0xD0 <= d[p + 1] <= 0xD7):
            p += 1
        return p

    def first_stuffed_after(d, p, b):
        while not (d[p] == 0xFF and d[p + 1] == 0x00):
            p += 1
            assert p < b
        return p

    base = ff_file(W, H, progressive)
    spans = scan_bytes(base)
    for what, target in (("stuffed", 63), ("stuffed", 127), ("rst", 63), ("fill", 66)):
        shifts = []
        for a, b in spans:
            r = first_rst(base, a, b)
            at = first_stuffed_after(base, r + 2, b) if what == "stuffed" else r
            assert at - a <= target - (4 if what == "fill" else 0)
            shifts.append(target - (at - a))
        data = ff_file(W, H, progressive, shift=shifts)

        def check(d, what=what, target=target):
            for a, b in scan_bytes(d):
                if what == "stuffed":
                    assert d[a + target] == 0xFF and d[a + target + 1] == 0x00 and d[a + target - 1] != 0xFF
                elif what == "rst":
                    assert d[a + target] == 0xFF and 0xD0 <= d[a + target + 1] <= 0xD7 and (target + 1) % 64 == 0
                else:
                    assert bytes(d[a + 62:a + 67]) == b"\xff" * 5 and 0xD0 <= d[a + 67] <= 0xD7
        out.append((f"{what}{target}", data, check))
    # the end of every scan: the 0xFF of the marker that ends it (the next SOS; EOI) as a chunk's last byte, and as the next chunk's first
    for target in (63, 64):
        small = ff_file(24, 8, progressive, dri=1)
        data = ff_file(24, 8, progressive, dri=1, shift=[target - (b - a) for a, b in scan_bytes(small)])

        def check(d, target=target):
            spans = scan_bytes(d)
            for k, (a, b) in enumerate(spans):
                assert b - a == target and d[b] == 0xFF and d[b + 1] == (0xD9 if k == len(spans) - 1 else 0xDA), (k, a, b)
            assert d[spans[-1][1]:] == b"\xff\xd9"
        out.append((f"eoi{target}", data, check))
    return out


def _reach_blocks():
    """hand-made grey blocks for the ends of a block's symbol sequence, in zigzag order"""
    only63, zrl3, full, empty = (np.zeros(64, np.int64) for _ in range(4))
    only63[63] = 2                                     # 62 zeros: three ZRL, then (14, 2)
    zrl3[14], zrl3[63] = -3, 1                         # after coefficient 14: 48 zeros, three ZRL in a row, then (0, 1)
    full[1:] = np.where(np.arange(63) % 2, 1, -1)      # ends at coefficient 63: no EOB
    seq = [only63, zrl3, full, empty, full, empty, empty, full, full, empty, only63, empty, zrl3, full, empty] * 2
    b = np.array(seq[:24]).reshape(3, 8, 64).copy()
    b[..., 0] = np.arange(24).reshape(3, 8) % 5 - 2
    return b


def _checker(H, W):
    """8 x 8 tiles in turn black, white and a one-pixel 0 / 255 checkerboard"""
    y, x = np.mgrid[0:H, 0:W]
    kind = (y // 8 + x // 8) % 3
    return np.where(kind == 0, 0, np.where(kind == 1, 255, ((y + x) % 2) * 255)).astype(np.uint8)


def uniform(data):
    """a baseline file of three components that all decode under one DC and one AC table (by content, whatever the ids): the bits of
    such a file never tell the block slot, and the library decodes a call that holds one with another family of slot kernels"""
    frame, scans = R.P.walk(data)
    if frame["sof"] == 0xC2 or len(frame["comps"]) != 3:
        return False
    (sc,) = scans
    return len({(repr(sc["dc"][td]), repr(sc["ac"][ta])) for _, td, ta in sc["comps"]}) == 1


@functools.lru_cache(maxsize=None)
def catalogue():
    out = []

    def add(name, data, layout, progressive=False, tags=()):
        out.append(Case(name, data, progressive, layout, tuple(tags) + (("uniform",) if uniform(data) else ())))

    # 1. never synchronises: odd first block (DC 3: 5 bits), and its even twin (DC 4: 6 bits)
    for W, H in ((96, 80), (264, 200)):
        for layout in ("grey", "420"):
            for parity, dc in (("odd", 3), ("even", 4)):
                add(f"never/{layout}/{W}x{H}/{parity}", flat(W, H, layout, dc), layout, tags=("never", parity))
                add(f"never/{layout}/{W}x{H}/{parity}/rows", flat(W, H, layout, dc, dri=Wr.grid(W, H, layout)[2]), layout, tags=("never-rows", parity))
    # 2. segments and slots
    for layout in ("grey", "420"):
        add(f"segments/flat/{layout}/dri1", flat(96, 80, layout, 3, dri=1), layout)
    for layout in LAYOUTS:
        comps = Wr.random_comps(_rng("segments", layout), W0, H0, layout)
        for dri in (1, 2, 3, 7, 1000):
            add(f"segments/{layout}/dri{dri}", Wr.write(W0, H0, comps, dri=dri), layout)
    # 3. padding and stray bytes, baseline and every scan of a progressive file
    stray = [("pad0", dict(pad=0)), ("fill1", dict(fill=1)), ("fill3", dict(fill=3)), ("fill70", dict(fill=70)), ("junk1", dict(junk=b"\x5a")),
             ("junk5", dict(junk=b"\x00\x12\xd0\xfe\x80")), ("junk-fill-eoi", dict(final=(b"\xa7\x01", 2))), ("pad0-junk-fill", dict(pad=0, junk=b"\x33", fill=2))]
    for k, (name, kw) in enumerate(stray):
        for j in range(2):
            layout = LAYOUTS[(2 * k + j) % 5]
            comps = Wr.random_comps(_rng("stray", name, layout), W0, H0, layout)
            add(f"stray/{name}/{layout}", Wr.write(W0, H0, comps, dri=2, **kw), layout)
            n = len(comps)
            add(f"stray/{name}/{layout}/progressive", Wr.write(W0, H0, comps, dri=3, sof=0xC2, script=script_simple(n), ac_tables=PROG_AC, **kw),
                layout, True)
    # 4. chunk boundaries (the positions are asserted by the tests: placements())
    for progressive in (False, True):
        for name, data, _ in placements(progressive):
            add(f"chunk/{name}" + ("/progressive" if progressive else ""), data, "grey", progressive, tags=("chunk",))
    # 5. code shapes
    big_ac = Wr.AC_SYMBOLS + [s for s in range(256) if s not in Wr.AC_SYMBOLS]
    shapes = [("long-tail", Wr.chain(Wr.DC_SYMBOLS), Wr.long_tail(Wr.AC_SYMBOLS, HOT), "each"),
              ("flat16-dc", Wr.flat16(Wr.DC_SYMBOLS), Wr.spread(Wr.AC_SYMBOLS), "one"),
              ("from3", Wr.from_length(Wr.DC_SYMBOLS, 3), Wr.from_length(Wr.AC_SYMBOLS, 3), "each"),
              ("single-dc", Wr.single(0), Wr.spread(Wr.AC_SYMBOLS[::-1]), "each"),
              ("lut-edge", Wr.lut_edge(Wr.DC_SYMBOLS[::-1]), Wr.lut_edge(Wr.AC_SYMBOLS), "one"),
              ("256", Wr.lut_edge(Wr.DC_SYMBOLS), Wr.long_tail(big_ac, HOT), "each"),
              ("twice", Wr.chain(Wr.DC_SYMBOLS[::-1]), Wr.long_tail(Wr.AC_SYMBOLS[::-1], [0x00]), "twice")]
    for k, (name, dct, act, dht) in enumerate(shapes):
        for j, layout in enumerate(LAYOUTS):
            comps = Wr.random_comps(_rng("shapes", name, layout), W0, H0, layout)
            if name == "single-dc":
                for c in comps:
                    c[2][..., 0] = 0
            n = len(comps)
            act1 = shapes[(k + 1) % len(shapes)][2]      # the chroma's AC table: the next shape's, so that the bits tell luma from chroma
            add(f"shapes/{name}/{layout}", Wr.write(W0, H0, comps, dc_tables={0: dct, 1: dct}, ac_tables={0: act, 1: act1},
                                                    selectors=[(0, 0, 0)] + [(1, 1, 1)] * (n - 1), dht=dht, dri=(0, 4)[j % 2]), layout)
            if n == 3 and j == (k + 1) % 4:            # and once with every component under the one pair (group "uniform")
                add(f"uniform/{name}/{layout}", Wr.write(W0, H0, comps, dc_tables={0: dct}, ac_tables={0: act}, selectors=[(0, 0, 0)] + [(1, 0, 0)] * 2,
                                                         dht=dht, dri=(0, 3)[k % 2]), layout)
            if j == k % 5:                             # the same as the DC and AC tables of a progressive file
                pact = {"long-tail": Wr.long_tail(Wr.PROG_AC_SYMBOLS, HOT + [0x10]), "from3": Wr.from_length(Wr.PROG_AC_SYMBOLS, 3),
                        "lut-edge": Wr.lut_edge(Wr.PROG_AC_SYMBOLS),
                        "256": Wr.long_tail(Wr.PROG_AC_SYMBOLS + [s for s in range(256) if s not in Wr.PROG_AC_SYMBOLS], HOT),
                        "twice": Wr.long_tail(Wr.PROG_AC_SYMBOLS[::-1], [0x00])}.get(name, Wr.spread(Wr.PROG_AC_SYMBOLS))
                add(f"shapes/{name}/{layout}/progressive",
                    Wr.write(W0, H0, comps, dc_tables={0: dct}, ac_tables={0: pact}, selectors=[(0, 0, 0)] + [(1, 0, 0)] * (n - 1), dht=dht, sof=0xC2,
                             script=script_refine(n), eob_cap=3), layout, True)
    # 6. selectors
    q90 = [(q, 0) for q in J.quant_tables(90)]
    four_q = [q90[1], q90[1], q90[1], q90[0]]
    dcs = {0: Wr.chain(Wr.DC_SYMBOLS), 1: J.DC_CHROMA, 2: Wr.lut_edge(Wr.DC_SYMBOLS), 3: J.DC_LUMA}
    acs = {0: Wr.spread(Wr.AC_SYMBOLS), 1: J.AC_CHROMA, 2: J.AC_LUMA, 3: Wr.long_tail(Wr.AC_SYMBOLS, HOT)}
    selector_cases = [("ids23", [(3, 3, 2), (1, 2, 3), (2, 2, 3)], None, 0xC0), ("cb-cr-differ", [(3, 0, 0), (1, 1, 3), (2, 2, 1)], None, 0xC0),
                      ("one-pair", [(1, 2, 3)] * 3, None, 0xC0), ("ids012", [(3, 3, 2), (2, 1, 1), (2, 1, 1)], [0, 1, 2], 0xC0),
                      ("ids102030", [(3, 3, 2), (1, 0, 0), (2, 1, 3)], [10, 20, 30], 0xC0), ("sof1", [(3, 3, 2), (1, 2, 3), (2, 2, 3)], None, 0xC1)]
    for k, (name, sel, ids, sof) in enumerate(selector_cases):
        for layout in (("444", "420", "422", "440")[k % 4], "grey"):
            comps = Wr.random_comps(_rng("selectors", name, layout), W0, H0, layout)
            add(f"selectors/{name}/{layout}", Wr.write(W0, H0, comps, qtables=four_q, dqt_split=k % 2 == 0, dc_tables=dcs, ac_tables=acs,
                                                       selectors=sel[:len(comps)], ids=ids[:len(comps)] if ids else None, sof=sof, dri=(0, 5)[k % 2]), layout)
    # 7. coefficient reach
    ones3 = [np.ones(64, np.int64)] * 3
    for name, img in (("checker", _checker(H0, W0)), ("checker-t", _checker(W0, H0).T)):
        for layout in ("grey", "420", "444"):
            rgb = img if layout == "grey" else np.stack([img, img[::-1], img[:, ::-1]], -1)
            comps = []
            for h, v, b in Wr.from_pixels(np.ascontiguousarray(rgb), ones3, layout):
                ac = np.clip(b, -1023, 1023)           # what an 8-bit file can hold: AC category 10, DC category 11
                ac[..., 0] = b[..., 0]
                comps.append((h, v, ac))
            add(f"reach/{name}/{layout}", Wr.write(W0, H0, comps, qtables=ONES + ONES, dc_tables={0: Wr.chain(Wr.DC_SYMBOLS[::-1]), 1: J.DC_CHROMA},
                                                   ac_tables={0: Wr.spread(Wr.AC_SYMBOLS[::-1]), 1: J.AC_CHROMA}), layout, tags=("reach",))
    add("reach/ends/grey", Wr.write(64, 24, [(1, 1, _reach_blocks())], qtables=ONES, selectors=[(0, 0, 0)]), "grey", tags=("reach",))
    # 8. 16-bit quantisation tables: the same values, and values above 255 on blocks that keep the samples inside +-512
    for layout in ("420", "422", "grey"):
        comps = Wr.random_comps(_rng("pq1-same", layout), W0, H0, layout)
        add(f"pq1/same/{layout}", Wr.write(W0, H0, comps, qtables=[(q, 1) for q in J.quant_tables(90)], dqt_split=False), layout, tags=("pq1",))
    for layout in ("444", "420", "440", "grey"):
        rng = _rng("pq1-big", layout)
        comps = Wr.random_comps(rng, W0, H0, layout)
        for h, v, b in comps:                          # DC +-6 and two AC terms +-1: |sample - 128| <= (6 / 8 + 2 * 0.25) * 400 = 500
            b[...] = 0
            b[..., 0] = rng.integers(-6, 7, b.shape[:2])
            pick = rng.integers(1, 64, b.shape[:2] + (2,))
            np.put_along_axis(b, pick, rng.choice([-1, 1], pick.shape), -1)
        big = [(rng.integers(256, 401, 64), 1), (rng.integers(256, 401, 64), 1)]
        add(f"pq1/big/{layout}", Wr.write(W0, H0, comps, qtables=big), layout, tags=("pq1",))
        add(f"pq1/big/{layout}/progressive", Wr.write(W0, H0, comps, qtables=big, sof=0xC2, script=script_simple(len(comps)), ac_tables=PROG_AC),
            layout, True, tags=("pq1",))
    # 9. progressive only
    def band(W, H, cap, dri=0, ends=True):
        _, _, mx, my = Wr.grid(W, H, "grey")
        b = np.zeros((my, mx, 64), np.int64)
        b[..., 0] = 40
        if ends:
            b[0, 0, 5] = b[-1, -1, 9] = 1              # something at either end of the band
        return Wr.write(W, H, [(1, 1, b)], sof=0xC2, script=[([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0)], ac_tables={0: Wr.spread(Wr.PROG_AC_SYMBOLS)},
                        selectors=[(0, 0, 0)], eob_cap=cap, dri=dri)
    add("eobrun/cat0", band(96, 80, 1), "grey", True)
    add("eobrun/cat1", band(96, 80, 2), "grey", True)
    add("eobrun/cat7", band(264, 200, 200), "grey", True)
    add("eobrun/cat9-one-run", band(264, 200, 0x7FFF), "grey", True)
    add("eobrun/cat14", band(1024, 1024, 0x7FFF, ends=False), "grey", True, tags=("large",))      # 16384 blocks: the smallest picture that holds such a run
    add("eobrun/ends-at-restart", band(96, 80, 0x7FFF, dri=12), "grey", True)
    for layout in LAYOUTS:
        comps = Wr.random_comps(_rng("prog", layout), W0, H0, layout)
        n = len(comps)
        add(f"refine/open-eobrun/{layout}", Wr.write(W0, H0, comps, sof=0xC2, script=script_refine(n), ac_tables=PROG_AC, eob_cap=0x7FFF, dri=(0, 6)[n % 2]),
            layout, True)
        add(f"refine/al3-steps/{layout}", Wr.write(W0, H0, comps, sof=0xC2, script=script_steps(n), ac_tables=PROG_AC,
                                                   scan_tables={2: ({0: Wr.chain(Wr.DC_SYMBOLS)}, {1: Wr.spread(Wr.PROG_AC_SYMBOLS[::-1])})}), layout, True)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# ---- outside the catalogue: what the decoders refuse -------------------------------------------------------------------------------------------
def refusal_files():
    """-> {name: (data, Pillow decodes it)}.  dc12: a DC difference of category 12, which T.81 allows only for 12-bit samples and libjpeg
    decodes all the same; dc16: a DC table that lists symbol 16; all-ones: a table whose last 16-bit code is all ones (code lengths
    1 .. 16 and one more of 16: the code space is full), which libjpeg refuses as over-subscribed"""
    rng = np.random.default_rng(12)
    comps = Wr.random_comps(rng, W0, H0, "grey", amplitude=40)
    wide = [(1, 1, comps[0][2].copy())]
    wide[0][2][1, 2, 0] = 3000                                     # differences of +-(3000 - its neighbours): category 12
    dc12 = Wr.write(W0, H0, wide, qtables=ONES, dc_tables={0: Wr.chain(list(range(13)))}, selectors=[(0, 0, 0)])
    dc16 = Wr.write(W0, H0, comps, dc_tables={0: Wr.chain(list(range(12)) + [16])}, selectors=[(0, 0, 0)])
    full = ([1] * 15 + [2], Wr.AC_SYMBOLS[:17])
    ok = Wr.write(W0, H0, comps, dc_tables={0: J.DC_LUMA}, ac_tables={0: J.AC_LUMA}, selectors=[(0, 0, 0)])
    at = ok.index(b"\xff\xc4", ok.index(b"\xff\xc4") + 2)          # the second DHT segment: the AC table's
    n = int.from_bytes(ok[at + 2:at + 4], "big")
    all_ones = ok[:at] + Wr._dht([(1, 0, full)], "each") + ok[at + 2 + n:]
    return {"dc12": (dc12, True), "dc16": (dc16, False), "all-ones": (all_ones, False)}
