"""Coefficient sets for the baseline (sequential) block coder that pixels never produce, the call of the host entry
aej_test_jfif_seq_scan_host on them, and the bytes and histograms the tests' restatements expect (jfif_options_reference's walk, cut
into restart intervals by jfif_restart_reference's rules).  Shared by tests/test_jfif_seq_host.py and tests/test_gpu_jfif_seq.py."""
import ctypes

import numpy as np

import jfif_options_reference as O
import jfif_restart_reference as RR

# name -> (hs, vs, components, W, H): grey 2 x 1 blocks; 4:4:4 two MCUs; 4:2:0 2 x 2 MCUs whose right column and bottom row hold both
# kinds of dummy block; 4:2:2 3 x 1 MCUs with a dummy at the right edge; 4:4:0 1 x 2 MCUs with a dummy at the bottom
LAYOUTS = {"grey": (1, 1, 1, 16, 8), "4:4:4": (1, 1, 3, 16, 8), "4:2:0": (2, 2, 3, 17, 17), "4:2:2": (2, 1, 3, 33, 8), "4:4:0": (1, 2, 3, 8, 24)}
AEJ_ERR_ARG, AEJ_ERR_CAPACITY = -1, -4


def geometry(layout):
    """-> (hs, vs, components, blocks per MCU, mcux, mcuy)"""
    hs, vs, nc, W, H = LAYOUTS[layout]
    return hs, vs, nc, hs * vs + nc - 1, -(-W // (8 * hs)), -(-H // (8 * vs))


def blocks_of(layout):
    _, _, _, bpm, mcux, mcuy = geometry(layout)
    return bpm * mcux * mcuy


def _reach():
    """the hand-made blocks of jpeg_stream_catalogue._reach_blocks, in its order: three ZRL then (14, 2); 48 zeros in the middle; a block
    that ends at coefficient 63 (no EOB); an empty one"""
    only63, zrl3, full, empty = (np.zeros(64, np.int64) for _ in range(4))
    only63[63] = 2
    zrl3[14], zrl3[63] = -3, 1
    full[1:] = np.where(np.arange(63) % 2, 1, -1)
    return [only63, zrl3, full, empty, full, empty, empty, full, full, empty, only63, empty, zrl3, full, empty]


def _extremes():
    """DC category 11 (the difference of 1023 and -1024) and AC category 10 at both signs, first and last coefficient"""
    out = []
    for dc, ac, where in ((1023, 1023, 1), (-1024, -1023, 1), (1023, -1023, 63), (-1024, 1023, 63)):
        b = np.zeros(64, np.int64)
        b[0], b[where], b[5] = dc, ac, -2
        out.append(b)
    return out


def _runs():
    """a zero run of exactly 16, 32 and 48 before a value; 47 zeros before coefficient 63; exactly 16 zeros before coefficient 63"""
    out = []
    for at, v in ((17, 3), (33, -3), (49, 7)):
        b = np.zeros(64, np.int64)
        b[at] = v                                                # zeros 1 .. at - 1
        out.append(b)
    b = np.zeros(64, np.int64)
    b[15], b[63] = 1, -5
    out.append(b)
    b = np.zeros(64, np.int64)
    b[1:47], b[63] = 1, 1
    out.append(b)
    return out


def _cycle(seq, n, phase):
    c = np.array([seq[(phase + i) % len(seq)] for i in range(n)], np.int64)
    return c


def sets(layout):
    """-> [(name, int16 [blocks][64] in zigzag and MCU order)]: the sequences above from several phases (a short layout sees every pair
    of neighbours), and a seeded random fill of amplitude 250"""
    n = blocks_of(layout)
    out = []
    reach = _reach()
    for phase in range(0, len(reach), max(1, n - 1)):
        c = _cycle(reach, n, phase)
        c[:, 0] = (np.arange(n) + phase) % 5 - 2
        out.append((f"reach{phase}", c))
    for name, seq in (("extremes", _extremes()), ("runs", _runs())):
        for phase in range(0, len(seq), max(1, n - 1)):
            c = _cycle(seq, n, phase)
            if name == "runs":
                c[:, 0] = (np.arange(n) * 7 + phase) % 9 - 4
            out.append((f"{name}{phase}", c))
    rng = np.random.default_rng(20260 + n)
    out.append(("random", rng.integers(-250, 251, (n, 64))))
    return [(name, np.ascontiguousarray(c, np.int16)) for name, c in out]


def intervals(layout):
    """the restart intervals the tests run: none, every MCU, every second, and one longer than the scan"""
    _, _, _, _, mcux, mcuy = geometry(layout)
    return (0, 1, 2, mcux * mcuy + 1)


def scan_host(lib, coef, layout, R, optimize, capacity=None):
    """aej_test_jfif_seq_scan_host -> (rc, bytes, int64 [4][257], length)"""
    hs, vs, nc, bpm, mcux, mcuy = geometry(layout) if isinstance(layout, str) else layout
    coef = np.ascontiguousarray(coef, np.int16)
    assert coef.shape == (bpm * mcux * mcuy, 64)
    cap = coef.shape[0] * 53 * 4 * 2 + 64 if capacity is None else capacity
    out, n = (ctypes.c_uint8 * max(cap, 1))(), ctypes.c_uint64()
    hist = np.full((4, 257), -7, np.int64)
    rc = lib.aej_test_jfif_seq_scan_host(coef.ctypes.data, mcux * mcuy, hs, vs, nc, R, optimize, hist.ctypes.data, ctypes.addressof(out), cap,
                                         ctypes.addressof(n))
    return rc, bytes(out[:min(n.value, cap)]), hist, n.value


def scan_blocks(coef, layout):
    """the (component, block) list jfif_options_reference walks"""
    hs, vs, nc, bpm, _, _ = geometry(layout)
    return [(max(0, i % bpm - hs * vs + 1), coef[i].astype(np.int64)) for i in range(coef.shape[0])]


def writer_comps(coef, layout):
    """the coefficients as tests/jpeg_stream_writer.write takes them: [(h, v, blocks [rows][cols][64])] over the whole MCU grid"""
    hs, vs, nc, bpm, mcux, mcuy = geometry(layout)
    c = coef.astype(np.int64).reshape(mcuy, mcux, bpm, 64)
    luma = c[:, :, :hs * vs].reshape(mcuy, mcux, vs, hs, 64).transpose(0, 2, 1, 3, 4).reshape(mcuy * vs, mcux * hs, 64)
    return [(hs, vs, luma)] + [(1, 1, c[:, :, hs * vs + k]) for k in range(nc - 1)]


def expected(coef, layout, R, optimize):
    """-> (the stuffed scan bytes with RSTn markers, the histograms [4][257]) by the restatements: every restart interval is a scan of
    its own for jfif_options_reference (predictors 0, padded to a byte), under the tables of the whole scan's symbols"""
    hs, vs, nc, bpm, mcux, mcuy = geometry(layout)
    blocks = scan_blocks(coef, layout)
    W, H = LAYOUTS[layout][3:]
    if layout == "4:4:0":                                        # the rules know an MCU by its block count alone: 4:2:2 transposed
        ivs, resets, marks = RR.block_map(W, H, "4:2:2", 3, R)
    else:
        ivs, resets, marks = RR.block_map(H, W, "4:4:4" if nc == 1 else layout, nc, R)
    assert len(ivs) == len(blocks)
    parts = [[b for b, iv in zip(blocks, ivs) if iv == k] for k in range(len(marks))]
    for k in range(len(marks)):                                  # the interval's first block of every component resets, and no other
        first = ivs.index(k)
        assert [i for i, r in enumerate(resets) if r and ivs[i] == k] == [first + j for j in range(bpm) if j == 0 or j >= hs * vs]
    hist = sum(O.histogram(p) for p in parts)
    if optimize:
        tabs = [O.optimal_table(h) for h in hist[:2 if nc == 1 else 4]]
    else:
        tabs = O.tables(None, False)
    tabs = (tabs * 2)[:4]                                        # (grey: the chroma slots are never used)
    data = b"".join((bytes([0xFF, m]) if m else b"") + O.entropy(p, tabs) for p, m in zip(parts, marks))
    return data, hist
