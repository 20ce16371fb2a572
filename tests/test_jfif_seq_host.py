"""The baseline (sequential) entropy coder on the host side (no GPU needed): aej_test_jfif_seq_scan_host -- the block coder, DC
predictor, interval placement, padding and stuffing the kernels of csrc/jfif.hip run -- against the tests' restatements on coefficient
sets pixels never produce, with and without restart intervals; whole files of seeded images against Pillow; the refusals and the ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_restart_reference as RR  # noqa: E402
import jfif_seq_cases as C  # noqa: E402

from adaptive_edge_aware_jpeg_amd import standard_jpeg as S  # noqa: E402
from adaptive_edge_aware_jpeg_amd._lib import SIGNATURES, load_library  # noqa: E402

PILLOW_LAYOUTS = ("grey", "4:4:4", "4:2:2", "4:2:0")


@pytest.mark.parametrize("layout", list(C.LAYOUTS))
def test_host_coder_equals_the_restatement(layout):
    """every coefficient set: the Annex K tables without intervals, the scan's own tables with every interval"""
    lib = load_library()
    seen = set()
    for name, coef in C.sets(layout):
        for R, opt in [(0, 0)] + [(R, 1) for R in C.intervals(layout)]:
            rc, data, hist, n = C.scan_host(lib, coef, layout, R, opt)
            want, want_hist = C.expected(coef, layout, R, opt)
            assert rc == 0 and n == len(data), (name, R, opt)
            assert np.array_equal(hist, want_hist), (name, R, opt)
            assert data == want, (name, R, opt)
        seen.add(name.rstrip("0123456789"))
    assert seen == {"reach", "extremes", "runs", "random"}


def test_the_sets_hold_what_they_are_for():
    """ZRL symbols alone and in a row, blocks without EOB, DC category 11, AC category 10, and with intervals RST markers in the bytes"""
    lib = load_library()
    hist = sum(C.scan_host(lib, coef, "4:2:0", 0, 1)[2] for _, coef in C.sets("4:2:0"))
    assert hist[1, 0xF0] > 0 and hist[0, 11] > 0 and hist[1, 0x0A] > 0 and hist[1, 0x9A] > 0 and hist[1, 0xE2] > 0 and hist[1, 0xF3] > 0
    n = C.blocks_of("4:2:0")
    name, coef = C.sets("4:2:0")[0]
    assert name == "reach0" and C.scan_host(lib, coef, "4:2:0", 0, 1)[2][[1, 3], 0x00].sum() < n      # blocks that end at coefficient 63
    data = C.scan_host(lib, coef, "4:2:0", 1, 1)[1]
    assert [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and data[i + 1] != 0] == [0xD0, 0xD1, 0xD2]


@pytest.mark.parametrize("layout", ["grey", "4:2:0"])
def test_the_files_of_the_gpu_test_hold_the_sets(layout):
    """tests/test_gpu_jfif_seq.py hands the sets to the transcoder as files of tests/jpeg_stream_writer.py: under the Annex K tables
    their scan is the host entry's, so the blocks are where the entry expects them"""
    import jpeg_stream_writer as W
    lib = load_library()
    for name, coef in C.sets(layout):
        data = W.write(*C.LAYOUTS[layout][3:], C.writer_comps(coef, layout))
        (sos,) = [(a, b) for m, a, b in RR.walk(data) if m == 0xDA]
        assert data[sos[0] + 2 + int.from_bytes(data[sos[0] + 2:sos[0] + 4], "big"):sos[1]] == C.scan_host(lib, coef, layout, 0, 0)[1], name


def _coefs(lib, x, q, layout):
    h, w = x.shape[:2]
    if layout == "grey":
        call = lambda src, dst, cap: lib.aej_jfif_many_coefs_grey_host(w, h, q, src, dst, cap)  # noqa: E731
    else:
        call = lambda src, dst, cap: lib.aej_jfif_many_coefs_host(w, h, q, S.SUBSAMPLING[layout], src, dst, cap)  # noqa: E731
    n = call(None, None, 0)
    out = np.zeros((n, 64), np.int16)
    x = np.ascontiguousarray(x)
    assert n > 0 and call(x.ctypes.data, out.ctypes.data, n) == n
    return out


def _dht(cls_id, bits, vals):
    body = bytes([cls_id]) + bytes(bits) + bytes(vals)
    return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body


def file_of(lib, coef, geom, q, H, W, layout, optimize):
    """the whole baseline file without a device: the library's markers (with the DHTs of the scan's own histograms when optimised), the
    host entry's scan, EOI"""
    rc, data, hist, _ = C.scan_host(lib, coef, geom, 0, optimize)
    assert rc == 0
    hdr = S.headers(q, H, W, "4:4:4" if layout == "grey" else layout, mode="L" if layout == "grey" else "RGB")
    if optimize:
        segs = RR.walk(hdr + b"\xff\xd9")
        ids = [hdr[a + 4] for m, a, b in segs if m == 0xC4]
        assert ids == [0x00, 0x10, 0x01, 0x11][:len(ids)]
        own = b"".join(_dht(i, *S.huffman_table(hist[t])) for t, i in enumerate(ids))
        first = min(a for m, a, b in segs if m == 0xC4)
        hdr = hdr[:first] + own + b"".join(hdr[a:b] for m, a, b in segs if m == 0xDA)
    return hdr + data + b"\xff\xd9"


@pytest.mark.parametrize("layout", PILLOW_LAYOUTS)
def test_whole_files_equal_pillow(layout):
    """aej_jfif_many_coefs_host, then the host entry, then the library's markers: Pillow's file of a 17 x 17 image, byte for byte"""
    lib = load_library()
    H = W = 17
    x = RR.gradient(H, W, seed=17)
    hs, vs, nc = C.LAYOUTS[layout][:3]
    geom = (hs, vs, nc, hs * vs + nc - 1, -(-W // (8 * hs)), -(-H // (8 * vs)))
    if layout == "grey":
        x = np.ascontiguousarray(x[:, :, 1])
    for q in (30, 90):
        coef = _coefs(lib, x, q, layout)
        for opt in (0, 1):
            kw = {} if layout == "grey" else dict(subsampling=layout)
            assert file_of(lib, coef, geom, q, H, W, layout, opt) == RR.pil_save(x, q, optimize=bool(opt), **kw), (q, opt)


def test_refusals():
    lib = load_library()
    coef = C.sets("4:2:0")[0][1]
    ok = lambda *a, **k: C.scan_host(lib, *a, **k)[0]  # noqa: E731
    assert ok(coef, "4:2:0", 0, 0) == 0
    assert ok(coef, "4:2:0", 1, 0) == C.AEJ_ERR_ARG              # an interval needs the scan's own tables, as in the chain
    assert ok(coef, "4:2:0", -1, 1) == C.AEJ_ERR_ARG and ok(coef, "4:2:0", 65536, 1) == C.AEJ_ERR_ARG and ok(coef, "4:2:0", 65535, 1) == 0
    assert ok(coef, "4:2:0", 0, 2) == C.AEJ_ERR_ARG
    for v, at in ((2048, 0), (-2048, 7), (2048, 24 * 64 - 1)):
        bad = coef.copy()
        bad.reshape(-1)[at] = v
        assert ok(bad, "4:2:0", 0, 1) == C.AEJ_ERR_ARG, (v, at)
        bad.reshape(-1)[at] = 2047 if v > 0 else -2047
        assert ok(bad, "4:2:0", 0, 1) == 0, (v, at)
    for hs, vs, nc in ((3, 1, 3), (0, 1, 3), (1, 4, 3), (2, 2, 2), (1, 1, 0), (1, 1, 4)):
        assert ok(np.zeros(((hs * vs + 2), 64), np.int16), (hs, vs, nc, hs * vs + 2, 1, 1), 0, 1) == C.AEJ_ERR_ARG, (hs, vs, nc)
    assert ok(np.zeros((1, 64), np.int16), (2, 2, 1, 1, 1, 1), 0, 1) == 0      # one component is sampled 1 x 1 whatever it says
    rc, _, _, n = C.scan_host(lib, coef, "4:2:0", 0, 1, capacity=3)
    full = C.scan_host(lib, coef, "4:2:0", 0, 1)
    assert rc == C.AEJ_ERR_CAPACITY and n == full[3] > 3
    hist, out, n = np.zeros((4, 257), np.int64), (ctypes.c_uint8 * 4096)(), ctypes.c_uint64()
    args = [coef.ctypes.data, 4, 2, 2, 3, 0, 1, hist.ctypes.data, ctypes.addressof(out), 4096, ctypes.addressof(n)]
    assert lib.aej_test_jfif_seq_scan_host(*args) == 0
    for null in (0, 7, 8, 10):
        assert lib.aej_test_jfif_seq_scan_host(*[None if i == null else a for i, a in enumerate(args)]) == C.AEJ_ERR_ARG, null
    assert lib.aej_test_jfif_seq_scan_host(*[0 if i == 1 else a for i, a in enumerate(args)]) == C.AEJ_ERR_ARG


def test_symbol_exported_and_declared():
    lib = load_library()
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "aej_testing.h")) as f:
        ht = f.read()
    name = "aej_test_jfif_seq_scan_host"
    assert name in SIGNATURES and getattr(lib, name) is not None and f" {name}(" in ht
    assert lib.aej_abi_version() == 3
