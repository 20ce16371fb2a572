"""CPU: the one chroma up-sampling rule of the JPEG reconstruction kernels (jd_up_chroma of csrc/jpegdec_core.h, through its host twin
aej_test_jpeg_upsample_host) against the independent models the other tests already judge whole decodes by -- _upsample_h2v1 of
tests/progressive_reference.py, upsample_h1v2 of tests/scaled_decode_reference.py, the h2v2 _upsample of tests/jfif_reference.py,
np.repeat for replication -- and the one MCU window (aej_jpegdec_sbox_window_host) against the rule: a part of the plane that holds the
window's samples alone is enough for every pixel of the box."""
import ctypes

import numpy as np
import pytest

import jfif_reference as J
import progressive_reference as P
import scaled_decode_reference as SD

WIDTHS = (1, 2, 3, 4, 9)          # chroma samples a row: replication up to two wide, the first filtered width, interior
HEIGHTS = (1, 2, 3)
COMBOS = ((1, 1, True), (2, 1, True), (2, 1, False), (1, 2, True), (1, 2, False), (2, 2, True))      # uh, uv, fancy
LAYOUTS = (("444", 1, 1), ("422", 2, 1), ("420", 2, 2), ("440", 1, 2))


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


def reference(c, uh, uv, fancy, OH, OW):
    """the real samples c [hc][wc] up-sampled to [OH][OW] by libjpeg's rule for (uh, uv, fancy), from the models of the other tests"""
    c = c.astype(np.int64)
    if not fancy:
        return np.repeat(np.repeat(c, uv, 0), uh, 1)[:OH, :OW]
    if (uh, uv) == (1, 1):
        return c[:OH, :OW]
    if (uh, uv) == (2, 1):
        return P._upsample_h2v1(c, OW)[:OH]
    if (uh, uv) == (1, 2):
        return SD.upsample_h1v2(c, OH)[:, :OW]
    return J._upsample(c, OH, OW)


def rule(lib, part, stride, off, uh, uv, fancy, wc, hc, box):
    """aej_test_jpeg_upsample_host over the pixels of box = (l, t, r, b); part: a uint8 array whose first byte is the part's first"""
    l, t, r, b = box
    out = np.full((b - t, r - l), 77, np.uint8)
    rc = lib.aej_test_jpeg_upsample_host(part.ctypes.data, stride, off, uh, uv, int(fancy), wc, hc, l, t, r, b, out.ctypes.data)
    assert rc == 0, (uh, uv, fancy, wc, hc, box)
    return out


@pytest.mark.parametrize("uh,uv,fancy", COMBOS, ids=["%dx%d%s" % (c[0], c[1], "" if c[2] else "-plain") for c in COMBOS])
def test_rule_equals_the_models(lib, uh, uv, fancy):
    rng = np.random.default_rng(1000 * uh + 100 * uv + fancy)
    for wc in WIDTHS:
        for hc in HEIGHTS:
            for OW in ((2 * wc - 1, 2 * wc) if uh == 2 else (wc,)):    # output sizes of both parities over wc x hc real samples
                for OH in ((2 * hc - 1, 2 * hc) if uv == 2 else (hc,)):
                    # the plane is wider and taller than its real samples, as a plane of whole MCUs is, and what lies outside them is
                    # noise: the edge rules go by wc and hc
                    plane = rng.integers(0, 256, (hc + 2, wc + 3), dtype=np.uint8)
                    want = reference(plane[:hc, :wc], uh, uv, fancy, OH, OW)
                    got = rule(lib, plane, wc + 3, 0, uh, uv, fancy, wc, hc, (0, 0, OW, OH))
                    assert np.array_equal(got, want), (uh, uv, fancy, wc, hc, OW, OH)
                    l, t = OW // 2, OH // 2                             # a rectangle that starts inside, at either parity over the sizes
                    assert np.array_equal(rule(lib, plane, wc + 3, 0, uh, uv, fancy, wc, hc, (l, t, OW, OH)), want[t:, l:])


def test_rule_refuses(lib):
    p, o = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    f = lib.aej_test_jpeg_upsample_host
    assert f(p.ctypes.data, 8, 0, 2, 2, 1, 4, 4, 0, 0, 8, 8, o.ctypes.data) == 0
    assert f(None, 8, 0, 2, 2, 1, 4, 4, 0, 0, 8, 8, o.ctypes.data) == -1
    assert f(p.ctypes.data, 8, 0, 2, 2, 1, 4, 4, 0, 0, 8, 8, None) == -1
    for uh, uv in ((0, 1), (3, 1), (4, 2), (1, 0), (1, 3), (2, 4), (-1, 1)):
        assert f(p.ctypes.data, 8, 0, uh, uv, 1, 2, 2, 0, 0, 1, 1, o.ctypes.data) == -1, (uh, uv)
    assert f(p.ctypes.data, 8, 0, 2, 2, 0, 4, 4, 0, 0, 8, 8, o.ctypes.data) == -1      # 2 x 2 without fancy: no decoder uses it
    assert not o.any()


def _plan(hs, vs, s):
    """libjpeg at scale s for luma factors hs x vs over 1 x 1 chroma: the chroma IDCT size nc and what is left to up-sample.  2 x 2 at a
    scale: an IDCT twice the luma's brings the chroma to luma resolution; beside a 1 x 1 IDCT nothing is filtered."""
    m = 8 // s
    if s > 1 and (hs, vs) == (2, 2):
        return m, 2 * m, 1, 1, True
    return m, m, hs, vs, m > 1


def _some_boxes(ow, oh, rng):
    """every left edge with a few right edges, paired with every top edge with a few bottom edges"""
    cols = sorted({(l, r) for l in range(ow) for r in (l + 1, min(l + 2, ow), min(l + 17, ow), ow)})
    rows = sorted({(t, b) for t in range(oh) for b in (t + 1, min(t + 2, oh), min(t + 9, oh), oh)})
    n = max(len(cols), len(rows))
    ci, ri = rng.permutation(n) % len(cols), rng.permutation(n) % len(rows)
    return [(cols[i][0], rows[j][0], cols[i][1], rows[j][1]) for i, j in zip(ci, ri)]


@pytest.mark.parametrize("s", (1, 2, 4, 8))
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_window_holds_what_the_rule_reads(lib, layout, s):
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc
    _, hs, vs = layout
    m, nc, uh, uv, fancy = _plan(hs, vs, s)
    rng = np.random.default_rng(10 * s + hs + 3 * vs)
    box4, win = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    for W, H in ((41, 29), (5, 20)):
        ow, oh = -(-W // s), -(-H // s)
        wc, hc = -(-ow // uh), -(-oh // uv)
        mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
        d = JpegDecDesc()
        d.width, d.height, d.hs, d.vs, d.ncomp = W, H, hs, vs, 3
        # the chroma plane at this scale, whole MCUs; far from 127.5, so that 255 - v in the place of v changes every filtered value
        # (the smallest weight is 1 / 16, the smallest difference 55)
        stride = mcux * nc
        plane = rng.integers(0, 101, (mcuy * nc, stride), dtype=np.uint8)
        plane = np.where(rng.integers(0, 2, plane.shape) == 1, 255 - plane, plane).astype(np.uint8)
        want = reference(plane[:hc, :wc], uh, uv, fancy, oh, ow)
        for box in _some_boxes(ow, oh, rng):
            box4[:] = box
            assert lib.aej_jpegdec_sbox_window_host(ctypes.addressof(d), s, ctypes.addressof(box4), ctypes.addressof(win)) == 0, box
            mx0, my0, mx1, my1 = win
            buf = (255 - plane).astype(np.uint8)
            buf[my0 * nc:my1 * nc, mx0 * nc:mx1 * nc] = plane[my0 * nc:my1 * nc, mx0 * nc:mx1 * nc]
            off = my0 * nc * stride + mx0 * nc                          # the part starts at the window's first sample
            part = buf.reshape(-1)[off:]
            l, t, r, b = box
            got = rule(lib, part, stride, off, uh, uv, fancy, wc, hc, box)
            assert np.array_equal(got, want[t:b, l:r]), (layout, s, (W, H), box, tuple(win))
