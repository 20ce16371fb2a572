"""CPU: conforming JPEG streams that no libjpeg encoder writes (tests/jpeg_stream_catalogue.py, built by tests/jpeg_stream_writer.py)
without a device.  Every case of the catalogue is decoded by live Pillow and the tests' Python reference must equal it, at every
scale; the library's two marker parsers must accept every case and derive the Huffman decode tables of T.81 C.2; the library's
per-thread entropy decoders, stepped through on the host (aej_test_jpegdec_coefs_host, aej_test_jpegprog_coefs_host), must give the
reference's coefficients; and a ladder of one-block files measures where "identical to Pillow" ends."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import jfif_reference as J
import jpeg_stream_catalogue as C
import jpeg_stream_writer as Wr
import progressive_reference as P
import scaled_decode_reference as R

CASES = C.catalogue()
BASELINE = [c for c in CASES if not c.progressive]
PROGRESSIVE = [c for c in CASES if c.progressive]


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


def _pillow(data, scale=1, mode="RGB"):
    import jpeg_luma_reference as LR
    im = LR.draft(data, "L" if mode == "L" else None, scale)
    return np.asarray(im if mode == "L" else im.convert("RGB"))


# ---- the writer's tables are what it says -----------------------------------------------------------------------------------------------
def test_table_builders():
    assert Wr.codes(Wr.chain([5, 6, 7])) == {5: (0b0, 1), 6: (0b10, 2), 7: (0b110, 3)}
    assert Wr.codes(Wr.single(9)) == {9: (0, 1)}
    lt = Wr.codes(Wr.long_tail(Wr.AC_SYMBOLS, C.HOT))
    assert sorted(n for _, n in lt.values()) == list(range(1, 9)) + [16] * 154 and all(lt[s][1] == 16 for s in C.HOT)
    assert lt[0xF0] == (0xFF00 + 153, 16)                          # the last code, below the unused all-ones
    f16 = Wr.codes(Wr.flat16(Wr.DC_SYMBOLS))
    assert [f16[s] for s in Wr.DC_SYMBOLS] == [(k, 16) for k in range(12)]
    assert min(n for _, n in Wr.codes(Wr.from_length(Wr.AC_SYMBOLS, 3)).values()) == 3
    edge = sorted(n for _, n in Wr.codes(Wr.lut_edge(Wr.AC_SYMBOLS)).values())
    assert 9 in edge and 10 in edge
    assert len(Wr.long_tail(Wr.AC_SYMBOLS + [s for s in range(256) if s not in Wr.AC_SYMBOLS], C.HOT)[1]) == 256
    for bad in ([1, 1], [1, 2, 2], [2, 2, 2, 2]):
        with pytest.raises(AssertionError):
            Wr.lengths(range(len(bad)), bad)


def test_chunk_placements_lie_where_they_should():
    for progressive in (False, True):
        for name, data, check in C.placements(progressive):
            check(data)


# ---- every case against live Pillow -------------------------------------------------------------------------------------------------------
def test_catalogue_covers_the_issue():
    names = {c.name.split("/")[0] for c in CASES}
    assert names == {"never", "segments", "stray", "chunk", "shapes", "uniform", "selectors", "reach", "pq1", "eobrun", "refine"}
    assert {c.layout for c in CASES} == set(C.LAYOUTS) and len(PROGRESSIVE) >= 40 and len(BASELINE) >= 100


@pytest.mark.parametrize("part", range(8))
def test_every_case_equals_pillow(part):
    """no case is skipped: the eight parts tile the catalogue.  Scale 1 for every case; every scale and the luma plane for the 16-bit
    tables and a rotating share of the rest"""
    seen = 0
    for k, c in enumerate(CASES):
        if k % 8 != part:
            continue
        seen += 1
        want = _pillow(c.data)
        assert np.array_equal(C.reference(c.data), want), c.name
        if "pq1" in c.tags or "reach" in c.tags or (k // 8) % 3 == 0:
            if "large" in c.tags:
                continue
            for s in (2, 4, 8):
                assert np.array_equal(C.reference(c.data, s), _pillow(c.data, s)), (c.name, s)
            s = (1, 2, 4, 8)[(k // 8) % 4]
            assert np.array_equal(C.reference(c.data, s, "L"), _pillow(c.data, s, "L")), (c.name, s, "L")
    assert seen == len(range(part, len(CASES), 8))


def test_reach_cases_reach():
    """the coefficient-reach files hold what they are for: DC category 11, AC category 10, coefficient 63 behind three ZRL"""
    for name in ("reach/checker/grey", "reach/checker-t/grey"):
        (c,) = [c for c in CASES if c.name == name]
        (coef,) = R.baseline_coefficients(c.data)
        dc = coef[..., 0].reshape(-1)                              # raster order: the order of a one-component scan
        assert np.abs(np.diff(dc)).max() >= 1024 and np.abs(coef[..., 1:]).max() >= 512, name
    (c,) = [c for c in CASES if c.name == "reach/ends/grey"]
    coef = R.baseline_coefficients(c.data)[0]
    assert (coef[..., 63] != 0).any() and ((coef[..., 1:63] == 0).all(-1) & (coef[..., 63] != 0)).any()


# ---- the library's parsers ------------------------------------------------------------------------------------------------------------------
def _derive(counts, symbols):
    """T.81 C.2 / F.2.2.3 in plain Python: (lut, maxcode, valoff) as aej_jpegdec_huff holds them"""
    lut, maxcode, valoff, code, k = [0] * 512, [0] + [-1] * 17, [0] * 18, 0, 0
    for length in range(1, 17):
        if counts[length - 1]:
            valoff[length] = k - code
        for _ in range(counts[length - 1]):
            if length <= 9:
                for e in range(1 << (9 - length)):
                    lut[(code << (9 - length)) + e] = (length << 8) | symbols[k]
            maxcode[length] = code
            code += 1
            k += 1
        code <<= 1
    return lut, maxcode, valoff


def _same_table(h, table):
    lut, maxcode, valoff = _derive(*table)
    assert list(h.lut) == lut
    assert list(h.maxcode)[1:] == maxcode[1:]
    for length in range(1, 17):
        if table[0][length - 1]:
            assert h.valoff[length] == valoff[length], length
    assert bytes(h.vals)[:len(table[1])] == bytes(table[1])


@pytest.mark.parametrize("part", range(4))
def test_baseline_parser_reads_every_case(SJ, part):
    for c in BASELINE[part::4]:
        d = SJ.parse_header(c.data, layout_440=True)
        frame, (sc,) = P.walk(c.data)
        assert (d.width, d.height, d.ncomp, d.sof) == (frame["width"], frame["height"], len(frame["comps"]), frame["sof"]), c.name
        assert d.restart_interval == sc["ri"] and (d.scan_offset, d.scan_offset + d.scan_length) == (sc["start"], len(c.data))
        assert d.precision16 == ("pq1" in c.tags)
        mx, my, geo = P._geometry(frame)
        assert (d.mcux, d.mcuy, d.hs, d.vs) == (mx, my, geo[0]["h"], geo[0]["v"])
        assert d.n_segments == (-(-mx * my // sc["ri"]) if sc["ri"] else 1)
        for i, (ci, td, ta) in enumerate(sc["comps"]):
            assert ci == i and d.comp_id[i] == frame["comps"][i]["id"] and d.comp_tq[i] == frame["comps"][i]["tq"]
            assert list(d.qt[i]) == sc["qts"][i], (c.name, i)
            _same_table(d.dc[i], sc["dc"][td])
            _same_table(d.ac[i], sc["ac"][ta])


@pytest.mark.parametrize("part", range(4))
def test_progressive_parser_reads_every_case(SJ, part):
    for c in PROGRESSIVE[part::4]:
        frame, scans = SJ.parse_scans(c.data, layout_440=True)
        rframe, rscans = P.walk(c.data)
        assert (frame.width, frame.height, frame.ncomp, frame.n_scans) == (rframe["width"], rframe["height"], len(rframe["comps"]), len(rscans)), c.name
        assert frame.precision16 == ("pq1" in c.tags)
        for s, r in zip(scans, rscans):
            assert [(s.comp[i], s.td[i], s.ta[i]) for i in range(s.ncomp)] == r["comps"], c.name
            assert (s.ss, s.se, s.ah, s.al, s.restart_interval) == (r["ss"], r["se"], r["ah"], r["al"], r["ri"])
            end = s.data_offset + s.data_length                       # fill bytes in front of the next marker may count as the scan's
            assert s.data_offset == r["start"] and r["end"] <= end and c.data[r["end"]:end + 1] == b"\xff" * (end + 1 - r["end"]), c.name
            assert c.data[end + 1] not in (0x00, 0xFF) and not 0xD0 <= c.data[end + 1] <= 0xD7
            if s.ss == 0 and s.ah == 0:
                for i in range(s.ncomp):
                    _same_table(s.dc[i], r["dc"][s.td[i]])
            if s.ss > 0:
                _same_table(s.ac, r["ac"][s.ta[0]])
        for i in range(frame.ncomp):
            assert list(frame.qt[i]) == next(r["qts"][i] for r in rscans if i in r["qts"])


# ---- the library's entropy decoders, stepped through on the host -------------------------------------------------------------------------
def _host_baseline(SJ, lib, data):
    d = SJ.parse_header(data, layout_440=True)
    nb = d.mcux * d.mcuy * d.blocks_per_mcu
    out = np.full((nb + 1, 64), 0x5A5A, np.int16)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    rc = lib.aej_test_jpegdec_coefs_host(ctypes.addressof(d), ctypes.addressof(buf), len(data), out.ctypes.data, nb)
    assert (out[nb] == 0x5A5A).all()
    return rc, out[:nb]


@pytest.mark.parametrize("part", range(4))
def test_host_stepped_baseline_decode_equals_the_reference(SJ, lib, part):
    """jd_byte_class, jd_huff and jd_run -- the functions the kernels call -- on every baseline case"""
    for c in BASELINE[part::4]:
        rc, got = _host_baseline(SJ, lib, c.data)
        assert rc == 0, c.name
        assert np.array_equal(got, P.mcu_order(c.data, R.baseline_coefficients(c.data))), c.name


@pytest.mark.parametrize("part", range(4))
def test_host_stepped_progressive_decode_equals_the_reference(SJ, lib, part):
    from adaptive_edge_aware_jpeg_amd import _lib
    for c in PROGRESSIVE[part::4]:
        frame, scans = SJ.parse_scans(c.data, layout_440=True)
        arr = (_lib.JpegProgScan * len(scans))(*scans)
        nb = frame.mcux * frame.mcuy * frame.blocks_per_mcu
        out = np.zeros((nb, 64), np.int16)
        buf = (ctypes.c_uint8 * len(c.data)).from_buffer_copy(c.data)
        assert lib.aej_test_jpegprog_coefs_host(ctypes.addressof(frame), ctypes.addressof(arr), ctypes.addressof(buf), len(c.data), 1 << 30,
                                                out.ctypes.data, nb) == 0, c.name
        assert np.array_equal(out, P.mcu_order(c.data, P.coefficients(c.data))), c.name


def test_host_entry_refuses(lib):
    from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc
    d, out = JpegDecDesc(), np.zeros((4, 64), np.int16)
    buf = (ctypes.c_uint8 * 16)()
    assert lib.aej_test_jpegdec_coefs_host(None, ctypes.addressof(buf), 16, out.ctypes.data, 4) == -1
    assert lib.aej_test_jpegdec_coefs_host(ctypes.addressof(d), ctypes.addressof(buf), 16, out.ctypes.data, 4) == -1      # an unwritten descriptor


# ---- refusals: what the decoders do not take, and what Pillow does with it -------------------------------------------------------------------
def test_refusals_on_the_host(SJ, lib):
    from adaptive_edge_aware_jpeg_amd._lib import JPEGDEC_STATUS
    files = C.refusal_files()
    for name, (data, pillow_decodes) in files.items():
        try:
            Image.open(io.BytesIO(data)).convert("RGB")
            decoded = True
        except OSError:
            decoded = False
        assert decoded == pillow_decodes, name
    rc, _ = _host_baseline(SJ, lib, files["dc12"][0])              # the parser takes the table; the decode refuses the symbol when it is used
    assert "DC" in JPEGDEC_STATUS[rc], JPEGDEC_STATUS[rc]
    with pytest.raises(ValueError, match="DC Huffman symbol above 15"):
        SJ.parse_header(files["dc16"][0])
    with pytest.raises(ValueError, match="over-subscribed"):
        SJ.parse_header(files["all-ones"][0])


# ---- the ladder: where "identical to Pillow" ends ---------------------------------------------------------------------------------------------
# One grey 8 x 8 file per rung, one term under a 16-bit quantiser.  amp: the term's largest contribution to a sample (before the +128).
LADDER = [(term, sign * prod) for term in (0, 1) for prod in (800, 2000, 2800, 4000, 4100, 6000, 8200, 20000, 32000, 40000, 65535)
          for sign in (1, -1)]


def _ladder_file(term, product):
    b = np.zeros((1, 1, 64), np.int64)
    b[0, 0, term] = 1 if product > 0 else -1
    qt = np.ones(64, np.int64)
    qt[J.ZIGZAG[term]] = abs(product)
    return Wr.write(8, 8, [(1, 1, b)], qtables=[(qt, 1)], selectors=[(0, 0, 0)]), b, qt


def _exact_samples(b, qt):
    """the islow IDCT's output in unbounded integers, before any range limit"""
    nat = np.zeros(64, np.int64)
    nat[J.ZIGZAG] = b.reshape(64)
    d = (nat * qt).reshape(8, 8)
    ws = np.swapaxes(J._idct_1d(np.swapaxes(d, -1, -2), True), -1, -2)
    return J._idct_1d(ws, False)


def test_ladder():
    """Measured with Pillow 12.2.0 / libjpeg-turbo 3.1.4.1 on x86-64: the C-semantics reference (and with it jd_range_limit and the
    kernels) equals Pillow on every rung whose exact IDCT output stays in [-512, 511]; on every rung outside, Pillow equals the
    SIMD-semantics reference (saturation) and not the C one (the masked table wraps) -- except where both happen to give the same pixels.
    Asserted: the rungs inside the boundary against Pillow, and that the ladder has rungs on both sides of +-128, +-512 and of the int16
    limit of the dequantised product.  The rungs outside are recorded (printed), not asserted."""
    record, spans = [], set()
    for term, product in LADDER:
        data, b, qt = _ladder_file(term, product)
        x = _exact_samples(b, qt)
        inside = -512 <= x.min() and x.max() <= 511
        pil = _pillow(data, 1, "L")
        c_equal = np.array_equal(R.decode(data, 1, "L"), pil)
        simd_equal = np.array_equal(R.decode(data, 1, "L", simd=True), pil)
        record.append((term, product, int(x.min()), int(x.max()), inside, c_equal, simd_equal))
        print("ladder term %d product %6d samples %6d..%6d inside %d  Pillow == C %d  Pillow == SIMD %d" % record[-1])
        spans.add((np.abs(x).max() > 128, np.abs(x).max() > 512, abs(product) > 32767))
        if inside:
            assert c_equal and simd_equal, record[-1]
    assert spans >= {(False, False, False), (True, False, False), (True, True, False), (True, True, True)}
    assert sum(r[4] for r in record) >= 8 and sum(not r[4] for r in record) >= 8
