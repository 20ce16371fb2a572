"""GPU: the baseline entropy kernels of csrc/jfif.hip against the host entry that steps through the same text
(aej_test_jfif_seq_scan_host), on the coefficient sets of tests/jfif_seq_cases.py -- blocks no pixels produce, so the Pillow suites
never reach them.  The sets go in as conforming baseline files (tests/jpeg_stream_writer.py) through the lossless transcoder, which
entropy-codes the very coefficients again under the file's own tables, without and with a restart interval of one MCU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_restart_reference as RR  # noqa: E402
import jfif_seq_cases as C  # noqa: E402
import jpeg_stream_writer as W  # noqa: E402

pytestmark = pytest.mark.gpu


def _dht(cls_id, bits, vals):
    body = bytes([cls_id]) + bytes(bits) + bytes(vals)
    return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body


def test_kernels_equal_the_host_entry_on_blocks_pixels_never_give():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as A
    from adaptive_edge_aware_jpeg_amd import standard_jpeg as S
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    lib = load_library()
    cases = [(layout, name, coef) for layout in ("grey", "4:2:0") for name, coef in C.sets(layout)]
    files = [W.write(*C.LAYOUTS[layout][3:], C.writer_comps(coef, layout)) for layout, _, coef in cases]
    for R, kw in ((0, {}), (1, dict(restart_marker_blocks=1))):
        out = A.standard_jpeg_transcode_many(files, grey=True, **kw)
        assert len(out) == len(cases)
        for (layout, name, coef), o in zip(cases, out):
            rc, data, hist, _ = C.scan_host(lib, coef, layout, R, 1)
            assert rc == 0
            segs = RR.walk(o)
            (sos,) = [(a, b) for m, a, b in segs if m == 0xDA]
            hdr = 2 + int.from_bytes(o[sos[0] + 2:sos[0] + 4], "big")
            assert o[sos[0] + hdr:sos[1]] == data and o[sos[1]:] == b"\xff\xd9", (layout, name, R)
            ids = [0x00, 0x10] if layout == "grey" else [0x00, 0x10, 0x01, 0x11]
            assert [o[a:b] for m, a, b in segs if m == 0xC4] == [_dht(i, *S.huffman_table(hist[t])) for t, i in enumerate(ids)], (layout, name, R)
            assert (RR.dri_sequence(o), len(RR.markers(o)[0])) == ([1 if R else None], C.blocks_of(layout) // (1 if layout == "grey" else 6) - 1 if R else 0)
