"""CPU: what the baseline entropy decoder (csrc/jpegdec_core.h, jd_run / jd_symbol, stepped through on the host by
aej_test_jpegdec_coefs_host) says of a restart segment that ends inside a symbol must not depend on the bytes that follow the segment
in memory.  The un-stuffed segments of a scan lie back to back, so the bytes behind a cut segment are the next segment's: here that
segment is replaced by 0x00 bytes, by 0xFF data bytes (the all-ones prefix no Huffman table assigns) and by 0x55 bytes, for every
length every segment can be cut to, and the status is AEJ_JPEGDEC_TRUNCATED every time -- the text the Python layer raises with."""
import ctypes
import io

import numpy as np
import pytest

TRUNCATED = 1                                                       # AEJ_JPEGDEC_TRUNCATED (include/aej.h)
BEHIND = {"0x00": b"\x00" * 8, "0xFF": b"\xff\x00" * 8, "0x55": b"\x55" * 8}      # (a data byte 0xFF is stuffed in the file)


@pytest.fixture(scope="module")
def SJ():
    from adaptive_edge_aware_jpeg_amd import standard_jpeg
    return standard_jpeg


@pytest.fixture(scope="module")
def lib():
    from adaptive_edge_aware_jpeg_amd._lib import load_library
    return load_library()


def _file(subsampling):
    from PIL import Image
    x = np.random.default_rng(7).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, "JPEG", quality=90, subsampling=subsampling, restart_marker_blocks=1)
    return buf.getvalue()


def _scan_segments(scan):
    """the scan's bytes between its RSTn markers (stuffed, as in the file) and what follows the last one (EOI)"""
    cuts = [i for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    eoi = scan.rindex(b"\xff\xd9")
    starts = [0] + [c + 2 for c in cuts]
    ends = cuts + [eoi]
    return [scan[a:b] for a, b in zip(starts, ends)], scan[eoi:]


def _decode(SJ, lib, data):
    d = SJ.parse_header(data)
    nb = d.mcux * d.mcuy * d.blocks_per_mcu
    out = np.zeros((nb, 64), np.int16)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    return lib.aej_test_jpegdec_coefs_host(ctypes.addressof(d), ctypes.addressof(buf), len(data), out.ctypes.data, nb)


@pytest.mark.parametrize("subsampling", ["4:4:4", "4:2:0"])
def test_a_cut_segment_is_truncated_whatever_follows_it(SJ, lib, subsampling):
    from adaptive_edge_aware_jpeg_amd._lib import JPEGDEC_STATUS
    assert JPEGDEC_STATUS[TRUNCATED] == "truncated scan (it ends before the last MCU)"
    data = _file(subsampling)
    d = SJ.parse_header(data)
    assert d.restart_interval == 1 and d.n_segments >= 6
    head, scan = data[:d.scan_offset], data[d.scan_offset:]
    segs, tail = _scan_segments(scan)
    assert len(segs) == d.n_segments and _decode(SJ, lib, data) == 0
    seen = {k: [] for k in BEHIND}
    for i in range(len(segs) - 1):                                  # segment i keeps its first `cut` bytes, segment i + 1 becomes `behind`
        for cut in range(len(segs[i])):
            if cut and segs[i][cut - 1] == 0xFF:
                continue                                            # (that would split a stuffed byte from its zero)
            for k, behind in BEHIND.items():
                parts = segs[:i] + [segs[i][:cut], behind] + segs[i + 2:]
                body = b"".join(p + bytes([0xFF, 0xD0 + (j & 7)]) for j, p in enumerate(parts[:-1])) + parts[-1] + tail
                seen[k].append((i, cut, _decode(SJ, lib, head + body)))
    assert len(seen["0xFF"]) > 200
    for k in BEHIND:
        wrong = [c for c in seen[k] if c[2] != TRUNCATED]
        assert wrong == [], f"behind {k} bytes: (segment, bytes left, status) {wrong[:6]}"
