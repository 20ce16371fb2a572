"""Record what the two JPEG marker parsers (aej_jpegdec_parse_host, aej_jpegprog_parse_host) answer for a deterministic corpus of
valid, cut, corrupted and hand-made files -> tests/golden/jpegparse/pins.json.  tests/test_jpeg_parse_pins.py rebuilds the corpus
with corpus() and compares case by case with parse_case(), so a change of the parsers that is meant to keep their behaviour can be
checked on a machine without a GPU (both entries are host code).

    python tools/record_jpeg_parse_pins.py            # run at the commit whose behaviour is to be kept

The corpus, for every committed .jpg under tests/golden/{jpegdec,jpegprog,jfif,jfif_options,jfif_progressive}:
  the file itself; the file cut at every marker boundary before the first scan, one byte later and one byte into the segment's
  payload; MUTATIONS single-byte replacements, position and value from numpy.random.default_rng(SEED), before the end of the last
  SOS segment (of an SOF2 file: anywhere up to EOI) -- every other one anywhere in that region with any value, the rest on a marker
  code, a length or the first payload bytes of a segment, half of those with a value that is itself a marker code, so that the
  structural refusals are met and not only table contents change; and once the hand-made refusals of tests/test_jpegdec_host.py
  and tests/test_jpegprog_host.py.  Every case goes through both parsers, whichever kind of file it is."""
import ctypes
import glob
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden")
PINS = os.path.join(GOLDEN, "jpegparse", "pins.json")
FOLDERS = ("jpegdec", "jpegprog", "jfif", "jfif_options", "jfif_progressive")
SEED = 20261017
MUTATIONS = 32           # per file: 59 files and their cuts keep the fixture near 250 KiB
MARKER_CODES = bytes([0x00, 0x01, 0xFF, 0xD0, 0xD8, 0xD9, 0xDA, 0xDB, 0xDC, 0xDD, 0xE0, 0xEE, 0xFE]) + bytes(range(0xC0, 0xD0))


def _segment_starts(data):
    """(offsets of the markers SOI+2 .. first SOS, end of the last SOS segment, whether the frame is SOF2, the structural bytes:
    marker code, length and up to 12 payload bytes of each of those segments and of every later SOS)"""
    starts, p, last_sos_end, sof2, heads = [], 2, 0, False, []
    while p + 4 <= len(data) and data[p] == 0xFF:
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        starts.append(p)
        heads += range(p + 1, min(p + 16, p + 2 + n))
        sof2 |= m == 0xC2
        p += 2 + n
        if m == 0xDA:
            break
    q = 0
    while True:                                  # the last FF DA of the file (an entropy-coded FF is followed by 00 or RSTn)
        q = data.find(b"\xff\xda", q)
        if q < 0:
            break
        last_sos_end = q + 2 + int.from_bytes(data[q + 2:q + 4], "big")
        heads += range(q + 1, min(last_sos_end, len(data)))
        q += 2
    return starts, last_sos_end, sof2, sorted(set(heads))


def corpus():
    """[(case name, bytes)], the same list on every run"""
    import test_jpegdec_host as TB
    import test_jpegprog_host as TP
    rng = np.random.default_rng(SEED)
    cases = []
    for folder in FOLDERS:
        for path in sorted(glob.glob(os.path.join(GOLDEN, folder, "*.jpg"))):
            with open(path, "rb") as f:
                data = f.read()
            name = folder + "/" + os.path.basename(path)[:-4]
            cases.append((name, data))
            starts, sos_end, sof2, heads = _segment_starts(data)
            for p in starts:
                for cut in (p, p + 1, p + 5):
                    cases.append((f"{name} cut at {cut}", data[:cut]))
            region = len(data) if sof2 else sos_end
            heads = [h for h in heads if h < region]
            for k in range(MUTATIONS):
                pos = int(rng.integers(0, region)) if k % 2 == 0 else heads[int(rng.integers(0, len(heads)))]
                val = (data[pos] + 1 + int(rng.integers(0, 255))) & 255      # never the byte that is there
                if k % 4 == 3:
                    val = [v for v in MARKER_CODES if v != data[pos]][int(rng.integers(0, len(MARKER_CODES) - 1))]
                cases.append((f"{name} byte {pos} = {val:02X}", data[:pos] + bytes([val]) + data[pos + 1:]))
    for label, made in (("baseline unsupported", TB._unsupported_files()), ("baseline malformed", TB._malformed_files()),
                        ("progressive malformed", TP._malformed(None)), ("progressive unsupported", TP._unsupported(None))):
        cases += [(f"{label}: {kind}", data) for kind, data in made.items()]
    return cases


def parse_case(lib, L, data):
    """-> the record of one case: baseline (rc, message, SHA-256 of the descriptor), progressive count query (rc, message, SHA-256 of
    the frame), progressive full call (rc, message, SHA-256 of the frame and all scan structs; None when the query failed), n_scans"""
    buf = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    d, msg = L.JpegDecDesc(), ctypes.create_string_buffer(256)
    rc = lib.aej_jpegdec_parse_host(ctypes.addressof(buf), len(data), ctypes.addressof(d), ctypes.addressof(msg), 256)
    rec = [int(rc), msg.value.decode("latin-1"), hashlib.sha256(bytes(d)).hexdigest()]
    frame, msg = L.JpegProgFrame(), ctypes.create_string_buffer(256)
    rc = lib.aej_jpegprog_parse_host(ctypes.addressof(buf), len(data), ctypes.addressof(frame), None, 0, ctypes.addressof(msg), 256)
    rec += [int(rc), msg.value.decode("latin-1"), hashlib.sha256(bytes(frame)).hexdigest()]
    n_scans = int(frame.n_scans)
    if rc == 0:
        scans, msg = (L.JpegProgScan * n_scans)(), ctypes.create_string_buffer(256)
        rc = lib.aej_jpegprog_parse_host(ctypes.addressof(buf), len(data), ctypes.addressof(frame), ctypes.addressof(scans), n_scans,
                                         ctypes.addressof(msg), 256)
        rec += [int(rc), msg.value.decode("latin-1"), hashlib.sha256(bytes(frame) + bytes(scans)).hexdigest()]
    else:
        rec += [None, None, None]
    return rec + [n_scans]


def record():
    """every case's record, with the strings (messages, digests) kept once in a table and referred to by index"""
    from adaptive_edge_aware_jpeg_amd import _lib as L
    lib = L.load_library()
    table, index, rows = [], {}, []

    def ref(s):
        if s not in index:
            index[s] = len(table)
            table.append(s)
        return index[s]
    messages = set()
    for name, data in corpus():
        rec = parse_case(lib, L, data)
        messages.update(m for m in (rec[1], rec[4], rec[7]) if m)
        rows.append([hashlib.sha256(data).hexdigest()[:12]] + [ref(v) if isinstance(v, str) else v for v in rec])
    return {"seed": SEED, "mutations_per_file": MUTATIONS, "n_cases": len(rows), "n_messages": len(messages),
            "messages": sorted(messages), "strings": table, "cases": rows}


if __name__ == "__main__":
    pins = record()
    os.makedirs(os.path.dirname(PINS), exist_ok=True)
    with open(PINS, "w") as f:
        json.dump(pins, f, separators=(",", ":"))
        f.write("\n")
    print("\n".join(pins["messages"]))
    print(f"{pins['n_cases']} cases, {pins['n_messages']} distinct messages, {os.path.getsize(PINS)} bytes -> {PINS}")
