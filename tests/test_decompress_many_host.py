"""CPU: the container framing parser and the header checks of Jpeg.decompress_many (no GPU calls)."""
import json
import os
import zlib

import numpy as np
import pytest

from adaptive_edge_aware_jpeg_amd.jpeg import HEADER_FIELDS, check_same_headers, parse_container
from conftest import GOLDEN

FIXTURES = sorted(f for f in os.listdir(GOLDEN) if f.endswith(".ajpg"))


def _reference_read(data):
    """What Jpeg._entropy_decode reads, without applying anything (jpeg.py:599-661)."""
    from io import BytesIO
    s = BytesIO(data)
    meta = json.loads(s.read(int.from_bytes(s.read(4), "big")).decode("utf-8"))
    out = []
    for _ in range(meta["num_layers"]):
        bits_len = int.from_bytes(s.read(4), "big")
        root = int.from_bytes(s.read(4), "big")
        packed = np.frombuffer(s.read((bits_len + 7) // 8), np.uint8)
        st = np.stack([(packed >> 6) & 3, (packed >> 4) & 3, (packed >> 2) & 3, packed & 3], 1).reshape(-1)[: bits_len // 2]
        clen = int.from_bytes(s.read(4), "big")
        out.append((st, root, s.read(clen)))
    return meta, out


@pytest.mark.parametrize("name", FIXTURES)
def test_parse_container_matches_the_reference_reader(name):
    data = open(os.path.join(GOLDEN, name), "rb").read()
    meta, layers = parse_container(data)
    ref_meta, ref = _reference_read(data)
    assert meta == ref_meta and len(layers) == 3
    for (n, root, packed, stream), (st, rroot, rstream) in zip(layers, ref):
        assert n == len(st) and root == rroot and bytes(stream) == rstream
        p = np.frombuffer(packed, np.uint8)
        got = np.stack([(p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3], 1).reshape(-1)[:n]
        assert np.array_equal(got, st)
        zlib.decompress(bytes(stream))


def test_parse_container_short_reads_like_the_reference():
    data = open(os.path.join(GOLDEN, FIXTURES[0]), "rb").read()
    for cut in (len(data) - 1, len(data) - 100, len(data) // 2):
        meta, layers = parse_container(data[:cut])
        _, ref = _reference_read(data[:cut])
        assert [(n, r, bytes(s)) for n, r, _, s in layers] == [(len(st), r, s) for st, r, s in ref]


def test_header_mismatch_and_empty_input():
    data = open(os.path.join(GOLDEN, FIXTURES[0]), "rb").read()
    meta, _ = parse_container(data)
    assert check_same_headers([meta, dict(meta)]) == meta
    for k in HEADER_FIELDS:
        other = dict(meta)
        other[k] = "x" if not isinstance(meta[k], str) else meta[k] + "x"
        with pytest.raises(ValueError, match=rf"file 2 .*{k}"):
            check_same_headers([meta, meta, other])
    with pytest.raises(ValueError):
        check_same_headers([dict(meta, num_layers=2)])


def test_decompress_many_rejects_empty_and_mixed_without_a_gpu():
    import adaptive_edge_aware_jpeg_amd as A
    codec = A.Jpeg.__new__(A.Jpeg)          # the checks come before any device work
    with pytest.raises(ValueError):
        codec.decompress_many([])
    with pytest.raises(ValueError):
        codec.decompress_many([b"\x00"], entropy="cpu")
    a = open(os.path.join(GOLDEN, FIXTURES[0]), "rb").read()
    b = next(open(os.path.join(GOLDEN, f), "rb").read() for f in FIXTURES[1:]
             if parse_container(open(os.path.join(GOLDEN, f), "rb").read())[0] != parse_container(a)[0])
    with pytest.raises(ValueError, match="file 1"):
        codec.decompress_many([a, b])
