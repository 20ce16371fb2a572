"""GPU: Jpeg.decompress_many (aej_inflate_batch + aej_decode_headers) against Jpeg.decompress, the oracle and zlib."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN
from inflate_helpers import BitWriter, rebuild, run_inflate, zhdr

pytestmark = pytest.mark.gpu

FIXTURES = sorted(f[:-5] for f in os.listdir(GOLDEN) if f.endswith(".ajpg"))
ROUNDTRIP = [("YCbCr", 256, 384, (4, 64)), ("OKLAB", 250, 332, (4, 128)), ("ICtCp", 128, 256, (4, 32)), ("ICaCb", 96, 128, (4, 16)),
             ("JzAzBz", 120, 200, (8, 64)), ("YCoCg", 101, 67, (4, 32)), ("YCoCg-R", 33, 35, (2, 16)), ("YCbCr", 1080, 1920, (4, 64))]


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(A):
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    return get_context()


def synth(oracle, H, W, seed):
    return oracle.synth_image(H, W, seed).astype(np.float32) / np.float32(255.0)


def codec(A):
    return A.Jpeg(A.JpegCompressionSettings())


# ---------------------------------------------------------------------------------------------------------------- whole files
def test_reference_fixtures(A, oracle):
    meta = json.load(open(os.path.join(GOLDEN, "decode_cases.json")))
    for name in FIXTURES:
        data = open(os.path.join(GOLDEN, name + ".ajpg"), "rb").read()
        want = codec(A).decompress(data).data
        assert np.array_equal(want, oracle.decode_image(data))
        for entropy in ("gpu", "host"):
            one = codec(A).decompress_many([data], entropy=entropy).cpu().numpy()
            three = codec(A).decompress_many([data] * 3, entropy=entropy).cpu().numpy()
            assert one.shape == (1,) + want.shape and np.array_equal(one[0], want), (name, entropy)
            for b in range(3):
                assert np.array_equal(three[b], want), (name, entropy, b)
            if name in meta:
                assert hashlib.sha256(np.ascontiguousarray(one[0]).tobytes()).hexdigest() == meta[name]["sha256"]


@pytest.mark.parametrize("case", range(len(ROUNDTRIP)), ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in ROUNDTRIP])
def test_round_trip_every_writer(A, oracle, case):
    space, H, W, br = ROUNDTRIP[case]
    B = 1 + case % 4
    x = np.stack([synth(oracle, H, W, 300 + case * 7 + b) for b in range(B)])
    c = A.Jpeg(A.JpegCompressionSettings(space, (40, 80), br))
    want = c.decompress_batch(c.compress_batch(x)).cpu().numpy()
    modes = [dict(entropy="host", zlib_level=lv) for lv in (0, 1, 6, 9)] + [dict(entropy="gpu"), dict(entropy="gpu-fixed")]
    if H * W > 1_000_000:
        modes = [dict(entropy="host", zlib_level=1), dict(entropy="gpu"), dict(entropy="gpu-fixed")]
    for m in modes:
        files = c.compress_many(x, extension=".png", **m)
        for entropy in ("gpu", "host"):
            got = A.Jpeg(A.JpegCompressionSettings()).decompress_many(files, entropy=entropy).cpu().numpy()
            assert np.array_equal(got, want), (m, entropy)


def test_full_size_natural_tiles(A):
    import torch
    from tools.benchlib.data import natural_batch
    x = natural_batch(torch, 8, 2160, 3840, 5, torch.device("cuda", 0)).cpu().numpy()
    c = A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), (4, 64)))
    for kind in ("host", "gpu"):
        files = c.compress_many(x, extension=".png", entropy=kind)
        want = np.stack([A.Jpeg(A.JpegCompressionSettings()).decompress(f).data for f in files])
        for entropy in ("gpu", "host"):
            got = A.Jpeg(A.JpegCompressionSettings()).decompress_many(files, entropy=entropy).cpu().numpy()
            assert np.array_equal(got, want), (kind, entropy)


def test_mixed_headers_and_empty(A):
    a = open(os.path.join(GOLDEN, FIXTURES[0] + ".ajpg"), "rb").read()
    b = open(os.path.join(GOLDEN, FIXTURES[1] + ".ajpg"), "rb").read()
    with pytest.raises(ValueError, match="file 1"):
        codec(A).decompress_many([a, b])
    with pytest.raises(ValueError):
        codec(A).decompress_many([])


# ---------------------------------------------------------------------------------------------------------------- inflate alone
def good_streams():
    rng = np.random.default_rng(7)
    raw = [rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), b"",
           (rng.integers(-3, 4, 40000).astype(np.int32)).tobytes(),
           bytes(70000), bytes(range(256)) * 300]
    x = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    raw.append(x + x + x[:258] + x)                 # matches at distance 32768, length 258
    out = []
    for r in raw:
        for level in (0, 1, 6, 9):
            out.append(zlib.compress(r, level))
        for strategy in (zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY, zlib.Z_FILTERED):
            co = zlib.compressobj(9, zlib.DEFLATED, 15, 9, strategy)
            out.append(co.compress(r) + co.flush())
    return out


def test_inflate_matches_zlib(A, ctx):
    streams = good_streams()
    outs, st, guards = run_inflate(A, ctx, streams)
    assert guards and not st.any(), st
    for s, o in zip(streams, outs):
        assert o == zlib.decompress(s)


def test_inflate_gpu_deflate_multi_megabyte_block(A, oracle, ctx):
    img = synth(oracle, 1080, 1920, 11)
    c = A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), (4, 64)))
    enc = c.compress_batch(img[None])
    streams = [bytes(s) for s in c.deflate_batch(enc)[0]] + [bytes(s) for s in c.deflate_batch(enc, adaptive=False)[0]]
    assert max(len(zlib.decompress(s)) for s in streams) > 2 << 20
    outs, st, guards = run_inflate(A, ctx, streams)
    assert guards and not st.any()
    for s, o in zip(streams, outs):
        assert o == zlib.decompress(s)


def corrupt_cases():
    good = zlib.compress(bytes(range(256)) * 40, 9)
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for _ in range(4): w.put(1, 3)                                  # four 1-bit codes: over-subscribed
    over = zhdr() + w.bytes() + bytes(8)
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4); w.put(1, 3); w.put(0, 3); w.put(0, 3); w.put(0, 3)
    incomplete = zhdr() + w.bytes() + bytes(8)
    w = BitWriter(); w.put(1, 1); w.put(1, 2); w.code(1, 7); w.put(0, 5); w.code(0, 7)     # length 3 at distance 1 before any output
    far = zhdr() + w.bytes() + bytes(4)
    w = BitWriter(); w.put(1, 1); w.put(3, 2)
    btype3 = zhdr() + w.bytes() + bytes(8)
    stored = zhdr(0x78) + bytes([1, 5, 0, 0, 0]) + b"hello" + bytes(4)
    adler = good[:-1] + bytes([good[-1] ^ 1])
    return [(b"\x79\x9c" + good[2:], 1), (good[:1] + bytes([good[1] ^ 1]) + good[2:], 1), (zhdr(fdict=1) + good[2:], 1),
            (btype3, 2), (over, 3), (incomplete, 3), (far, 5), (stored, 6), (good[:-5], 7), (b"", 7), (adler, 9)]


def test_inflate_corruption_statuses(A, ctx):
    good = good_streams()[:6]
    cases = corrupt_cases()
    streams, caps, want = [], [], []
    for i, (bad, code) in enumerate(cases):
        with pytest.raises(zlib.error):
            zlib.decompress(bad)
        streams += [good[i % len(good)], bad]
        caps += [len(zlib.decompress(good[i % len(good)])), 1 << 14]
        want += [0, code]
    big = zlib.compress(bytes(range(256)) * 64, 6)                 # 16 KiB into 10 000 bytes
    streams.append(big); caps.append(10000); want.append(8)
    outs, st, guards = run_inflate(A, ctx, streams, caps)
    assert guards
    assert list(st) == want, list(st)
    for i in range(0, len(cases) * 2, 2):
        assert outs[i] == zlib.decompress(streams[i])


# ---------------------------------------------------------------------------------------------------------------- corrupt files
def mutations(data):
    from adaptive_edge_aware_jpeg_amd.jpeg import parse_container
    mlen = int.from_bytes(data[:4], "big")
    head = data[:4 + mlen]
    _, layers = parse_container(data)
    base = [[2 * n, r, bytes(p), bytes(s)] for n, r, p, s in layers]

    def sym_set(packed, i, v):
        p = bytearray(packed)
        sh = 6 - 2 * (i % 4)
        p[i // 4] = (p[i // 4] & ~(3 << sh)) | (v << sh)
        return bytes(p)

    out = []
    for l in range(3):
        def with_(**kw):
            m = [list(x) for x in base]
            for k, v in kw.items():
                m[l][{"bits": 0, "root": 1, "packed": 2, "stream": 3}[k]] = v
            return rebuild(head, m)
        bits, root, packed, stream = base[l]
        n = bits // 2
        out += [with_(bits=bits - 2), with_(bits=bits + 8, packed=packed + b"\x00"), with_(bits=bits + 8, packed=packed + b"\x55"),
                with_(packed=sym_set(packed, 0, 3)), with_(packed=sym_set(packed, n // 2, 3)), with_(packed=sym_set(packed, n - 1, 1)),
                with_(root=root * 2), with_(root=root // 2), with_(root=root + 1), with_(packed=sym_set(packed, 0, 0)),
                with_(stream=zlib.compress(zlib.decompress(stream)[:-4])), with_(stream=zlib.compress(zlib.decompress(stream) + bytes(4))),
                with_(stream=stream[:-3])]
        for i in (1, n // 3, n // 2):
            for v in (0, 1, 2):
                out.append(with_(packed=sym_set(packed, i, v)))
    return out


def test_corrupt_files_raise_exactly_when_decompress_does(A):
    data = open(os.path.join(GOLDEN, "crop_ycbcr_4_64.ajpg"), "rb").read()
    raised = 0
    for k, bad in enumerate(mutations(data)):
        try:
            want = codec(A).decompress(bad).data
        except (ValueError, zlib.error):
            want = None
        for entropy in ("gpu", "host"):
            if want is None:
                with pytest.raises(ValueError):
                    codec(A).decompress_many([data, bad], entropy=entropy)
            else:
                got = codec(A).decompress_many([bad, data], entropy=entropy).cpu().numpy()
                assert np.array_equal(got[0], want), (k, entropy)
        raised += want is None
    assert raised >= 10
