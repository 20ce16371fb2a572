"""GPU: csrc/inflate.hip on the deflate stream catalogue (tests/deflate_stream_catalogue.py): conforming streams zlib never writes, and
malformed ones.  Every comparison is exact equality against tests/inflate_reference.py, which tests/test_inflate_streams_host.py has held
against ``zlib.decompress`` on the same bytes.  The gaps between the streams in the source buffer hold 0xFF, not the zeros the kernel
substitutes past the end of a stream: a read beyond ``in_len`` decodes garbage."""
import zlib

import numpy as np
import pytest

import deflate_stream_catalogue as C
import inflate_reference as R
import png_reference as P
from inflate_helpers import rebuild, run_inflate

pytestmark = pytest.mark.gpu
FILL = 0xFF


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


@pytest.fixture(scope="module")
def valid():
    """[(name, stream, payload)]: the catalogue, the reference's reading of every stream confirmed once, and two ordinary zlib streams
    placed among it"""
    out = []
    for c in C.catalogue():
        assert R.inflate(c.data) == (c.payload, R.OK), c.name
        out.append((c.name, c.data, c.payload))
    rng = np.random.default_rng(11)
    for k, raw in enumerate((bytes(range(256)) * 40, rng.integers(-3, 4, 9000).astype(np.int32).tobytes())):
        out.insert((k + 1) * len(out) // 3, (f"zlib/{k}", zlib.compress(raw, 6 + 3 * k), raw))
    return out


def first_difference(got, want):
    n = min(len(got), len(want))
    return next((i for i in range(n) if got[i] != want[i]), n), len(got), len(want)


@pytest.mark.parametrize("order", ("catalogue", "reversed"))
def test_valid_catalogue_in_one_launch(A, ctx, valid, order):
    """exact capacities, so that one byte too many is an error and one byte beyond lands in a guard"""
    cases = valid if order == "catalogue" else valid[::-1]
    outs, st, guards = run_inflate(A, ctx, [s for _, s, _ in cases], [len(p) for _, _, p in cases], fill=FILL)
    assert [(n, int(x)) for (n, _, _), x in zip(cases, st) if x] == []
    for (name, _, payload), got in zip(cases, outs):
        assert len(got) == len(payload) and got == payload, (name, first_difference(got, payload))
    assert guards


def test_capacity_one_byte_short(A, ctx, valid):
    """every stream into a slot one byte too small: OVER_CAPACITY, whole 256-byte pieces of the true payload stored and counted, nothing
    at or beyond the capacity (the guards begin there)"""
    cases = [c for c in valid if len(c[2]) >= 1]
    outs, st, guards = run_inflate(A, ctx, [s for _, s, _ in cases], [len(p) - 1 for _, _, p in cases], fill=FILL)
    assert [(n, int(x)) for (n, _, _), x in zip(cases, st) if x != R.OVER_CAPACITY] == []
    assert guards
    for (name, _, payload), got in zip(cases, outs):
        assert len(got) % 256 == 0 and len(got) < len(payload) and payload.startswith(got), (name, len(got))


def test_malformed_catalogue(A, ctx, valid):
    """each malformed stream between two good ones: its status as the reference gives it, the neighbours untouched"""
    good = [c for c in valid if 0 < len(c[2]) < 5000]
    streams, caps, want, names = [], [], [], []
    for k, b in enumerate(C.malformed()):
        assert R.inflate(b.data)[1] == b.status
        g = good[(7 * k) % len(good)]
        streams += [g[1], b.data]
        caps += [len(g[2]), 1 << 16]
        want += [0, b.status]
        names += [g[0], b.name]
    g = good[-1]
    streams.append(g[1]); caps.append(len(g[2])); want.append(0); names.append(g[0])
    outs, st, guards = run_inflate(A, ctx, streams, caps, fill=FILL)
    assert [(n, int(x), w) for n, x, w in zip(names, st, want) if x != w] == []
    assert guards
    by = {c[0]: c[2] for c in valid}
    for i in range(0, len(streams), 2):
        assert outs[i] == by[names[i]], names[i]
    for i in range(1, len(streams), 2):                   # what a refused stream had stored is a prefix of what the reference had decoded
        assert len(outs[i]) % 256 == 0 and R.inflate(streams[i])[0].startswith(outs[i]), names[i]


def test_every_strict_prefix_is_truncated(A, ctx):
    streams, caps, names, full = [], [], [], []
    for name in C.PREFIX_CASES:
        c = C.by_name(name)
        for n in range(len(c.data)):
            streams.append(c.data[:n]); caps.append(len(c.payload)); names.append((name, n)); full.append(c.payload)
    outs, st, guards = run_inflate(A, ctx, streams, caps, fill=FILL)
    assert [(n, int(x)) for n, x in zip(names, st) if x != R.TRUNCATED] == []
    assert guards
    for n, got, payload in zip(names, outs, full):
        assert len(got) % 256 == 0 and payload.startswith(got), n


# ---------------------------------------------------------------------------------------------------------------- through the callers
def _pictures():
    """(w, h, depth, colour type, samples, filters): 64 x 64 RGBA with periodic rows (overlapped matches of every odd period up to 63),
    noisy rows under every filter and rows of zeros (matches of 258); 13 x 7 RGB"""
    rng = np.random.default_rng(3)
    s = P.random_samples(rng, 64, 64, 8, 6)
    for y in range(32):
        unit = rng.integers(0, 256, 1 + 2 * y, dtype=np.uint8)
        s[y] = np.resize(unit, 256).reshape(64, 4)
    s[48:] = 0
    filters = [0] * 32 + [y % 5 for y in range(16)] + [0] * 16
    return [(64, 64, 8, 6, s, filters), (13, 7, 8, 2, P.random_samples(rng, 13, 7, 8, 2), P.PATTERNS["cycle"](7))]


def test_through_png_decode_many(A):
    """the writer's streams as the IDAT data of small files, split into chunks of 1, 3 and 5 bytes: inflate="gpu" against Pillow, the
    plain PNG reader and inflate="host" """
    import torch
    files, names = [], []
    for k, style in enumerate(sorted(C.STYLES)):
        for j, (w, h, depth, ct, samples, filters) in enumerate(_pictures()):
            split = (1, 3, 5)[(k + j) % 3]
            files.append(P.make_png(w, h, depth, ct, samples, filters, idat_split=split,
                                    stream_edit=lambda z, style=style: C.restream(zlib.decompress(z), style)))
            names.append((style, w, split))
    assert len(C.STYLES) == 12 and {n[2] for n in names} == {1, 3, 5}
    gpu = A.png_decode_many(files, inflate="gpu")
    host = A.png_decode_many(files, inflate="host")
    for n, f, g, h in zip(names, files, gpu, host):
        want = P.reference(f, "RGB")
        assert np.array_equal(want, P.pillow(f, "RGB")), n
        assert g.shape == want.shape and np.array_equal(g.cpu().numpy(), want), n
        assert torch.equal(g, h), n


def test_through_decompress_many(A):
    """a 33 x 35 YCoCg-R .ajpg whose layer streams are rewritten stored-only and with a long-tailed dynamic code"""
    from adaptive_edge_aware_jpeg_amd.jpeg import parse_container
    x = np.random.default_rng(5).random((1, 33, 35, 3), dtype=np.float32)
    c = A.Jpeg(A.JpegCompressionSettings("YCoCg-R", (40, 80), (2, 16)))
    data = c.compress_many(x, extension=".png", zlib_level=6)[0]
    plain = A.Jpeg(A.JpegCompressionSettings())
    want = plain.decompress(data).data
    head = data[:4 + int.from_bytes(data[:4], "big")]
    _, layers = parse_container(data)
    files = []
    for style in ("stored", "long_literal_codes", "block_mix"):
        new = [[2 * n, r, bytes(p), C.restream(zlib.decompress(bytes(s)), style)] for n, r, p, s in layers]
        assert all(a[3] != bytes(b[3]) for a, b in zip(new, layers))
        files.append(rebuild(head, new))
        assert np.array_equal(plain.decompress(files[-1]).data, want), style
    got = plain.decompress_many([data] + files, entropy="gpu").cpu().numpy()
    for k in range(len(files) + 1):
        assert np.array_equal(got[k], want), k
