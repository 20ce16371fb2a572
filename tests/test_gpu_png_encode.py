"""GPU: png_encode_many -- the scanline filter (csrc/png.hip, Pillow's choice rule) and the deflate of byte streams (csrc/deflate.hip,
aej_deflate_bytes_*).  The references are tests/png_encode_reference.py (which tests/test_png_encode_host.py holds against Pillow),
Pillow itself, zlib, and the package's own decoder."""
import ctypes
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_encode_cases as C
import png_encode_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def pil_save(x, **kw):
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, "PNG", **kw)
    return buf.getvalue()


def all_cases():
    out = dict(C.mode_cases())
    out.update(C.crafted_cases())
    out["split"] = C.split_image()
    return out


def device_scanlines(A, images, optimize=False):
    """The scanline streams the filter kernel writes for `images` (one call), as bytes."""
    from adaptive_edge_aware_jpeg_amd import png as P
    ctx = A._lib.get_context(0)
    items = P._check_images(images, "auto", optimize, 6, "gpu", None)
    raw, offs, sizes, keep = P._filter_on_device(ctx, items, optimize)
    host = raw.cpu().numpy()
    return [host[o:o + k].tobytes() for o, k in zip(offs, sizes)]


# ---- entropy="host": Pillow's file, byte for byte
@pytest.mark.parametrize("optimize,level", [(False, 6), (False, 1), (False, 9), (True, 6)])
def test_host_entropy_equals_pillow_in_one_mixed_call(A, optimize, level):
    cases = all_cases()
    names = sorted(cases)
    got = A.png_encode_many([cases[n] for n in names], optimize=optimize, compress_level=level, entropy="host")
    assert len(got) == len(names)
    for n, g in zip(names, got):
        assert isinstance(g, bytes)
        assert g == pil_save(cases[n], optimize=optimize, compress_level=level), n


def test_host_entropy_input_kinds(A, torch):
    """device tensors, host tensors and numpy arrays in one call; a non-contiguous tensor and array (accepted: made contiguous first); a
    device tensor at an odd address"""
    x = C.smooth(21, 37, 3, noise=3, seed=1)
    wide = C.smooth(21, 80, 4, noise=3, seed=2)
    flat = torch.from_numpy(np.concatenate([[0], x.reshape(-1)]).astype(np.uint8)).cuda()
    odd = flat[1:].view(21, 37, 3)
    assert odd.data_ptr() % 2 == 1
    images = [torch.from_numpy(x).cuda(), torch.from_numpy(x), x, torch.from_numpy(wide).cuda()[:, ::2], wide[:, ::2], odd,
              torch.from_numpy(wide).cuda().permute(1, 0, 2), np.asfortranarray(x[..., 0])]
    assert not images[3].is_contiguous() and not images[4].flags["C_CONTIGUOUS"] and not images[6].is_contiguous()
    want = [x, x, x, wide[:, ::2], wide[:, ::2], x, wide.transpose(1, 0, 2), x[..., 0]]
    got = A.png_encode_many(images, entropy="host")
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == pil_save(np.ascontiguousarray(w)), i
    for m, c in C.CHANNELS.items():
        assert A.png_encode_many([C.smooth(5, 6, c)], mode=m, entropy="host")[0] == pil_save(C.smooth(5, 6, c))


# ---- the filter kernel's edges: the scanline stream itself against the reference
EDGE_BYTES = (1, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)      # a lane loads 4 bytes, a wave 256 a step


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_filter_kernel_edges(A, c, optimize):
    """row bytes around a lane's dword and a wave's step of 256 bytes (rounded up to whole pixels); heights 1, 2 and 5 -- one row more
    than a workgroup's four waves take; a 1 x 1 image; all of it in one launch, so the rows' destinations fall on every alignment"""
    images = []
    for k, nb in enumerate(EDGE_BYTES):
        w = -(-nb // c)
        for h in (1, 2, 5):
            images.append(C.smooth(h, w, c, noise=6, seed=100 * k + h) if (k + h) % 2 else C.noise(h, w, c, seed=100 * k + h))
    images.append(C.noise(1, 1, c, seed=9))
    got = device_scanlines(A, images, optimize)
    for x, g in zip(images, got):
        want = R.scanlines(x, optimize)
        assert g == want, (x.shape, np.flatnonzero(np.frombuffer(g, np.uint8) != np.frombuffer(want, np.uint8))[:4].tolist())


def test_filter_kernel_decisions(A):
    cases = all_cases()
    names = sorted(cases)
    for optimize in (False, True):
        got = device_scanlines(A, [cases[n] for n in names], optimize)
        for n, g in zip(names, got):
            assert g == R.scanlines(cases[n], optimize), (n, optimize)
    assert device_scanlines(A, [C.tie_image("average")], True)[0][7] == 3
    assert device_scanlines(A, [C.tie_image("average")], False)[0][7] == 4


def test_filter_more_images_than_one_launch_takes(A):
    """65 images: the second launch of the call starts its row table again"""
    images = [C.smooth(3 + i % 4, 5 + i, 1 + i % 4, noise=3, seed=i) for i in range(65)]
    for x, g in zip(images, device_scanlines(A, images)):
        assert g == R.scanlines(x)


# ---- entropy="gpu"
def check_gpu_files(A, images, files, optimize=False):
    assert len(files) == len(images)
    for x, f in zip(images, files):
        stream, n_idat = R.idat(f)
        assert n_idat == -(-len(stream) // R.IDAT_BYTES)
        assert f == R.frame(x.shape, stream)
        assert zlib.decompress(stream) == R.scanlines(x, optimize)
        opened = Image.open(io.BytesIO(f))
        opened.load()
        assert np.array_equal(np.asarray(opened), x)
    for inflate in ("gpu", "host"):
        back = A.png_decode_many(files, mode="auto", inflate=inflate)
        for x, b in zip(images, back):
            b = b.cpu().numpy()
            assert b.shape == x.shape and np.array_equal(b, x), (x.shape, inflate)


@pytest.mark.parametrize("optimize", [False, True])
def test_gpu_entropy_mixed_call(A, optimize):
    cases = all_cases()
    names = sorted(cases)
    images = [cases[n] for n in names]
    files = A.png_encode_many(images, optimize=optimize)
    check_gpu_files(A, images, files, optimize)
    assert A.png_encode_many(images, optimize=optimize, compress_level=1) == files       # compress_level is ignored; same input, same bytes
    for i in (0, len(names) // 2, len(names) - 1):
        assert A.png_encode_many([images[i]], optimize=optimize)[0] == files[i], names[i]  # a file of a batch equals the file encoded alone


def test_gpu_entropy_round_trip_on_the_device(A, torch):
    """png_decode_many(png_encode_many(x)) == x for device tensors, decoded tensors fed back in"""
    images = [torch.from_numpy(x).cuda() for x in (C.smooth(70, 90, 3, noise=2), C.noise(33, 20, 4), C.smooth(40, 41, 1, noise=9), C.smooth(9, 300, 2, noise=1))]
    files = A.png_encode_many(images)
    for inflate in ("gpu", "host"):
        back = A.png_decode_many(files, mode="auto", inflate=inflate)
        assert all(torch.equal(a, b) for a, b in zip(images, back))
        assert A.png_encode_many(back) == files


def test_gpu_entropy_rows_that_repeat(A):
    """rows that repeat every 2 rows (Up costs nothing from row 2 on -- but Pillow filters against the row above, so the period shows in
    the scanline stream at two scanlines' distance), a period of one pixel, and a large IDAT (noise: more than one chunk of 65536)"""
    two = C.noise(2, 300, 3, seed=4)
    images = [np.tile(two, (40, 1, 1)), np.tile(C.noise(1, 1, 3, seed=5), (30, 200, 1)), C.split_image(), C.smooth(130, 2800, 4, noise=1, seed=6)]
    files = A.png_encode_many(images)
    check_gpu_files(A, images, files)
    assert R.idat(files[2])[1] >= 2
    assert len(files[0]) < R.huffman_only(R.scanlines(images[0])) and len(files[1]) < 2000


# Size of the entropy="gpu" file over Pillow's compress_level=1 file (and, for noise, over Pillow's default file, which is stored
# blocks), as measured and rounded up to two decimals (EXPERIMENTS.md): the output is deterministic, so the bound only catches regressions.
RATIO_TO_LEVEL_1 = {"gradient": 1.03, "tiles": 1.74, "lena-tiled": 1.01}      # measured 1.0275, 1.7352, 1.0099
NOISE_RATIO = 1.00                                                             # measured 0.9995


def test_size(A):
    size_set = C.size_set()
    names = sorted(size_set)
    files = A.png_encode_many([size_set[n] for n in names] + [C.size_noise()])
    check_gpu_files(A, [size_set[n] for n in names] + [C.size_noise()], files)
    rows = []
    for n, f in zip(names, files):
        x = size_set[n]
        l1, l6, huff = len(pil_save(x, compress_level=1)), len(pil_save(x, compress_level=6)), R.huffman_only(R.scanlines(x))
        print(f"png_encode size {n}: gpu {len(f)} level-1 {l1} level-6 {l6} huffman-only {huff} ratio-1 {len(f) / l1:.4f} ratio-6 {len(f) / l6:.4f}")
        rows.append((n, len(f), l1, huff))
    pn = len(pil_save(C.size_noise()))
    print(f"png_encode size noise: gpu {len(files[-1])} pillow {pn} ratio {len(files[-1]) / pn:.4f}")
    for n, size, l1, huff in rows:
        assert size < huff, n                                   # matches are found and coded
        assert size / l1 <= RATIO_TO_LEVEL_1[n], n
    assert len(files[-1]) / pn <= NOISE_RATIO


# ---- the byte deflate on streams no image gives: driven through ctypes
class Deflater:
    def __init__(self, A):
        import torch
        self.t, self.ctx, self.lib = torch, A._lib.get_context(0), A._lib.get_context(0).lib

    def run(self, streams, adaptive=True, caps=None, fill=0xAB):
        """streams: [(bytes, bpp, stride)] -> (return code of aej_deflate_bytes_batch, [zlib streams], the whole output buffer)"""
        t, ctx, lib, n = self.t, self.ctx, self.lib, len(streams)
        offs, pos = [], 0
        for s, _, _ in streams:
            offs.append(pos)
            pos = (pos + len(s) + 3) // 4 * 4
        host = np.full(pos + 4, 0xEE, np.uint8)               # (the bytes between the streams are not zero)
        for o, (s, _, _) in zip(offs, streams):
            host[o:o + len(s)] = np.frombuffer(s, np.uint8)
        src = t.from_numpy(host).cuda()
        caps = caps or [(int(lib.aej_deflate_stream_bound(ctypes.c_uint64(len(s)))) + 3) // 4 * 4 for s, _, _ in streams]
        out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        descs = np.array([(offs[i], len(s), bpp, stride, out_off[i], caps[i]) for i, (s, bpp, stride) in enumerate(streams)], np.int64).reshape(n, 6)
        nws = int(lib.aej_deflate_bytes_workspace_bytes(descs.ctypes.data, n))
        if nws == 0:
            return -1, None, None
        ws = t.empty(nws, dtype=t.uint8, device="cuda")
        out = t.full((int(out_off[n]) + 64,), fill, dtype=t.uint8, device="cuda")
        sizes = t.zeros(n, dtype=t.int64, device="cuda")
        common = (ctx.handle, src.data_ptr(), ctypes.c_uint64(src.numel()), descs.ctypes.data, n)
        tabs = None
        if adaptive:
            hist = t.zeros((n, 320), dtype=t.int32, device="cuda")
            ctx.check(lib.aej_deflate_bytes_histogram(*common, hist.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws)))
            h = np.ascontiguousarray(hist.cpu().numpy())
            tab = np.zeros((n, 448), np.uint32)
            assert lib.aej_deflate_bytes_build_tables(h.ctypes.data, n, tab.ctypes.data) == 0
            tabs = t.from_numpy(tab.view(np.int32)).cuda()
        rc = lib.aej_deflate_bytes_batch(*common, tabs.data_ptr() if adaptive else None, 1 if adaptive else 0, out.data_ptr(),
                                         ctypes.c_uint64(int(out_off[n])), sizes.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws))
        o, k = out.cpu().numpy(), sizes.cpu().numpy()
        return rc, [o[int(out_off[i]):int(out_off[i]) + int(k[i])].tobytes() for i in range(n)], (o, out_off, caps)

    def check(self, streams, adaptive=True):
        rc, got, (o, out_off, caps) = self.run(streams, adaptive)
        assert rc == 0
        for i, ((s, _, _), g) in enumerate(zip(streams, got)):
            assert zlib.decompress(g) == s, (i, len(s))
            assert (o[int(out_off[i]) + (len(g) + 3) // 4 * 4:int(out_off[i]) + caps[i]] == 0xAB).all(), i     # nothing written behind the stream's last dword
        assert (o[int(out_off[-1]):] == 0xAB).all()
        return got


@pytest.fixture(scope="module")
def deflater(A):
    return Deflater(A)


def periodic(period, n, seed):
    return np.resize(np.random.default_rng(seed).integers(0, 256, period, dtype=np.uint8), n).tobytes()


def matcher_streams():
    rng = np.random.default_rng(11)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    small = lambda n: rng.integers(0, 3, n, dtype=np.uint8).tobytes()
    out = [(bytes([7] * n), 1, 2) for n in (1, 2, 3, 4)] + [(rnd(n), 3, 10) for n in (1, 2, 3, 4, 5)]
    out += [(small(n), 3, 301) for n in (8191, 8192, 8193, 16385)]                 # one chunk - 1, one chunk, + 1, two chunks + 1
    out += [(periodic(100, 8192 + 130, 1), 4, 401)]                                # matches up to and across the chunk edge, and every sub-block edge
    out += [(rnd(50) + periodic(61, 8192 - 50 + 61, 2), 1, 62)]                    # a scanline-distance match whose source lies in the chunk before
    out += [(rnd(300) + bytes([200] * 1000) + rnd(300) + bytes(700), 3, 100)]      # runs of one value longer than 258
    out += [(periodic(32767, 32767 + 8400, 3), 1, 32767)]                          # the largest distance a chunk with its history reaches
    out += [(periodic(32768, 32768 + 8400, 4), 4, 32768 - 4)]                      # stride + bpp = 32768: beyond what the history holds, never taken
    out += [(periodic(32769, 32769 + 100, 5), 1, 32769)]                           # a distance deflate cannot code
    out += [(periodic(3, 5000, 6), 3, 1 + 3 * 40), (periodic(4, 9000, 7), 4, 1 + 4 * 40)]       # period bpp
    out += [(rnd(20000), 3, 301)]                                                  # uniform noise
    return out


@pytest.mark.parametrize("adaptive", [True, False])
def test_matcher_inputs(deflater, adaptive):
    streams = matcher_streams()
    got = deflater.check(streams, adaptive)
    assert got == deflater.check(streams, adaptive)                                # deterministic
    alone = deflater.check([streams[13]], adaptive)
    assert alone[0] == got[13]
    if adaptive:
        size = {len(s): len(g) for (s, _, _), g in zip(streams, got)}
        # literals cost at most 9 bits and a code's description at most 524 bytes; a match of a whole 64-byte sub-block about 3 bytes
        assert size[8192 + 130] < 1200 and size[8192 + 61] < 1200                 # the periods are found, across the chunk edge too
        assert size[5000] < 400 and size[9000] < 600
        assert size[2300] < 1400                                                   # 600 random bytes, and 1700 in runs


def test_matcher_more_streams_than_one_launch_takes(deflater):
    rng = np.random.default_rng(12)
    streams = [(rng.integers(0, 4, 50 + 700 * i, dtype=np.uint8).tobytes(), 1 + i % 4, 31 + i) for i in range(35)]
    deflater.check(streams)


def test_matcher_refusals(deflater, A):
    one = [(bytes(100), 1, 10)]
    assert deflater.run([(b"", 1, 10)])[0] == -1                                   # no rows: an empty stream has no workspace size ...
    lib, ctx, t = deflater.lib, deflater.ctx, deflater.t
    buf = t.zeros(4096, dtype=t.uint8, device="cuda")
    sizes = t.zeros(1, dtype=t.int64, device="cuda")

    def batch(desc, in_bytes=1024, out_bytes=1024):
        d = np.array([desc], np.int64)
        return lib.aej_deflate_bytes_batch(ctx.handle, buf.data_ptr(), ctypes.c_uint64(in_bytes), d.ctypes.data, 1, None, 0, buf.data_ptr() + 2048,
                                           ctypes.c_uint64(out_bytes), sizes.data_ptr(), buf.data_ptr(), ctypes.c_uint64(0))
    for desc in ([0, 0, 1, 10, 0, 64], [2, 100, 1, 10, 0, 64], [0, 2000, 1, 10, 0, 64], [0, 100, 5, 10, 0, 64], [0, 100, 1, 0, 0, 64],
                 [0, 100, 1, 10, 2, 64], [0, 100, 1, 10, 0, 12], [0, 100, 1, 10, 1000, 64], [4, 1022, 1, 10, 0, 64]):
        assert batch(desc) == A._lib.AEJ_ERR_ARG, desc                             # ... and the entry refuses it, like every bad descriptor
    assert batch([0, 100, 1, 10, 0, 64]) == A._lib.AEJ_ERR_CAPACITY                # (no workspace)
    # a stream that does not fit its slot: an error return, its size reported, and not a byte written outside
    noise = np.random.default_rng(13).integers(0, 256, 3000, dtype=np.uint8).tobytes()
    rc, got, (o, out_off, caps) = deflater.run([(bytes(20000), 1, 10), (noise, 1, 10)], caps=[64, 4000])
    assert rc == A._lib.AEJ_ERR_CAPACITY
    assert (o[64 + 4000:] == 0xAB).all()
    assert "does not fit" in lib.aej_last_error(ctx.handle).decode()


def test_zero_rows_are_refused(A):
    with pytest.raises(ValueError, match="image 0: .*no pixels"):
        A.png_encode_many([np.zeros((0, 4, 3), np.uint8)])
