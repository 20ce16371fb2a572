"""GPU: aej_requantise_batch, aej_decode_batch_tables and sweep() against the existing public calls."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_image

pytestmark = pytest.mark.gpu
GUARD = -0x5A5A5A5B


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def S(A):
    return importlib.import_module("adaptive_edge_aware_jpeg_amd.sweep")


def synth(oracle, H, W, seed, kind="mixed"):
    return oracle.synth_image(H, W, seed, kind).astype(np.float32) / np.float32(255)


def requantise(ctx, enc, blob_host, n_sets, out=None, stride=None):
    t = ctx.torch
    p = enc.plan
    n = p.batch * p.coeff_stride
    stride = n if stride is None else stride
    if out is None:
        out = t.full((n_sets * stride,), GUARD, dtype=t.int32, device=ctx.device)
    blob = ctx.to_device(np.ascontiguousarray(blob_host, np.int32), t.int32)
    rc = ctx.lib.aej_requantise_batch(ctx.handle, enc.dct.data_ptr(), enc.leaves.data_ptr(), enc.counts.data_ptr(), p.batch, p.H, p.W, n_sets,
                                      blob.data_ptr(), out.data_ptr(), ctypes.c_uint64(stride))
    return rc, out


def layer_slices(p, cnt, b, l):
    o = b * p.coeff_stride + p.coeff_off[l]
    end = b * p.coeff_stride + (p.coeff_off[l + 1] if l < 2 else p.coeff_stride)
    return o, o + int(cnt[b, l, 0]), end


@pytest.mark.parametrize("space, br, qrs", [
    ("YCbCr", (4, 64), [(40, 80), (10, 90), (75, 75)]),
    ("YCoCg-R", (2, 32), [(10, 10), (50, 90)]),
    ("OKLAB", (4, 128), [(25, 75), (90, 90), (10, 50)]),
    ("YCbCr", (8, 8), [(50, 50), (10, 25)]),
    ("ICtCp", (32, 256), [(40, 80), (10, 90)]),
])
def test_requantise_equals_compress_batch(A, S, oracle, space, br, qrs):
    imgs = np.stack([synth(oracle, 333, 517, 11), synth(oracle, 333, 517, 12, "noise")])
    base = A.Jpeg(A.JpegCompressionSettings(space, (40, 80), br))
    enc = base.compress_batch(imgs, want_dct=True)
    ctx = base._bind()
    rc, out = requantise(ctx, enc, np.concatenate([S.qmats_blob(space, qr, br) for qr in qrs]), len(qrs))
    assert rc == 0, ctx.lib.aej_last_error(ctx.handle)
    out = out.view(len(qrs), -1).cpu().numpy()
    p, cnt = enc.plan, enc.counts_host
    for j, qr in enumerate(qrs):
        ref = A.Jpeg(A.JpegCompressionSettings(space, qr, br)).compress_batch(imgs)
        want = ref.coeffs.cpu().numpy()
        assert np.array_equal(ref.counts_host, cnt)
        for b in range(2):
            for l in range(3):
                o, e, end = layer_slices(p, cnt, b, l)
                assert np.array_equal(out[j, o:e], want[o:e]), (qr, b, l)
                assert (out[j, e:end] == GUARD).all(), (qr, b, l)           # nothing beyond n_coeffs


def test_requantise_equals_numpy_on_adversarial_tables(A, S, oracle):
    space, br = "YCbCr", (4, 32)
    img = synth(oracle, 200, 264, 5)[None]
    codec = A.Jpeg(A.JpegCompressionSettings(space, (40, 80), br))
    enc = codec.compress_batch(img, want_dct=True)
    ctx = codec._bind()
    words = S.qmats_blob(space, (40, 80), br).size
    rng = np.random.default_rng(3)
    sets = [np.ones(words, np.int32),                                                  # all 1: the plain rounding
            (1 << rng.integers(0, 5, words)).astype(np.int32),                          # powers of two: exact ties
            rng.integers((1 << 22) + 1, 1 << 30, words).astype(np.int32)]               # above 2^22: the float64 path
    rc, out = requantise(ctx, enc, np.concatenate(sets), 3)
    assert rc == 0
    out = out.view(3, -1).cpu().numpy()
    Y = enc.dct.cpu().numpy()
    sizes = [4, 8, 16, 32]
    lw = sum(s * s for s in sizes)
    p, cnt = enc.plan, enc.counts_host
    for j, qs in enumerate(sets):
        for l in range(3):
            lay = enc.layer(0, l)
            o0 = p.coeff_off[l]
            for (x, y, s), off in zip(lay["leaves"], lay["leaf_coeff_offsets"]):
                zz = S.tables.zigzag_ordering(int(s))
                k = sizes.index(int(s))
                q = qs[l * lw + sum(t * t for t in sizes[:k]):][:s * s].astype(np.float64)
                yv = Y[o0 + off:o0 + off + s * s].astype(np.float64)
                want = np.rint(yv[zz] / q[zz]).astype(np.int32)
                assert np.array_equal(out[j, o0 + off:o0 + off + s * s], want), (j, l, x, y, s)


def test_decode_batch_tables_equals_decode_batch(A, S, oracle):
    imgs = np.stack([synth(oracle, 240, 320, 7), synth(oracle, 240, 320, 8)])
    for space, qr, br in (("YCbCr", (10, 90), (4, 64)), ("YCoCg-R", (75, 75), (2, 32))):
        codec = A.Jpeg(A.JpegCompressionSettings(space, qr, br))
        enc = codec.compress_batch(imgs)
        want = codec.decompress_batch(enc).cpu().numpy()
        other = A.Jpeg(A.JpegCompressionSettings(space, (50, 50), br))
        ctx = other._bind()                              # the context's own tables are another quality's
        t = ctx.torch
        p = enc.plan
        blob = ctx.to_device(S.qmats_blob(space, qr, br), t.int32)
        rgb = ctx.empty((p.batch, p.H, p.W, 3), t.float32)
        nb = int(ctx.lib.aej_decode_workspace_bytes(ctx.handle, p.batch, p.H, p.W))
        ws = ctx.workspace(nb)
        rc = ctx.lib.aej_decode_batch_tables(ctx.handle, enc.coeffs.data_ptr(), enc.leaves.data_ptr(), enc.counts.data_ptr(), p.batch, p.H, p.W,
                                             blob.data_ptr(), rgb.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nb))
        assert rc == 0
        assert np.array_equal(rgb.cpu().numpy(), want)
        assert not np.array_equal(other.decompress_batch(enc).cpu().numpy(), want)      # the tables given were used


def test_corrupt_leaf_tables_are_refused_and_nothing_is_written(A, S, oracle):
    space, br = "YCbCr", (4, 64)
    codec = A.Jpeg(A.JpegCompressionSettings(space, (40, 80), br))
    enc = codec.compress_batch(synth(oracle, 200, 264, 9)[None], want_dct=True)
    ctx = codec._bind()
    blob = S.qmats_blob(space, (10, 90), br)
    good = enc.leaves.clone()
    lo = enc.plan.leaf_off[1]
    for col, val in ((2, 128), (2, 2), (2, 12), (3, 1 << 28), (3, -4), (0, 4096)):
        enc.leaves.copy_(good)
        enc.leaves[lo + 3, col] = val
        rc, out = requantise(ctx, enc, np.concatenate([blob, blob]), 2)
        assert rc == -1, (col, val)
        assert (out.cpu().numpy() == GUARD).all(), (col, val)
    enc.leaves.copy_(good)
    counts = enc.counts.clone()
    enc.counts[0, 2, 1] = 1 << 40                                      # n_leaves over capacity
    rc, out = requantise(ctx, enc, blob, 1)
    assert rc == -1 and (out.cpu().numpy() == GUARD).all()
    enc.counts.copy_(counts)
    bad = blob.copy()
    bad[17] = 0                                                        # a quantiser < 1
    rc, out = requantise(ctx, enc, bad, 1)
    assert rc == -1 and (out.cpu().numpy() == GUARD).all()
    rc, _ = requantise(ctx, enc, blob, 1)
    assert rc == 0


def independent(A, x, cs, qr, br, which, extension):
    codec = A.Jpeg(A.JpegCompressionSettings(cs, qr, br))
    m = A.EvaluationMetrics.batch(x, codec.decompress_batch(codec.compress_batch(x)), which).cpu().numpy()
    return m, [len(f) for f in codec.compress_many(x, extension=extension)], codec


def test_sweep_equals_independent_calls(A, S, oracle):
    x = np.stack([synth(oracle, 176, 200, 21), synth(oracle, 176, 200, 22, "noise"), synth(oracle, 176, 200, 23)])
    spaces, qrs, brs = ("YCbCr", "YCoCg-R"), [(10, 50), (75, 90), (40, 80)], [(4, 64), (8, 8)]
    res = A.sweep(x, spaces, qrs, brs, extension=".png", names=["a", "b", "c"])
    gpu = A.sweep(x, spaces, qrs, brs, metrics=0, sizes="gpu")
    assert len(res.cells) == 12 and res.cells[1] == ("YCbCr", (10, 50), (8, 8))
    for j, (cs, qr, br) in enumerate(res.cells):
        m, n, codec = independent(A, x, cs, qr, br, 7, ".png")
        assert np.array_equal(res.psnr[:, j], m[:, 0]) and np.array_equal(res.ssim[:, j], m[:, 1]) and np.array_equal(res.ms_ssim[:, j], m[:, 2])
        assert res.bytes[:, j].tolist() == n, (cs, qr, br)
        assert np.array_equal(res.compression_ratio[:, j], 176 * 200 * 3 / np.array(n, np.float64))
        for sub in gpu.sub_batches[cs, br]:
            g = [len(f) for f in codec.compress_many(x[sub], entropy="gpu")]
            assert gpu.bytes[sub, j].tolist() == g, (cs, qr, br)
    assert np.isnan(gpu.psnr).all()


def test_sweep_sizes_match_the_reference_files(A, lena):
    meta = json.load(open(os.path.join(GOLDEN, "compress_cases.json")))
    for name, m in meta.items():
        img = lena if m["image"] == "lena" else golden_image(m["image"])
        if m["crop"]:
            y, x, h, w = m["crop"]
            img = np.ascontiguousarray(img[y:y + h, x:x + w])
        data = open(os.path.join(GOLDEN, name + ".ajpg"), "rb").read()
        ext = json.loads(data[4:4 + int.from_bytes(data[:4], "big")])["extension"]
        res = A.sweep(img[None], (m["space"],), [tuple(m["quality_range"]), (10, 90)], [tuple(m["block_size_range"])], metrics=0, extension=ext)
        assert int(res.bytes[0, 0]) == m["bytes"] == len(data), name


def test_budget_and_mixed_sizes_do_not_change_results(A, oracle):
    x = np.stack([synth(oracle, 192, 240, s) for s in (31, 32, 33)])
    grid = (("YCbCr", "OKLAB"), [(10, 90), (50, 50), (25, 75)], [(4, 32), (16, 16)])
    full = A.sweep(x, *grid)
    tiny = A.sweep(x, *grid, max_bytes=1)
    assert all(len(s) == 1 for subs in tiny.sub_batches.values() for s in subs)
    for k in ("psnr", "ssim", "ms_ssim", "bytes"):
        assert np.array_equal(getattr(full, k), getattr(tiny, k)), k
    y = synth(oracle, 200, 168, 34)
    mixed = A.sweep([x[0], y, x[1]], *grid)
    alone = A.sweep(y[None], *grid)
    for k in ("psnr", "ssim", "ms_ssim", "bytes"):
        assert np.array_equal(getattr(mixed, k)[[0, 2]], getattr(full, k)[[0, 1]]), k
        assert np.array_equal(getattr(mixed, k)[1], getattr(alone, k)[0]), k
    u8 = A.sweep((x * 255).round().astype(np.uint8), *grid)
    for k in ("psnr", "ssim", "ms_ssim", "bytes"):
        assert np.array_equal(getattr(u8, k), getattr(full, k)), k
