"""GPU: PSNR / SSIM / MS-SSIM (metrics.hip) against the float64 restatement (oracle/metrics_oracle.py, separable form) at the shapes the
sweep and the benchmarks use -- 1080p, 4K and 8K batches whose strips are 32, 64 and 128 rows high, every grey-pool factor and tie, strip
edges, the MS-SSIM pad chain -- to stated float32 bounds; localised differences whose deficit only the right geometry explains; and
bit-identical scores across calls, batch sizes, batch orders and the sweep's sub-batching.

Bounds.  PSNR: each squared difference is within 2 u (u = 2^-24) of exact, a float sum of 12 within 11 u more, the rest is float64: the
mean square is within 16 u relative, PSNR within 10 / ln 10 * 16 u dB.  SSIM / MS-SSIM: M.ssim_stats' first-order worst case of the
kernel's float32 arithmetic, evaluated on the pair itself (its docstring).  The reference uses the kernel's taps, float32(g), so the bound
covers arithmetic only; the taps' distance from piq's float32 2-D window is tests/test_metrics.py's concern.
Worst errors seen: profiles/metrics_worst_errors.txt (written when METRICS_WORST_ERRORS names a file)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import golden_image
from oracle import metrics_oracle as M

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
G32 = M.gaussian_1d().astype(np.float32).astype(np.float64)          # the kernel's taps
NATURAL = ["baboon", "bikes", "buildings", "house", "jelly_beans", "peppers"]
WORST = {}
POOL = ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0))))


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    yield pkg
    out = os.environ.get("METRICS_WORST_ERRORS")
    if out:
        with open(out, "w") as fh:
            for k in sorted(WORST):
                e, b = WORST[k]
                fh.write(f"{k}: worst |gpu - float64| {e:.3e} (its bound {b:.3e})\n")


def _fit(img, H, W):
    """img tiled (mirrored) to cover H x W, cropped"""
    reps = (-(-H // img.shape[0]), -(-W // img.shape[1]))
    t = np.concatenate([np.concatenate([img if (j % 2 == 0) else img[:, ::-1] for j in range(reps[1])], 1) if i % 2 == 0 else
                        np.concatenate([img[::-1] if (j % 2 == 0) else img[::-1, ::-1] for j in range(reps[1])], 1) for i in range(reps[0])], 0)
    return np.ascontiguousarray(t[:H, :W])


def natural(H, W, i):
    return _fit(golden_image("natural/" + NATURAL[i % len(NATURAL)]), H, W)


def pairs(A, H, W, n, seed):
    """[n, H, W, 3] float32 pairs: codec round trips (two settings), natural + noise, exact k/255 levels one level apart, b = 1 - a
    (negative cs: MS-SSIM's relu)"""
    rng = np.random.default_rng(seed)
    a = np.stack([natural(H, W, seed + i) for i in range(n)])
    b = np.empty_like(a)
    kinds = [i % 5 for i in range(n)]
    for k, qr in ((0, (10, 50)), (1, (60, 90))):
        idx = [i for i in range(n) if kinds[i] == k]
        if idx:
            codec = A.Jpeg(A.JpegCompressionSettings("YCbCr", qr, (4, 64)))
            b[idx] = codec.decompress_batch(codec.compress_batch(a[idx])).cpu().numpy()
    for i in range(n):
        if kinds[i] == 2:
            b[i] = np.clip(a[i] + rng.normal(0, 0.02, a[i].shape).astype(np.float32), 0, 1)
        elif kinds[i] == 3:
            lv = np.clip(np.round(a[i] * 255) + rng.integers(-1, 2, a[i].shape), 0, 255)
            b[i] = (lv / 255).astype(np.float32)
            a[i] = (np.round(a[i] * 255) / 255).astype(np.float32)
        elif kinds[i] == 4:
            b[i] = (1 - a[i]).astype(np.float32)
    return a, np.ascontiguousarray(b)


def reference(a, b, which=7):
    """(psnr, psnr bound), (ssim, bound), (ms_ssim, bound) of one pair"""
    p = M.psnr(a, b)
    mse = 10 ** (-p / 10) - 1e-8
    out = [(p, 10 / np.log(10) * 16 * U * mse / (mse + 1e-8) + 1e-12)]
    out.append(M.ssim_fast(a, b, g=G32) if which & 2 else (np.nan, 0))
    out.append(M.ms_ssim_fast(a, b, g=G32) if which & 4 else (np.nan, 0))
    return out


def check(A, a, b, got, idx, label, which=7):
    refs = list(POOL.map(lambda i: reference(a[i], b[i], which), idx))
    for i, ref in zip(idx, refs):
        for col, name in enumerate(("psnr", "ssim", "ms_ssim")):
            if not which & (1 << col):
                assert np.isnan(got[i, col])
                continue
            want, bound = ref[col]
            err = abs(float(got[i, col]) - want)
            key = f"{name} {label}"
            if err > WORST.get(key, (-1, 0))[0]:
                WORST[key] = (err, bound)
            assert err <= bound, (label, i, name, float(got[i, col]), want, err, bound)


# ------------------------------------------------------------------ accuracy where the strips are 32, 64 and 128 rows
@pytest.mark.parametrize("H,W,Bs,idx", [(1080, 1920, (1, 8, 24), (0, 3, 4, 7, 23)), (2160, 3840, (1, 2, 6), (0, 1, 4))],
                         ids=["1080p", "4K"])
def test_accuracy_at_batch_shapes(A, H, W, Bs, idx):
    a, b = pairs(A, H, W, Bs[-1], 5)
    for B in Bs:
        got = A.EvaluationMetrics.batch(a[:B], b[:B]).cpu().numpy()
        check(A, a, b, got, [i for i in idx if i < B], f"{H}x{W} B={B}")
    assert (got[[i for i in range(Bs[-1]) if i % 5 == 4], 2] < 0.2).all()         # 1 - a: relu'd scales


def test_accuracy_8k(A):
    a, b = pairs(A, 4320, 7680, 1, 0)
    assert M.grey_pool_factor(4320, 7680) == 17
    got = A.EvaluationMetrics.batch(a, b, 3).cpu().numpy()
    check(A, a, b, got, [0], "8K", 3)


# ------------------------------------------------------------------ grey-pool factors and strip geometry
GREY = [(383, 500), (384, 500), (385, 500), (639, 700), (640, 700), (641, 700), (895, 1000), (896, 1000), (700, 769), (1000, 1152),
        (1153, 1300), (2050, 2100), (11, 11), (11, 300), (300, 11), (60, 100), (41, 137), (42, 138), (43, 139), (137, 265), (138, 266),
        (139, 267), (171, 900)]


@pytest.mark.parametrize("H,W", GREY, ids=[f"{h}x{w}" for h, w in GREY])
def test_grey_pool_and_strip_edges(A, H, W):
    a, b = pairs(A, H, W, 3, H + W)
    got = A.EvaluationMetrics.batch(a, b, 3).cpu().numpy()
    check(A, a, b, got, [0, 1, 2], f"grey f={M.grey_pool_factor(H, W)}", 3)


def _chain(H, W):
    out = []
    for _ in range(4):
        out.append((H % 2, W % 2))
        p = max(H % 2, W % 2)
        H, W = (H + p) // 2, (W + p) // 2
    return out


CHAIN = [(161, 161), (322, 323), (323, 322), (338, 404), (404, 339), (520, 700)]


def test_chain_sizes_cover_every_parity():
    seen = {pq for s in CHAIN for pq in _chain(*s)}
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {_chain(*s)[0] == (0, 0) for s in CHAIN} == {True, False}      # the fused scale-0 pool and k_pool2_rgb


@pytest.mark.parametrize("H,W", CHAIN, ids=[f"{h}x{w}" for h, w in CHAIN])
def test_ms_ssim_scale_chain(A, H, W):
    a, b = pairs(A, H, W, 5, H * W)
    got = A.EvaluationMetrics.batch(a, b).cpu().numpy()
    check(A, a, b, got, range(5), "ms chain")


# ------------------------------------------------------------------ localised differences
def _deficit_gpu(A, a, b, which):
    got = A.EvaluationMetrics.batch(np.stack([a, a]), np.stack([a, b]), which).cpu().numpy()
    col = 1 if which == 2 else 2
    return float(got[0, col] - got[1, col])


def _deficit_ref(a, b, metric, **geom):
    if metric == "ssim":
        s0, _ = M.ssim_fast(a, a, g=G32, **geom)
        s1, bound = M.ssim_fast(a, b, g=G32, diff_only=True, **geom)
    else:
        s0, _ = M.ms_ssim_fast(a, a, g=G32, **geom)
        s1, bound = M.ms_ssim_fast(a, b, g=G32, diff_only=True, **geom)
    return s0 - s1, bound


def _patched(a, y, x, h, w):
    b = a.copy()
    b[y:y + h, x:x + w] = 1 - b[y:y + h, x:x + w]
    return b


# (metric, H, W, patch (y, x, h, w) with negatives from the end, the wrong reference: geometry keywords or a patch shift)
PROBES = [
    ("ssim", 300, 267, (0, 0, 8, 8), (1, 1)),                         # first rows / columns
    ("ssim", 300, 267, (-8, -8, 8, 8), (-1, -1)),                     # last rows / columns
    ("ssim", 300, 267, (-3, 120, 3, 20), (-1, 0)),                    # last rows, across the first strip's last columns
    ("ms_ssim", 322, 402, (-12, -12, 12, 12), {"pad": "bottom_right"}),  # even sizes: the scale-1 halo the last strip writes
    ("ms_ssim", 322, 402, (100, -6, 120, 6), {"pad": "bottom_right"}),  # last columns of an even scale, odd next scale
    ("ms_ssim", 323, 403, (0, 0, 12, 12), {"pad": "bottom_right"}),   # replicated top-left row and column (odd scale)
    ("ms_ssim", 323, 402, (100, -1, 40, 1), {"pad": "bottom_right"}),  # the column avg_pool2d drops after the pad
    ("ms_ssim", 324, 401, (-1, 100, 1, 40), (-1, 0)),                 # the row avg_pool2d drops
    ("ssim", 1082, 1925, (-2, 0, 2, 1925), {"crop": "top_left"}),     # rows the grey pool crops (f = 4): no effect
    ("ssim", 1082, 1925, (0, -1, 1082, 1), {"crop": "top_left"}),     # the column it crops
    ("ssim", 640, 700, (300, 300, 4, 4), {"f_round": "half_up"}),     # 2.5 -> 2 (ties to even)
    ("ssim", 1152, 1300, (300, 301, 4, 4), {"f_round": "half_up"}),   # 4.5 -> 4
    ("ssim", 1152, 1300, (300, 301, 4, 4), (0, -1)),                  # the patch one pixel over, across a pool phase
]


@pytest.mark.parametrize("metric,H,W,patch,wrong", PROBES, ids=[f"{p[0]}-{p[1]}x{p[2]}-{i}" for i, p in enumerate(PROBES)])
def test_localised_difference(A, metric, H, W, patch, wrong):
    a = natural(H, W, H)
    y, x, h, w = patch
    y, x = y % H, x % W
    b = _patched(a, y, x, h, w)
    which = 2 if metric == "ssim" else 4
    got = _deficit_gpu(A, a, b, which)
    want, bound = _deficit_ref(a, b, metric)
    key = f"{metric} deficit"
    if abs(got - want) > WORST.get(key, (-1, 0))[0]:
        WORST[key] = (abs(got - want), bound)
    assert abs(got - want) <= bound, (got, want, bound)
    if want == 0:
        assert got == 0.0                                            # nothing the score reads has changed: bit-identical
    else:
        assert want > 4 * bound                                      # the probe is above its noise
    if isinstance(wrong, dict):
        alt, _ = _deficit_ref(a, b, metric, **wrong)
    else:
        dy, dx = wrong
        alt, _ = _deficit_ref(a, _patched(a, y + dy, x + dx, h, w), metric)
    assert abs(alt - got) > bound, ("the wrong geometry is not told apart", alt, got, bound)


# ------------------------------------------------------------------ determinism and batch invariance
@pytest.mark.parametrize("H,W,Bs", [(1080, 1920, (1, 8, 24)), (2160, 3840, (1, 6))], ids=["1080p", "4K"])
def test_batch_invariance(A, H, W, Bs):
    a, b = pairs(A, H, W, Bs[-1], 11)
    full = A.EvaluationMetrics.batch(a, b).cpu().numpy()
    again = A.EvaluationMetrics.batch(a, b).cpu().numpy()
    assert np.array_equal(full, again)
    for B in Bs[:-1]:
        part = A.EvaluationMetrics.batch(a[:B], b[:B]).cpu().numpy()
        assert np.array_equal(part, full[:B]), (B, np.abs(part - full[:B]).max(axis=0))
    perm = np.random.default_rng(0).permutation(Bs[-1])
    shuffled = A.EvaluationMetrics.batch(a[perm], b[perm]).cpu().numpy()
    assert np.array_equal(shuffled, full[perm]), np.abs(shuffled - full[perm]).max(axis=0)


def test_sweep_metrics_do_not_depend_on_max_bytes(A):
    x = np.stack([natural(1080, 1920, i) for i in range(8)])
    grid = (("YCbCr",), [(20, 60)], [(4, 64)])
    full = A.sweep(x, *grid, sizes=None, standard_qualities=(50,))
    tiny = A.sweep(x, *grid, sizes=None, standard_qualities=(50,), max_bytes=1)
    assert all(len(s) == 1 for subs in tiny.sub_batches.values() for s in subs)
    for k in ("psnr", "ssim", "ms_ssim"):
        assert np.array_equal(getattr(full, k), getattr(tiny, k)), (k, np.abs(getattr(full, k) - getattr(tiny, k)).max())
        assert np.array_equal(getattr(full.standard, k), getattr(tiny.standard, k)), k
