"""Helpers of tests/test_gpu_large_image.py: periodic images of up to 2^29 pixels built on the device, expectations evaluated on one
period on the CPU, comparisons that stay on the device, and closed forms of the quadtree of an (almost) empty edge map.
TEST INFRASTRUCTURE ONLY.

Shapes.  S1 = 16384 x 21888 is the smallest convenient image whose float32 RGB exceeds 2^32 bytes (byte offsets in [2^31, 2^32) occur
inside it too); S2 = 16384 x 32768 = 2^29 pixels is the codec's stated limit: a float32 plane is exactly 2^31 bytes, float32 RGB 6 GiB.

Inputs.  A band of BAND_ROWS random rows repeats down the image.  Its period is a whole number of 12-byte pixels, which 2^32 and 2^31 are
not: a read whose byte offset wrapped lands in other content, and a channel late (band_detects_wraps)."""
import numpy as np
import pytest

S1 = (16384, 21888)
S2 = (16384, 32768)
LIMIT = 1 << 29
BAND_ROWS = 64
GIB = float(1 << 30)


def torch_mod():
    import torch
    return torch


def device():
    return torch_mod().device("cuda", 0)


def need_memory(nbytes, what):
    """skip (with both numbers) when the card has less free memory than the test's shapes need"""
    t = torch_mod()
    t.cuda.empty_cache()
    free, _ = t.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{what}: needs {nbytes / GIB:.1f} GiB of device memory, {free / GIB:.1f} GiB are free")


def release(*contexts):
    """the big tensors are the caller's to `del`; this drops the contexts' cached workspaces and the allocator's cache"""
    t = torch_mod()
    for c in contexts:
        c._ws = None
        c._pinned = None
    t.cuda.synchronize()
    t.cuda.empty_cache()


# ------------------------------------------------------------------ periodic inputs
def band_u8(W, seed, channels=3):
    shape = (BAND_ROWS, W, channels) if channels else (BAND_ROWS, W)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def band_f32(u8):
    """float32(v) / 255, as conftest.golden_image forms it"""
    return u8.astype(np.float32) / np.float32(255.0)


def band_detects_wraps(band):
    """the band differs from itself shifted by 2^32 and 2^31 bytes (mod its period) at nearly every element: a wrapped read shows"""
    b = np.ascontiguousarray(band).ravel()
    for wrap in (1 << 32, 1 << 31):
        shift = wrap % b.nbytes
        assert shift % (band.itemsize * 3) != 0, "the wrap is a whole number of pixels: the shifted read would see the same channel"
        assert shift % band.itemsize == 0           # (a whole number of elements, so elements are compared: two random levels agree 1 time in 256)
        same = (b == np.roll(b, -(shift // band.itemsize))).mean()
        assert same < 0.01, (wrap, shift, same)
    return True


def tiled(band_np, H, dtype=None):
    """the band repeated down H rows, on the device: [H, W, ...]"""
    t = torch_mod()
    b = t.from_numpy(np.ascontiguousarray(band_np)).to(device())
    if dtype is not None:
        b = b.to(dtype)
    assert H % band_np.shape[0] == 0
    return b.repeat(H // band_np.shape[0], *([1] * (b.ndim - 1)))


def differs_from_period(got, period_np, what, bound_np=None):
    """got: a flat device tensor that should be `period_np` repeated.  Compared on the device; only the count and the first position
    of a mismatch come back.  With bound_np: |got - period| <= bound elementwise in float64 instead of equality.  -> None or a message"""
    t = torch_mod()
    per = t.from_numpy(np.ascontiguousarray(period_np).reshape(-1)).to(got.device)
    n = per.numel()
    assert got.numel() % n == 0, (what, got.numel(), n)
    g = got.reshape(-1, n)
    if bound_np is None:
        bad = g != per[None]
    else:
        bnd = t.from_numpy(np.ascontiguousarray(bound_np, dtype=np.float64).reshape(-1)).to(got.device)
        bad = t.zeros(g.shape, dtype=t.bool, device=got.device)
        step = max(1, (1 << 27) // n)               # float64 temporaries of at most 1 GiB
        for r in range(0, g.shape[0], step):
            bad[r:r + step] = (g[r:r + step].double() - per[None].double()).abs() > bnd[None]
    count = int(bad.sum())
    if count == 0:
        return None
    first = int(bad.reshape(-1).to(t.uint8).argmax())
    return (f"{what}: {count} of {got.numel()} elements differ, first at {first} (period {first // n}, offset {first % n}): "
            f"got {g.reshape(-1)[first].item()!r}, want {per[first % n].item()!r}")


# ------------------------------------------------------------------ quadtree closed forms
def root_size(H, W):
    """twice the largest power of two strictly below max(H, W) (utils.py:41)"""
    n = max(H, W)
    lp = 1
    while lp * 2 < n:
        lp *= 2
    return lp * 2 if n > 2 else n * 2


def _compact(m):
    """the even bits of m, packed"""
    m = m & 0x5555555555555555
    for s, k in ((1, 0x3333333333333333), (2, 0x0F0F0F0F0F0F0F0F), (4, 0x00FF00FF00FF00FF), (8, 0x0000FFFF0000FFFF), (16, 0x00000000FFFFFFFF)):
        m = (m | (m >> s)) & k
    return m


def uniform_leaves(H, W, s):
    """[n, 4] int32 (x, y, size, coefficient offset): the leaves of a plane whose every leaf has size s, in the quadtree's depth-first
    order -- Morton order of the cells, x in the even bits, the cells outside the plane left out.  H, W: multiples of s."""
    assert H % s == 0 and W % s == 0
    side = root_size(H, W) // s
    m = np.arange(side * side, dtype=np.int64)
    x, y = _compact(m), _compact(m >> 1)
    keep = (x < W // s) & (y < H // s)
    x, y = x[keep] * s, y[keep] * s
    n = x.size
    assert n == (H // s) * (W // s)
    return np.stack([x, y, np.full(n, s), np.arange(n, dtype=np.int64) * s * s], 1).astype(np.int32)


def tree(H, W, bmin, bmax, has_edge):
    """the reference's top-down walk (quadtree.py:93-165) with the edge test given in closed form: has_edge(x, y, s) -> bool.
    -> leaves [n, 4] int32 (x, y, size, coefficient offset), states uint8 (0 leaf, 1 internal, 2 outside the image)"""
    leaves, states, coef = [], [], 0
    stack = [(0, 0, root_size(H, W))]
    while stack:
        x, y, s = stack.pop()
        if x >= W or y >= H:
            states.append(2)
            continue
        if s > bmax or (s > bmin and has_edge(x, y, s)):
            states.append(1)
            h = s // 2
            stack += [(x + h, y + h, h), (x, y + h, h), (x + h, y, h), (x, y, h)]
        else:
            states.append(0)
            leaves.append((x, y, s, coef))
            coef += s * s
    return np.array(leaves, np.int32).reshape(-1, 4), np.array(states, np.uint8)
