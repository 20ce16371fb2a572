"""Float64 restatement of ``Jpeg.decompress`` after entropy decoding, with an elementwise bound on what a float32 implementation
may differ from it.  TEST INFRASTRUCTURE ONLY.

Written from the definitions, not from the oracle or the kernels:
  * inverse zigzag (the JPEG anti-diagonal walk) and dequantisation as the integer product ``block * qmatrix``;
  * ``cv.idct`` = the orthonormal inverse DCT-II ``X = C^T Y C``, ``C[k, n] = a_k cos(pi (2n + 1) k / 2s)``, ``a_0 = sqrt(1/s)``,
    ``a_k = sqrt(2/s)``, built here in float64;
  * quadtree merge (a leaf of size s sits at a multiple of s) and crop to the layer shape;
  * ``_denormalize``: ``v / scale + mid`` with the colour module's float32 constants;
  * ``cv.resize(INTER_LINEAR)`` as OpenCV 4.x ``resize`` / ``resizeGeneric_`` defines it: equal sizes are a copy; otherwise
    ``fx = (float)((dx + 0.5) * scale_x - 0.5)``, ``sx = cvFloor(fx)``, weights ``(1 - fx', fx')`` of the fraction; the x index is
    clamped to ``[0, w - 1]`` with its weight forced to 0 at both ends, the y rows are clamped with the weights left as computed;
  * the inverse colour transform of the matrix spaces, in float64 with the reference's float32 inverse matrices as recorded by
    executing it (tests/golden/color_constants.json), clipped to [0, 1].

Error bound of a float32 implementation (``u = 2**-24``, the unit roundoff):
  * IDCT, two passes of k-ordered float32 chains with a correctly rounded float32 matrix ``D`` (``|D - C| <= u |C|``) and exact
    float32 ``Y`` (integers below 2**24).  Pass 1 ``T = D^T Y``: ``|dT| <= (s + 1) u |C|^T |Y|`` (``s`` roundings of the chain,
    one of ``D``).  Pass 2 ``X = T D``: ``|dX| <= |dT| |C| + |T| |D - C| + s u |T| |C| <= (2s + 2) u |C|^T |Y| |C|`` to first
    order.  The bound used is ``(2s + 8) u |C|^T |Y| |C|``: 6 u of slack for the second-order terms (``s u <= 2**-14``).
  * denormalise: two roundings, ``e / scale + 3u (|X| / scale + |mid|)``.
  * upsample: the convex weights carry the plane's bound; each pass adds ``4u (|a| + |b|)`` of its two inputs (the rounded
    ``1 - fx``, two products, one sum).
  * colour: ``|M| e + 3u |M| |p|`` for the three-term chain, plus 2u.  The clip to [0, 1] is 1-Lipschitz and keeps the bound.

Mutants (``idct=``, ``upsample=``) are the plausible wrong kernels the tests use to show the bound has teeth.
"""
import json
import os

import numpy as np

U = 2.0 ** -24
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# MIDPOINTS / SCALE_FACTORS of the colour modules, float32 of these literals
NORM = {
    "YCbCr": ([0.5000000037252903, 7.450580596923828e-09, 0.0], [253.99999810755253, 254.000003784895, 254.0]),
    "YCoCg": ([0.5, 0.0, 0.0], [254.0, 254.0, 254.0]),
    "YCoCg-R": ([0.5, 0.0, 0.0], [254.0, 127.0, 127.0]),
    "OKLAB": ([0.4999999, 0.021152213, -0.056563325], [254.00005, 497.9055, 497.94604]),
    "ICtCp": ([0.07497266, -0.0008235276, 0.023989676], [1693.9674, 1133.9044, 1694.004]),
    "ICaCb": ([0.07498085, 0.02180194, -0.018250957], [1693.7823, 1838.5665, 1330.3855]),
    "JzAzBz": ([0.0087900255, 0.00048353244, -0.0020741792], [14448.194, 7590.505, 5552.201]),
}

# (rh, rw) per layer
RATIOS = {"YCbCr": [(1, 1), (2, 2), (2, 2)], "YCoCg": [(1, 1), (2, 2), (2, 2)], "YCoCg-R": [(1, 1), (2, 2), (2, 2)],
          "OKLAB": [(1, 1), (2, 2), (2, 2)], "JzAzBz": [(1, 1), (2, 2), (2, 2)],
          "ICtCp": [(1, 1), (1, 4), (1, 4)], "ICaCb": [(1, 1), (1, 4), (1, 4)]}

MATRIX_SPACES = ("YCbCr", "YCoCg", "YCoCg-R")

IDCT_MUTANTS = ("transposed", "dc_1_over_s", "drop_last_k")
UPSAMPLE_MUTANTS = ("align_corners", "no_half_pixel", "nearest")


def zigzag(s):
    """raster index of the i-th coefficient in JPEG zigzag order: anti-diagonals d = r + c, odd ones walked with the row rising,
    even ones with the row falling"""
    r, c = np.divmod(np.arange(s * s), s)
    d = r + c
    return np.lexsort((np.where(d % 2 == 1, r, -r), d)).astype(np.int64)


def dct_matrix(s, dc_weight=None):
    k = np.arange(s, dtype=np.float64)
    C = np.sqrt(2.0 / s) * np.cos(np.pi * (2.0 * k[None, :] + 1.0) * k[:, None] / (2.0 * s))
    C[0, :] = np.sqrt(1.0 / s) if dc_weight is None else dc_weight
    return C


def inverse_matrix(space):
    """the reference's float32 inverse matrix of a matrix space (row-major, space -> sRGB), as float64"""
    with open(os.path.join(_GOLDEN, "color_constants.json")) as f:
        bits = json.load(f)[space + ".inv"]
    return np.array([int(b, 16) for b in bits], np.uint32).view(np.float32).reshape(3, 3).astype(np.float64)


def layer_shapes(H, W, space):
    return [(H // rh, W // rw) for rh, rw in RATIOS[space]]


def dequantised_blocks(coeffs, offsets, s, qm):
    """(n, s, s) float64 Y of the leaves of size s whose coefficients start at ``offsets`` (zigzag order in the stream)"""
    zz = zigzag(s)
    c = np.asarray(coeffs, np.int64)[np.asarray(offsets, np.int64)[:, None] + np.arange(s * s)[None, :]]
    q = np.asarray(qm, np.int64).reshape(-1)
    Y = np.zeros((len(offsets), s * s), np.int64)
    Y[:, zz] = c * q[zz][None, :]
    return Y.reshape(-1, s, s).astype(np.float64)


def idct(Y, variant="exact"):
    """X = C^T Y C for a stack of blocks, or one of the mutants"""
    s = Y.shape[-1]
    C = dct_matrix(s, 1.0 / s if variant == "dc_1_over_s" else None)
    if variant == "transposed":
        Y = np.swapaxes(Y, -1, -2)
    elif variant == "drop_last_k":
        Y = Y.copy()
        Y[..., -1, :] = 0.0
        Y[..., :, -1] = 0.0
    elif variant not in ("exact", "dc_1_over_s"):
        raise ValueError(variant)
    return C.T @ Y @ C


def idct_bound(Y):
    s = Y.shape[-1]
    A = np.abs(dct_matrix(s))
    return (2 * s + 8) * U * (A.T @ np.abs(Y) @ A)


def blocks_decode(coeffs, leaves, qm_by_size, space, layer, h, w, offsets=None, idct_variant="exact"):
    """one layer's plane (h, w) float64 and its bound.  leaves: (n, 3) [x, y, s] in stream order; qm_by_size: s -> (s, s) int"""
    leaves = np.asarray(leaves, np.int64).reshape(-1, 3)
    sizes = leaves[:, 2]
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(sizes ** 2)[:-1]]).astype(np.int64)
    offsets = np.asarray(offsets, np.int64)
    mid = float(np.float32(NORM[space][0][layer]))
    scale = float(np.float32(NORM[space][1][layer]))
    plane = np.full((h, w), np.nan)
    bound = np.full((h, w), np.nan)
    for s in np.unique(sizes):
        s = int(s)
        sel = np.nonzero(sizes == s)[0]
        Y = dequantised_blocks(coeffs, offsets[sel], s, qm_by_size[s])
        assert np.abs(Y).max(initial=0) < 2 ** 24, "dequantised values beyond float32's exact integers"
        X = idct(Y, idct_variant)
        eX = idct_bound(Y)
        v = X / scale + mid
        ev = eX / scale * (1 + 4 * U) + 3 * U * (np.abs(X) / scale + abs(mid))
        nby, nbx = -(-h // s), -(-w // s)
        by, bx = leaves[sel, 1] // s, leaves[sel, 0] // s
        assert (leaves[sel, 0] % s == 0).all() and (leaves[sel, 1] % s == 0).all(), "leaf off its quadtree grid"
        for dst, src in ((plane, v), (bound, ev)):
            canvas = np.full((nby, nbx, s, s), np.nan)
            canvas[by, bx] = src
            full = canvas.transpose(0, 2, 1, 3).reshape(nby * s, nbx * s)[:h, :w]
            m = ~np.isnan(full)
            assert np.isnan(dst[m]).all(), "overlapping leaves"
            dst[m] = full[m]
    assert not np.isnan(plane).any(), "the leaves do not tile the layer"
    return plane, bound


def _linear_taps(n_src, n_dst, mode):
    """source indices (i0, i1) and float64 weights (w0, w1) per destination index for one axis, plus whether the index is
    clamped with its weight forced to 0 (x) -- the y rule is applied by the caller"""
    d = np.arange(n_dst, dtype=np.float64)
    if mode == "linear":
        scale = 1.0 / (n_dst / n_src)
        f = ((d + 0.5) * scale - 0.5).astype(np.float32).astype(np.float64)
    elif mode == "no_half_pixel":
        f = d * (n_src / n_dst)
    elif mode == "align_corners":
        f = d * ((n_src - 1) / (n_dst - 1)) if n_dst > 1 else np.zeros_like(d)
    elif mode == "nearest":
        i = np.minimum(np.floor(d * (n_src / n_dst)), n_src - 1).astype(np.int64)
        return i, i, np.ones_like(d), np.zeros_like(d)
    else:
        raise ValueError(mode)
    i0 = np.floor(f)
    fr = f - i0
    return i0.astype(np.int64), i0.astype(np.int64) + 1, 1.0 - fr, fr


def upsample(plane, bound, H, W, mode="linear"):
    """cv.resize(plane, (W, H), INTER_LINEAR) in float64 with the carried bound, or one of the mutants"""
    h, w = plane.shape
    if (h, w) == (H, W):
        return plane.copy(), bound.copy()
    x0, x1, a0, a1 = _linear_taps(w, W, mode)
    lo, hi = x0 < 0, x0 >= w - 1                 # x: clamp, weight forced to 0 at both ends
    x0 = np.clip(x0, 0, w - 1)
    a1 = np.where(lo | hi, 0.0, a1)
    a0 = np.where(lo | hi, 1.0, a0)
    x1 = np.clip(x1, 0, w - 1)
    y0, y1, b0, b1 = _linear_taps(h, H, mode)
    y0, y1 = np.clip(y0, 0, h - 1), np.clip(y1, 0, h - 1)   # y: rows clamped, weights as computed
    ap = np.abs(plane)
    r = plane[:, x0] * a0 + plane[:, x1] * a1
    er = bound[:, x0] * a0 + bound[:, x1] * a1 + 4 * U * (ap[:, x0] + ap[:, x1])
    out = r[y0, :] * b0[:, None] + r[y1, :] * b1[:, None]
    ar = np.abs(r)
    eo = er[y0, :] * b0[:, None] + er[y1, :] * b1[:, None] + 4 * U * (ar[y0, :] + ar[y1, :])
    return out, eo


def color_inverse(planes, bounds, space):
    """(H, W, 3) planes and bounds -> clip(M^-1 p, 0, 1) in float64 and its bound"""
    M = inverse_matrix(space)
    aM = np.abs(M)
    p = np.asarray(planes, np.float64)
    ap = np.abs(p)
    out = np.clip(p @ M.T, 0.0, 1.0)
    eb = bounds @ aM.T + 3 * U * (ap @ aM.T) + 2 * U
    return out, eb


def decode(layers, space, H, W, idct_variant="exact", upsample_mode="linear", return_planes=False):
    """layers: three dicts with ``coeffs`` (zigzag order, leaves in stream order), ``leaves`` (n, 3) [x, y, s], ``qm`` (s -> (s, s)
    int) and optionally ``offsets``.  -> rgb (H, W, 3) float64 in [0, 1] and its elementwise bound"""
    planes, bounds, layer_planes = [], [], []
    for l, ((h, w), L) in enumerate(zip(layer_shapes(H, W, space), layers)):
        p, e = blocks_decode(L["coeffs"], L["leaves"], L["qm"], space, l, h, w, L.get("offsets"), idct_variant)
        layer_planes.append((p, e))
        p, e = upsample(p, e, H, W, upsample_mode)
        planes.append(p)
        bounds.append(e)
    rgb, eb = color_inverse(np.stack(planes, -1), np.stack(bounds, -1), space)
    if return_planes:
        return rgb, eb, layer_planes, list(zip(planes, bounds))
    return rgb, eb


# ------------------------------------------------------------------ coefficient patterns for the tests
PATTERNS = ("basis", "dc", "highest", "checker", "dense", "max")


def leaf_pattern(kind, s, rng, basis=None):
    """desired (s, s) float64 Y of one leaf: a basis function (k, j), a lone DC, all energy in (s-1, s-1), a pixel checkerboard's
    spectrum, or random dense coefficients"""
    Y = np.zeros((s, s))
    if kind == "basis":
        k, j = basis if basis is not None else rng.integers(0, s, 2)
        Y[k, j] = 1.0
    elif kind == "dc":
        Y[0, 0] = 1.0
    elif kind == "highest":
        Y[s - 1, s - 1] = 1.0
    elif kind == "checker":
        n = np.arange(s)
        C = dct_matrix(s)
        Y = C @ np.where((n[:, None] + n[None, :]) % 2 == 0, 1.0, -1.0) @ C.T
    elif kind == "dense":
        Y = rng.standard_normal((s, s))
    else:
        raise ValueError(kind)
    return Y * (1.0 if rng.random() < 0.5 else -1.0)


def make_coeffs(leaves, qm_by_size, seed, amp=100.0, saturate_every=5, kinds=PATTERNS, basis_walk=False):
    """int32 coefficients (zigzag order, leaves in stream order) cycling the leaves through ``kinds``.  Each pattern is scaled so
    that the IDCT's peak is ``amp`` (normalised units; luma's scale is 254 per unit of [0, 1]), every ``saturate_every``-th leaf
    at 4 * amp so that the clip is exercised.  "max" puts rint(127 s / q) -- the largest dequantised magnitude the encoder emits
    for a block of 8-bit samples, 127 s at the DC -- at random positions with random signs.  basis_walk: leaf i of size s carries
    basis function i mod s^2 (raster order), so that s^2 leaves of one size cover all of them."""
    rng = np.random.default_rng(seed)
    leaves = np.asarray(leaves, np.int64).reshape(-1, 3)
    out, seen = [], {}
    for i, s in enumerate(leaves[:, 2]):
        s = int(s)
        q = np.asarray(qm_by_size[s], np.float64).reshape(s, s)
        n = seen.get(s, 0)
        seen[s] = n + 1
        kind = "basis" if basis_walk else kinds[i % len(kinds)]
        if kind == "max":
            c = np.rint(127.0 * s / q) * np.where(rng.random((s, s)) < 0.5, -1, 1) * (rng.random((s, s)) < 0.3)
            c[0, 0] = np.rint(127.0 * s / q[0, 0]) * (1 if rng.random() < 0.5 else -1)
        else:
            Y = leaf_pattern(kind, s, rng, divmod(n % (s * s), s) if basis_walk else None)
            a = amp * (4.0 if saturate_every and i % saturate_every == saturate_every - 1 else 1.0)
            Y *= a / np.abs(idct(Y)).max()
            c = np.rint(Y / q)
            if kind in ("basis", "dc", "highest"):      # a lone coefficient must survive the division by a coarse q
                c[Y != 0] = np.where(c[Y != 0] == 0, np.sign(Y[Y != 0]), c[Y != 0])
        out.append(c.reshape(-1)[zigzag(s)])
    return np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)


# ------------------------------------------------------------------ checks shared by the CPU and GPU tests
def assert_within(got, ref, bound, what=""):
    """|got - ref| <= bound everywhere (got: float32 from the code under test)"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    excess = np.abs(got - ref) - bound
    i = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess[i] <= 0, f"{what}: |got - ref| = {abs(got[i] - ref[i]):.3g} > bound {bound[i]:.3g} at {i} (got {got[i]!r}, ref {ref[i]!r})"


def assert_mutants_caught(variant_fn, variants, ref, bound, what=""):
    """every mutant's output leaves twice the bound somewhere: a kernel computing it would fail ``assert_within``"""
    for v in variants:
        m = variant_fn(v)
        assert (np.abs(m - ref) > 2 * bound).any(), f"{what}: the bound does not reject the {v} mutant"
