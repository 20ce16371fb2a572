"""Vectorised restatements of the OpenCV 4.x stages of ``EdgeDetection.canny``.  TEST INFRASTRUCTURE ONLY.

Written from OpenCV's algorithms, not from the oracle or the kernels; each function takes the previous stage's output so that every
stage can be checked on its own:
  * ``clahe``: ``CLAHE_Impl::apply`` / ``CLAHE_CalcLut_Body`` / ``CLAHE_Interpolation_Body`` (imgproc/src/clahe.cpp), 8-bit, 4 x 4
    tiles.  When either side is not a multiple of 4 the source is padded by ``copyMakeBorder(0, 4 - H % 4, 0, 4 - W % 4,
    BORDER_REFLECT_101)`` -- bottom and right only, and a side that is already a multiple of 4 gets 4 whole rows or columns.
    Clip limit ``max(int(clip * area / 256), 1)``, none when ``clip <= 0``; the clipped excess is redistributed as a uniform batch
    and a residual in steps of ``max(256 / residual, 1)``; ``lut = saturate_cast<uchar>(float(sum) * float(255 / area))``.  The
    bilinear blend of the four tile LUTs is evaluated in float64 and returned before rounding.
  * ``bilateral``: ``bilateralFilter_8u`` (imgproc/src/bilateral_filter.dispatch.cpp), d = 5: radius 2, circular mask ``r <= 2``,
    sigmas <= 0 become 1, weights ``(float)exp(double)``, BORDER_REFLECT_101; ``sum / wsum`` in float64, returned before rounding.
  * ``canny_*``: ``cv::Canny`` (imgproc/src/canny.cpp), aperture 3: Sobel with BORDER_REPLICATE, L2 (``dx^2 + dy^2``) or L1
    magnitude, zero magnitude outside the image, NMS with ``TG22 = 13573`` (``>`` / ``>=`` along x and along y, ``>`` / ``>`` on the
    diagonals), thresholds swapped if lo > hi, clamped to 32767 and squared for L2, floored; hysteresis as the 8-connected
    components of the candidate pixels that hold a strong pixel (``scipy.ndimage.label``), the same set as OpenCV's stack walk.
The float stages are compared by ``rounded_matches``: equal away from half-integers, one of the two neighbours near one.
"""
import numpy as np

TG22 = 13573


def reflect101(i, n):
    """BORDER_REFLECT_101 index (gfedcb|abcdefgh|gfedcba), any distance"""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def cv_round(x):
    """cvRound: round half to even (lrint in the default rounding mode)"""
    return np.rint(x)


def clahe_luts(src, clip_limit=0.75, tiles=4):
    """(tiles*tiles, 256) uint8 LUTs and the tile size (th, tw)"""
    H, W = src.shape
    if H % tiles or W % tiles:
        ys = reflect101(np.arange(H + tiles - H % tiles), H)
        xs = reflect101(np.arange(W + tiles - W % tiles), W)
        ext = src[ys[:, None], xs[None, :]]
    else:
        ext = src
    th, tw = ext.shape[0] // tiles, ext.shape[1] // tiles
    area = th * tw
    t = ext[:tiles * th, :tiles * tw].reshape(tiles, th, tiles, tw).transpose(0, 2, 1, 3).reshape(tiles * tiles, area)
    hist = np.zeros((tiles * tiles, 256), np.int64)
    np.add.at(hist, (np.repeat(np.arange(tiles * tiles), area), t.reshape(-1).astype(np.int64)), 1)
    if clip_limit > 0:
        clip = max(int(clip_limit * area / 256), 1)
        clipped = np.maximum(hist - clip, 0).sum(1)
        hist = np.minimum(hist, clip)
        batch = clipped // 256
        hist += batch[:, None]
        resid = clipped - batch * 256
        for r in range(tiles * tiles):
            if resid[r]:
                step = max(256 // int(resid[r]), 1)
                idx = np.arange(0, 256, step)[:resid[r]]
                hist[r, idx] += 1
    scale = np.float32(255.0) / np.float32(area)
    lut = cv_round(np.cumsum(hist, 1).astype(np.float32) * scale)
    return np.clip(lut, 0, 255).astype(np.uint8), (th, tw)


def clahe(src, clip_limit=0.75, tiles=4):
    """-> float64 value before cvRound (the blend of the tile LUTs), plus the LUTs"""
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    lut, (th, tw) = clahe_luts(src, clip_limit, tiles)
    tyf = np.arange(H) / th - 0.5
    txf = np.arange(W) / tw - 0.5
    ty1, tx1 = np.floor(tyf).astype(np.int64), np.floor(txf).astype(np.int64)
    ya, xa = tyf - ty1, txf - tx1
    ty2, tx2 = np.minimum(ty1 + 1, tiles - 1), np.minimum(tx1 + 1, tiles - 1)
    ty1, tx1 = np.maximum(ty1, 0), np.maximum(tx1, 0)
    v = src.astype(np.int64)
    L = lut.astype(np.float64)

    def at(ty, tx):
        return L[(ty[:, None] * tiles + tx[None, :]), v]

    top = at(ty1, tx1) * (1 - xa)[None, :] + at(ty1, tx2) * xa[None, :]
    bot = at(ty2, tx1) * (1 - xa)[None, :] + at(ty2, tx2) * xa[None, :]
    return top * (1 - ya)[:, None] + bot * ya[:, None], lut


def bilateral(src, sigma_color=75.0, sigma_space=75.0, d=5):
    """-> float64 sum / wsum before cvRound"""
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    sigma_color = 1.0 if sigma_color <= 0 else float(sigma_color)
    sigma_space = 1.0 if sigma_space <= 0 else float(sigma_space)
    gc, gs = -0.5 / (sigma_color * sigma_color), -0.5 / (sigma_space * sigma_space)
    radius = max(d // 2, 1)
    color_w = np.exp(np.arange(256, dtype=np.float64) ** 2 * gc).astype(np.float32).astype(np.float64)
    ys, xs = reflect101(np.arange(-radius, H + radius), H), reflect101(np.arange(-radius, W + radius), W)
    pad = src[ys[:, None], xs[None, :]].astype(np.int64)
    c = src.astype(np.int64)
    num = np.zeros((H, W))
    den = np.zeros((H, W))
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            r = np.sqrt(float(i * i + j * j))
            if r > radius:
                continue
            sw = float(np.float32(np.exp(r * r * gs)))
            v = pad[radius + i:radius + i + H, radius + j:radius + j + W]
            w = sw * color_w[np.abs(v - c)]
            num += v * w
            den += w
    return num / den


def rounded_matches(got, pre, tau=1e-3):
    """got (uint8) equals cvRound(pre) wherever pre is more than tau from a half-integer; elsewhere it is one of the two neighbouring
    integers.  -> (ok mask, number of exempt pixels)"""
    got = np.asarray(got, np.int64)
    frac = pre - np.floor(pre)
    near = np.abs(frac - 0.5) <= tau
    want = np.clip(cv_round(pre), 0, 255).astype(np.int64)
    ok = np.where(near, (got == np.clip(np.floor(pre), 0, 255)) | (got == np.clip(np.ceil(pre), 0, 255)), got == want)
    return ok, int(near.sum())


def canny_thresholds(lo, hi, l2=True):
    if lo > hi:
        lo, hi = hi, lo
    if l2:
        lo, hi = min(32767.0, lo), min(32767.0, hi)
        if lo > 0:
            lo *= lo
        if hi > 0:
            hi *= hi
    return int(np.floor(lo)), int(np.floor(hi))


def percentile_thresholds(blur, low_ratio=0.10, high_ratio=0.30):
    """np.percentile(blur, ratio * 100) as the reference's EdgeDetection.canny computes its thresholds"""
    return float(np.percentile(blur, low_ratio * 100)), float(np.percentile(blur, high_ratio * 100))


def sobel(src):
    p = np.pad(np.asarray(src, np.int64), 1, mode="edge")           # BORDER_REPLICATE
    a, b, c = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    d, f = p[1:-1, :-2], p[1:-1, 2:]
    g, h, i = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    return (c + 2 * f + i) - (a + 2 * d + g), (g + 2 * h + i) - (a + 2 * b + c)


def canny_nms(src, low, high, l2=True):
    """-> map: 0 candidate (weak), 1 suppressed, 2 strong (OpenCV's map values)"""
    dx, dy = sobel(src)
    mag = dx * dx + dy * dy if l2 else np.abs(dx) + np.abs(dy)
    H, W = mag.shape
    m = np.zeros((H + 2, W + 2), np.int64)
    m[1:-1, 1:-1] = mag

    def nb(oy, ox):
        return m[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]

    ax, ay = np.abs(dx), np.abs(dy) << 15
    tg22x = ax * TG22
    tg67x = tg22x + (ax << 16)
    horiz = ay < tg22x
    vert = ~horiz & (ay > tg67x)
    diag = ~horiz & ~vert
    s = np.where((dx ^ dy) < 0, -1, 1)
    keep_h = (mag > nb(0, -1)) & (mag >= nb(0, 1))
    keep_v = (mag > nb(-1, 0)) & (mag >= nb(1, 0))
    # diagonal: m > mag[y-1][x-s] and m > mag[y+1][x+s]
    keep_d = np.where(s < 0, (mag > nb(-1, 1)) & (mag > nb(1, -1)), (mag > nb(-1, -1)) & (mag > nb(1, 1)))
    keep = (mag > low) & ((horiz & keep_h) | (vert & keep_v) | (diag & keep_d))
    return np.where(keep, np.where(mag > high, 2, 0), 1).astype(np.uint8)


def hysteresis(nms_map):
    """edge (0/1): the 8-connected components of the candidates (0 or 2) that contain a strong pixel (2)"""
    from scipy import ndimage
    cand = nms_map != 1
    lab, n = ndimage.label(cand, structure=np.ones((3, 3), bool))
    strong = np.zeros(n + 1, bool)
    strong[lab[nms_map == 2]] = True
    strong[0] = False
    return strong[lab].astype(np.uint8)


# ------------------------------------------------------------------ inputs and the stage-by-stage comparison
def test_plane(H, W, seed):
    """float32 plane in [0, 1] with flat plateaus (a constant tile makes CLAHE clip and redistribute with a residual), ramps for the
    NMS tie rules, ramps at angles near 22.5 and 67.5 degrees, a faint chain whose pieces touch only diagonally, lines that run into
    the border, and a little noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    p = 0.35 + 0.02 * rng.standard_normal((H, W))
    p[: H // 3, : W // 3] = 0.62                                         # plateau
    p += np.where(x > 0.6 * W, 0.002 * (x - 0.6 * W), 0)                  # ramp
    for ang, off in ((np.deg2rad(22.3), 0.2), (np.deg2rad(67.7), 0.7)):   # near the NMS sector boundaries
        t = (x * np.cos(ang) + y * np.sin(ang)) / max(H, W)
        p += 0.12 * (np.abs(t - off) < 0.03)
    for k in range(min(H, W) // 3):                                      # staircase touching only at corners
        yy, xx = H // 2 + k, W // 4 + 2 * k // 2 + k % 2
        if yy < H and xx < W:
            p[yy, xx] += 0.06
    p[:, 0] += 0.15                                                      # lines on the border
    p[-1, :] -= 0.1
    return np.clip(p, 0, 1).astype(np.float32)


def check_stages(stages, edge, thr, params, tau_clahe=1e-4, tau_bilateral=1e-3, label=""):
    """stages: [scaled, clahe, gauss, bilateral(, nms map)] uint8 of one run, edge {0,1}, thr: the integer thresholds (or None) ->
    exempt counts.  params as aej_canny_params: (low ratio, high ratio, clip limit, sigma colour, sigma space, L2).
    tau: a float32 blend of four LUT values <= 255 is off by a few 1e-5 at most, so 1e-4 keeps CLAHE's exempt pixels to the exact
    ties at tile boundaries; the bilateral ratio of two 13-term float32 sums may be off by a few 1e-4."""
    lo_r, hi_r, clip, sc, ss, l2 = params
    H, W = stages[0].shape
    pre_c, _ = clahe(stages[0], clip)
    ok, ex_c = rounded_matches(stages[1], pre_c, tau_clahe)
    assert ok.all(), f"{label} CLAHE differs at {np.argwhere(~ok)[:5].tolist()}"
    pre_b = bilateral(stages[2], sc, ss)
    ok, ex_b = rounded_matches(stages[3], pre_b, tau_bilateral)
    assert ok.all(), f"{label} bilateral differs at {np.argwhere(~ok)[:5].tolist()}"
    low, high = canny_thresholds(*percentile_thresholds(stages[3], lo_r, hi_r), l2=bool(l2))
    if thr is not None:
        assert tuple(thr) == (low, high), label
    nms = canny_nms(stages[3], low, high, bool(l2))
    if len(stages) > 4:
        assert np.array_equal(stages[4], nms), f"{label} NMS differs at {np.argwhere(stages[4] != nms)[:5].tolist()}"
    ref_edge = hysteresis(nms)
    assert np.array_equal(np.asarray(edge).astype(np.uint8), ref_edge), f"{label} edge map differs"
    n = H * W
    print(f"{label}: {H}x{W} exempt CLAHE {ex_c}, bilateral {ex_b} of {n}")
    # nearly all exempt pixels are exact ties of the blend (weights of 0.5 at tile centres in narrow tiles): few, never most
    assert ex_c <= 2 + n // 5 and ex_b <= 2 + n // 100, (ex_c, ex_b)
    return ex_c, ex_b
