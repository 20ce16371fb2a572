"""CPU restatement of the reference's EvaluationMetrics (src/image/evaluation_metrics.py:50-89) -- TEST INFRASTRUCTURE ONLY.

Only tests/ may import this module; the product (adaptive_edge_aware_jpeg_amd) never does.

The arithmetic lives in two third-party packages that are absent from /root/reference and from this container:
piq==0.8.0 (requirements.txt:22) and opencv-python==4.11.0.86 (requirements.txt:18).  Their published algorithms are
restated here in numpy:
  * piq/psnr.py `psnr`: x, y / data_range; mse = mean((x - y)^2) over (C, H, W); -10 log10(mse + 1e-8)
  * piq/functional/filters.py `gaussian_filter`: coords = arange(k) - (k - 1) / 2; g = exp(-(c_i^2 + c_j^2) / (2 sigma^2)); g /= g.sum()
    (float32, as the tensors are)
  * piq/ssim.py `ssim`: x, y / data_range; f = max(1, round(min(H, W) / 256)); avg_pool2d(f) if f > 1;
    `_ssim_per_channel`: 'valid' correlation with the window of x, y, x^2, y^2, xy; c1 = k1^2, c2 = k2^2 (k1 = .01, k2 = .03);
    cs = (2 s_xy + c2) / (s_xx + s_yy + c2); ss = (2 mu_xy + c1) / (mu_xx + mu_yy + c1) * cs; spatial means; channel mean
  * piq/ms_ssim.py `multi_scale_ssim`: weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); between scales
    pad = max(H % 2, W % 2) replicated on the left and top, then avg_pool2d(2); relu; prod(mcs^w) with the last scale's ssim; channel mean
  * cv.cvtColor(COLOR_RGB2GRAY) on uint8: (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14
Call sites and arguments are the reference's own (evaluation_metrics.py:57-61, 70-76, 85-89).  No golden vector exists for
these in the reference's tests and neither package can run here: **parity unpinned** for this row -- the GPU path is checked
against this restatement to a float tolerance, plus independent properties (identical images, known MSE).
"""
import numpy as np


def get_uint8(data):                      # image.py:120-127
    return (data * 255).astype(np.uint8)


def rgb2gray_u8(u8):
    r, g, b = (u8[..., i].astype(np.int64) for i in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14).astype(np.uint8)


def gaussian_window(k=11, sigma=1.5):
    c = np.arange(k, dtype=np.float32) - np.float32((k - 1) / 2.0)
    g = c ** 2
    g = np.exp(-(g[None, :] + g[:, None]) / np.float32(2 * sigma ** 2)).astype(np.float32)
    return (g / g.sum(dtype=np.float32)).astype(np.float32)


def _valid_corr(x, win):
    """'valid' 2-D correlation of (C, H, W) with a (k, k) window, accumulated in float64."""
    k = win.shape[0]
    C, H, W = x.shape
    out = np.zeros((C, H - k + 1, W - k + 1), np.float64)
    xd = x.astype(np.float64)
    for i in range(k):
        for j in range(k):
            out += float(win[i, j]) * xd[:, i:i + H - k + 1, j:j + W - k + 1]
    return out


def _ssim_per_channel(x, y, win, k1=0.01, k2=0.03):
    if x.shape[-1] < win.shape[-1] or x.shape[-2] < win.shape[-2]:
        raise ValueError(f"Kernel size can't be greater than actual input size. Input size: {x.shape}. Kernel size: {win.shape}")
    c1, c2 = k1 ** 2, k2 ** 2
    mu_x, mu_y = _valid_corr(x, win), _valid_corr(y, win)
    mu_xx, mu_yy, mu_xy = mu_x ** 2, mu_y ** 2, mu_x * mu_y
    s_xx = _valid_corr(x.astype(np.float64) ** 2, win) - mu_xx
    s_yy = _valid_corr(y.astype(np.float64) ** 2, win) - mu_yy
    s_xy = _valid_corr(x.astype(np.float64) * y.astype(np.float64), win) - mu_xy
    cs = (2.0 * s_xy + c2) / (s_xx + s_yy + c2)
    ss = (2.0 * mu_xy + c1) / (mu_xx + mu_yy + c1) * cs
    return ss.mean(axis=(-1, -2)), cs.mean(axis=(-1, -2))


def _avg_pool(x, f):
    C, H, W = x.shape
    h, w = H // f, W // f
    return x[:, :h * f, :w * f].reshape(C, h, f, w, f).astype(np.float64).mean(axis=(2, 4)).astype(np.float32)


def psnr(a, b):
    """a, b: (H, W, 3) float32 in [0, 1]."""
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float(-10.0 * np.log10(mse + 1e-8))


def ssim(a, b):
    ga = rgb2gray_u8(get_uint8(a))[None].astype(np.float32) / np.float32(255.0)
    gb = rgb2gray_u8(get_uint8(b))[None].astype(np.float32) / np.float32(255.0)
    f = max(1, round(min(ga.shape[-2:]) / 256))
    if f > 1:
        ga, gb = _avg_pool(ga, f), _avg_pool(gb, f)
    ss, _ = _ssim_per_channel(ga, gb, gaussian_window())
    return float(ss.mean())


def ms_ssim(a, b):
    x = np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32)
    y = np.ascontiguousarray(b.transpose(2, 0, 1)).astype(np.float32)
    weights = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=np.float32).astype(np.float64)
    win = gaussian_window()
    levels = len(weights)
    min_size = (win.shape[-1] - 1) * 2 ** (levels - 1) + 1
    if x.shape[-1] < min_size or x.shape[-2] < min_size:
        raise ValueError(f"Invalid size of the input images, expected at least {min_size}x{min_size}.")
    mcs = []
    ss = None
    for it in range(levels):
        if it > 0:
            p = max(x.shape[1] % 2, x.shape[2] % 2)
            x = np.pad(x, ((0, 0), (p, 0), (p, 0)), mode="edge")
            y = np.pad(y, ((0, 0), (p, 0), (p, 0)), mode="edge")
            x, y = _avg_pool(x, 2), _avg_pool(y, 2)
        ss, cs = _ssim_per_channel(x, y, win)
        mcs.append(cs)
    stack = np.maximum(np.stack(mcs[:-1] + [ss], axis=0), 0.0)           # (level, channel)
    return float(np.prod(stack ** weights[:, None], axis=0).mean())


# ---------------------------------------------------------------------------------------------------------------------------------------
# Fast float64 restatement (4K and 8K pairs in seconds): the same scores with the Gaussian applied as two separable 11-tap passes of the
# float64 1-D window g (g g^T is the exact 2-D window), where the definition above applies piq's float32 2-D window entry by entry.  The
# two windows differ by the float32 rounding of each entry, relative 2^-24 at most; tests/test_metrics.py states the resulting bound on the
# scores and checks it.  The keyword arguments select a DELIBERATELY WRONG geometry -- the tests use it to show that each probe can tell
# piq's rules from a near miss:
#   f_round="half_up"      f = floor(min(H, W) / 256 + 1/2) instead of Python's round (ties to even: 384 -> 2, 640 -> 2, 896 -> 4)
#   crop="top_left"        the grey pool drops the first H - (H // f) f rows / columns instead of the last (avg_pool2d floors at the end)
#   pad="bottom_right"     the odd MS-SSIM scales replicate the last row / column instead of the first
def gaussian_1d(k=11, sigma=1.5):
    c = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = np.exp(-(c ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _valid_sep(x, g):
    """'valid' correlation of (..., H, W) float64 with the separable window g g^T"""
    k = len(g)
    H, W = x.shape[-2:]
    t = g[0] * x[..., :, 0:W - k + 1]
    for j in range(1, k):
        t += g[j] * x[..., :, j:j + W - k + 1]
    out = g[0] * t[..., 0:H - k + 1, :]
    for i in range(1, k):
        out += g[i] * t[..., i:i + H - k + 1, :]
    return out


U32 = 2.0 ** -24          # float32 unit roundoff


def ssim_stats(x, y, g=None, e_in=0.0, diff_only=False, rho=None, k1=0.01, k2=0.03):
    """One channel pair (H, W) -> (ss mean, cs mean, ss bound, cs bound), float64.

    g: the 1-D taps (default gaussian_1d(); the GPU kernel's are float32(gaussian_1d()), pass those to compare with it).
    The bounds are first-order worst cases of |float32 kernel - this| for the means, the way metrics.hip computes them: inputs off by at
    most e_in u relative (u = 2^-24; the grey pool's float sums, earlier MS-SSIM pools); each Gaussian mean an 11-term fma chain per
    direction (22 roundings on non-negative terms: 22 u relative), x^2 + y^2 and xy one or two more; mu^2 squares of those (2 x 22 + 1);
    two subtractions; cs and the luminance term by the hardware reciprocal (1 ulp) and two products; each lane adds at most 64 window
    values in float32 before the sum leaves float (a further 64 u of the |values|).  diff_only: sum the bounds only over windows that see a
    pixel where x != y -- for two calls whose pairs differ only there, every other window is computed identically and cancels (its float
    accumulation rounding is the 64 u term).
    rho: instead, the bounds against the definition above: no float32 arithmetic, inputs rounded to float32 (e_in u) and a window
    differing from g g^T by a zero-sum perturbation of at most rho relative per entry, which moves a local variance or covariance by at most
    rho times sigma_x^2 + sigma_y^2 (or its half) and a local mean by at most rho sigma."""
    g = gaussian_1d() if g is None else np.asarray(g, np.float64)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    if x.shape[-1] < len(g) or x.shape[-2] < len(g):
        raise ValueError(f"Kernel size can't be greater than actual input size. Input size: {x.shape}. Kernel size: 11x11")
    c1, c2 = k1 ** 2, k2 ** 2
    mu_x, mu_y = _valid_sep(x, g), _valid_sep(y, g)
    mu_xx, mu_yy, mu_xy = mu_x * mu_x, mu_y * mu_y, mu_x * mu_y
    v2 = _valid_sep(x * x + y * y, g)
    v3 = _valid_sep(x * y, g)
    s_sum = v2 - mu_xx - mu_yy
    s_xy = v3 - mu_xy
    cs = (2.0 * s_xy + c2) / (s_sum + c2)
    lum = (2.0 * mu_xy + c1) / (mu_xx + mu_yy + c1)
    ss = lum * cs
    e = e_in
    if rho is not None:
        sd = np.sqrt(np.maximum(s_sum, 0.0))
        d_sum = 2 * e * U32 * (v2 + mu_xx + mu_yy) + rho * np.maximum(s_sum, 0.0)
        d_xy = 2 * e * U32 * (v3 + mu_xy) + rho * np.maximum(s_sum, 0.0) / 2
        d_cs = (2 * d_xy + d_sum * np.abs(cs)) / (s_sum + c2)
        d_mu = e * U32 * (mu_x + mu_y) + rho * sd                     # |d mu_x| + |d mu_y|
        d_lum = 2 * d_mu * (np.abs(mu_x) + np.abs(mu_y)) * (1 + np.abs(lum)) / (mu_xx + mu_yy + c1)
        d_ss = np.abs(lum) * d_cs + np.abs(cs) * d_lum
        return float(ss.mean()), float(cs.mean()), float(d_ss.mean()), float(d_cs.mean())
    d_sum = (26 + 2 * e) * U32 * v2 + (46 + 2 * e) * U32 * (mu_xx + mu_yy)
    d_xy = (25 + 2 * e) * U32 * v3 + (46 + 2 * e) * U32 * mu_xy
    d_cs = (2 * d_xy + d_sum * np.abs(cs)) / (s_sum + c2) + 5 * U32 * np.abs(cs)
    d_m = (46 + 2 * e) * U32
    d_lum = (2 * d_m * mu_xy + d_m * (mu_xx + mu_yy) * np.abs(lum)) / (mu_xx + mu_yy + c1) + 5 * U32 * np.abs(lum)
    d_ss = np.abs(lum) * d_cs + np.abs(cs) * d_lum + U32 * np.abs(ss)
    n = cs.size
    if diff_only:
        m = _valid_sep((x != y).astype(np.float64), np.ones(len(g))) > 0
        k = int(m.sum())
        acc_ss, acc_cs = 2 * 64 * U32 * 64 * k / n, 2 * 64 * U32 * 64 * k / n        # each lane-band with a changed window, in both calls
        b_ss, b_cs = float(d_ss[m].sum()) / n + acc_ss, float(d_cs[m].sum()) / n + acc_cs
    else:
        b_ss = float(d_ss.mean()) + 64 * U32 * float(np.abs(ss).mean())
        b_cs = float(d_cs.mean()) + 64 * U32 * float(np.abs(cs).mean())
    return float(ss.mean()), float(cs.mean()), b_ss, b_cs


def ssim_maps(x, y, k1=0.01, k2=0.03):
    """(ss, cs) maps of one channel pair (H, W), float64"""
    g = gaussian_1d()
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    if x.shape[-1] < len(g) or x.shape[-2] < len(g):
        raise ValueError(f"Kernel size can't be greater than actual input size. Input size: {x.shape}. Kernel size: 11x11")
    c1, c2 = k1 ** 2, k2 ** 2
    mu_x, mu_y = _valid_sep(x, g), _valid_sep(y, g)
    mu_xx, mu_yy, mu_xy = mu_x * mu_x, mu_y * mu_y, mu_x * mu_y
    s_sum = _valid_sep(x * x + y * y, g) - mu_xx - mu_yy
    s_xy = _valid_sep(x * y, g) - mu_xy
    cs = (2.0 * s_xy + c2) / (s_sum + c2)
    ss = (2.0 * mu_xy + c1) / (mu_xx + mu_yy + c1) * cs
    return ss, cs


def grey_pool_factor(H, W, f_round="even"):
    m = min(H, W) / 256
    f = round(m) if f_round == "even" else int(np.floor(m + 0.5))
    return max(1, f)


def grey_planes(a, b, f_round="even", crop="bottom_right"):
    """piq.ssim's input: 8-bit grey / 255, average-pooled by f (float64 means of the float32 levels; avg_pool2d floors)"""
    out = []
    for img in (a, b):
        gr = rgb2gray_u8(get_uint8(img)).astype(np.float32) / np.float32(255.0)
        H, W = gr.shape
        f = grey_pool_factor(H, W, f_round)
        if f > 1:
            h, w = H // f, W // f
            y0, x0 = (H - h * f, W - w * f) if crop == "top_left" else (0, 0)
            gr = gr[y0:y0 + h * f, x0:x0 + w * f].astype(np.float64).reshape(h, f, w, f).mean(axis=(1, 3))
        out.append(gr.astype(np.float64))
    return out


def ssim_fast(a, b, f_round="even", crop="bottom_right", g=None, diff_only=False, rho=None):
    """-> (ssim, bound): bound as ssim_stats, for the grey planes the GPU pools in float (f^2 + 2 roundings per value when f > 1)"""
    xa, xb = grey_planes(a, b, f_round, crop)
    f = grey_pool_factor(*np.shape(a)[:2], f_round)
    ss, _, b_ss, _ = ssim_stats(xa, xb, g, e_in=(1 if rho is not None else f * f + 2) if f > 1 else 0, diff_only=diff_only, rho=rho)
    return ss, b_ss


def ms_ssim_scales(a, b, pad="top_left", g=None, diff_only=False, rho=None):
    """per scale l, ((3,) channel means, (3,) bounds) of cs (scales 0..3) or ss (scale 4); a, b (H, W, 3).  The GPU pools each scale in
    float (three additions and an exact quarter: 3 u relative per scale, accumulated)."""
    x = np.asarray(a, np.float64).transpose(2, 0, 1)
    y = np.asarray(b, np.float64).transpose(2, 0, 1)
    if min(x.shape[1:]) < 161:
        raise ValueError("Invalid size of the input images, expected at least 161x161.")
    out = []
    for it in range(5):
        if it > 0:
            p = max(x.shape[1] % 2, x.shape[2] % 2)
            w = ((0, 0), (p, 0), (p, 0)) if pad == "top_left" else ((0, 0), (0, p), (0, p))
            x, y = (np.pad(v, w, mode="edge") for v in (x, y))
            h2, w2 = x.shape[1] // 2, x.shape[2] // 2
            x, y = (v[:, :2 * h2, :2 * w2].reshape(3, h2, 2, w2, 2).mean(axis=(2, 4)) for v in (x, y))
        st = [ssim_stats(x[c], y[c], g, e_in=(1 if rho is not None else 3) * it, diff_only=diff_only, rho=rho) for c in range(3)]
        k = 0 if it == 4 else 1
        out.append((np.array([t[k] for t in st]), np.array([t[k + 2] for t in st])))
    return out


def ms_ssim_from_scales(scales):
    """-> (ms_ssim, first-order bound) from ms_ssim_scales' output"""
    weights = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=np.float32).astype(np.float64)
    v = np.stack([s[0] for s in scales], axis=0)
    d = np.stack([s[1] for s in scales], axis=0)
    prod = np.prod(np.maximum(v, 0.0) ** weights[:, None], axis=0)
    hi = np.prod(np.maximum(v + d, 0.0) ** weights[:, None], axis=0)
    lo = np.prod(np.maximum(v - d, 0.0) ** weights[:, None], axis=0)
    return float(prod.mean()), float(np.maximum(hi - prod, prod - lo).mean())


def ms_ssim_fast(a, b, pad="top_left", g=None, diff_only=False):
    return ms_ssim_from_scales(ms_ssim_scales(a, b, pad, g, diff_only))


def ms_ssim_scales_def(a, b):
    """the definition's per-scale (3,) channel means (cs for scales 0..3, ss for 4), as ms_ssim() forms them"""
    x = np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32)
    y = np.ascontiguousarray(b.transpose(2, 0, 1)).astype(np.float32)
    win = gaussian_window()
    out = []
    for it in range(5):
        if it > 0:
            p = max(x.shape[1] % 2, x.shape[2] % 2)
            x = np.pad(x, ((0, 0), (p, 0), (p, 0)), mode="edge")
            y = np.pad(y, ((0, 0), (p, 0), (p, 0)), mode="edge")
            x, y = _avg_pool(x, 2), _avg_pool(y, 2)
        ss, cs = _ssim_per_channel(x, y, win)
        out.append(ss if it == 4 else cs)
    return out
