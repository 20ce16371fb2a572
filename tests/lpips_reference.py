"""Float64 restatements of LPIPS(net='alex') (lpips 0.1.4, evaluation_metrics.py:91-109) and seeded weights in the public layouts.

``lpips64`` uses torch's F.conv2d / F.max_pool2d in float64; ``lpips_loops`` is an independent numpy restatement (explicit loops over
kernel taps and pool windows) for small images.  Both apply the ScalingLayer in float32, exactly as the metric states it, and
everything after it in float64.
"""
import numpy as np

CONVS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))   # cin, cout, k, stride, pad
FEATURE_INDEX = (0, 3, 6, 8, 10)
SHIFT = np.array([-.030, -.088, -.188], np.float32)
SCALE = np.array([.458, .448, .450], np.float32)


def random_state_dicts(seed, conv1_bias=None, lin_scale=1.0):
    """(torchvision AlexNet state dict, lpips lin state dict) of seeded weights: Kaiming-normal convolutions (fan-in, ReLU gain), biases
    N(0, 0.01^2), non-negative lin weights.  conv1_bias: a value for every conv1 bias (negative values kill conv1's ReLUs)."""
    import torch
    g = np.random.default_rng(seed)
    alex, lin = {}, {}
    for l, ((cin, cout, k, _, _), idx) in enumerate(zip(CONVS, FEATURE_INDEX)):
        w = g.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))
        b = g.standard_normal(cout) * 0.01
        if l == 0 and conv1_bias is not None:
            b[:] = conv1_bias
        alex[f"features.{idx}.weight"] = torch.from_numpy(w.astype(np.float32))
        alex[f"features.{idx}.bias"] = torch.from_numpy(b.astype(np.float32))
        lin[f"lin{l}.model.1.weight"] = torch.from_numpy((g.uniform(0, 16.0 / cout, cout) * lin_scale).astype(np.float32).reshape(1, cout, 1, 1))
    alex["classifier.1.weight"] = torch.zeros(8, 4)          # ignored by the loader
    return alex, lin


def lpips_state_dict(alex, lin, scaling=True):
    """The same weights as one LPIPS(net='alex').state_dict()"""
    import torch
    d = {}
    for l, idx in enumerate(FEATURE_INDEX):
        for p in ("weight", "bias"):
            d[f"net.slice{l + 1}.{idx}.{p}"] = alex[f"features.{idx}.{p}"].clone()
        d[f"lin{l}.model.1.weight"] = lin[f"lin{l}.model.1.weight"].clone()
    if scaling:
        d["scaling_layer.shift"] = torch.from_numpy(SHIFT.reshape(1, 3, 1, 1).copy())
        d["scaling_layer.scale"] = torch.from_numpy(SCALE.reshape(1, 3, 1, 1).copy())
    return d


def _params(alex, lin):
    convs = [(alex[f"features.{i}.weight"].double().numpy(), alex[f"features.{i}.bias"].double().numpy()) for i in FEATURE_INDEX]
    lins = [lin[f"lin{l}.model.1.weight"].double().numpy().reshape(-1) for l in range(5)]
    return convs, lins


def _scaled(x):
    x = np.asarray(x, np.float32)
    return ((x * np.float32(2) - np.float32(1) - SHIFT) / SCALE).astype(np.float64)     # [H, W, 3], float32 arithmetic


def _head(f0, f1, w):
    """f: [C, h, w] float64 taps -> mean over pixels of sum_c w_c (n0 - n1)^2"""
    n0 = f0 / (np.sqrt((f0 ** 2).sum(0, keepdims=True)) + 1e-10)
    n1 = f1 / (np.sqrt((f1 ** 2).sum(0, keepdims=True)) + 1e-10)
    return float((w[:, None, None] * (n0 - n1) ** 2).sum(0).mean())


def taps64(x, alex):
    """The five taps [C, h, w] (float64, after each ReLU) of one [H, W, 3] image, with torch float64."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(_scaled(x)).permute(2, 0, 1)[None]
    out = []
    for l, ((_, _, _, s, p), idx) in enumerate(zip(CONVS, FEATURE_INDEX)):
        if l in (1, 2):
            t = F.max_pool2d(t, 3, 2)
        t = F.relu(F.conv2d(t, alex[f"features.{idx}.weight"].double(), alex[f"features.{idx}.bias"].double(), stride=s, padding=p))
        out.append(t[0].numpy())
    return out


def lpips64(x0, x1, alex, lin):
    """LPIPS of two [H, W, 3] float32 images, float64 after the ScalingLayer (torch F.conv2d)."""
    if x0.shape[0] < 31 or x0.shape[1] < 31:
        raise ValueError("LPIPS needs at least 31x31")
    _, lins = _params(alex, lin)
    a, b = taps64(x0, alex), taps64(x1, alex)
    return sum(_head(a[l], b[l], lins[l]) for l in range(5))


def _conv_loops(x, w, b, s, p):
    """x [C, H, W], w [O, C, k, k]: one loop per kernel tap, pixels and channels vectorised"""
    C, H, W = x.shape
    O, _, k, _ = w.shape
    xp = np.zeros((C, H + 2 * p, W + 2 * p))
    xp[:, p:p + H, p:p + W] = x
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    y = np.zeros((O, oh, ow))
    for ky in range(k):
        for kx in range(k):
            patch = xp[:, ky:ky + s * (oh - 1) + 1:s, kx:kx + s * (ow - 1) + 1:s]
            y += np.einsum("oc,chw->ohw", w[:, :, ky, kx], patch)
    return np.maximum(y + b[:, None, None], 0.0)


def _pool_loops(x):
    C, H, W = x.shape
    oh, ow = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    y = np.full((C, oh, ow), -np.inf)
    for i in range(oh):
        for j in range(ow):
            y[:, i, j] = x[:, 2 * i:2 * i + 3, 2 * j:2 * j + 3].reshape(C, -1).max(1)
    return y


def lpips_loops(x0, x1, alex, lin):
    """The same metric restated with numpy loops (small images only)."""
    convs, lins = _params(alex, lin)
    total = 0.0
    feats = []
    for x in (x0, x1):
        t = _scaled(x).transpose(2, 0, 1)
        taps = []
        for l, (_, _, _, s, p) in enumerate(CONVS):
            if l in (1, 2):
                t = _pool_loops(t)
            t = _conv_loops(t, convs[l][0], convs[l][1], s, p)
            taps.append(t)
        feats.append(taps)
    for l in range(5):
        total += _head(feats[0][l], feats[1][l], lins[l])
    return total
