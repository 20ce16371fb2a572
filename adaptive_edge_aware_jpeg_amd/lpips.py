"""``LpipsWeights`` -- the parameters of ``lpips.LPIPS(net='alex')`` (lpips 0.1.4), supplied by the user, for the GPU LPIPS.

The reference builds the metric with ``lpips.LPIPS(net='alex')`` (evaluation_metrics.py:34-36), which downloads torchvision's AlexNet
(``alexnet-owt-7be5be79.pth``) and ships its own linear layers (``weights/v0.1/alex.pth``).  No copy of either exists offline, so this
package ships none: ``LpipsWeights.load`` reads the two files (or in-memory state dicts) the user has.  Accepted layouts:

* torchvision AlexNet: ``features.{0,3,6,8,10}.{weight,bias}`` (``classifier.*`` is ignored);
* lpips linear layers: ``lin{0..4}.model.1.weight``, shapes ``[1, C, 1, 1]``;
* a whole ``LPIPS(net='alex').state_dict()`` passed as ``alexnet`` with ``lin=None``: ``net.slice1.0.*``, ``net.slice2.3.*``,
  ``net.slice3.6.*``, ``net.slice4.8.*``, ``net.slice5.10.*`` and ``lin{k}.model.1.weight``, optionally ``scaling_layer.shift`` /
  ``scaling_layer.scale``, which must then hold the constants the kernels use.

These key names are written from memory of the public packages; they could not be checked against the real files here.  The tests
(tests/test_lpips_host.py) define the format this loader accepts.
"""
import ctypes
import os

import numpy as np

# (Cin, Cout, kernel) of AlexNet's five convolutions and their indices in torchvision's `features` Sequential
CONVS = ((3, 64, 11), (64, 192, 5), (192, 384, 3), (384, 256, 3), (256, 256, 3))
FEATURE_INDEX = (0, 3, 6, 8, 10)
SHIFT = np.array([-.030, -.088, -.188], np.float32)      # lpips ScalingLayer
SCALE = np.array([.458, .448, .450], np.float32)
MIN_SIZE = 31                                             # below this AlexNet's second maxpool has no output (torch raises)


def _read(src, what):
    if src is None:
        return None
    if isinstance(src, (str, os.PathLike)):
        import torch
        src = torch.load(src, map_location="cpu", weights_only=True)
    if not hasattr(src, "keys"):
        raise TypeError(f"{what}: expected a state dict or a path to one, got {type(src)}")
    return src


def _array(d, key, shape):
    if key not in d:
        raise ValueError(f"LPIPS weights: missing key {key!r}")
    v = d[key]
    v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    if tuple(v.shape) != tuple(shape):
        raise ValueError(f"LPIPS weights: {key!r} has shape {tuple(v.shape)}, expected {tuple(shape)}")
    v = v.astype(np.float32)
    if not np.all(np.isfinite(v)):
        raise ValueError(f"LPIPS weights: {key!r} holds non-finite values")
    return v


class LpipsWeights:
    """AlexNet conv weights / biases and the five lin weights as float32 arrays; packed for the kernels once per device."""

    def __init__(self, conv_weights, conv_biases, lins):
        self.conv_weights = [np.ascontiguousarray(w, np.float32) for w in conv_weights]
        self.conv_biases = [np.ascontiguousarray(b, np.float32) for b in conv_biases]
        self.lins = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in lins]
        for l, (cin, cout, k) in enumerate(CONVS):
            if self.conv_weights[l].shape != (cout, cin, k, k) or self.conv_biases[l].shape != (cout,) or self.lins[l].shape != (cout,):
                raise ValueError(f"LPIPS weights: layer {l} has the wrong shapes")
        self._device = {}

    @classmethod
    def load(cls, alexnet, lin=None):
        """alexnet: torchvision AlexNet state dict (or a whole LPIPS state dict, then lin=None); lin: lpips linear-layer state dict.
        Each may be a path (read with torch.load(map_location="cpu", weights_only=True)) or an in-memory dict."""
        a = _read(alexnet, "alexnet")
        ln = _read(lin, "lin")
        if a is None:
            raise TypeError("alexnet weights are required")
        full = any(str(k).startswith("net.slice") for k in a.keys())
        ws, bs = [], []
        for l, ((cin, cout, k), idx) in enumerate(zip(CONVS, FEATURE_INDEX)):
            pre = f"net.slice{l + 1}.{idx}" if full else f"features.{idx}"
            ws.append(_array(a, pre + ".weight", (cout, cin, k, k)))
            bs.append(_array(a, pre + ".bias", (cout,)))
        src = ln if ln is not None else a
        lins = [_array(src, f"lin{l}.model.1.weight", (1, cout, 1, 1)).reshape(cout) for l, (_, cout, _) in enumerate(CONVS)]
        for d in (a, ln):
            if d is None:
                continue
            for key, want in (("scaling_layer.shift", SHIFT), ("scaling_layer.scale", SCALE)):
                if key in d:
                    got = _array(d, key, (1, 3, 1, 1)).reshape(3)
                    if not np.array_equal(got, want):
                        raise ValueError(f"LPIPS weights: {key!r} is {got.tolist()}, the metric's ScalingLayer is {want.tolist()}")
        return cls(ws, bs, lins)

    def params(self):
        """The canonical parameter list of include/aej.h: conv1..5 (weight OIHW, bias), then lin0..4; float32."""
        parts = []
        for w, b in zip(self.conv_weights, self.conv_biases):
            parts += [w.ravel(), b]
        return np.concatenate(parts + self.lins).astype(np.float32)

    def packed_host(self):
        """The kernels' weight layout (aej_lpips_pack_weights_host), as host bytes."""
        from ._lib import load_library
        lib = load_library()
        p = self.params()
        out = np.zeros(int(lib.aej_lpips_weights_bytes()), np.uint8)
        if lib.aej_lpips_pack_weights_host(p.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(p.size), out.ctypes.data_as(ctypes.c_void_p)):
            raise ValueError(f"LPIPS weights: {p.size} parameters, the library expects {lib.aej_lpips_param_count()}")
        return out

    def on(self, ctx):
        """The packed weights on ctx's device (packed and copied once per device; caller-owned tensor kept here)."""
        key = ctx.device.index
        if key not in self._device:
            self._device[key] = ctx.to_device(self.packed_host(), ctx.torch.uint8)
        return self._device[key]


def check_size(H, W, what="image"):
    if H < MIN_SIZE or W < MIN_SIZE:
        raise ValueError(f"{what} ({H}x{W}): LPIPS needs images of at least {MIN_SIZE}x{MIN_SIZE}.")


def features(ctx, weights, x):
    """Normalised taps of the device batch x [B, H, W, 3] float32: a flat float32 device tensor (aej_lpips_features)."""
    t = ctx.torch
    B, H, W, _ = x.shape
    check_size(H, W)
    lib = ctx.lib
    feats = ctx.empty((int(lib.aej_lpips_features_bytes(B, H, W)) // 4,), t.float32)
    nbytes = int(lib.aej_lpips_workspace_bytes(B, H, W))
    ws = ctx.workspace(nbytes)
    ctx.check(lib.aej_lpips_features(ctx.handle, weights.on(ctx).data_ptr(), x.data_ptr(), B, H, W, feats.data_ptr(), ws.data_ptr(),
                                     ctypes.c_uint64(nbytes)))
    return feats


def score(ctx, weights, xb, xa=None, feats_a=None):
    """float64 device tensor [B]: LPIPS(xa or the taps feats_a, xb) (aej_lpips_batch)."""
    t = ctx.torch
    B, H, W, _ = xb.shape
    check_size(H, W)
    lib = ctx.lib
    nbytes = int(lib.aej_lpips_workspace_bytes(B, H, W)) + (int(lib.aej_lpips_features_bytes(B, H, W)) if xa is not None else 0)
    ws = ctx.workspace(nbytes)
    out = ctx.empty((B,), t.float64)
    ctx.check(lib.aej_lpips_batch(ctx.handle, weights.on(ctx).data_ptr(), None if xa is None else xa.data_ptr(),
                                  None if feats_a is None else feats_a.data_ptr(), xb.data_ptr(), B, H, W, out.data_ptr(), ws.data_ptr(),
                                  ctypes.c_uint64(nbytes)))
    return out
