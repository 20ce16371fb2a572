"""Writes the fixtures of tests/test_jfif_grey_host.py and tests/test_gpu_jfif_grey.py: for each case the grey source pixels and the three
.jpg files Pillow writes for that mode-"L" image -- plain, ``optimize=True`` and ``progressive=True`` -- plus the Pillow / libjpeg-turbo
versions that made them (meta.json).  The images are noise over a ramp; each size is the smallest at which one thing can break: a
single block, an exact block, partial edges on either axis, one-block-wide strips, more than one wave's worth of blocks.

    python tests/golden/jfif_grey/make_jfif_grey_golden.py
"""
import io
import json
import os

import numpy as np
from PIL import Image, ImageFile, features

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (1, 40), (40, 1), (37, 53), (255, 257)]      # (H, W)
QUALITIES = [75, 1, 100, 10, 95, 50, 75, 100, 50]
KINDS = {"": dict(), "_opt": dict(optimize=True), "_prog": dict(progressive=True)}


def image(h, w, seed):
    rng = np.random.default_rng(seed)
    ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5) % 256
    return ((rng.integers(0, 256, (h, w)) + ramp) // 2).astype(np.uint8)


def cases():
    return [(f"ramp_{h}x{w}_q{q}", image(h, w, 11 * k + 1), q) for k, ((h, w), q) in enumerate(zip(SIZES, QUALITIES))]


def save(x, q, **kw):
    """Pillow's file (a larger ImageFile.MAXBLOCK lets the one-piece scans of noise through and does not change the bytes)"""
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * x.size + 4096)
    try:
        Image.fromarray(x).save(buf, "JPEG", quality=q, **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


def main():
    meta = {"pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"), "cases": []}
    arrays = {}
    for name, x, q in cases():
        assert Image.fromarray(x).mode == "L"
        for suffix, kw in KINDS.items():
            with open(os.path.join(HERE, name + suffix + ".jpg"), "wb") as f:
                f.write(save(x, q, **kw))
        arrays[name + "_src"] = x
        meta["cases"].append({"name": name, "height": int(x.shape[0]), "width": int(x.shape[1]), "quality": q})
    np.savez_compressed(os.path.join(HERE, "pixels.npz"), **arrays)
    with open(os.path.join(HERE, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
