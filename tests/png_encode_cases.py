"""The images tests/test_png_encode_host.py and tests/test_gpu_png_encode.py encode: generated from seeded generators, small, and chosen
for the decisions of Pillow's filter rule (tests/png_encode_reference.py) and for the edges of the kernels."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CHANNELS = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4}


def _shape(a, c):
    return a[..., 0] if c == 1 else a


def smooth(h, w, c, noise=0, seed=0):
    """A diagonal ramp per channel, with uniform noise of +-`noise` levels."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = (2 * x + 3 * y)[..., None] + 40 * np.arange(c)
    if noise:
        base = base + rng.integers(-noise, noise + 1, base.shape)
    return _shape(np.clip(base, 0, 255).astype(np.uint8), c)


def noise(h, w, c, seed=0):
    return _shape(np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8), c)


def mode_cases():
    """name -> image: every mode with a smooth, a noisy and a random image, identical rows and an all-zero row."""
    out = {}
    for m, c in CHANNELS.items():
        out[f"{m}-smooth"] = smooth(33, 47, c)
        out[f"{m}-noisy"] = smooth(31, 45, c, noise=3, seed=c)
        out[f"{m}-noise"] = noise(9, 11, c, seed=10 + c)
        same = smooth(6, 21, c, noise=2, seed=20 + c)
        same[1:] = same[:1]                      # every row equals the row above: Up costs 0
        out[f"{m}-same-rows"] = same
        zero = smooth(7, 19, c, noise=2, seed=30 + c)
        zero[0] = 0                              # all-zero first row and all-zero row under a non-zero one: None at cost 0, nothing else tried
        zero[4] = 0
        out[f"{m}-zero-rows"] = zero
        out[f"{m}-1x1"] = noise(1, 1, c, seed=40 + c)
        out[f"{m}-width1"] = noise(5, 1, c, seed=50 + c)      # rows of bpp bytes: no byte has a left neighbour
        out[f"{m}-width2"] = smooth(4, 2, c, noise=5, seed=60 + c)
        out[f"{m}-height1"] = smooth(1, 40, c, noise=4, seed=70 + c)
        out[f"{m}-height2"] = smooth(2, 40, c, noise=4, seed=80 + c)
    return out


# Two-row grey images (row above, row) whose second row decides the rule; the costs are (None, Sub, Up, Average, Paeth).
TIES = {
    "none-up": ([36, 30, 60, 40, 24, 70], [78, 96, 9, 102, 15, 0], (300, 378, 300, 339, 397), 0),       # None = Up < the rest: None stays
    "up-sub": ([25, 32, 8, 36, 0, 36], [26, 18, 38, 7, 32, 22], (143, 120, 120, 121, 122), 2),           # Up = Sub < the rest: Up stays
    "sub-paeth": ([0, 6, 7, 3, 2, 22], [38, 22, 23, 20, 25, 31], (159, 69, 119, 76, 69), 1),             # Sub = Paeth < the rest: Sub stays
}
# Average alone is cheapest: chosen with optimize=True; without it the best of the others, Paeth
AVERAGE = ([57, 96, 15, 93, 12, 54], [24, 26, 22, 56, 20, 78], (226, 158, 179, 96, 140), 3, 4)


def tie_image(name):
    up, row = (TIES[name] if name in TIES else AVERAGE)[:2]
    return np.array([up, row], np.uint8)


def fold_image():
    """Bytes 127, 128, 129 under a zero row: the cost function folds at 128 (127 -> 127, 128 -> 128, 129 -> 127)."""
    return np.array([[0, 0, 0, 0, 0, 0], [127, 128, 129, 128, 127, 129], [129, 129, 129, 128, 128, 128]], np.uint8)


def crafted_cases():
    out = {f"tie-{k}": tie_image(k) for k in TIES}
    out["average"] = tie_image("average")
    out["fold"] = fold_image()
    return out


def split_image():
    """Noise whose zlib stream exceeds 65536 bytes: more than one IDAT chunk."""
    return noise(160, 150, 3, seed=99)


def size_set():
    """name -> image of about 256 x 256 in which a deflate with a matcher must beat Huffman coding alone."""
    from PIL import Image
    rng = np.random.default_rng(5)
    tile = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    lena = np.asarray(Image.open(os.path.join(HERE, "golden", "jfif", "lena_61x90_q50.jpg")).convert("RGB"))[:60, 10:74]
    return {
        "gradient": smooth(256, 256, 3, noise=1, seed=3),
        "tiles": np.tile(tile, (16, 16, 1)),
        "lena-tiled": np.ascontiguousarray(np.tile(lena, (5, 4, 1))[:256, :256]),
    }


def size_noise():
    return noise(256, 256, 3, seed=77)
