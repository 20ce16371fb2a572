"""Writes the fixtures of tests/test_gpu_jfif_progressive.py and tests/test_jfif_progressive_host.py: for each case the source pixels,
the .jpg Pillow writes for them with ``progressive=True`` and Pillow's decode of that file, plus the Pillow / libjpeg-turbo versions
that made them (meta.json).  Every layout occurs.

    python tests/golden/jfif_progressive/make_jfif_progressive_golden.py
"""
import io
import json
import os

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)


def cases():
    g = np.random.default_rng(20261017)
    lena = np.asarray(Image.open(os.path.join(GOLDEN, "lena.png")).convert("RGB"))
    prim = np.zeros((17, 33, 3), np.uint8)
    prim[:, :11, 0] = prim[:, 11:22, 1] = prim[:, 22:, 2] = 255
    prim[8:, :] = 255 - prim[8:, :]
    noise = g.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    crop = np.ascontiguousarray(lena[200:261, 230:320])
    return [("noise_37x53_q75_444", noise, 75, "4:4:4"),
            ("noise_37x53_q100_420", noise, 100, "4:2:0"),
            ("lena_61x90_q50_422", crop, 50, "4:2:2"),
            ("lena_61x90_q95_444", crop, 95, "4:4:4"),
            ("lena_61x90_q10_420", crop, 10, "4:2:0"),
            ("primaries_17x33_q90_420", prim, 90, "4:2:0"),
            ("flat_16x24_q1_444", np.full((16, 24, 3), (30, 140, 220), np.uint8), 1, "4:4:4"),
            ("noise_9x3_q100_422", g.integers(0, 256, (9, 3, 3), dtype=np.uint8), 100, "4:2:2")]


def main():
    meta = {"pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"), "cases": []}
    arrays = {}
    for name, x, q, ss in cases():
        buf = io.BytesIO()
        Image.fromarray(x).save(buf, "JPEG", quality=q, subsampling=ss, progressive=True)
        with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
            f.write(buf.getvalue())
        arrays[name + "_src"] = x
        arrays[name + "_dec"] = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        meta["cases"].append({"name": name, "quality": q, "subsampling": ss})
    np.savez_compressed(os.path.join(HERE, "pixels.npz"), **arrays)
    with open(os.path.join(HERE, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
