"""Writes the standard-JPEG fixtures of tests/test_gpu_jfif.py: for each case the source pixels, the .jpg Pillow writes for them and
Pillow's decode of that file, plus the Pillow / libjpeg-turbo versions that made them (meta.json).

    python tests/golden/jfif/make_jfif_golden.py
"""
import io
import json
import os

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)


def cases():
    g = np.random.default_rng(20261015)
    lena = np.asarray(Image.open(os.path.join(GOLDEN, "lena.png")).convert("RGB"))
    prim = np.zeros((17, 33, 3), np.uint8)
    prim[:, :11, 0] = prim[:, 11:22, 1] = prim[:, 22:, 2] = 255
    prim[8:, :] = 255 - prim[8:, :]
    return [("noise_37x53_q90", g.integers(0, 256, (37, 53, 3), dtype=np.uint8), 90),
            ("noise_9x4_q100", g.integers(0, 256, (9, 4, 3), dtype=np.uint8), 100),
            ("lena_61x90_q50", np.ascontiguousarray(lena[200:261, 230:320]), 50),
            ("flat_16x24_q10", np.full((16, 24, 3), (30, 140, 220), np.uint8), 10),
            ("primaries_17x33_q75", prim, 75),
            ("lena_8x8_q1", np.ascontiguousarray(lena[256:264, 256:264]), 1)]


def main():
    meta = {"pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"), "cases": []}
    arrays = {}
    for name, x, q in cases():
        buf = io.BytesIO()
        Image.fromarray(x).save(buf, "JPEG", quality=q)
        with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
            f.write(buf.getvalue())
        arrays[name + "_src"] = x
        arrays[name + "_dec"] = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        meta["cases"].append({"name": name, "quality": q})
    np.savez_compressed(os.path.join(HERE, "pixels.npz"), **arrays)
    with open(os.path.join(HERE, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
