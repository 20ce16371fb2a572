"""Fixtures for the scaled decode (tests/test_gpu_jpegdec_scaled.py): Pillow's pixels of every file of tests/golden/jpegdec/ (baseline)
and tests/golden/jpegprog/ (progressive) at scale 2, 4 and 8.

    python tests/golden/jpegdec_scaled/make_jpegdec_scaled_golden.py

writes pixels.npz, keys "<folder>/<case>/<scale>", and meta.json (the Pillow / libjpeg-turbo versions, and which entries Pillow could
not give).  The pixels are ``im.draft("RGB", (W // s, H // s)); np.asarray(im.convert("RGB"))``, with ``im.decoderconfig == (s, 0)``
asserted.  draft() cannot force scale s on a file with min(W, H) < s (its requested size would be 0): for those entries -- listed in
meta.json under "from_model" -- the pixels are those of the NumPy model tests/scaled_decode_reference.py, which equals Pillow on every
other entry (asserted here).  The input files are read only."""
import io
import json
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(GOLDEN))
import scaled_decode_reference as R  # noqa: E402

SCALES = (2, 4, 8)


def main():
    pixels, from_model = {}, []
    for folder in ("jpegdec", "jpegprog"):
        with open(os.path.join(GOLDEN, folder, "meta.json")) as f:
            names = [c["name"] for c in json.load(f)["cases"]]
        for name in names:
            with open(os.path.join(GOLDEN, folder, name + ".jpg"), "rb") as f:
                data = f.read()
            for s in SCALES:
                key = f"{folder}/{name}/{s}"
                model = R.decode(data, s)
                im = Image.open(io.BytesIO(data))
                W, H = im.size
                if min(W, H) < s:
                    pixels[key] = model
                    from_model.append(key)
                    continue
                im.draft("RGB", (W // s, H // s))
                assert im.decoderconfig == (s, 0), (key, im.decoderconfig)
                pixels[key] = np.asarray(im.convert("RGB"))
                assert pixels[key].shape == (-(-H // s), -(-W // s), 3) and np.array_equal(pixels[key], model), key
    np.savez_compressed(os.path.join(HERE, "pixels.npz"), **pixels)
    with open(os.path.join(HERE, "meta.json"), "w") as f:
        json.dump(dict(pillow=features.version("pil"),
                       libjpeg_turbo=features.version("libjpeg_turbo"), scales=list(SCALES), entries=sorted(pixels), from_model=from_model), f, indent=1)
    print(len(pixels), "entries,", len(from_model), "from the model")


if __name__ == "__main__":
    main()
