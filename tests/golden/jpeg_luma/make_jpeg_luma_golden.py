"""Fixtures for the mode-"L" output of standard_jpeg_decode_many / standard_jpeg_thumbnail_many (tests/test_jpeg_luma_host.py,
tests/test_gpu_jpeg_luma.py): Pillow's own pixels of the JPEG files already under tests/golden/jpegdec and tests/golden/jpegprog.

    python tests/golden/jpeg_luma/make_jpeg_luma_golden.py

writes pixels.npz and meta.json (the cases, the Pillow / libjpeg-turbo versions that made them).  No JPEG file is written: the inputs
are read only.  Keys of pixels.npz, per file "<folder>/<case>":
    <file>/L<s>                          ``im.draft("L", (W // s, H // s)); np.asarray(im)`` for s = 1, 2, 4, 8: a grey file's samples, a
                                         colour file's luma plane (tests/jpeg_luma_reference.py draft_l)
    <file>/auto                          ``np.asarray(Image.open(f))``, a colour file as RGB
    <file>/t<mode>_<w>x<h>_<filter>_<gap>  the thumbnail under mode "L" / "auto" (jpeg_luma_reference.thumbnail), sizes (16, 16) and
                                         (40, 24), bicubic and lanczos, reducing_gap None and 2.0
Asserted here, and again by the tests: for at least one colour file of each sampling (4:4:4, 4:2:2, 4:2:0) the draft("L") image differs
from ``convert("RGB").convert("L")`` -- otherwise a test could not tell the two meanings of "L" apart."""
import json
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(GOLDEN))
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))
import jpeg_luma_reference as LR  # noqa: E402

FOLDERS = ("jpegdec", "jpegprog")
SCALES = (1, 2, 4, 8)
SIZES = ((16, 16), (40, 24))
RESAMPLE = ("bicubic", "lanczos")
GAPS = (None, 2.0)


def thumb_key(name, mode, size, resample, gap):
    return f"{name}/t{mode}_{size[0]}x{size[1]}_{resample}_{gap}"


def files():
    for folder in FOLDERS:
        for fn in sorted(os.listdir(os.path.join(GOLDEN, folder))):
            if fn.endswith(".jpg"):
                with open(os.path.join(GOLDEN, folder, fn), "rb") as f:
                    yield f"{folder}/{fn[:-4]}", f.read()


def main():
    from adaptive_edge_aware_jpeg_amd.standard_jpeg import thumbnail_plan
    pixels, cases, differ = {}, [], {}
    for name, data in files():
        samp = LR.sampling(data)
        for s in SCALES:
            pixels[f"{name}/L{s}"] = LR.draft_l(data, s)
        pixels[f"{name}/auto"] = LR.auto(data)
        for mode in ("L", "auto"):
            for size in SIZES:
                for r in RESAMPLE:
                    for g in GAPS:
                        pixels[thumb_key(name, mode, size, r, g)] = LR.thumbnail(data, size, r, g, mode, thumbnail_plan)
        d = 0
        if samp != "grey":
            d = int(np.abs(pixels[f"{name}/L1"].astype(int) - LR.convert_l(data).astype(int)).max())
            differ[samp] = max(differ.get(samp, 0), d)
        H, W = pixels[f"{name}/L1"].shape
        cases.append({"name": name, "size": [W, H], "sampling": samp, "luma_vs_convert_l": d})
    for samp in ("4:4:4", "4:2:2", "4:2:0"):
        assert differ.get(samp, 0) >= 1, f"no {samp} fixture tells draft('L') from convert('L')"
    np.savez_compressed(os.path.join(HERE, "pixels.npz"), **pixels)
    meta = {"pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"), "scales": list(SCALES),
            "sizes": [list(s) for s in SIZES], "resample": list(RESAMPLE), "gaps": list(GAPS), "cases": cases}
    with open(os.path.join(HERE, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
