"""Writes the fixtures of this folder: the files of CASES, NARROW and RESTART (tests/jpeg_adobe_reference.py makes them), Pillow's pixels
of every one in both modes (pixels.npz: "<name>/auto" is np.asarray(Image.open(f)), "<name>/RGB" its convert("RGB")) and meta.json with
the versions that produced them.  Run from the repository root:  python tests/golden/jpeg_adobe/generate.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import jpeg_adobe_reference as R  # noqa: E402

W, H = 83, 61
# name: (kind, layout, progressive)
CASES = {
    "cmyk_1x1": ("cmyk", "1x1", False), "cmyk_2x1": ("cmyk", "2x1", False), "cmyk_2x2": ("cmyk", "2x2", False),
    "cmyk_2x2_prog": ("cmyk", "2x2", True), "cmyk_1x1_prog": ("cmyk", "1x1", True),
    "ycck_1x1": ("ycck", "1x1", False), "ycck_2x1_prog": ("ycck", "2x1", True), "ycck_2x2": ("ycck", "2x2", False),
    "plain_2x2": ("plain", "2x2", False),
    "cmyk_2x2k": ("cmyk", "2x2k", False), "ycck_2x1k": ("ycck", "2x1k", False), "plain_2x1k": ("plain", "2x1k", False),
    "cmyk_2x2k_prog": ("cmyk", "2x2k", True), "ycck_2x1k_prog": ("ycck", "2x1k", True), "plain_2x2k_prog": ("plain", "2x2k", True),
    "rgb_1x1": ("rgb", "1x1", False), "rgb_2x1": ("rgb", "2x1", False), "rgb_2x2": ("rgb", "2x2", False), "rgb_1x1_prog": ("rgb", "1x1", True),
    "rgb_2x2_prog": ("rgb", "2x2", True),
}
# planes at most 2 samples wide are replicated, 3 wide filtered: widths 1..5 at height 20, and two more odd sizes
NARROW = {f"{kind}_{layout}_{w}x{h}": (kind, layout, w, h)
          for kind in ("cmyk", "ycck") for layout in ("2x1", "2x2") for w, h in [(w, 20) for w in range(1, 6)] + [(1, 1), (17, 33)]}
# restart intervals through Pillow's save, and a quality-100 noise file whose one segment spans many subsequences
RESTART = {
    "cmyk_2x2_rows": dict(kind="cmyk", layout="2x2", W=W, H=H, restart_marker_rows=1),
    "ycck_2x1_blocks": dict(kind="ycck", layout="2x1", W=W, H=H, restart_marker_blocks=2),
    "cmyk_2x2k_rst3": dict(kind="cmyk", layout="2x2k", W=W, H=H, restart_interval=3),
}
NOISE = "cmyk_2x2_noise_96x80_q100"


def noise_file():
    return R._save(R.noise_picture(80, 96, 4), "CMYK", quality=100, subsampling=2)


def main():
    from PIL import __version__ as pillow, features
    files = {n: R.make_file(k, l, W, H, p) for n, (k, l, p) in CASES.items()}
    files.update({n: R.make_file(k, l, w, h, seed=w + h) for n, (k, l, w, h) in NARROW.items()})
    files.update({n: R.make_file(**kw) for n, kw in RESTART.items()})
    files[NOISE] = noise_file()
    px = {}
    for n, f in files.items():
        with open(os.path.join(HERE, n + ".jpg"), "wb") as fh:
            fh.write(f)
        px[n + "/auto"], px[n + "/RGB"] = R.pillow_pixels(f)
    np.savez_compressed(os.path.join(HERE, "pixels.npz"), **px)
    meta = {"pillow": pillow, "libjpeg_turbo": features.version("libjpeg_turbo"), "size": [W, H],
            "cases": [{"name": n, "kind": k, "layout": l, "progressive": p} for n, (k, l, p) in CASES.items()],
            "narrow": [{"name": n, "kind": k, "layout": l, "size": [w, h]} for n, (k, l, w, h) in NARROW.items()],
            "restart": sorted(RESTART), "noise": NOISE}
    with open(os.path.join(HERE, "meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
