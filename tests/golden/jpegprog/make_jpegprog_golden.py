"""Fixtures for standard_jpeg_decode_many(..., progressive=True) (tests/test_jpegprog_host.py, tests/test_gpu_jpegprog.py): small
progressive files written by Pillow over every supported layout and option, and Pillow's own decode of each.

    python tests/golden/jpegprog/make_jpegprog_golden.py

writes <case>.jpg, pixels.npz (Pillow's ``convert("RGB")`` of every file) and meta.json (the cases, each file's scan list as
[components, Ss, Se, Ah, Al, restart interval], and the Pillow / libjpeg-turbo versions that wrote them).  Sources are the repository's
own test images (tests/golden/lena.png, tests/golden/natural/*.png), a flat image and seeded noise."""
import io
import json
import os

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)


def _src(name, y, x, H, W, mode="RGB"):
    if name == "flat":
        a = np.full((H, W, 3), (90, 140, 200), np.uint8)
    elif name == "noise":
        a = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
    else:
        a = np.asarray(Image.open(os.path.join(GOLDEN, name + ".png")).convert("RGB"))[y:y + H, x:x + W]
    out = Image.fromarray(np.ascontiguousarray(a))
    return out.convert("L") if mode == "L" else out


def _exif():
    e = Image.Exif()
    e[0x0112] = 6                       # orientation: rotate 90 (Image.open ignores it)
    e[0x010F] = "fixture"
    return e.tobytes()


def scan_list(data):
    """[[component ids], Ss, Se, Ah, Al, restart interval] of every SOS, by a plain marker walk"""
    out, p, ri = [], 2, 0
    while data[p + 1] != 0xD9:
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        body = data[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xDD:
            ri = int.from_bytes(body, "big")
        if m == 0xDA:
            ns = body[0]
            out.append([[body[1 + 2 * i] for i in range(ns)], body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns] >> 4, body[3 + 2 * ns] & 15, ri])
            while not (data[p] == 0xFF and data[p + 1] != 0 and not 0xD0 <= data[p + 1] <= 0xD7 and data[p + 1] != 0xFF):
                p += 1
    return out


# name -> (source, y, x, H, W, mode, save options); every file is saved with progressive=True
QT16 = [[min(65535, 2 + 9 * i) for i in range(64)], [min(65535, 300 + i) for i in range(64)]]
CASES = {
    "lena_64x64_420_q75": ("lena", 200, 220, 64, 64, "RGB", dict(quality=75, subsampling=2)),
    "baboon_48x40_422_q50": ("natural/baboon", 10, 30, 48, 40, "RGB", dict(quality=50, subsampling=1)),
    "peppers_40x56_444_q90": ("natural/peppers", 100, 100, 40, 56, "RGB", dict(quality=90, subsampling=0)),
    "house_45x61_grey_q60": ("natural/house", 50, 70, 45, 61, "L", dict(quality=60)),
    "buildings_50x66_rst3_q70": ("natural/buildings", 120, 40, 50, 66, "RGB", dict(quality=70, restart_marker_blocks=3)),
    "jelly_40x70_rstrow_422_q80": ("natural/jelly_beans", 60, 60, 40, 70, "RGB", dict(quality=80, subsampling=1, restart_marker_rows=1)),
    "bikes_53x37_rstrow_444_q75": ("natural/bikes", 100, 200, 53, 37, "RGB", dict(quality=75, subsampling=0, restart_marker_rows=1)),
    "grey_33x47_rst3_q40": ("lena", 300, 100, 33, 47, "L", dict(quality=40, restart_marker_blocks=3)),
    "grey_40x24_rstrow_q85": ("natural/house", 90, 30, 40, 24, "L", dict(quality=85, restart_marker_rows=1)),
    "lena_32x48_qt16": ("lena", 250, 250, 32, 48, "RGB", dict(qtables=QT16, subsampling=2)),
    "peppers_24x40_exif_com_q75": ("natural/peppers", 20, 20, 24, 40, "RGB", dict(quality=75, exif=_exif(), comment=b"a COM segment")),
    "lena_1x1_420_q75": ("lena", 256, 256, 1, 1, "RGB", dict(quality=75)),
    "baboon_4x9_444_q100": ("natural/baboon", 0, 0, 4, 9, "RGB", dict(quality=100, subsampling=0)),
    "baboon_4x9_420_q90": ("natural/baboon", 0, 0, 4, 9, "RGB", dict(quality=90, subsampling=2)),
    "house_33x17_420_q10": ("natural/house", 5, 5, 33, 17, "RGB", dict(quality=10)),
    "house_33x17_422_q50": ("natural/house", 5, 5, 33, 17, "RGB", dict(quality=50, subsampling=1)),
    "bikes_53x37_422_q1": ("natural/bikes", 300, 400, 53, 37, "RGB", dict(quality=1, subsampling=1)),
    "bikes_53x37_420_rst3_q50": ("natural/bikes", 300, 400, 53, 37, "RGB", dict(quality=50, subsampling=2, restart_marker_blocks=3)),
    "buildings_128x96_q90": ("natural/buildings", 200, 300, 128, 96, "RGB", dict(quality=90)),
    "flat_96x128_420_q75": ("flat", 0, 0, 96, 128, "RGB", dict(quality=75)),
    "noise_64x64_444_q100": ("noise", 0, 0, 64, 64, "RGB", dict(quality=100, subsampling=0)),
    "noise_37x53_420_q100": ("noise", 0, 0, 37, 53, "RGB", dict(quality=100, subsampling=2)),
}


def main():
    pixels, cases = {}, []
    for name, (src, y, x, H, W, mode, opts) in CASES.items():
        buf = io.BytesIO()
        _src(src, y, x, H, W, mode).save(buf, "JPEG", progressive=True, **opts)
        data = buf.getvalue()
        with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
            f.write(data)
        im = Image.open(io.BytesIO(data))
        pixels[name] = np.asarray(im.convert("RGB"))
        cases.append({"name": name, "size": list(im.size), "mode": im.mode,
                      "layer": [[c[0], c[1], c[2], c[3]] for c in im.layer],
                      "quantization": {str(k): list(v) for k, v in im.quantization.items()},
                      "scans": scan_list(data)})
    np.savez_compressed(os.path.join(HERE, "pixels.npz"), **pixels)
    meta = {"pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"), "cases": cases}
    with open(os.path.join(HERE, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
