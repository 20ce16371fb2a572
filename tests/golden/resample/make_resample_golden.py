"""Fixtures for resize_many and standard_jpeg_thumbnail_many (tests/test_gpu_resample.py, tests/test_resample_host.py): Pillow's pixels.

    python tests/golden/resample/make_resample_golden.py

writes pixels.npz and meta.json (the Pillow / libjpeg-turbo versions and every case with what it exercises).
  * "thumb/<k>": ``im = Image.open(file); im.thumbnail(size, F, reducing_gap=g); np.asarray(im.convert("RGB"))`` for files of
    tests/golden/jpegdec (baseline) and tests/golden/jpegprog (progressive), read only.  meta records the draft scale Pillow chose
    (im.decoderconfig), the reduce factors and the final size, which tests/resample_reference.py's plan must reproduce (asserted).
  * "resize/<k>": ``Image.fromarray(src).resize(size, F, box=box, reducing_gap=g)`` of "src/<j>", small arrays from a seeded generator.
Every entry equals the NumPy model (asserted), and the properties the tests rely on are asserted at the end, so a fixture set that
loses one fails here."""
import io
import json
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(GOLDEN))
import resample_reference as M  # noqa: E402

NAMES = ("box", "bilinear", "hamming", "bicubic", "lanczos")
SIZES = [(5, 5), (20, 12), (9, 30), (3, 3), (33, 17), (16, 64), (7, 2)]
GAPS = [2.0, 1.0, 1.0, None, 3.0, 1.0, 2.0]
COVERED = {("jpegdec", "lena_1x1_420_q75"), ("jpegdec", "baboon_9x4_444_q100"), ("jpegprog", "grey_33x47_rst3_q40")}
# thumbnails of the largest files by hand: scale 8 with and without a reduce after it, scale 4, the drafted size equal to the final one
EXTRA = [("jpegdec", "buildings_96x128_crop_q95", (8, 6), "bicubic", 2.0), ("jpegdec", "buildings_96x128_crop_q95", (3, 3), "lanczos", 2.0),
         ("jpegdec", "buildings_96x128_crop_q95", (16, 12), "hamming", 2.0), ("jpegprog", "flat_96x128_420_q75", (4, 4), "box", 1.0),
         ("jpegprog", "buildings_128x96_q90", (12, 16), "bilinear", 2.0), ("jpegdec", "lena_64x64_420_q75", (32, 32), "bicubic", 1.0),
         ("jpegdec", "lena_64x64_420_q75", (16, 16), "lanczos", 2.0), ("jpegprog", "lena_64x64_420_q75", (8, 8), "box", 1.0),
         ("jpegdec", "buildings_96x128_crop_q95", (3, 3), "hamming", 1.0), ("jpegprog", "buildings_128x96_q90", (30, 30), "bicubic", 1.0)]


def sources():
    rng = np.random.default_rng(20261017)
    shapes = [(37, 53), (19, 40), (1, 1), (5, 7), (9, 1), (48, 64), (1, 30)]
    out = []
    for h, w in shapes:
        y, x = np.mgrid[0:h, 0:w]
        smooth = np.stack([(x * 9 + y * 3) % 256, (y * 11 + x) % 256, (x * y + 40) % 256], -1)
        out.append(np.clip(smooth + rng.integers(-60, 61, (h, w, 3)), 0, 255).astype(np.uint8))
    out.append(np.full((37, 53, 3), 255, np.uint8))
    return out


# (source, size, filter, box, reducing_gap)
RESIZES = [(0, (20, 11), "bicubic", None, None), (0, (53, 20), "lanczos", None, None), (0, (10, 37), "box", None, None),
           (0, (80, 60), "hamming", None, None), (0, (13, 9), "bilinear", (2.5, 1.25, 47.75, 30.5), None),
           (0, (53, 37), "bicubic", (0, 0, 52.5, 37), None), (0, (30, 30), "lanczos", (10, 5, 40, 35), None),
           (0, (6, 5), "bicubic", None, 1.0), (0, (5, 4), "hamming", None, 2.0), (0, (4, 7), "box", (20.5, 3.5, 50, 36), 1.0),
           (0, (3, 2), "bilinear", (25, 10, 45.5, 30.25), 1.5), (0, (27, 19), "lanczos", None, 1.0), (0, (53, 37), "box", None, 2.0),
           (1, (7, 40), "bicubic", None, None), (1, (19, 5), "hamming", None, 3.0), (2, (5, 7), "bicubic", None, None),
           (2, (1, 1), "lanczos", None, None), (3, (1, 1), "lanczos", None, None), (3, (1, 1), "box", None, 2.0),
           (4, (3, 4), "bilinear", None, None), (4, (1, 20), "bicubic", None, None), (5, (64, 48), "bicubic", (0.5, 0.5, 63.5, 47.5), None),
           (5, (9, 9), "lanczos", None, 2.0), (5, (8, 6), "box", None, 1.0), (5, (100, 3), "hamming", (3, 3, 61, 44.5), 1.0),
           (6, (7, 1), "box", None, None), (6, (45, 2), "lanczos", None, None), (7, (9, 5), "bicubic", None, 1.0),
           (7, (20, 20), "lanczos", None, None)]


def main():
    pixels, cases = {}, []
    files = []
    for folder in ("jpegdec", "jpegprog"):
        with open(os.path.join(GOLDEN, folder, "meta.json")) as f:
            files += [(folder, c["name"]) for c in json.load(f)["cases"]]
    thumbs = []
    for i, (folder, name) in enumerate(files):
        for k in range(3):
            j = (i + 2 * k) % len(SIZES)
            thumbs.append((folder, name, SIZES[j], NAMES[(i + k) % 5], GAPS[(i + j) % len(GAPS)]))
        if (folder, name) in COVERED:
            thumbs.append((folder, name, (200, 100), NAMES[i % 5], (2.0, 1.0)[i % 2]))
            thumbs.append((folder, name, (64, 64), NAMES[(i + 1) % 5], (1.0, 2.0)[i % 2]))
    thumbs += EXTRA
    for k, (folder, name, size, filt, gap) in enumerate(thumbs):
        with open(os.path.join(GOLDEN, folder, name + ".jpg"), "rb") as f:
            data = f.read()
        im = Image.open(io.BytesIO(data))
        W, H = im.size
        grey = im.mode == "L"
        im.thumbnail(size, M.FILTERS[filt], reducing_gap=gap)
        scale = im.decoderconfig[0] if im.decoderconfig else 1
        px = np.asarray(im.convert("RGB"))
        plan = M.thumbnail_plan(W, H, size, gap)
        assert (plan is None) == (px.shape[:2] == (H, W) and not im.decoderconfig), (k, plan)
        if plan is not None:
            assert plan[0] == scale and plan[2] == (px.shape[1], px.shape[0]), (k, plan, scale, px.shape)
        assert np.array_equal(px, M.thumbnail(data, size, filt, gap)), ("thumb", k)
        drafted = (-(-W // scale), -(-H // scale))
        pixels[f"thumb/{k}"] = px
        cases.append(dict(kind="thumb", key=f"thumb/{k}", folder=folder, name=name, size=list(size), filter=filt, gap=gap, file_size=[W, H],
                          unchanged=plan is None, scale=scale, factors=list(plan[1]) if plan else [1, 1], final=[px.shape[1], px.shape[0]],
                          drafted_is_final=plan is not None and drafted == plan[2], grey=grey, restart="rst" in name))
    srcs = sources()
    for j, a in enumerate(srcs):
        pixels[f"src/{j}"] = a
    for k, (j, size, filt, box, gap) in enumerate(RESIZES):
        a = srcs[j]
        px = np.asarray(Image.fromarray(a).resize(size, M.FILTERS[filt], box=box, reducing_gap=gap))
        assert np.array_equal(px, M.resize(a, size, filt, box, gap)), ("resize", k)
        wh = (a.shape[1], a.shape[0])
        b = box or (0, 0) + wh
        fac = M.reduce_factors(b, size, gap)
        rb = M.safe_box(wh, size, filt, b) if max(fac) > 1 else None
        pixels[f"resize/{k}"] = px
        cases.append(dict(kind="resize", key=f"resize/{k}", source=j, size=list(size), filter=filt, box=list(box) if box else None, gap=gap,
                          factors=list(fac), safe_box_is_whole=rb is None or tuple(rb) == (0, 0) + wh))

    th = [c for c in cases if c["kind"] == "thumb"]
    rs = [c for c in cases if c["kind"] == "resize"]
    changed = [c for c in th if not c["unchanged"]]
    assert {c["filter"] for c in th} == set(NAMES) and {c["filter"] for c in rs} == set(NAMES)
    assert {c["scale"] for c in changed} == {1, 2, 4, 8}
    assert any(max(c["factors"]) > 1 for c in changed) and any(max(c["factors"]) == 1 and not c["drafted_is_final"] for c in changed)
    assert any(max(c["factors"]) > 1 and c["scale"] == 8 for c in changed)

    def partial(c):          # factors that differ per axis and leave partial cells at both edges
        fx, fy = c["factors"]
        w, h = -(-c["file_size"][0] // c["scale"]), -(-c["file_size"][1] // c["scale"])
        return fx != fy and fx > 1 and fy > 1 and w % fx and h % fy
    assert any(partial(c) for c in changed)
    assert any(c["drafted_is_final"] and c["scale"] > 1 for c in changed) and any(c["unchanged"] for c in th)
    assert any(c["grey"] and not c["unchanged"] for c in th) and any(c["restart"] and not c["unchanged"] for c in th)
    assert any(c["file_size"] == [1, 1] for c in th)
    assert {c["folder"] for c in th} == {"jpegdec", "jpegprog"}
    one = [c for c in th if c["gap"] == 1.0]          # the classes again within one reducing_gap: one call can hold them all
    assert {c["scale"] for c in one if not c["unchanged"]} == {1, 2, 4, 8} and {c["filter"] for c in one} == set(NAMES)
    assert any(c["unchanged"] for c in one) and any(c["drafted_is_final"] for c in one) and any(partial(c) for c in one)
    assert any(max(c["factors"]) == 1 and not c["drafted_is_final"] and not c["unchanged"] for c in one)
    assert any(c["grey"] and not c["unchanged"] for c in one) and any(c["restart"] and not c["unchanged"] for c in one)
    assert any(c["file_size"] == [1, 1] for c in one) and {c["folder"] for c in one} == {"jpegdec", "jpegprog"}
    assert any(c["box"] and max(c["factors"]) > 1 and not c["safe_box_is_whole"] for c in rs)
    assert any(c["factors"][0] != c["factors"][1] and min(c["factors"]) > 1 for c in rs)
    assert any(c["size"][0] > srcs[c["source"]].shape[1] for c in rs)          # up-scaling

    np.savez_compressed(os.path.join(HERE, "pixels.npz"), **pixels)
    with open(os.path.join(HERE, "meta.json"), "w") as f:
        json.dump(dict(pillow=features.version("pil"), libjpeg_turbo=features.version("libjpeg_turbo"), cases=cases), f, indent=1)
    print(len(th), "thumbnails,", len(rs), "resizes,", os.path.getsize(os.path.join(HERE, "pixels.npz")), "bytes")


if __name__ == "__main__":
    main()
