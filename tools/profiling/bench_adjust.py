"""adjust_many / histogram_many timing: 64 device-resident RGB images of 3840 x 2160 (bench_filter.py's, the natural fixtures
mirror-tiled) through Brightness(1.2), Color(1.2), Invert, Contrast(1.2), AutoContrast(), Equalize(), Sharpness(2), the ColorJitter chain
(Brightness, Contrast, Color, Sharpness), Equalize on 64 CONSTANT images (every lane of a wave counts into one bin: the worst case of the
LDS histogram) and histogram_many; and, in the same run as the yardstick, transpose_many("FLIP_LEFT_RIGHT"), which reads and writes every
byte once:

    python tools/profiling/bench_adjust.py [--batch 64] [--reps 7] [--pillow-images 16] [--out FILE]

    gpu       the call on the whole batch
    pillow    Pillow's own call on the first --pillow-images images on a pool of 16 threads (host only: no upload, no download),
              compared per image

Every time is a host clock around the whole call, which ends in a stream synchronise; one warm-up call, then --reps timed ones; the
best, the median and the spread (max - min over the median) are kept.  Every row is checked against Pillow on the first 2 images,
whole, before timing.  `expected` is the row's byte traffic over the flip's (a table-only or Color row 1, a row with one histogram pass
1.5: the source is read twice; histogram_many 0.5), `over` the row's best time over expected x the flip's best time: above 1.25 the
row owes an explanation (EXPERIMENTS.md).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image, ImageEnhance, ImageOps  # noqa: E402

from bench_filter import COPY_RATE, POOL, A, H, W, tiled  # noqa: E402

E = ImageEnhance


def _jitter(im):
    for cls, f in ((E.Brightness, 1.2), (E.Contrast, 0.8), (E.Color, 1.1), (E.Sharpness, 1.5)):
        im = cls(im).enhance(f)
    return im


JITTER = (A.Brightness(1.2), A.Contrast(0.8), A.Color(1.1), A.Sharpness(1.5))
# name, ours, Pillow's, expected bytes over the flip's, flat sources
ROWS = [
    ("FLIP_LEFT_RIGHT (yardstick)", lambda x: A.transpose_many(x, "FLIP_LEFT_RIGHT"), lambda im: im.transpose(Image.Transpose.FLIP_LEFT_RIGHT), 1.0, False),
    ("Brightness(1.2)", lambda x: A.adjust_many(x, A.Brightness(1.2)), lambda im: E.Brightness(im).enhance(1.2), 1.0, False),
    ("Color(1.2)", lambda x: A.adjust_many(x, A.Color(1.2)), lambda im: E.Color(im).enhance(1.2), 1.0, False),
    ("Invert", lambda x: A.adjust_many(x, A.Invert()), ImageOps.invert, 1.0, False),
    ("Contrast(1.2)", lambda x: A.adjust_many(x, A.Contrast(1.2)), lambda im: E.Contrast(im).enhance(1.2), 1.5, False),
    ("AutoContrast()", lambda x: A.adjust_many(x, A.AutoContrast()), ImageOps.autocontrast, 1.5, False),
    ("Equalize()", lambda x: A.adjust_many(x, A.Equalize()), ImageOps.equalize, 1.5, False),
    ("Sharpness(2)", lambda x: A.adjust_many(x, A.Sharpness(2)), lambda im: E.Sharpness(im).enhance(2), 2.0, False),      # SMOOTH: read, write; blend: two reads, write
    ("ColorJitter chain", lambda x: A.adjust_many(x, JITTER), _jitter, 3.5, False),      # histogram read; apply read + write; SMOOTH read + write; blend two reads + write
    ("Equalize() flat", lambda x: A.adjust_many(x, A.Equalize()), ImageOps.equalize, 1.5, True),
    ("histogram_many", lambda x: A.histogram_many(x), lambda im: np.array(im.histogram()), 0.5, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pillow-images", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    with ThreadPoolExecutor(POOL) as pool:
        host = list(pool.map(tiled, range(a.batch)))
    images = [torch.from_numpy(x).cuda() for x in host]
    flat_host = [np.full((H, W, 3), 40 + k, np.uint8) for k in range(2)]
    flat = [torch.full((H, W, 3), 40 + k % 2, dtype=torch.uint8, device="cuda") for k in range(a.batch)]
    np_ = max(2, min(a.pillow_images, a.batch))
    res = {"batch": a.batch, "H": H, "W": W, "copy_rate_tb_s": COPY_RATE / 1e12, "pool": POOL, "reps": a.reps, "pillow_images": np_, "rows": {}}
    flip_best = None
    for name, ours, theirs, expected, is_flat in ROWS:
        src_host = (flat_host * np_)[:np_] if is_flat else host[:np_]
        src = flat if is_flat else images
        t0 = time.perf_counter()
        with ThreadPoolExecutor(POOL) as pool:
            want = list(pool.map(lambda x: np.asarray(theirs(Image.fromarray(x))), src_host))
        row = {"pillow_pool_ms": (time.perf_counter() - t0) * 1e3}
        got = ours(src)                                          # the warm-up, and the check: whole images against Pillow's
        for i in range(2):
            assert np.array_equal(got[i].cpu().numpy(), want[i]), (name, i)
        del got, want
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ours(src)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            del out
        best, med = min(ts), statistics.median(ts)
        if flip_best is None:
            flip_best = best
        nbytes = expected * 2 * a.batch * H * W * 3
        row.update({"best_ms": best, "median_ms": med, "spread": (max(ts) - min(ts)) / med, "all_ms": ts, "expected": expected,
                    "over": best / (expected * flip_best), "tb_s": nbytes / best / 1e9, "gpu_ms_per_image": best / a.batch,
                    "pillow_ms_per_image": row["pillow_pool_ms"] / np_})
        row["speedup_per_image"] = row["pillow_ms_per_image"] / row["gpu_ms_per_image"]
        res["rows"][name] = row
        print(f"{name}: {best:.2f} ms (median {med:.2f}, spread {100 * row['spread']:.0f} %), {row['tb_s']:.3f} TB/s of expected bytes, {row['over']:.2f} x the "
              f"expectation ({expected} x the flip); Pillow on {POOL} threads {row['pillow_pool_ms']:.0f} ms for {np_} images: {row['speedup_per_image']:.0f} x per image",
              flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
