"""convert_many / hue_many timing: 64 device-resident RGB images of 3840 x 2160 (bench_filter.py's, the natural fixtures mirror-tiled)
through RGB -> L, RGB -> YCbCr, RGB -> HSV, HSV -> RGB (the same bytes taken as HSV), hue_many(0.1), CMYK -> RGB and RGBA -> RGB (the
images with a fourth band); and, in the same run as the yardstick, transpose_many("FLIP_LEFT_RIGHT"), which reads and writes every byte
once:

    python tools/profiling/bench_convert.py [--batch 64] [--reps 7] [--pillow-images 16] [--out FILE]

    gpu       the call on the whole batch
    pillow    Pillow's own call on the first --pillow-images images on a pool of 16 threads (host only: no upload, no download),
              compared per image

Every time is a host clock around the whole call, which ends in a stream synchronise; one warm-up call, then --reps timed ones; the
best, the median and the spread (max - min over the median) are kept.  Every row is checked against Pillow on the first 2 images,
whole, before timing.  `expected` is the row's byte traffic over the flip's (3 -> 3 channels 1, RGB -> L 4/6, 4 -> 3 channels 7/6),
`over` the row's best time over expected x the flip's best time.  Prints one JSON line (and writes it to --out)."""
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
from PIL import Image  # noqa: E402

from bench_filter import COPY_RATE, POOL, A, H, W, tiled  # noqa: E402


def _pil_hue(im, f=0.1):
    h, s, v = im.convert("HSV").split()
    h = Image.fromarray(((np.asarray(h).astype(np.int64) + int(f * 255)) & 255).astype(np.uint8))
    return Image.merge("HSV", (h, s, v)).convert("RGB")


# name, ours, Pillow's (of the array), expected bytes over the flip's, four-band sources
ROWS = [
    ("FLIP_LEFT_RIGHT (yardstick)", lambda x: A.transpose_many(x, "FLIP_LEFT_RIGHT"), lambda a: Image.fromarray(a).transpose(Image.Transpose.FLIP_LEFT_RIGHT), 1.0, False),
    ("RGB -> L", lambda x: A.convert_many(x, "L"), lambda a: Image.fromarray(a).convert("L"), 4 / 6, False),
    ("RGB -> YCbCr", lambda x: A.convert_many(x, "YCbCr"), lambda a: Image.fromarray(a).convert("YCbCr"), 1.0, False),
    ("RGB -> HSV", lambda x: A.convert_many(x, "HSV"), lambda a: Image.fromarray(a).convert("HSV"), 1.0, False),
    ("HSV -> RGB", lambda x: A.convert_many(x, "RGB", source_mode="HSV"), lambda a: Image.fromarray(a, "HSV").convert("RGB"), 1.0, False),
    ("hue_many(0.1)", lambda x: A.hue_many(x, 0.1), lambda a: _pil_hue(Image.fromarray(a)), 1.0, False),
    ("CMYK -> RGB", lambda x: A.convert_many(x, "RGB", source_mode="CMYK"), lambda a: Image.fromarray(a, "CMYK").convert("RGB"), 7 / 6, True),
    ("RGBA -> RGB", lambda x: A.convert_many(x, "RGB"), lambda a: Image.fromarray(a, "RGBA").convert("RGB"), 7 / 6, True),
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
    np_ = max(2, min(a.pillow_images, a.batch))
    four = [torch.cat([x, x[:, :, 1:2].flip(1)], dim=2) for x in images]      # the fourth band: the green band mirrored
    four_host = [x.cpu().numpy() for x in four[:np_]]
    res = {"batch": a.batch, "H": H, "W": W, "copy_rate_tb_s": COPY_RATE / 1e12, "pool": POOL, "reps": a.reps, "pillow_images": np_, "rows": {}}
    flip_best = None
    for name, ours, theirs, expected, is_four in ROWS:
        src_host = four_host if is_four else host[:np_]
        src = four if is_four else images
        t0 = time.perf_counter()
        with ThreadPoolExecutor(POOL) as pool:
            want = list(pool.map(lambda x: np.asarray(theirs(x)), src_host))
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
              f"expectation ({expected:.3f} x the flip); Pillow on {POOL} threads {row['pillow_pool_ms']:.0f} ms for {np_} images: {row['speedup_per_image']:.0f} x per image",
              flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
