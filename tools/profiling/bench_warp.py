"""transform_many / rotate_many / transpose_many timing: 64 device-resident RGB images of 3840 x 2160 (bench_filter.py's, the natural
fixtures mirror-tiled) through rotate_many(30) under the three filters, rotate_many(30, expand=True) under bicubic, a RandomAffine-like
matrix under bilinear, a perspective under bicubic, and transpose_many with FLIP_LEFT_RIGHT and ROTATE_90; and, in the same run as
yardsticks from the existing code, resize_many to the same size under bicubic (over a box half a pixel inside the image, so that it
resamples) and filter_many with SHARPEN:

    python tools/profiling/bench_warp.py [--batch 64] [--reps 7] [--pillow-images 16] [--out FILE]

    gpu       the call on the whole batch
    pillow    Pillow's own call on the first --pillow-images images on a pool of 16 threads (host only: no upload, no download),
              compared per image

Every time is a host clock around the whole call, which ends in a stream synchronise; one warm-up call, then --reps timed ones; the
best, the median and the spread (max - min over the median) are kept.  Every row is checked against Pillow on the first 2 images,
whole, before timing.  A flip moves 2 x 3 bytes a pixel and does no arithmetic: the run fails if it takes longer than SHARPEN.
Prints one JSON line (and writes it to --out)."""
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
from PIL import Image, ImageFilter  # noqa: E402

from bench_filter import COPY_RATE, POOL, A, H, W, tiled  # noqa: E402

R = Image.Resampling
AFFINE = (0.93, 0.21, -310.0, -0.17, 1.05, 240.0)           # RandomAffine-like: 12 degrees, a scale, a shear and a translation
PERSPECTIVE = (1.08, 0.06, -120.0, 0.03, 1.1, -90.0, 2.0e-5, 1.5e-5)
BOX = (0.5, 0.5, W - 0.5, H - 0.5)
ROWS = [
    ("rotate(30) nearest", lambda x: A.rotate_many(x, 30, "nearest"), lambda im: im.rotate(30, R.NEAREST)),
    ("rotate(30) bilinear", lambda x: A.rotate_many(x, 30, "bilinear"), lambda im: im.rotate(30, R.BILINEAR)),
    ("rotate(30) bicubic", lambda x: A.rotate_many(x, 30, "bicubic"), lambda im: im.rotate(30, R.BICUBIC)),
    ("rotate(30, expand) bicubic", lambda x: A.rotate_many(x, 30, "bicubic", expand=True), lambda im: im.rotate(30, R.BICUBIC, expand=True)),
    ("affine bilinear", lambda x: A.transform_many(x, (W, H), "affine", AFFINE, "bilinear"), lambda im: im.transform((W, H), Image.Transform.AFFINE, AFFINE, R.BILINEAR)),
    ("perspective bicubic", lambda x: A.transform_many(x, (W, H), "perspective", PERSPECTIVE, "bicubic"),
     lambda im: im.transform((W, H), Image.Transform.PERSPECTIVE, PERSPECTIVE, R.BICUBIC)),
    ("FLIP_LEFT_RIGHT", lambda x: A.transpose_many(x, "FLIP_LEFT_RIGHT"), lambda im: im.transpose(Image.Transpose.FLIP_LEFT_RIGHT)),
    ("ROTATE_90", lambda x: A.transpose_many(x, "ROTATE_90"), lambda im: im.transpose(Image.Transpose.ROTATE_90)),
    ("resize bicubic (yardstick)", lambda x: A.resize_many(x, (W, H), "bicubic", box=BOX), lambda im: im.resize((W, H), R.BICUBIC, box=BOX)),
    ("SHARPEN (yardstick)", lambda x: A.filter_many(x, ImageFilter.SHARPEN), lambda im: im.filter(ImageFilter.SHARPEN)),
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
    res = {"batch": a.batch, "H": H, "W": W, "copy_rate_tb_s": COPY_RATE / 1e12, "pool": POOL, "reps": a.reps, "pillow_images": np_, "rows": {}}
    for name, ours, theirs in ROWS:
        t0 = time.perf_counter()
        with ThreadPoolExecutor(POOL) as pool:
            want = list(pool.map(lambda x: np.asarray(theirs(Image.fromarray(x))), host[:np_]))
        row = {"pillow_pool_ms": (time.perf_counter() - t0) * 1e3}
        got = ours(images)                                       # the warm-up, and the check: whole images against Pillow's
        for i in range(2):
            assert np.array_equal(got[i].cpu().numpy(), want[i]), (name, i)
        out_bytes = sum(g.numel() for g in got)
        del got, want
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ours(images)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            del out
        best, med = min(ts), statistics.median(ts)
        nbytes = a.batch * H * W * 3 + out_bytes                 # one read of the sources, one write of the outputs
        row.update({"best_ms": best, "median_ms": med, "spread": (max(ts) - min(ts)) / med, "all_ms": ts, "out_mb": out_bytes / 1e6,
                    "tb_s": nbytes / best / 1e9, "share_of_copy": nbytes / (best * 1e-3) / COPY_RATE, "gpu_ms_per_image": best / a.batch,
                    "pillow_ms_per_image": row["pillow_pool_ms"] / np_})
        row["speedup_per_image"] = row["pillow_ms_per_image"] / row["gpu_ms_per_image"]
        res["rows"][name] = row
        print(f"{name}: {best:.2f} ms (median {med:.2f}, spread {100 * row['spread']:.0f} %), {row['tb_s']:.3f} TB/s = {100 * row['share_of_copy']:.1f} % of copy; "
              f"Pillow on {POOL} threads {row['pillow_pool_ms']:.0f} ms for {np_} images: {row['speedup_per_image']:.0f} x per image", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    flip, sharpen = res["rows"]["FLIP_LEFT_RIGHT"]["median_ms"], res["rows"]["SHARPEN (yardstick)"]["median_ms"]
    assert flip <= sharpen, f"FLIP_LEFT_RIGHT takes {flip:.2f} ms, SHARPEN {sharpen:.2f} ms: the flip's access pattern is wrong"


if __name__ == "__main__":
    main()
