"""filter_many timing for the window filters: 64 device-resident RGB images of 3840 x 2160 (bench_filter.py's, the natural fixtures
mirror-tiled) through SHARPEN, SMOOTH_MORE, MinFilter(3), MedianFilter(3), MedianFilter(5), RankFilter(15, 112), ModeFilter(3) and
ModeFilter(7), and through GaussianBlur(2) in the same run as the yardstick:

    python tools/profiling/bench_window_filter.py [--batch 64] [--reps 5] [--pillow-images 64] [--pillow-rows 2160] [--out FILE]

    gpu       filter_many(images, F)
    pillow    Image.fromarray(a).filter(F) over the top --pillow-rows rows of the first --pillow-images images on a pool of 16 threads
              (host only: no upload, no download).  Pillow's RankFilter(15, 112) takes minutes per 4K image, so its rows may be timed
              on fewer and shorter images: the two are compared per image, Pillow's time scaled by 2160 / --pillow-rows

Every time is a host clock around the whole call, which ends in a stream synchronise; one warm-up call, then --reps timed ones; the
best and the median are kept.  The rate is the algorithm's bytes -- one read and one write of the images -- over the best time, also
as a share of the 6.29 TB/s the project has measured for a device copy.  Every filter is checked against Pillow on the first 2 images
before timing.  Prints one JSON line (and writes it to --out)."""
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

FILTERS = [("SHARPEN", ImageFilter.SHARPEN), ("SMOOTH_MORE", ImageFilter.SMOOTH_MORE), ("MinFilter(3)", ImageFilter.MinFilter(3)),
           ("MedianFilter(3)", ImageFilter.MedianFilter(3)), ("MedianFilter(5)", ImageFilter.MedianFilter(5)),
           ("RankFilter(15,112)", ImageFilter.RankFilter(15, 112)), ("ModeFilter(3)", ImageFilter.ModeFilter(3)), ("ModeFilter(7)", ImageFilter.ModeFilter(7)),
           ("GaussianBlur(2)", ImageFilter.GaussianBlur(2))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pillow-images", type=int, default=64)
    ap.add_argument("--pillow-rows", type=int, default=H)
    ap.add_argument("--out")
    a = ap.parse_args()
    with ThreadPoolExecutor(POOL) as pool:
        host = list(pool.map(tiled, range(a.batch)))
    images = [torch.from_numpy(x).cuda() for x in host]
    nbytes = 2 * a.batch * H * W * 3
    np_, rows = max(2, min(a.pillow_images, a.batch)), max(32, min(a.pillow_rows, H))
    res = {"batch": a.batch, "H": H, "W": W, "algorithmic_mb": nbytes / 1e6, "copy_rate_tb_s": COPY_RATE / 1e12, "pool": POOL, "reps": a.reps,
           "pillow_images": np_, "pillow_rows": rows, "filters": {}}
    print(f"{a.batch} images, {nbytes / 2e6:.1f} MB", flush=True)
    for name, f in FILTERS:
        print(f"{name}: Pillow ...", flush=True)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(POOL) as pool:
            want = list(pool.map(lambda x: np.asarray(Image.fromarray(x[:rows]).filter(f)), host[:np_]))
        row = {"pillow_pool_ms": (time.perf_counter() - t0) * 1e3}
        got = A.filter_many(images, f)                           # the warm-up
        small = A.filter_many([x[:rows] for x in host[:2]], f)   # the check: what Pillow filtered
        for i, w in enumerate(want[:2]):
            assert np.array_equal(small[i].cpu().numpy(), w), (name, i)
        del got, small, want
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = A.filter_many(images, f)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            del out
        best = min(ts)
        row.update({"best_ms": best, "median_ms": statistics.median(ts), "all_ms": ts, "tb_s": nbytes / best / 1e9,
                    "share_of_copy": nbytes / (best * 1e-3) / COPY_RATE, "gpu_ms_per_image": best / a.batch,
                    "pillow_ms_per_image": row["pillow_pool_ms"] / np_ * H / rows})
        row["speedup_per_image"] = row["pillow_ms_per_image"] / row["gpu_ms_per_image"]
        res["filters"][name] = row
        print(f"{name}: {best:.2f} ms (median {row['median_ms']:.2f}), {row['tb_s']:.3f} TB/s = {100 * row['share_of_copy']:.1f} % of copy; "
              f"Pillow on {POOL} threads {row['pillow_pool_ms']:.0f} ms for {np_} images of {rows} rows: {row['speedup_per_image']:.0f} x per image", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
