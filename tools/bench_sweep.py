"""Rate-distortion sweep timing: A.sweep() against a per-cell loop of the existing public calls, interleaved in one process.

    python tools/bench_sweep.py [--repeats 3] [--workloads natural,4k] [--sizes none,gpu,zlib] [--out FILE]

Workloads
  natural  the reference study's grid (A.reference_grid(): YCbCr x 15 quality ranges x 21 block ranges = 315 cells) on the six natural
           test images (tests/golden/natural); "zlib" sizes on the first --zlib-block-ranges block ranges only (host zlib-9 dominates)
  4k       8 synthetic 2160 x 3840 images (oracle.synth_image), YCbCr x 5 quality ranges x 3 block ranges = 15 cells; no "zlib"
The loop per cell: compress_batch -> decompress_batch -> EvaluationMetrics.batch (PSNR | SSIM | MS-SSIM), plus compress_many for the
sizes ("zlib": host level 9, "gpu": entropy="gpu").  Both sides start from the same device-resident (or, for mixed sizes, host) images.
Every time is a host clock around work that ends in a device synchronise, after one warm-up of each side; sweep and loop alternate.
Prints one JSON line (and writes it to --out).  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` in a separate run.
"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
from adaptive_edge_aware_jpeg_amd.evaluation_metrics import MS_SSIM, PSNR, SSIM  # noqa: E402

NATURAL = ("baboon", "bikes", "buildings", "house", "jelly_beans", "peppers")


def natural_images():
    from PIL import Image as PILImage
    d = os.path.join(ROOT, "tests", "golden", "natural")
    return [np.asarray(PILImage.open(os.path.join(d, n + ".png")).convert("RGB")).astype(np.float32) / np.float32(255.0) for n in NATURAL]


def synthetic_4k(n):
    from oracle import oracle as O
    return np.stack([O.synth_image(2160, 3840, 7000 + i).astype(np.float32) / np.float32(255.0) for i in range(n)])


def loop(groups, grid, sizes):
    """the per-cell loop of the existing public calls; groups: [(image indices, device batch)]"""
    out = []
    for cs, qr, br in itertools.product(*grid):
        codec = A.Jpeg(A.JpegCompressionSettings(cs, qr, br))
        for _, x in groups:
            m = A.EvaluationMetrics.batch(x, codec.decompress_batch(codec.compress_batch(x)), PSNR | SSIM | MS_SSIM)
            if sizes == "zlib":
                out.append(len(b"".join(codec.compress_many(x, extension=".png"))))
            elif sizes == "gpu":
                out.append(len(b"".join(codec.compress_many(x, extension=".png", entropy="gpu"))))
            out.append(m)
    torch.cuda.synchronize()
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default="natural,4k")
    ap.add_argument("--sizes", default="none,gpu,zlib")
    ap.add_argument("--zlib-block-ranges", type=int, default=3)
    ap.add_argument("--images-4k", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sweep.py measures on the GPU"
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "cases": []}
    for wl in a.workloads.split(","):
        if wl == "natural":
            imgs = natural_images()
            spaces, qrs, brs = A.reference_grid()
            shapes = {}
            for i, x in enumerate(imgs):
                shapes.setdefault(x.shape, []).append(i)
            groups = [(idx, torch.from_numpy(np.stack([imgs[i] for i in idx])).to(dev)) for idx in shapes.values()]
            sweep_in = imgs
        else:
            x = torch.from_numpy(synthetic_4k(a.images_4k)).to(dev)
            spaces, qrs, brs = ("YCbCr",), [(10, 50), (25, 75), (40, 80), (50, 90), (90, 90)], [(4, 64), (8, 32), (16, 128)]
            groups = [(list(range(a.images_4k)), x)]
            sweep_in = x
        for sz in a.sizes.split(","):
            sizes = None if sz == "none" else sz
            if sizes == "zlib" and wl != "natural":
                continue
            grid = (spaces, qrs, brs[:a.zlib_block_ranges] if sizes == "zlib" else brs)
            n_cells = len(grid[0]) * len(grid[1]) * len(grid[2])
            run_sweep = lambda: A.sweep(sweep_in, *grid, sizes=sizes, extension=".png")      # noqa: E731
            run_loop = lambda: loop(groups, grid, sizes)                                      # noqa: E731
            run_sweep()
            run_loop()
            ts, tl = [], []
            for _ in range(a.repeats):
                ts.append(timed(run_sweep))
                tl.append(timed(run_loop))
            case = {"workload": wl, "sizes": sz, "cells": n_cells, "images": sum(len(i) for i, _ in groups),
                    "sweep_ms_per_cell": [round(1e3 * t / n_cells, 3) for t in ts], "loop_ms_per_cell": [round(1e3 * t / n_cells, 3) for t in tl],
                    "speedup_median": round(float(np.median(tl) / np.median(ts)), 2)}
            result["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
