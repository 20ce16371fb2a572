"""Lossless crop and chroma drop, timed: 64 natural 4K 4:2:0 files through standard_jpeg_transform_many with crop= and drop_chroma=,
beside the transform "none" (the plain transcode) of the same files on the same commit.

    python tools/bench_jfif_cut.py [--batch 64] [--repeats 5] [--progressive] [--routes a,b] [--out FILE]

Routes (all over the same files, baseline output unless --progressive):
  none         standard_jpeg_transform_many(files, "none"): every block of the source is coded again
  crop_1024    ... crop=(1408, 568, 2432, 1592): the centre 1024 x 1024 of a 3840 x 2160 frame; the corner moves up to the 16 x 16 grid,
               (1408, 560), so the files are 1024 x 1032 (with the chroma dropped the grid is 8 x 8: 1024 x 1024)
  drop_chroma  ... drop_chroma=True: the luma blocks alone, two thirds of the 4:2:0 source's blocks
  crop_drop    both
Every route Huffman-decodes the whole source; only what follows the bridge shrinks with the output.  Every time is a host clock around
work that ends in a device synchronise, after one warm-up round; the routes alternate inside a round, and the median of --repeats
rounds is reported with every single time.  Prints one JSON line (and writes it to --out).  --routes a,b restricts the run, for a
profiler: the per-stage split comes from a kernel trace of one route, not from this clock.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
from bench_jfif import H, W, images  # noqa: E402

CENTRE = ((W - 1024) // 2, (H - 1024) // 2, (W + 1024) // 2, (H + 1024) // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--progressive", action="store_true")
    ap.add_argument("--routes")
    ap.add_argument("--out")
    a = ap.parse_args()
    files = A.standard_jpeg_many(images(a.batch), 75, subsampling="4:2:0")
    T = lambda **kw: A.standard_jpeg_transform_many(files, "none", progressive=a.progressive, **kw)  # noqa: E731
    routes = {"none": lambda: T(), "crop_1024": lambda: T(crop=CENTRE), "drop_chroma": lambda: T(drop_chroma=True),
              "crop_drop": lambda: T(crop=CENTRE, drop_chroma=True)}
    if a.routes:
        routes = {k: routes[k] for k in a.routes.split(",")}
    kept = {False: A.transform_crop_box(files[0], "none", CENTRE), True: A.transform_crop_box(files[0], "none", CENTRE, drop_chroma=True)}
    times, size = {k: [] for k in routes}, {}
    for r in range(a.repeats + 1):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if r:
                times[k].append((time.perf_counter() - t0) * 1e3)
            size[k] = sum(len(f) for f in out)
    mcu = lambda w, h: -(-w // 16) * -(-h // 16)  # noqa: E731
    size_of = lambda b: (b[2] - b[0], b[3] - b[1])  # noqa: E731
    blocks = {"none": 6 * mcu(W, H), "crop_1024": 6 * mcu(*size_of(kept[False])), "drop_chroma": -(-W // 8) * -(-H // 8),
              "crop_drop": -(-size_of(kept[True])[0] // 8) * -(-size_of(kept[True])[1] // 8)}
    res = {"mode": "cut", "batch": a.batch, "H": H, "W": W, "subsampling": "4:2:0", "quality": 75, "progressive": a.progressive,
           "repeats": a.repeats, "crop": CENTRE, "kept": kept[False], "kept_drop_chroma": kept[True], "source_bytes": sum(len(f) for f in files), "output_bytes": size,
           "output_blocks_per_file": {k: blocks[k] for k in routes}, "ms": {k: float(np.median(v)) for k, v in times.items()}, "ms_all": times}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
