"""filter_many timing for Color3DLUT: 64 device-resident RGB images of 3840 x 2160 (bench_filter.py's, the natural fixtures
mirror-tiled) through tables of size 17 and 33 with 3 channels, size 65 with 3 and with 4 channels (RGBA out), and the same images with
an alpha channel through a 4-channel table; and in the same run, as yardsticks,
transpose_many(FLIP_LEFT_RIGHT) and convert_many(RGB -> YCbCr) -- the project's cheapest one-read-one-write calls -- and a device copy
of the images' bytes:

    python tools/profiling/bench_lut3d.py [--batch 64] [--reps 5] [--warmup 3] [--pillow-images 16] [--out FILE]

    gpu       filter_many(images, table)
    pillow    Image.fromarray(a).filter(table) over the first --pillow-images images on a pool of 16 threads (host only)

Every time is a host clock around the whole call, which ends in a stream synchronise; --warmup warm-up calls (three: the first
timed calls after a single one still fall from run to run), then --reps timed ones; the
best and the median are kept.  The rate is the algorithm's bytes -- one read and one write of the images -- over the best time, also
as a share of the copy measured in this run.  Every table is checked against Pillow on the first 2 images before timing.  Prints one
JSON line (and writes it to --out)."""
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

from bench_filter import POOL, A, H, W, tiled  # noqa: E402


def look(size, channels, target_mode=None):
    """a film look as a table: a contrast curve per channel, a little cross-talk, lifted shadows; values leave [0, 1] in places"""
    g = np.linspace(0.0, 1.0, size)
    b, gr, r = np.meshgrid(g, g, g, indexing="ij")
    curve = lambda v: 0.5 + 1.15 * (v - 0.5) + 0.25 * np.sin(2 * np.pi * v) / (2 * np.pi)      # noqa: E731
    planes = [curve(0.9 * r + 0.1 * gr) + 0.02, curve(0.05 * r + 0.9 * gr + 0.05 * b), curve(0.15 * gr + 0.85 * b) - 0.03]
    if channels == 4:
        planes.append(0.25 + 0.75 * (0.299 * r + 0.587 * gr + 0.114 * b))
    return ImageFilter.Color3DLUT(size, np.stack(planes, -1).astype(np.float32), channels, target_mode)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del out
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pillow-images", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    with ThreadPoolExecutor(POOL) as pool:
        host = list(pool.map(tiled, range(a.batch)))
    alpha = ((np.arange(H)[:, None] + 3 * np.arange(W)[None, :]) % 256).astype(np.uint8)
    host4 = [np.dstack([x, alpha]) for x in host[:max(2, min(a.pillow_images, a.batch))]]
    rgb = [torch.from_numpy(x).cuda() for x in host]
    rgba = [torch.cat([x, torch.from_numpy(alpha).cuda()[:, :, None]], 2).contiguous() for x in rgb]
    n_pil = len(host4)
    res = {"batch": a.batch, "H": H, "W": W, "pool": POOL, "reps": a.reps, "warmup": a.warmup, "pillow_images": n_pil, "geometry": A.filters.lut3d_geometry(), "rows": {}}

    # the copy of this run: the RGB images' bytes from one buffer to another
    flat = torch.cat([x.reshape(-1) for x in rgb])
    other = torch.empty_like(flat)
    other.copy_(flat)
    ts = timed(lambda: other.copy_(flat), a.reps)
    copy_rate = 2 * flat.numel() / (min(ts) * 1e-3)
    res["copy"] = {"best_ms": min(ts), "median_ms": statistics.median(ts), "all_ms": ts, "tb_s": copy_rate / 1e12}
    print(f"{a.batch} images, {flat.numel() / 1e6:.1f} MB; device copy {min(ts):.3f} ms = {copy_rate / 1e12:.3f} TB/s", flush=True)
    del flat, other

    def row(name, ts, nbytes, extra=None):
        best = min(ts)
        r = {"best_ms": best, "median_ms": statistics.median(ts), "all_ms": ts, "spread_ms": max(ts) - best, "algorithmic_mb": nbytes / 1e6,
             "tb_s": nbytes / best / 1e9, "share_of_copy": nbytes / (best * 1e-3) / copy_rate, "gpu_ms_per_image": best / a.batch}
        r.update(extra or {})
        res["rows"][name] = r
        print(f"{name}: {best:.3f} ms (median {r['median_ms']:.3f}), {r['tb_s']:.3f} TB/s = {100 * r['share_of_copy']:.1f} % of the copy"
              + (f"; Pillow on {POOL} threads {r['pillow_pool_ms']:.0f} ms for {n_pil} images: {r['speedup_per_image']:.0f} x per image" if extra else ""), flush=True)

    px = a.batch * H * W
    rows = [("size17_rgb", rgb, host, look(17, 3), 3), ("size33_rgb", rgb, host, look(33, 3), 3), ("size65_rgb", rgb, host, look(65, 3), 3),
            ("size65_rgb_4ch_table", rgb, host, look(65, 4, "RGBA"), 4), ("size33_rgba_4ch_table", rgba, host4, look(33, 4), 4)]
    for name, images, plain, f, co in rows:
        small = A.filter_many(plain[:2], f)                       # the check: what Pillow filtered
        with ThreadPoolExecutor(POOL) as pool:
            for i, w in enumerate(pool.map(lambda x: np.asarray(Image.fromarray(x).filter(f)), plain[:2])):
                assert np.array_equal(small[i].cpu().numpy(), w), (name, i)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(POOL) as pool:
            list(pool.map(lambda x: Image.fromarray(x).filter(f), plain[:n_pil]))
        pillow_ms = (time.perf_counter() - t0) * 1e3
        del small
        for _ in range(a.warmup):
            A.filter_many(images, f)
        ts = timed(lambda: A.filter_many(images, f), a.reps)
        nbytes = px * (images[0].shape[2] + co)
        row(name, ts, nbytes, {"pillow_pool_ms": pillow_ms, "pillow_ms_per_image": pillow_ms / n_pil,
                               "speedup_per_image": pillow_ms / n_pil / (min(ts) / a.batch)})

    # the yardsticks
    for name, fn in (("FLIP_LEFT_RIGHT", lambda: A.transpose_many(rgb, "FLIP_LEFT_RIGHT")), ("convert_RGB_to_YCbCr", lambda: A.convert_many(rgb, "YCbCr"))):
        for _ in range(a.warmup):
            fn()
        row(name, timed(fn, a.reps), px * 6)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
