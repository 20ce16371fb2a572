"""filter_many timing: 64 device-resident RGB images of 3840 x 2160 -- the natural fixtures (tests/golden/natural) mirror-tiled as
tools/benchlib/data.py's natural_batch tiles them -- through GaussianBlur(2), UnsharpMask(2, 150, 3), BoxBlur(5) and GaussianBlur(20),
and through three filters around the fused kernel's halo limit, on both kernel paths:

    python tools/profiling/bench_filter.py [--batch 64] [--reps 5] [--out FILE]

    fused     filter_many(images, F, _path="fused")     one launch, the whole filter in LDS (only where the halo allows)
    passes    filter_many(images, F, _path="passes")    one launch per pass through the workspace
    pillow    Image.fromarray(a).filter(F) over the same images on a pool of 16 threads (host only: no upload, no download)

Every time is a host clock around the whole call, which ends in a stream synchronise; one warm-up call of each way, then --reps rounds
in which the two paths alternate; the best and the median are kept.  The rate is the algorithm's bytes -- one read and one write of
the images -- over the best time, also as a share of the 6.29 TB/s the project has measured for a device copy.  Both paths are checked
against Pillow on the first 2 images before timing.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image, ImageFilter  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402

H, W = 2160, 3840
POOL = 16
COPY_RATE = 6.29e12
FILTERS = [("GaussianBlur(2)", ImageFilter.GaussianBlur(2)), ("UnsharpMask(2,150,3)", ImageFilter.UnsharpMask(2, 150, 3)),
           ("BoxBlur(5)", ImageFilter.BoxBlur(5)), ("GaussianBlur(20)", ImageFilter.GaussianBlur(20))]
AROUND_THE_LIMIT = [("GaussianBlur(3.5)", ImageFilter.GaussianBlur(3.5)), ("GaussianBlur(5)", ImageFilter.GaussianBlur(5)),
                    ("BoxBlur(15)", ImageFilter.BoxBlur(15))]


def tiled(b, seed=0):
    """image b of natural_batch(torch, B, H, W, seed, device) as uint8 levels, on the host"""
    d = os.path.join(ROOT, "tests", "golden", "natural")
    names = sorted(f for f in os.listdir(d) if f.endswith(".png"))
    k = seed + b
    src = np.asarray(Image.open(os.path.join(d, names[k % len(names)])).convert("RGB"))
    period = np.concatenate([np.concatenate([src, src[:, ::-1]], 1), np.concatenate([src[::-1], src[::-1, ::-1]], 1)], 0)
    ph, pw = period.shape[:2]
    ys, xs = (np.arange(H) + (k * 37) % ph) % ph, (np.arange(W) + (k * 53) % pw) % pw
    return np.ascontiguousarray(period[ys][:, xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    with ThreadPoolExecutor(POOL) as pool:
        host = list(pool.map(tiled, range(a.batch)))
    images = [torch.from_numpy(x).cuda() for x in host]
    nbytes = 2 * a.batch * H * W * 3
    limit = A.filters.filter_geometry()["max_halo"]
    res = {"batch": a.batch, "H": H, "W": W, "algorithmic_mb": nbytes / 1e6, "copy_rate_tb_s": COPY_RATE / 1e12, "pool": POOL, "reps": a.reps,
           "max_halo": limit, "filters": {}}
    print(f"{a.batch} images, {nbytes / 2e6:.1f} MB", flush=True)
    for name, f in FILTERS + AROUND_THE_LIMIT:
        xy = f.radius if isinstance(f.radius, (tuple, list)) else (f.radius, f.radius)
        halo = max(A.filters._halo(A.filters.filter_plan(f.name, xy[0], xy[1])))
        paths = (["fused"] if halo <= limit else []) + ["passes"]
        row = {"halo": halo}
        if (name, f) in FILTERS:
            t0 = time.perf_counter()
            with ThreadPoolExecutor(POOL) as pool:
                want = list(pool.map(lambda x: np.asarray(Image.fromarray(x).filter(f)), host))
            row["pillow_pool_ms"] = (time.perf_counter() - t0) * 1e3
            want = want[:2]
        else:
            want = [np.asarray(Image.fromarray(x).filter(f)) for x in host[:2]]
        for p in paths:                                      # the check, and the warm-up of every shape the timed calls use
            got = A.filter_many(images, f, _path=p)
            for i, w in enumerate(want):
                assert np.array_equal(got[i].cpu().numpy(), w), (name, p, i)
            del got
        ts = {p: [] for p in paths}
        for _ in range(a.reps):
            for p in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = A.filter_many(images, f, _path=p)
                torch.cuda.synchronize()
                ts[p].append((time.perf_counter() - t0) * 1e3)
                del out
        for p in paths:
            best = min(ts[p])
            row[p] = {"best_ms": best, "median_ms": statistics.median(ts[p]), "all_ms": ts[p], "tb_s": nbytes / best / 1e9,
                      "share_of_copy": nbytes / (best * 1e-3) / COPY_RATE}
        res["filters"][name] = row
        print(f"{name}: halo {halo}; " + "; ".join(f"{p} {row[p]['best_ms']:.2f} ms (median {row[p]['median_ms']:.2f}), {row[p]['tb_s']:.2f} TB/s = "
                                                 f"{100 * row[p]['share_of_copy']:.1f} % of copy" for p in paths)
              + (f"; Pillow on {POOL} threads {row['pillow_pool_ms']:.0f} ms" if "pillow_pool_ms" in row else ""), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
