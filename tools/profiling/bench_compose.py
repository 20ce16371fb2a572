"""paste_many / alpha_composite_many / blend_many / composite_many / chop_many timing: 64 device-resident RGB images of 3840 x 2160
(bench_filter.py's, the natural fixtures mirror-tiled) through blend_many(0.3), chop_many("multiply"), composite_many with an L mask,
alpha_composite_many on RGBA (the same images with an alpha band) and paste_many of ONE shared 512 x 512 RGBA logo with mask="alpha";
and, in the same run as the yardstick, transpose_many("FLIP_LEFT_RIGHT"), which reads and writes every byte once:

    python tools/profiling/bench_compose.py [--batch 64] [--reps 7] [--pillow-images 16] [--out FILE]

    gpu       the call on the whole batch
    pillow    Pillow's own call on the first --pillow-images elements on a pool of 16 threads (host only: no upload, no download),
              compared per image

Every time is a host clock around the whole call, which ends in a stream synchronise; one warm-up call, then --reps timed ones; the
best, the median and the spread (max - min over the median) are kept.  Every row is checked against Pillow on the first 2 elements,
whole, before timing.  `expected` is the row's byte traffic over the RGB flip's: two full reads and one write 1.5, with a one-channel
mask 1.5 + 1/6, the logo paste about 1 (the logo stays in the caches), the RGBA row 1.5 x 4/3; `over` is the row's best time over
expected x the flip's best time: above 1 the row owes an explanation (EXPERIMENTS.md).  Prints one JSON line (and writes it to --out)."""
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
from PIL import Image, ImageChops  # noqa: E402

from bench_filter import COPY_RATE, POOL, A, H, W, tiled  # noqa: E402

AT = (1700, 800)


def _paste(b, logo):
    b = b.copy()
    b.paste(logo, AT, logo)
    return b


# name, ours(firsts, seconds, masks), Pillow's(first, second, mask), expected bytes over the flip's, what the sources are
ROWS = [
    ("FLIP_LEFT_RIGHT (yardstick)", lambda x, y, m: A.transpose_many(x, "FLIP_LEFT_RIGHT"), lambda a, b, m: a.transpose(Image.Transpose.FLIP_LEFT_RIGHT), 1.0, "rgb"),
    ("blend_many(0.3)", lambda x, y, m: A.blend_many(x, y, 0.3), lambda a, b, m: Image.blend(a, b, 0.3), 1.5, "rgb"),
    ("chop_many('multiply')", lambda x, y, m: A.chop_many(x, y, "multiply"), lambda a, b, m: ImageChops.multiply(a, b), 1.5, "rgb"),
    ("composite_many, L mask", lambda x, y, m: A.composite_many(x, y, m), lambda a, b, m: Image.composite(a, b, m), 1.5 + 1 / 6, "rgb"),
    ("alpha_composite_many RGBA", lambda x, y, m: A.alpha_composite_many(x, y), lambda a, b, m: Image.alpha_composite(a, b), 1.5 * 4 / 3, "rgba"),
    ("paste_many, shared 512 x 512 RGBA logo", lambda x, y, m: A.paste_many(x, y, AT, "alpha"), lambda a, b, m: _paste(a, b), 1.0, "logo"),
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
    n = a.batch
    np_ = max(2, min(a.pillow_images, n))
    rng = np.random.default_rng(3)
    images = [torch.from_numpy(x).cuda() for x in host]
    order = [(i + 1) % n for i in range(n)]                    # image i's partner is image i + 1
    mask_host = [np.ascontiguousarray(host[order[i]][..., 1]) for i in range(np_)]
    masks = [images[order[i]][..., 1].contiguous() for i in range(n)]
    alpha = lambda x: np.concatenate([x, (x[..., :1] // 2 + x[..., 1:2] // 2)], axis=2)      # noqa: E731
    rgba = [torch.cat([t, (t[..., :1] // 2 + t[..., 1:2] // 2)], dim=2).contiguous() for t in images]
    logo_host = rng.integers(0, 256, (512, 512, 4), dtype=np.uint8)
    logo_host[..., 3] = np.clip(np.hypot(*np.mgrid[-256:256, -256:256]) * 1.2, 0, 255).astype(np.uint8)[::-1]
    logo = torch.from_numpy(logo_host).cuda()
    res = {"batch": n, "H": H, "W": W, "copy_rate_tb_s": COPY_RATE / 1e12, "pool": POOL, "reps": a.reps, "pillow_images": np_, "rows": {}}
    flip_best = None
    for name, ours, theirs, expected, what in ROWS:
        if what == "rgba":
            firsts, seconds, ms = rgba, [rgba[j] for j in order], None
            triples = [(alpha(host[i]), alpha(host[order[i]]), None) for i in range(np_)]
        elif what == "logo":
            firsts, seconds, ms = images, logo, None
            triples = [(host[i], logo_host, None) for i in range(np_)]
        else:
            firsts, seconds, ms = images, [images[j] for j in order], masks
            triples = [(host[i], host[order[i]], mask_host[i]) for i in range(np_)]
        pil = lambda x: None if x is None else Image.fromarray(x)      # noqa: E731
        t0 = time.perf_counter()
        with ThreadPoolExecutor(POOL) as pool:
            want = list(pool.map(lambda t: np.asarray(theirs(pil(t[0]), pil(t[1]), pil(t[2]))), triples))
        row = {"pillow_pool_ms": (time.perf_counter() - t0) * 1e3}
        del triples
        got = ours(firsts, seconds, ms)                          # the warm-up, and the check: whole images against Pillow's
        for i in range(2):
            assert np.array_equal(got[i].cpu().numpy(), want[i]), (name, i)
        del got, want
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ours(firsts, seconds, ms)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            del out
        best, med = min(ts), statistics.median(ts)
        if flip_best is None:
            flip_best = best
        nbytes = expected * 2 * n * H * W * 3
        row.update({"best_ms": best, "median_ms": med, "spread": (max(ts) - min(ts)) / med, "all_ms": ts, "expected": expected,
                    "over": best / (expected * flip_best), "tb_s": nbytes / best / 1e9, "gpu_ms_per_image": best / n,
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
