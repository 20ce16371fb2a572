"""PNG decode timing: 64 PNG files of 3840 x 2160 -- the natural fixtures (tests/golden/natural) mirror-tiled as
tools/benchlib/data.py's natural_batch tiles them, saved by Pillow at its default compression level -- decoded three ways:

    python tools/profiling/bench_png_decode.py [--batch 64] [--out FILE]

    gpu_inflate    png_decode_many(files, inflate="gpu")     IDAT bytes up in one copy, aej_inflate_batch (one wave per file), un-filter
    host_inflate   png_decode_many(files, inflate="host")    zlib.decompress on a pool of 16 threads, scanlines up, un-filter
    pillow_pool    np.asarray(Image.open(f).convert("RGB")) on a pool of 16 threads, then the upload of its pixels (uint8)

Every time is a host clock around the whole call, ending in a device synchronise; the best of 2 after one warm-up call.  The device
results are checked against Pillow on the first 2 files before timing.  The two kernels' times (events around aej_inflate_batch and
aej_png_unfilter_batch in one more call of either way) are printed beside them.  Prints one JSON line (and writes it to --out)."""
import argparse
import io
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
from adaptive_edge_aware_jpeg_amd import png as P  # noqa: E402
from adaptive_edge_aware_jpeg_amd._lib import get_context  # noqa: E402

H, W = 2160, 3840
POOL = 16


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


def save(b):
    buf = io.BytesIO()
    Image.fromarray(tiled(b)).save(buf, "PNG")
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    with ThreadPoolExecutor(POOL) as pool:
        files = list(pool.map(save, range(a.batch)))
    print(f"{a.batch} files, {sum(map(len, files)) / 1e6:.1f} MB", flush=True)

    def pillow_pool():
        with ThreadPoolExecutor(POOL) as pool:
            px = list(pool.map(lambda f: np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), files))
        return [torch.from_numpy(x).cuda() for x in px]

    ways = {"gpu_inflate": lambda: A.png_decode_many(files, inflate="gpu"),
            "host_inflate": lambda: A.png_decode_many(files, inflate="host", workers=POOL),
            "pillow_pool": pillow_pool}
    for i in range(min(2, a.batch)):
        want = np.asarray(Image.open(io.BytesIO(files[i])).convert("RGB"))
        for how in ("gpu", "host"):
            assert np.array_equal(A.png_decode_many(files[i:i + 1], inflate=how)[0].cpu().numpy(), want), (i, how)
    filters = np.bincount(np.concatenate([np.frombuffer(zlib.decompress(b"".join(files[i][o:o + k] for o, k in A.png_parse_header(files[i]).idat_spans)),
                                                        np.uint8)[::1 + 3 * W] for i in range(min(2, a.batch))]), minlength=5)
    res = {"batch": a.batch, "H": H, "W": W, "file_mb": sum(map(len, files)) / 1e6, "pixel_mb": a.batch * H * W * 3 / 1e6,
           "filter_rows_of_2_files": filters.tolist(), "pool": POOL, "best_of": 2, "ms": {}, "kernel_ms": {}}
    for way, fn in ways.items():
        ts = []
        for r in range(3):                                   # call 0: the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
        res["ms"][way] = {"best": min(ts), "both": ts}
        print(f"{way}: {min(ts):.2f} ms (best of 2: {ts[0]:.2f}, {ts[1]:.2f})", flush=True)
    ctx = get_context(0)
    parsed = [A.png_parse_header(f, i) for i, f in enumerate(files)]
    views = [memoryview(f) for f in files]
    for how in ("gpu", "host"):
        ev = {}
        P._decode_parsed(ctx, parsed, views, ["RGB"] * a.batch, how, POOL, events=ev)
        torch.cuda.synchronize()
        res["kernel_ms"][how] = {k: v[0].elapsed_time(v[1]) for k, v in ev.items()}
        print(f"kernels, inflate={how!r}: " + ", ".join(f"{k} {ms:.2f} ms" for k, ms in res["kernel_ms"][how].items()), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
