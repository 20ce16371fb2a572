"""Standard-JPEG timing: 64 x 4K images through csrc/jfif.hip, per quality and with the five qualities of the reference comparison
(10, 25, 50, 75, 90) in one call, against Pillow's save + load on a thread pool.

    python tools/bench_jfif.py [--batch 64] [--repeats 3] [--threads 16] [--subsampling 4:2:0] [--optimize] [--progressive]
                               [--grouped-only] [--no-pillow] [--out FILE]

--subsampling / --optimize / --progressive are Pillow's keywords of the same names, given to both sides; --grouped-only times the five-quality call
alone and --no-pillow leaves the CPU side out (for A/B runs of the library against itself).

"encode" is aej_jfif_encode_batch writing the files to device memory (the library waits for the total length at its end); "encode+recon"
adds aej_jfif_recon_batch, Pillow's decode of every file as device uint8.  Neither copies the files back to the host.  Pillow does
Image.fromarray(x).save(buf, "JPEG", quality=q) and then np.asarray(Image.open(buf).convert("RGB")) for each image, on --threads threads.
Every time is a host clock around work that ends in a device synchronise, after one warm-up; the median of --repeats is reported, as
gigapixels per second (images x H x W x qualities / time).  Prints one JSON line (and writes it to --out).
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
from adaptive_edge_aware_jpeg_amd import standard_jpeg as S  # noqa: E402

H, W = 2160, 3840
QUALITIES = (10, 25, 50, 75, 90)


def images(n):
    """n different 4K frames: the natural test images tiled, mirrored and shifted"""
    srcs = [np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "natural", f + ".png")).convert("RGB"))
            for f in ("baboon", "bikes", "buildings", "house", "jelly_beans", "peppers")]
    out = np.empty((n, H, W, 3), np.uint8)
    for i in range(n):
        s = srcs[i % len(srcs)]
        t = np.concatenate([s, s[:, ::-1]], 1)
        t = np.concatenate([t, t[::-1]], 0)
        reps = (-(-H // t.shape[0]) + 1, -(-W // t.shape[1]) + 1)
        big = np.tile(t, (reps[0], reps[1], 1))
        dy, dx = (37 * i) % t.shape[0], (53 * i) % t.shape[1]
        out[i] = big[dy:dy + H, dx:dx + W]
    return out


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--subsampling", default="4:2:0", choices=("4:4:4", "4:2:2", "4:2:0"))
    ap.add_argument("--optimize", action="store_true")
    ap.add_argument("--progressive", action="store_true")
    ap.add_argument("--grouped-only", action="store_true")
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    kw = dict(subsampling=a.subsampling, optimize=a.optimize, progressive=a.progressive)
    x = images(a.batch)
    ctx = A._lib.get_context(0)
    xd = ctx.to_device(x, torch.uint8)
    gp = a.batch * H * W / 1e9
    res = {"batch": a.batch, "H": H, "W": W, "subsampling": a.subsampling, "optimize": a.optimize, "progressive": a.progressive, "per_quality": {}}

    def enc(qs, recon):
        e = S.encode_decode(ctx, xd, qs, want_bytes=True, **kw)
        if recon:
            e.decoded()
        return e

    for q in () if a.grouped_only else QUALITIES:
        te = timed(lambda: enc([q], False), a.repeats)
        tr = timed(lambda: enc([q], True), a.repeats)
        mb = float(enc([q], False).lengths.sum()) / 1e6
        res["per_quality"][q] = {"encode_ms": te * 1e3, "encode_gps": gp / te, "encode_recon_ms": tr * 1e3, "encode_recon_gps": gp / tr,
                                 "file_mb": mb}
        print(f"q={q:3d}: encode {te * 1e3:8.1f} ms ({gp / te:6.2f} GP/s), +recon {tr * 1e3:8.1f} ms ({gp / tr:6.2f} GP/s), {mb:.1f} MB of files",
              flush=True)
    te = timed(lambda: enc(list(QUALITIES), False), a.repeats)
    tr = timed(lambda: enc(list(QUALITIES), True), a.repeats)
    n = len(QUALITIES)
    res["grouped"] = {"encode_ms": te * 1e3, "encode_gps": n * gp / te, "encode_recon_ms": tr * 1e3, "encode_recon_gps": n * gp / tr,
                      "file_mb": float(enc(list(QUALITIES), False).lengths.sum()) / 1e6}
    print(f"5 qualities in one call: encode {te * 1e3:.1f} ms ({n * gp / te:.2f} GP/s), +recon {tr * 1e3:.1f} ms ({n * gp / tr:.2f} GP/s)", flush=True)

    if a.no_pillow:
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return

    # the GPU's files are Pillow's: check one image per quality before timing Pillow
    for q in QUALITIES:
        buf = io.BytesIO()
        Image.fromarray(x[0]).save(buf, "JPEG", quality=q, **kw)
        assert A.standard_jpeg_many(x[:1], q, **kw)[0] == buf.getvalue(), q

    def pil_one(i, q, load):
        buf = io.BytesIO()
        Image.fromarray(x[i]).save(buf, "JPEG", quality=q, **kw)
        if load:
            buf.seek(0)
            np.asarray(Image.open(buf).convert("RGB"))
        return buf.tell()

    pool = ThreadPoolExecutor(a.threads)
    pil = {}
    for load in (False, True):
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for q in QUALITIES:
                list(pool.map(lambda i: pil_one(i, q, load), range(a.batch)))
            ts.append(time.perf_counter() - t0)
        pil["save_load" if load else "save"] = n * gp / float(np.median(ts))
    pool.shutdown()
    res["pillow_threads"] = a.threads
    res["pillow_save_gps"], res["pillow_save_load_gps"] = pil["save"], pil["save_load"]
    res["speedup_encode"] = res["grouped"]["encode_gps"] / pil["save"]
    res["speedup_encode_recon"] = res["grouped"]["encode_recon_gps"] / pil["save_load"]
    print(f"Pillow on {a.threads} threads: save {pil['save']:.3f} GP/s, save+load {pil['save_load']:.3f} GP/s", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
