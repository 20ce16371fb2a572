"""Standard-JPEG timing: 64 x 4K images through csrc/jfif.hip, per quality and with the five qualities of the reference comparison
(10, 25, 50, 75, 90) in one call, against Pillow's save + load on a thread pool.

    python tools/bench_jfif.py [--batch 64] [--repeats 3] [--threads 16] [--subsampling 4:2:0] [--optimize] [--progressive]
                               [--grouped-only] [--no-pillow] [--transcode [--ab ROOT] [--routes a,b]] [--out FILE]

--subsampling / --optimize / --progressive are Pillow's keywords of the same names, given to both sides; --grouped-only times the five-quality call
alone and --no-pillow leaves the CPU side out (for A/B runs of the library against itself).  --transcode is a mode of its own: the
lossless transcoder against decode + encode over pixels (see transcode()).

"encode" is aej_jfif_encode_batch writing the files to device memory (the library waits for the total length at its end); "encode+recon"
adds aej_jfif_recon_batch, Pillow's decode of every file as device uint8.  Neither copies the files back to the host.  Pillow does
Image.fromarray(x).save(buf, "JPEG", quality=q) and then np.asarray(Image.open(buf).convert("RGB")) for each image, on --threads threads.
Every time is a host clock around work that ends in a device synchronise, after one warm-up; the median of --repeats is reported, as
gigapixels per second (images x H x W x qualities / time).  Prints one JSON line (and writes it to --out).
"""
import argparse
import inspect
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --root DIR: import the package of another checkout (the --ab worker); the test images always come from this one
sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv[1:-1] else ROOT)

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


def transcode_routes(a):
    """name -> callable returning the bytes a route wrote (0 where it writes none), for the package this process imported"""
    x = images(a.batch)
    files = A.standard_jpeg_many(x, 75, subsampling=a.subsampling)
    xd = A._lib.get_context(0).to_device(x, torch.uint8)

    def pixels(**kw):
        dec = A.standard_jpeg_decode_many(files)
        return sum(len(f) for f in A.standard_jpeg_many(torch.stack(dec), 75, subsampling=a.subsampling, **kw))

    def batch_default():
        A.standard_jpeg_batch(xd, [75])
        return 0

    def decode_default():
        A.standard_jpeg_decode_many(files)
        return 0

    routes = {"decode_encode_optimize": lambda: pixels(optimize=True), "decode_encode_progressive": lambda: pixels(progressive=True),
              "standard_jpeg_batch": batch_default, "standard_jpeg_decode_many": decode_default}
    if hasattr(A, "standard_jpeg_transcode_many"):
        routes["transcode_optimize"] = lambda: sum(len(f) for f in A.standard_jpeg_transcode_many(files, progressive=False))
        routes["transcode_progressive"] = lambda: sum(len(f) for f in A.standard_jpeg_transcode_many(files, progressive=True))
    if hasattr(A, "standard_jpeg_transform_many"):               # the transcode with a lossless transform on the way, over the same files
        routes["transform_rot90"] = lambda: sum(len(f) for f in A.standard_jpeg_transform_many(files, "rot90", progressive=False))
        routes["transform_flip_h"] = lambda: sum(len(f) for f in A.standard_jpeg_transform_many(files, "flip_h", progressive=False))
    if hasattr(A, "standard_jpeg_encode_many"):                  # the ragged encoder over the same frames, already on the device
        frames = [xd[i] for i in range(a.batch)]
        many = lambda **kw: sum(len(f) for f in A.standard_jpeg_encode_many(frames, 75, subsampling=a.subsampling, **kw))  # noqa: E731
        routes["encode_many_annexk"] = lambda: many()
        routes["encode_many_optimize"] = lambda: many(optimize=True)
        routes["encode_many_progressive"] = lambda: many(progressive=True)
        if "restart_marker_rows" in inspect.signature(A.standard_jpeg_encode_many).parameters:      # restart markers: one per MCU row
            rows = dict(restart_marker_rows=1)
            routes["encode_many_annexk_rows1"] = lambda: many(**rows)
            routes["encode_many_optimize_rows1"] = lambda: many(optimize=True, **rows)
            routes["encode_many_progressive_rows1"] = lambda: many(progressive=True, **rows)
            routes["transcode_optimize_rows1"] = lambda: sum(len(f) for f in A.standard_jpeg_transcode_many(files, progressive=False, **rows))
            routes["transcode_progressive_rows1"] = lambda: sum(len(f) for f in A.standard_jpeg_transcode_many(files, progressive=True, **rows))
    return routes, sum(len(f) for f in files)


def run_route(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nbytes = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, int(nbytes)


def worker(a):
    """--worker: name the routes this package has ("@@ ready a,b,..."), then serve one route per line of standard input, answer
    "@@ <ms> <bytes>" (the other side of --ab: a process that imported the package of another checkout through --root)"""
    routes, _ = transcode_routes(a)
    print("@@ ready " + ",".join(routes), flush=True)
    for line in sys.stdin:
        name = line.strip()
        if name == "quit":
            break
        ms, nbytes = run_route(routes[name])
        print(f"@@ {ms} {nbytes}", flush=True)


def transcode(a):
    """--transcode: --batch natural 4K files (quality 75, --subsampling, plain baseline) through standard_jpeg_transcode_many to
    optimised baseline and to progressive files, beside the lossy route over pixels on the same files (standard_jpeg_decode_many, then
    standard_jpeg_many(optimize=True / progressive=True)) and the plain standard_jpeg_batch / standard_jpeg_decode_many calls; the
    routes transform_rot90 and transform_flip_h are standard_jpeg_transform_many over the same files (baseline output); encode_many_*
    are standard_jpeg_encode_many (the ragged encoder) over the same frames as device tensors, under the Annex K tables, optimised and
    progressive, and the *_rows1 routes are the ragged encoder and the transcoder with restart_marker_rows=1.  With
    --ab ROOT a second process imports the package of the checkout at ROOT (its library built there) and runs the routes it has; the
    two sides alternate route by route inside every round, so both see the same machine state.  One warm-up round, then the medians
    of --repeats rounds, with the bytes of the sources and of the outputs.  --routes a,b restricts the run (for a profiler)."""
    import subprocess
    routes, source_bytes = transcode_routes(a)
    if a.routes:
        routes = {k: routes[k] for k in a.routes.split(",")}
    child, sides = None, {"branch": list(routes)}
    if a.ab:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--root", a.ab, "--batch", str(a.batch), "--subsampling",
                                  a.subsampling], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

        def answer():
            for line in child.stdout:
                if line.startswith("@@ "):
                    return line.split()[1:]
            raise RuntimeError("the --ab worker ended")

        has = answer()[1].split(",")                   # the routes the other checkout's package offers
        sides["parent"] = [k for k in routes if k in has]

    def ask(name):
        child.stdin.write(name + "\n")
        child.stdin.flush()
        ms, nbytes = answer()
        return float(ms), int(nbytes)

    times = {s: {k: [] for k in ks} for s, ks in sides.items()}
    size = {s: {} for s in sides}
    for r in range(a.repeats + 1):
        for k in routes:
            for s in sides:
                if k not in times[s]:
                    continue
                ms, nbytes = run_route(routes[k]) if s == "branch" else ask(k)
                if r:
                    times[s][k].append(ms)
                size[s][k] = nbytes
    if child:
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait()
    res = {"mode": "transcode", "batch": a.batch, "H": H, "W": W, "subsampling": a.subsampling, "quality": 75, "repeats": a.repeats,
           "source_bytes": source_bytes, "output_bytes": size,
           "ms": {s: {k: float(np.median(v)) for k, v in t.items()} for s, t in times.items()}, "ms_all": times}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


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
    ap.add_argument("--transcode", action="store_true")
    ap.add_argument("--ab", metavar="ROOT")
    ap.add_argument("--routes")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.transcode:
        return transcode(a)
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
