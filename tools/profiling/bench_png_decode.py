"""PNG decode timing: 64 PNG files of 3840 x 2160 -- the natural fixtures (tests/golden/natural) mirror-tiled as
tools/benchlib/data.py's natural_batch tiles them, saved by Pillow at its default compression level -- decoded three ways:

    python tools/profiling/bench_png_decode.py [--batch 64] [--out FILE] [--interlaced] [--depth16] [--own-writer]

--interlaced and --depth16 build the same pixels as Adam7-interlaced and / or 16-bit files (sample = 257 x level, so that Pillow's high
byte is the level).  Pillow writes neither, so those files come from a writer in this tool: every row of every pass filtered with
Paeth (numpy, no recurrence on the encoding side), zlib at level 6.  --own-writer builds the plain 8-bit files with that writer too: the
twin to compare an interlaced or 16-bit run with, since Pillow picks other filters.

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
import struct
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


ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))      # x0, y0, dx, dy


def _paeth_rows(rows, bpp):
    """rows [h, rb] uint8 -> the scanline stream of the image with every row filtered by Paeth (type 4)"""
    x = rows.astype(np.int16)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    out = np.empty((rows.shape[0], 1 + rows.shape[1]), np.uint8)
    out[:, 0] = 4
    out[:, 1:] = (x - pred).astype(np.uint8)
    return out.tobytes()


def save_own(b, interlaced, depth16):
    """image b written by this tool: colour type 2, all rows Paeth; interlaced and / or 16 bits deep on request"""
    px = tiled(b)
    if depth16:
        px = (px.astype(np.uint16) * 257).astype(">u2").view(np.uint8).reshape(H, W, 6)
    bpp = px.shape[2]
    if interlaced:
        raw = b"".join(_paeth_rows(np.ascontiguousarray(px[y0::dy, x0::dx]).reshape(-1, len(range(x0, W, dx)) * bpp), bpp)
                       for x0, y0, dx, dy in ADAM7 if x0 < W and y0 < H)
    else:
        raw = _paeth_rows(px.reshape(H, W * bpp), bpp)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16 if depth16 else 8, 2, 0, 0, int(interlaced)))
            + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out")
    ap.add_argument("--interlaced", action="store_true", help="Adam7-interlaced files (this tool's writer)")
    ap.add_argument("--depth16", action="store_true", help="16-bit files (this tool's writer)")
    ap.add_argument("--own-writer", action="store_true", help="plain 8-bit files from this tool's writer, all rows Paeth")
    ap.add_argument("--repeat-kernels", type=int, default=1, help="calls whose kernel times are recorded, per inflate")
    a = ap.parse_args()
    own = a.interlaced or a.depth16 or a.own_writer
    kw = dict(interlaced=True, depth16=True) if own else {}
    with ThreadPoolExecutor(POOL) as pool:
        files = list(pool.map((lambda b: save_own(b, a.interlaced, a.depth16)) if own else save, range(a.batch)))
    print(f"{a.batch} files, {sum(map(len, files)) / 1e6:.1f} MB", flush=True)

    def pillow_pool():
        with ThreadPoolExecutor(POOL) as pool:
            px = list(pool.map(lambda f: np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), files))
        return [torch.from_numpy(x).cuda() for x in px]

    ways = {"gpu_inflate": lambda: A.png_decode_many(files, inflate="gpu", **kw),
            "host_inflate": lambda: A.png_decode_many(files, inflate="host", workers=POOL, **kw),
            "pillow_pool": pillow_pool}
    for i in range(min(2, a.batch)):
        want = np.asarray(Image.open(io.BytesIO(files[i])).convert("RGB"))
        for how in ("gpu", "host"):
            assert np.array_equal(A.png_decode_many(files[i:i + 1], inflate=how, **kw)[0].cpu().numpy(), want), (i, how)
    if own:
        filters = np.bincount([4], minlength=5) * 2 * H      # (the writer's: every row Paeth)
    else:
        filters = np.bincount(np.concatenate([np.frombuffer(zlib.decompress(b"".join(files[i][o:o + k] for o, k in A.png_parse_header(files[i]).idat_spans)),
                                                            np.uint8)[::1 + 3 * W] for i in range(min(2, a.batch))]), minlength=5)
    res = {"batch": a.batch, "H": H, "W": W, "file_mb": sum(map(len, files)) / 1e6, "pixel_mb": a.batch * H * W * 3 / 1e6,
           "interlaced": a.interlaced, "depth16": a.depth16, "writer": "own" if own else "pillow",
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
    parsed = [A.png_parse_header(f, i, **kw) for i, f in enumerate(files)]
    views = [memoryview(f) for f in files]
    res["kernel_ms_all"] = {}
    for how in ("gpu", "host"):
        runs = []
        for _ in range(max(1, a.repeat_kernels)):
            ev = {}
            P._decode_parsed(ctx, parsed, views, ["RGB"] * a.batch, how, POOL, events=ev)
            torch.cuda.synchronize()
            runs.append({k: v[0].elapsed_time(v[1]) for k, v in ev.items()})
        res["kernel_ms"][how] = runs[0]
        res["kernel_ms_all"][how] = runs                     # "unfilter" spans the un-filter launches and, for interlaced files, the interleave
        print(f"kernels, inflate={how!r}: " + "; ".join(", ".join(f"{k} {ms:.2f} ms" for k, ms in r.items()) for r in runs), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
