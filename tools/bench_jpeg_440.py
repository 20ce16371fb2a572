"""The 4:4:0 routes, timed beside their nearest existing neighbours: 64 x 4K Pillow files (quality 75).

    python tools/bench_jpeg_440.py [--batch 64] [--repeats 3] [--out FILE]

  rot90_422_to_440   standard_jpeg_transform_many(4:2:2 files, "rot90", layout_440=True): the output is 4:4:0
  rot90_420          the same pictures saved as 4:2:0, rotated in the same run (the same kernels: bridge, entropy chain, scatter)
  decode_440_s1/_s4  standard_jpeg_decode_many of the 4:4:0 files above at scale 1 and 4 (the h1v2 branch; k_jd_scaled_h1v2)
  decode_422_s1/_s4  the same of the 4:2:2 sources
The 4:4:0 files' pixels are checked against Pillow's at both scales before timing.  Every time is a host clock around work that ends in
a device synchronise or a read-back, after one warm-up; the median of --repeats.  Prints one JSON line (and writes it to --out)."""
import argparse
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_jfif import H, W, images, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    x = images(a.batch)
    pool = ThreadPoolExecutor(a.threads)

    def save(i, ss):
        buf = io.BytesIO()
        Image.fromarray(x[i]).save(buf, "JPEG", quality=75, subsampling=ss)
        return buf.getvalue()

    def pil_load(f, s):
        im = Image.open(io.BytesIO(f))
        if s != 1:
            im.draft("RGB", (im.size[0] // s, im.size[1] // s))
        return np.asarray(im.convert("RGB"))

    f422 = list(pool.map(lambda i: save(i, "4:2:2"), range(a.batch)))
    f420 = list(pool.map(lambda i: save(i, "4:2:0"), range(a.batch)))
    res = {"batch": a.batch, "H": H, "W": W, "quality": 75, "routes": {}}

    def rot(files, **kw):
        return A.standard_jpeg_transform_many(files, "rot90", **kw)

    f440 = rot(f422, layout_440=True)
    assert Image.open(io.BytesIO(f440[0])).size == (H, W) and tuple(Image.open(io.BytesIO(f440[0])).layer[0])[1:3] == (1, 2)
    for s in (1, 4):
        got = A.standard_jpeg_decode_many(f440, scale=s, layout_440=True)
        want = list(pool.map(lambda f: pil_load(f, s), f440))
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w), s
        del got

    def decode(files, s, **kw):
        out = A.standard_jpeg_decode_many(files, scale=s, **kw)
        torch.cuda.synchronize()
        return out

    routes = (("rot90_422_to_440", lambda: rot(f422, layout_440=True), f422), ("rot90_420", lambda: rot(f420), f420),
              ("decode_440_s1", lambda: decode(f440, 1, layout_440=True), f440), ("decode_422_s1", lambda: decode(f422, 1), f422),
              ("decode_440_s4", lambda: decode(f440, 4, layout_440=True), f440), ("decode_422_s4", lambda: decode(f422, 4), f422))
    for name, fn, files in routes:
        t = timed(fn, a.repeats)
        res["routes"][name] = {"ms": t * 1e3, "source_mb": sum(len(f) for f in files) / 1e6}
        print(f"{name}: {t * 1e3:.1f} ms", flush=True)
    pool.shutdown()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
