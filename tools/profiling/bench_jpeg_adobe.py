"""Four-component JPEG decode timing: 64 files of 1920 x 1080, quality 90, component 0 sampled 2 x 2, baseline, as Pillow writes them
(K sub-sampled with the chroma: 7 blocks per MCU), beside the three-component 4:2:0 files of the same pictures (6 blocks per MCU) and a
Pillow host loop over the four-component files.

    python tools/profiling/bench_jpeg_adobe.py [--batch 64] [--out FILE]

    cmyk_rgb     standard_jpeg_decode_many(cmyk_files, adobe=True)                   -> [H, W, 3] each
    cmyk_auto    standard_jpeg_decode_many(cmyk_files, adobe=True, mode="auto")      -> [H, W, 4] each
    ycbcr_rgb    standard_jpeg_decode_many(ycbcr_files)                              -> [H, W, 3] each
    pillow_cmyk  [np.asarray(Image.open(f).convert("RGB")) for f in cmyk_files]      on the host, one thread

Every time is a host clock around the whole call -- header parsing, the copy of the scans, every device stage, the status read-back --
ending in a device synchronise; the best of 2 after one warm-up call, as tools/bench_decode.py takes it.  The two device results are
checked against Pillow on the first 4 files before timing.

A second set times files with DISTINCT Huffman tables per component, which take the ordinary synchronising route (the files above have
one table pair for all components, JdFile::uniform).  Pillow cannot write the Photoshop layout (K at full resolution, 10 blocks per MCU),
so the test suite's pure-Python writer makes ONE file of 1024 x 1024 from random quantised blocks (tests/jpeg_adobe_reference.py:
component 0 under the Annex K luminance tables, the others under the chrominance ones) and the call decodes --writer-copies of it; the
same blocks without K, as a three-component 2 x 2 file of 6 blocks per MCU, stand beside it:

    k10_rgb      standard_jpeg_decode_many([ten_block_file] * copies, adobe=True)
    k10_auto     the same with mode="auto"
    ycc6_rgb     standard_jpeg_decode_many([six_block_file] * copies)
    pillow_k10   the Pillow loop over the ten-block files

with the sync rounds of each device call.  Prints one JSON line (and writes it to --out)."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_jfif import images  # noqa: E402
import jpeg_adobe_reference as R  # noqa: E402

H, W = 1080, 1920


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--writer-copies", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    x = images(a.batch)
    rgb = np.ascontiguousarray(x[:, :H, :W])
    k = np.ascontiguousarray(x[:, H:2 * H, W:2 * W, 1:2])      # the K channel: another part of the same frame
    cmyk = np.concatenate([rgb, k], -1)
    del x

    def save(job):
        arr, mode = job
        buf = io.BytesIO()
        Image.fromarray(arr, mode).save(buf, "JPEG", quality=90, subsampling=2)
        return buf.getvalue()
    with ThreadPoolExecutor(16) as pool:
        cmyk_files = list(pool.map(save, [(c, "CMYK") for c in cmyk]))
        ycc_files = list(pool.map(save, [(c, "RGB") for c in rgb]))
    ways = {"cmyk_rgb": lambda: A.standard_jpeg_decode_many(cmyk_files, adobe=True),
            "cmyk_auto": lambda: A.standard_jpeg_decode_many(cmyk_files, adobe=True, mode="auto"),
            "ycbcr_rgb": lambda: A.standard_jpeg_decode_many(ycc_files),
            "pillow_cmyk": lambda: [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in cmyk_files]}
    for i in range(min(4, a.batch)):
        im = Image.open(io.BytesIO(cmyk_files[i]))
        assert np.array_equal(A.standard_jpeg_decode_many(cmyk_files[i:i + 1], adobe=True, mode="auto")[0].cpu().numpy(), np.asarray(im))
        assert np.array_equal(A.standard_jpeg_decode_many(cmyk_files[i:i + 1], adobe=True)[0].cpu().numpy(), np.asarray(im.convert("RGB")))
    res = {"batch": a.batch, "H": H, "W": W, "quality": 90, "layout": "2x2, K 1x1 (7 blocks per MCU) / 4:2:0 (6 blocks per MCU)",
           "file_mb": {"cmyk": sum(map(len, cmyk_files)) / 1e6, "ycbcr": sum(map(len, ycc_files)) / 1e6}, "best_of": 2, "ms": {}}
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
    res["cmyk_over_ycbcr"] = res["ms"]["cmyk_rgb"]["best"] / res["ms"]["ycbcr_rgb"]["best"]
    # distinct tables per component: the writer's ten-block file and the same blocks without K
    S = 1024
    rng = np.random.default_rng(4)
    comps = [(2, 2, R.random_blocks(rng, S // 8, S // 8)), (1, 1, R.random_blocks(rng, S // 16, S // 16)), (1, 1, R.random_blocks(rng, S // 16, S // 16)),
             (2, 2, R.random_blocks(rng, S // 8, S // 8))]
    k10, ycc6 = R.write_baseline(S, S, comps, transform=0), R.write_baseline(S, S, comps[:3])
    im = Image.open(io.BytesIO(k10))
    assert np.array_equal(A.standard_jpeg_decode_many([k10], adobe=True, mode="auto")[0].cpu().numpy(), np.asarray(im))
    assert np.array_equal(A.standard_jpeg_decode_many([ycc6])[0].cpu().numpy(), np.asarray(Image.open(io.BytesIO(ycc6)).convert("RGB")))
    n = a.writer_copies
    ways = {"k10_rgb": lambda: A.standard_jpeg_decode_many([k10] * n, adobe=True),
            "k10_auto": lambda: A.standard_jpeg_decode_many([k10] * n, adobe=True, mode="auto"),
            "ycc6_rgb": lambda: A.standard_jpeg_decode_many([ycc6] * n),
            "pillow_k10": lambda: [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in [k10] * n]}
    res["writer"] = {"copies": n, "H": S, "W": S, "file_bytes": {"k10": len(k10), "ycc6": len(ycc6)}, "ms": {}, "sync_rounds": {}}
    for way, fn in ways.items():
        ts = []
        for r in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
        res["writer"]["ms"][way] = {"best": min(ts), "both": ts}
        if not way.startswith("pillow"):
            res["writer"]["sync_rounds"][way] = A.standard_jpeg.decode_sync_rounds()
        print(f"{way}: {min(ts):.2f} ms (best of 2: {ts[0]:.2f}, {ts[1]:.2f})", flush=True)
    res["writer"]["k10_over_ycc6"] = res["writer"]["ms"]["k10_rgb"]["best"] / res["writer"]["ms"]["ycc6_rgb"]["best"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
