"""Decode-side timing: a loop of Jpeg.decompress() against Jpeg.decompress_many(entropy="host" / "gpu") on the same .ajpg files.

    python tools/bench_decode.py [--batch 64] [--height 2160] [--width 3840] [--loop-files 8] [--repeats 3] [--out FILE]

Files: --batch images of synthetic data and of the natural test images mirror-tiled to the size (tools/benchlib/data.py), each written as
both container kinds -- host zlib level 9 (the reference's bytes) and compress_many(entropy="gpu").  Every time is a host clock around
work that ends in a device synchronise, after one warm-up call.  The decompress() loop is timed on --loop-files files and scaled to the
batch (it is per file and serial).  Prints one JSON line (and writes it to --out).  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a separate run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
from benchlib.data import natural_batch, synth_batch  # noqa: E402


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best.append(time.perf_counter() - t0)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--loop-files", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--data", default="synthetic,natural")
    ap.add_argument("--containers", default="host9,gpu")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode.py measures on the GPU"
    dev = torch.device("cuda", 0)
    codec = A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), (4, 64)))
    result = {"batch": a.batch, "H": a.height, "W": a.width, "device": torch.cuda.get_device_name(0), "cases": []}
    for data in a.data.split(","):
        make = natural_batch if data == "natural" else synth_batch
        x = make(torch, a.batch, a.height, a.width, 2024, dev).cpu().numpy()
        for kind in a.containers.split(","):
            files = codec.compress_many(x, extension=".png", **({"entropy": "gpu"} if kind == "gpu" else {}))
            case = {"data": data, "container": kind, "mbytes": round(sum(len(f) for f in files) / 1e6, 2)}
            dec = A.Jpeg(A.JpegCompressionSettings())
            k = min(a.loop_files, a.batch)
            loop, t_loop = timed(lambda: [dec.decompress(f).data for f in files[:k]], 1)
            case["decompress_loop_s_per_file"] = t_loop[0] / k
            case["decompress_loop_s_batch_est"] = t_loop[0] / k * a.batch
            outs = {}
            for entropy in ("host", "gpu"):
                out, t = timed(lambda: dec.decompress_many(files, entropy=entropy), a.repeats)
                case[f"many_{entropy}_s"] = min(t)
                case[f"many_{entropy}_s_all"] = t
                outs[entropy] = out.cpu().numpy()
            case["identical"] = bool(np.array_equal(outs["host"], outs["gpu"])
                                     and all(np.array_equal(outs["gpu"][i], loop[i]) for i in range(k)))
            case["speedup_gpu_vs_loop"] = case["decompress_loop_s_batch_est"] / case["many_gpu_s"]
            case["speedup_gpu_vs_host"] = case["many_host_s"] / case["many_gpu_s"]
            result["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
