"""LPIPS timing: EvaluationMetrics.lpips_batch on 8 x 4K and 64 x 1080p pairs, and MIOpen's float32 conv2d on the same five layers.

    python tools/bench_lpips.py [--repeats 5] [--out FILE] [--stats kernel_stats.csv]

Seeded weights (no pretrained weights ship; the timing does not depend on their values).  Every time is a host clock around work that
ends in a device synchronise, after one warm-up; the median of --repeats is reported.  The yardstick is torch.nn.functional.conv2d
(MIOpen, float32, channels-last input and weights) on each layer's input shape at batch 8 x 4K, with bias and ReLU, timed the same way.
Per-kernel times of the library come from a separate `rocprofv3 --kernel-trace --stats` run of `--workloads 4k`; given its
kernel_stats.csv, `--stats FILE` (no device work) derives achieved TFLOP/s per conv layer (counted FLOPs, 2 per multiply-add; two
trunks per call, --repeats + 1 calls) against the 157.3 TFLOP/s float32 MFMA peak.  Prints one JSON line (and writes it to --out).
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
import lpips_reference as R  # noqa: E402

PEAK_TF = 157.3
# (Cin, Cout, k, stride, pad) and the kernel template each layer runs (k_lpips_conv<KH, KW, S, CK, RW, RAW>)
LAYERS = R.CONVS
KERNELS = ("k_lpips_conv<11, 11, 4, 4, 1, true>", "k_lpips_conv<5, 5, 1, 32, 2, false>", "k_lpips_conv<3, 3, 1, 32, 2, false>")


def shapes(H, W):
    """input (h, w) and output (h, w) of each conv layer"""
    o1 = ((H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1)
    p1 = ((o1[0] - 3) // 2 + 1, (o1[1] - 3) // 2 + 1)
    p2 = ((p1[0] - 3) // 2 + 1, (p1[1] - 3) // 2 + 1)
    return [((H, W), o1), (p1, p1), (p2, p2), (p2, p2), (p2, p2)]


def flops(B, H, W):
    return [2.0 * B * o[0] * o[1] * cout * cin * k * k for (cin, cout, k, _, _), (_, o) in zip(LAYERS, shapes(H, W))]


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


def miopen_layers(B, H, W, sd, repeats):
    out = []
    for l, ((cin, cout, k, s, p), (i, _)) in enumerate(zip(LAYERS, shapes(H, W))):
        x = torch.rand((B, cin, i[0], i[1]), device="cuda").to(memory_format=torch.channels_last)
        w = sd[f"features.{R.FEATURE_INDEX[l]}.weight"].cuda().to(memory_format=torch.channels_last)
        b = sd[f"features.{R.FEATURE_INDEX[l]}.bias"].cuda()
        out.append(timed(lambda: torch.relu(torch.nn.functional.conv2d(x, w, b, stride=s, padding=p)), repeats))
        del x
    return out


def from_stats(path, B, H, W, n_calls):
    """per conv layer: (ms per call, TFLOP/s) from rocprofv3 kernel_stats.csv -- conv3..5 share a kernel and are reported together"""
    rows = list(csv.DictReader(open(path)))
    f = flops(B, H, W)
    res = {}
    for name, layers in zip(KERNELS, ([0], [1], [2, 3, 4])):
        key = name.replace(" ", "")
        hit = [r for r in rows if key in r["Name"].replace(" ", "")]
        if not hit:
            continue
        ms = float(hit[0]["TotalDurationNs"]) / 1e6 / n_calls
        res["+".join(f"conv{l + 1}" for l in layers)] = {"ms": ms, "tflops": sum(f[l] for l in layers) / ms / 1e9}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--stats")
    ap.add_argument("--workloads", default="4k,1080p")
    a = ap.parse_args()
    if a.stats:      # post-processing of a rocprofv3 run of `--workloads 4k` (no device work)
        print(json.dumps(from_stats(a.stats, 8, 2160, 3840, 2 * (a.repeats + 1))))
        return
    sd, lin = R.random_state_dicts(1)
    w = A.LpipsWeights.load(sd, lin)
    g = np.random.default_rng(0)
    res = {"peak_tflops_f32_mfma": PEAK_TF, "repeats": a.repeats}
    for wl, (B, H, W) in (("4k", (8, 2160, 3840)), ("1080p", (64, 1080, 1920))):
        if wl not in a.workloads.split(","):
            continue
        x = torch.from_numpy(g.random((B, H, W, 3), dtype=np.float32)).cuda()
        y = (x + 0.02 * torch.randn_like(x)).clamp(0, 1)
        t = timed(lambda: A.EvaluationMetrics.lpips_batch(x, y, w), a.repeats)
        f = flops(B, H, W)
        r = {"batch": B, "H": H, "W": W, "lpips_batch_s": t, "ms_per_pair": 1e3 * t / B, "conv_gflop_per_image": [v / B / 1e9 for v in f],
             "tflops_whole_call": 2 * sum(f) / t / 1e12}
        if wl == "4k":
            m = miopen_layers(B, H, W, sd, a.repeats)
            r["miopen_conv_ms"] = [1e3 * v for v in m]
            r["miopen_tflops"] = [fl / v / 1e12 for fl, v in zip(f, m)]
        res[wl] = r
        del x, y
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
