"""JPEG thumbnail timing: 64 x 4K Pillow files (quality 75, 4:2:0) to thumbnails of (256, 256) and (1024, 1024), bicubic, three ways:

    python tools/bench_jpeg_thumbnail.py [--batch 64] [--repeats 3] [--threads 16] [--mode RGB|L] [--out FILE]

"gpu" is standard_jpeg_thumbnail_many: header parsing and the plan on the host, the scaled decode, then csrc/resample.hip on the
decoder's output; it ends with device uint8 [h, w, 3] tensors and reads nothing back but the decoder's status words.
"decode_host_resize" is the route without it: standard_jpeg_decode_many(scale=s) with thumbnail_plan's scale, a copy of the pixels to
the host, Pillow's Image.resize with the box and reducing_gap on --threads threads, one upload of the results.
"pillow" is Image.open(buf).thumbnail(size) per file on --threads threads, then one upload of the results.
--mode L: every route in one channel -- standard_jpeg_thumbnail_many(..., mode="L") and standard_jpeg_decode_many(..., mode="L") end with
uint8 [h, w] tensors, and Pillow is the thumbnail of the file's one draft("L", ...) call (pil_thumbnail below), not convert("L").
Every time is a host clock around work that ends in a device synchronise, after one warm-up; the median of --repeats is reported.  The
GPU's pixels are checked against Pillow's for every file before timing.  Prints one JSON line (and writes it to --out).

Per-kernel times and the launch count, in a run of their own (no counters in it):

    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -- python tools/bench_jpeg_thumbnail.py --trace-calls 4
    python tools/bench_jpeg_thumbnail.py --trace-summary DIR [--out FILE]

--trace-calls N runs, per size, N thumbnail calls and then N calls of the scaled decode alone (standard_jpeg_decode_many at the plan's
scale), each call between two synchronised marker kernels (a fill of MARKER_BYTES bytes) so that the summary can cut the trace into
calls; --trace-summary reads the trace (no device work): per call the dispatches and the device time of every kernel, the copies by
direction, and what a thumbnail call adds to a decode call.
"""
import argparse
import csv
import glob
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

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_jfif import H, W, images  # noqa: E402

BICUBIC = 3
SIZES = ((256, 256), (1024, 1024))
MARKER_BYTES = 7717          # the marker's grid is like no other launch's of the run


def save_files(x, pool):
    def save(i):
        buf = io.BytesIO()
        Image.fromarray(x[i]).save(buf, "JPEG", quality=75)
        return buf.getvalue()

    return list(pool.map(save, range(len(x))))


def pil_thumbnail(f, size, mode, gap=2.0):
    """Pillow's thumbnail of one file.  mode "L": the one it makes when the file's one draft() call asks for mode "L" (thumbnail()'s own
    draft does nothing after a first one): the draft at thumbnail()'s requested size, then thumbnail()'s resize over the box it returns"""
    im = Image.open(io.BytesIO(f))
    if mode != "L":
        im.thumbnail(size, BICUBIC, reducing_gap=gap)
        return np.asarray(im.convert("RGB"))
    plan = A.thumbnail_plan(im.size[0], im.size[1], size, gap)
    res = im.draft("L", (int(size[0] * gap), int(size[1] * gap)) if plan is not None else None)
    if plan is not None and im.size != tuple(plan[2]):
        im = im.resize(tuple(plan[2]), BICUBIC, box=res[1], reducing_gap=gap)
    return np.asarray(im)


def trace_calls(a):
    """the calls of the kernel-trace run: the first of each kind also warms the workspace up and is left out of the summary"""
    pool = ThreadPoolExecutor(a.threads)
    files = save_files(images(a.batch), pool)
    pool.shutdown()
    marker = torch.empty(MARKER_BYTES, dtype=torch.uint8, device="cuda:0")

    def mark():
        marker.fill_(1)
        torch.cuda.synchronize()

    for size in SIZES:
        scale = A.thumbnail_plan(W, H, size)[0]
        for fn in (lambda: A.standard_jpeg_thumbnail_many(files, size, **a.how), lambda: A.standard_jpeg_decode_many(files, scale=scale, **a.how)):
            for _ in range(a.trace_calls):
                mark()
                out = fn()
                torch.cuda.synchronize()
                del out
    mark()
    print(json.dumps({"batch": a.batch, "calls_per_kind": a.trace_calls, "sizes": [list(s) for s in SIZES], "mode": a.mode}))


def short(name):
    return name.split("(")[0].replace("void ", "").replace("aej::", "")


def trace_summary(a):
    """cut the trace at the marker kernels; calls come as, per size, n thumbnail calls then n decode calls"""
    f = glob.glob(os.path.join(a.trace_summary, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"]))
                  for r in csv.DictReader(open(f)))
    fills = [r for r in rows if "aej::" not in r[2] and "fill" in r[2].lower()]
    grids = sorted({r[3] for r in fills}, key=lambda g: sum(1 for r in fills if r[3] == g))
    n = a.trace_calls
    want = 2 * n * len(SIZES) + 1
    marks = next(([r for r in fills if r[3] == g] for g in grids if sum(1 for r in fills if r[3] == g) == want), None)
    assert marks is not None, f"no fill kernel with {want} launches of one grid: the markers of --trace-calls {n}"
    cf = glob.glob(os.path.join(a.trace_summary, "**", "*memory_copy_trace.csv"), recursive=True)
    copies = sorted((int(r["Start_Timestamp"]), r.get("Direction") or r["Kind"]) for r in csv.DictReader(open(cf[0]))) if cf else None
    lines = [f"# rocprofv3 --kernel-trace --memory-copy-trace --stats (no counters) of tools/bench_jpeg_thumbnail.py --trace-calls {n}: {a.batch} x {W}x{H} Pillow",
             "# files (quality 75, 4:2:0), bicubic, reducing_gap 2.0, MI355X.  Per size: thumbnail calls (standard_jpeg_thumbnail_many) and calls of",
             "# the scaled decode alone (standard_jpeg_decode_many at the plan's scale); the first call of each kind is left out.  Per kernel: its",
             "# dispatches in one call (the same in every call unless a range is shown) and the median over the calls of its device time summed",
             "# over the call.  copies: the memory copies of one call by direction.", ""]
    worst = 0
    for si, size in enumerate(SIZES):
        plan = A.thumbnail_plan(W, H, size)
        lines.append(f"thumbnail to {size}: draft scale {plan[0]}, reduce factors {plan[1]}, final size {plan[2]}")
        per_kind = []
        for kind in range(2):
            base = (si * 2 + kind) * n
            calls = []
            for c in range(base + 1, base + n):      # not the first
                lo, hi = marks[c][1], marks[c + 1][0]
                ks = [r for r in rows if lo <= r[0] < hi and "aej::" in r[2]]
                cp = [d for t, d in copies if lo <= t < hi] if copies is not None else None
                calls.append((ks, cp))
            names = []
            for ks, _ in calls:
                for r in ks:
                    if short(r[2]) not in names:
                        names.append(short(r[2]))
            lines.append(f"  {('standard_jpeg_thumbnail_many', f'standard_jpeg_decode_many(scale={plan[0]})')[kind]}: {len(calls)} calls")
            tot, count = 0.0, {}
            for nm in names:
                disp = [sum(1 for r in ks if short(r[2]) == nm) for ks, _ in calls]
                ms = float(np.median([sum(r[1] - r[0] for r in ks if short(r[2]) == nm) for ks, _ in calls])) / 1e6
                tot += ms
                count[nm] = max(disp)
                lines.append(f"    {nm:18s} dispatches {disp[0] if min(disp) == max(disp) else f'{min(disp)}-{max(disp)}':>5}  median {ms:8.3f} ms")
            span = float(np.median([ks[-1][1] - ks[0][0] for ks, _ in calls])) / 1e6
            lines.append(f"    sum of medians {tot:.2f} ms; first launch start to last launch end: median {span:.2f} ms")
            dirs = None
            if copies is not None:
                dirs = {d: [sum(1 for x in cp if x == d) for _, cp in calls] for d in sorted({x for _, cp in calls for x in cp})}
                lines.append("    copies: " + ", ".join(f"{d} {v[0] if min(v) == max(v) else f'{min(v)}-{max(v)}'}" for d, v in dirs.items()))
            per_kind.append((count, dirs))
        (kt, ct), (kd, cd) = per_kind
        extra = {k: v - kd.get(k, 0) for k, v in kt.items() if v - kd.get(k, 0)}
        worst = max(worst, sum(extra.values()))
        lines.append(f"  a thumbnail call adds to the decode call: launches {extra} = {sum(extra.values())}"
                     + ("" if ct is None else "; copies " + str({d: max(ct.get(d, [0])) - max(cd.get(d, [0])) for d in sorted(set(ct) | set(cd))})))
        lines.append("")
    lines.append(f"launches a thumbnail call adds beyond the decode's own, at most: {worst}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as o:
            o.write(text)


def times(fn, repeats):
    """one warm-up, then the host clock around `repeats` calls, each ended by a device synchronise: -> the list, in seconds"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--mode", default="RGB", choices=("RGB", "L"), help="L: one-channel thumbnails of the luma plane (Pillow: Image.draft('L', ...))")
    ap.add_argument("--out")
    ap.add_argument("--trace-calls", type=int, default=0, help="the run to put under rocprofv3: this many calls of each kind per size")
    ap.add_argument("--trace-summary", help="the directory rocprofv3 wrote such a run's trace to (with --trace-calls as in that run)")
    a = ap.parse_args()
    a.how = {} if a.mode == "RGB" else {"mode": a.mode}      # RGB: the calls without the keyword
    if a.trace_summary:
        a.trace_calls = a.trace_calls or 4
        return trace_summary(a)
    if a.trace_calls:
        assert a.trace_calls >= 2, "the first call of each kind is left out"
        return trace_calls(a)
    pool = ThreadPoolExecutor(a.threads)
    files = save_files(images(a.batch), pool)
    res = {"batch": a.batch, "H": H, "W": W, "quality": 75, "filter": "bicubic", "reducing_gap": 2.0, "pillow_threads": a.threads,
           "file_mb": sum(len(f) for f in files) / 1e6, "mode": a.mode, "cases": {}}
    for size in SIZES:
        plan = A.thumbnail_plan(W, H, size)
        scale, factors, final, box = plan

        def pil_thumb(f):
            return pil_thumbnail(f, size, a.mode)

        def gpu():
            return A.standard_jpeg_thumbnail_many(files, size, **a.how)

        def pillow():
            return torch.from_numpy(np.stack(list(pool.map(pil_thumb, files)))).to("cuda:0")

        def decode_host_resize():
            dec = A.standard_jpeg_decode_many(files, scale=scale, **a.how)
            host = [d.cpu().numpy() for d in dec]
            out = pool.map(lambda p: np.asarray(Image.fromarray(p).resize(final, BICUBIC, box=box, reducing_gap=2.0)), host)
            return torch.from_numpy(np.stack(list(out))).to("cuda:0")

        got = gpu()
        want = list(pool.map(pil_thumb, files))
        for g, w_ in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w_), size
        assert np.array_equal(decode_host_resize().cpu().numpy(), np.stack(want))
        del got
        runs = {"gpu": [], "decode_host_resize": [], "pillow_upload": []}
        for name, fn in (("gpu", gpu), ("decode_host_resize", decode_host_resize), ("pillow_upload", pillow)):
            runs[name] = [t * 1e3 for t in times(fn, a.repeats)]
        tg, th, tp = (float(np.median(runs[k])) / 1e3 for k in ("gpu", "decode_host_resize", "pillow_upload"))
        res["cases"][f"{size[0]}x{size[1]}"] = {"draft_scale": scale, "reduce_factors": list(factors), "final_size": list(final), "gpu_ms": tg * 1e3,
                                                "decode_host_resize_ms": th * 1e3, "pillow_upload_ms": tp * 1e3,
                                                "vs_decode_host_resize": th / tg, "vs_pillow": tp / tg, "repeats_ms": runs}
        print(f"{size}: scale {scale}, factors {factors}, final {final}; GPU {tg * 1e3:.1f} ms, scaled decode + host resize {th * 1e3:.1f} ms "
              f"(x{th / tg:.2f}), Pillow on {a.threads} threads + upload {tp * 1e3:.1f} ms (x{tp / tg:.2f})", flush=True)
    pool.shutdown()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
