"""Boxed JPEG decode timing: 64 files of 3840 x 2160, 4:2:0, quality 90, (1) as Pillow writes them, without restart markers, and (2) the
same files through standard_jpeg_transcode_many(..., restart_marker_rows=1).  Per file set, three ways to a centred region:

    a  standard_jpeg_decode_many(files), then [t:b, l:r].contiguous() of every image -- all there was before box=
    b  standard_jpeg_decode_many(files, box=centred 512 x 512)
    c  standard_jpeg_decode_many(files, box=centred 1024 x 1024)

    python tools/profiling/bench_jpeg_box.py [--batch 64] [--rounds 7] [--out FILE] [--only WAY --set NAME]

Every time is a host clock around the whole call -- header parsing, the copy of the scans, every device stage, the status read-back --
ending in a device synchronise.  The three ways run interleaved, round after round in one process, after one warm-up round; the median
and the minimum over --rounds are reported.  Before timing, b and c are checked against the slices of a.  The workspace sizes are what
aej_jpegdec_workspace_bytes_box answers for the call without boxes and with each box; decode_box_stats gives the segments decoded and
the coefficient blocks stored.  Prints one JSON line (and writes it to --out).

--only a_full_then_slice_512 | b_box_512 | c_box_1024 with --set no_restarts | transcoded_rows_1 runs that one way on that one file set,
unchecked, and nothing else on the device but the transcode that makes the second set: the form to put under
``rocprofv3 --kernel-trace --stats`` for the way's kernel times (a run of its own; its host times are the tracer's, not the library's)."""
import argparse
import ctypes
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
from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc, get_context  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_jfif import H, W, images  # noqa: E402


def centred(size):
    l, t = (W - size) // 2, (H - size) // 2
    return l, t, l + size, t + size


def workspace(files, box):
    ctx = get_context(0)
    descs = (JpegDecDesc * len(files))(*[A.standard_jpeg.parse_header(f) for f in files])
    boxes = None if box is None else np.ascontiguousarray(np.tile(np.array(box, np.int32), (len(files), 1)))
    return int(ctx.lib.aej_jpegdec_workspace_bytes_box(ctx.handle, ctypes.addressof(descs), len(files), None, None,
                                                       None if boxes is None else boxes.ctypes.data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--only", choices=("a_full_then_slice_512", "b_box_512", "c_box_1024"))
    ap.add_argument("--set", choices=("no_restarts", "transcoded_rows_1"))
    a = ap.parse_args()
    if (a.only is None) != (a.set is None):
        ap.error("--only and --set go together")
    x = images(a.batch)

    def save(i):
        buf = io.BytesIO()
        Image.fromarray(x[i]).save(buf, "JPEG", quality=90, subsampling="4:2:0")
        return buf.getvalue()
    with ThreadPoolExecutor(16) as pool:
        plain = list(pool.map(save, range(a.batch)))
    sets = {"no_restarts": plain}
    if a.set != "no_restarts":
        sets["transcoded_rows_1"] = A.standard_jpeg_transcode_many(plain, restart_marker_rows=1)
    if a.set:
        sets = {a.set: sets[a.set]}
    b512, b1024 = centred(512), centred(1024)
    res = {"batch": a.batch, "H": H, "W": W, "quality": 90, "subsampling": "4:2:0", "rounds": a.rounds, "boxes": {"512": b512, "1024": b1024},
           "cases": {}}
    for name, files in sets.items():
        def slice_of(box):
            l, t, r, b = box
            return [im[t:b, l:r].contiguous() for im in A.standard_jpeg_decode_many(files)]
        ways = {"a_full_then_slice_512": lambda: slice_of(b512), "b_box_512": lambda: A.standard_jpeg_decode_many(files, box=b512),
                "c_box_1024": lambda: A.standard_jpeg_decode_many(files, box=b1024)}
        stats = {}
        if a.only:
            ways = {a.only: ways[a.only]}
        else:
            want512, want1024 = slice_of(b512), slice_of(b1024)
            for way, box, want in (("b_box_512", b512, want512), ("c_box_1024", b1024, want1024)):
                got = ways[way]()
                stats[way] = A.decode_box_stats()
                assert all(torch.equal(g, w) for g, w in zip(got, want)), (name, way)
            del want512, want1024, got
        times = {way: [] for way in ways}
        for r in range(a.rounds + 1):                        # round 0: the warm-up
            for way, fn in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r:
                    times[way].append((time.perf_counter() - t0) * 1e3)
        case = {"file_mb": sum(len(f) for f in files) / 1e6,
                "workspace_mb": {"no_box": workspace(files, None) / 1e6, "box_512": workspace(files, b512) / 1e6, "box_1024": workspace(files, b1024) / 1e6}}
        for way, ts in times.items():
            case[way] = {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}
            if way in stats:
                case[way].update(dict(zip(("segments_total", "segments_decoded", "coef_blocks"), stats[way])))
            print(f"{name}: {way}: median {case[way]['median_ms']:.2f} ms, min {case[way]['min_ms']:.2f} ms", flush=True)
        print(f"{name}: workspace {case['workspace_mb']}", flush=True)
        res["cases"][name] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
