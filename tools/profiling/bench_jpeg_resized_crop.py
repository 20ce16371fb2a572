"""Resized-crop timing: 64 files of 3840 x 2160, quality 90, in 4:2:0 and 4:2:2, each (1) baseline as Pillow writes it, (2) the same
through standard_jpeg_transcode_many(..., restart_marker_rows=1) and (3) progressive.  One seeded box per file -- 8 to 100 % of the
area, aspect ratio 3/4 to 4/3, as RandomResizedCrop draws them -- resized to 224 x 224, bilinear, with reducing_gap None and 2.0.
Per file set and gap, three ways to the [64, 224, 224, 3] batch:

    a_resized_crop        standard_jpeg_resized_crop_many(files, boxes, (224, 224), "bilinear", reducing_gap=g)
    b_scaled_then_resize  standard_jpeg_decode_many(files, scale=s_i), then resize_many(box=box_i / s_i, reducing_gap=g): the whole
                          scaled image is reconstructed, written and read back (s_i: resized_crop_plan's, 1 without a gap)
    c_box_then_resize     standard_jpeg_decode_many(files, box=box_i) at full size, then resize_many(reducing_gap=g)

    python tools/profiling/bench_jpeg_resized_crop.py [--batch 64] [--rounds 7] [--prog-rounds N] [--out FILE] [--only WAY --set NAME --gap G]

b and c are what there was before the call.  Every time is a host clock around the whole route -- header parsing, the copy of the
scans, every device stage, the status read-back -- ending in a device synchronise.  The ways run interleaved, round after round in one
process, after one warm-up round; the median, the minimum and the maximum over --rounds are reported (the spread is max - min;
--prog-rounds, default --rounds, for the progressive sets, whose calls take seconds).  Before
timing, a is checked against b (they are equal by definition; c filters across the box's edge differently and is not).  Prints one
JSON line (and writes it to --out).

--only WAY with --set NAME and --gap G (0: None) runs that one way on that one file set, unchecked: the form to put under
``rocprofv3 --kernel-trace --stats`` for the way's kernel times (a run of its own; its host times are the tracer's)."""
import argparse
import io
import json
import math
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
from bench_jfif import H, W, images  # noqa: E402

SIZE = (224, 224)
WAYS = ("a_resized_crop", "b_scaled_then_resize", "c_box_then_resize")
SETS = tuple(f"{ss}_{kind}" for ss in ("420", "422") for kind in ("baseline", "rows_1", "progressive"))


def random_boxes(n, seed=20261019):
    """RandomResizedCrop's draw: area 8 .. 100 % of the image, log-uniform aspect ratio 3/4 .. 4/3, integer corners"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        area = W * H * rng.uniform(0.08, 1.0)
        ar = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
        if 0 < w <= W and 0 < h <= H:
            l, t = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
            out.append((l, t, l + w, t + h))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--prog-rounds", type=int)
    ap.add_argument("--out")
    ap.add_argument("--only", choices=WAYS)
    ap.add_argument("--set", choices=SETS)
    ap.add_argument("--gap", type=float)
    a = ap.parse_args()
    if (a.only is None) != (a.set is None) or (a.only is None) != (a.gap is None):
        ap.error("--only, --set and --gap go together")
    x = images(a.batch)
    boxes = random_boxes(a.batch)

    def save(job):
        i, ss, prog = job
        buf = io.BytesIO()
        Image.fromarray(x[i]).save(buf, "JPEG", quality=90, subsampling=ss, progressive=prog)
        return buf.getvalue()

    sets = {}
    with ThreadPoolExecutor(16) as pool:
        for ss, sub in (("420", "4:2:0"), ("422", "4:2:2")):
            if a.set and not a.set.startswith(ss):
                continue
            if a.set in (None, f"{ss}_baseline", f"{ss}_rows_1"):
                plain = list(pool.map(save, [(i, sub, False) for i in range(a.batch)]))
                if a.set != f"{ss}_rows_1":
                    sets[f"{ss}_baseline"] = plain
                if a.set != f"{ss}_baseline":
                    sets[f"{ss}_rows_1"] = A.standard_jpeg_transcode_many(plain, restart_marker_rows=1)
            if a.set in (None, f"{ss}_progressive"):
                sets[f"{ss}_progressive"] = list(pool.map(save, [(i, sub, True) for i in range(a.batch)]))
    gaps = [None, 2.0] if a.gap is None else [a.gap or None]
    res = {"batch": a.batch, "H": H, "W": W, "quality": 90, "size": SIZE, "filter": "bilinear", "rounds": a.rounds,
           "box_area_fraction": [float(np.min([(b[2] - b[0]) * (b[3] - b[1]) for b in boxes]) / (W * H)),
                                 float(np.mean([(b[2] - b[0]) * (b[3] - b[1]) for b in boxes]) / (W * H))], "cases": {}}
    for name, files in sets.items():
        for gap in gaps:
            plans = [A.resized_crop_plan(W, H, b, SIZE, "bilinear", gap) for b in boxes]
            scales = [p["scale"] for p in plans]

            def way_a():
                return A.standard_jpeg_resized_crop_many(files, boxes, SIZE, "bilinear", reducing_gap=gap, progressive=True)

            def way_b():
                ims = A.standard_jpeg_decode_many(files, scale=scales, progressive=True)
                return A.resize_many(ims, SIZE, "bilinear", box=[p["box"] for p in plans], reducing_gap=gap)

            def way_c():
                ims = A.standard_jpeg_decode_many(files, box=boxes, progressive=True)
                return A.resize_many(ims, SIZE, "bilinear", reducing_gap=gap)

            ways = dict(zip(WAYS, (way_a, way_b, way_c)))
            if a.only:
                ways = {a.only: ways[a.only]}
            else:
                got, want = way_a(), way_b()
                assert all(torch.equal(g, w) for g, w in zip(got, want)), (name, gap)
                del got, want
            times = {way: [] for way in ways}
            rounds = a.prog_rounds if a.prog_rounds and name.endswith("progressive") else a.rounds
            for r in range(rounds + 1):                    # round 0: the warm-up
                for way, fn in ways.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r:
                        times[way].append((time.perf_counter() - t0) * 1e3)
            px = [(p["window"][2] - p["window"][0]) * (p["window"][3] - p["window"][1]) for p in plans]
            case = {"file_mb": sum(len(f) for f in files) / 1e6, "scales": {str(s): scales.count(s) for s in sorted(set(scales))},
                    "rounds": rounds, "window_megapixels": sum(px) / 1e6,
                    "scaled_image_megapixels": sum(-(-W // s) * -(-H // s) for s in scales) / 1e6}
            for way, ts in times.items():
                case[way] = {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}
                print(f"{name} gap {gap}: {way}: median {case[way]['median_ms']:.2f} ms, min {case[way]['min_ms']:.2f}, max {case[way]['max_ms']:.2f}", flush=True)
            res["cases"][f"{name}/gap_{gap}"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
