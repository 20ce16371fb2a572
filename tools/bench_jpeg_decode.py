"""Baseline-JPEG decode timing: 64 x 4K Pillow files (quality 75, 4:2:0) through csrc/jpegdec.hip, written (a) without restart
markers -- Pillow's default, decoded by the self-synchronising subsequences -- and (b) with restart_marker_rows=1, against Pillow
decoding them on a thread pool and uploading its pixels.

    python tools/bench_jpeg_decode.py [--batch 64] [--repeats 3] [--threads 16] [--subseq-bits N] [--progressive] [--scale S]
                                      [--mode RGB|L] [--transcoded] [--no-pillow] [--out FILE]

--progressive writes the same files with progressive=True and decodes them with standard_jpeg_decode_many(..., progressive=True)
(csrc/jpegprog.hip: one thread per restart segment and dependency level, so the files without restart markers are a serial decode
per scan and the restart-per-row files show what the kernels do when the format allows parallelism).

--scale 2 / 4 / 8 decodes at that fraction of the size on both sides: standard_jpeg_decode_many(..., scale=S) (csrc/jpegdec.hip
k_jd_scaled) against Pillow after im.draft("RGB", (W // S, H // S)); the gigapixels per second still count the files' full-size pixels.

--mode L decodes to the luma plane alone on both sides: standard_jpeg_decode_many(..., mode="L") (csrc/jpegdec.hip k_jd_luma), uint8
[h, w] tensors, against Pillow after im.draft("L", (W // S, H // S)) -- not convert("L").

--transcoded adds a third case: the files without restart markers put through standard_jpeg_transcode_many(...,
restart_marker_rows=1) (progressive output with --progressive) -- the lossless way to make an archive cheap to decode -- with the time
of that transcode; --no-pillow leaves the CPU side's timing out.

"gpu" is standard_jpeg_decode_many: host header parsing, one copy of the scans, every device stage, the per-file status read-back;
it ends with device uint8 [H, W, 3] tensors.  "pillow" is np.asarray(Image.open(buf).convert("RGB")) per file on --threads threads, then
one stacked host-to-device copy of the pixels.  Every time is a host clock around work that ends in a device synchronise, after one
warm-up; the median of --repeats is reported, as gigapixels per second.  The GPU's pixels are checked against Pillow's for every file
before timing.  Prints one JSON line (and writes it to --out) with the sync rounds of each case.
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

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_jfif import H, W, images, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--subseq-bits", type=int, default=0, help="jpegdec_subseq_bits (0: the library's default)")
    ap.add_argument("--progressive", action="store_true", help="progressive files through csrc/jpegprog.hip")
    ap.add_argument("--scale", type=int, default=1, choices=(1, 2, 4, 8), help="decode at 1 / scale of the size (Pillow: Image.draft)")
    ap.add_argument("--mode", default="RGB", choices=("RGB", "L"), help="L: the luma plane alone (Pillow: Image.draft('L', ...))")
    ap.add_argument("--transcoded", action="store_true", help="also: the no-restart files transcoded with restart_marker_rows=1")
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    x = images(a.batch)
    ctx = A._lib.get_context(0)
    if a.subseq_bits:
        ctx.set_option("jpegdec_subseq_bits", a.subseq_bits)
    gp = a.batch * H * W / 1e9
    res = {"batch": a.batch, "H": H, "W": W, "quality": 75, "subseq_bits": ctx.get_option("jpegdec_subseq_bits"),
           "pillow_threads": a.threads, "progressive": a.progressive, "cases": {}}
    if a.scale != 1:
        res["scale"] = a.scale
    if a.mode != "RGB":
        res["mode"] = a.mode
    pool = ThreadPoolExecutor(a.threads)

    def save(i, opts):
        buf = io.BytesIO()
        Image.fromarray(x[i]).save(buf, "JPEG", quality=75, **opts)
        return buf.getvalue()

    def pil_load(f):
        im = Image.open(io.BytesIO(f))
        if a.scale != 1 or a.mode == "L":
            im.draft(a.mode, (W // a.scale, H // a.scale))
        return np.asarray(im if a.mode == "L" else im.convert("RGB"))

    def decode(files):
        how = dict(scale=a.scale) if a.scale != 1 else {}
        if a.mode != "RGB":
            how["mode"] = a.mode
        return A.standard_jpeg_decode_many(files, progressive=True, **how) if a.progressive else A.standard_jpeg_decode_many(files, **how)

    plain, extra = None, {}
    for name, opts in (("no_restarts", {}), ("restart_rows_1", {"restart_marker_rows": 1})) + ((("transcoded_rows_1", None),) if a.transcoded else ()):
        if opts is None:                                 # the lossless route: the first case's files, transcoded
            again = lambda: A.standard_jpeg_transcode_many(plain, progressive=a.progressive, restart_marker_rows=1)  # noqa: E731
            files = again()
            extra = {"transcode_ms": timed(again, a.repeats) * 1e3}
        else:
            if a.progressive:
                opts = dict(opts, progressive=True)
            files = list(pool.map(lambda i: save(i, opts), range(a.batch)))
            plain = plain or files
        got = decode(files)
        rounds = S.decode_sync_rounds()
        for f, g in zip(files, got):
            assert np.array_equal(g.cpu().numpy(), pil_load(f)), name
        del got
        tg = timed(lambda: decode(files), a.repeats)

        def pillow():
            px = np.stack(list(pool.map(pil_load, files)))
            return torch.from_numpy(px).to("cuda:0")
        mb = sum(len(f) for f in files) / 1e6
        res["cases"][name] = {"file_mb": mb, "sync_rounds": rounds, "gpu_ms": tg * 1e3, "gpu_gps": gp / tg, **extra}
        print(f"{name}: {mb:.1f} MB of files, {rounds} sync rounds; GPU {tg * 1e3:.1f} ms ({gp / tg:.2f} GP/s)", flush=True)
        if a.no_pillow:
            continue
        tp = timed(pillow, a.repeats)
        res["cases"][name].update({"pillow_upload_ms": tp * 1e3, "pillow_upload_gps": gp / tp, "speedup": tp / tg})
        print(f"{name}: Pillow on {a.threads} threads + upload {tp * 1e3:.1f} ms ({gp / tp:.2f} GP/s): x{tp / tg:.2f}", flush=True)
    pool.shutdown()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
