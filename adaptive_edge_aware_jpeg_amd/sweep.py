"""``sweep`` -- the reference's rate-distortion study (test/analysis/metrics_computation.py) as one batched GPU schedule.

The reference runs every image through ``itertools.product(color_spaces, quality_ranges, block_size_ranges)`` and, per cell,
``compress`` -> ``decompress`` -> PSNR / SSIM / MS-SSIM -> ``compression_ratio = H * W * 3 / len(ajpg)``.  The encode is separable:
colour, Canny, quadtree and DCT depend on the colour space and the block-size range only; the quality range enters through the
quantisation matrices alone (jpeg.py:356-404, 485-506, 688-705).  So per colour space x block range x image sub-batch this module

1. binds the settings once (the path ``Jpeg._bind`` takes),
2. runs one encode that keeps the pre-quantisation DCT values,
3. requantises them for a group of quality ranges in one ``aej_requantise_batch`` call (csrc/requant.hip),
4. per quality range: ``aej_decode_batch_tables`` -> ``aej_metrics_batch``, plus the container size.

With ``lpips=`` (an ``LpipsWeights``) the originals' LPIPS features are computed once per image sub-batch (``aej_lpips_features``)
and every decoded quality set is scored against them (``aej_lpips_batch``): the ``lpips`` column of the reference's CSV.

Sizes: ``"zlib"`` (the default, the reference's number) is host zlib level 9 of every layer on a thread pool, fed by one device-to-host
copy per quality set and overlapped with the GPU work of the next sets.  ``"gpu"`` takes the lengths of the GPU deflate's streams
(``Jpeg.deflate_batch``) without copying them back: about 10 % larger than zlib-9, so NOT the reference's compression ratio, and -- the GPU
deflate counts one Huffman code per layer over a whole call -- dependent on which images share a sub-batch (``SweepResult.sub_batches``).
``None`` skips sizes.

With ``standard_qualities=`` (e.g. ``(10, 25, 50, 75, 90)``, the qualities of metrics_comparison.py) the same images also go through
standard JPEG (standard_jpeg.py: Pillow's files, byte for byte, and Pillow's decode of them), scored with the same metrics against the
same originals: ``SweepResult.standard`` and ``SweepResult.to_csv_standard``.
"""
import csv
import ctypes
import itertools
import json
import math
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import tables
from ._lib import AejError, get_context
from .evaluation_metrics import MS_SSIM, PSNR, SSIM
from . import lpips as _lpips
from . import standard_jpeg as _std
from .jpeg import Jpeg, usable_cpus
from .settings import JpegCompressionSettings

CSV_COLUMNS = ("image_name", "color_space", "min_quality", "max_quality", "min_block_size", "max_block_size", "psnr", "ssim", "ms_ssim",
               "compression_ratio")      # metrics_computation.py:185-197 without 'lpips' (its weights are a download)
CSV_COLUMNS_LPIPS = CSV_COLUMNS[:9] + ("lpips",) + CSV_COLUMNS[9:]      # the reference's full header: sweep(..., lpips=weights)
STANDARD_COLUMNS = ("image_name", "quality", "psnr", "ssim", "ms_ssim", "compression_ratio")      # keys of metrics_comparison.py:26-32
STANDARD_COLUMNS_LPIPS = STANDARD_COLUMNS[:5] + ("lpips",) + STANDARD_COLUMNS[5:]
DEFAULT_MEMORY_FRACTION = 0.5            # max_bytes=None: this share of the device memory free when the sweep starts


def reference_grid():
    """-> (color_spaces, quality_ranges, block_size_ranges) of the reference study (metrics_computation.py:296-316): YCbCr, the 15
    ranges min <= max over (10, 25, 50, 75, 90), the 21 ranges min <= max over (4, 8, ..., 128), in its order."""
    qv, bv = (10, 25, 50, 75, 90), (4, 8, 16, 32, 64, 128)
    return (("YCbCr",), [(a, b) for a in qv for b in qv if a <= b], [(a, b) for a in bv for b in bv if a <= b])


def container_length(H, W, color_space, quality_range, block_size_range, extension, n_states, stream_lengths) -> int:
    """Bytes of the .ajpg container Jpeg.compress writes (jpeg.py:531-597): 4 + JSON header + per layer 12 + packed 2-bit states +
    zlib stream.  n_states / stream_lengths: per layer."""
    meta = {"height": int(H), "width": int(W), "num_layers": len(n_states), "color_space": color_space,
            "quality_min": quality_range[0], "quality_max": quality_range[1],
            "block_size_min": block_size_range[0], "block_size_max": block_size_range[1], "extension": extension}
    n = 4 + len(json.dumps(meta).encode("utf-8"))
    for ns, sl in zip(n_states, stream_lengths):
        n += 12 + (int(ns) + 3) // 4 + int(sl)
    return n


def check_block_size_range(block_size_range):
    """The rule aej_set_settings applies to every Jpeg call, with its errors: powers of two, 2 <= min <= max <= 1024, at most 8 sizes."""
    lo, hi = (int(v) for v in block_size_range)
    pow2 = lambda v: v > 0 and v & (v - 1) == 0      # noqa: E731
    if not pow2(lo) or not pow2(hi) or lo > hi or lo < 2:
        raise ValueError(f"block size range ({lo}, {hi}): powers of two with 2 <= min <= max required")
    if hi > 1024:
        raise NotImplementedError(f"block size range ({lo}, {hi}): no kernel for blocks above 1024")
    if int(math.log2(hi)) - int(math.log2(lo)) + 1 > 8:
        raise NotImplementedError(f"block size range ({lo}, {hi}) spans more than 8 sizes")


def qmats_blob(color_space, quality_range, block_size_range) -> np.ndarray:
    """[layer][size][s*s] int32 of Jpeg.precompute_caches for these settings (the layout aej_set_settings and the requantisation take)."""
    settings = JpegCompressionSettings(color_space, tuple(quality_range), tuple(block_size_range))
    sizes = tables.block_sizes(settings.block_size_range)
    return np.concatenate([tables.quantization_matrix(qm, s, tables.quality_factor(s, settings.block_size_range, settings.quality_range)).ravel()
                           for qm in settings.quantization_matrices for s in sizes]).astype(np.int32)


class StandardResult:
    """Standard JPEG of every image at every quality: [image, quality] arrays; ``bytes`` are len() of Pillow's files."""

    def __init__(self, qualities, n, lpips=False, subsampling="4:2:0", optimize=False, progressive=False):
        self.qualities: List[int] = list(qualities)
        self.subsampling: str = subsampling      # "4:4:4" / "4:2:2" / "4:2:0": the one setting of the sweep
        self.optimize: bool = optimize
        self.progressive: bool = progressive
        q = len(self.qualities)
        self.psnr = np.full((n, q), np.nan)
        self.ssim = np.full((n, q), np.nan)
        self.ms_ssim = np.full((n, q), np.nan)
        self.lpips = np.full((n, q), np.nan) if lpips else None
        self.bytes = np.zeros((n, q), np.int64)
        self.compression_ratio = np.full((n, q), np.nan)


class SweepResult:
    """One row per image, one column per cell; ``cells`` in the reference's ``product`` order."""

    def __init__(self, cells, names, shapes, which, sizes, lpips=False):
        n, c = len(names), len(cells)
        self.cells: List[Tuple[str, Tuple[int, int], Tuple[int, int]]] = cells
        self.names: List[str] = names
        self.shapes = shapes
        self.psnr = np.full((n, c), np.nan)
        self.ssim = np.full((n, c), np.nan)
        self.ms_ssim = np.full((n, c), np.nan)
        self.lpips = np.full((n, c), np.nan) if lpips else None      # only when the sweep was given LPIPS weights
        self.bytes = np.zeros((n, c), np.int64)
        self.compression_ratio = np.full((n, c), np.nan)
        self.sizes = sizes
        self.which = which
        self.sub_batches = {}          # (color_space, block_size_range) -> [[image indices of one encode call], ...]
        self.standard: Optional[StandardResult] = None      # sweep(..., standard_qualities=...)

    def columns(self):
        """CSV_COLUMNS_LPIPS when the sweep computed LPIPS, else CSV_COLUMNS."""
        return CSV_COLUMNS_LPIPS if self.lpips is not None else CSV_COLUMNS

    def rows(self):
        """dicts with the reference CSV's column names (metrics_computation.py:185-197), ``lpips`` only when the sweep computed it; image
        by image, cells in order."""
        out = []
        for i, name in enumerate(self.names):
            for j, (cs, qr, br) in enumerate(self.cells):
                r = {"image_name": name, "color_space": cs, "min_quality": qr[0], "max_quality": qr[1], "min_block_size": br[0],
                     "max_block_size": br[1], "psnr": float(self.psnr[i, j]), "ssim": float(self.ssim[i, j]), "ms_ssim": float(self.ms_ssim[i, j])}
                if self.lpips is not None:
                    r["lpips"] = float(self.lpips[i, j])
                r["compression_ratio"] = float(self.compression_ratio[i, j])
                out.append(r)
        return out

    def to_csv(self, path):
        """The reference's CSV (DataFrame.to_csv(index=False)): its column order, metrics and ratio as ``:.4f``; ``lpips`` only when the
        sweep computed it."""
        cols = self.columns()
        with open(path, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(cols)
            for r in self.rows():
                w.writerow([r[k] if k in CSV_COLUMNS[:6] else f"{r[k]:.4f}" for k in cols])


    def to_csv_standard(self, path):
        """The standard-JPEG rows (sweep(..., standard_qualities=...)): image by image, qualities in order; metrics and ratio as ``:.4f``,
        ``lpips`` only when the sweep computed it."""
        st = self.standard
        if st is None:
            raise ValueError("the sweep ran without standard_qualities")
        cols = STANDARD_COLUMNS_LPIPS if st.lpips is not None else STANDARD_COLUMNS
        with open(path, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(cols)
            for i, name in enumerate(self.names):
                for j, q in enumerate(st.qualities):
                    v = {"psnr": st.psnr[i, j], "ssim": st.ssim[i, j], "ms_ssim": st.ms_ssim[i, j], "compression_ratio": st.compression_ratio[i, j]}
                    if st.lpips is not None:
                        v["lpips"] = st.lpips[i, j]
                    w.writerow([name, q] + [f"{float(v[k]):.4f}" for k in cols[2:]])


def _shape_groups(images):
    """-> (list of (indices, batch), shapes): arrays / tensors [B, H, W, 3] as one group, lists grouped by shape."""
    if hasattr(images, "ndim") and images.ndim == 4:
        if images.shape[3] != 3:
            raise ValueError("Input batch must be [B, H, W, 3].")
        return [(list(range(images.shape[0])), images)], [tuple(images.shape[1:3])] * images.shape[0]
    items = list(images)
    if not items:
        raise ValueError("sweep needs at least one image")
    shapes = []
    for x in items:
        if x.ndim != 3 or x.shape[2] != 3:
            raise ValueError(f"Unexpected shape: {tuple(x.shape)}")
        shapes.append(tuple(x.shape[:2]))
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)
    out = []
    for s, idx in groups.items():
        first = items[idx[0]]
        if type(first).__module__.startswith("torch"):
            import torch
            out.append((idx, torch.stack([items[i] for i in idx])))
        else:
            out.append((idx, np.stack([np.asarray(items[i]) for i in idx])))
    return out, shapes


class _Plan:
    """Sub-batch and quality-group sizes of one (shape, colour space, block range) under the byte budget."""

    def __init__(self, ctx, n_img, H, W, n_q, which, sizes, max_bytes, in_bytes, lpips=False):
        lib = ctx.lib

        def cost(b, g):
            p = ctx.plan(b, H, W)
            coef = 4 * b * p.coeff_stride
            c = in_bytes * b * H * W * 3 + 4 * b * H * W * 3       # input (+ its float32 copy for the metrics) ...
            c += 2 * coef + 16 * b * p.leaf_stride + b * p.state_stride + p.workspace_bytes      # encode outputs with dct_f32, workspace
            c += g * coef + 4 * b * H * W * 3                       # the quality sets, one decoded batch
            c += max(int(lib.aej_decode_workspace_bytes(ctx.handle, b, H, W)), int(lib.aej_metrics_workspace_bytes(b, H, W)) if which else 0,
                     int(lib.aej_lpips_workspace_bytes(b, H, W)) if lpips else 0)
            if lpips:                                               # the originals' LPIPS features
                c += int(lib.aej_lpips_features_bytes(b, H, W))
            if sizes == "gpu":
                c += int(lib.aej_deflate_workspace_bytes(ctx.handle, b, H, W)) + 2 * coef
            return c

        self.batch = 1
        lo, hi = 1, n_img
        while lo <= hi:                                             # largest sub-batch that fits with one quality set
            mid = (lo + hi) // 2
            if cost(mid, 1) <= max_bytes:
                self.batch, lo = mid, mid + 1
            else:
                hi = mid - 1
        self.group = 1
        for g in range(n_q, 0, -1):
            if cost(self.batch, g) <= max_bytes:
                self.group = g
                break


def _gpu_stream_sizes(ctx, coeffs, counts, B, H, W):
    """Lengths of the zlib streams Jpeg.deflate_batch(adaptive=True) writes for these coefficients, without copying the streams back."""
    from . import deflate_tables as DT
    t = ctx.torch
    lib = ctx.lib
    p = ctx.plan(B, H, W)
    nbytes = int(lib.aej_deflate_workspace_bytes(ctx.handle, B, H, W))
    ws = ctx.workspace(nbytes)
    hist = ctx.empty((3, DT.HIST_BINS), t.int32)
    ctx.check(lib.aej_deflate_histogram(ctx.handle, coeffs.data_ptr(), counts.data_ptr(), B, H, W, hist.data_ptr(), ws.data_ptr(),
                                        ctypes.c_uint64(nbytes)))
    h = np.ascontiguousarray(hist.cpu().numpy(), dtype=np.int32)
    cover = np.zeros(3, np.int32)
    tab = np.empty((3, DT.TABLE_WORDS), np.uint32)
    if lib.aej_deflate_build_tables(h.ctypes.data, cover.ctypes.data, tab.ctypes.data):
        raise AejError("aej_deflate_build_tables failed")
    tabs = ctx.to_device(tab.view(np.int32), t.int32)
    cap = max((p.coeff_off[l + 1] if l < 2 else p.coeff_stride) - p.coeff_off[l] for l in range(3))
    stride = (int(lib.aej_deflate_stream_bound(ctypes.c_uint64(4 * cap))) + 255) // 256 * 256
    streams = ctx.empty((3 * B, stride), t.uint8)
    sizes = ctx.empty((3 * B,), t.int64)
    ctx.check(lib.aej_deflate_batch(ctx.handle, coeffs.data_ptr(), counts.data_ptr(), B, H, W, tabs.data_ptr(), 1, streams.data_ptr(),
                                    ctypes.c_uint64(stride), sizes.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nbytes)))
    return sizes.cpu().numpy().reshape(B, 3)


def sweep(images, color_spaces: Sequence[str] = ("YCbCr",), quality_ranges: Sequence[Tuple[int, int]] = ((40, 80),),
          block_size_ranges: Sequence[Tuple[int, int]] = ((4, 64),), metrics: int = PSNR | SSIM | MS_SSIM, sizes: Optional[str] = "zlib",
          extension: Optional[str] = None, names: Optional[Sequence[str]] = None, device: int = 0, max_bytes: Optional[int] = None,
          workers: Optional[int] = None, lpips: Optional[_lpips.LpipsWeights] = None,
          standard_qualities: Optional[Sequence[int]] = None, standard_subsampling="4:2:0", standard_optimize: bool = False,
          standard_progressive: bool = False) -> SweepResult:
    """Every (colour space, quality range, block range) cell for every image: metrics and container sizes equal to
    ``EvaluationMetrics.batch(x, decompress_batch(compress_batch(x)))`` and ``len(compress_many(x, extension=...))`` of that cell.

    images: float32 (in [0, 1]) or uint8 [B, H, W, 3] (numpy or torch), or a list of [H, W, 3] arrays of any sizes (grouped by shape).
    metrics: PSNR | SSIM | MS_SSIM (evaluation_metrics.py); columns not requested are NaN.  sizes: "zlib" | "gpu" | None (module doc).
    max_bytes: device bytes the sweep's buffers may use at their peak (default DEFAULT_MEMORY_FRACTION of the free memory); images are
    sub-batched and quality ranges grouped to stay below it -- metrics and "zlib" sizes do not depend on it.  workers: host zlib threads
    (default: the cores this process may use).  lpips: LpipsWeights -> also ``SweepResult.lpips`` (equal to
    ``EvaluationMetrics.lpips_batch`` of every cell) and the ``lpips`` CSV column; images must then be at least 31x31.
    standard_qualities: JPEG qualities (1..100) -> ``SweepResult.standard``: the same metrics (and LPIPS) of Pillow's standard-JPEG decode
    (``u8 / 255``) against the same originals, and ``compression_ratio = H * W * 3 / len(file)`` (module doc).
    standard_subsampling ("4:4:4", "4:2:2", "4:2:0" or 0, 1, 2), standard_optimize (bool): Pillow's ``subsampling=`` and ``optimize=`` of
    those files, one setting per sweep, recorded in ``SweepResult.standard.subsampling / .optimize``; they need standard_qualities.
    standard_progressive (bool): Pillow's ``progressive=`` of those files (``SweepResult.standard.progressive``): the sizes and ratios
    are the progressive files', the metrics do not change.  The settings are bound on the device's context of the current stream, as Jpeg does: other
    Jpeg objects bind theirs again on their next call."""
    if sizes not in ("zlib", "gpu", None):
        raise ValueError("sizes must be 'zlib', 'gpu' or None")
    if metrics & ~(PSNR | SSIM | MS_SSIM):
        raise ValueError("metrics must be a combination of PSNR, SSIM and MS_SSIM")
    if lpips is not None and not isinstance(lpips, _lpips.LpipsWeights):
        raise TypeError("lpips must be LpipsWeights (LpipsWeights.load(...)) or None")
    color_spaces, quality_ranges, block_size_ranges = list(color_spaces), [tuple(q) for q in quality_ranges], [tuple(b) for b in block_size_ranges]
    if not color_spaces or not quality_ranges or not block_size_ranges:
        raise ValueError("every axis of the grid needs at least one value")
    # everything is checked before any device work, with the errors a Jpeg of those settings raises
    blobs = {}
    for cs, qr, br in itertools.product(color_spaces, quality_ranges, block_size_ranges):
        JpegCompressionSettings(cs, qr, br)
        check_block_size_range(br)
        blobs[cs, qr, br] = qmats_blob(cs, qr, br)
    groups, shapes = _shape_groups(images)
    n_img = len(shapes)
    names = [f"image_{i}" for i in range(n_img)] if names is None else [str(n) for n in names]
    if len(names) != n_img:
        raise ValueError(f"{len(names)} names for {n_img} images")
    if metrics & MS_SSIM:
        for i, (h, w) in enumerate(shapes):
            if h < 161 or w < 161:
                raise ValueError(f"image {i} ({h}x{w}): MS-SSIM needs images of at least 161x161.")
    if lpips is not None:
        for i, (h, w) in enumerate(shapes):
            _lpips.check_size(h, w, f"image {i}")
    std_ss, std_opt = _std._check_subsampling(standard_subsampling), _std._check_bool("optimize", standard_optimize)
    std_prog = _std._check_bool("progressive", standard_progressive)
    if standard_qualities is None and (std_ss != 2 or std_opt or std_prog):
        raise ValueError("standard_subsampling / standard_optimize / standard_progressive need standard_qualities")
    if standard_qualities is not None:
        standard_qualities = [_std._check_quality(q) for q in standard_qualities]
        if not standard_qualities:
            raise ValueError("standard_qualities needs at least one quality")
        for i, (h, w) in enumerate(shapes):
            if h > 65535 or w > 65535:
                raise ValueError(f"image {i} ({h}x{w}): baseline JPEG holds at most 65535 x 65535")
    cells = list(itertools.product(color_spaces, quality_ranges, block_size_ranges))
    res = SweepResult(cells, names, shapes, metrics, sizes, lpips=lpips is not None)
    if standard_qualities is not None:
        res.standard = StandardResult(standard_qualities, n_img, lpips=lpips is not None, subsampling=_std.SUBSAMPLING_NAMES[std_ss],
                                      optimize=std_opt, progressive=std_prog)
    col = {c: j for j, c in enumerate(cells)}

    ctx = get_context(device)
    t = ctx.torch
    if max_bytes is None:
        max_bytes = int(DEFAULT_MEMORY_FRACTION * t.cuda.mem_get_info(ctx.device)[0])
    codec = Jpeg(JpegCompressionSettings(color_spaces[0], quality_ranges[0], block_size_ranges[0]), device=device)
    n_workers = workers or usable_cpus()
    pending = None
    pool = ThreadPoolExecutor(max_workers=n_workers) if sizes == "zlib" else None
    try:
        for idx, batch in groups:
            is_u8 = str(getattr(batch, "dtype", "")) in ("uint8", "torch.uint8")
            x_all = ctx.to_device(batch, t.uint8 if is_u8 else t.float32)
            H, W = int(x_all.shape[1]), int(x_all.shape[2])
            ten_f32_255 = t.full((), 255.0, dtype=t.float32, device=ctx.device)
            feats = {}                                              # (first image, count) -> the originals' LPIPS features of that sub-batch
            for cs, br in itertools.product(color_spaces, block_size_ranges):
                codec.update_settings(JpegCompressionSettings(cs, quality_ranges[0], br))
                ctx = codec._bind()
                pending = _Pending(2 * n_workers // 3 // max(1, len(idx)) + 2) if pending is None else pending
                plan = _Plan(ctx, len(idx), H, W, len(quality_ranges), metrics, sizes, max_bytes, 1 if is_u8 else 4, lpips is not None)
                res.sub_batches.setdefault((cs, br), [])
                for b0 in range(0, len(idx), plan.batch):
                    sub = idx[b0:b0 + plan.batch]
                    res.sub_batches[cs, br].append(list(sub))
                    x = x_all[b0:b0 + len(sub)]
                    xf = (x.float() / ten_f32_255) if is_u8 else x      # Image.load's float32(v) / 255 (a tensor divisor: torch multiplies
                                                                         # by the reciprocal of a Python scalar, which is not always the quotient)
                    fa = None
                    if lpips is not None:                           # computed once per sub-batch, reused while the sub-batches repeat
                        fa = feats.get((b0, len(sub)))
                        if fa is None:
                            feats.clear()
                            fa = feats[b0, len(sub)] = _lpips.features(ctx, lpips, xf.contiguous())
                    _sweep_sub(ctx, codec, res, col, blobs, cs, br, quality_ranges, plan.group, sub, x, xf, metrics, sizes, extension,
                               pool, pending, lpips, fa)
            if standard_qualities is not None:
                _sweep_standard(ctx, res.standard, idx, x_all, is_u8, ten_f32_255, metrics, lpips, max_bytes)
        while pending:
            _collect(res, pending.pop(0))
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
    if sizes is not None:
        px = np.array([h * w * 3 for h, w in shapes], np.float64)
        res.compression_ratio = px[:, None] / res.bytes
    if res.standard is not None:
        px = np.array([h * w * 3 for h, w in shapes], np.float64)
        res.standard.compression_ratio = px[:, None] / res.standard.bytes
    return res


def _standard_plan(ctx, n_img, H, W, n_q, which, max_bytes, in_bytes, lpips, subsampling=2, optimize=False, progressive=False):
    """(images per call, qualities per call) of the standard-JPEG pass under the byte budget"""
    lib = ctx.lib

    def cost(b, g):
        c = in_bytes * b * H * W * 3 + 4 * b * H * W * 3 + b * H * W * 3        # input, its float32 copy, its uint8 form
        c += _std.workspace_bytes(ctx, b, H, W, g, subsampling, optimize, progressive) + g * b * H * W * 3 + 4 * b * H * W * 3     # encode, decoded sets, one float32 set
        c += max(int(lib.aej_metrics_workspace_bytes(b, H, W)) if which else 0, int(lib.aej_lpips_workspace_bytes(b, H, W)) if lpips else 0)
        if lpips:
            c += int(lib.aej_lpips_features_bytes(b, H, W))
        return c

    batch, lo, hi = 1, 1, n_img
    while lo <= hi:
        mid = (lo + hi) // 2
        if cost(mid, 1) <= max_bytes:
            batch, lo = mid, mid + 1
        else:
            hi = mid - 1
    group = next((g for g in range(n_q, 0, -1) if cost(batch, g) <= max_bytes), 1)
    return batch, group


def _sweep_standard(ctx, st, idx, x_all, is_u8, ten_f32_255, metrics, lpips, max_bytes):
    """Standard JPEG of one shape group: per image sub-batch one encode for a group of qualities, then per quality Pillow's decode scored
    against the originals (as the adaptive cells are)."""
    t = ctx.torch
    lib = ctx.lib
    H, W = int(x_all.shape[1]), int(x_all.shape[2])
    batch, group = _standard_plan(ctx, len(idx), H, W, len(st.qualities), metrics, max_bytes, 1 if is_u8 else 4, lpips is not None,
                                  st.subsampling, st.optimize, st.progressive)
    for b0 in range(0, len(idx), batch):
        sub = idx[b0:b0 + batch]
        x = x_all[b0:b0 + len(sub)]
        B = len(sub)
        xf = (x.float() / ten_f32_255) if is_u8 else x
        x_u8 = x if is_u8 else _std._to_u8(ctx, x)
        fa = _lpips.features(ctx, lpips, xf.contiguous()) if lpips is not None else None
        for g0 in range(0, len(st.qualities), group):
            qs = st.qualities[g0:g0 + group]
            enc = _std.encode_decode(ctx, x_u8, qs, False, st.subsampling, st.optimize, st.progressive)
            dec = enc.decoded()
            scores, lp = [], []
            for s in range(len(qs)):
                rgb = dec[s].float() / ten_f32_255
                if metrics:
                    ws_bytes = int(lib.aej_metrics_workspace_bytes(B, H, W))
                    ws = ctx.workspace(ws_bytes)
                    m = ctx.empty((B, 3), t.float64)
                    ctx.check(lib.aej_metrics_batch(ctx.handle, xf.data_ptr(), rgb.data_ptr(), B, H, W, metrics, m.data_ptr(), ws.data_ptr(),
                                                    ctypes.c_uint64(ws_bytes)))
                    scores.append(m)
                if lpips is not None:
                    lp.append(_lpips.score(ctx, lpips, rgb, feats_a=fa))
            for s in range(len(qs)):
                j = g0 + s
                for bi, i in enumerate(sub):
                    st.bytes[i, j] = int(enc.lengths[s, bi])
            if scores:
                vals = t.stack(scores).cpu().numpy()
                for s in range(len(qs)):
                    for bi, i in enumerate(sub):
                        st.psnr[i, g0 + s], st.ssim[i, g0 + s], st.ms_ssim[i, g0 + s] = vals[s, bi]
            if lp:
                vals = t.stack(lp).cpu().numpy()
                for s in range(len(qs)):
                    for bi, i in enumerate(sub):
                        st.lpips[i, g0 + s] = vals[s, bi]


def _sweep_sub(ctx, codec, res, col, blobs, cs, br, quality_ranges, group, sub, x, xf, metrics, sizes, extension, pool, pending, lpips=None,
               feats=None):
    """Steps 2-4 of the module doc for one image sub-batch under one (colour space, block range)."""
    t = ctx.torch
    lib = ctx.lib
    enc = codec.compress_batch(x, want_dct=True)
    p = enc.plan
    B, H, W = p.batch, p.H, p.W
    cnt = enc.counts_host
    set_elems = B * p.coeff_stride
    dec_ws_bytes = int(lib.aej_decode_workspace_bytes(ctx.handle, B, H, W))
    met_ws_bytes = int(lib.aej_metrics_workspace_bytes(B, H, W)) if metrics else 0
    lp_ws_bytes = int(lib.aej_lpips_workspace_bytes(B, H, W)) if lpips is not None else 0
    rgb = ctx.empty((B, H, W, 3), t.float32)
    scores, lp_scores = [], []
    for g0 in range(0, len(quality_ranges), group):
        qrs = quality_ranges[g0:g0 + group]
        blob_host = np.concatenate([blobs[cs, qr, br] for qr in qrs])
        blob = ctx.to_device(blob_host, t.int32)
        set_words = blob_host.size // len(qrs)
        out = ctx.empty((len(qrs), set_elems), t.int32)
        ctx.check(lib.aej_requantise_batch(ctx.handle, enc.dct.data_ptr(), enc.leaves.data_ptr(), enc.counts.data_ptr(), B, H, W, len(qrs),
                                           blob.data_ptr(), out.data_ptr(), ctypes.c_uint64(set_elems)))
        for s, qr in enumerate(qrs):
            j = col[cs, qr, br]
            coeffs = out[s]
            qset = blob[s * set_words:(s + 1) * set_words]
            if metrics or lpips is not None:
                ws = ctx.workspace(max(dec_ws_bytes, met_ws_bytes, lp_ws_bytes))
                ctx.check(lib.aej_decode_batch_tables(ctx.handle, coeffs.data_ptr(), enc.leaves.data_ptr(), enc.counts.data_ptr(), B, H, W,
                                                      qset.data_ptr(), rgb.data_ptr(), ws.data_ptr(), ctypes.c_uint64(dec_ws_bytes)))
            if metrics:
                m = ctx.empty((B, 3), t.float64)
                ctx.check(lib.aej_metrics_batch(ctx.handle, xf.data_ptr(), rgb.data_ptr(), B, H, W, metrics, m.data_ptr(), ws.data_ptr(),
                                                ctypes.c_uint64(met_ws_bytes)))
                scores.append((j, m))
            if lpips is not None:
                lp_scores.append((j, _lpips.score(ctx, lpips, rgb, feats_a=feats)))
            if sizes is None:
                continue
            hdr = container_length(H, W, cs, qr, br, extension, [0, 0, 0], [0, 0, 0]) - 36
            if sizes == "gpu":
                lens = _gpu_stream_sizes(ctx, coeffs, enc.counts, B, H, W).reshape(-1)
                for bi, i in enumerate(sub):
                    res.bytes[i, j] = hdr + sum(12 + (int(cnt[bi, l, 2]) + 3) // 4 + int(lens[3 * bi + l]) for l in range(3))
            else:
                # one device-to-host copy of the set into page-locked memory; the host threads wait for it and deflate its layers while
                # the GPU goes on with the next sets
                while len(pending) >= pending.limit:            # bounded page-locked memory: the oldest set's deflates finish first
                    _collect(res, pending.pop(0))
                host = t.empty((set_elems,), dtype=t.int32, pin_memory=True)
                host.copy_(coeffs, non_blocking=True)
                ev = t.cuda.Event()
                ev.record(t.cuda.current_stream(ctx.device))
                a = host.numpy()
                futs = [pool.submit(_deflate_layer, ev, a, b * p.coeff_stride + p.coeff_off[l], int(cnt[b, l, 0]))
                        for b in range(B) for l in range(3)]
                pending.append((futs, host, sub, j, cnt, hdr))
    if scores:
        vals = t.stack([m for _, m in scores]).cpu().numpy()      # [sets, B, 3]
        for (j, _), v in zip(scores, vals):
            for bi, i in enumerate(sub):
                res.psnr[i, j], res.ssim[i, j], res.ms_ssim[i, j] = v[bi]
    if lp_scores:
        vals = t.stack([m for _, m in lp_scores]).cpu().numpy()   # [sets, B]
        for (j, _), v in zip(lp_scores, vals):
            for bi, i in enumerate(sub):
                res.lpips[i, j] = v[bi]


class _Pending(list):
    """The quality sets whose host deflates are in flight: (futures per (image, layer), page-locked copy, images, column, counts, header)."""

    def __init__(self, limit):
        super().__init__()
        self.limit = max(2, limit)


def _deflate_layer(ev, a, o, n):
    """Host zlib level 9 of one layer's coefficients (jpeg.py:588-590) once the copy has landed: -> the stream's length."""
    ev.synchronize()
    return len(zlib.compress(a[o:o + n].tobytes(), level=9))


def _collect(res, entry):
    futs, _host, sub, j, cnt, hdr = entry
    lens = [f.result() for f in futs]
    for bi, i in enumerate(sub):
        res.bytes[i, j] = hdr + sum(12 + (int(cnt[bi, l, 2]) + 3) // 4 + lens[3 * bi + l] for l in range(3))
