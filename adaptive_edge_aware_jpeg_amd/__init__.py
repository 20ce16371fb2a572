"""adaptive_edge_aware_jpeg_amd -- MI355X (gfx950) implementation of the adaptive edge-aware JPEG ENCODE hot path.

Same Python surface as the reference for this path (fevzibabaoglu/adaptive-edge-aware-jpeg):
``Jpeg``, ``JpegCompressionSettings``, ``Image``, ``EvaluationMetrics``, ``EdgeDetection``, ``QuadTree``, ``convert``,
``apply_normalization``, ``get_color_spaces``; and standard JPEG (``standard_jpeg_many`` / ``standard_jpeg_batch``, byte-identical to
Pillow's files) for the reference's comparison against it, and ``standard_jpeg_decode_many`` (baseline .jpg files decoded on the GPU,
pixel-identical to Pillow), ``resize_many`` (``Image.resize``) and ``standard_jpeg_thumbnail_many`` (``Image.thumbnail`` on JPEG files),
both pixel-identical to Pillow too; ``standard_jpeg_encode_many`` encodes images of mixed sizes and qualities in one call and
``standard_jpeg_thumbnail_jpeg_many`` goes from JPEG files to their JPEG thumbnails on the device; ``png_decode_many`` decodes PNG files
on the device, pixel-identical to Pillow, and ``png_encode_many`` writes them there with Pillow's scanline filtering; ``filter_many`` is ``Image.filter`` with Pillow's ``BoxBlur``,
``GaussianBlur`` and ``UnsharpMask``, its ``Kernel`` (``SHARPEN`` and the other built-ins), rank (``MedianFilter`` ...) and mode filters and its ``Color3DLUT``, pixel-identical as well;
``adjust_many`` is ``ImageEnhance`` (``Brightness``, ``Contrast``, ``Color``, ``Sharpness``) and the point operations of ``ImageOps`` (``AutoContrast``, ``Equalize``,
``Posterize``, ``Solarize``, ``Invert``, ``Grayscale``) and ``Image.point``, one op or a chain per image, and ``histogram_many`` is ``Image.histogram``;
``paste_many``, ``alpha_composite_many``, ``blend_many``, ``composite_many`` and ``chop_many`` are ``Image.paste`` (with every mask Pillow takes), ``Image.alpha_composite``,
``Image.blend``, ``Image.composite`` and ``ImageChops`` for lists of image pairs; ``convert_many`` is ``Image.convert`` between "L", "LA", "RGB", "RGBA", "YCbCr",
"HSV" and "CMYK" (and ``convert(mode, matrix)``), ``hue_many`` torchvision's ``adjust_hue`` and ``colorize_many`` ``ImageOps.colorize``.  The arithmetic runs in hand-written HIP kernels behind the
C ABI of ``libaejpeg_hip.so`` (include/aej.h); there is no CPU fallback.
"""
from ._lib import _look_at_hw_queues, configure_hw_queues, hw_queues, set_hw_queues

# Streams beyond the HIP runtime's hardware queues share queues and serialise; the library's overlap of sub-batches and calls wants a
# queue per stream.  Importing this package only LOOKS at GPU_MAX_HW_QUEUES (it never writes the environment); `configure_hw_queues()`
# is the explicit opt-in, `hw_queues()` reports what the library schedules for, `set_hw_queues(n)` states it (policy: _lib.py).
_look_at_hw_queues()

from .adjust import (AutoContrast, Brightness, Color, Colorize, Contrast, Equalize, Grayscale, Hue, Invert, Point, Posterize, Sharpness, Solarize,  # noqa: E402
                     adjust_many, adjust_plan, histogram_many)
# (the submodule convert.py is imported BEFORE the function of the same name: the package attribute `convert` stays the function)
from .convert import colorize_many, convert_many, convert_plan, hue_many  # noqa: E402
from .color import apply_normalization, convert, get_color_spaces  # noqa: E402
from .compose import ChopAdd, ChopSubtract, alpha_composite_many, blend_many, chop_many, compose_plan, composite_many, paste_many  # noqa: E402
from .edge_detection import EdgeDetection  # noqa: E402
from .evaluation_metrics import EvaluationMetrics  # noqa: E402
from .filters import (BLUR, CONTOUR, DETAIL, EDGE_ENHANCE, EDGE_ENHANCE_MORE, EMBOSS, FIND_EDGES, SHARPEN, SMOOTH, SMOOTH_MORE, BoxBlur, Color3DLUT, GaussianBlur, Kernel,  # noqa: E402
                      MaxFilter, MedianFilter, MinFilter, ModeFilter, RankFilter, UnsharpMask, filter_many, lut3d_plan)
from .geometry import rotate_many, transform_many, transform_plan, transpose_many  # noqa: E402
from .image import Image  # noqa: E402
from .jpeg import EncodedBatch, Jpeg  # noqa: E402
from .lpips import LpipsWeights  # noqa: E402
from .png import png_adam7_passes, png_decode_many, png_encode_many, png_parse_header  # noqa: E402
from .quadtree import QuadNode, QuadTree  # noqa: E402
from .settings import JpegCompressionSettings  # noqa: E402
from .resample import resize_many  # noqa: E402
from .standard_jpeg import (decode_box_stats, decode_box_window, draft_scale, encode_groups, exif_orientation, resized_crop_plan, standard_jpeg_batch, standard_jpeg_decode_many,  # noqa: E402
                            standard_jpeg_encode_many, standard_jpeg_many, standard_jpeg_resized_crop_many, standard_jpeg_thumbnail_jpeg_many, standard_jpeg_thumbnail_many, standard_jpeg_transcode_many, standard_jpeg_transform_many, thumbnail_plan,
                            transform_crop_box, transform_prefix)
from .sweep import SweepResult, reference_grid, sweep  # noqa: E402

__all__ = ["Jpeg", "JpegCompressionSettings", "EncodedBatch", "Image", "EvaluationMetrics", "EdgeDetection", "QuadTree", "QuadNode",
           "convert", "apply_normalization", "get_color_spaces", "hw_queues", "set_hw_queues", "configure_hw_queues",
           "sweep", "reference_grid", "SweepResult", "LpipsWeights", "standard_jpeg_many", "standard_jpeg_batch",
           "standard_jpeg_decode_many", "standard_jpeg_transcode_many", "standard_jpeg_transform_many", "exif_orientation", "draft_scale",
           "resize_many", "standard_jpeg_thumbnail_many", "thumbnail_plan", "standard_jpeg_encode_many", "standard_jpeg_thumbnail_jpeg_many",
           "encode_groups", "transform_prefix", "transform_crop_box", "decode_box_window", "decode_box_stats", "resized_crop_plan",
           "standard_jpeg_resized_crop_many", "png_decode_many", "png_parse_header", "png_adam7_passes", "png_encode_many",
           "BoxBlur", "GaussianBlur", "UnsharpMask", "filter_many", "Kernel", "RankFilter", "MedianFilter", "MinFilter", "MaxFilter", "ModeFilter", "Color3DLUT", "lut3d_plan",
           "BLUR", "CONTOUR", "DETAIL", "EDGE_ENHANCE", "EDGE_ENHANCE_MORE", "EMBOSS", "FIND_EDGES", "SHARPEN", "SMOOTH", "SMOOTH_MORE",
           "transform_many", "rotate_many", "transpose_many", "transform_plan",
           "adjust_many", "histogram_many", "adjust_plan", "Brightness", "Contrast", "Color", "Sharpness", "AutoContrast", "Equalize", "Posterize",
           "Solarize", "Invert", "Grayscale", "Point", "Colorize", "Hue",
           "paste_many", "alpha_composite_many", "blend_many", "composite_many", "chop_many", "compose_plan", "ChopAdd", "ChopSubtract",
           "convert_many", "hue_many", "colorize_many", "convert_plan"]
