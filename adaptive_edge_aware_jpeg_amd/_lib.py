"""ctypes binding of libaejpeg_hip.so (include/aej.h) + a small device-context wrapper.

PyTorch-ROCm is used for device memory and streams only: every tensor handed to the library is a
``torch`` CUDA(=HIP) tensor and the library receives raw device pointers.  There is no CPU fallback: if
the shared library is missing or no GPU is visible, the calls raise.
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AEJ_LIBRARY: developer override used by tools/profiling/variants.py to time experimental builds of the same ABI side by side
# (they live under build/variants/, never in place of the in-tree library)
LIB_PATH = os.environ.get("AEJ_LIBRARY") or os.path.join(_HERE, "libaejpeg_hip.so")

SPACE_IDS = {"YCbCr": 0, "YCoCg": 1, "YCoCg-R": 2, "OKLAB": 3, "ICtCp": 4, "ICaCb": 5, "JzAzBz": 6}
CONVERT_IDS = dict(SPACE_IDS, XYZ=7)     # color.convert also serves the helper space XYZ (conversion.py:63-68); not a codec space

AEJ_ERR_ARG, AEJ_ERR_HIP, AEJ_ERR_STATE, AEJ_ERR_CAPACITY, AEJ_ERR_UNSUPPORTED = -1, -2, -3, -4, -5


class AejError(RuntimeError):
    pass


class AejPlan(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("layer_h", ctypes.c_int32 * 3), ("layer_w", ctypes.c_int32 * 3), ("root_size", ctypes.c_int32 * 3),
        ("coeff_off", ctypes.c_int64 * 3), ("coeff_stride", ctypes.c_int64),
        ("leaf_off", ctypes.c_int64 * 3), ("leaf_stride", ctypes.c_int64),
        ("state_off", ctypes.c_int64 * 3), ("state_stride", ctypes.c_int64),
        ("workspace_bytes", ctypes.c_uint64),
    ]


_lib = None
_lib_lock = threading.Lock()

# ---- hardware queues ------------------------------------------------------------------------------------------------
# HIP maps streams onto at most GPU_MAX_HW_QUEUES hardware queues (default 4) and two streams on one queue run one after the other.
# The library overlaps sub-batches and calls on several streams and picks its schedule by the number of queues --
# which only the host can know: the runtime reads the variable once, when it initialises (any HIP call does that,
# torch.cuda.is_available() included).  IMPORTING THIS PACKAGE CHANGES NOTHING IN THE PROCESS: it only looks.
#   * the variable is in the environment when the package is imported (set by the launcher, or by a script before it imported torch,
#     as bench.py does): that is what the runtime starts with -- its value is what the library is told;
#   * otherwise the library is told HIP's default of 4 (its conservative two-sub-batch schedule).  An application that wants the wide
#     schedule calls configure_hw_queues() BEFORE anything initialises HIP (it sets the variable, explicitly, at the caller's request),
#     or states the value its runtime really started with through set_hw_queues().
HIP_DEFAULT_HW_QUEUES = 4
_hw_queues = HIP_DEFAULT_HW_QUEUES
_hw_queues_source = "HIP default (assumed)"


def _look_at_hw_queues():
    """Called once at package import: read-only (see the policy above)."""
    global _hw_queues, _hw_queues_source
    present = os.environ.get("GPU_MAX_HW_QUEUES")
    if present is not None:
        try:
            v = int(present)
        except ValueError:
            v = 0
        if v > 0:
            _hw_queues, _hw_queues_source = v, "GPU_MAX_HW_QUEUES was in the environment when the package was imported"
    return _hw_queues


def configure_hw_queues(want=16):
    """Explicit opt-in, to be called BEFORE `import torch` (the HIP runtime reads GPU_MAX_HW_QUEUES once, when it initialises, and
    torch.cuda.is_available() / device_count() already initialise it): puts GPU_MAX_HW_QUEUES=<want> into this process's environment so
    that every stream of the library gets a hardware queue of its own, and tells the library.  If torch is already imported nobody can
    know whether the runtime has read the variable: it is still set (it cannot hurt) but the library keeps HIP's default of 4 -- told 16
    while the runtime has 4 it would put four sub-batches on streams that serialise, measured slower than the conservative schedule --
    unless the application states the real value through set_hw_queues().  Returns the queue count the library will schedule for."""
    global _hw_queues, _hw_queues_source
    import sys
    if os.environ.get("GPU_MAX_HW_QUEUES") is not None:
        return _look_at_hw_queues()
    trusted = "torch" not in sys.modules
    os.environ["GPU_MAX_HW_QUEUES"] = str(int(want))
    if trusted:
        _hw_queues, _hw_queues_source = int(want), "configure_hw_queues() before torch was imported"
        for ctx in _contexts.values():
            ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, _hw_queues))
    return _hw_queues


def set_hw_queues(n):
    """For applications that initialise HIP before importing this package: the value of GPU_MAX_HW_QUEUES their runtime started
    with.  Applies to contexts created afterwards and to the existing ones."""
    global _hw_queues, _hw_queues_source
    _hw_queues, _hw_queues_source = int(n), "stated by the application (set_hw_queues)"
    for ctx in _contexts.values():
        ctx.check(ctx.lib.aej_set_hw_queues(ctx.handle, _hw_queues))


def hw_queues():
    """-> (queues the library schedules for, where the number comes from)"""
    return _hw_queues, _hw_queues_source


_warned_queue_limited = False


def warn_if_queue_limited(ctx, batch, H, W):
    """Once per process: a call large enough for the library to cut it into four overlapping sub-batches runs the conservative schedule
    because the library was told the HIP runtime has fewer than 8 hardware queues (its default is 4) -- the drop-in then runs about 10 %
    below what bench.py measures.  Says how to get the wide schedule."""
    global _warned_queue_limited
    if _warned_queue_limited:
        return
    sch = ctx.schedule(batch, H, W)
    if sch["limited_by_hw_queues"]:
        _warned_queue_limited = True
        import warnings
        warnings.warn(f"adaptive_edge_aware_jpeg_amd: this call ({batch} x {W}x{H}) would run as more overlapping sub-batches with more hardware "
                      f"queues; the library schedules for {sch['hw_queues']} ({_hw_queues_source}).  Put GPU_MAX_HW_QUEUES=16 into the environment "
                      "(or call adaptive_edge_aware_jpeg_amd.configure_hw_queues()) before `import torch`, or state the runtime's real value with "
                      "set_hw_queues().", RuntimeWarning, stacklevel=3)


# name -> (restype, argtypes); exactly the symbols declared in include/aej.h
_P, _I, _I64, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
class CannyParams(ctypes.Structure):
    """aej_canny_params (include/aej.h)"""
    _fields_ = [("canny_low_ratio", ctypes.c_double), ("canny_high_ratio", ctypes.c_double), ("clahe_clip_limit", ctypes.c_double),
                ("bilateral_sigma_color", ctypes.c_double), ("bilateral_sigma_space", ctypes.c_double), ("use_l2_gradient", ctypes.c_int)]


class JpegDecHuff(ctypes.Structure):
    """aej_jpegdec_huff (include/aej.h)"""
    _fields_ = [("lut", ctypes.c_uint16 * 512), ("maxcode", ctypes.c_int32 * 18), ("valoff", ctypes.c_int32 * 18), ("vals", ctypes.c_uint8 * 256)]


class JfifManyDesc(ctypes.Structure):
    """aej_jfif_many_desc (include/aej.h): one image of aej_jfif_many_encode"""
    _fields_ = [("src_offset", ctypes.c_int64), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("quality", ctypes.c_int32),
                ("components", ctypes.c_int32)]      # 0 or 3: packed RGB; 1: packed grey


class JpegDecDesc(ctypes.Structure):
    """aej_jpegdec_desc (include/aej.h): what aej_jpegdec_parse_host reads from a file's markers"""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("hs", ctypes.c_int32), ("vs", ctypes.c_int32),
                ("mcux", ctypes.c_int32), ("mcuy", ctypes.c_int32), ("blocks_per_mcu", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
                ("n_segments", ctypes.c_int32), ("sof", ctypes.c_int32), ("precision16", ctypes.c_int32),
                ("comp_id", ctypes.c_uint8 * 4), ("comp_h", ctypes.c_uint8 * 4), ("comp_v", ctypes.c_uint8 * 4), ("comp_tq", ctypes.c_uint8 * 4),
                ("qt", (ctypes.c_uint16 * 64) * 3), ("dc", JpegDecHuff * 3), ("ac", JpegDecHuff * 3),
                ("scan_offset", ctypes.c_int64), ("scan_length", ctypes.c_int64)]


class JpegAdobe(ctypes.Structure):
    """aej_jpeg_adobe (include/aej.h): the colour model of a file (JPEG_COLOURS) and, of a four-component one, component 3's sampling
    factors and tables -- what the _adobe parsers write beside the descriptor"""
    _fields_ = [("colour", ctypes.c_int32), ("h3", ctypes.c_int32), ("v3", ctypes.c_int32), ("tq3", ctypes.c_int32),
                ("qt3", ctypes.c_uint16 * 64), ("dc3", JpegDecHuff), ("ac3", JpegDecHuff)]


JPEG_COLOURS = ("YCbCr", "RGB", "CMYK", "YCCK")      # AEJ_JPEG_*: aej_jpeg_adobe.colour ("YCbCr" also for a one-component file)


class JpegProgFrame(ctypes.Structure):
    """aej_jpegprog_frame (include/aej.h): the frame of a progressive file"""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("hs", ctypes.c_int32), ("vs", ctypes.c_int32),
                ("mcux", ctypes.c_int32), ("mcuy", ctypes.c_int32), ("blocks_per_mcu", ctypes.c_int32), ("sof", ctypes.c_int32),
                ("precision16", ctypes.c_int32), ("n_scans", ctypes.c_int32), ("n_levels", ctypes.c_int32),
                ("comp_id", ctypes.c_uint8 * 4), ("comp_h", ctypes.c_uint8 * 4), ("comp_v", ctypes.c_uint8 * 4), ("comp_tq", ctypes.c_uint8 * 4),
                ("qt", (ctypes.c_uint16 * 64) * 3)]


class JpegProgScan(ctypes.Structure):
    """aej_jpegprog_scan (include/aej.h): one scan of a progressive file, with the Huffman tables in force at its SOS"""
    _fields_ = [("ncomp", ctypes.c_int32), ("comp", ctypes.c_int32 * 4), ("td", ctypes.c_int32 * 4), ("ta", ctypes.c_int32 * 4),
                ("ss", ctypes.c_int32), ("se", ctypes.c_int32), ("ah", ctypes.c_int32), ("al", ctypes.c_int32),
                ("restart_interval", ctypes.c_int32), ("units_x", ctypes.c_int32), ("units_y", ctypes.c_int32),
                ("n_segments", ctypes.c_int32), ("level", ctypes.c_int32), ("dc", JpegDecHuff * 3), ("ac", JpegDecHuff),
                ("data_offset", ctypes.c_int64), ("data_length", ctypes.c_int64)]


class ResampleDesc(ctypes.Structure):
    """aej_resample_desc (include/aej.h): one image of aej_resample_batch"""
    _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64), ("src_w", ctypes.c_int32), ("src_h", ctypes.c_int32),
                ("dst_w", ctypes.c_int32), ("dst_h", ctypes.c_int32), ("box", ctypes.c_float * 4), ("filter", ctypes.c_int32),
                ("reduce_x", ctypes.c_int32), ("reduce_y", ctypes.c_int32), ("reduce_box", ctypes.c_int32 * 4), ("reserved", ctypes.c_int32)]


class FilterDesc(ctypes.Structure):
    """aej_filter_desc (include/aej.h): one image of aej_filter_batch"""
    _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("kind", ctypes.c_int32), ("xradius", ctypes.c_float), ("yradius", ctypes.c_float),
                ("percent", ctypes.c_int32), ("threshold", ctypes.c_int32)]


class FilterPlan(ctypes.Structure):
    """aej_filter_plan (include/aej.h): what aej_filter_plan_host makes of a filter, per axis (x, y)"""
    _fields_ = [("passes", ctypes.c_int32), ("box", ctypes.c_float * 2), ("r", ctypes.c_int32 * 2), ("ww", ctypes.c_uint32 * 2),
                ("fw", ctypes.c_uint32 * 2)]


class WindowDesc(ctypes.Structure):
    """aej_window_desc (include/aej.h): one image of aej_window_batch"""
    _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("kind", ctypes.c_int32), ("size", ctypes.c_int32), ("rank", ctypes.c_int32),
                ("scale", ctypes.c_float), ("offset", ctypes.c_float), ("kernel", ctypes.c_float * 25), ("reserved", ctypes.c_int32)]


class Lut3dDesc(ctypes.Structure):
    """aej_lut3d_desc (include/aej.h): one image of aej_lut3d_batch"""
    _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("channels_in", ctypes.c_int32), ("channels_out", ctypes.c_int32), ("table_channels", ctypes.c_int32),
                ("size", ctypes.c_int32 * 3), ("table", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class WarpDesc(ctypes.Structure):
    """aej_warp_desc (include/aej.h): one image of aej_warp_batch"""
    _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64), ("src_w", ctypes.c_int32), ("src_h", ctypes.c_int32),
                ("dst_w", ctypes.c_int32), ("dst_h", ctypes.c_int32), ("channels", ctypes.c_int32), ("path", ctypes.c_int32),
                ("method", ctypes.c_int32), ("filter", ctypes.c_int32), ("coef", ctypes.c_double * 8), ("fill", ctypes.c_uint8 * 4),
                ("premultiply", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


class WarpPlan(ctypes.Structure):
    """aej_warp_plan (include/aej.h): what aej_warp_plan_host makes of one descriptor"""
    _fields_ = [("path", ctypes.c_int32), ("premultiply", ctypes.c_int32), ("fixed", ctypes.c_int64 * 6)]


class AdjustOp(ctypes.Structure):
    """aej_adjust_op (include/aej.h): one op of a chain"""
    _fields_ = [("kind", ctypes.c_int32), ("table", ctypes.c_int32), ("factor", ctypes.c_float), ("preserve_tone", ctypes.c_int32),
                ("cutoff", ctypes.c_double * 2), ("ignore", ctypes.c_uint32 * 8)]


class AdjustDesc(ctypes.Structure):
    """aej_adjust_desc (include/aej.h): one image of aej_adjust_batch and aej_histogram_batch"""
    _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("n_ops", ctypes.c_int32), ("ops", AdjustOp * 8)]


class AdjustPlan(ctypes.Structure):
    """aej_adjust_plan (include/aej.h): what aej_adjust_plan_host makes of one descriptor"""
    _fields_ = [("out_channels", ctypes.c_int32), ("n_segments", ctypes.c_int32), ("n_passes", ctypes.c_int32), ("n_smooths", ctypes.c_int32),
                ("n_launches", ctypes.c_int32), ("segment_first", ctypes.c_int32 * 8), ("reserved", ctypes.c_int32 * 3)]


class ComposeDesc(ctypes.Structure):
    """aej_compose_desc (include/aej.h): one element of aej_compose_batch"""
    _fields_ = [("base_offset", ctypes.c_int64), ("over_offset", ctypes.c_int64), ("mask_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64),
                ("kind", ctypes.c_int32), ("op", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("channels", ctypes.c_int32),
                ("over_width", ctypes.c_int32), ("over_height", ctypes.c_int32), ("over_channels", ctypes.c_int32),
                ("mask_width", ctypes.c_int32), ("mask_height", ctypes.c_int32), ("mask_channels", ctypes.c_int32), ("mask_kind", ctypes.c_int32),
                ("x", ctypes.c_int32), ("y", ctypes.c_int32), ("box", ctypes.c_int32 * 4), ("alpha", ctypes.c_float), ("scale", ctypes.c_float),
                ("offset", ctypes.c_float), ("colour", ctypes.c_uint8 * 4), ("reserved", ctypes.c_int32 * 2)]


class ComposePlan(ctypes.Structure):
    """aej_compose_plan (include/aej.h): what aej_compose_plan_host makes of one descriptor"""
    _fields_ = [("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32), ("out_channels", ctypes.c_int32), ("region", ctypes.c_int32 * 4),
                ("reads_overlay", ctypes.c_int32), ("reads_mask", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class ConvertDesc(ctypes.Structure):
    """aej_convert_desc (include/aej.h): one image of aej_convert_batch"""
    _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("source_mode", ctypes.c_int32), ("target_mode", ctypes.c_int32), ("kind", ctypes.c_int32),
                ("hue_shift", ctypes.c_int32), ("table", ctypes.c_int32), ("matrix", ctypes.c_float * 12), ("reserved", ctypes.c_int32 * 2)]


class ConvertPlan(ctypes.Structure):
    """aej_convert_plan (include/aej.h): what aej_convert_plan_host makes of one descriptor"""
    _fields_ = [("out_channels", ctypes.c_int32), ("n_steps", ctypes.c_int32), ("step_from", ctypes.c_int32 * 2), ("step_to", ctypes.c_int32 * 2),
                ("reserved", ctypes.c_int32 * 2)]


class PngDesc(ctypes.Structure):
    """aej_png_desc (include/aej.h): what aej_png_parse_host reads from a file's chunks"""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("bit_depth", ctypes.c_int32), ("colour_type", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("row_bytes", ctypes.c_int32), ("interlace", ctypes.c_int32), ("n_idat", ctypes.c_int32),
                ("palette_len", ctypes.c_int32), ("has_trns", ctypes.c_int32), ("idat_bytes", ctypes.c_int64),
                ("palette", ctypes.c_uint8 * 768), ("mode_chars", ctypes.c_char * 8)]

    @property
    def mode(self) -> str:
        """Pillow's mode of the opened file"""
        return self.mode_chars.decode()

    @property
    def raw_bytes(self) -> int:
        """aej_png_raw_bytes: the inflated size the file must have -- height x (1 + row_bytes), or for an interlaced file the sum over
        its non-empty passes of h_p x (1 + row_bytes_p)"""
        return int(load_library().aej_png_raw_bytes(ctypes.addressof(self)))


SIGNATURES = {
    "aej_abi_version": (_I, []),
    "aej_create": (_P, [_I, _P]),
    "aej_destroy": (None, [_P]),
    "aej_last_error": (ctypes.c_char_p, [_P]),
    "aej_synchronize": (_I, [_P]),
    "aej_set_stream": (_I, [_P, _P]),
    "aej_get_hysteresis_stats": (_I, [_P, _P]),
    "aej_set_graph_mode": (_I, [_P, _I]),
    "aej_set_sub_batches": (_I, [_P, _I]),
    "aej_set_hw_queues": (_I, [_P, _I]),
    "aej_get_schedule_host": (_I, [_P, _I, _I, _I, _P]),
    "aej_set_option": (_I, [_P, ctypes.c_char_p, _I64]),
    "aej_get_option": (_I, [_P, ctypes.c_char_p, _P]),
    "aej_test_fail_after_stage": (_I, [_P, _I]),            # include/aej_testing.h (tests only)
    "aej_encode_batch_begin": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _U64]),
    "aej_encode_batch_end": (_I, [_P]),
    "aej_get_split_calls": (ctypes.c_int64, [_P]),
    "aej_get_graph_stats": (_I, [_P, _P]),
    "aej_set_profiling": (_I, [_P, _I]),
    "aej_get_stage_ms": (_I, [_P, _P]),
    "aej_stage_name": (ctypes.c_char_p, [_I]),
    "aej_set_settings": (_I, [_P, _I, _I, _I, _P]),
    "aej_encode_plan": (_I, [_P, _I, _I, _I, ctypes.POINTER(AejPlan)]),
    "aej_encode_batch": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _U64]),
    "aej_encode_batch_u8": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _U64]),
    "aej_metrics_workspace_bytes": (_U64, [_I, _I, _I]),
    "aej_metrics_batch": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _U64]),
    "aej_color_convert": (_I, [_P, _I, _P, _P, _I64]),
    "aej_color_planes": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "aej_canny_workspace_bytes": (_U64, [_I, _I]),
    "aej_canny": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _U64]),
    "aej_set_canny_params": (_I, [_P, _P]),
    "aej_quadtree_workspace_bytes": (_U64, [_I, _I, _I, _I]),
    "aej_quadtree_capacity": (_I, [_I, _I, _I, _I, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "aej_quadtree": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _U64]),
    "aej_dct_quant_zigzag": (_I, [_P, _P, _I, _I, _I, _P, _I64, _P, _P]),
    "aej_deflate_stream_bound": (_U64, [_U64]),
    "aej_deflate_workspace_bytes": (_U64, [_P, _I, _I, _I]),
    "aej_deflate_histogram": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _U64]),
    "aej_deflate_batch": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _P, _U64, _P, _P, _U64]),
    "aej_deflate_build_tables": (_I, [_P, _P, _P]),
    "aej_deflate_bytes_workspace_bytes": (_U64, [_P, _I]),
    "aej_deflate_bytes_histogram": (_I, [_P, _P, _U64, _P, _I, _P, _P, _U64]),
    "aej_deflate_bytes_build_tables": (_I, [_P, _I, _P]),
    "aej_deflate_bytes_batch": (_I, [_P, _P, _U64, _P, _I, _P, _I, _P, _U64, _P, _P, _U64]),
    "aej_pack_u8_levels_host": (_I, [_P, _I64, _P, _I]),
    "aej_decode_workspace_bytes": (_U64, [_P, _I, _I, _I]),
    "aej_decode_batch": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _U64]),
    "aej_decode_batch_tables": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _U64]),
    "aej_requantise_batch": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _U64]),
    "aej_color_convert_inverse": (_I, [_P, _I, _P, _P, _I64]),
    "aej_leaf_positions_host": (_I64, [_P, _I64, _I, _I, _I, _P]),
    "aej_inflate_batch": (_I, [_P, _P, _P, _I, _P, _U64, _P, _P]),
    "aej_decode_headers_workspace_bytes": (_U64, [_P, _I, _I, _I]),
    "aej_decode_headers": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _U64]),
    "aej_lpips_weights_bytes": (_U64, []),
    "aej_lpips_param_count": (_I64, []),
    "aej_lpips_pack_weights_host": (_I, [_P, _I64, _P]),
    "aej_lpips_features_bytes": (_U64, [_I, _I, _I]),
    "aej_lpips_workspace_bytes": (_U64, [_I, _I, _I]),
    "aej_lpips_features": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _U64]),
    "aej_lpips_batch": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _U64]),
    "aej_jfif_workspace_bytes": (_U64, [_I, _I, _I, _I]),
    "aej_jfif_headers_host": (_I, [_I, _I, _I, _P, _I]),
    "aej_jfif_encode_batch": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _U64, _P, _P, _P, _P, _U64]),
    "aej_jfif_recon_batch": (_I, [_P, _I, _I, _I, _I, _P, _P, _U64]),
    "aej_jfif_workspace_bytes_opt": (_U64, [_I, _I, _I, _I, _I, _I]),
    "aej_jfif_headers_host_opt": (_I, [_I, _I, _I, _I, _P, _I]),
    "aej_jfif_huffman_host": (_I, [_P, _P, _P, _I]),
    "aej_jfif_encode_batch_opt": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _I, _P, _U64, _P, _P, _P, _P, _U64]),
    "aej_jfif_recon_batch_opt": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _U64]),
    "aej_jfif_workspace_bytes_prog": (_U64, [_I, _I, _I, _I, _I]),
    "aej_jfif_encode_batch_prog": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _P, _U64, _P, _P, _P, _P, _U64]),
    "aej_jfif_recon_batch_prog": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _U64]),
    "aej_test_jfif_prog_scan_host": (_I, [_P, ctypes.c_int64, _I, _I, _I, _I, _P, _U64, _P, _P, _P]),        # include/aej_testing.h (tests only)
    "aej_test_jfif_prog_scan": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _I, _P, _U64, _P, _P, _P]),         # include/aej_testing.h (tests only)
    "aej_test_jfif_seq_scan_host": (_I, [_P, ctypes.c_int64, _I, _I, _I, _I, _I, _P, _P, _U64, _P]),            # include/aej_testing.h (tests only)
    "aej_jpegdec_parse_host": (_I, [_P, _U64, _P, _P, _I]),
    "aej_jpegdec_workspace_bytes": (_U64, [_P, _P, _I]),
    "aej_jpegdec_batch": (_I, [_P, _P, _I, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegdec_sync_rounds": (_I64, [_P]),
    "aej_jpegdec_workspace_bytes_scaled": (_U64, [_P, _P, _I, _P]),
    "aej_jpegdec_batch_scaled": (_I, [_P, _P, _I, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegdec_workspace_bytes_mode": (_U64, [_P, _P, _I, _P, _P]),
    "aej_jpegdec_batch_mode": (_I, [_P, _P, _I, _P, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegdec_workspace_bytes_box": (_U64, [_P, _P, _I, _P, _P, _P]),
    "aej_jpegdec_batch_box": (_I, [_P, _P, _I, _P, _P, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegdec_box_window_host": (_I, [_P, _P, _P]),
    "aej_jpegprog_box_window_host": (_I, [_P, _P, _P]),
    "aej_jpegdec_box_stats": (_I, [_P, _P]),
    "aej_jpegdec_workspace_bytes_sbox": (_U64, [_P, _P, _I, _P, _P, _P]),
    "aej_jpegdec_batch_sbox": (_I, [_P, _P, _I, _P, _P, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegdec_sbox_window_host": (_I, [_P, _I, _P, _P]),
    "aej_jpegprog_sbox_window_host": (_I, [_P, _I, _P, _P]),
    "aej_jpegprog_workspace_bytes_sbox": (_U64, [_P, _P, _P, _I, _P, _P, _P]),
    "aej_jpegprog_batch_sbox": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegprog_workspace_bytes_box": (_U64, [_P, _P, _P, _I, _P, _P, _P]),
    "aej_jpegprog_batch_box": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegdec_parse_host_adobe": (_I, [_P, _U64, _P, _P, _P, _I, _I]),
    "aej_jpegprog_parse_host_adobe": (_I, [_P, _U64, _P, _P, _I, _P, _P, _I, _I]),
    "aej_jpegdec_workspace_bytes_adobe": (_U64, [_P, _P, _I, _P, _P, _P, _P]),
    "aej_jpegdec_batch_adobe": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegprog_workspace_bytes_adobe": (_U64, [_P, _P, _P, _I, _P, _P, _P, _P]),
    "aej_jpegprog_batch_adobe": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegprog_parse_host": (_I, [_P, _U64, _P, _P, _I, _P, _I]),
    "aej_jpegprog_workspace_bytes": (_U64, [_P, _P, _P, _I]),
    "aej_jpegprog_batch": (_I, [_P, _P, _P, _I, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegprog_workspace_bytes_scaled": (_U64, [_P, _P, _P, _I, _P]),
    "aej_jpegprog_batch_scaled": (_I, [_P, _P, _P, _I, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jpegprog_workspace_bytes_mode": (_U64, [_P, _P, _P, _I, _P, _P]),
    "aej_jpegprog_batch_mode": (_I, [_P, _P, _P, _I, _P, _P, _P, _U64, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_jfif_transcode_headers_host": (_I, [_P, _P, _P, _I, _P, _I]),
    "aej_jfif_transcode_workspace_bytes": (_U64, [_P, _P, _I, _P, _P, _I, _I]),
    "aej_jfif_transcode_batch": (_I, [_P, _P, _I, _P, _U64, _P, _P, _P, _I, _P, _U64, _P, _P, _I, _P, _U64, _P, _P, _P, _P, _P, _P, _U64]),
    "aej_jfif_many_workspace_bytes": (_U64, [_P, _P, _I, _I, _I, _I]),
    "aej_jfif_many_encode": (_I, [_P, _P, _I, _P, _U64, _I, _I, _I, _P, _U64, _P, _P, _P, _P, _P, _U64]),
    "aej_jfif_many_coefs_host": (_I64, [_I, _I, _I, _I, _P, _P, _I64]),
    "aej_jfif_headers_grey_host": (_I, [_I, _I, _I, _P, _I]),
    "aej_jfif_many_coefs_grey_host": (_I64, [_I, _I, _I, _P, _P, _I64]),
    "aej_jfif_transform_geometry_host": (_I, [_I, _I, _I, _I, _I, _I, _P]),
    "aej_jfif_transform_coefs_host": (_I64, [_I, _I, _I, _I, _I, _I, _P, _I64, _P, _I64]),
    "aej_jfif_transform_coefs_grey_host": (_I64, [_I, _I, _I, _I, _P, _I64, _P, _I64]),
    "aej_jfif_transform_headers_host": (_I, [_P, _P, _P, _I, _I, _I, _P, _I]),
    "aej_jfif_transform_workspace_bytes": (_U64, [_P, _P, _I, _P, _P, _I, _I, _P, _I]),
    "aej_jfif_transform_batch": (_I, [_P, _P, _I, _P, _U64, _P, _P, _P, _I, _P, _U64, _P, _P, _I, _P, _I, _P, _U64, _P, _P, _P, _P, _P, _P, _U64]),
    "aej_jfif_many_workspace_bytes_rst": (_U64, [_P, _P, _I, _I, _I, _I, _I, _I]),
    "aej_jfif_many_encode_rst": (_I, [_P, _P, _I, _P, _U64, _I, _I, _I, _I, _I, _P, _U64, _P, _P, _P, _P, _P, _U64]),
    "aej_jfif_transcode_workspace_bytes_rst": (_U64, [_P, _P, _I, _P, _P, _I, _I, _I, _I]),
    "aej_jfif_transcode_batch_rst": (_I, [_P, _P, _I, _P, _U64, _P, _P, _P, _I, _P, _U64, _P, _P, _I, _I, _I, _P, _U64, _P, _P, _P, _P, _P, _P, _U64]),
    "aej_jfif_transform_workspace_bytes_rst": (_U64, [_P, _P, _I, _P, _P, _I, _I, _P, _I, _I, _I]),
    "aej_jfif_transform_batch_rst": (_I, [_P, _P, _I, _P, _U64, _P, _P, _P, _I, _P, _U64, _P, _P, _I, _P, _I, _I, _I, _P, _U64, _P, _P, _P, _P, _P, _P,
                                          _U64]),
    "aej_jfif_headers_rst_host": (_I, [_I, _I, _I, _I, _I, _I, _I, _P, _I]),
    "aej_jpegdec_parse_host_440": (_I, [_P, _U64, _P, _P, _I, _I]),
    "aej_jpegprog_parse_host_440": (_I, [_P, _U64, _P, _P, _I, _P, _I, _I]),
    "aej_jfif_transform_geometry_host_440": (_I, [_I, _I, _I, _I, _I, _I, _I, _P]),
    "aej_jfif_transform_coefs_host_440": (_I64, [_I, _I, _I, _I, _I, _I, _I, _P, _I64, _P, _I64]),
    "aej_jfif_transform_headers_host_440": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I]),
    "aej_jfif_transform_workspace_bytes_440": (_U64, [_P, _P, _I, _P, _P, _I, _I, _P, _I, _I, _I, _I]),
    "aej_jfif_transform_geometry_host_cut": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "aej_jfif_transform_coefs_host_cut": (_I64, [_I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I64, _P, _I64]),
    "aej_jfif_transform_headers_host_cut": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I]),
    "aej_jfif_transform_workspace_bytes_cut": (_U64, [_P, _P, _I, _P, _P, _I, _I, _P, _I, _I, _I, _I, _P, _I]),
    "aej_jfif_transform_batch_cut": (_I, [_P, _P, _I, _P, _U64, _P, _P, _P, _I, _P, _U64, _P, _P, _I, _P, _I, _I, _I, _I, _P, _I, _P, _U64, _P, _P, _P, _P, _P,
                                          _P, _U64]),
    "aej_jfif_transform_batch_440": (_I, [_P, _P, _I, _P, _U64, _P, _P, _P, _I, _P, _U64, _P, _P, _I, _P, _I, _I, _I, _I, _P, _U64, _P, _P, _P, _P, _P,
                                          _P, _U64]),
    "aej_jfif_restart_map_host": (_I, [_I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I64, _P, _I64, _P]),
    "aej_resample_taps_host": (_I, [_I, ctypes.c_float, ctypes.c_float, _I, _I, _P, _P, _I64]),
    "aej_resample_workspace_bytes": (_U64, [_P, _P, _I]),
    "aej_resample_batch": (_I, [_P, _P, _I, _P, _U64, _P, _U64, _P, _U64]),
    "aej_resample_workspace_bytes_ch": (_U64, [_P, _P, _I, _P]),
    "aej_resample_batch_ch": (_I, [_P, _P, _I, _P, _P, _U64, _P, _U64, _P, _U64]),
    "aej_resample_workspace_bytes_win": (_U64, [_P, _P, _I, _P, _P]),
    "aej_resample_batch_win": (_I, [_P, _P, _I, _P, _P, _P, _U64, _P, _U64, _P, _U64]),
    "aej_png_parse_host": (_I, [_P, _U64, _P, _P, _I, _P, _I]),
    "aej_png_parse_host_accept": (_I, [_P, _U64, ctypes.c_uint32, _P, _P, _I, _P, _I]),
    "aej_png_raw_bytes": (_U64, [_P]),
    "aej_png_adam7_passes_host": (_I, [_I, _I, _P]),
    "aej_png_workspace_bytes": (_U64, [_P, _P, _I]),
    "aej_png_unfilter_batch": (_I, [_P, _P, _I, _P, _U64, _P, _P, _P, _P, _P, _P, _U64, _P, _P, _P, _U64]),
    "aej_png_filter_bytes": (_U64, [_I, _I, _I]),
    "aej_png_filter_batch": (_I, [_P, _P, _I, _I, _P, _U64]),
    "aej_filter_plan_host": (_I, [_I, ctypes.c_float, ctypes.c_float, _P]),
    "aej_filter_geometry_host": (_I, [_P]),
    "aej_filter_workspace_bytes": (_U64, [_P, _P, _I, _I]),
    "aej_filter_batch": (_I, [_P, _P, _I, _I, _P, _U64, _P, _U64, _P, _U64]),
    "aej_window_geometry_host": (_I, [_P]),
    "aej_window_workspace_bytes": (_U64, [_P, _P, _I]),
    "aej_window_batch": (_I, [_P, _P, _I, _P, _U64, _P, _U64, _P, _U64]),
    "aej_lut3d_prepare_host": (_I, [_P, _I64, _P]),
    "aej_lut3d_geometry_host": (_I, [_P]),
    "aej_lut3d_workspace_bytes": (_U64, [_P, _P, _I]),
    "aej_lut3d_batch": (_I, [_P, _P, _I, _P, _P, _I, _P, _U64, _P, _U64, _P, _U64]),
    "aej_warp_geometry_host": (_I, [_P]),
    "aej_warp_plan_host": (_I, [_P, _P, _P, _I64]),
    "aej_warp_workspace_bytes": (_U64, [_P, _P, _I]),
    "aej_warp_batch": (_I, [_P, _P, _I, _P, _U64, _P, _U64, _P, _U64]),
    "aej_adjust_geometry_host": (_I, [_P]),
    "aej_adjust_plan_host": (_I, [_P, _P]),
    "aej_adjust_workspace_bytes": (_U64, [_P, _P, _I]),
    "aej_adjust_batch": (_I, [_P, _P, _I, _P, _I, _P, _U64, _P, _U64, _P, _U64]),
    "aej_histogram_batch": (_I, [_P, _P, _I, _P, _U64, _P, _U64, _P, _U64]),
    "aej_compose_geometry_host": (_I, [_P]),
    "aej_compose_plan_host": (_I, [_P, _P]),
    "aej_compose_workspace_bytes": (_U64, [_P, _P, _I]),
    "aej_compose_batch": (_I, [_P, _P, _I, _P, _U64, _P, _U64, _P, _U64]),
    "aej_convert_geometry_host": (_I, [_P]),
    "aej_convert_plan_host": (_I, [_P, _P]),
    "aej_convert_workspace_bytes": (_U64, [_P, _P, _I]),
    "aej_convert_batch": (_I, [_P, _P, _I, _P, _I, _P, _U64, _P, _U64, _P, _U64]),
    "aej_test_jpegprog_coefs": (_I, [_P, _P, _P, _I, _P, _U64, _P, _I, _P, _U64, _P, _P, _U64]),             # include/aej_testing.h (tests only)
    "aej_test_jpegprog_coefs_host": (_I, [_P, _P, _P, _U64, _I, _P, _U64]),                                 # include/aej_testing.h (tests only)
    "aej_test_jpeg_adobe_pixels_host": (_I, [_P, _I64, _I, _I, _P]),                                        # include/aej_testing.h (tests only)
    "aej_test_jpeg_upsample_host": (_I, [_P, _I64, _I64, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),          # include/aej_testing.h (tests only)
    "aej_test_jpegdec_idct_host": (_I, [_P, _P, _I, _P]),                                                   # include/aej_testing.h (tests only)
    "aej_test_jpegdec_coefs_host": (_I, [_P, _P, _U64, _P, _U64]),                                          # include/aej_testing.h (tests only)
}

# status values of aej_inflate_batch / aej_decode_headers (include/aej.h AEJ_INFLATE_* / AEJ_HEADER_*)
INFLATE_STATUS = ["ok", "bad zlib header", "bad block type", "bad code lengths", "invalid literal/length or distance code",
                  "distance too far back", "stored block LEN/NLEN mismatch", "truncated stream", "output over capacity",
                  "Adler-32 mismatch", "bad stream descriptor"]
JPEGDEC_STATUS = ["ok", "truncated scan (it ends before the last MCU)", "bad Huffman code", "coefficient run past 63",
                  "DC category above 11", "restart marker out of sequence, missing or unexpected",
                  "coefficient out of range for an 8-bit JPEG (AC beyond +-1023 or DC outside -1024..1023)"]
PNG_STATUS = ["ok", "the zlib stream of its IDAT chunks does not inflate", "inflated size is not height x (1 + row bytes)",
              "a filter byte above 4"]
HEADER_STATUS = ["ok", "more leaves than the layer holds", "leaf size outside the block-size range of the header",
                 "quadtree header does not tile the layer", "coefficient count does not match the quadtree header", "bad layer descriptor"]


def load_library():
    """Load libaejpeg_hip.so and declare every signature.  Raises if the HIP extension is not built."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise AejError(
                    f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
            # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  The
            # device pointers we receive come from that runtime, so it must be the one this library binds to:
            # import torch first, then the loader resolves our NEEDED libamdhip64.so.7 to the loaded copy.
            import torch  # noqa: F401
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise AejError("no HIP device visible to PyTorch-ROCm: the adaptive-JPEG encode path runs on the GPU only")
    return torch


class Context:
    """One aej_ctx bound to a device and to ONE torch stream of it (the stream that was current when get_context()
    created it).  Everything torch does for a call -- input copies, output and workspace allocation -- happens on the stream
    current at call time, so the library must enqueue on that same stream; get_context() therefore hands out one context per
    (device, stream), each with its own workspace, and `check_stream()` refuses a context used under another stream."""

    def __init__(self, device=0):
        self.torch = _torch()
        self.lib = load_library()
        self.device = self.torch.device("cuda", device if isinstance(device, int) else device.index or 0)
        self.stream = self.torch.cuda.current_stream(self.device).cuda_stream
        self.handle = self.lib.aej_create(self.device.index, ctypes.c_void_p(self.stream))
        if not self.handle:
            raise AejError(self.lib.aej_last_error(None).decode())
        self.check(self.lib.aej_set_hw_queues(self.handle, _hw_queues))
        self.settings_key = None
        self._ws = None

    def check_stream(self):
        cur = self.torch.cuda.current_stream(self.device).cuda_stream
        if cur != self.stream:
            raise AejError(f"context bound to stream {self.stream:#x} used while torch's current stream is {cur:#x}: "
                           "obtain the context with get_context() inside the `torch.cuda.stream(...)` block")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.aej_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # -- helpers
    def check(self, rc):
        if rc == 0:
            return
        msg = self.lib.aej_last_error(self.handle).decode()
        if rc == AEJ_ERR_ARG:
            raise ValueError(msg)
        if rc == AEJ_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        raise AejError(f"aej error {rc}: {msg}")

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    def workspace(self, nbytes):
        """Scratch of at least `nbytes`, reused across calls.  It is allocated on, and only ever used by kernels of, this
        context's stream, so dropping the old tensor when a larger one is needed is safe: torch's caching allocator hands a
        freed block only to later work of the same stream."""
        self.check_stream()
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = self.torch.empty(int(nbytes), dtype=self.torch.uint8, device=self.device)
        return self._ws

    def pinned(self, nbytes):
        """Page-locked host staging buffer of at least `nbytes`, reused across calls (device-to-host copies into pageable memory run at
        a third of the PCIe rate).  Its contents are only valid until the next call that uses it."""
        if getattr(self, "_pinned", None) is None or self._pinned.numel() < nbytes:
            self._pinned = None
            self._pinned = self.torch.empty(int(max(nbytes, 1 << 20)), dtype=self.torch.uint8, pin_memory=True)
        return self._pinned

    def hysteresis_stats(self):
        """-> dict(calls, queued): whole-path calls on this context, tiles that went through the device-side hysteresis work queue
        in the last completed call (include/aej.h)."""
        buf = (ctypes.c_int64 * 4)()      # (4: round 3 libraries, loaded through AEJ_LIBRARY for A / B runs, wrote four)
        self.check(self.lib.aej_get_hysteresis_stats(self.handle, ctypes.cast(buf, ctypes.c_void_p)))
        return {"calls": int(buf[0]), "queued": int(buf[1])}

    def set_canny_params(self, params=None):
        """aej_set_canny_params: (low_ratio, high_ratio, clip_limit, sigma_color, sigma_space, use_l2) or None for the defaults"""
        if params is None:
            self.check(self.lib.aej_set_canny_params(self.handle, None))
            return
        lo, hi, clip, sc, ss, l2 = params
        v = CannyParams(float(lo), float(hi), float(clip), float(sc), float(ss), 1 if l2 else 0)
        self.check(self.lib.aej_set_canny_params(self.handle, ctypes.cast(ctypes.pointer(v), ctypes.c_void_p)))

    def set_sub_batches(self, n):
        """0 = automatic (default), 1 = never split a call, 2..8 = that many sub-batches on private streams (include/aej.h)"""
        self.check(self.lib.aej_set_sub_batches(self.handle, int(n)))

    def schedule(self, batch, H, W):
        """-> dict(hw_queues, sub_batches, limited): what the automatic mode would do for this call (aej_get_schedule_host)"""
        buf = (ctypes.c_int32 * 4)()
        self.check(self.lib.aej_get_schedule_host(self.handle, int(batch), int(H), int(W), ctypes.cast(buf, ctypes.c_void_p)))
        return {"hw_queues": int(buf[0]), "sub_batches": int(buf[1]), "limited_by_hw_queues": bool(buf[2]), "hw_queues_source": _hw_queues_source}

    def set_option(self, name, value):
        """aej_set_option: the library's tuning / A-B choices (table in include/aej.h); it reads no environment variable."""
        self.check(self.lib.aej_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name):
        v = ctypes.c_int64()
        self.check(self.lib.aej_get_option(self.handle, name.encode(), ctypes.cast(ctypes.pointer(v), ctypes.c_void_p)))
        return int(v.value)

    def split_calls(self):
        return int(self.lib.aej_get_split_calls(self.handle))

    def set_graph_mode(self, mode):
        """0 = never replay a captured hipGraph (default), 1 = automatic (small calls), 2 = whenever possible (include/aej.h)"""
        self.check(self.lib.aej_set_graph_mode(self.handle, int(mode)))

    def graph_stats(self):
        buf = (ctypes.c_int64 * 3)()
        self.check(self.lib.aej_get_graph_stats(self.handle, ctypes.cast(buf, ctypes.c_void_p)))
        return {"launches": int(buf[0]), "captures": int(buf[1]), "cached": int(buf[2])}

    def to_device(self, arr, dtype):
        t = self.torch
        if isinstance(arr, t.Tensor):
            return arr.to(device=self.device, dtype=dtype).contiguous()
        return t.from_numpy(np.ascontiguousarray(arr)).to(device=self.device, dtype=dtype).contiguous()

    def set_settings(self, space, bmin, bmax, qmats):
        """qmats: int32 numpy array laid out [layer][size][s*s] (see include/aej.h)."""
        key = (space, bmin, bmax, qmats.tobytes())
        if key == self.settings_key:
            return
        q = np.ascontiguousarray(qmats, dtype=np.int32)
        self.check(self.lib.aej_set_settings(self.handle, SPACE_IDS[space], bmin, bmax, q.ctypes.data_as(ctypes.c_void_p)))
        self.settings_key = key

    N_STAGES = 18

    def set_profiling(self, on):
        self.check(self.lib.aej_set_profiling(self.handle, 1 if on else 0))

    def stage_ms(self):
        """-> {stage name: milliseconds} for the last aej_encode_batch call (profiling must be on)."""
        buf = (ctypes.c_float * self.N_STAGES)()
        self.check(self.lib.aej_get_stage_ms(self.handle, ctypes.cast(buf, ctypes.c_void_p)))
        return {self.lib.aej_stage_name(i).decode(): float(buf[i]) for i in range(self.N_STAGES)}

    def plan(self, batch, H, W):
        p = AejPlan()
        self.check(self.lib.aej_encode_plan(self.handle, batch, H, W, ctypes.byref(p)))
        return p


_contexts = {}


def get_context(device=0):
    """The context of (device, torch's current stream on it); created on first use."""
    idx = device if isinstance(device, int) else (device.index or 0)
    torch = _torch()
    key = (idx, torch.cuda.current_stream(torch.device("cuda", idx)).cuda_stream)
    ctx = _contexts.get(key)
    if ctx is None:
        ctx = _contexts[key] = Context(idx)
    return ctx


def release_context(ctx):
    """Destroy a context handed out by get_context() and forget it: the library's state for it is freed (aej_destroy) and its
    workspace goes back to torch's allocator.  For callers that walk through many streams or batch shapes (bench.py's other_configs)."""
    for key, known in list(_contexts.items()):
        if known is ctx:
            del _contexts[key]
    ctx._ws = None
    ctx._pinned = None
    ctx._in_flight = None
    if getattr(ctx, "handle", None):
        ctx.lib.aej_destroy(ctx.handle)
        ctx.handle = None
