"""ctypes loader for the in-tree C-ABI library `lib/libore.so` (include/ore.h).

The library is the product: there is no CPU fallback.  If it is missing the import of any
entry point raises, so a GPU run never silently computes through something else.
"""
from __future__ import annotations

import ctypes
import os

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ORE_LIB selects another build of the same library (tools/build_exp.sh A/B variants)
LIB_PATH = os.environ.get("ORE_LIB") or os.path.join(PKG_ROOT, "lib", "libore.so")

ORE_OK = 0
STATUS_NAMES = {0: "ORE_OK", 1: "ORE_ERR_INVALID", 2: "ORE_ERR_UNSUPPORTED", 3: "ORE_ERR_HIP",
                4: "ORE_ERR_OOM", 5: "ORE_ERR_PARSE"}

# ore_model_set_fusion flags (include/ore.h)
FUSE_CONV_RELU, FUSE_CONCAT, FUSE_ALIAS, KEEP_VALUES, FUSE_CONV_POOL = 1, 2, 4, 8, 32
FUSE_FIRE, FUSE_CONCAT_POOL, FUSE_FIRE_POOL, FUSE_FIRST_SQUEEZE, FUSE_POOL_SQUEEZE = 64, 128, 256, 512, 1024
FUSE_CONV_GAP, FUSE_POOL_EXPAND = 4096, 8192
FUSE_EAGER = 2048  # tests: every eligible fusion regardless of the size heuristics
FUSE_ALL = 14311
LOAD_F16 = 1  # ore_model_load_ex flag: the fp16 variant
LOAD_NO_WINOGRAD = 4  # ore_model_load_ex flag: 3x3 stride-1 convs on the direct kernels only
LOAD_RETIRED_MASK = 10  # ABI 1's LOAD_X3 / LOAD_X3_ALL: rejected (ORE_ERR_UNSUPPORTED) since ABI 2
ABI_VERSION = 2  # ORE_ABI_VERSION this binding was written against
CONV_ALGO_DIRECT, CONV_ALGO_WINOGRAD = 0, 1  # ore_ctx_set_conv_algo (per-op ore_conv2d_f32)
PRE_REVERSE_CHANNELS = 1  # ore_preprocess_u8 / _resize_u8 / ore_model_set_input_norm flag: RGB <-> BGR
FILTER_BILINEAR, FILTER_BILINEAR_AA = 0, 1  # ore_resize_filter (the _ex resize entries)
FILTER_CUBIC_BIT, FILTER_BICUBIC, FILTER_BICUBIC_AA = 256, 256, 257  # ORE_FILTER_BICUBIC*: values of the filter word beside the enum
CUBIC_AA_MAX_RATIO = 16  # ORE_CUBIC_AA_MAX_RATIO: the antialiased cubic filter's shrink limit
AA_MAX_RATIO, AA_MAX_TAPS = 32, 64  # ORE_AA_MAX_RATIO / ORE_AA_MAX_TAPS: the antialiased filter's shrink limit and taps per axis
YUV_BT601, YUV_BT709, YUV_BT601_FULL = 0, 1, 2  # ore_yuv_matrix (ore_yuv_to_rgb, the NV12 image lists)
YUV_MATRICES = {"bt601": YUV_BT601, "bt709": YUV_BT709, "bt601_full": YUV_BT601_FULL}
IMAGE_INTERLEAVED, IMAGE_NV12, IMAGE_YUV = 0, 1, 2  # ore_image_format (ore_image_list_format)
# ore_yuv_format: the per-descriptor plane layout of a YUV image list (ore_image_yuv.format)
YUV_FORMATS = {"nv12": 0, "yuyv": 1, "i444": 2, "i440": 3, "i422": 4, "i420": 5, "i411": 6, "gray": 7}
IMAGE_FLIP_H = 1  # ORE_IMAGE_FLIP_H: the per-descriptor flag of ore_image_list_set_ex / _set_nv12_ex
MAX_VIEWS = 64  # ORE_MAX_VIEWS (ore_topk_mean_f32, ore_model_set_views)
CAM_BOX_MAX_MAP = 4096  # ORE_CAM_BOX_MAX_MAP (ore_cam_boxes_f32: Hm * Wm)
CAM_BOX_MAX_SIDE = 512  # ORE_CAM_BOX_MAX_SIDE (ore_cam_boxes_f32: H, W)
PAD = {"NOTSET": 0, "NOT_SET": 0, "SAME_UPPER": 1, "SAME_LOWER": 2, "VALID": 3}

# every symbol include/ore.h declares (checked by tests/test_abi.py on CPU)
EXPORTED = [
    "ore_abi_version", "ore_ctx_create", "ore_ctx_destroy", "ore_ctx_set_stream", "ore_ctx_get_stream",
    "ore_ctx_set_conv_algo", "ore_ctx_set_conv_tile", "ore_ctx_set_pool_variant", "ore_sync", "ore_last_error", "ore_malloc", "ore_free", "ore_upload", "ore_download",
    "ore_conv_out_shape", "ore_pool_out_shape", "ore_conv2d_f32", "ore_maxpool2d_f32", "ore_relu_f32",
    "ore_add_f32", "ore_softmax_f32", "ore_matmul_f32", "ore_gap_f32", "ore_concat_f32", "ore_dropout_f32",
    "ore_reshape", "ore_preprocess_u8", "ore_model_set_input_norm", "ore_model_run_u8", "ore_model_graph_capture_u8",
    "ore_resize_taps", "ore_preprocess_resize_u8", "ore_model_set_input_resize",
    "ore_image_check", "ore_image_list_create", "ore_image_list_destroy", "ore_image_list_set", "ore_image_list_count",
    "ore_resize_aa_taps", "ore_preprocess_resize_u8_ex", "ore_image_check_ex", "ore_image_list_create_ex", "ore_image_list_filter",
    "ore_model_set_input_resize_ex", "ore_ctx_set_resize_variant", "ore_resize_cubic_taps",
    "ore_yuv_to_rgb", "ore_image_check_nv12", "ore_image_list_create_nv12", "ore_image_list_set_nv12", "ore_image_list_format",
    "ore_image_list_matrix",
    "ore_image_check_yuv", "ore_image_list_create_yuv", "ore_image_list_set_yuv", "ore_image_list_set_yuv_ex",
    "ore_preprocess_list_u8", "ore_model_run_u8_list", "ore_model_classify_u8_list", "ore_model_graph_capture_u8_list",
    "ore_model_graph_capture_classify_u8_list",
    "ore_topk_f32", "ore_model_set_topk", "ore_model_classify", "ore_model_classify_u8",
    "ore_model_graph_capture_classify", "ore_model_graph_capture_classify_u8",
    "ore_image_list_set_ex", "ore_image_list_set_nv12_ex", "ore_topk_mean_f32", "ore_model_set_views",
    "ore_orient_geometry", "ore_image_check_oriented", "ore_image_check_nv12_oriented", "ore_image_check_yuv_oriented",
    "ore_image_list_set_oriented", "ore_image_list_set_nv12_oriented", "ore_image_list_set_yuv_oriented", "ore_image_list_oriented",
    "ore_model_parse", "ore_model_load", "ore_model_load_ex", "ore_model_destroy", "ore_model_set_fusion", "ore_model_input_dims",
    "ore_model_output_elems", "ore_model_run", "ore_model_read_value", "ore_model_autotune",
    "ore_model_step_tile", "ore_model_set_step_tile", "ore_model_step_mfma_flops", "ore_model_set_streams",
    "ore_model_graph_capture", "ore_model_graph_launch", "ore_model_enable_timing",
    "ore_model_step_count", "ore_model_step_info", "ore_model_step_times", "ore_model_run_batch",
    "ore_ctx_set_alloc_fill", "ore_model_fill_scratch", "ore_model_scratch_info",
    "ore_class_maps_f32", "ore_model_cam_dims", "ore_model_set_cam",
    "ore_upsample_maps_f32", "ore_cam_boxes_f32", "ore_cam_box_host", "ore_model_set_cam_boxes",
]


class OreError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class Tensor(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("ndim", ctypes.c_int32), ("dims", ctypes.c_int64 * 4),
                ("nstride", ctypes.c_int64)]


class Resize(ctypes.Structure):
    """ore_resize: the source image resized to rh x rw, of which the window at (top, left) is produced."""
    _fields_ = [("rh", ctypes.c_int64), ("rw", ctypes.c_int64), ("top", ctypes.c_int64), ("left", ctypes.c_int64)]


class ImageU8(ctypes.Structure):
    """ore_image_u8: one image of an image list: a DEVICE pointer, its size, the bytes from a row to the next
    (0: dense) and its own geometry."""
    _fields_ = [("data", ctypes.c_void_p), ("hs", ctypes.c_int64), ("ws", ctypes.c_int64), ("row_stride", ctypes.c_int64),
                ("g", Resize)]


class ImageNv12(ctypes.Structure):
    """ore_image_nv12: one frame of an NV12 image list: DEVICE pointers to its Y and UV planes, its size, the bytes
    from a row to the next of each plane (0: dense) and its own geometry."""
    _fields_ = [("y", ctypes.c_void_p), ("uv", ctypes.c_void_p), ("hs", ctypes.c_int64), ("ws", ctypes.c_int64),
                ("y_stride", ctypes.c_int64), ("uv_stride", ctypes.c_int64), ("g", Resize)]


class ImageYuv(ctypes.Structure):
    """ore_image_yuv: one frame of a YUV image list: DEVICE pointers to up to three planes (unused ones null), the
    bytes from a row to the next of each (0: dense), its size, its ore_yuv_format and its own geometry."""
    _fields_ = [("plane", ctypes.c_void_p * 3), ("stride", ctypes.c_int64 * 3), ("hs", ctypes.c_int64), ("ws", ctypes.c_int64),
                ("format", ctypes.c_int32), ("reserved", ctypes.c_int32), ("g", Resize)]


assert ctypes.sizeof(ImageYuv) == 104


class ConvAttrs(ctypes.Structure):
    _fields_ = [("auto_pad", ctypes.c_int32), ("n_pads", ctypes.c_int32), ("pads", ctypes.c_int64 * 4),
                ("strides", ctypes.c_int64 * 2), ("dilations", ctypes.c_int64 * 2), ("group", ctypes.c_int64),
                ("fuse_relu", ctypes.c_int32)]


class PoolAttrs(ctypes.Structure):
    _fields_ = [("auto_pad", ctypes.c_int32), ("n_pads", ctypes.c_int32), ("pads", ctypes.c_int64 * 4),
                ("kernel", ctypes.c_int64 * 2), ("strides", ctypes.c_int64 * 2)]


_lib = None


def load():
    """Load libore.so (raises if it has not been built: no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} not built; run `make -C {PKG_ROOT}` (or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, cs = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_char_p
    T = ctypes.POINTER(Tensor)
    I64P = ctypes.POINTER(ctypes.c_int64)
    F32P = ctypes.POINTER(ctypes.c_float)
    U8P = ctypes.POINTER(ctypes.c_uint8)
    sig = {
        "ore_abi_version": (i32, []),
        "ore_ctx_create": (i32, [i32, ctypes.POINTER(vp)]),
        "ore_ctx_destroy": (i32, [vp]),
        "ore_ctx_set_stream": (i32, [vp, vp]),
        "ore_ctx_get_stream": (vp, [vp]),
        "ore_ctx_set_conv_algo": (i32, [vp, i32]),
        "ore_ctx_set_conv_tile": (i32, [vp, i32]),
        "ore_ctx_set_pool_variant": (i32, [vp, i32]),
        "ore_sync": (i32, [vp]),
        "ore_last_error": (cs, [vp]),
        "ore_malloc": (i32, [vp, ctypes.c_size_t, ctypes.POINTER(vp)]),
        "ore_free": (i32, [vp, vp]),
        "ore_upload": (i32, [vp, vp, vp, ctypes.c_size_t]),
        "ore_download": (i32, [vp, vp, vp, ctypes.c_size_t]),
        "ore_conv_out_shape": (i32, [I64P, I64P, ctypes.POINTER(ConvAttrs), I64P, I64P]),
        "ore_pool_out_shape": (i32, [I64P, ctypes.POINTER(PoolAttrs), I64P, I64P]),
        "ore_conv2d_f32": (i32, [vp, T, T, T, ctypes.POINTER(ConvAttrs), T]),
        "ore_maxpool2d_f32": (i32, [vp, T, ctypes.POINTER(PoolAttrs), T]),
        "ore_relu_f32": (i32, [vp, T, T]),
        "ore_add_f32": (i32, [vp, T, T, T]),
        "ore_softmax_f32": (i32, [vp, T, T]),
        "ore_matmul_f32": (i32, [vp, T, T, T]),
        "ore_gap_f32": (i32, [vp, T, T]),
        "ore_concat_f32": (i32, [vp, T, T, i64, T]),
        "ore_dropout_f32": (i32, [vp, T, T]),
        "ore_reshape": (i32, [T, I64P, i32, T]),
        "ore_preprocess_u8": (i32, [vp, vp, i64, i64, i64, i64, F32P, F32P, i32, T]),
        "ore_model_set_input_norm": (i32, [vp, F32P, F32P, i32, i32]),
        "ore_model_run_u8": (i32, [vp, vp, i64, vp]),
        "ore_model_graph_capture_u8": (i32, [vp, vp, i64, vp]),
        "ore_resize_taps": (i32, [i64, i64, i64, i64, vp, vp, vp]),
        "ore_preprocess_resize_u8": (i32, [vp, vp, i64, i64, i64, i64, ctypes.POINTER(Resize), F32P, F32P, i32, T]),
        "ore_model_set_input_resize": (i32, [vp, i64, i64, ctypes.POINTER(Resize)]),
        "ore_image_check": (i32, [ctypes.POINTER(ImageU8), i64, i64, i64, i64, I64P]),
        "ore_image_list_create": (i32, [vp, i64, i64, i64, i64, ctypes.POINTER(vp)]),
        "ore_image_list_destroy": (i32, [vp]),
        "ore_image_list_set": (i32, [vp, ctypes.POINTER(ImageU8), i64]),
        "ore_image_list_count": (i64, [vp]),
        "ore_preprocess_list_u8": (i32, [vp, vp, F32P, F32P, i32, T]),
        "ore_resize_aa_taps": (i32, [i64, i64, i64, i64, vp, vp, vp, vp]),
        "ore_resize_cubic_taps": (i32, [i64, i64, i64, i64, i32, vp, vp, vp, vp]),
        "ore_preprocess_resize_u8_ex": (i32, [vp, vp, i64, i64, i64, i64, ctypes.POINTER(Resize), i32, F32P, F32P, i32, T]),
        "ore_image_check_ex": (i32, [ctypes.POINTER(ImageU8), i64, i64, i64, i64, i32, I64P]),
        "ore_image_list_create_ex": (i32, [vp, i64, i64, i64, i64, i32, ctypes.POINTER(vp)]),
        "ore_image_list_filter": (i32, [vp]),
        "ore_yuv_to_rgb": (i32, [i32, vp, vp, vp, i64, vp]),
        "ore_image_check_nv12": (i32, [ctypes.POINTER(ImageNv12), i64, i64, i64, i32, I64P]),
        "ore_image_list_create_nv12": (i32, [vp, i64, i64, i64, i32, i32, ctypes.POINTER(vp)]),
        "ore_image_list_set_nv12": (i32, [vp, ctypes.POINTER(ImageNv12), i64]),
        "ore_image_check_yuv": (i32, [ctypes.POINTER(ImageYuv), i64, i64, i64, i32, I64P]),
        "ore_image_list_create_yuv": (i32, [vp, i64, i64, i64, i32, i32, ctypes.POINTER(vp)]),
        "ore_image_list_set_yuv": (i32, [vp, ctypes.POINTER(ImageYuv), i64]),
        "ore_image_list_set_yuv_ex": (i32, [vp, ctypes.POINTER(ImageYuv), ctypes.POINTER(ctypes.c_uint32), i64]),
        "ore_image_list_format": (i32, [vp]),
        "ore_image_list_matrix": (i32, [vp]),
        "ore_model_set_input_resize_ex": (i32, [vp, i64, i64, ctypes.POINTER(Resize), i32]),
        "ore_ctx_set_resize_variant": (i32, [vp, i32]),
        "ore_model_run_u8_list": (i32, [vp, vp, vp]),
        "ore_model_classify_u8_list": (i32, [vp, vp, vp, vp]),
        "ore_model_graph_capture_u8_list": (i32, [vp, vp, vp]),
        "ore_model_graph_capture_classify_u8_list": (i32, [vp, vp, vp, vp]),
        "ore_topk_f32": (i32, [vp, T, i32, vp, vp]),
        "ore_model_set_topk": (i32, [vp, i32]),
        "ore_model_classify": (i32, [vp, vp, i64, vp, vp]),
        "ore_model_classify_u8": (i32, [vp, vp, i64, vp, vp]),
        "ore_model_graph_capture_classify": (i32, [vp, vp, i64, vp, vp]),
        "ore_model_graph_capture_classify_u8": (i32, [vp, vp, i64, vp, vp]),
        "ore_image_list_set_ex": (i32, [vp, ctypes.POINTER(ImageU8), ctypes.POINTER(ctypes.c_uint32), i64]),
        "ore_image_list_set_nv12_ex": (i32, [vp, ctypes.POINTER(ImageNv12), ctypes.POINTER(ctypes.c_uint32), i64]),
        "ore_orient_geometry": (i32, [i32, ctypes.POINTER(Resize), i64, i64, ctypes.POINTER(Resize), I64P, I64P,
                                      ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "ore_image_check_oriented": (i32, [ctypes.POINTER(ImageU8), i64, i64, i64, i64, i32, U8P, I64P]),
        "ore_image_check_nv12_oriented": (i32, [ctypes.POINTER(ImageNv12), i64, i64, i64, i32, U8P, I64P]),
        "ore_image_check_yuv_oriented": (i32, [ctypes.POINTER(ImageYuv), i64, i64, i64, i32, U8P, I64P]),
        "ore_image_list_set_oriented": (i32, [vp, ctypes.POINTER(ImageU8), ctypes.POINTER(ctypes.c_uint32), U8P, i64]),
        "ore_image_list_set_nv12_oriented": (i32, [vp, ctypes.POINTER(ImageNv12), ctypes.POINTER(ctypes.c_uint32), U8P, i64]),
        "ore_image_list_set_yuv_oriented": (i32, [vp, ctypes.POINTER(ImageYuv), ctypes.POINTER(ctypes.c_uint32), U8P, i64]),
        "ore_image_list_oriented": (i32, [vp]),
        "ore_topk_mean_f32": (i32, [vp, T, i32, i32, vp, vp]),
        "ore_model_set_views": (i32, [vp, i32]),
        "ore_class_maps_f32": (i32, [vp, T, vp, vp, i64, i32, vp, i32, i32, vp]),
        "ore_model_cam_dims": (i32, [vp, I64P]),
        "ore_model_set_cam": (i32, [vp, vp, i64]),
        "ore_upsample_maps_f32": (i32, [vp, vp, i64, i64, i64, i64, i64, vp]),
        "ore_cam_boxes_f32": (i32, [vp, vp, i64, i64, i64, i64, i64, ctypes.c_float, vp, vp]),
        "ore_cam_box_host": (i32, [vp, i64, i64, i64, i64, ctypes.c_float, vp, vp]),
        "ore_model_set_cam_boxes": (i32, [vp, vp, vp, i64, ctypes.c_float]),
        "ore_model_parse": (i32, [ctypes.c_char_p, ctypes.c_size_t]),
        "ore_model_load": (i32, [vp, ctypes.c_char_p, ctypes.c_size_t, i64, ctypes.POINTER(vp)]),
        "ore_model_load_ex": (i32, [vp, ctypes.c_char_p, ctypes.c_size_t, i64, i32, ctypes.POINTER(vp)]),
        "ore_model_destroy": (i32, [vp]),
        "ore_model_set_fusion": (i32, [vp, i32]),
        "ore_model_input_dims": (i32, [vp, I64P]),
        "ore_model_output_elems": (i32, [vp, I64P]),
        "ore_model_run": (i32, [vp, vp, i64, vp]),
        "ore_model_read_value": (i32, [vp, cs, vp, ctypes.c_size_t, I64P, ctypes.POINTER(i32)]),
        "ore_model_enable_timing": (i32, [vp, i32]),
        "ore_model_set_streams": (i32, [vp, i32]),
        "ore_model_autotune": (i32, [vp, vp, i64, vp, i32]),
        "ore_model_step_tile": (i32, [vp, i32]),
        "ore_model_set_step_tile": (i32, [vp, i32, i32]),
        "ore_model_step_mfma_flops": (i32, [vp, i32, ctypes.POINTER(ctypes.c_double)]),
        "ore_model_graph_capture": (i32, [vp, vp, i64, vp]),
        "ore_model_graph_launch": (i32, [vp]),
        "ore_model_step_count": (i32, [vp]),
        "ore_model_run_batch": (i64, [vp]),
        "ore_model_step_info": (i32, [vp, i32, ctypes.POINTER(cs), ctypes.POINTER(cs),
                                      ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
        "ore_model_step_times": (i32, [vp, ctypes.POINTER(ctypes.c_float), i32]),
        "ore_ctx_set_alloc_fill": (i32, [vp, i32, ctypes.c_uint32]),
        "ore_model_fill_scratch": (i32, [vp, ctypes.c_uint32]),
        "ore_model_scratch_info": (i32, [vp, i32, ctypes.POINTER(cs), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status: int, ctx=None):
    if status != ORE_OK:
        msg = load().ore_last_error(ctx)
        raise OreError(status, msg.decode() if msg else "")
