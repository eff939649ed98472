"""ore — MI355X-native (gfx950) fp32 ONNX op executor for the op path of
jackperlo/onnx-rusty-inference-engine.  Python host mirror over the C ABI in include/ore.h;
all compute runs as HIP kernels in lib/libore.so (no CPU fallback)."""
from ._lib import (CONV_ALGO_DIRECT, CONV_ALGO_WINOGRAD, FUSE_ALIAS, FUSE_ALL, FUSE_CONCAT, FUSE_CONCAT_POOL,  # noqa: F401
                   FUSE_CONV_POOL, FUSE_CONV_RELU, FUSE_EAGER, FUSE_FIRE, FUSE_FIRE_POOL, FUSE_FIRST_SQUEEZE,
                   FUSE_POOL_SQUEEZE, FUSE_CONV_GAP, FUSE_POOL_EXPAND, KEEP_VALUES, LIB_PATH, LOAD_F16, LOAD_NO_WINOGRAD, OreError,
                   ABI_VERSION, PRE_REVERSE_CHANNELS, FILTER_BILINEAR, FILTER_BILINEAR_AA, FILTER_BICUBIC, FILTER_BICUBIC_AA, CUBIC_AA_MAX_RATIO, AA_MAX_RATIO, AA_MAX_TAPS,
                   YUV_BT601, YUV_BT709, YUV_BT601_FULL, IMAGE_INTERLEAVED, IMAGE_NV12, IMAGE_YUV, YUV_FORMATS, IMAGE_FLIP_H, MAX_VIEWS,
                   CAM_BOX_MAX_MAP, CAM_BOX_MAX_SIDE, load)
from .engine import (Context, ImageList, Model, Nv12ImageList, YuvImageList, add, center_crop_geometry, class_maps, concatenation, conv_out_shape, convolution, drop_out,  # noqa: F401
                     global_average_pool, inference, max_pool, mul, multi_crop_geometries, nv12_to_rgb, pool_out_shape, preprocess_list_u8, preprocess_resize_u8,
                     preprocess_u8, relu, reshape, resize_aa_taps, resize_cubic_taps, resize_taps, softmax, topk, topk_mean, yuv_planes_to_rgb, yuv_to_rgb,
                     apply_orientation, orient_geometry, oriented_hw, rotation_orientation,
                     box_to_source, cam_box_reference, cam_boxes, upsample_maps)

__version__ = "0.1.0"
