"""Host-side mirror of the reference's operator interface over the C ABI (include/ore.h).

Names follow the reference: one function per `node_inference` arm
(/root/reference/src/inference_engine/model_inference.rs:137-161) —
`convolution`, `max_pool`, `relu`, `add`, `softmax`, `mul`, `global_average_pool`,
`concatenation`, `drop_out`, `reshape` — and `inference()` for the graph walker
(model_inference.rs:29-120).  Tensors are torch CUDA tensors (PyTorch is only the device
memory / stream plumbing); every computation is a HIP kernel in libore.so.  Errors the
reference reports by panicking raise `OreError`.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (LOAD_F16, LOAD_NO_WINOGRAD, PRE_REVERSE_CHANNELS, ConvAttrs, OreError, PoolAttrs, Resize,
                   Tensor, check, load)

__all__ = ["Context", "Model", "OreError", "convolution", "max_pool", "relu", "add", "softmax", "mul",
           "global_average_pool", "concatenation", "drop_out", "reshape", "preprocess_u8", "preprocess_resize_u8", "ImageList", "Nv12ImageList", "YuvImageList", "yuv_to_rgb", "nv12_to_rgb", "yuv_planes_to_rgb", "preprocess_list_u8", "resize_taps", "resize_aa_taps", "resize_cubic_taps", "center_crop_geometry", "topk", "inference",
           "conv_out_shape", "pool_out_shape"]


def _torch():
    import torch
    return torch


class Context:
    """One device + one HIP stream (ore_ctx).  Not thread-safe; one per host thread/device."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        L = load()
        h = ctypes.c_void_p()
        check(L.ore_ctx_create(int(device), ctypes.byref(h)))
        self.h = h
        self.device = device
        if use_torch_stream:
            torch = _torch()
            self.set_stream(torch.cuda.current_stream(device).cuda_stream)

    def set_stream(self, stream_ptr: Optional[int]):
        check(load().ore_ctx_set_stream(self.h, ctypes.c_void_p(stream_ptr or None)), self.h)

    def set_conv_algo(self, algo: int):
        """ore_ctx_set_conv_algo: the per-op convolution()'s algorithm (CONV_ALGO_DIRECT, the
        reference's k order; CONV_ALGO_WINOGRAD, F(2x2, 3x3) on eligible 3x3 stride-1 convs)."""
        check(load().ore_ctx_set_conv_algo(self.h, int(algo)), self.h)

    def set_conv_tile(self, tile: int = -1):
        """ore_ctx_set_conv_tile: force a tile id on every conv planned on this context afterwards
        (per-op calls and models loaded later); -1 = the per-layer heuristic.  Results do not depend
        on it (parity tests sweep it)."""
        check(load().ore_ctx_set_conv_tile(self.h, int(tile)), self.h)

    def set_pool_variant(self, variant: int = 0):
        """ore_ctx_set_pool_variant: force a MaxPool kernel (2 direct, 3 column strip, 4 plane-staged,
        5 chunk-staged; 0 = by layout)."""
        check(load().ore_ctx_set_pool_variant(self.h, int(variant)), self.h)

    def set_resize_variant(self, variant: int = 0):
        """ore_ctx_set_resize_variant: force a kernel of the antialiased resize (1 one thread per output
        pixel; 0 = by geometry, which is that kernel today).  Results do not depend on it."""
        check(load().ore_ctx_set_resize_variant(self.h, int(variant)), self.h)

    def set_alloc_fill(self, on: bool, pattern: int = 0):
        """ore_ctx_set_alloc_fill (debug): while on, every device allocation the library makes for itself on
        this context is filled with the 32-bit pattern before anything else touches it."""
        check(load().ore_ctx_set_alloc_fill(self.h, 1 if on else 0, int(pattern) & 0xFFFFFFFF), self.h)

    @property
    def stream(self) -> int:
        return load().ore_ctx_get_stream(self.h) or 0

    def sync(self):
        check(load().ore_sync(self.h), self.h)

    def close(self):
        if getattr(self, "h", None):
            load().ore_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _desc(t, ndim: Optional[int] = None) -> Tensor:
    torch = _torch()
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise OreError(1, "expected a float32 CUDA tensor")
    if not t.is_contiguous():
        raise OreError(1, "expected a contiguous tensor")
    d = Tensor()
    d.data = t.data_ptr()
    d.ndim = t.dim() if ndim is None else ndim
    for i, s in enumerate(t.shape):
        d.dims[i] = int(s)
    d.nstride = 0
    return d


def _conv_attrs(auto_pad, pads, strides, dilations, group, fuse_relu) -> ConvAttrs:
    a = ConvAttrs()
    a.auto_pad = _lib.PAD[auto_pad]
    pads = list(pads) if pads is not None else []
    a.n_pads = min(len(pads), 4)
    for i in range(a.n_pads):
        a.pads[i] = int(pads[i])
    a.strides[0], a.strides[1] = int(strides[0]), int(strides[1])
    a.dilations[0], a.dilations[1] = int(dilations[0]), int(dilations[1])
    a.group = int(group)
    a.fuse_relu = 1 if fuse_relu else 0
    return a


def _pool_attrs(kernel_shape, strides, auto_pad, pads) -> PoolAttrs:
    a = PoolAttrs()
    a.auto_pad = _lib.PAD[auto_pad]
    pads = list(pads) if pads is not None else []
    a.n_pads = min(len(pads), 4)
    for i in range(a.n_pads):
        a.pads[i] = int(pads[i])
    a.kernel[0], a.kernel[1] = int(kernel_shape[0]), int(kernel_shape[1])
    a.strides[0], a.strides[1] = int(strides[0]), int(strides[1])
    return a


def conv_out_shape(x_shape, w_shape, auto_pad="VALID", pads=None, strides=(1, 1), dilations=(1, 1), group=1):
    """-> (y_dims, pads_tlbr) as the reference resolves them (host-only, no GPU needed)."""
    a = _conv_attrs(auto_pad, pads, strides, dilations, group, False)
    xd = (ctypes.c_int64 * 4)(*x_shape)
    wd = (ctypes.c_int64 * 4)(*w_shape)
    yd = (ctypes.c_int64 * 4)()
    p = (ctypes.c_int64 * 4)()
    check(load().ore_conv_out_shape(xd, wd, ctypes.byref(a), yd, p))
    return tuple(yd), tuple(p)


def pool_out_shape(x_shape, kernel_shape, strides, auto_pad="VALID", pads=None):
    a = _pool_attrs(kernel_shape, strides, auto_pad, pads)
    xd = (ctypes.c_int64 * 4)(*x_shape)
    yd = (ctypes.c_int64 * 4)()
    p = (ctypes.c_int64 * 4)()
    check(load().ore_pool_out_shape(xd, ctypes.byref(a), yd, p))
    return tuple(yd), tuple(p)


# ------------------------------------------------------------------------------ op arms
def convolution(ctx: Context, x, w, bias=None, auto_pad="VALID", pads=None, strides=(1, 1), dilations=(1, 1),
                group=1, fuse_relu=False):
    """convolution_op.rs:94-193."""
    torch = _torch()
    yd, _ = conv_out_shape(tuple(x.shape), tuple(w.shape), auto_pad, pads, strides, dilations, group)
    y = torch.empty(yd, dtype=torch.float32, device=x.device)
    a = _conv_attrs(auto_pad, pads, strides, dilations, group, fuse_relu)
    b = ctypes.byref(_desc(bias)) if bias is not None else None
    check(load().ore_conv2d_f32(ctx.h, ctypes.byref(_desc(x)), ctypes.byref(_desc(w)), b, ctypes.byref(a),
                                ctypes.byref(_desc(y))), ctx.h)
    return y


def max_pool(ctx: Context, x, kernel_shape, strides, auto_pad="VALID", pads=None):
    """max_pool_op.rs:65-129."""
    torch = _torch()
    yd, _ = pool_out_shape(tuple(x.shape), kernel_shape, strides, auto_pad, pads)
    y = torch.empty(yd, dtype=torch.float32, device=x.device)
    a = _pool_attrs(kernel_shape, strides, auto_pad, pads)
    check(load().ore_maxpool2d_f32(ctx.h, ctypes.byref(_desc(x)), ctypes.byref(a), ctypes.byref(_desc(y))), ctx.h)
    return y


def relu(ctx: Context, x):
    """relu_op.rs:11-33."""
    y = _torch().empty_like(x)
    check(load().ore_relu_f32(ctx.h, ctypes.byref(_desc(x)), ctypes.byref(_desc(y))), ctx.h)
    return y


def add(ctx: Context, a, b):
    """add_op.rs:16-107 (b broadcast onto a)."""
    y = _torch().empty_like(a)
    check(load().ore_add_f32(ctx.h, ctypes.byref(_desc(a)), ctypes.byref(_desc(b)), ctypes.byref(_desc(y))), ctx.h)
    return y


def softmax(ctx: Context, x):
    """softmax_op.rs:45-57: (N, C*H*W) rows."""
    torch = _torch()
    rows = x.shape[0]
    y = torch.empty((rows, x.numel() // max(rows, 1)), dtype=torch.float32, device=x.device)
    check(load().ore_softmax_f32(ctx.h, ctypes.byref(_desc(x)), ctypes.byref(_desc(y))), ctx.h)
    return y


def mul(ctx: Context, a, b):
    """MatMul, mul_op.rs:11-32."""
    torch = _torch()
    y = torch.empty((a.shape[0], b.shape[1]), dtype=torch.float32, device=a.device)
    check(load().ore_matmul_f32(ctx.h, ctypes.byref(_desc(a)), ctypes.byref(_desc(b)), ctypes.byref(_desc(y))), ctx.h)
    return y


def global_average_pool(ctx: Context, x):
    """global_average_pool_op.rs:11-51."""
    torch = _torch()
    y = torch.empty((x.shape[0], x.shape[1], 1, 1), dtype=torch.float32, device=x.device)
    check(load().ore_gap_f32(ctx.h, ctypes.byref(_desc(x)), ctypes.byref(_desc(y))), ctx.h)
    return y


def concatenation(ctx: Context, a, b, axis: int = 1):
    """concatenate_op.rs:11-41."""
    torch = _torch()
    shape = list(a.shape)
    shape[axis] += b.shape[axis]
    y = torch.empty(shape, dtype=torch.float32, device=a.device)
    check(load().ore_concat_f32(ctx.h, ctypes.byref(_desc(a)), ctypes.byref(_desc(b)), int(axis),
                                ctypes.byref(_desc(y))), ctx.h)
    return y


def drop_out(ctx: Context, x, ratio: Optional[float] = None):
    """dropout_op.rs:12-89: identity at inference."""
    y = _torch().empty_like(x)
    check(load().ore_dropout_f32(ctx.h, ctypes.byref(_desc(x)), ctypes.byref(_desc(y))), ctx.h)
    return y


def reshape(x, shape: Sequence[int]):
    """reshape_op.rs:16-92: metadata-only 2-D view."""
    s = (ctypes.c_int64 * len(shape))(*shape)
    y = Tensor()
    check(load().ore_reshape(ctypes.byref(_desc(x)), s, len(shape), ctypes.byref(y)))
    return x.view(int(y.dims[0]), int(y.dims[1]))


def _check_u8(x, device: int, name: str = "x"):
    """A uint8 image batch handed to the library as a raw device pointer: a contiguous torch.uint8 CUDA
    tensor [n, H, W, C] on the context's device."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.uint8:
        raise OreError(1, f"{name}: expected a uint8 CUDA tensor")
    if x.device.index != device:
        raise OreError(1, f"{name}: on cuda:{x.device.index}, the context is on cuda:{device}")
    if x.dim() != 4:
        raise OreError(1, f"{name}: expected [n, H, W, C], got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise OreError(1, f"{name}: expected a contiguous tensor")


def _norm_arg(v, c: int, name: str):
    """scale / shift -> a ctypes float[c] (None stays None: the library's default)."""
    if v is None:
        return None
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
    if a.size != c:
        raise OreError(1, f"{name}: {a.size} values for {c} channels")
    return (ctypes.c_float * c)(*a.tolist())


def preprocess_u8(ctx: Context, x, scale=None, shift=None, reverse_channels: bool = False):
    """ore_preprocess_u8 (extension): uint8 [n, H, W, C] -> float32 [n, C, H, W] with
    y[:, c] = float32(x[..., cs]) * scale[c] + shift[c] (two float32 roundings; cs = C-1-c when
    reverse_channels).  scale / shift: C floats each (None: 1 / 0)."""
    torch = _torch()
    _check_u8(x, ctx.device)
    n, h, w, c = (int(d) for d in x.shape)
    if not 1 <= c <= 4:
        raise OreError(1, f"x: {c} channels (1..4 supported)")
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    flags = PRE_REVERSE_CHANNELS if reverse_channels else 0
    check(load().ore_preprocess_u8(ctx.h, ctypes.c_void_p(x.data_ptr()), n, h, w, c, _norm_arg(scale, c, "scale"),
                                   _norm_arg(shift, c, "shift"), flags, ctypes.byref(_desc(y))), ctx.h)
    return y


def resize_taps(src: int, resized: int, origin: int, count: int):
    """ore_resize_taps (host only): the bilinear tap table of one axis of `src` samples resized to `resized`,
    for the `count` resized indices from `origin`: (i0 int32, i1 int32, t float32), sample = s[i0] +
    (s[i1] - s[i0]) * t.  The table the resize kernels use (half-pixel centres, no antialiasing)."""
    n = min(max(int(count), 0), 16384)  # the library rejects anything outside 1..16384
    i0, i1, t = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
    check(load().ore_resize_taps(int(src), int(resized), int(origin), int(count), i0.ctypes.data_as(ctypes.c_void_p),
                                 i1.ctypes.data_as(ctypes.c_void_p), t.ctypes.data_as(ctypes.c_void_p)))
    return i0, i1, t


def center_crop_geometry(src_hw, short: int, out_hw):
    """(resized_hw, origin) of "resize the short side to `short`, centre-crop `out_hw`" for a source of
    `src_hw`, by this helper's own rule: the short side becomes `short`, the long side
    (short * long) // short_src, and the crop starts at ((Rh - H) // 2, (Rw - W) // 2).  Libraries differ in
    how they round both: a caller following another convention passes its four integers instead."""
    hs, ws = (int(v) for v in src_hw)
    h, w = (int(v) for v in out_hw)
    short = int(short)
    if min(hs, ws, h, w, short) < 1:
        raise OreError(1, f"center_crop_geometry: sizes must be positive, got {tuple(src_hw)}, {short}, {tuple(out_hw)}")
    if hs <= ws:
        rh, rw = short, (short * ws) // hs
    else:
        rh, rw = (short * hs) // ws, short
    if h > rh or w > rw:
        raise OreError(1, f"center_crop_geometry: the {h} x {w} crop is larger than the {rh} x {rw} resized image")
    return (rh, rw), ((rh - h) // 2, (rw - w) // 2)


def multi_crop_geometries(src_hw, short: int, out_hw, crops: int = 5):
    """[(resized_hw, origin, flip), ...] of the five- or ten-crop protocol for a source of `src_hw`: the short
    side resized to `short` by center_crop_geometry's rule, then, in torchvision's FiveCrop / TenCrop order, the
    `out_hw` windows at the top left, top right, bottom left and bottom right corners and the centre one
    (center_crop_geometry's).  crops=10 adds the five crops of the mirrored image: a flipped list image is the
    mirror of its window, so these are the top right, top left, bottom right, bottom left and centre windows
    with flip=True.  Feed ImageList.set with geometries=[(r, o) ...] and flips=[f ...] of the entries."""
    if crops not in (5, 10):
        raise OreError(1, f"multi_crop_geometries: crops = {crops} (5 or 10)")
    resized, centre = center_crop_geometry(src_hw, short, out_hw)
    bottom, right = resized[0] - int(out_hw[0]), resized[1] - int(out_hw[1])
    five = [(0, 0), (0, right), (bottom, 0), (bottom, right), centre]
    out = [(resized, o, False) for o in five]
    if crops == 10:
        out += [(resized, five[i], True) for i in (1, 0, 3, 2, 4)]
    return out


def resize_aa_taps(src: int, resized: int, origin: int, count: int):
    """ore_resize_aa_taps (host only): the antialiased filter's table of one shrinking axis (`src` > `resized`,
    at most 32 times), for the `count` resized indices from `origin`: (first int32, ntaps int32, sum int32,
    weights int32 [count, 64]): index k blends source samples first[k] .. first[k] + ntaps[k] - 1 with the
    integer weights weights[k, :ntaps[k]] out of sum[k]."""
    n = min(max(int(count), 0), 16384)  # the library rejects anything outside 1..16384
    first, ntaps, total = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
    weights = np.empty((n, _lib.AA_MAX_TAPS), np.int32)
    check(load().ore_resize_aa_taps(int(src), int(resized), int(origin), int(count), first.ctypes.data_as(ctypes.c_void_p),
                                    ntaps.ctypes.data_as(ctypes.c_void_p), total.ctypes.data_as(ctypes.c_void_p),
                                    weights.ctypes.data_as(ctypes.c_void_p)))
    return first, ntaps, total, weights


def _resize_arg(src_hw, out_hw, resized_hw, origin, antialias=False, name="resize", cubic=False):
    """The ore_resize of a [hs, ws] -> resized_hw (None: out_hw, a plain resize) -> out_hw window at origin.
    Under antialias the ratio rule (32 times; 16 under cubic) is checked here as the library checks it."""
    rh, rw = (int(v) for v in (out_hw if resized_hw is None else resized_hw))
    top, left = (int(v) for v in origin)
    if antialias:
        ratio = _lib.CUBIC_AA_MAX_RATIO if cubic else _lib.AA_MAX_RATIO
        for axis, s, d in (("rows", int(src_hw[0]), rh), ("columns", int(src_hw[1]), rw)):
            if d >= 1 and s > ratio * d:
                raise OreError(1, f"{name}: the antialiasing filter shrinks an axis at most {ratio} times, "
                                  f"the {axis} go {s} -> {d}")
    return Resize(rh, rw, top, left)


def _filter(antialias, cubic=False) -> int:
    """The filter word of the _ex entries: bit 0 antialiased, bit 8 the cubic kernel."""
    return (_lib.FILTER_CUBIC_BIT if cubic else 0) | (_lib.FILTER_BILINEAR_AA if antialias else _lib.FILTER_BILINEAR)


def resize_cubic_taps(src: int, resized: int, origin: int, count: int, antialias: bool = False):
    """ore_resize_cubic_taps (host only): the cubic filters' table of one axis for the `count` resized indices from
    `origin`: (first int32, ntaps int32, weights float32 [count, 64] zero padded, sum float32).  Tap k of index i
    reads source sample clamp(first[i] + k, 0, src - 1) with weight weights[i, k]; plain: 4 taps, first may be
    negative, sum 1; antialiased: the run lies inside the image, its weights are divided by sum."""
    n = min(max(int(count), 0), 16384)  # the library rejects anything outside 1..16384
    first, ntaps, total = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
    weights = np.empty((n, _lib.AA_MAX_TAPS), np.float32)
    check(load().ore_resize_cubic_taps(int(src), int(resized), int(origin), int(count), _filter(antialias, True),
                                       first.ctypes.data_as(ctypes.c_void_p), ntaps.ctypes.data_as(ctypes.c_void_p),
                                       weights.ctypes.data_as(ctypes.c_void_p), total.ctypes.data_as(ctypes.c_void_p)))
    return first, ntaps, weights, total


def preprocess_resize_u8(ctx: Context, x, out_hw, resized_hw=None, origin=(0, 0), scale=None, shift=None,
                         reverse_channels: bool = False, antialias: bool = False, cubic: bool = False):
    """ore_preprocess_resize_u8_ex (extension): uint8 [n, Hs, Ws, C] -> float32 [n, C, H, W] = out_hw: the images
    bilinearly resized to resized_hw (None: out_hw), of which the window at `origin` is kept, then normalised
    as preprocess_u8 does, in one launch.  antialias=True: axes that shrink take the area-weighted filter of
    F.interpolate(antialias=True) / PIL's BILINEAR (each by at most 32 times).  cubic=True: the bicubic filters
    instead -- a = -0.75 with 4 x 4 taps (F.interpolate(mode="bicubic"), cv2.INTER_CUBIC), or under antialias
    a = -0.5 with the support widened by the shrink ratio (PIL's BICUBIC; each axis by at most 16 times).  Overshoot
    is kept: the result is not clamped to the bytes' range."""
    torch = _torch()
    _check_u8(x, ctx.device)
    n, hs, ws, c = (int(d) for d in x.shape)
    if not 1 <= c <= 4:
        raise OreError(1, f"x: {c} channels (1..4 supported)")
    h, w = (int(v) for v in out_hw)
    if h < 1 or w < 1:
        raise OreError(1, f"out_hw: {(h, w)}")
    g = _resize_arg((hs, ws), (h, w), resized_hw, origin, antialias, cubic=cubic)
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    flags = PRE_REVERSE_CHANNELS if reverse_channels else 0
    check(load().ore_preprocess_resize_u8_ex(ctx.h, ctypes.c_void_p(x.data_ptr()), n, hs, ws, c, ctypes.byref(g),
                                             _filter(antialias, cubic), _norm_arg(scale, c, "scale"), _norm_arg(shift, c, "shift"),
                                             flags, ctypes.byref(_desc(y))), ctx.h)
    return y


def _check_image_u8(x, device: int, c: int, name: str):
    """One image of an image list, handed to the library as a raw device pointer with a row stride: a
    torch.uint8 CUDA tensor [Hs, Ws, C] on the context's device whose pixels are dense (stride(2) == 1,
    stride(1) == C) and whose rows do not overlap (stride(0) >= Ws * C); a sliced view qualifies."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.uint8:
        raise OreError(1, f"{name}: expected a uint8 CUDA tensor")
    if x.device.index != device:
        raise OreError(1, f"{name}: on cuda:{x.device.index}, the context is on cuda:{device}")
    if x.dim() != 3:
        raise OreError(1, f"{name}: expected [Hs, Ws, C], got {tuple(x.shape)}")
    hs, ws, cc = (int(d) for d in x.shape)
    if cc != c:
        raise OreError(1, f"{name}: {cc} channels, the list takes {c}")
    if hs < 1 or ws < 1:
        raise OreError(1, f"{name}: empty image {tuple(x.shape)}")
    if x.stride(2) != 1 or x.stride(1) != c or x.stride(0) < ws * c:
        raise OreError(1, f"{name}: strides {tuple(x.stride())}: expected dense pixels (C, 1) and a row stride >= Ws * C")


def _flip_words(flips, n: int):
    """The HOST flag array of ore_image_list_set_ex / _set_nv12_ex from `flips`, one bool per image."""
    flips = list(flips)
    if len(flips) != n:
        raise OreError(1, f"set: {len(flips)} flips for {n} images")
    words = (ctypes.c_uint32 * max(n, 1))()
    for i, f in enumerate(flips):
        words[i] = _lib.IMAGE_FLIP_H if f else 0
    return words


# EXIF orientation code -> (rows reversed, columns reversed, transposed): include/ore.h, ore_orient_geometry
_ORIENT_BITS = {1: (False, False, False), 2: (False, True, False), 3: (True, True, False), 4: (True, False, False),
                5: (False, False, True), 6: (True, False, True), 7: (True, True, True), 8: (False, True, True)}


def _orient_code(code, name: str = "orientation") -> int:
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or int(code) not in _ORIENT_BITS:
        raise OreError(1, f"{name}: orientation {code!r} is not an EXIF code 1..8")
    return int(code)


def oriented_hw(src_hw, code):
    """The displayed size of a stored image of `src_hw` under EXIF orientation `code`: (ws, hs) for codes 5..8."""
    hs, ws = (int(v) for v in src_hw)
    return (ws, hs) if _ORIENT_BITS[_orient_code(code)][2] else (hs, ws)


def apply_orientation(x, code):
    """The displayed image of a stored [H, W, ...] numpy array or torch tensor under EXIF orientation `code`
    (include/ore.h has the pixel table; it is PIL's ImageOps.exif_transpose): rows and / or columns reversed, then
    transposed.  A view of a numpy array; torch reverses by copying.  For references and tests: the oriented lists
    never materialise it."""
    rev_rows, rev_cols, transpose = _ORIENT_BITS[_orient_code(code)]
    if len(x.shape) < 2:
        raise OreError(1, f"apply_orientation: expected [H, W, ...], got {tuple(x.shape)}")
    if isinstance(x, np.ndarray):
        if rev_rows:
            x = x[::-1]
        if rev_cols:
            x = x[:, ::-1]
        return x.swapaxes(0, 1) if transpose else x
    dims = [d for d, on in ((0, rev_rows), (1, rev_cols)) if on]
    if dims:
        x = x.flip(dims)
    return x.transpose(0, 1) if transpose else x


def rotation_orientation(degrees_clockwise) -> int:
    """The EXIF code of a video display matrix's rotation: the frame is to be rotated `degrees_clockwise` to be
    displayed.  0 -> 1, 90 -> 6, 180 -> 3, 270 -> 8; other angles are not orientations."""
    table = {0: 1, 90: 6, 180: 3, 270: 8}
    if isinstance(degrees_clockwise, bool) or not isinstance(degrees_clockwise, (int, np.integer)) or int(degrees_clockwise) % 360 not in table:
        raise OreError(1, f"rotation_orientation: {degrees_clockwise!r} degrees (a multiple of 90)")
    return table[int(degrees_clockwise) % 360]


def orient_geometry(code, resized_hw, origin, out_hw):
    """ore_orient_geometry (host only): a displayed-space geometry (resized_hw, origin) of an `out_hw` list under EXIF
    orientation `code`, in stored space: ((rh_s, rw_s), (top_s, left_s), (hz, wz), rev_rows, rev_cols, transpose).
    Oriented image = the unoriented image of an (hz, wz) list with that stored geometry, its rows and / or columns
    reversed and then transposed as the three flags say.  The map the kernels use."""
    g = Resize(int(resized_hw[0]), int(resized_hw[1]), int(origin[0]), int(origin[1]))
    sg = Resize()
    hz, wz = ctypes.c_int64(), ctypes.c_int64()
    rr, rc, tr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    check(load().ore_orient_geometry(int(code), ctypes.byref(g), int(out_hw[0]), int(out_hw[1]), ctypes.byref(sg), ctypes.byref(hz),
                                     ctypes.byref(wz), ctypes.byref(rr), ctypes.byref(rc), ctypes.byref(tr)))
    return (sg.rh, sg.rw), (sg.top, sg.left), (hz.value, wz.value), bool(rr.value), bool(rc.value), bool(tr.value)


def _orient_bytes(orientations, n: int):
    """The HOST code array of the _set_oriented entries from `orientations`, one EXIF code per image."""
    if orientations is None:
        raise OreError(1, "set_oriented: orientations is None (set() is the entry without them)")
    codes = list(orientations)
    if len(codes) != n:
        raise OreError(1, f"set_oriented: {len(codes)} orientations for {n} images")
    arr = (ctypes.c_uint8 * max(n, 1))()
    for i, c in enumerate(codes):
        arr[i] = _orient_code(c, f"orientations[{i}]")
    return arr


class ImageList:
    """ore_image_list: up to `capacity` uint8 images of their own sizes and row strides, each resized and
    cropped to out_hw by its own geometry in ONE launch (preprocess_list_u8, Model.run_u8_list, ...).  The
    device table and its pinned mirror are allocated here; set() only fills and uploads them.  antialias=True
    makes it a list of the antialiased filter, cubic=True of the bicubic ones (see preprocess_resize_u8): properties
    of the list."""

    antialias = False
    cubic = False
    # what a descriptor format has of its own: its set entries, its ctypes descriptor, what messages call its items,
    # and _describe below
    _SET, _SET_EX, _SET_ORIENTED = "ore_image_list_set", "ore_image_list_set_ex", "ore_image_list_set_oriented"
    _DESC = _lib.ImageU8
    _NOUN = "images"

    def __init__(self, ctx: Context, capacity: int, out_hw, channels: int = 3, antialias: bool = False, cubic: bool = False):
        self._create(ctx, capacity, out_hw, channels, antialias, cubic, "ore_image_list_create_ex", lead=(int(channels),))

    def _create(self, ctx, capacity, out_hw, channels, antialias, cubic, entry, lead=(), tail=()):
        """The attributes every list has, and its handle from the format's create entry: entry(ctx, capacity, *lead,
        h, w, filter, *tail, &handle)."""
        h, w = (int(v) for v in out_hw)
        self.ctx = ctx
        self.capacity = int(capacity)
        self.out_hw = (h, w)
        self.channels = int(channels)
        self.antialias = bool(antialias)
        self.cubic = bool(cubic)
        self._images = ()
        self.h = None
        hnd = ctypes.c_void_p()
        check(getattr(load(), entry)(ctx.h, self.capacity, *lead, h, w, _filter(antialias, cubic), *tail, ctypes.byref(hnd)), ctx.h)
        self.h = hnd

    def _describe(self, d, x, name):
        """The format's own fields of descriptor d from item x of a set, after the item's host checks -> (hs, ws)."""
        _check_image_u8(x, self.ctx.device, self.channels, name)
        d.data = x.data_ptr()
        d.row_stride = int(x.stride(0))
        return int(x.shape[0]), int(x.shape[1])

    def _descriptors(self, items, geometries, short, codes=None):
        """The host checks of set() and set_oriented() (codes: its EXIF codes, one per item): the descriptor array of
        `items`, before any library call."""
        if geometries is not None and short is not None:
            raise OreError(1, "set: pass geometries or short, not both")
        items = list(items)
        if len(items) > self.capacity:
            raise OreError(1, f"set: {len(items)} {self._NOUN} exceed the list's capacity {self.capacity}")
        if geometries is not None and len(geometries) != len(items):
            raise OreError(1, f"set: {len(geometries)} geometries for {len(items)} {self._NOUN}")
        arr = (self._DESC * max(len(items), 1))()
        for i, x in enumerate(items):
            name = f"{self._NOUN}[{i}]"
            hs, ws = self._describe(arr[i], x, name)
            arr[i].hs, arr[i].ws = hs, ws
            arr[i].g = self._geometry(i, hs, ws, geometries, short, name, None if codes is None else codes[i])
        return items, arr

    def _geometry(self, i, hs, ws, geometries, short, name, code=None):
        """The ore_resize of item i of a set: in displayed space, which under an orientation code is the oriented size."""
        shown = (hs, ws) if code is None else oriented_hw((hs, ws), code)
        if geometries is not None:
            resized, origin = geometries[i]
        elif short is not None:
            resized, origin = center_crop_geometry(shown, short, self.out_hw)
        else:
            resized, origin = None, (0, 0)
        return _resize_arg(shown, self.out_hw, resized, origin, self.antialias, name, self.cubic)

    def set(self, images, geometries=None, short=None, flips=None):
        """ore_image_list_set: images is a sequence of uint8 CUDA tensors [Hs, Ws, C] (sliced views included:
        that is where row strides come from); the frame lists take frames as their classes say.  Geometry per image:
        geometries[i] = (resized_hw, origin); or short=S for center_crop_geometry(src_hw, S, out_hw); or neither, a
        plain resize to out_hw.  The upload is ordered on the context's stream; a rejected set leaves the list as it
        was.  The list keeps references to the tensors.  flips (ore_image_list_set_ex, _set_nv12_ex, _set_yuv_ex):
        one bool per image; a flipped image is its unflipped output with the columns reversed, bit for bit -- the
        mirror of the window, not a resize of the mirrored source."""
        images, arr = self._descriptors(images, geometries, short)
        if flips is None:
            check(getattr(load(), self._SET)(self.h, arr, len(images)), self.ctx.h)
        else:
            words = _flip_words(flips, len(images))
            check(getattr(load(), self._SET_EX)(self.h, arr, words, len(images)), self.ctx.h)
        self._images = tuple(images)
        return self

    def set_oriented(self, images, orientations, geometries=None, short=None, flips=None):
        """set() with one EXIF orientation code 1..8 per image (the _set_oriented entries; rotation_orientation maps a
        video's display rotation): what the decoder left undone.  The tensors stay the STORED images; geometries,
        short= and the default plain resize are in DISPLAYED space (oriented_hw), as out_hw is.  Image i is, bit for
        bit, the unoriented image of the stored-space window orient_geometry gives, permuted -- a permutation of the
        resized stored image, not a resize of apply_orientation's bytes (last bits differ).  flips compose on top.
        The first call marks the list (include/ore.h: captures of a marked list serve later orientations)."""
        images = list(images)
        codes = _orient_bytes(orientations, len(images))
        images, arr = self._descriptors(images, geometries, short, list(codes)[:len(images)])
        words = None if flips is None else _flip_words(flips, len(images))
        check(getattr(load(), self._SET_ORIENTED)(self.h, arr, words, codes, len(images)), self.ctx.h)
        self._images = tuple(images)
        return self

    @property
    def oriented(self) -> bool:
        """ore_image_list_oriented: an oriented set has succeeded on the list."""
        return bool(load().ore_image_list_oriented(self.h))

    @property
    def count(self) -> int:
        return int(load().ore_image_list_count(self.h))

    def close(self):
        if getattr(self, "h", None):
            load().ore_image_list_destroy(self.h)
            self.h = None
            self._images = ()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _yuv_matrix(matrix) -> int:
    """An ore_yuv_matrix id from its name ("bt601", "bt709", "bt601_full") or the id itself."""
    if isinstance(matrix, str):
        if matrix.lower() not in _lib.YUV_MATRICES:
            raise OreError(1, f"matrix: {matrix!r} is not one of {sorted(_lib.YUV_MATRICES)}")
        return _lib.YUV_MATRICES[matrix.lower()]
    return int(matrix)


def yuv_to_rgb(y, u, v, matrix="bt601"):
    """ore_yuv_to_rgb (host only): uint8 arrays y, u, v of one shape -> uint8 [..., 3] of R, G, B, by the integer
    conversion the NV12 kernels use (include/ore.h has the formula and the three matrices)."""
    y, u, v = (np.require(a, requirements="C") for a in (y, u, v))  # 0-d arrays stay 0-d
    for name, a in (("y", y), ("u", u), ("v", v)):
        if a.dtype != np.uint8:
            raise OreError(1, f"{name}: expected uint8, got {a.dtype}")
    if not y.shape == u.shape == v.shape:
        raise OreError(1, f"y, u, v: shapes {y.shape}, {u.shape}, {v.shape} differ")
    rgb = np.empty(y.shape + (3,), np.uint8)
    vp = ctypes.c_void_p
    check(load().ore_yuv_to_rgb(_yuv_matrix(matrix), y.ctypes.data_as(vp), u.ctypes.data_as(vp), v.ctypes.data_as(vp),
                                y.size, rgb.ctypes.data_as(vp)))
    return rgb


def nv12_to_rgb(y_plane, uv_plane, matrix="bt601"):
    """An NV12 frame on the host -- y_plane uint8 [Hs, Ws], uv_plane uint8 [ceil(Hs/2), ceil(Ws/2), 2] -> uint8
    [Hs, Ws, 3]: pixel (r, j) takes the UV pair at (r >> 1, j >> 1) through yuv_to_rgb.  These are the bytes an
    Nv12ImageList resizes: image i of one equals image i of an ImageList fed this array."""
    y_plane, uv_plane = np.asarray(y_plane), np.asarray(uv_plane)
    if y_plane.ndim != 2 or y_plane.size == 0:
        raise OreError(1, f"y_plane: expected [Hs, Ws], got {y_plane.shape}")
    hs, ws = y_plane.shape
    if uv_plane.shape != ((hs + 1) // 2, (ws + 1) // 2, 2):
        raise OreError(1, f"uv_plane: expected {((hs + 1) // 2, (ws + 1) // 2, 2)} for a {hs} x {ws} frame, got {uv_plane.shape}")
    uv = uv_plane[np.arange(hs)[:, None] >> 1, np.arange(ws)[None, :] >> 1]
    return yuv_to_rgb(y_plane, uv[..., 0], uv[..., 1], matrix)


def _check_plane_u8(x, device: int, name: str):
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.uint8:
        raise OreError(1, f"{name}: expected a uint8 CUDA tensor")
    if x.device.index != device:
        raise OreError(1, f"{name}: on cuda:{x.device.index}, the context is on cuda:{device}")


def _check_frame_nv12(frame, device: int, name: str):
    """One frame of an NV12 list, handed to the library as two raw device pointers with a pitch each (on the
    pattern of _check_image_u8): y a torch.uint8 CUDA tensor [Hs, Ws] with unit column stride, uv one of
    [ceil(Hs/2), ceil(Ws/2), 2] whose last two dims are dense; rows of neither overlap; views qualify."""
    try:
        y, uv = frame
    except (TypeError, ValueError):
        raise OreError(1, f"{name}: expected a (y, uv) pair of uint8 CUDA tensors") from None
    _check_plane_u8(y, device, f"{name}.y")
    _check_plane_u8(uv, device, f"{name}.uv")
    if y.dim() != 2:
        raise OreError(1, f"{name}.y: expected [Hs, Ws], got {tuple(y.shape)}")
    hs, ws = (int(d) for d in y.shape)
    if hs < 1 or ws < 1:
        raise OreError(1, f"{name}.y: empty plane {tuple(y.shape)}")
    hc, wc = (hs + 1) // 2, (ws + 1) // 2
    if tuple(uv.shape) != (hc, wc, 2):
        raise OreError(1, f"{name}.uv: expected {(hc, wc, 2)} for a {hs} x {ws} frame, got {tuple(uv.shape)}")
    if y.stride(1) != 1 or y.stride(0) < ws:
        raise OreError(1, f"{name}.y: strides {tuple(y.stride())}: expected a unit column stride and a row stride >= Ws")
    if uv.stride(2) != 1 or uv.stride(1) != 2 or uv.stride(0) < 2 * wc:
        raise OreError(1, f"{name}.uv: strides {tuple(uv.stride())}: expected dense pairs (2, 1) and a row stride >= 2 * ceil(Ws / 2)")
    return y, uv, hs, ws


class Nv12ImageList(ImageList):
    """An ore_image_list of NV12 frames (ore_image_list_create_nv12): what a video decoder leaves -- a Y plane and a
    half-resolution plane of (U, V) pairs, each with its own pitch -- resized, cropped and normalised in ONE launch
    with the colour conversion inside it.  Image i is bit for bit image i of an ImageList fed nv12_to_rgb of the
    frame.  Three channels (R, G, B); the matrix ("bt601", "bt709", "bt601_full") and the filter are properties of
    the list.  Model.run_u8_list, classify_u8_list and the captures take it as they take an ImageList.

    set() (ore_image_list_set_nv12) takes a sequence of (y, uv) pairs of uint8 CUDA tensors, y [Hs, Ws] and uv
    [ceil(Hs/2), ceil(Ws/2), 2], views included: the pitches are the tensors' row strides.  A window of a
    larger frame must start at an even row and column (y[y0:, x0:] with uv[y0 // 2:, x0 // 2:]).  Geometry,
    flips (ore_image_list_set_nv12_ex), ordering and what a rejected set leaves behind are ImageList.set's."""

    _SET, _SET_EX, _SET_ORIENTED = "ore_image_list_set_nv12", "ore_image_list_set_nv12_ex", "ore_image_list_set_nv12_oriented"
    _DESC = _lib.ImageNv12
    _NOUN = "frames"

    def __init__(self, ctx: Context, capacity: int, out_hw, matrix="bt601", antialias: bool = False, cubic: bool = False):
        self.matrix = _yuv_matrix(matrix)
        self._create(ctx, capacity, out_hw, 3, antialias, cubic, "ore_image_list_create_nv12", tail=(self.matrix,))

    def _describe(self, d, frame, name):
        y, uv, hs, ws = _check_frame_nv12(frame, self.ctx.device, name)
        d.y, d.uv = y.data_ptr(), uv.data_ptr()
        d.y_stride, d.uv_stride = int(y.stride(0)), int(uv.stride(0))
        return hs, ws


# ore_yuv_format name -> (planes in use, sx, sy): the chroma shifts of include/ore.h
_YUV_LAYOUT = {"nv12": (2, 1, 1), "yuyv": (1, 1, 0), "i444": (3, 0, 0), "i440": (3, 0, 1), "i422": (3, 1, 0),
               "i420": (3, 1, 1), "i411": (3, 2, 0), "gray": (1, 0, 0)}


def _yuv_plane_shapes(fmt: str, hs: int, ws: int):
    """The shapes of the planes of an hs x ws frame of format fmt, as YuvImageList.set and yuv_planes_to_rgb take them."""
    _, sx, sy = _YUV_LAYOUT[fmt]
    hc, wc = -(-hs // (1 << sy)), -(-ws // (1 << sx))
    if fmt == "yuyv":
        return [(hs, wc, 4)]
    if fmt == "nv12":
        return [(hs, ws), (hc, wc, 2)]
    if fmt == "gray":
        return [(hs, ws)]
    return [(hs, ws), (hc, wc), (hc, wc)]


def _yuv_frame_parts(frame, name: str):
    """(fmt, planes, ws or None) of a frame given as (fmt, plane, ...), with a trailing int width for YUYV only."""
    if not isinstance(frame, (tuple, list)) or not frame or not isinstance(frame[0], str):
        raise OreError(1, f"{name}: expected (format, plane, ...) with the format's name first")
    fmt, *planes = frame
    if fmt.lower() not in _YUV_LAYOUT:
        raise OreError(1, f"{name}: format {fmt!r} is not one of {sorted(_YUV_LAYOUT)}")
    fmt = fmt.lower()
    ws = None
    if fmt == "yuyv" and len(planes) == 2 and isinstance(planes[1], int):
        ws = int(planes.pop())
    if len(planes) != _YUV_LAYOUT[fmt][0]:
        raise OreError(1, f"{name}: {fmt} has {_YUV_LAYOUT[fmt][0]} plane(s), got {len(planes)}")
    return fmt, planes, ws


def _yuv_frame_size(fmt: str, shape0, ws, name: str):
    """(hs, ws) of a frame from the shape of its plane 0 (and, for YUYV, the stated width: a packed row of wc groups
    is 2 wc columns wide, or 2 wc - 1 when the caller says so)."""
    if fmt == "yuyv":
        if len(shape0) != 3 or shape0[2] != 4:
            raise OreError(1, f"{name}: plane 0: expected [Hs, ceil(Ws/2), 4] groups of Y0 U Y1 V, got {tuple(shape0)}")
        hs, wc = int(shape0[0]), int(shape0[1])
        if ws is None:
            ws = 2 * wc
        if ws not in (2 * wc, 2 * wc - 1):
            raise OreError(1, f"{name}: a width of {ws} does not have {wc} groups")
    else:
        if len(shape0) != 2:
            raise OreError(1, f"{name}: plane 0: expected [Hs, Ws], got {tuple(shape0)}")
        hs, ws = int(shape0[0]), int(shape0[1])
    if hs < 1 or ws < 1:
        raise OreError(1, f"{name}: plane 0: empty plane {tuple(shape0)}")
    return hs, ws


def yuv_planes_to_rgb(fmt, planes, matrix="bt601_full", ws=None):
    """A YUV frame on the host -> uint8 [Hs, Ws, 3]: pixel (r, j) takes Y at (r, j) and the chroma sample at
    (r >> sy, j >> sx) through yuv_to_rgb; a grey frame has U = V = 128.  planes are uint8 arrays shaped as
    YuvImageList.set takes them (ws: the width of a YUYV frame when it is odd).  These are the bytes a YuvImageList
    resizes: image i of one equals image i of an ImageList fed this array."""
    fmt, planes, ws = _yuv_frame_parts((fmt, *planes) + (() if ws is None else (int(ws),)), "planes")
    planes = [np.asarray(p) for p in planes]
    hs, ws = _yuv_frame_size(fmt, planes[0].shape, ws, "planes")
    for k, (p, want) in enumerate(zip(planes, _yuv_plane_shapes(fmt, hs, ws))):
        if p.dtype != np.uint8:
            raise OreError(1, f"planes: plane {k}: expected uint8, got {p.dtype}")
        if p.shape != want:
            raise OreError(1, f"planes: plane {k}: expected {want} for a {hs} x {ws} {fmt} frame, got {p.shape}")
    _, sx, sy = _YUV_LAYOUT[fmt]
    rr, cc = np.arange(hs)[:, None] >> sy, np.arange(ws)[None, :] >> sx
    if fmt == "yuyv":
        g = planes[0]
        y = g[:, :, 0::2].reshape(hs, -1)[:, :ws]
        u, v = g[rr, cc, 1], g[rr, cc, 3]
    elif fmt == "nv12":
        y, u, v = planes[0], planes[1][rr, cc, 0], planes[1][rr, cc, 1]
    elif fmt == "gray":
        y = planes[0]
        u = v = np.full((hs, ws), 128, np.uint8)
    else:
        y, u, v = planes[0], planes[1][rr, cc], planes[2][rr, cc]
    return yuv_to_rgb(y, u, v, matrix)


def _check_frame_yuv(frame, device: int, name: str):
    """One frame of a YUV list, handed to the library as raw device pointers with a pitch each (on the pattern of
    _check_frame_nv12): -> (format id, planes, hs, ws).  Every plane is a torch.uint8 CUDA tensor on the context's
    device whose last dimension(s) are dense and whose rows do not overlap; views qualify."""
    fmt, planes, ws = _yuv_frame_parts(frame, name)
    for k, p in enumerate(planes):
        _check_plane_u8(p, device, f"{name}: plane {k}")
    hs, ws = _yuv_frame_size(fmt, tuple(planes[0].shape), ws, name)
    for k, (p, want) in enumerate(zip(planes, _yuv_plane_shapes(fmt, hs, ws))):
        if tuple(p.shape) != want:
            raise OreError(1, f"{name}: plane {k}: expected {want} for a {hs} x {ws} {fmt} frame, got {tuple(p.shape)}")
        inner = 1 if len(want) == 2 else want[2]  # bytes of one element of a row: 1, a UV pair, a YUYV group
        dense = (inner, 1) if len(want) == 3 else (1,)
        if tuple(p.stride()[1:]) != dense or p.stride(0) < want[1] * inner:
            raise OreError(1, f"{name}: plane {k}: strides {tuple(p.stride())}: expected dense rows {dense} and a row stride >= {want[1] * inner}")
    return _lib.YUV_FORMATS[fmt], planes, hs, ws


class YuvImageList(ImageList):
    """An ore_image_list of YUV frames of mixed layouts (ore_image_list_create_yuv): what a JPEG decoder leaves --
    three planes, a packed YUYV plane, NV12 or a single Y plane, as each file's chroma subsampling dictates --
    resized, cropped and normalised in ONE launch with the colour conversion inside it.  Image i is bit for bit
    image i of an ImageList fed yuv_planes_to_rgb of the frame.  Three channels (R, G, B); the matrix (a JPEG's is
    "bt601_full") and the filter are properties of the list, the layout is each frame's own.  Model.run_u8_list,
    classify_u8_list, the captures and set_views take it as they take an ImageList.

    set() (ore_image_list_set_yuv) takes a sequence of (fmt, plane, ...) with fmt one of "nv12" "yuyv" "i444"
    "i440" "i422" "i420" "i411" "gray" and the planes uint8 CUDA tensors, views included (the pitches are the
    tensors' row strides):
        i4xx   y [Hs, Ws], u and v [ceil(Hs / 2^sy), ceil(Ws / 2^sx)]
        nv12   y [Hs, Ws], uv [ceil(Hs/2), ceil(Ws/2), 2]
        yuyv   one plane [Hs, ceil(Ws/2), 4] of Y0 U Y1 V groups; the width is twice the groups, or one less
               when given: ("yuyv", plane, ws)
        gray   y [Hs, Ws]
    A window of a larger frame must start at a row and column that are multiples of (2^sy, 2^sx).  Geometry,
    flips (ore_image_list_set_yuv_ex), ordering and what a rejected set leaves behind are ImageList.set's."""

    _SET, _SET_EX, _SET_ORIENTED = "ore_image_list_set_yuv", "ore_image_list_set_yuv_ex", "ore_image_list_set_yuv_oriented"
    _DESC = _lib.ImageYuv
    _NOUN = "frames"

    def __init__(self, ctx: Context, capacity: int, out_hw, matrix="bt601_full", antialias: bool = False, cubic: bool = False):
        self.matrix = _yuv_matrix(matrix)
        self._create(ctx, capacity, out_hw, 3, antialias, cubic, "ore_image_list_create_yuv", tail=(self.matrix,))

    def _describe(self, d, frame, name):
        fmt, planes, hs, ws = _check_frame_yuv(frame, self.ctx.device, name)
        for k, p in enumerate(planes):
            d.plane[k] = p.data_ptr()
            d.stride[k] = int(p.stride(0))
        d.format = fmt
        return hs, ws


def preprocess_list_u8(ctx: Context, lst: ImageList, scale=None, shift=None, reverse_channels: bool = False):
    """ore_preprocess_list_u8 (extension): the images of `lst` -> float32 [count, C, H, W], image i resized,
    cropped and normalised exactly as preprocess_resize_u8 would a dense copy of it alone, in one launch."""
    torch = _torch()
    if not isinstance(lst, ImageList) or lst.h is None:
        raise OreError(1, "lst: expected an open ImageList")
    if lst.ctx is not ctx:
        raise OreError(1, "lst: the image list belongs to another context")
    c = lst.channels
    y = torch.empty((lst.count, c) + lst.out_hw, dtype=torch.float32, device=f"cuda:{ctx.device}")
    if y.shape[0] == 0:  # nothing to launch (and an empty tensor has no pointer to hand over)
        return y
    flags = PRE_REVERSE_CHANNELS if reverse_channels else 0
    check(load().ore_preprocess_list_u8(ctx.h, lst.h, _norm_arg(scale, c, "scale"), _norm_arg(shift, c, "shift"), flags,
                                        ctypes.byref(_desc(y))), ctx.h)
    return y


def topk(ctx: Context, x, k: int):
    """ore_topk_f32 (extension): the k best elements of every row of x [rows, ...] (the row is the flattened
    rest), as (values float32 [rows, k], indices int32 [rows, k]).  Larger first, equal values by lower index,
    NaNs last: np.argsort(-x, axis=1, kind="stable")[:, :k].  1 <= k <= min(row length, 64)."""
    torch = _torch()
    d = _desc(x)
    rows = int(x.shape[0])
    D = 1
    for s in x.shape[1:]:
        D *= int(s)
    if not 1 <= int(k) <= min(D, 64):
        raise OreError(1, f"k = {k} outside 1..{min(D, 64)} (min(row length, 64))")
    values = torch.empty((rows, int(k)), dtype=torch.float32, device=x.device)
    indices = torch.empty((rows, int(k)), dtype=torch.int32, device=x.device)
    check(load().ore_topk_f32(ctx.h, ctypes.byref(d), int(k), ctypes.c_void_p(values.data_ptr()),
                              ctypes.c_void_p(indices.data_ptr())), ctx.h)
    return values, indices


def topk_mean(ctx: Context, x, views: int, k: int):
    """ore_topk_mean_f32 (extension): topk over the mean rows of groups of `views` consecutive rows of x, as
    (values float32 [rows // views, k], indices int32 [rows // views, k]).  The mean is the float32 sum in
    ascending row order divided by float32(views), every operation rounded on its own; views=1 is topk."""
    torch = _torch()
    d = _desc(x)
    rows = int(x.shape[0])
    D = 1
    for s in x.shape[1:]:
        D *= int(s)
    views = int(views)
    if not 1 <= views <= _lib.MAX_VIEWS:
        raise OreError(1, f"views = {views} outside 1..{_lib.MAX_VIEWS}")
    if rows % views:
        raise OreError(1, f"{rows} rows are not a multiple of views = {views}")
    if not 1 <= int(k) <= min(D, 64):
        raise OreError(1, f"k = {k} outside 1..{min(D, 64)} (min(row length, 64))")
    values = torch.empty((rows // views, int(k)), dtype=torch.float32, device=x.device)
    indices = torch.empty((rows // views, int(k)), dtype=torch.int32, device=x.device)
    check(load().ore_topk_mean_f32(ctx.h, ctypes.byref(d), views, int(k), ctypes.c_void_p(values.data_ptr()),
                                   ctypes.c_void_p(indices.data_ptr())), ctx.h)
    return values, indices


def class_maps(ctx: Context, x, w, bias, classes, relu: bool = True, views: int = 1):
    """ore_class_maps_f32 (extension): the class activation maps of the selected classes, a gathered 1x1 conv.
    x float32 [n, C, H, W] (images may be strided: x.stride(0) >= C*H*W with dense images), w float32 [M, C]
    (or [M, C, 1, 1]), bias float32 [M] or None, classes int32 [n // views, k]; returns float32 [n, k, H, W] with
    maps[i, j] = relu?(conv1x1(x[i], w[classes[i // views, j]]) + bias[...]), the conv kernels' bits."""
    torch = _torch()
    for name, t, dt in (("x", x, torch.float32), ("w", w, torch.float32), ("classes", classes, torch.int32)) + \
            ((("bias", bias, torch.float32),) if bias is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
            raise OreError(1, f"{name}: expected a {str(dt).split('.')[-1]} CUDA tensor")
        if t.device.index != ctx.device:
            raise OreError(1, f"{name}: on cuda:{t.device.index}, the context is on cuda:{ctx.device}")
    if x.dim() != 4:
        raise OreError(1, f"x: expected [n, C, H, W], got {tuple(x.shape)}")
    n, C, H, W = (int(s) for s in x.shape)
    if n and (not x[0].is_contiguous() or (n > 1 and x.stride(0) < C * H * W)):
        raise OreError(1, "x: expected dense images at an image stride of at least C*H*W")
    if not w.is_contiguous() or w.dim() not in (2, 4) or int(w.shape[1]) != C or w.numel() != int(w.shape[0]) * C:
        raise OreError(1, f"w: expected a contiguous [M, {C}] tensor, got {tuple(w.shape)}")
    M = int(w.shape[0])
    if bias is not None and (not bias.is_contiguous() or tuple(bias.shape) != (M,)):
        raise OreError(1, f"bias: expected a contiguous [{M}] tensor, got {tuple(bias.shape)}")
    views = int(views)
    if not 1 <= views <= _lib.MAX_VIEWS:
        raise OreError(1, f"views = {views} outside 1..{_lib.MAX_VIEWS}")
    if n % views:
        raise OreError(1, f"{n} images are not a multiple of views = {views}")
    if classes.dim() != 2 or not classes.is_contiguous() or int(classes.shape[0]) != n // views:
        raise OreError(1, f"classes: expected a contiguous [{n // views}, k] tensor, got {tuple(classes.shape)}")
    k = int(classes.shape[1])
    if not 1 <= k <= min(M, 64):
        raise OreError(1, f"k = {k} outside 1..{min(M, 64)} (min(M, 64))")
    d = Tensor()
    d.data = x.data_ptr()
    d.ndim = 4
    d.dims[0], d.dims[1], d.dims[2], d.dims[3] = n, C, H, W
    d.nstride = int(x.stride(0)) if n > 1 else 0
    maps = torch.empty((n, k, H, W), dtype=torch.float32, device=x.device)
    if n == 0:
        return maps
    check(load().ore_class_maps_f32(ctx.h, ctypes.byref(d), ctypes.c_void_p(w.data_ptr()),
                                    ctypes.c_void_p(bias.data_ptr()) if bias is not None else None, M, 1 if relu else 0,
                                    ctypes.c_void_p(classes.data_ptr()), k, views, ctypes.c_void_p(maps.data_ptr())), ctx.h)
    return maps


def _check_maps(ctx: Context, maps, out_hw, name: str):
    """(planes, Hm, Wm, H, W) of contiguous float32 CUDA maps [..., Hm, Wm] on the context's device."""
    torch = _torch()
    if not isinstance(maps, torch.Tensor) or not maps.is_cuda or maps.dtype != torch.float32:
        raise OreError(1, f"{name}: maps: expected a float32 CUDA tensor")
    if maps.device.index != ctx.device:
        raise OreError(1, f"{name}: maps: on cuda:{maps.device.index}, the context is on cuda:{ctx.device}")
    if maps.dim() < 2 or not maps.is_contiguous():
        raise OreError(1, f"{name}: maps: expected a contiguous [..., Hm, Wm] tensor, got {tuple(maps.shape)}")
    hm, wm = (int(s) for s in maps.shape[-2:])
    h, w = (int(v) for v in out_hw)
    if min(hm, wm, h, w) < 1:
        raise OreError(1, f"{name}: a {hm} x {wm} map resized to {h} x {w}: sizes must be positive")
    planes = 1
    for s in maps.shape[:-2]:
        planes *= int(s)
    return planes, hm, wm, h, w


def upsample_maps(ctx: Context, maps, out_hw):
    """ore_upsample_maps_f32 (extension): float32 maps [..., Hm, Wm] resized to [..., H, W] with the bilinear filter
    of resize_taps on floats (H >= Hm, W >= Wm), every operation rounded on its own: numpy reproduces the bits."""
    torch = _torch()
    planes, hm, wm, h, w = _check_maps(ctx, maps, out_hw, "upsample_maps")
    out = torch.empty(tuple(maps.shape[:-2]) + (h, w), dtype=torch.float32, device=maps.device)
    if planes == 0:
        return out
    check(load().ore_upsample_maps_f32(ctx.h, ctypes.c_void_p(maps.data_ptr()), planes, hm, wm, h, w,
                                       ctypes.c_void_p(out.data_ptr())), ctx.h)
    return out


def cam_boxes(ctx: Context, maps, out_hw, frac: float = 0.2):
    """ore_cam_boxes_f32 (extension): for every plane of float32 maps [..., Hm, Wm], the bounding box (top, left,
    bottom, right), half-open, in the H x W grid, of the largest 8-connected component of the upsampled plane at or
    above lo + frac * (hi - lo), and that component's pixel count: (boxes int32 [..., 4], areas int32 [...]).  An
    empty mask gives (0, 0, 0, 0) and 0; among equal counts the component met first in raster order wins."""
    torch = _torch()
    planes, hm, wm, h, w = _check_maps(ctx, maps, out_hw, "cam_boxes")
    lead = tuple(maps.shape[:-2])
    boxes = torch.empty(lead + (4,), dtype=torch.int32, device=maps.device)
    areas = torch.empty(lead, dtype=torch.int32, device=maps.device)
    if planes == 0:
        return boxes, areas
    check(load().ore_cam_boxes_f32(ctx.h, ctypes.c_void_p(maps.data_ptr()), planes, hm, wm, h, w, float(frac),
                                   ctypes.c_void_p(boxes.data_ptr()), ctypes.c_void_p(areas.data_ptr())), ctx.h)
    return boxes, areas


def cam_box_reference(map_np, out_hw, frac: float = 0.2):
    """ore_cam_box_host (host only): the box and the area of one float32 plane [Hm, Wm] by the library's plain C++
    restatement of cam_boxes' arithmetic: ((top, left, bottom, right), area)."""
    m = np.ascontiguousarray(map_np, dtype=np.float32)
    if m.ndim != 2:
        raise OreError(1, f"cam_box_reference: expected one [Hm, Wm] plane, got {m.shape}")
    h, w = (int(v) for v in out_hw)
    box = (ctypes.c_int32 * 4)()
    area = ctypes.c_int32()
    check(load().ore_cam_box_host(m.ctypes.data_as(ctypes.c_void_p), m.shape[0], m.shape[1], h, w, float(frac), box,
                                  ctypes.byref(area)))
    return tuple(int(v) for v in box), int(area.value)


def box_to_source(box, src_hw, resized_hw, origin, out_hw, flip: bool = False):
    """Host arithmetic only: a box (top, left, bottom, right) of the model's H x W window (out_hw) as float
    (y0, x0, y1, x1) in the displayed source image of src_hw = (Hs, Ws), for the window that starts at `origin` of
    the image resized to resized_hw = (rh, rw) -- the geometry an image list or set_input_resize was given.  Columns
    are mirrored within W first when the descriptor was flipped; then the origin is added and rows scale by Hs / rh,
    columns by Ws / rw.  List geometries describe the displayed (oriented) image, so orientations need nothing."""
    t, l, b, r = (float(v) for v in box)
    hs, ws = (int(v) for v in src_hw)
    rh, rw = (int(v) for v in resized_hw)
    top, left = (int(v) for v in origin)
    h, w = (int(v) for v in out_hw)
    if min(hs, ws, rh, rw, h, w) < 1 or top < 0 or left < 0 or top + h > rh or left + w > rw:
        raise OreError(1, f"box_to_source: a {h} x {w} window at {(top, left)} of a {rh} x {rw} resized image of {hs} x {ws}")
    if flip:
        l, r = w - r, w - l
    sy, sx = hs / rh, ws / rw
    return (t + top) * sy, (l + left) * sx, (b + top) * sy, (r + left) * sx


# ------------------------------------------------------------------------------ graph walker
class Model:
    """ore_model: the device-resident walker over one ONNX graph."""

    views = 1  # set_views: the classify entries' images per subject

    def __init__(self, ctx: Context, onnx_bytes: bytes, max_batch: int, precision: str = "f32",
                 winograd: bool = True):
        """precision "f32": convs on the f32-input MFMA; "f16": the fp16 variant (ORE_LOAD_F16).
        Input / output stay f32.  winograd (f32 only): 3x3 stride-1 pad-1 convs that no direct-kernel
        fusion takes run Winograd F(2x2, 3x3) in f32; False = ORE_LOAD_NO_WINOGRAD (direct kernels
        only).  Any max_batch loads: batches past run_batch run in image chunks (ore_model_run)."""
        if precision not in ("f32", "f16"):
            raise OreError(1, f"precision must be 'f32' or 'f16', not {precision!r}")
        self.ctx = ctx
        self.precision = precision
        h = ctypes.c_void_p()
        flags = {"f32": 0, "f16": LOAD_F16}[precision]
        if not winograd:
            flags |= LOAD_NO_WINOGRAD
        check(load().ore_model_load_ex(ctx.h, onnx_bytes, len(onnx_bytes), int(max_batch), flags, ctypes.byref(h)),
              ctx.h)
        self.h = h
        self.max_batch = max_batch
        # images per pass of the graph: larger batches run in image chunks inside ore_model_run
        self.run_batch = int(load().ore_model_run_batch(h))
        d = (ctypes.c_int64 * 4)()
        check(load().ore_model_input_dims(self.h, d), ctx.h)
        self.input_dims = tuple(d)[1:]
        e = ctypes.c_int64()
        check(load().ore_model_output_elems(self.h, ctypes.byref(e)), ctx.h)
        self.output_elems = e.value
        self.topk = 1  # k of the classify entries (set_topk)
        self.input_src_hw = None  # (Hs, Ws) the _u8 entries take after set_input_resize; None: the model's (H, W)

    def set_fusion(self, flags: int):
        check(load().ore_model_set_fusion(self.h, int(flags)), self.ctx.h)

    def fill_scratch(self, pattern: int):
        """ore_model_fill_scratch (debug): fill the model's activation memory (arena with its lead, xcvt, stage,
        rows) with the 32-bit pattern, stream-ordered; refused inside a capture."""
        check(load().ore_model_fill_scratch(self.h, int(pattern) & 0xFFFFFFFF), self.ctx.h)

    def scratch_buffers(self):
        """ore_model_scratch_info: [(name, device pointer, bytes)] of the model's activation buffers."""
        out = []
        name, ptr, size = ctypes.c_char_p(), ctypes.c_void_p(), ctypes.c_size_t()
        while load().ore_model_scratch_info(self.h, len(out), ctypes.byref(name), ctypes.byref(ptr),
                                            ctypes.byref(size)) == _lib.ORE_OK:
            out.append((name.value.decode(), ptr.value, size.value))
        return out

    def _check_io(self, x, out):
        """The walker reads x and writes out through raw device pointers: both must be contiguous
        float32 tensors on this context's device, x [n, C, H, W] with n <= max_batch and out holding
        n * output_elems floats (the same contract _desc() enforces for the per-op entries)."""
        torch = _torch()
        for name, t in (("x", x), ("out", out)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
                raise OreError(1, f"{name}: expected a float32 CUDA tensor")
            if t.device.index != self.ctx.device:
                raise OreError(1, f"{name}: on cuda:{t.device.index}, the context is on cuda:{self.ctx.device}")
            if not t.is_contiguous():
                raise OreError(1, f"{name}: expected a contiguous tensor")
        n = x.shape[0]
        if tuple(x.shape[1:]) != self.input_dims:
            raise OreError(1, f"input dims {tuple(x.shape[1:])} != model {self.input_dims}")
        if out.numel() < n * self.output_elems:
            raise OreError(1, f"out holds {out.numel()} floats, {n} images need {n * self.output_elems}")
        return n

    def run_into(self, x, out):
        """Asynchronous on the context stream; x [n, C, H, W], out [n, output_elems] (CUDA)."""
        n = self._check_io(x, out)
        check(load().ore_model_run(self.h, ctypes.c_void_p(x.data_ptr()), int(n), ctypes.c_void_p(out.data_ptr())),
              self.ctx.h)
        return out

    def run(self, x):
        torch = _torch()
        out = torch.empty((x.shape[0], self.output_elems), dtype=torch.float32, device=x.device)
        return self.run_into(x, out)

    def set_input_norm(self, scale=None, shift=None, reverse_channels: bool = False):
        """ore_model_set_input_norm: the per-channel scale / shift (C floats each, None: 1 / 0) and the
        channel reversal run_u8 / capture_u8 apply (see preprocess_u8)."""
        c = int(self.input_dims[0])
        flags = PRE_REVERSE_CHANNELS if reverse_channels else 0
        sc, sh = _norm_arg(scale, c, "scale"), _norm_arg(shift, c, "shift")
        check(load().ore_model_set_input_norm(self.h, sc, sh, c, flags), self.ctx.h)

    def set_input_resize(self, src_hw, resized_hw=None, origin=(0, 0), antialias: bool = False, cubic: bool = False):
        """ore_model_set_input_resize_ex: from now on run_u8 / classify_u8 / capture_u8 / capture_classify_u8 take
        uint8 [n, Hs, Ws, C] batches with (Hs, Ws) = src_hw, resized to resized_hw (None: the model's H x W) and
        cropped to the model's H x W at `origin` on the device (see preprocess_resize_u8, also for antialias and cubic),
        with the normalisation of set_input_norm.  src_hw None: back to [n, H, W, C]."""
        if src_hw is None:
            check(load().ore_model_set_input_resize(self.h, 0, 0, None), self.ctx.h)
            self.input_src_hw = None
            return
        hs, ws = (int(v) for v in src_hw)
        g = _resize_arg((hs, ws), self.input_dims[1:], resized_hw, origin, antialias, "set_input_resize", cubic)
        check(load().ore_model_set_input_resize_ex(self.h, hs, ws, ctypes.byref(g), _filter(antialias, cubic)), self.ctx.h)
        self.input_src_hw = (hs, ws)

    def _check_u8_dims(self, x):
        """x [n, Hs, Ws, C] against the model's C and the size the _u8 entries take: the model's (H, W), or the
        source size of set_input_resize; returns n."""
        n, h, w, c = (int(d) for d in x.shape)
        src = getattr(self, "input_src_hw", None)
        want = (int(self.input_dims[0]),) + (tuple(self.input_dims[1:]) if src is None else tuple(src))
        if (c, h, w) != want:
            what = "model (C, H, W)" if src is None else "(C,) + the source size of set_input_resize"
            raise OreError(1, f"input dims (H, W, C) = {(h, w, c)} != {what} = {want}")
        return n

    def _check_out(self, out):
        """The output of a _u8 / _u8_list entry, written through a raw device pointer: a contiguous float32
        CUDA tensor on this context's device."""
        torch = _torch()
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
            raise OreError(1, "out: expected a float32 CUDA tensor")
        if out.device.index != self.ctx.device:
            raise OreError(1, f"out: on cuda:{out.device.index}, the context is on cuda:{self.ctx.device}")
        if not out.is_contiguous():
            raise OreError(1, "out: expected a contiguous tensor")

    def _check_io_u8(self, x, out):
        """As _check_io for a uint8 input: x [n, H, W, C] matching the model's (C, H, W), n <= max_batch."""
        _check_u8(x, self.ctx.device)
        self._check_out(out)
        n = self._check_u8_dims(x)
        if n > self.max_batch:
            raise OreError(1, f"batch {n} exceeds max_batch {self.max_batch}")
        if out.numel() < n * self.output_elems:
            raise OreError(1, f"out holds {out.numel()} floats, {n} images need {n * self.output_elems}")
        return n

    def run_u8_into(self, x, out):
        """ore_model_run_u8: run_into on a uint8 [n, H, W, C] batch, converted on the device with the
        normalisation of set_input_norm (asynchronous on the context stream)."""
        n = self._check_io_u8(x, out)
        check(load().ore_model_run_u8(self.h, ctypes.c_void_p(x.data_ptr()), int(n), ctypes.c_void_p(out.data_ptr())),
              self.ctx.h)
        return out

    def run_u8(self, x):
        torch = _torch()
        _check_u8(x, self.ctx.device)
        out = torch.empty((x.shape[0], self.output_elems), dtype=torch.float32, device=x.device)
        return self.run_u8_into(x, out)

    def capture_u8(self, x, out):
        """ore_model_graph_capture_u8: capture run_u8_into(x, out), the conversion included, as a HIP
        graph; replay() converts and runs whatever the uint8 buffer holds then."""
        n = self._check_io_u8(x, out)
        self._graph_bufs = (x, out)  # the graph holds these pointers
        check(load().ore_model_graph_capture_u8(self.h, ctypes.c_void_p(x.data_ptr()), int(n),
                                                ctypes.c_void_p(out.data_ptr())), self.ctx.h)
        return out

    def set_topk(self, k: int):
        """ore_model_set_topk: how many classes per image classify* / capture_classify* keep,
        1 <= k <= min(output_elems, 64); default 1."""
        kmax = min(int(self.output_elems), 64)
        if not 1 <= int(k) <= kmax:
            raise OreError(1, f"k = {k} outside 1..{kmax} (min(output elems, 64))")
        check(load().ore_model_set_topk(self.h, int(k)), self.ctx.h)
        self.topk = int(k)

    def set_views(self, views: int):
        """ore_model_set_views: classify* / capture_classify* treat every `views` consecutive images as the views
        of one subject and select over the mean of their rows (topk_mean): scores and classes are
        [n // views, topk], n a multiple of views.  1 <= views <= min(64, run_batch); default 1.  run* ignore it."""
        check(load().ore_model_set_views(self.h, int(views)), self.ctx.h)
        self.views = int(views)

    # ---- class activation maps (ore_model_set_cam): the map-conv planes of the selected classes
    _cam_out = None  # the tensor of set_cam_output (kept alive: the library holds its pointer)

    @property
    def cam_hw(self):
        """ore_model_cam_dims: (Hm, Wm) of the model's class activation maps; raises ORE_ERR_UNSUPPORTED for a
        model without a map conv (a 1x1 Conv [-> Relu] -> GlobalAveragePool head)."""
        hw = (ctypes.c_int64 * 2)()
        check(load().ore_model_cam_dims(self.h, hw), self.ctx.h)
        return int(hw[0]), int(hw[1])

    def set_cam_output(self, maps):
        """ore_model_set_cam: while a float32 CUDA tensor is set, classify* / capture_classify* also write the
        class activation maps of the classes they select into it, as [n, topk, Hm, Wm] (maps[i, j] belongs to
        classes[i // views, j]); it must hold n * topk * Hm * Wm floats for every call.  None turns the maps
        off.  Turning them on or off replans the model (re-capture graphs afterwards); another tensor does not."""
        torch = _torch()
        if maps is None:
            check(load().ore_model_set_cam(self.h, None, 0), self.ctx.h)
            self._cam_out = None
            self._cam_boxes = None  # the boxes go with the maps
        else:
            if not isinstance(maps, torch.Tensor) or not maps.is_cuda or maps.dtype != torch.float32:
                raise OreError(1, "maps: expected a float32 CUDA tensor")
            if maps.device.index != self.ctx.device:
                raise OreError(1, f"maps: on cuda:{maps.device.index}, the context is on cuda:{self.ctx.device}")
            if not maps.is_contiguous():
                raise OreError(1, "maps: expected a contiguous tensor")
            check(load().ore_model_set_cam(self.h, ctypes.c_void_p(maps.data_ptr()), int(maps.numel())), self.ctx.h)
            self._cam_out = maps
        self.run_batch = int(load().ore_model_run_batch(self.h))

    def _with_cam(self, n: int, call):
        """call() with a fresh [n, topk, Hm, Wm] tensor set as the map output; the previous setting is restored."""
        torch = _torch()
        maps = torch.empty((n, self.topk) + self.cam_hw, dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        if n == 0:
            return call() + (maps,)
        prev = self._cam_out
        self.set_cam_output(maps)
        try:
            return call() + (maps,)
        finally:
            self.set_cam_output(prev)

    def classify_cam(self, x):
        """classify(x) with the class activation maps: (scores, classes, maps [n, topk, Hm, Wm]).  A convenience: it
        sets a fresh buffer and restores the previous setting, two replans per call from off; for repeated calls
        set_cam_output once and use classify_into."""
        return self._with_cam(self._check_classify_in(x, False), lambda: self.classify(x))

    def classify_cam_u8(self, x):
        """classify_u8(x) with the class activation maps."""
        return self._with_cam(self._check_classify_in(x, True), lambda: self.classify_u8(x))

    def classify_cam_u8_list(self, lst):
        """classify_u8_list(lst) with the class activation maps."""
        return self._with_cam(self._check_list(lst), lambda: self.classify_u8_list(lst))

    # ---- boxes of the class activation maps (ore_model_set_cam_boxes)
    _cam_boxes = None  # (boxes, areas, frac) of set_cam_boxes (kept alive: the library holds their pointers)

    def set_cam_boxes(self, boxes, areas=None, frac: float = 0.2):
        """ore_model_set_cam_boxes: while an int32 CUDA tensor is set, classify* / capture_classify* also write, for
        every map of set_cam_output, the box (top, left, bottom, right) in the model's H x W input of the largest
        component of the upsampled map at or above lo + frac * (hi - lo): boxes as [n, topk, 4], areas (optional) as
        [n, topk].  Both must hold n * topk planes for every call.  The maps must be on; None turns the boxes off, and
        so does set_cam_output(None).  It never replans."""
        torch = _torch()
        if boxes is None:
            check(load().ore_model_set_cam_boxes(self.h, None, None, 0, 0.0), self.ctx.h)
            self._cam_boxes = None
            return
        for name, t in (("boxes", boxes),) + ((("areas", areas),) if areas is not None else ()):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32:
                raise OreError(1, f"{name}: expected an int32 CUDA tensor")
            if t.device.index != self.ctx.device:
                raise OreError(1, f"{name}: on cuda:{t.device.index}, the context is on cuda:{self.ctx.device}")
            if not t.is_contiguous():
                raise OreError(1, f"{name}: expected a contiguous tensor")
        cap = int(boxes.numel()) // 4
        if areas is not None:
            cap = min(cap, int(areas.numel()))
        check(load().ore_model_set_cam_boxes(self.h, ctypes.c_void_p(boxes.data_ptr()),
                                             ctypes.c_void_p(areas.data_ptr()) if areas is not None else None, cap, float(frac)),
              self.ctx.h)
        self._cam_boxes = (boxes, areas, float(frac))

    def _with_boxes(self, n: int, call, frac: float):
        """_with_cam(n, call) with fresh [n, topk, 4] / [n, topk] tensors set as the box output; the previous
        settings are restored (set_cam_output(None) inside _with_cam drops the boxes with the maps)."""
        torch = _torch()
        dev = f"cuda:{self.ctx.device}"
        boxes = torch.empty((n, self.topk, 4), dtype=torch.int32, device=dev)
        areas = torch.empty((n, self.topk), dtype=torch.int32, device=dev)
        prev = self._cam_boxes

        def inner():
            if n:
                self.set_cam_boxes(boxes, areas, frac)
            return call()

        try:
            return self._with_cam(n, inner) + (boxes, areas)
        finally:
            if self._cam_out is None:  # the library dropped the boxes with the maps
                self._cam_boxes = None
            elif prev is not None:
                self.set_cam_boxes(*prev)
            else:
                self.set_cam_boxes(None)

    def classify_boxes(self, x, frac: float = 0.2):
        """classify_cam(x) with the boxes: (scores, classes, maps, boxes [n, topk, 4], areas [n, topk]).  A convenience
        built on classify_cam, with its two replans per call from off; for repeated calls set_cam_output and
        set_cam_boxes once and use classify_into."""
        return self._with_boxes(self._check_classify_in(x, False), lambda: self.classify(x), frac)

    def classify_boxes_u8(self, x, frac: float = 0.2):
        """classify_u8(x) with the class activation maps and their boxes."""
        return self._with_boxes(self._check_classify_in(x, True), lambda: self.classify_u8(x), frac)

    def classify_boxes_u8_list(self, lst, frac: float = 0.2):
        """classify_u8_list(lst) with the class activation maps and their boxes."""
        return self._with_boxes(self._check_list(lst), lambda: self.classify_u8_list(lst), frac)

    def _subjects(self, n: int) -> int:
        """The output rows of a classification of n images: n // views, n a multiple of views."""
        if n % self.views:
            raise OreError(1, f"{n} images are not a multiple of views = {self.views}")
        return n // self.views

    def _check_classify_in(self, x, u8: bool):
        """The input checks of run_into (float32 [n, C, H, W]) or run_u8_into (uint8 [n, H, W, C]); returns n."""
        torch = _torch()
        if u8:
            _check_u8(x, self.ctx.device)
            n = self._check_u8_dims(x)
        else:
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
                raise OreError(1, "x: expected a float32 CUDA tensor")
            if x.device.index != self.ctx.device:
                raise OreError(1, f"x: on cuda:{x.device.index}, the context is on cuda:{self.ctx.device}")
            if not x.is_contiguous():
                raise OreError(1, "x: expected a contiguous tensor")
            n = int(x.shape[0])
            if tuple(x.shape[1:]) != tuple(self.input_dims):
                raise OreError(1, f"input dims {tuple(x.shape[1:])} != model {self.input_dims}")
        if n > self.max_batch:
            raise OreError(1, f"batch {n} exceeds max_batch {self.max_batch}")
        return n

    def _check_classify_out(self, n: int, scores, classes):
        """The walker writes scores and classes through raw device pointers: contiguous CUDA tensors on this
        context's device, float32 and int32, both [n, topk]; n is the number of output rows (images // views)."""
        torch = _torch()
        for name, t, dt, dn in (("scores", scores, torch.float32, "float32"), ("classes", classes, torch.int32, "int32")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
                raise OreError(1, f"{name}: expected a {dn} CUDA tensor")
            if t.device.index != self.ctx.device:
                raise OreError(1, f"{name}: on cuda:{t.device.index}, the context is on cuda:{self.ctx.device}")
            if not t.is_contiguous():
                raise OreError(1, f"{name}: expected a contiguous tensor")
            if tuple(t.shape) != (n, self.topk):
                raise OreError(1, f"{name}: shape {tuple(t.shape)}, {n} images at k = {self.topk} need {(n, self.topk)}")

    def _classify(self, entry, x, scores, classes, u8: bool):
        n = self._check_classify_in(x, u8)
        self._check_classify_out(self._subjects(n), scores, classes)
        check(entry(self.h, ctypes.c_void_p(x.data_ptr()), int(n), ctypes.c_void_p(scores.data_ptr()),
                    ctypes.c_void_p(classes.data_ptr())), self.ctx.h)
        return scores, classes

    def _classify_bufs(self, x, u8: bool):
        torch = _torch()
        g = self._subjects(self._check_classify_in(x, u8))
        return (torch.empty((g, self.topk), dtype=torch.float32, device=x.device),
                torch.empty((g, self.topk), dtype=torch.int32, device=x.device))

    def classify_into(self, x, scores, classes):
        """ore_model_classify: run_into that keeps the rows on the device and writes only the topk best
        classes per image: scores float32 [n, topk] and classes int32 [n, topk], in topk()'s order
        (asynchronous on the context stream)."""
        return self._classify(load().ore_model_classify, x, scores, classes, False)

    def classify(self, x):
        return self.classify_into(x, *self._classify_bufs(x, False))

    def classify_u8_into(self, x, scores, classes):
        """ore_model_classify_u8: classify_into on a uint8 [n, H, W, C] batch (see run_u8_into)."""
        return self._classify(load().ore_model_classify_u8, x, scores, classes, True)

    def classify_u8(self, x):
        return self.classify_u8_into(x, *self._classify_bufs(x, True))

    def capture_classify(self, x, scores, classes):
        """ore_model_graph_capture_classify: capture classify_into(x, scores, classes) as a HIP graph;
        replay() runs and selects on whatever x holds then and refills scores and classes."""
        self._graph_bufs = (x, scores, classes)  # the graph holds these pointers
        return self._classify(load().ore_model_graph_capture_classify, x, scores, classes, False)

    def capture_classify_u8(self, x, scores, classes):
        """ore_model_graph_capture_classify_u8: as capture_classify on a uint8 batch, the conversion
        included (see capture_u8)."""
        self._graph_bufs = (x, scores, classes)
        return self._classify(load().ore_model_graph_capture_classify_u8, x, scores, classes, True)

    # ---- image-list input (ore_model_*_u8_list): the _u8 entries with an ImageList as the input
    def _check_list(self, lst):
        """An open ImageList of this model's context and input dims, holding at most max_batch images; returns
        its count."""
        if not isinstance(lst, ImageList) or lst.h is None:
            raise OreError(1, "lst: expected an open ImageList")
        if lst.ctx is not self.ctx:
            raise OreError(1, "lst: the image list belongs to another context than the model")
        if (lst.channels,) + tuple(lst.out_hw) != tuple(self.input_dims):
            raise OreError(1, f"lst: the list produces (C, H, W) = {(lst.channels,) + tuple(lst.out_hw)}, the model "
                              f"input is {tuple(self.input_dims)}")
        n = lst.count
        if n > self.max_batch:
            raise OreError(1, f"batch {n} exceeds max_batch {self.max_batch}")
        return n

    def _check_list_out(self, n: int, out):
        self._check_out(out)
        if out.numel() < n * self.output_elems:
            raise OreError(1, f"out holds {out.numel()} floats, {n} images need {n * self.output_elems}")

    def run_u8_list_into(self, lst, out):
        """ore_model_run_u8_list: run_u8_into on the images of an ImageList, each resized and cropped by its own
        geometry (set_input_resize does not apply) with the normalisation of set_input_norm."""
        n = self._check_list(lst)
        self._check_list_out(n, out)
        check(load().ore_model_run_u8_list(self.h, lst.h, ctypes.c_void_p(out.data_ptr())), self.ctx.h)
        return out

    def run_u8_list(self, lst):
        torch = _torch()
        n = self._check_list(lst)
        out = torch.empty((n, self.output_elems), dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        if n == 0:
            return out
        return self.run_u8_list_into(lst, out)

    def _classify_list(self, entry, lst, scores, classes):
        n = self._check_list(lst)
        self._check_classify_out(self._subjects(n), scores, classes)
        check(entry(self.h, lst.h, ctypes.c_void_p(scores.data_ptr()), ctypes.c_void_p(classes.data_ptr())), self.ctx.h)
        return scores, classes

    def classify_u8_list_into(self, lst, scores, classes):
        """ore_model_classify_u8_list: classify_u8_into on the images of an ImageList."""
        return self._classify_list(load().ore_model_classify_u8_list, lst, scores, classes)

    def classify_u8_list(self, lst):
        torch = _torch()
        n = self._check_list(lst)
        dev = f"cuda:{self.ctx.device}"
        g = self._subjects(n)
        scores = torch.empty((g, self.topk), dtype=torch.float32, device=dev)
        classes = torch.empty((g, self.topk), dtype=torch.int32, device=dev)
        if n == 0:
            return scores, classes
        return self.classify_u8_list_into(lst, scores, classes)

    def capture_u8_list(self, lst, out):
        """ore_model_graph_capture_u8_list: capture run_u8_list_into(lst, out) as a HIP graph.  replay()
        converts whatever the list's table holds then: lst.set(...) with the same count, then replay(), runs
        new images of new sizes; with another count replay() raises.  The list must outlive the graph."""
        n = self._check_list(lst)
        self._check_list_out(n, out)
        self._graph_bufs = (lst, out)  # the graph holds the table's and out's pointers
        check(load().ore_model_graph_capture_u8_list(self.h, lst.h, ctypes.c_void_p(out.data_ptr())), self.ctx.h)
        return out

    def capture_classify_u8_list(self, lst, scores, classes):
        """ore_model_graph_capture_classify_u8_list: as capture_u8_list with the selection inside the graph."""
        self._graph_bufs = (lst, scores, classes)
        return self._classify_list(load().ore_model_graph_capture_classify_u8_list, lst, scores, classes)

    def read_value(self, name: str) -> np.ndarray:
        dims = (ctypes.c_int64 * 4)()
        nd = ctypes.c_int32()
        check(load().ore_model_read_value(self.h, name.encode(), None, 0, dims, ctypes.byref(nd)), self.ctx.h)
        shape = tuple(dims)[: nd.value]
        buf = np.empty(shape, dtype=np.float32)
        check(load().ore_model_read_value(self.h, name.encode(), buf.ctypes.data_as(ctypes.c_void_p), buf.size,
                                          dims, ctypes.byref(nd)), self.ctx.h)
        return buf

    def autotune(self, x, out, reps: int = 3):
        """Per-layer block-tile search on a real run (ore_model_autotune); synchronous."""
        self._check_io(x, out)
        check(load().ore_model_autotune(self.h, ctypes.c_void_p(x.data_ptr()), int(x.shape[0]),
                                        ctypes.c_void_p(out.data_ptr()), int(reps)), self.ctx.h)

    # tile ids (ore_model_step_tile); None = a retired id (kernels removed after measuring slower)
    TILE_NAMES = ["128x128", "96x128", "64x128", "32x256",
                  None, None, None, None,  # 4-7: the LDS-free direct conv
                  None, None, None, None,  # 8-11: the warp-specialised conv_gemm_kernel
                  "stream 64x128", "stream 32x256", "stream 16x256", "stream 48x128", "stream 64x64",
                  "stream 128x64", "stream 64x64 d8", "stream 32x128", "stream 48x64", "fire",
                  "epool patch", "epool walk48", "epool walk96", "epool walk64",
                  "epool walk64 b3", None,  # 27: the 2-band walker
                  None, None, None, None, None, None, None, None,  # 28-35: ABI 1's bf16x3 kernels
                  "wino 32x32 d4", "wino 32x32 d2", "wino16 32x16", "wino16 16x32",
                  "wino lds", None,  # 41: the Winograd fire module (retired)
                  "fire f16", "first conv pool f16", "epool window f32", "fire pool f32",
                  "stream1x1 persist 32x128", "stream1x1 persist 64x64", "stream1x1 persist 16x256",
                  "conv1x1 gap f16", "conv1x1 gap f32", "epool band f32", "epool band f16"]

    def tiles(self):
        """Block tile per exec step (-1 for non-conv steps); names in TILE_NAMES."""
        return [load().ore_model_step_tile(self.h, i) for i in range(load().ore_model_step_count(self.h))]

    def set_tile(self, step: int, tile: int):
        """ore_model_set_step_tile: run exec step `step` on tile id `tile` (one of its autotune
        candidates; e.g. to restore a saved autotune result)."""
        check(load().ore_model_set_step_tile(self.h, int(step), int(tile)), self.ctx.h)

    def set_streams(self, streams: int):
        """2: run independent neighbouring steps (the fire modules' expand branches) on a side
        stream (ore_model_set_streams)."""
        check(load().ore_model_set_streams(self.h, int(streams)), self.ctx.h)

    def capture(self, x, out):
        """Capture run_into(x, out) as a HIP graph on the context stream (ore_model_graph_capture);
        replay() re-runs it on whatever x / out hold then."""
        n = self._check_io(x, out)
        self._graph_bufs = (x, out)  # the graph holds these pointers
        check(load().ore_model_graph_capture(self.h, ctypes.c_void_p(x.data_ptr()), int(n),
                                             ctypes.c_void_p(out.data_ptr())), self.ctx.h)
        return out

    def replay(self):
        check(load().ore_model_graph_launch(self.h), self.ctx.h)
        return self._graph_bufs[1]

    def enable_timing(self, on: bool = True):
        check(load().ore_model_enable_timing(self.h, 1 if on else 0), self.ctx.h)

    def steps(self):
        L = load()
        out = []
        for i in range(L.ore_model_step_count(self.h)):
            op, name = ctypes.c_char_p(), ctypes.c_char_p()
            fl, by = ctypes.c_double(), ctypes.c_double()
            check(L.ore_model_step_info(self.h, i, ctypes.byref(op), ctypes.byref(name), ctypes.byref(fl),
                                        ctypes.byref(by)), self.ctx.h)
            mf = ctypes.c_double()
            check(L.ore_model_step_mfma_flops(self.h, i, ctypes.byref(mf)), self.ctx.h)
            out.append({"op": op.value.decode(), "name": name.value.decode(), "flops": fl.value, "bytes": by.value,
                        "mfma_flops": mf.value})
        return out

    def step_times_ms(self):
        n = load().ore_model_step_count(self.h)
        buf = (ctypes.c_float * max(n, 1))()
        check(load().ore_model_step_times(self.h, buf, n), self.ctx.h)
        return list(buf)[:n]

    def close(self):
        if getattr(self, "h", None):
            load().ore_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def inference(onnx_bytes: bytes, input_data, input_tensor_name=None, device: int = 0) -> np.ndarray:
    """inference() (model_inference.rs:29-120) on the GPU: returns graph.output[0] for the batch
    (the reference only prints it).  input_data: array [n, C, H, W] or the flat per-image vector
    the reference takes (then n = 1).  input_tensor_name is accepted for signature parity; the
    seeded input is the graph input that is not an initializer (utils.rs:29-45)."""
    torch = _torch()
    ctx = Context(device)
    try:
        x = np.asarray(input_data, dtype=np.float32)
        m = Model(ctx, onnx_bytes, max_batch=max(1, x.shape[0] if x.ndim == 4 else 1))
        if x.ndim != 4:
            x = x.reshape((1,) + tuple(m.input_dims))
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{device}")
        y = m.run(xd)
        torch.cuda.synchronize(device)
        out = y.cpu().numpy()
        m.close()
        return out
    finally:
        ctx.close()
