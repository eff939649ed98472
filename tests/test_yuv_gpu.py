"""GPU: YUV image lists -- a JPEG decoder's surfaces of mixed layouts (three planes, packed YUYV, NV12, a single Y
plane) straight into the list kernels (ore_image_list_create_yuv / _set_yuv, ore_preprocess_list_u8 and the model's
_u8_list entries on such a list).

Image i of a YUV list is defined as the bits the interleaved path gives for the [hs, ws, 3] R, G, B bytes of that
frame under the pixel rule of include/ore.h.  Every comparison here is exact and over all elements, twice: against
an ImageList fed ore.yuv_planes_to_rgb of the frame, and against the numpy references (tests/_resize_ref.py,
tests/_resize_aa_ref.py) on the bytes of the independent expansion in tests/_yuv_ref.py.  No descriptor in this file
points outside its tensor: every one is made from a torch tensor or a view of one."""
import contextlib
import ctypes
import functools
import warnings

import numpy as np
import pytest

from _nv12_ref import NAMES as MATRICES
from _resize_aa_ref import resize_aa_ref
from _resize_ref import resize_ref
from _yuv_ref import FORMATS, NAMES, extremes, frame, make_planes, yuv_planes_to_rgb_ref, yuyv_width

pytestmark = pytest.mark.gpu

_MEAN = np.array([0.485, 0.456, 0.406], np.float32)
_STD = np.array([0.229, 0.224, 0.225], np.float32)
SCALE = (np.float32(1.0) / (np.float32(255.0) * _STD)).astype(np.float32)
SHIFT = (-_MEAN / _STD).astype(np.float32)
SIZES = [(1, 1), (2, 2), (3, 5), (7, 9), (4, 4), (33, 47), (64, 96), (64, 64)]
FILTERS = pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Frame:
    """A host frame: its format, planes and size; w is the width argument an odd YUYV frame carries."""

    def __init__(self, fmt, planes, hs, ws):
        self.fmt, self.planes, self.hs, self.ws = fmt, planes, hs, ws
        self.w = yuyv_width(fmt, ws)

    def rgb(self, matrix):
        return yuv_planes_to_rgb_ref(self.fmt, self.planes, matrix, self.w)

    def dev(self):
        return frame(self.fmt, [_cuda(p) for p in self.planes], self.w)


def _make(fmt, hs, ws, seed):
    return Frame(fmt, make_planes(fmt, hs, ws, seed), hs, ws)


@functools.lru_cache(maxsize=None)
def _frames(fmt):
    """The frames of the equivalence tests of one format, made once: 1x1, 2x2, two odd sizes (the last row and column
    have a chroma sample of their own), 4x4, 33x47, 64x96, 64x64 and the extremes."""
    base = 300 + 20 * NAMES.index(fmt)
    return tuple(_make(fmt, hs, ws, base + i) for i, (hs, ws) in enumerate(SIZES)) + (Frame(fmt, extremes(fmt), 4, 6),)


@functools.lru_cache(maxsize=None)
def _rgb(fmt, i, matrix):
    """The converted bytes of frame i: the library's host conversion, checked against the independent one."""
    import ore
    f = _frames(fmt)[i]
    rgb = ore.yuv_planes_to_rgb(fmt, f.planes, matrix, ws=f.w)
    np.testing.assert_array_equal(rgb, f.rgb(matrix))
    return rgb  # shared: nothing writes to it


def _ref(rgbs, geoms, out_hw, antialias, scale=None, shift=None, reverse=False):
    fn = resize_aa_ref if antialias else resize_ref
    return np.concatenate([fn(x[None], g[0], g[1], out_hw, scale, shift, reverse) for x, g in zip(rgbs, geoms)])


@contextlib.contextmanager
def _lists(ctx, capacity, out_hw, matrix="bt601_full", antialias=False):
    """A YUV list and the interleaved list of the same shape and filter, closed after the launches finished."""
    import torch
    import ore
    yl = ore.YuvImageList(ctx, capacity, out_hw, matrix, antialias)
    il = ore.ImageList(ctx, capacity, out_hw, 3, antialias)
    try:
        yield yl, il
    finally:
        torch.cuda.synchronize()
        yl.close()
        il.close()


# out shape -> geometry of every frame that can go there; None: the frame is left out (the AA filter shrinks an axis
# at most 32 times).  The geometries are those of tests/test_nv12_gpu.py.
def _geoms(out_hw, antialias):
    h, w = out_hw
    out = []
    for i, (hs, ws) in enumerate(SIZES + [(4, 6)]):
        if antialias and (hs > 32 * h or ws > 32 * w):
            out.append(None)
        elif i in (1, 3, 8):
            out.append(((h + 2, w + 3), (2, 1)))  # a window of a larger resized image
        else:
            out.append(((h, w), (0, 0)))
    return out


def test_extremes_meet_every_clamp():
    """The extremes frame of every format with chroma drives R, G and B each to 0 and to 255, under every matrix."""
    for fmt in NAMES:
        for matrix in MATRICES:
            rgb = _frames(fmt)[8].rgb(matrix)
            assert rgb.shape == (4, 6, 3)
            for ch in range(3):
                assert {0, 255} <= set(rgb[..., ch].ravel().tolist()), (fmt, matrix, ch)


@pytest.mark.parametrize("matrix", MATRICES)
@FILTERS
@pytest.mark.parametrize("fmt", NAMES)
def test_equals_the_interleaved_list(gpu_ctx, fmt, antialias, matrix):
    import torch
    import ore
    frames = _frames(fmt)
    dev = [f.dev() for f in frames]
    for out_hw in [(9, 9), (8, 8), (5, 7), (2, 2)]:
        geoms = _geoms(out_hw, antialias)
        keep = [i for i, g in enumerate(geoms) if g is not None]
        # a frame is left out by the 32x ratio rule alone: the 64 x 96 one at (2, 2) under the antialiased filter
        assert {0, 1, 2, 3, 4, 5, 7, 8} <= set(keep) and (6 in keep or (antialias and out_hw == (2, 2)))
        gs = [geoms[i] for i in keep]
        rgbs = [_rgb(fmt, i, matrix) for i in keep]
        with _lists(gpu_ctx, len(frames), out_hw, matrix, antialias) as (yl, il):
            assert ore.load().ore_image_list_format(yl.h) == ore.IMAGE_YUV == 2
            assert ore.load().ore_image_list_matrix(yl.h) == MATRICES.index(matrix)
            assert ore.load().ore_image_list_filter(yl.h) == int(antialias)
            yl.set([dev[i] for i in keep], geometries=gs)
            il.set([_cuda(x) for x in rgbs], geometries=gs)
            assert yl.count == il.count == len(keep)
            for reverse in (False, True):
                got = ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT, reverse_channels=reverse)
                want = ore.preprocess_list_u8(gpu_ctx, il, SCALE, SHIFT, reverse_channels=reverse)
                torch.cuda.synchronize()
                assert tuple(got.shape) == (len(keep), 3) + out_hw
                assert torch.equal(got, want), (out_hw, reverse)
                np.testing.assert_array_equal(got.cpu().numpy(), _ref(rgbs, gs, out_hw, antialias, SCALE, SHIFT, reverse))
            # defaults: scale 1, shift 0
            np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, yl).cpu().numpy(), _ref(rgbs, gs, out_hw, antialias))


@pytest.mark.parametrize("matrix", MATRICES)
@FILTERS
def test_nv12_descriptors_equal_an_nv12_list(gpu_ctx, antialias, matrix):
    """ORE_YUV_FMT_NV12 descriptors and an Nv12ImageList of the same tensors, flips included."""
    import torch
    import ore
    dev = [f.dev() for f in _frames("nv12")]
    flips = [i % 2 == 1 for i in range(len(dev))]
    for out_hw in [(9, 9), (5, 7), (2, 2)]:
        geoms = _geoms(out_hw, antialias)
        keep = [i for i, g in enumerate(geoms) if g is not None]
        gs = [geoms[i] for i in keep]
        nv = ore.Nv12ImageList(gpu_ctx, len(dev), out_hw, matrix, antialias)
        with _lists(gpu_ctx, len(dev), out_hw, matrix, antialias) as (yl, _):
            try:
                for fl in (None, [flips[i] for i in keep]):
                    yl.set([dev[i] for i in keep], geometries=gs, flips=fl)
                    nv.set([dev[i][1:] for i in keep], geometries=gs, flips=fl)
                    got = ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT)
                    want = ore.preprocess_list_u8(gpu_ctx, nv, SCALE, SHIFT)
                    torch.cuda.synchronize()
                    assert torch.equal(got, want), (out_hw, fl)
            finally:
                torch.cuda.synchronize()
                nv.close()


@FILTERS
def test_one_mixed_list(gpu_ctx, antialias):
    """All eight formats interleaved in a shuffled order, every other image flipped, in ONE launch: image i equals
    what a list of its format alone gives, and a flipped image its unflipped output with the columns reversed."""
    import torch
    import ore
    out_hw = (6, 7)
    picks = [(fmt, i) for fmt in NAMES for i in (3, 5, 6)]  # 7 x 9, 33 x 47, 64 x 96
    order = np.random.default_rng(7).permutation(len(picks))
    picks = [picks[k] for k in order]
    assert len({p[0] for p in picks[:8]}) >= 4  # the formats do alternate
    geoms = [((6, 7), (0, 0)) if k % 3 else ((9, 11), (2, 3)) for k in range(len(picks))]
    flips = [k % 2 == 1 for k in range(len(picks))]
    frames = [_frames(fmt)[i] for fmt, i in picks]
    dev = [f.dev() for f in frames]
    rgbs = [_rgb(fmt, i, "bt601_full") for fmt, i in picks]
    want = _ref(rgbs, geoms, out_hw, antialias, SCALE, SHIFT)
    with _lists(gpu_ctx, len(picks), out_hw, "bt601_full", antialias) as (yl, il):
        yl.set(dev, geometries=geoms)
        plain = ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT).clone()
        np.testing.assert_array_equal(plain.cpu().numpy(), want)
        for fmt in NAMES:  # the list of one format alone
            idx = [k for k, p in enumerate(picks) if p[0] == fmt]
            assert len(idx) == 3
            yl.set([dev[k] for k in idx], geometries=[geoms[k] for k in idx])
            single = ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT)
            torch.cuda.synchronize()
            assert torch.equal(single, plain[idx]), fmt
        yl.set(dev, geometries=geoms, flips=flips)
        il.set([_cuda(x) for x in rgbs], geometries=geoms, flips=flips)
        for reverse in (False, True):
            got = ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT, reverse_channels=reverse)
            ref = ore.preprocess_list_u8(gpu_ctx, il, SCALE, SHIFT, reverse_channels=reverse)
            torch.cuda.synchronize()
            assert torch.equal(got, ref), reverse
        got = ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT)
        torch.cuda.synchronize()
        for k, fl in enumerate(flips):
            assert torch.equal(got[k], plain[k].flip(-1) if fl else plain[k]), k
        assert not torch.equal(got, plain)


def _padded(plane, pad, off, extra):
    """A plane as a view `off` bytes into a wider allocation filled with `pad`, at a pitch of its row bytes + extra."""
    import torch
    shape = plane.shape
    inner = 1 if plane.ndim == 2 else shape[2]
    pitch = shape[1] * inner + extra
    buf = torch.full((off + shape[0] * pitch + 8,), pad, dtype=torch.uint8, device="cuda")
    v = torch.as_strided(buf, shape, (pitch, 1) if plane.ndim == 2 else (pitch, inner, 1), off)
    v.copy_(_cuda(plane))
    return v


@FILTERS
def test_pitches_alignment_and_slices(gpu_ctx, antialias):
    """Every plane of every format a view at an odd byte offset into a wider, poisoned allocation with a pitch of its
    own (the three planes of a planar frame: three different pitches): the result does not depend on the bytes around
    the planes.  y is a slice with an image stride above 3*H*W (raw ABI): the elements between images, NaN before, are
    NaN after."""
    import torch
    import ore
    from ore import _lib
    sizes = [(33, 47), (20, 31), (7, 9), (16, 64), (5, 6), (9, 13), (12, 10), (3, 3)]
    frames = [_make(fmt, hs, ws, 520 + i) for i, (fmt, (hs, ws)) in enumerate(zip(NAMES, sizes))]
    layout = [(1, 13), (3, 6), (5, 1)]  # per plane: byte offset, extra pitch
    out_hw = (6, 5)
    geoms = [((8, 8), (1, 2)), (out_hw, (0, 0)), ((9, 12), (3, 7)), ((6, 8), (0, 1))] * 2
    want = _ref([f.rgb("bt709") for f in frames], geoms, out_hw, antialias, SCALE, SHIFT)
    n, (h, w), gap = len(frames), out_hw, 7
    per = 3 * h * w
    L = ore.load()
    F = ctypes.c_float * 3
    with _lists(gpu_ctx, n, out_hw, "bt709", antialias) as (yl, _):
        for pad in (0, 255):
            views = []
            for f in frames:
                ps = [_padded(p, pad, *layout[k]) for k, p in enumerate(f.planes)]
                assert all(p.data_ptr() % 2 == 1 for p in ps)
                assert not any(p.is_contiguous() for p in ps)
                if len(ps) == 3:
                    assert len({p.stride(0) for p in ps}) == 3
                views.append(frame(f.fmt, ps, f.w))
            yl.set(views, geometries=geoms)
            np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT).cpu().numpy(), want)
            ybuf = torch.full((n, per + gap), float("nan"), dtype=torch.float32, device="cuda")
            t = _lib.Tensor()
            t.data, t.ndim, t.nstride = ybuf.data_ptr(), 4, per + gap
            for i, d in enumerate((n, 3, h, w)):
                t.dims[i] = d
            st = L.ore_preprocess_list_u8(gpu_ctx.h, yl.h, F(*SCALE.tolist()), F(*SHIFT.tolist()), 0, ctypes.byref(t))
            assert st == 0, L.ore_last_error(gpu_ctx.h)
            got = ybuf.cpu().numpy()
            np.testing.assert_array_equal(got[:, :per].reshape(n, 3, h, w), want)
            assert np.isnan(got[:, per:]).all()


@FILTERS
def test_overlapping_rois_of_one_frame(gpu_ctx, antialias):
    """Several descriptors into one I420, one I422 and one YUYV frame at legal origins -- multiples of (2^sy, 2^sx), an
    even column for YUYV -- on overlapping bytes: each equals its window copied out."""
    import torch
    import ore
    out_hw = (7, 6)
    rois = {"i420": [(4, 6, 21, 31), (10, 20, 30, 44), (0, 2, 9, 9)],     # y0, x0, hs, ws
            "i422": [(3, 6, 21, 31), (11, 20, 29, 44), (1, 0, 8, 10)],    # any row, an even column
            "yuyv": [(5, 6, 21, 31), (10, 20, 30, 44), (7, 2, 4, 5)]}
    views, hosts, geoms = [], [], []
    for k, (fmt, rs) in enumerate(rois.items()):
        _, sx, sy = FORMATS[fmt]
        full = _make(fmt, 40, 64, 530 + k)
        dev = [_cuda(p) for p in full.planes]
        for y0, x0, hs, ws in rs:
            assert y0 % (1 << sy) == 0 and x0 % (1 << sx) == 0
            hc, wc = (hs + (1 << sy) - 1) >> sy, (ws + (1 << sx) - 1) >> sx
            cy, cx = y0 >> sy, x0 >> sx
            if fmt == "yuyv":
                cut = lambda ps: [ps[0][y0:y0 + hs, cx:cx + wc]]  # noqa: E731
            else:
                cut = lambda ps: [ps[0][y0:y0 + hs, x0:x0 + ws], ps[1][cy:cy + hc, cx:cx + wc], ps[2][cy:cy + hc, cx:cx + wc]]  # noqa: E731
            w = yuyv_width(fmt, ws)
            views.append(frame(fmt, cut(dev), w))
            hosts.append(Frame(fmt, [np.ascontiguousarray(p) for p in cut(full.planes)], hs, ws))
            geoms.append(((9, 8), (2, 1)) if len(geoms) % 2 else (out_hw, (0, 0)))
    assert not views[0][1].is_contiguous()
    with _lists(gpu_ctx, len(views), out_hw, "bt601_full", antialias) as (yl, _):
        yl.set(views, geometries=geoms)
        got = ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT).clone()
        yl.set([f.dev() for f in hosts], geometries=geoms)
        dense = ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT)
        torch.cuda.synchronize()
        assert torch.equal(got, dense)
    np.testing.assert_array_equal(got.cpu().numpy(), _ref([f.rgb("bt601_full") for f in hosts], geoms, out_hw, antialias, SCALE, SHIFT))


@FILTERS
def test_past_the_grid_limit(gpu_ctx, antialias):
    """65,539 frames of 2 x 2 -> 1 x 1 cycling over the eight formats, more than a grid's 65,535 rows: the blockIdx.y
    loop and the 64-bit index into the 80-byte table (on the pattern of test_nv12_gpu.py::test_past_the_grid_limit)."""
    import ore
    n = 65539
    pool = [_make(fmt, 2, 2, 550 + i) for i, fmt in enumerate(NAMES)]
    dev = [f.dev() for f in pool]
    geoms = [((1, 1), (0, 0))] * len(pool)
    refs = _ref([f.rgb("bt601_full") for f in pool], geoms, (1, 1), antialias)  # [8, 3, 1, 1]
    assert len({r.tobytes() for r in refs}) == len(pool)
    idx = np.arange(n) % len(pool)
    with _lists(gpu_ctx, n, (1, 1), "bt601_full", antialias) as (yl, _):
        yl.set([dev[i] for i in idx], geometries=[geoms[i] for i in idx])
        assert yl.count == n
        y = ore.preprocess_list_u8(gpu_ctx, yl).cpu().numpy()
    np.testing.assert_array_equal(y, refs[idx])


def _fill(arr, frames, geoms):
    """Raw ore_image_yuv descriptors of device frames (fmt, plane, ...[, ws])."""
    from ore import _lib
    for i, (f, g) in enumerate(zip(frames, geoms)):
        planes = [p for p in f[1:] if not isinstance(p, int)]
        for k in range(3):
            arr[i].plane[k] = planes[k].data_ptr() if k < len(planes) else None
            arr[i].stride[k] = int(planes[k].stride(0)) if k < len(planes) else 0
        if f[0] == "yuyv":
            arr[i].hs, arr[i].ws = int(planes[0].shape[0]), int(f[-1]) if isinstance(f[-1], int) else 2 * int(planes[0].shape[1])
        else:
            arr[i].hs, arr[i].ws = int(planes[0].shape[0]), int(planes[0].shape[1])
        arr[i].format, arr[i].reserved = FORMATS[f[0]][0], 0
        arr[i].g = _lib.Resize(g[0][0], g[0][1], g[1][0], g[1][1])


def test_set_semantics(gpu_ctx):
    import torch
    import ore
    from ore import _lib
    L = ore.load()
    out_hw = (6, 5)
    a = [_make(fmt, hs, ws, 560 + i) for i, (fmt, (hs, ws)) in enumerate([("i444", (7, 5)), ("yuyv", (33, 21)), ("gray", (12, 12))])]
    b = [_make(fmt, hs, ws, 565 + i) for i, (fmt, (hs, ws)) in enumerate([("i411", (20, 33)), ("nv12", (6, 5)), ("i440", (9, 31))])]
    ga = [((8, 6), (2, 1)), (out_hw, (0, 0)), ((6, 6), (0, 1))]
    gb = [(out_hw, (0, 0)), (out_hw, (0, 0)), ((7, 9), (1, 4))]
    da, db = [f.dev() for f in a], [f.dev() for f in b]
    ref_a = _ref([f.rgb("bt601_full") for f in a], ga, out_hw, False)
    ref_b = _ref([f.rgb("bt601_full") for f in b], gb, out_hw, False)
    rgb_b = [_cuda(f.rgb("bt601_full")) for f in b]
    nv = ore.Nv12ImageList(gpu_ctx, 3, out_hw, "bt601_full")
    with _lists(gpu_ctx, 3, out_hw) as (yl, il):
        try:
            yl.set(da, geometries=ga)
            il.set(rgb_b, geometries=gb)
            nv.set([db[1][1:]], geometries=gb[1:2])
            ref_nv = ore.preprocess_list_u8(gpu_ctx, nv).cpu().numpy()
            # the wrong kind of set, in all three directions: refused, content and count as they were
            arr_u8 = (_lib.ImageU8 * 3)()
            for i, (x, g) in enumerate(zip(rgb_b, gb)):
                arr_u8[i].data, arr_u8[i].hs, arr_u8[i].ws, arr_u8[i].row_stride = x.data_ptr(), x.shape[0], x.shape[1], x.stride(0)
                arr_u8[i].g = _lib.Resize(g[0][0], g[0][1], g[1][0], g[1][1])
            arr_nv = (_lib.ImageNv12 * 1)()
            arr_nv[0].y, arr_nv[0].uv = db[1][1].data_ptr(), db[1][2].data_ptr()
            arr_nv[0].hs, arr_nv[0].ws, arr_nv[0].g = 6, 5, _lib.Resize(6, 5, 0, 0)
            arr = (_lib.ImageYuv * 4)()
            _fill(arr, db, gb)
            assert L.ore_image_list_set(yl.h, arr_u8, 3) == 1 and b"YUV list" in L.ore_last_error(gpu_ctx.h)
            assert L.ore_image_list_set(yl.h, arr_u8, 0) == 1
            assert L.ore_image_list_set_ex(yl.h, arr_u8, None, 3) == 1
            assert L.ore_image_list_set_nv12(yl.h, arr_nv, 1) == 1 and b"YUV list" in L.ore_last_error(gpu_ctx.h)
            assert L.ore_image_list_set_nv12_ex(yl.h, arr_nv, None, 0) == 1
            assert L.ore_image_list_set_yuv(il.h, arr, 3) == 1 and b"interleaved" in L.ore_last_error(gpu_ctx.h)
            assert L.ore_image_list_set_yuv(il.h, arr, 0) == 1
            assert L.ore_image_list_set_yuv(nv.h, arr, 3) == 1 and b"NV12 list" in L.ore_last_error(gpu_ctx.h)
            assert L.ore_image_list_set_yuv_ex(nv.h, arr, None, 0) == 1
            assert yl.count == 3 and il.count == 3 and nv.count == 1
            np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, yl).cpu().numpy(), ref_a)
            np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, il).cpu().numpy(), ref_b)
            np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, nv).cpu().numpy(), ref_nv)
            # a failed check keeps the previous table; so do a count above the capacity and an unknown flag bit
            with pytest.raises(ore.OreError, match="image 2.*outside"):
                yl.set(db, geometries=[gb[0], gb[1], (out_hw, (1, 0))])
            with pytest.raises(ore.OreError, match="capacity"):
                yl.set(db + db[:1], geometries=gb + gb[:1])
            _fill(arr, db + db[:1], gb + gb[:1])
            assert L.ore_image_list_set_yuv(yl.h, arr, 4) == 1 and b"capacity" in L.ore_last_error(gpu_ctx.h)  # the library's own check
            assert L.ore_image_list_set_yuv(yl.h, None, 2) == 1
            assert L.ore_image_list_set_yuv(yl.h, arr, -1) == 1
            W = ctypes.c_uint32 * 3
            assert L.ore_image_list_set_yuv_ex(yl.h, arr, W(0, 0, 6), 3) == 1 and b"image 2" in L.ore_last_error(gpu_ctx.h)
            arr[1].reserved = 1
            assert L.ore_image_list_set_yuv(yl.h, arr, 3) == 1 and b"image 1: reserved" in L.ore_last_error(gpu_ctx.h)
            arr[1].reserved = 0
            arr[1].plane[2] = arr[1].plane[1]  # NV12 with a third plane
            assert L.ore_image_list_set_yuv(yl.h, arr, 3) == 1 and b"image 1: plane 2 must be null" in L.ore_last_error(gpu_ctx.h)
            assert yl.count == 3
            np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, yl).cpu().numpy(), ref_a)
            # set, run, set, run without a sync in between: each run reads its own table, and the descriptor array is
            # the caller's again as soon as set returns
            torch.cuda.synchronize()
            _fill(arr, db, gb)
            assert L.ore_image_list_set_yuv(yl.h, arr, 3) == 0
            _fill(arr, da, ga)  # overwritten right away
            y1 = ore.preprocess_list_u8(gpu_ctx, yl)
            assert L.ore_image_list_set_yuv(yl.h, arr, 3) == 0
            ctypes.memset(arr, 0, ctypes.sizeof(arr))
            y2 = ore.preprocess_list_u8(gpu_ctx, yl)
            _fill(arr, db[:2], gb[:2])
            assert L.ore_image_list_set_yuv_ex(yl.h, arr, W(0, 1, 0), 2) == 0
            y3 = ore.preprocess_list_u8(gpu_ctx, yl)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(y1.cpu().numpy(), ref_b)
            np.testing.assert_array_equal(y2.cpu().numpy(), ref_a)
            np.testing.assert_array_equal(y3.cpu().numpy(), np.stack([ref_b[0], ref_b[1][..., ::-1]]))
            yl.set([])
            assert yl.count == 0 and tuple(ore.preprocess_list_u8(gpu_ctx, yl).shape) == (0, 3) + out_hw
            yl.set(da, geometries=ga)
            assert L.ore_image_list_set_yuv_ex(yl.h, arr, W(1, 1, 1), 0) == 0 and yl.count == 0  # n == 0 empties
        finally:
            torch.cuda.synchronize()
            nv.close()


# ---------------------------------------------------------------------------------------------- models
@contextlib.contextmanager
def _model(ctx, onnx_bytes, **kw):
    """A model closed even when the test fails: it must not outlive the session's context."""
    import ore
    m = ore.Model(ctx, onnx_bytes, **kw)
    try:
        yield m
    finally:
        m.close()


_MODEL_FRAMES = [("i444", (90, 120)), ("yuyv", (64, 64)), ("i411", (51, 71)), ("gray", (70, 65))]
_MODEL_GEOMS = [((72, 96), (4, 16)), ((64, 64), (0, 0)), ((80, 112), (16, 48)), ((70, 65), (3, 1))]


@FILTERS
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_squeezenet_run_u8_list(gpu_ctx, precision, antialias):
    """run_u8_list and classify_u8_list on a mixed YUV list equal the same calls on the RGB list of the converted
    frames; set_views on the mixed list selects over the mean of each pair of rows."""
    import torch
    import ore
    from ore import squeezenet
    frames = [_make(fmt, hs, ws, 570 + i) for i, (fmt, (hs, ws)) in enumerate(_MODEL_FRAMES)]
    rgbs = [f.rgb("bt601_full") for f in frames]
    with _model(gpu_ctx, squeezenet.build(64), max_batch=4, precision=precision) as m:
        m.set_input_norm(SCALE, SHIFT)
        steps = len(m.steps())
        with _lists(gpu_ctx, 4, (64, 64), "bt601_full", antialias) as (yl, il):
            yl.set([f.dev() for f in frames], geometries=_MODEL_GEOMS)
            il.set([_cuda(x) for x in rgbs], geometries=_MODEL_GEOMS)
            want = m.run_u8_list(il).clone()
            got = m.run_u8_list(yl).clone()
            pre = m.run(ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT)).clone()
            torch.cuda.synchronize()
            assert tuple(got.shape) == (4, m.output_elems) and bool(torch.isfinite(got).all())
            assert torch.equal(got, want) and torch.equal(got, pre)
            assert not torch.equal(got[0], got[1])
            assert len(m.steps()) == steps  # the conversion is not an exec step
            m.set_topk(3)
            ws_, wc_ = (t.clone() for t in m.classify_u8_list(il))
            gs_, gc_ = m.classify_u8_list(yl)
            torch.cuda.synchronize()
            assert tuple(gs_.shape) == (4, 3) and torch.equal(gs_, ws_) and torch.equal(gc_, wc_)
            # two views a subject, the second of each mirrored
            m.set_views(2)
            flips = [False, True, False, True]
            yl.set([f.dev() for f in frames], geometries=_MODEL_GEOMS, flips=flips)
            il.set([_cuda(x) for x in rgbs], geometries=_MODEL_GEOMS, flips=flips)
            ws_, wc_ = (t.clone() for t in m.classify_u8_list(il))
            gs_, gc_ = m.classify_u8_list(yl)
            rows = m.run_u8_list(yl)
            ms_, mc_ = ore.topk_mean(gpu_ctx, rows, 2, 3)
            torch.cuda.synchronize()
            assert tuple(gs_.shape) == (2, 3) and torch.equal(gs_, ws_) and torch.equal(gc_, wc_)
            assert torch.equal(gs_, ms_) and torch.equal(gc_, mc_)
            m.set_views(1)


def test_chunked_run_u8_list(gpu_ctx):
    """On the pattern of test_nv12_gpu.py::test_chunked_run_u8_list: a list above run_batch goes in chunks, and chunk
    i0 must start at descriptor i0 of the 80-byte table -- the descriptors cycle over seven tiny frames of seven
    formats, and the chunk length is no multiple of seven."""
    import torch
    import ore
    from ore import squeezenet
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        n = m.run_batch + 5
        if ((n + 1) // 2) % 7 == 0:
            n += 1
        assert n <= 2048 and m.run_batch < n <= 2 * m.run_batch
        pool = [_make(fmt, 16, 16, 580 + i).dev() for i, fmt in enumerate(NAMES[:7])]
        m.set_input_norm(SCALE, SHIFT)
        yl = ore.YuvImageList(gpu_ctx, n, (224, 224))
        try:
            yl.set([pool[i % 7] for i in range(n)])
            want = torch.empty((n, m.output_elems), device="cuda")
            m.run_into(ore.preprocess_list_u8(gpu_ctx, yl, SCALE, SHIFT), want)
            got = m.run_u8_list(yl)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
            assert not torch.equal(got[0], got[1])  # the sources do differ
        finally:
            torch.cuda.synchronize()
            yl.close()


def test_capture_u8_list_replays_current_table():
    """On the pattern of test_nv12_gpu.py::test_capture_u8_list_replays_current_table, with a context of its own: the
    graph reads the YUV table at replay, so a set with the same count followed by a replay runs new frames of other
    formats and sizes; another count is refused; a set inside a capture is refused."""
    import torch
    import ore
    from ore import squeezenet
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    m = ore.Model(ctx, squeezenet.build(64), max_batch=2)
    yl = ore.YuvImageList(ctx, 3, (64, 64), "bt601_full")
    try:
        m.set_input_norm(SCALE, SHIFT, reverse_channels=True)
        f1, g1 = [_make("i420", 90, 120, 590), _make("yuyv", 64, 63, 592)], [((72, 96), (4, 16)), ((64, 64), (0, 0))]
        f2, g2 = [_make("gray", 71, 51, 594), _make("i422", 33, 100, 596)], [((80, 64), (16, 0)), ((64, 70), (0, 3))]
        wants = []
        for fs, gs in ((f1, g1), (f2, g2)):
            ref = _ref([f.rgb("bt601_full") for f in fs], gs, (64, 64), False, SCALE, SHIFT, reverse=True)
            want = torch.empty((2, m.output_elems), device="cuda")
            torch.cuda.synchronize()
            m.run_into(_cuda(ref), want)
            s.synchronize()
            wants.append(want)
        assert not torch.equal(wants[0], wants[1])
        d1, d2 = [f.dev() for f in f1], [f.dev() for f in f2]
        yl.set(d1, geometries=g1)
        out = torch.empty_like(wants[0])
        torch.cuda.synchronize()
        m.capture_u8_list(yl, out)
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[0])
        yl.set(d2, geometries=g2)  # the same count: new frames of other formats and sizes
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[1])
        yl.set(d1[:1], geometries=g1[:1])
        with pytest.raises(ore.OreError, match="captured on a list of 2") as e:
            m.replay()
        assert e.value.status == 1  # ORE_ERR_INVALID
        yl.set(d1, geometries=g1)
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[0])
        # a set inside a stream capture is ORE_ERR_INVALID, and leaves the list as it was
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(ore.OreError, match="capture") as e:
                    yl.set(d2, geometries=g2)
                assert e.value.status == 1
            finally:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # torch remarks that the captured graph is empty: it is meant to be
                    g.capture_end()
        assert yl.count == 2
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[0])
    finally:
        s.synchronize()
        m.close()
        yl.close()
        ctx.close()
