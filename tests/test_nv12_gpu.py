"""GPU: NV12 image lists -- a video decoder's Y and UV planes straight into the list kernels
(ore_image_list_create_nv12 / _set_nv12, ore_preprocess_list_u8 and the model's _u8_list entries on such a list).

Image i of an NV12 list is defined as the bits the interleaved path gives for the [hs, ws, 3] R, G, B bytes of that
frame under the integer conversion of include/ore.h.  Every comparison here is exact and over all elements, twice:
against an ImageList fed ore.nv12_to_rgb of the frame, and against the numpy references (tests/_resize_ref.py,
tests/_resize_aa_ref.py) on the bytes of the independent conversion in tests/_nv12_ref.py.  No descriptor in this
file points outside its tensor: every one is made from a torch tensor or a view of one."""
import contextlib
import ctypes
import functools
import warnings

import numpy as np
import pytest

from _nv12_ref import NAMES, nv12_to_rgb_ref
from _resize_aa_ref import resize_aa_ref
from _resize_ref import images, resize_ref

pytestmark = pytest.mark.gpu

_MEAN = np.array([0.485, 0.456, 0.406], np.float32)
_STD = np.array([0.229, 0.224, 0.225], np.float32)
SCALE = (np.float32(1.0) / (np.float32(255.0) * _STD)).astype(np.float32)
SHIFT = (-_MEAN / _STD).astype(np.float32)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frame(hs, ws, seed):
    """Random planes of a hs x ws frame; bytes cover 0..255 where there is room, so the clamps are met."""
    return images((hs, ws), seed=seed), images(((hs + 1) // 2, (ws + 1) // 2, 2), seed=seed + 1000)


def _extremes():
    """Y = 255 with U = V = 0 over Y = 0 with U = V = 255: every channel at or past a clamp."""
    y = np.repeat(np.uint8([255, 255, 0, 0]), 6).reshape(4, 6)
    uv = np.repeat(np.uint8([0, 255]), 6).reshape(2, 3, 2)
    return y, uv


@functools.lru_cache(maxsize=None)
def _frames():
    """The frames of the equivalence tests, made once: 1x1, 2x2, two odd sizes (the last row and column share a
    chroma pair with nothing), 4x4, 33x47, 64x96, 64x64 and the extremes."""
    sizes = [(1, 1), (2, 2), (3, 5), (7, 9), (4, 4), (33, 47), (64, 96), (64, 64)]
    return tuple(_frame(hs, ws, 300 + i) for i, (hs, ws) in enumerate(sizes)) + (_extremes(),)


@functools.lru_cache(maxsize=None)
def _rgb(i, matrix):
    """The converted bytes of frame i: the library's host conversion, checked against the independent one."""
    import ore
    y, uv = _frames()[i]
    rgb = ore.nv12_to_rgb(y, uv, matrix)
    np.testing.assert_array_equal(rgb, nv12_to_rgb_ref(y, uv, matrix))
    return rgb  # shared: nothing writes to it


def _ref(rgbs, geoms, out_hw, antialias, scale=None, shift=None, reverse=False):
    fn = resize_aa_ref if antialias else resize_ref
    return np.concatenate([fn(x[None], g[0], g[1], out_hw, scale, shift, reverse) for x, g in zip(rgbs, geoms)])


@contextlib.contextmanager
def _lists(ctx, capacity, out_hw, matrix="bt601", antialias=False):
    """An NV12 list and the interleaved list of the same shape and filter, closed after the launches finished."""
    import torch
    import ore
    nv = ore.Nv12ImageList(ctx, capacity, out_hw, matrix, antialias)
    il = ore.ImageList(ctx, capacity, out_hw, 3, antialias)
    try:
        yield nv, il
    finally:
        torch.cuda.synchronize()
        nv.close()
        il.close()


def _dev(frames):
    return [(_cuda(y), _cuda(uv)) for y, uv in frames]


# out shape -> geometry of every frame that can go there; None: the frame is left out (the AA filter shrinks an
# axis at most 32 times).  4x4 -> 9x9 scales up, 33x47 -> 8x8 and 64x96 -> 5x7 shrink both axes by odd ratios,
# 64x64 -> 2x2 is the ratio limit; the other geometries crop a window of a larger resized image.
def _geoms(out_hw, antialias):
    h, w = out_hw
    out = []
    for i, (y, _) in enumerate(_frames()):
        hs, ws = y.shape
        if antialias and (hs > 32 * h or ws > 32 * w):
            out.append(None)
        elif i in (1, 3, 8):
            out.append(((h + 2, w + 3), (2, 1)))  # a window of a larger resized image
        else:
            out.append(((h, w), (0, 0)))
    return out


@pytest.mark.parametrize("matrix", NAMES)
@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_equals_the_interleaved_list(gpu_ctx, antialias, matrix):
    import torch
    import ore
    frames = _frames()
    dev = _dev(frames)
    for out_hw in [(9, 9), (8, 8), (5, 7), (2, 2)]:
        geoms = _geoms(out_hw, antialias)
        keep = [i for i, g in enumerate(geoms) if g is not None]
        assert {0, 1, 2, 3, 4, 5, 7, 8} <= set(keep) and (6 in keep or (antialias and out_hw == (2, 2)))
        gs = [geoms[i] for i in keep]
        rgbs = [_rgb(i, matrix) for i in keep]
        with _lists(gpu_ctx, len(frames), out_hw, matrix, antialias) as (nv, il):
            assert ore.load().ore_image_list_format(nv.h) == ore.IMAGE_NV12 and ore.load().ore_image_list_format(il.h) == 0
            assert ore.load().ore_image_list_matrix(nv.h) == NAMES.index(matrix)
            assert ore.load().ore_image_list_filter(nv.h) == int(antialias)
            nv.set([dev[i] for i in keep], geometries=gs)
            il.set([_cuda(x) for x in rgbs], geometries=gs)
            assert nv.count == il.count == len(keep)
            for reverse in (False, True):
                got = ore.preprocess_list_u8(gpu_ctx, nv, SCALE, SHIFT, reverse_channels=reverse)
                want = ore.preprocess_list_u8(gpu_ctx, il, SCALE, SHIFT, reverse_channels=reverse)
                torch.cuda.synchronize()
                assert tuple(got.shape) == (len(keep), 3) + out_hw
                assert torch.equal(got, want), (out_hw, reverse)
                np.testing.assert_array_equal(got.cpu().numpy(), _ref(rgbs, gs, out_hw, antialias, SCALE, SHIFT, reverse))
            # defaults: scale 1, shift 0
            np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, nv).cpu().numpy(), _ref(rgbs, gs, out_hw, antialias))


def _padded(y, uv, pad, y_off, y_extra, uv_off, uv_extra):
    """The planes as views into wider allocations filled with `pad`: the Y base y_off bytes into its buffer at a
    pitch of ws + y_extra, the UV base uv_off bytes in at a pitch of 2 ceil(ws/2) + uv_extra."""
    import torch
    hs, ws = y.shape
    hc, wc = uv.shape[:2]
    yp, up = ws + y_extra, 2 * wc + uv_extra
    ybuf = torch.full((y_off + hs * yp + 8,), pad, dtype=torch.uint8, device="cuda")
    ubuf = torch.full((uv_off + hc * up + 8,), pad, dtype=torch.uint8, device="cuda")
    yv = torch.as_strided(ybuf, (hs, ws), (yp, 1), y_off)
    uvv = torch.as_strided(ubuf, (hc, wc, 2), (up, 2, 1), uv_off)
    yv.copy_(_cuda(y))
    uvv.copy_(_cuda(uv))
    return yv, uvv


@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_pitches_and_alignment(gpu_ctx, antialias):
    """Planes inside wider allocations at odd bases and odd pitches: the result does not depend on the bytes
    around them -- of an odd-width frame the bytes past 2 ceil(ws/2) of a UV row and past ws of a Y row included."""
    import ore
    frames = [_frame(33, 47, 320), _frame(20, 31, 322), _frame(7, 9, 324), _frame(16, 64, 326)]
    layouts = [(1, 13, 1, 5), (3, 1, 3, 1), (1, 0, 5, 0), (3, 6, 7, 3)]  # y_off, y_extra, uv_off, uv_extra
    out_hw = (6, 5)
    geoms = [((8, 8), (1, 2)), (out_hw, (0, 0)), ((9, 12), (3, 7)), ((6, 8), (0, 1))]
    rgbs = [nv12_to_rgb_ref(y, uv, "bt709") for y, uv in frames]
    want = _ref(rgbs, geoms, out_hw, antialias, SCALE, SHIFT)
    with _lists(gpu_ctx, 4, out_hw, "bt709", antialias) as (nv, _):
        for pad in (0, 255):
            views = [_padded(y, uv, pad, *lay) for (y, uv), lay in zip(frames, layouts)]
            for (yv, uvv), lay in zip(views, layouts):
                assert yv.data_ptr() % 2 == 1 and uvv.data_ptr() % 2 == 1 and yv.data_ptr() % 4 == lay[0]
            assert not views[0][0].is_contiguous() and views[0][1].stride(0) == 2 * 24 + 5
            nv.set(views, geometries=geoms)
            np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, nv, SCALE, SHIFT).cpu().numpy(), want)


@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_overlapping_rois_of_one_frame(gpu_ctx, antialias):
    """Two descriptors into one frame at even origins, on overlapping bytes: each equals its window copied out."""
    import torch
    import ore
    y, uv = _frame(40, 64, 330)
    yd, uvd = _cuda(y), _cuda(uv)
    rois = [(4, 6, 21, 31), (10, 20, 30, 44)]  # y0, x0, hs, ws: even origins, odd and even sizes
    views, hosts = [], []
    for y0, x0, hs, ws in rois:
        hc, wc = (hs + 1) // 2, (ws + 1) // 2
        views.append((yd[y0:y0 + hs, x0:x0 + ws], uvd[y0 // 2:y0 // 2 + hc, x0 // 2:x0 // 2 + wc]))
        hosts.append((np.ascontiguousarray(y[y0:y0 + hs, x0:x0 + ws]), np.ascontiguousarray(uv[y0 // 2:y0 // 2 + hc, x0 // 2:x0 // 2 + wc])))
    out_hw = (7, 6)
    geoms = [((9, 8), (2, 1)), (out_hw, (0, 0))]
    with _lists(gpu_ctx, 2, out_hw, "bt601", antialias) as (nv, _):
        nv.set(views, geometries=geoms)
        got = ore.preprocess_list_u8(gpu_ctx, nv, SCALE, SHIFT).clone()
        nv.set(_dev(hosts), geometries=geoms)
        dense = ore.preprocess_list_u8(gpu_ctx, nv, SCALE, SHIFT)
        torch.cuda.synchronize()
        assert torch.equal(got, dense)
    rgbs = [nv12_to_rgb_ref(a, b, "bt601") for a, b in hosts]
    np.testing.assert_array_equal(got.cpu().numpy(), _ref(rgbs, geoms, out_hw, antialias, SCALE, SHIFT))


@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_list_into_slice(gpu_ctx, antialias):
    """y with an image stride above 3*H*W (raw ABI): the elements between images, NaN before, are NaN after."""
    import torch
    import ore
    from ore import _lib
    frames = [_frame(33, 47, 340), _frame(12, 10, 342), _frame(9, 20, 344)]
    out_hw = (5, 6)
    geoms = [(out_hw, (0, 0)), ((7, 6), (1, 0)), ((5, 8), (0, 2))]
    n, (h, w), gap = 3, out_hw, 7
    per = 3 * h * w
    ybuf = torch.full((n, per + gap), float("nan"), dtype=torch.float32, device="cuda")
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = ybuf.data_ptr(), 4, per + gap
    for i, d in enumerate((n, 3, h, w)):
        t.dims[i] = d
    L = ore.load()
    F = ctypes.c_float * 3
    with _lists(gpu_ctx, n, out_hw, "bt601_full", antialias) as (nv, _):
        nv.set(_dev(frames), geometries=geoms)
        t.nstride = per - 1
        assert L.ore_preprocess_list_u8(gpu_ctx.h, nv.h, None, None, 0, ctypes.byref(t)) == 1
        assert b"stride" in L.ore_last_error(gpu_ctx.h)
        t.nstride = per + gap
        st = L.ore_preprocess_list_u8(gpu_ctx.h, nv.h, F(*SCALE.tolist()), F(*SHIFT.tolist()), 0, ctypes.byref(t))
        assert st == 0, L.ore_last_error(gpu_ctx.h)
        got = ybuf.cpu().numpy()
    rgbs = [nv12_to_rgb_ref(a, b, "bt601_full") for a, b in frames]
    np.testing.assert_array_equal(got[:, :per].reshape(n, 3, h, w), _ref(rgbs, geoms, out_hw, antialias, SCALE, SHIFT))
    assert np.isnan(got[:, per:]).all()


@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_past_the_grid_limit(gpu_ctx, antialias):
    """65,539 frames of 2 x 2 -> 1 x 1, more than a grid's 65,535 rows: the blockIdx.y loop and the 64-bit index
    into the 48-byte table (on the pattern of test_image_list_gpu.py::test_past_the_grid_limit)."""
    import ore
    n = 65539
    pool = [_frame(2, 2, 350 + i) for i in range(5)]
    dev = _dev(pool)
    geoms = [((1, 1), (0, 0))] * 5
    refs = _ref([nv12_to_rgb_ref(a, b, "bt601") for a, b in pool], geoms, (1, 1), antialias)  # [5, 3, 1, 1]
    assert len({r.tobytes() for r in refs}) == 5
    idx = np.arange(n) % 5
    with _lists(gpu_ctx, n, (1, 1), "bt601", antialias) as (nv, _):
        nv.set([dev[i] for i in idx], geometries=[geoms[i] for i in idx])
        assert nv.count == n
        y = ore.preprocess_list_u8(gpu_ctx, nv).cpu().numpy()
    np.testing.assert_array_equal(y, refs[idx])


def _fill(arr, frames, geoms):
    from ore import _lib
    for i, ((y, uv), g) in enumerate(zip(frames, geoms)):
        arr[i].y, arr[i].uv = y.data_ptr(), uv.data_ptr()
        arr[i].hs, arr[i].ws = int(y.shape[0]), int(y.shape[1])
        arr[i].y_stride, arr[i].uv_stride = int(y.stride(0)), int(uv.stride(0))
        arr[i].g = _lib.Resize(g[0][0], g[0][1], g[1][0], g[1][1])


def test_set_semantics(gpu_ctx):
    import torch
    import ore
    from ore import _lib
    L = ore.load()
    out_hw = (6, 5)
    a = [_frame(hs, ws, 360 + i) for i, (hs, ws) in enumerate([(7, 5), (33, 20), (12, 12)])]
    b = [_frame(hs, ws, 365 + i) for i, (hs, ws) in enumerate([(20, 33), (6, 5), (9, 31)])]
    ga = [((8, 6), (2, 1)), (out_hw, (0, 0)), ((6, 6), (0, 1))]
    gb = [(out_hw, (0, 0)), (out_hw, (0, 0)), ((7, 9), (1, 4))]
    da, db = _dev(a), _dev(b)
    ref_a = _ref([nv12_to_rgb_ref(y, uv, "bt601") for y, uv in a], ga, out_hw, False)
    ref_b = _ref([nv12_to_rgb_ref(y, uv, "bt601") for y, uv in b], gb, out_hw, False)
    rgb_b = [_cuda(nv12_to_rgb_ref(y, uv, "bt601")) for y, uv in b]
    with _lists(gpu_ctx, 3, out_hw) as (nv, il):
        nv.set(da, geometries=ga)
        il.set(rgb_b, geometries=gb)
        # the wrong kind of set, both ways: refused, content and count as they were
        arr_u8 = (_lib.ImageU8 * 3)()
        for i, (x, g) in enumerate(zip(rgb_b, gb)):
            arr_u8[i].data, arr_u8[i].hs, arr_u8[i].ws, arr_u8[i].row_stride = x.data_ptr(), x.shape[0], x.shape[1], x.stride(0)
            arr_u8[i].g = _lib.Resize(g[0][0], g[0][1], g[1][0], g[1][1])
        arr = (_lib.ImageNv12 * 4)()
        _fill(arr, db, gb)
        assert L.ore_image_list_set(nv.h, arr_u8, 3) == 1 and b"NV12" in L.ore_last_error(gpu_ctx.h)
        assert L.ore_image_list_set(nv.h, arr_u8, 0) == 1
        assert L.ore_image_list_set_nv12(il.h, arr, 3) == 1 and b"interleaved" in L.ore_last_error(gpu_ctx.h)
        assert L.ore_image_list_set_nv12(il.h, arr, 0) == 1
        assert nv.count == 3 and il.count == 3
        np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, nv).cpu().numpy(), ref_a)
        np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, il).cpu().numpy(), ref_b)
        # a failed check keeps the previous table; so does a count above the capacity
        with pytest.raises(ore.OreError, match="image 2.*outside"):
            nv.set(db, geometries=[gb[0], gb[1], (out_hw, (1, 0))])
        with pytest.raises(ore.OreError, match="capacity"):
            nv.set(db + db[:1], geometries=gb + gb[:1])
        _fill(arr, db + db[:1], gb + gb[:1])
        assert L.ore_image_list_set_nv12(nv.h, arr, 4) == 1 and b"capacity" in L.ore_last_error(gpu_ctx.h)  # the library's own check
        assert L.ore_image_list_set_nv12(nv.h, None, 2) == 1
        assert L.ore_image_list_set_nv12(nv.h, arr, -1) == 1
        assert nv.count == 3
        np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, nv).cpu().numpy(), ref_a)
        # set, run, set, run without a sync in between: each run reads its own table, and the descriptor array is
        # the caller's again as soon as set returns
        torch.cuda.synchronize()
        assert L.ore_image_list_set_nv12(nv.h, arr, 3) == 0
        _fill(arr, da, ga)  # overwritten right away
        y1 = ore.preprocess_list_u8(gpu_ctx, nv)
        assert L.ore_image_list_set_nv12(nv.h, arr, 3) == 0
        ctypes.memset(arr, 0, ctypes.sizeof(arr))
        y2 = ore.preprocess_list_u8(gpu_ctx, nv)
        _fill(arr, db[:2], gb[:2])
        assert L.ore_image_list_set_nv12(nv.h, arr, 2) == 0
        y3 = ore.preprocess_list_u8(gpu_ctx, nv)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(y1.cpu().numpy(), ref_b)
        np.testing.assert_array_equal(y2.cpu().numpy(), ref_a)
        np.testing.assert_array_equal(y3.cpu().numpy(), ref_b[:2])
        nv.set([])
        assert nv.count == 0 and tuple(ore.preprocess_list_u8(gpu_ctx, nv).shape) == (0, 3) + out_hw


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


@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_squeezenet_run_u8_list(gpu_ctx, precision, antialias):
    """run_u8_list and classify_u8_list on an NV12 list equal the same calls on the RGB list of the converted frames."""
    import torch
    import ore
    from ore import squeezenet
    frames = [_frame(hs, ws, 370 + i) for i, (hs, ws) in enumerate([(90, 120), (64, 64), (51, 71)])]
    geoms = [((72, 96), (4, 16)), ((64, 64), (0, 0)), ((80, 112), (16, 48))]
    rgbs = [nv12_to_rgb_ref(y, uv, "bt709") for y, uv in frames]
    with _model(gpu_ctx, squeezenet.build(64), max_batch=4, precision=precision) as m:
        m.set_input_norm(SCALE, SHIFT)
        steps = len(m.steps())
        with _lists(gpu_ctx, 4, (64, 64), "bt709", antialias) as (nv, il):
            nv.set(_dev(frames), geometries=geoms)
            il.set([_cuda(x) for x in rgbs], geometries=geoms)
            want = m.run_u8_list(il).clone()
            got = m.run_u8_list(nv).clone()
            pre = m.run(ore.preprocess_list_u8(gpu_ctx, nv, SCALE, SHIFT)).clone()
            torch.cuda.synchronize()
            assert tuple(got.shape) == (3, m.output_elems) and bool(torch.isfinite(got).all())
            assert torch.equal(got, want) and torch.equal(got, pre)
            assert not torch.equal(got[0], got[1])
            assert len(m.steps()) == steps  # the conversion is not an exec step
            m.set_topk(3)
            ws_, wc_ = (t.clone() for t in m.classify_u8_list(il))
            gs_, gc_ = m.classify_u8_list(nv)
            torch.cuda.synchronize()
            assert torch.equal(gs_, ws_) and torch.equal(gc_, wc_)


def test_chunked_run_u8_list(gpu_ctx):
    """On the pattern of test_image_list_gpu.py::test_chunked_run_u8_list: a list above run_batch goes in chunks, and
    chunk i0 must start at descriptor i0 of the 48-byte table -- the descriptors cycle over seven tiny frames, and
    the chunk length is no multiple of seven."""
    import torch
    import ore
    from ore import squeezenet
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        n = m.run_batch + 5
        if ((n + 1) // 2) % 7 == 0:
            n += 1
        assert n <= 2048 and m.run_batch < n <= 2 * m.run_batch
        pool = _dev([_frame(16, 16, 380 + i) for i in range(7)])
        m.set_input_norm(SCALE, SHIFT)
        nv = ore.Nv12ImageList(gpu_ctx, n, (224, 224))
        try:
            nv.set([pool[i % 7] for i in range(n)])
            want = torch.empty((n, m.output_elems), device="cuda")
            m.run_into(ore.preprocess_list_u8(gpu_ctx, nv, SCALE, SHIFT), want)
            got = m.run_u8_list(nv)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
            assert not torch.equal(got[0], got[1])  # the sources do differ
        finally:
            torch.cuda.synchronize()
            nv.close()


def test_capture_u8_list_replays_current_table():
    """On the pattern of test_image_list_gpu.py::test_capture_u8_list_replays_current_table, with a context of its
    own: the graph reads the NV12 table at replay, so a set with the same count followed by a replay runs new
    frames of other sizes; another count is refused; a set inside a capture is refused."""
    import torch
    import ore
    from ore import squeezenet
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    m = ore.Model(ctx, squeezenet.build(64), max_batch=2)
    nv = ore.Nv12ImageList(ctx, 3, (64, 64), "bt601")
    try:
        m.set_input_norm(SCALE, SHIFT, reverse_channels=True)
        f1, g1 = [_frame(90, 120, 390), _frame(64, 64, 392)], [((72, 96), (4, 16)), ((64, 64), (0, 0))]
        f2, g2 = [_frame(71, 51, 394), _frame(33, 100, 396)], [((80, 64), (16, 0)), ((64, 70), (0, 3))]
        wants = []
        for fs, gs in ((f1, g1), (f2, g2)):
            ref = _ref([nv12_to_rgb_ref(y, uv, "bt601") for y, uv in fs], gs, (64, 64), False, SCALE, SHIFT, reverse=True)
            want = torch.empty((2, m.output_elems), device="cuda")
            torch.cuda.synchronize()
            m.run_into(_cuda(ref), want)
            s.synchronize()
            wants.append(want)
        assert not torch.equal(wants[0], wants[1])
        d1, d2 = _dev(f1), _dev(f2)
        nv.set(d1, geometries=g1)
        out = torch.empty_like(wants[0])
        torch.cuda.synchronize()
        m.capture_u8_list(nv, out)
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[0])
        nv.set(d2, geometries=g2)  # the same count: new frames of other sizes
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[1])
        nv.set(d1[:1], geometries=g1[:1])
        with pytest.raises(ore.OreError, match="captured on a list of 2") as e:
            m.replay()
        assert e.value.status == 1  # ORE_ERR_INVALID
        nv.set(d1 + d2[:1], geometries=g1 + g2[:1])
        with pytest.raises(ore.OreError, match="captured on a list of 2"):
            m.replay()
        nv.set(d1, geometries=g1)
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[0])
        # a set inside a stream capture is ORE_ERR_INVALID, and leaves the list as it was
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(ore.OreError, match="capture") as e:
                    nv.set(d2, geometries=g2)
                assert e.value.status == 1
            finally:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # torch remarks that the captured graph is empty: it is meant to be
                    g.capture_end()
        assert nv.count == 2
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[0])
    finally:
        s.synchronize()
        m.close()
        nv.close()
        ctx.close()
