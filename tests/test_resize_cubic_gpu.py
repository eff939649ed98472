"""GPU: the cubic resize filters in front of the graph (filter words 256 and 257 through ore_preprocess_resize_u8_ex,
the three kinds of image list and ore_model_set_input_resize_ex).

The arithmetic is fixed (include/ore.h), so numpy reproduces it bit for bit (tests/_resize_cubic_ref.py): every
comparison here is exact and over all elements.  References are computed once per case and shared."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

from _resize_cubic_ref import cubic_aa_taps_ref, resize_cubic_ref
from _resize_ref import images
from _yuv_ref import NAMES as YUV_NAMES, frame, make_planes, yuyv_width

pytestmark = pytest.mark.gpu

_MEAN = np.array([0.485, 0.456, 0.406, 0.5], np.float32)
_STD = np.array([0.229, 0.224, 0.225, 0.25], np.float32)
FILTERS = pytest.mark.parametrize("aa", [False, True], ids=["cubic", "cubic_aa"])


def _norm(c):
    """ImageNet-style scale and shift for c channels."""
    return ((np.float32(1.0) / (np.float32(255.0) * _STD[:c])).astype(np.float32), (-_MEAN[:c] / _STD[:c]).astype(np.float32))


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(got, want, msg=""):
    """Equal as bit patterns (the sign of a zero included)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, msg
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=msg)


# name: (Hs, Ws), (Rh, Rw), (top, left), (H, W)
DENSE = {
    "grow_5x7": ((5, 7), (12, 20), (0, 0), (12, 20)),          # grows both ways: negative num, first = -2, all four borders
    "rows_shrink_cols_grow": ((40, 23), (12, 26), (0, 6), (12, 20)),
    "ratio_15.4": ((13, 200), (13, 13), (1, 0), (12, 13)),     # just under 16: 61- and 62-tap column runs
    "ratio_16": ((13, 208), (13, 13), (0, 0), (13, 13)),       # exactly 16: interior runs of 64 taps
    "identity": ((12, 20), (12, 20), (0, 0), (12, 20)),
    "one_pixel": ((1, 1), (12, 20), (0, 0), (12, 20)),
    "far_corner": ((31, 45), (30, 41), (18, 21), (12, 20)),    # the window ends at the resized image's last row and column
}


@functools.lru_cache(maxsize=None)
def _dense_case(name, c):
    src = DENSE[name][0]
    return images((3,) + src + (c,), seed=900 + 7 * c + list(DENSE).index(name))


def test_the_long_runs_are_long():
    """The geometry of the long-run cases, on the host: what the dense cases below exercise."""
    assert max(len(w) for _, w, _ in cubic_aa_taps_ref(200, 13, 0, 13)) == 62
    assert max(len(w) for _, w, _ in cubic_aa_taps_ref(208, 13, 0, 13)) == 64


@FILTERS
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("name", list(DENSE))
def test_dense_matches_numpy(gpu_ctx, name, c, aa):
    import ore
    _, resized, origin, out = DENSE[name]
    x = _dense_case(name, c)
    xd = _cuda(x)
    scale, shift = _norm(c)
    y = ore.preprocess_resize_u8(gpu_ctx, xd, out, resized, origin, scale, shift, antialias=aa, cubic=True)
    assert tuple(y.shape) == (3, c) + out
    _bits_equal(y.cpu().numpy(), resize_cubic_ref(x, resized, origin, out, aa, scale, shift))
    y = ore.preprocess_resize_u8(gpu_ctx, xd, out, resized, origin, antialias=aa, cubic=True)
    plain = resize_cubic_ref(x, resized, origin, out, aa)
    _bits_equal(y.cpu().numpy(), plain, "no norm")
    if name == "identity":  # the source bytes exactly
        _bits_equal(plain, np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32))
    if c == 3:
        y = ore.preprocess_resize_u8(gpu_ctx, xd, out, resized, origin, scale, shift, reverse_channels=True, antialias=aa, cubic=True)
        _bits_equal(y.cpu().numpy(), resize_cubic_ref(x, resized, origin, out, aa, scale, shift, reverse=True), "reversed")


@FILTERS
def test_plain_crop_is_preprocess_u8(gpu_ctx, aa):
    """The geometry {hs, ws, top, left}: the result is ore_preprocess_u8 of the cropped bytes."""
    import torch
    import ore
    x = images((2, 21, 30, 3), seed=930)
    scale, shift = _norm(3)
    got = ore.preprocess_resize_u8(gpu_ctx, _cuda(x), (12, 20), (21, 30), (9, 10), scale, shift, antialias=aa, cubic=True)
    want = ore.preprocess_u8(gpu_ctx, _cuda(x[:, 9:21, 10:30]), scale, shift)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@FILTERS
@pytest.mark.parametrize("out", [(17, 19), (33, 40)], ids=["323px", "1320px"])
def test_pixel_counts_across_workgroups(gpu_ctx, out, aa):
    """Output pixel counts above one workgroup and no multiple of it: the last workgroup is partial."""
    import ore
    x = images((2, 50, 47, 3), seed=931)
    scale, shift = _norm(3)
    y = ore.preprocess_resize_u8(gpu_ctx, _cuda(x), out, scale=scale, shift=shift, antialias=aa, cubic=True)
    _bits_equal(y.cpu().numpy(), resize_cubic_ref(x, out, (0, 0), out, aa, scale, shift))


def test_antialiased_differs_from_plain_where_nothing_shrinks(gpu_ctx):
    """257 on axes that do not shrink is the a = -0.5 kernel, 256 the a = -0.75 one: other bits, each its reference."""
    import ore
    x = _dense_case("grow_5x7", 3)
    xd = _cuda(x)
    a = ore.preprocess_resize_u8(gpu_ctx, xd, (12, 20), cubic=True).cpu().numpy()
    b = ore.preprocess_resize_u8(gpu_ctx, xd, (12, 20), antialias=True, cubic=True).cpu().numpy()
    _bits_equal(a, resize_cubic_ref(x, (12, 20), (0, 0), (12, 20), False))
    _bits_equal(b, resize_cubic_ref(x, (12, 20), (0, 0), (12, 20), True))
    assert not np.array_equal(a, b)
    assert a.min() < 0 or a.max() > 255  # overshoot is kept, not clamped


@FILTERS
def test_into_a_slice_with_poisoned_gaps(gpu_ctx, aa):
    """n = 5, y with an image stride of C*H*W + 3 (raw ABI): the elements between images, NaN before, are NaN after."""
    import torch
    import ore
    from ore import _lib
    n, hs, ws, c = shape = (5, 33, 64, 3)
    h, w, gap = 12, 20, 3
    x = images(shape, seed=932)
    xd = _cuda(x)
    scale, shift = _norm(c)
    ref = resize_cubic_ref(x, (18, 24), (5, 4), (h, w), aa, scale, shift)
    per = c * h * w
    F = ctypes.c_float * c
    ybuf = torch.full((n, per + gap), float("nan"), dtype=torch.float32, device="cuda")
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = ybuf.data_ptr(), 4, per + gap
    for i, d in enumerate((n, c, h, w)):
        t.dims[i] = d
    st = ore.load().ore_preprocess_resize_u8_ex(gpu_ctx.h, ctypes.c_void_p(xd.data_ptr()), n, hs, ws, c,
                                                ctypes.byref(_lib.Resize(18, 24, 5, 4)),
                                                ore.FILTER_BICUBIC_AA if aa else ore.FILTER_BICUBIC,
                                                F(*scale.tolist()), F(*shift.tolist()), 0, ctypes.byref(t))
    assert st == 0, ore.load().ore_last_error(gpu_ctx.h)
    got = ybuf.cpu().numpy()
    _bits_equal(got[:, :per].reshape(n, c, h, w), ref)
    assert np.isnan(got[:, per:]).all()


# ---------------------------------------------------------------------------------------------- lists
@contextlib.contextmanager
def _closing(*lists):
    try:
        yield lists
    finally:
        import torch
        torch.cuda.synchronize()  # the launches that read the tables have finished
        for lst in lists:
            lst.close()


def _ref(imgs, geoms, out_hw, aa, scale=None, shift=None, reverse=False):
    return np.concatenate([resize_cubic_ref(x[None], g[0], g[1], out_hw, aa, scale, shift, reverse) for x, g in zip(imgs, geoms)])


OUT = (12, 20)
SIZES = [(1, 1), (7, 5), (33, 64), (64, 33), (12, 20), (120, 90), (13, 300)]
GEOMS = [((12, 20), (0, 0)),    # every tap clamped
         ((20, 25), (8, 5)),    # grows, the far corner
         ((18, 24), (5, 4)),    # both shrink
         ((40, 40), (24, 18)),  # rows shrink, columns grow
         ((12, 20), (0, 0)),    # the identity
         ((12, 20), (0, 0)),    # strong shrink
         ((13, 20), (1, 0))]    # columns at ratio 15
FLIPS = [True, False, True, False, True, False, True]


@FILTERS
@pytest.mark.parametrize("c", [3, 1, 4])
def test_list_mixed_sizes_and_flips(gpu_ctx, c, aa):
    """Seven images of their own sizes in one launch: against numpy, against the dense entry on each image alone, and
    with every other descriptor flipped against the unflipped result with those images' columns reversed."""
    import torch
    import ore
    imgs = [images((hs, ws, c), seed=940 + i) for i, (hs, ws) in enumerate(SIZES)]
    dev = [_cuda(x) for x in imgs]
    scale, shift = _norm(c)
    want = _ref(imgs, GEOMS, OUT, aa, scale, shift)
    with _closing(ore.ImageList(gpu_ctx, 8, OUT, c, antialias=aa, cubic=True)) as (lst,):
        assert ore.load().ore_image_list_filter(lst.h) == (ore.FILTER_BICUBIC_AA if aa else ore.FILTER_BICUBIC)
        lst.set(dev, geometries=GEOMS)
        y = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift)
        _bits_equal(y.cpu().numpy(), want)
        for i, (d, (resized, origin)) in enumerate(zip(dev, GEOMS)):
            alone = ore.preprocess_resize_u8(gpu_ctx, d[None], OUT, resized, origin, scale, shift, antialias=aa, cubic=True)
            torch.cuda.synchronize()
            assert torch.equal(alone[0].view(torch.int32), y[i].view(torch.int32)), i
        if c == 3:
            r = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift, reverse_channels=True)
            _bits_equal(r.cpu().numpy(), _ref(imgs, GEOMS, OUT, aa, scale, shift, reverse=True))
        lst.set(dev, geometries=GEOMS, flips=FLIPS)
        f = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift).cpu().numpy()
        mirrored = np.stack([w[:, :, ::-1] if fl else w for w, fl in zip(want, FLIPS)])
        _bits_equal(f, mirrored, "flipped")


@FILTERS
def test_list_row_strides_alignment_and_overlap(gpu_ctx, aa):
    """Windows of a larger tensor: an odd base address, a row stride above ws*c, and descriptors on overlapping bytes
    of one source."""
    import ore
    big = images((48, 64, 3), seed=950)
    bd = _cuda(big)
    cuts = [(slice(3, 40), slice(5, 50)), (slice(10, 48), slice(0, 33)), (slice(5, 44), slice(7, 60)), (slice(47, 48), slice(63, 64))]
    views = [bd[r, q] for r, q in cuts]
    hosts = [np.ascontiguousarray(big[r, q]) for r, q in cuts]
    assert views[0].data_ptr() % 2 == 1 and views[0].stride(0) == 64 * 3 > 45 * 3 and not views[0].is_contiguous()
    geoms = [((20, 24), (8, 3)), ((12, 20), (0, 0)), ((17, 30), (1, 10)), ((12, 20), (0, 0))]
    scale, shift = _norm(3)
    with _closing(ore.ImageList(gpu_ctx, 4, OUT, 3, antialias=aa, cubic=True)) as (lst,):
        lst.set(views, geometries=geoms)
        y = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift)
        _bits_equal(y.cpu().numpy(), _ref(hosts, geoms, OUT, aa, scale, shift))


def test_list_set_rejects_a_ratio_of_17_by_index(gpu_ctx):
    import ore
    ok, far = _cuda(images((33, 64, 3), seed=951)), _cuda(images((205, 20, 3), seed=952))  # 205 -> 12 is above 16
    g = [((18, 24), (5, 4)), ((12, 20), (0, 0))]
    with _closing(ore.ImageList(gpu_ctx, 2, OUT, 3, antialias=True, cubic=True), ore.ImageList(gpu_ctx, 2, OUT, 3, cubic=True)) as (lst, plain):
        with pytest.raises(ore.OreError, match=r"images\[1\].*at most 16 times, the rows go 205 -> 12"):
            lst.set([ok, far], geometries=g)
        assert lst.count == 0
        plain.set([ok, far], geometries=g)  # the plain cubic list takes it
        assert plain.count == 2


# ---------------------------------------------------------------------------------------------- NV12 and YUV lists
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


NV12_SIZES = [(9, 11), (9, 11), (1, 1), (40, 66)]
NV12_GEOMS = [((12, 20), (0, 0)), ((15, 23), (3, 3)), ((12, 20), (0, 0)), ((12, 20), (0, 0))]


@FILTERS
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_nv12_equals_the_interleaved_list(gpu_ctx, matrix, aa):
    """Odd sizes (the last row and column share a chroma pair with nothing), planes at odd bases and pitches of their
    own: image i is the interleaved cubic list over ore.nv12_to_rgb of the frame, and the numpy reference of it;
    flips included."""
    import ore
    frames = [(images((hs, ws), seed=960 + i), images(((hs + 1) // 2, (ws + 1) // 2, 2), seed=970 + i))
              for i, (hs, ws) in enumerate(NV12_SIZES)]
    rgbs = [ore.nv12_to_rgb(y, uv, matrix) for y, uv in frames]
    scale, shift = _norm(3)
    want = _ref(rgbs, NV12_GEOMS, OUT, aa, scale, shift)
    flips = [False, True, False, True]
    nv = ore.Nv12ImageList(gpu_ctx, 4, OUT, matrix, antialias=aa, cubic=True)
    il = ore.ImageList(gpu_ctx, 4, OUT, 3, antialias=aa, cubic=True)
    with _closing(nv, il):
        assert ore.load().ore_image_list_filter(nv.h) == (257 if aa else 256)
        for pad in (0, 255):
            views = [(_padded(y, pad, 1, 13), _padded(uv, pad, 3, 6)) for y, uv in frames]
            assert all(a.data_ptr() % 2 == 1 and not b.is_contiguous() for a, b in views[:2])
            nv.set(views, geometries=NV12_GEOMS)
            _bits_equal(ore.preprocess_list_u8(gpu_ctx, nv, scale, shift).cpu().numpy(), want, f"pad {pad}")
        il.set([_cuda(x) for x in rgbs], geometries=NV12_GEOMS, flips=flips)
        nv.set(views, geometries=NV12_GEOMS, flips=flips)
        a = ore.preprocess_list_u8(gpu_ctx, nv, scale, shift, reverse_channels=True).cpu().numpy()
        b = ore.preprocess_list_u8(gpu_ctx, il, scale, shift, reverse_channels=True).cpu().numpy()
        _bits_equal(a, b, "against the interleaved list, flipped and reversed")


@FILTERS
def test_yuv_one_list_of_all_eight_layouts(gpu_ctx, aa):
    """Every ore_yuv_format at 10 x 13 in one list (every way to fetch a pixel in one launch): image i is the
    interleaved cubic list over ore.yuv_planes_to_rgb of the frame, and the numpy reference of it; the "nv12"
    descriptor equals the NV12 list's image."""
    import ore
    hs, ws = 10, 13
    planes = [make_planes(fmt, hs, ws, 980 + 10 * i) for i, fmt in enumerate(YUV_NAMES)]
    widths = [yuyv_width(fmt, ws) for fmt in YUV_NAMES]
    rgbs = [ore.yuv_planes_to_rgb(fmt, p, "bt601_full", ws=w) for fmt, p, w in zip(YUV_NAMES, planes, widths)]
    out = (5, 9)
    geoms = [((5, 9), (0, 0)), ((7, 11), (2, 2)), ((14, 24), (9, 15)), ((5, 20), (0, 11))] * 2
    flips = [False, True] * 4
    scale, shift = _norm(3)
    want = _ref(rgbs, geoms, out, aa, scale, shift)
    yl = ore.YuvImageList(gpu_ctx, 8, out, "bt601_full", antialias=aa, cubic=True)
    il = ore.ImageList(gpu_ctx, 8, out, 3, antialias=aa, cubic=True)
    nv = ore.Nv12ImageList(gpu_ctx, 1, out, "bt601_full", antialias=aa, cubic=True)
    with _closing(yl, il, nv):
        assert ore.load().ore_image_list_filter(yl.h) == (257 if aa else 256)
        dev = [frame(fmt, [_cuda(q) for q in p], w) for fmt, p, w in zip(YUV_NAMES, planes, widths)]
        yl.set(dev, geometries=geoms)
        y = ore.preprocess_list_u8(gpu_ctx, yl, scale, shift).cpu().numpy()
        _bits_equal(y, want)
        k = YUV_NAMES.index("nv12")
        nv.set([tuple(dev[k][1:3])], geometries=[geoms[k]])
        _bits_equal(ore.preprocess_list_u8(gpu_ctx, nv, scale, shift).cpu().numpy(), y[k:k + 1], "the NV12 list")
        yl.set(dev, geometries=geoms, flips=flips)
        il.set([_cuda(x) for x in rgbs], geometries=geoms, flips=flips)
        a = ore.preprocess_list_u8(gpu_ctx, yl, scale, shift).cpu().numpy()
        _bits_equal(a, ore.preprocess_list_u8(gpu_ctx, il, scale, shift).cpu().numpy(), "against the interleaved list, flipped")
        _bits_equal(a, np.stack([w[:, :, ::-1] if fl else w for w, fl in zip(want, flips)]), "flipped")


# ---------------------------------------------------------------------------------------------- model
@contextlib.contextmanager
def _model(ctx, onnx_bytes, **kw):
    """A model closed even when the test fails: it must not outlive the session's context."""
    import ore
    m = ore.Model(ctx, onnx_bytes, **kw)
    try:
        yield m
    finally:
        m.close()


M_SRC, M_RESIZED, M_ORIGIN = (150, 170), (72, 96), (4, 16)
M_SIZES = [(150, 170), (64, 64), (200, 90), (40, 51)]
M_GEOMS = [(M_RESIZED, M_ORIGIN), ((64, 64), (0, 0)), ((80, 64), (16, 0)), ((70, 90), (6, 26))]


def _run_u8_and_views(gpu_ctx, aa, precision):
    import torch
    import ore
    from ore import squeezenet
    x = images((3,) + M_SRC + (3,), seed=990)
    scale, shift = _norm(3)
    ref = resize_cubic_ref(x, M_RESIZED, M_ORIGIN, (64, 64), aa, scale, shift)
    xd = _cuda(x)
    with _model(gpu_ctx, squeezenet.build(64), max_batch=4, precision=precision) as m:
        m.set_input_norm(scale, shift)
        steps = len(m.steps())
        m.set_input_resize(M_SRC, M_RESIZED, M_ORIGIN, antialias=aa, cubic=True)
        y_ref = m.run(_cuda(ref)).clone()
        y_u8 = m.run_u8(xd).clone()
        torch.cuda.synchronize()
        assert torch.equal(y_u8, y_ref) and bool(torch.isfinite(y_u8).all()) and len(m.steps()) == steps
        # another filter on the same geometry gives other inputs
        m.set_input_resize(M_SRC, M_RESIZED, M_ORIGIN, antialias=aa)
        y_lin = m.run_u8(xd).clone()
        torch.cuda.synchronize()
        assert not torch.equal(y_lin, y_u8)
        # a cubic list through the _u8_list entries: rows, then two views per group
        imgs = [x[0]] + [images(s + (3,), seed=991 + i) for i, s in enumerate(M_SIZES[1:])]
        flips = [False, True, False, True]
        want_in = _ref(imgs, M_GEOMS, (64, 64), aa, scale, shift)
        want_in = np.stack([w[:, :, ::-1] if fl else w for w, fl in zip(want_in, flips)])
        with _closing(ore.ImageList(gpu_ctx, 4, (64, 64), 3, antialias=aa, cubic=True)) as (lst,):
            lst.set([_cuda(i) for i in imgs], geometries=M_GEOMS, flips=flips)
            rows = m.run(_cuda(want_in)).clone()
            got = m.run_u8_list(lst).clone()
            torch.cuda.synchronize()
            assert torch.equal(got, rows) and torch.equal(got[0], y_u8[0])
            m.set_topk(3)
            m.set_views(2)
            scores, classes = m.classify_u8_list(lst)
            want_s, want_c = ore.topk_mean(gpu_ctx, rows, 2, 3)
            torch.cuda.synchronize()
            assert tuple(scores.shape) == (2, 3)
            assert torch.equal(scores.view(torch.int32), want_s.view(torch.int32)) and torch.equal(classes, want_c)


@FILTERS
def test_model_run_u8_and_views(gpu_ctx, aa):
    """set_input_resize(cubic=True) + run_u8 == run on the numpy-preprocessed floats; run_u8_list on a cubic list
    likewise; classify_u8_list under set_views(2) == topk_mean of those rows."""
    _run_u8_and_views(gpu_ctx, aa, "f32")


def test_model_f16_path(gpu_ctx):
    _run_u8_and_views(gpu_ctx, True, "f16")


@FILTERS
def test_chunked_run_u8(gpu_ctx, aa):
    """On the pattern of test_chunked_run_u8_resized: a batch above run_batch runs in chunks, and chunk i0 must read
    from source image i0."""
    import torch
    import ore
    from ore import squeezenet
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        n = m.run_batch + 5
        assert n <= 2048
        g = torch.Generator(device="cuda").manual_seed(13)
        x = torch.randint(0, 256, (n, 250, 240, 3), dtype=torch.uint8, device="cuda", generator=g)
        scale, shift = _norm(3)
        m.set_input_norm(scale, shift)
        m.set_input_resize((250, 240), (226, 228), (1, 2), antialias=aa, cubic=True)
        want = torch.empty((n, m.output_elems), device="cuda")
        m.run_into(ore.preprocess_resize_u8(gpu_ctx, x, (224, 224), (226, 228), (1, 2), scale, shift, antialias=aa, cubic=True), want)
        got = m.run_u8(x)
        torch.cuda.synchronize()
        assert torch.equal(got, want)


@FILTERS
def test_capture_u8_list_replays_a_new_set(aa):
    """capture_u8_list, replay; then a set of the same count with an image of another size (longer runs than the
    captured ones) and replay again: each equals a direct run.  Graph capture needs a non-null context stream: a
    context of its own on a torch stream."""
    import torch
    import ore
    from ore import squeezenet
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    m = ore.Model(ctx, squeezenet.build(64), max_batch=1)
    lst = ore.ImageList(ctx, 2, (64, 64), 3, antialias=aa, cubic=True)
    try:
        scale, shift = _norm(3)
        m.set_input_norm(scale, shift)
        x1, g1 = images((70, 80, 3), seed=995), ((64, 64), (0, 0))
        x2, g2 = images((700, 90, 3), seed=996), ((80, 64), (16, 0))  # rows at ratio 8.75: 35-tap runs
        d1, d2 = _cuda(x1), _cuda(x2)
        refs = [_cuda(resize_cubic_ref(x[None], g[0], g[1], (64, 64), aa, scale, shift)) for x, g in ((x1, g1), (x2, g2))]
        wants = [torch.empty((1, m.output_elems), device="cuda") for _ in refs]
        out = torch.empty_like(wants[0])
        torch.cuda.synchronize()
        for r, w in zip(refs, wants):
            m.run_into(r, w)
        s.synchronize()
        assert not torch.equal(wants[0], wants[1])
        lst.set([d1], geometries=[g1])
        s.synchronize()
        m.capture_u8_list(lst, out)  # capture only: nothing runs yet
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[0])
        lst.set([d2], geometries=[g2])  # the same count: a new image of a new size
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[1])
    finally:
        s.synchronize()
        lst.close()
        m.close()
        ctx.close()
