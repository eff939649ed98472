"""GPU: image lists -- uint8 images of different sizes, row strides and geometries in one launch
(ore_image_list_*, ore_preprocess_list_u8, the model's _u8_list entries).

Image i of a list is defined as the bits ore_preprocess_resize_u8 gives for a dense copy of that image alone,
which is tests/_resize_ref.py::resize_ref: every comparison here is exact and over all elements.  No descriptor
in this file points outside its tensor: every one is made from a torch tensor or a view of one."""
import contextlib
import ctypes
import os
import warnings

import numpy as np
import pytest

from _resize_ref import images, resize_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

_MEAN = np.array([0.485, 0.456, 0.406, 0.5], np.float32)
_STD = np.array([0.229, 0.224, 0.225, 0.25], np.float32)


def _norm(c):
    """ImageNet-style scale and shift for c channels."""
    return ((np.float32(1.0) / (np.float32(255.0) * _STD[:c])).astype(np.float32), (-_MEAN[:c] / _STD[:c]).astype(np.float32))


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ref(imgs, geoms, out_hw, scale=None, shift=None, reverse=False):
    """The list's definition: resize_ref of every image alone, stacked."""
    return np.concatenate([resize_ref(x[None], g[0], g[1], out_hw, scale, shift, reverse) for x, g in zip(imgs, geoms)])


@contextlib.contextmanager
def _list(ctx, capacity, out_hw, channels):
    import ore
    lst = ore.ImageList(ctx, capacity, out_hw, channels)
    try:
        yield lst
    finally:
        import torch
        torch.cuda.synchronize()  # the launches that read the table have finished
        lst.close()


# seven sizes into 16 x 12, each with its own geometry (resized_hw, origin)
SIZES = [(1, 1), (7, 5), (5, 7), (33, 64), (64, 33), (16, 12), (120, 90)]
GEOMS = [((16, 12), (0, 0)),    # every tap clamped
         ((20, 15), (4, 3)),    # up-scale, the crop at the far corner: top + h == rh, left + w == rw
         ((16, 12), (0, 0)),    # up-scale
         ((18, 20), (1, 4)),    # down-scale with a crop
         ((40, 30), (24, 18)),  # rows down, the far corner again
         ((16, 12), (0, 0)),    # the identity
         ((16, 12), (0, 0))]    # strong down-scale: skipped rows and columns
OUT = (16, 12)


@pytest.mark.parametrize("c", [3, 1, 4])
def test_mixed_sizes(gpu_ctx, c):
    import ore
    imgs = [images((hs, ws, c), seed=40 + i) for i, (hs, ws) in enumerate(SIZES)]
    dev = [_cuda(x) for x in imgs]
    scale, shift = _norm(c)
    with _list(gpu_ctx, 8, OUT, c) as lst:
        assert lst.count == 0
        lst.set(dev, geometries=GEOMS)
        assert lst.count == 7
        y = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift)
        assert tuple(y.shape) == (7, c) + OUT
        np.testing.assert_array_equal(y.cpu().numpy(), _ref(imgs, GEOMS, OUT, scale, shift))
        # defaults: scale 1, shift 0
        np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, lst).cpu().numpy(), _ref(imgs, GEOMS, OUT))
        if c == 3:
            y = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift, reverse_channels=True)
            np.testing.assert_array_equal(y.cpu().numpy(), _ref(imgs, GEOMS, OUT, scale, shift, reverse=True))
        else:
            with pytest.raises(ore.OreError, match="3 channels"):
                ore.preprocess_list_u8(gpu_ctx, lst, reverse_channels=True)
        # the other two ways to state the geometry: a plain resize, and short= per image
        big = [d for d, (hs, ws) in zip(dev, SIZES) if min(hs, ws) >= 16]
        bigs = [x for x, (hs, ws) in zip(imgs, SIZES) if min(hs, ws) >= 16]
        lst.set(dev)
        np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, lst, scale, shift).cpu().numpy(),
                                      _ref(imgs, [(OUT, (0, 0))] * 7, OUT, scale, shift))
        lst.set(big, short=18)
        assert lst.count == len(big) == 3
        want = [ore.center_crop_geometry(x.shape[:2], 18, OUT) for x in bigs]
        np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, lst, scale, shift).cpu().numpy(),
                                      _ref(bigs, want, OUT, scale, shift))
        lst.set([])
        assert lst.count == 0 and tuple(ore.preprocess_list_u8(gpu_ctx, lst).shape) == (0, c) + OUT


def test_row_strides_and_alignment(gpu_ctx):
    """Windows of a larger tensor: an odd base address, a row stride above ws*c, and two descriptors on
    overlapping bytes of one source."""
    import ore
    big = images((48, 64, 3), seed=50)
    bd = _cuda(big)
    views = [bd[3:40, 5:50], bd[10:48, 0:33], bd[3:40, 5:50], bd[47:48, 63:64]]
    hosts = [big[3:40, 5:50], big[10:48, 0:33], big[3:40, 5:50], big[47:48, 63:64]]
    assert views[0].data_ptr() % 2 == 1 and views[0].stride(0) == 64 * 3 > 45 * 3 and not views[0].is_contiguous()
    geoms = [((20, 24), (2, 3)), ((16, 12), (0, 0)), ((37, 45), (21, 33)), ((16, 12), (0, 0))]
    scale, shift = _norm(3)
    with _list(gpu_ctx, 4, OUT, 3) as lst:
        lst.set(views, geometries=geoms)
        y = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift)
        np.testing.assert_array_equal(y.cpu().numpy(), _ref([np.ascontiguousarray(h) for h in hosts], geoms, OUT, scale, shift))


def test_equals_the_dense_entry(gpu_ctx):
    import torch
    import ore
    x = images((4, 30, 41, 3), seed=51)
    xd = _cuda(x)
    scale, shift = _norm(3)
    want = ore.preprocess_resize_u8(gpu_ctx, xd, (20, 32), (24, 36), (2, 3), scale, shift)
    with _list(gpu_ctx, 4, (20, 32), 3) as lst:
        lst.set([xd[i] for i in range(4)], geometries=[((24, 36), (2, 3))] * 4)
        got = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift)
        torch.cuda.synchronize()
        assert torch.equal(got, want)


@pytest.mark.parametrize("gap", [8, 3], ids=["aligned-gap", "odd-gap"])
def test_list_into_slice(gpu_ctx, gap):
    """y with an image stride above C*H*W (raw ABI): the elements between images keep their contents."""
    import torch
    import ore
    from ore import _lib
    c = 3
    imgs = [images((hs, ws, c), seed=52 + i) for i, (hs, ws) in enumerate(SIZES[1:5])]
    geoms = GEOMS[1:5]
    dev = [_cuda(x) for x in imgs]
    scale, shift = _norm(c)
    n, (h, w) = len(imgs), OUT
    per = c * h * w
    sentinel = -12345.0
    F = ctypes.c_float * c
    ybuf = torch.full((n, per + gap), sentinel, dtype=torch.float32, device="cuda")
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = ybuf.data_ptr(), 4, per + gap
    for i, d in enumerate((n, c, h, w)):
        t.dims[i] = d
    L = ore.load()
    with _list(gpu_ctx, n, OUT, c) as lst:
        lst.set(dev, geometries=geoms)
        t.nstride = per - 1
        assert L.ore_preprocess_list_u8(gpu_ctx.h, lst.h, None, None, 0, ctypes.byref(t)) == 1
        assert b"stride" in L.ore_last_error(gpu_ctx.h)
        t.dims[0] = n + 1
        assert L.ore_preprocess_list_u8(gpu_ctx.h, lst.h, None, None, 0, ctypes.byref(t)) == 1  # not [count, ...]
        t.dims[0], t.nstride = n, per + gap
        assert L.ore_preprocess_list_u8(gpu_ctx.h, lst.h, None, None, 2, ctypes.byref(t)) == 1
        assert b"flags" in L.ore_last_error(gpu_ctx.h)
        st = L.ore_preprocess_list_u8(gpu_ctx.h, lst.h, F(*scale.tolist()), F(*shift.tolist()), 0, ctypes.byref(t))
        assert st == 0, L.ore_last_error(gpu_ctx.h)
        got = ybuf.cpu().numpy()
    np.testing.assert_array_equal(got[:, :per].reshape(n, c, h, w), _ref(imgs, geoms, OUT, scale, shift))
    np.testing.assert_array_equal(got[:, per:], np.full((n, gap), sentinel, np.float32))


def test_past_the_grid_limit(gpu_ctx):
    """65,539 descriptors, more than a grid's 65,535 rows: the blockIdx.y loop and the 64-bit table index."""
    import ore
    n = 65539
    pool_sizes = [(3, 5), (6, 4), (2, 2), (9, 7), (1, 8)]
    pool = [images((hs, ws, 3), seed=60 + i) for i, (hs, ws) in enumerate(pool_sizes)]
    dev = [_cuda(x) for x in pool]
    geoms = [((2, 2), (0, 0)), ((3, 3), (1, 1)), ((2, 2), (0, 0)), ((4, 2), (2, 0)), ((2, 5), (0, 3))]
    refs = _ref(pool, geoms, (2, 2))  # [5, 3, 2, 2]
    idx = np.arange(n) % 5
    with _list(gpu_ctx, n, (2, 2), 3) as lst:
        lst.set([dev[i] for i in idx], geometries=[geoms[i] for i in idx])
        assert lst.count == n
        y = ore.preprocess_list_u8(gpu_ctx, lst).cpu().numpy()
    np.testing.assert_array_equal(y, refs[idx])


def _fill(arr, tensors, geoms):
    from ore import _lib
    for i, (x, g) in enumerate(zip(tensors, geoms)):
        arr[i].data = x.data_ptr()
        arr[i].hs, arr[i].ws, arr[i].row_stride = int(x.shape[0]), int(x.shape[1]), int(x.stride(0))
        arr[i].g = _lib.Resize(g[0][0], g[0][1], g[1][0], g[1][1])


def test_set_semantics(gpu_ctx):
    import torch
    import ore
    from ore import _lib
    L = ore.load()
    a = [images((hs, ws, 3), seed=70 + i) for i, (hs, ws) in enumerate(SIZES[1:4])]
    b = [images((hs, ws, 3), seed=75 + i) for i, (hs, ws) in enumerate(SIZES[4:7])]
    ga, gb = GEOMS[1:4], GEOMS[4:7]
    da, db = [_cuda(x) for x in a], [_cuda(x) for x in b]
    ref_a, ref_b = _ref(a, ga, OUT), _ref(b, gb, OUT)
    with _list(gpu_ctx, 3, OUT, 3) as lst:
        lst.set(da, geometries=ga)
        # a rejected set leaves the content and the count in place
        with pytest.raises(ore.OreError, match="image 2.*outside"):
            lst.set(db, geometries=[gb[0], gb[1], ((16, 12), (1, 0))])
        with pytest.raises(ore.OreError, match="capacity"):
            lst.set(db + db[:1], geometries=gb + gb[:1])
        arr4 = (_lib.ImageU8 * 4)()
        _fill(arr4, db + db[:1], gb + gb[:1])
        assert L.ore_image_list_set(lst.h, arr4, 4) == 1 and b"capacity" in L.ore_last_error(gpu_ctx.h)  # the library's own check
        assert L.ore_image_list_set(lst.h, None, 2) == 1
        assert L.ore_image_list_set(lst.h, arr4, -1) == 1
        assert lst.count == 3
        np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, lst).cpu().numpy(), ref_a)

        # set, run, set, run without a sync in between: each run reads its own table, and the descriptor array
        # is the caller's again as soon as set returns
        arr = (_lib.ImageU8 * 3)()
        torch.cuda.synchronize()
        _fill(arr, db, gb)
        assert L.ore_image_list_set(lst.h, arr, 3) == 0
        _fill(arr, da, ga)  # overwritten right away
        y1 = ore.preprocess_list_u8(gpu_ctx, lst)
        assert L.ore_image_list_set(lst.h, arr, 3) == 0
        ctypes.memset(arr, 0, ctypes.sizeof(arr))
        y2 = ore.preprocess_list_u8(gpu_ctx, lst)
        _fill(arr, db[:2], gb[:2])
        assert L.ore_image_list_set(lst.h, arr, 2) == 0
        ctypes.memset(arr, 0, ctypes.sizeof(arr))
        y3 = ore.preprocess_list_u8(gpu_ctx, lst)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(y1.cpu().numpy(), ref_b)
        np.testing.assert_array_equal(y2.cpu().numpy(), ref_a)
        np.testing.assert_array_equal(y3.cpu().numpy(), ref_b[:2])


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


def _model_list_checks(ctx, m, imgs, geoms, scale, shift):
    """run_u8_list == run(preprocess_list_u8(...)) == run(the numpy tensor), bit for bit; classify_u8_list == topk
    of those rows; the step list and a set_input_resize made before are untouched (on the pattern of
    _model_resize_checks)."""
    import torch
    import ore
    c, h, w = m.input_dims
    ref = _ref(imgs, geoms, (h, w), scale, shift)
    dev = [_cuda(x) for x in imgs]
    m.set_input_norm(scale, shift)
    src = images((2, 40, 50, c), seed=80)
    m.set_input_resize((40, 50), (h + 4, w + 8), (2, 4))
    before = m.run_u8(_cuda(src)).clone()
    steps = len(m.steps())
    with _list(ctx, 4, (h, w), c) as lst, _list(ctx, 4, (h, w + 1), c) as wrong:
        lst.set(dev, geometries=geoms)
        y_ref = m.run(_cuda(ref)).clone()
        y_pre = m.run(ore.preprocess_list_u8(ctx, lst, scale, shift)).clone()
        y_list = m.run_u8_list(lst).clone()
        torch.cuda.synchronize()
        assert tuple(y_list.shape) == (len(imgs), m.output_elems)
        assert torch.equal(y_list, y_pre) and torch.equal(y_list, y_ref)
        assert bool(torch.isfinite(y_list).all())
        assert len(m.steps()) == steps  # the conversion is not an exec step
        k = min(3, m.output_elems)
        m.set_topk(k)
        scores, classes = m.classify_u8_list(lst)
        want_s, want_c = ore.topk(ctx, y_list, k)
        torch.cuda.synchronize()
        assert torch.equal(scores, want_s) and torch.equal(classes, want_c)
        # the resize of the pointer entries is still in force, and still theirs alone
        after = m.run_u8(_cuda(src))
        torch.cuda.synchronize()
        assert torch.equal(after, before) and m.input_src_hw == (40, 50)
        # a list of another output shape, or of another context
        wrong.set([_cuda(images((9, 9, c), seed=81))])
        out = torch.empty((4, m.output_elems), device="cuda")
        with pytest.raises(ore.OreError):
            m.run_u8_list(wrong)
        assert ore.load().ore_model_run_u8_list(m.h, wrong.h, ctypes.c_void_p(out.data_ptr())) == 1
        assert ore.load().ore_model_classify_u8_list(m.h, wrong.h, ctypes.c_void_p(scores.data_ptr()),
                                                     ctypes.c_void_p(classes.data_ptr())) == 1
        ctx2 = ore.Context(0)
        try:
            with _list(ctx2, 4, (h, w), c) as other:
                other.set(dev, geometries=geoms)
                with pytest.raises(ore.OreError, match="context"):
                    m.run_u8_list(other)
                with pytest.raises(ore.OreError, match="context"):
                    ore.preprocess_list_u8(ctx, other)
                assert ore.load().ore_model_run_u8_list(m.h, other.h, ctypes.c_void_p(out.data_ptr())) == 1
                assert b"context" in ore.load().ore_last_error(ctx.h)
        finally:
            ctx2.close()
        assert torch.equal(m.run_u8_list_into(lst, out)[:len(imgs)], y_list)
        torch.cuda.synchronize()


def test_mnist_run_u8_list(gpu_ctx):
    with open(os.path.join(GOLD, "mnist-8.onnx"), "rb") as f:
        onnx = f.read()
    imgs = [images(s + (1,), seed=82 + i) for i, s in enumerate([(40, 50), (28, 28), (19, 33)])]
    geoms = [((32, 36), (2, 4)), ((28, 28), (0, 0)), ((30, 40), (2, 12))]
    with _model(gpu_ctx, onnx, max_batch=4) as m:
        assert m.input_dims == (1, 28, 28)
        _model_list_checks(gpu_ctx, m, imgs, geoms, np.array([1.0 / 255.0], np.float32), np.array([-0.5], np.float32))


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_squeezenet_run_u8_list(gpu_ctx, precision):
    from ore import squeezenet
    imgs = [images(s + (3,), seed=85 + i) for i, s in enumerate([(90, 120), (64, 64), (50, 70)])]
    geoms = [((72, 96), (4, 16)), ((64, 64), (0, 0)), ((80, 112), (16, 48))]
    scale, shift = _norm(3)
    with _model(gpu_ctx, squeezenet.build(64), max_batch=4, precision=precision) as m:
        _model_list_checks(gpu_ctx, m, imgs, geoms, scale, shift)


def test_chunked_run_u8_list(gpu_ctx):
    """On the pattern of test_chunked_run_u8_resized: a list above run_batch goes in chunks, and chunk i0 must
    start at descriptor i0 -- the descriptors cycle over seven sources of different sizes, and the chunk length
    is no multiple of seven."""
    import torch
    import ore
    from ore import squeezenet
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        n = m.run_batch + 5
        if ((n + 1) // 2) % 7 == 0:
            n += 1
        assert n <= 2048 and m.run_batch < n <= 2 * m.run_batch
        g = torch.Generator(device="cuda").manual_seed(11)
        sizes = [(230, 236), (224, 224), (250, 231), (300, 226), (225, 333), (240, 240), (227, 229)]
        pool = [torch.randint(0, 256, (hs, ws, 3), dtype=torch.uint8, device="cuda", generator=g) for hs, ws in sizes]
        geoms = [((226, 228), (1, 2)), ((224, 224), (0, 0)), ((240, 224), (16, 0)), ((224, 224), (0, 0)),
                 ((224, 300), (0, 76)), ((230, 230), (3, 3)), ((224, 224), (0, 0))]
        scale, shift = _norm(3)
        m.set_input_norm(scale, shift)
        with _list(gpu_ctx, n, (224, 224), 3) as lst:
            lst.set([pool[i % 7] for i in range(n)], geometries=[geoms[i % 7] for i in range(n)])
            want = torch.empty((n, m.output_elems), device="cuda")
            m.run_into(ore.preprocess_list_u8(gpu_ctx, lst, scale, shift), want)
            got = m.run_u8_list(lst)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
            assert not torch.equal(got[0], got[1])  # the sources do differ


@pytest.mark.parametrize("classify", [False, True], ids=["run", "classify"])
def test_capture_u8_list_replays_current_table(classify):
    """On the pattern of test_capture_u8_resized_replays_current_buffer: the graph reads the table at replay, so
    a set with the same count followed by a replay runs a new image of a new size; another count is refused."""
    import torch
    import ore
    from ore import squeezenet
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    m = ore.Model(ctx, squeezenet.build(64), max_batch=1)
    lst = ore.ImageList(ctx, 2, (64, 64), 3)
    try:
        scale, shift = np.ones(3, np.float32), -np.array([104.0, 117.0, 123.0], np.float32)
        m.set_input_norm(scale, shift, reverse_channels=True)
        m.set_input_resize((33, 44), (64, 64), (0, 0))  # ignored by the list entries
        x1, g1 = images((90, 120, 3), seed=90), ((72, 96), (4, 16))
        x2, g2 = images((70, 50, 3), seed=91), ((80, 64), (16, 0))
        refs = [_cuda(_ref([x], [g], (64, 64), scale, shift, reverse=True)) for x, g in ((x1, g1), (x2, g2))]
        d1, d2 = _cuda(x1), _cuda(x2)
        want1 = torch.empty((1, m.output_elems), device="cuda")
        want2 = torch.empty_like(want1)
        torch.cuda.synchronize()
        m.run_into(refs[0], want1)
        m.run_into(refs[1], want2)
        s.synchronize()
        assert not torch.equal(want1, want2)
        lst.set([d1], geometries=[g1])
        if classify:
            m.set_topk(3)
            scores = torch.empty((1, 3), dtype=torch.float32, device="cuda")
            classes = torch.empty((1, 3), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            m.capture_classify_u8_list(lst, scores, classes)  # capture only: nothing runs yet

            def check(want):
                ws, wc = ore.topk(ctx, want, 3)
                s.synchronize()
                assert torch.equal(scores, ws) and torch.equal(classes, wc)
        else:
            out = torch.empty_like(want1)
            torch.cuda.synchronize()
            m.capture_u8_list(lst, out)

            def check(want):
                assert torch.equal(out, want)
        m.replay()
        s.synchronize()
        check(want1)
        lst.set([d2], geometries=[g2])  # the same count: a new image of a new size
        m.replay()
        s.synchronize()
        check(want2)
        lst.set([])
        with pytest.raises(ore.OreError, match="captured on a list of 1"):
            m.replay()
        lst.set([d1, d2], geometries=[g1, g2])
        with pytest.raises(ore.OreError, match="captured on a list of 1"):
            m.replay()
        lst.set([d1], geometries=[g1])
        m.replay()
        s.synchronize()
        check(want1)
        # a set inside a stream capture is refused, and leaves the list as it was
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(ore.OreError, match="capture"):
                    lst.set([d2], geometries=[g2])
            finally:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # torch remarks that the captured graph is empty: it is meant to be
                    g.capture_end()
        assert lst.count == 1
    finally:
        s.synchronize()
        m.close()
        lst.close()
        ctx.close()
