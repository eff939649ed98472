"""GPU: the antialiased resize in front of the graph (ore_preprocess_resize_u8_ex, image lists created with
ORE_FILTER_BILINEAR_AA, ore_model_set_input_resize_ex).

The arithmetic is fixed (include/ore.h), so numpy reproduces it bit for bit (tests/_resize_aa_ref.py) and every
comparison here is exact and over all elements.  There is one kernel (one thread per output pixel; resize
variants 0 and 1 both select it), so each case runs once."""
import contextlib
import ctypes

import numpy as np
import pytest

from _resize_aa_ref import resize_aa_ref
from _resize_ref import images

pytestmark = pytest.mark.gpu

_MEAN = np.array([0.485, 0.456, 0.406, 0.5], np.float32)
_STD = np.array([0.229, 0.224, 0.225, 0.25], np.float32)


def _norm(c):
    """ImageNet-style scale and shift for c channels."""
    return ((np.float32(1.0) / (np.float32(255.0) * _STD[:c])).astype(np.float32), (-_MEAN[:c] / _STD[:c]).astype(np.float32))


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# (Hs, Ws), (Rh, Rw), (top, left), (H, W)
GEOMETRIES = [
    ((33, 64), (18, 20), (2, 8), (16, 12)),    # both axes shrink, the crop at the far corner
    ((64, 33), (40, 30), (24, 18), (16, 12)),  # rows shrink, columns are upscaled
    ((31, 17), (31, 5), (0, 0), (31, 5)),      # columns only
    ((7, 5), (3, 2), (0, 0), (3, 2)),          # clipped edge taps
    ((96, 64), (3, 2), (0, 0), (3, 2)),        # ratio exactly 32
]


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("src,resized,origin,out", GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_dense_matches_numpy(gpu_ctx, src, resized, origin, out, c):
    import ore
    x = images((2,) + src + (c,), seed=60)
    xd = _cuda(x)
    scale, shift = _norm(c)
    want = resize_aa_ref(x, resized, origin, out, scale, shift)
    plain = resize_aa_ref(x, resized, origin, out)
    rev = resize_aa_ref(x, resized, origin, out, scale, shift, reverse=True) if c == 3 else None
    y = ore.preprocess_resize_u8(gpu_ctx, xd, out, resized, origin, scale, shift, antialias=True)
    assert tuple(y.shape) == (2, c) + out
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    y = ore.preprocess_resize_u8(gpu_ctx, xd, out, resized, origin, antialias=True)
    np.testing.assert_array_equal(y.cpu().numpy(), plain, err_msg="no norm")
    if c == 3:
        y = ore.preprocess_resize_u8(gpu_ctx, xd, out, resized, origin, scale, shift, reverse_channels=True, antialias=True)
        np.testing.assert_array_equal(y.cpu().numpy(), rev, err_msg="reversed")


def test_five_images_into_a_slice(gpu_ctx):
    """n = 5, y with an image stride of C*H*W + 3 (raw ABI): the elements between images keep their contents."""
    import torch
    import ore
    from ore import _lib
    n, hs, ws, c = shape = (5, 33, 64, 3)
    h, w, gap = 16, 12, 3
    x = images(shape, seed=61)
    xd = _cuda(x)
    scale, shift = _norm(c)
    ref = resize_aa_ref(x, (18, 20), (2, 8), (h, w), scale, shift)
    per = c * h * w
    sentinel = -12345.0
    F = ctypes.c_float * c
    ybuf = torch.full((n, per + gap), sentinel, dtype=torch.float32, device="cuda")
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = ybuf.data_ptr(), 4, per + gap
    for i, d in enumerate((n, c, h, w)):
        t.dims[i] = d
    st = ore.load().ore_preprocess_resize_u8_ex(gpu_ctx.h, ctypes.c_void_p(xd.data_ptr()), n, hs, ws, c,
                                                ctypes.byref(_lib.Resize(18, 20, 2, 8)), ore.FILTER_BILINEAR_AA,
                                                F(*scale.tolist()), F(*shift.tolist()), 0, ctypes.byref(t))
    assert st == 0, ore.load().ore_last_error(gpu_ctx.h)
    got = ybuf.cpu().numpy()
    np.testing.assert_array_equal(got[:, :per].reshape(n, c, h, w), ref)
    np.testing.assert_array_equal(got[:, per:], np.full((n, gap), sentinel, np.float32))


def test_nothing_shrinks_equals_the_plain_entry(gpu_ctx):
    import torch
    import ore
    x = _cuda(images((2, 30, 40, 3), seed=62))
    scale, shift = _norm(3)
    for resized, origin, out in [((30, 40), (2, 3), (11, 13)), ((45, 61), (4, 7), (40, 50))]:
        want = ore.preprocess_resize_u8(gpu_ctx, x, out, resized, origin, scale, shift)
        got = ore.preprocess_resize_u8(gpu_ctx, x, out, resized, origin, scale, shift, antialias=True)
        torch.cuda.synchronize()
        assert torch.equal(got, want)


def test_resize_variants(gpu_ctx):
    """Variants 0 and 1 select the one kernel; 2 (the band kernel, removed) and anything else is refused."""
    import torch
    import ore
    x = images((3, 120, 90, 3), seed=63)  # 120 x 90 -> 50 x 37 whole: several workgroups, the last one partial
    xd = _cuda(x)
    scale, shift = _norm(3)
    try:
        gpu_ctx.set_resize_variant(1)
        y1 = ore.preprocess_resize_u8(gpu_ctx, xd, (50, 37), scale=scale, shift=shift, antialias=True)
        for v in (2, 3, -1):
            with pytest.raises(ore.OreError, match="variant"):
                gpu_ctx.set_resize_variant(v)
    finally:
        gpu_ctx.set_resize_variant(0)
    y0 = ore.preprocess_resize_u8(gpu_ctx, xd, (50, 37), scale=scale, shift=shift, antialias=True)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    np.testing.assert_array_equal(y1.cpu().numpy(), resize_aa_ref(x, (50, 37), (0, 0), (50, 37), scale, shift))


def test_widest_rows(gpu_ctx):
    """8 x 12001 -> 4 x 6000: 36 KB source rows and a 24 KB output row, the column taps far from the origin."""
    import ore
    x = images((1, 8, 12001, 3), seed=64)
    y = ore.preprocess_resize_u8(gpu_ctx, _cuda(x), (4, 6000), antialias=True)
    np.testing.assert_array_equal(y.cpu().numpy(), resize_aa_ref(x, (4, 6000), (0, 0), (4, 6000)))


def test_sixty_four_row_taps_into_a_wide_output(gpu_ctx):
    """640 x 40 -> 20 x 1400: every output row sums 64 source rows while the columns are upscaled."""
    import ore
    x = images((1, 640, 40, 1), seed=65)
    y = ore.preprocess_resize_u8(gpu_ctx, _cuda(x), (20, 1400), antialias=True)
    np.testing.assert_array_equal(y.cpu().numpy(), resize_aa_ref(x, (20, 1400), (0, 0), (20, 1400)))


# ---------------------------------------------------------------------------------------------- lists
@contextlib.contextmanager
def _list(ctx, capacity, out_hw, channels, antialias=True):
    import ore
    lst = ore.ImageList(ctx, capacity, out_hw, channels, antialias=antialias)
    try:
        yield lst
    finally:
        import torch
        torch.cuda.synchronize()  # the launches that read the table have finished
        lst.close()


def _ref(imgs, geoms, out_hw, scale=None, shift=None, reverse=False):
    return np.concatenate([resize_aa_ref(x[None], g[0], g[1], out_hw, scale, shift, reverse) for x, g in zip(imgs, geoms)])


# shrinking and plain images in one list, into 16 x 12
SIZES = [(1, 1), (7, 5), (33, 64), (64, 33), (16, 12), (120, 90), (31, 400)]
GEOMS = [((16, 12), (0, 0)),    # every tap clamped, nothing shrinks
         ((20, 15), (4, 3)),    # up-scale, the far corner
         ((18, 20), (2, 8)),    # both shrink, the far corner
         ((40, 30), (24, 18)),  # rows shrink, columns up
         ((16, 12), (0, 0)),    # the identity
         ((16, 12), (0, 0)),    # strong shrink
         ((31, 13), (9, 1))]    # columns only, ratio 30.8
OUT = (16, 12)


@pytest.mark.parametrize("c", [3, 1, 4])
def test_list_mixed_sizes(gpu_ctx, c):
    import torch
    import ore
    imgs = [images((hs, ws, c), seed=70 + i) for i, (hs, ws) in enumerate(SIZES)]
    dev = [_cuda(x) for x in imgs]
    scale, shift = _norm(c)
    want = _ref(imgs, GEOMS, OUT, scale, shift)
    with _list(gpu_ctx, 8, OUT, c) as lst:
        assert ore.load().ore_image_list_filter(lst.h) == ore.FILTER_BILINEAR_AA
        lst.set(dev, geometries=GEOMS)
        y = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift)
        np.testing.assert_array_equal(y.cpu().numpy(), want)
        # image i equals the dense _ex entry on that image alone
        for i, (d, (resized, origin)) in enumerate(zip(dev, GEOMS)):
            alone = ore.preprocess_resize_u8(gpu_ctx, d[None], OUT, resized, origin, scale, shift, antialias=True)
            torch.cuda.synchronize()
            assert torch.equal(alone[0], y[i]), i
        if c == 3:
            y = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift, reverse_channels=True)
            np.testing.assert_array_equal(y.cpu().numpy(), _ref(imgs, GEOMS, OUT, scale, shift, reverse=True))
    with _list(gpu_ctx, 8, OUT, c, antialias=False) as plain:  # ore_image_list_create's list is bilinear
        assert ore.load().ore_image_list_filter(plain.h) == ore.FILTER_BILINEAR


def test_list_row_strides_alignment_and_overlap(gpu_ctx):
    """Windows of a larger tensor: an odd base address, a row stride above ws*c, and two descriptors on
    overlapping bytes of one source."""
    import ore
    big = images((48, 64, 3), seed=71)
    bd = _cuda(big)
    views = [bd[3:40, 5:50], bd[10:48, 0:33], bd[5:44, 7:60], bd[47:48, 63:64]]
    hosts = [big[3:40, 5:50], big[10:48, 0:33], big[5:44, 7:60], big[47:48, 63:64]]
    assert views[0].data_ptr() % 2 == 1 and views[0].stride(0) == 64 * 3 > 45 * 3 and not views[0].is_contiguous()
    geoms = [((20, 24), (2, 3)), ((16, 12), (0, 0)), ((17, 30), (1, 18)), ((16, 12), (0, 0))]
    scale, shift = _norm(3)
    want = _ref([np.ascontiguousarray(h) for h in hosts], geoms, OUT, scale, shift)
    with _list(gpu_ctx, 4, OUT, 3) as lst:
        lst.set(views, geometries=geoms)
        y = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift)
        np.testing.assert_array_equal(y.cpu().numpy(), want)


def test_list_set_rejects_a_ratio_of_33_by_index(gpu_ctx):
    import ore
    a = [images((33, 64, 3), seed=72), images((64, 33, 3), seed=73)]
    ga = [((18, 20), (2, 8)), ((40, 30), (24, 18))]
    da = [_cuda(x) for x in a]
    far = _cuda(images((528, 20, 3), seed=74))  # 528 -> 16 is 33
    want = _ref(a, ga, OUT)
    with _list(gpu_ctx, 2, OUT, 3) as lst:
        lst.set(da, geometries=ga)
        with pytest.raises(ore.OreError, match=r"images\[1\].*rows go 528 -> 16"):  # the host mirror of the rule
            lst.set([da[0], far], geometries=[ga[0], ((16, 12), (0, 0))])
        from ore import _lib
        arr = (_lib.ImageU8 * 2)()
        for i, (x, g) in enumerate(zip([da[0], far], [ga[0], ((16, 12), (0, 0))])):
            arr[i].data, arr[i].hs, arr[i].ws, arr[i].row_stride = x.data_ptr(), x.shape[0], x.shape[1], x.stride(0)
            arr[i].g = _lib.Resize(g[0][0], g[0][1], g[1][0], g[1][1])
        L = ore.load()
        assert L.ore_image_list_set(lst.h, arr, 2) == 1  # the library's own check
        assert b"image 1" in L.ore_last_error(gpu_ctx.h) and b"rows" in L.ore_last_error(gpu_ctx.h)
        assert lst.count == 2
        np.testing.assert_array_equal(ore.preprocess_list_u8(gpu_ctx, lst).cpu().numpy(), want)  # the previous content
    with _list(gpu_ctx, 2, OUT, 3, antialias=False) as plain:  # the plain list takes it
        plain.set([da[0], far], geometries=[ga[0], ((16, 12), (0, 0))])
        assert plain.count == 2


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


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_model_run_u8_antialiased(gpu_ctx, precision):
    """run_u8 on the source batch == run(preprocess_resize_u8(antialias=True)) == run(the numpy tensor); classify_u8
    == topk of those rows; the plain filter on the same geometry gives other inputs; run_u8_list likewise."""
    import torch
    import ore
    from ore import squeezenet
    x = images((3, 150, 170, 3), seed=80)
    resized, origin = (72, 96), (4, 16)
    scale, shift = _norm(3)
    ref = resize_aa_ref(x, resized, origin, (64, 64), scale, shift)
    xd = _cuda(x)
    with _model(gpu_ctx, squeezenet.build(64), max_batch=4, precision=precision) as m:
        m.set_input_norm(scale, shift)
        steps = len(m.steps())
        m.set_input_resize((150, 170), resized, origin, antialias=True)
        y_ref = m.run(_cuda(ref)).clone()
        y_pre = m.run(ore.preprocess_resize_u8(gpu_ctx, xd, (64, 64), resized, origin, scale, shift, antialias=True)).clone()
        y_u8 = m.run_u8(xd).clone()
        torch.cuda.synchronize()
        assert torch.equal(y_u8, y_pre) and torch.equal(y_u8, y_ref)
        assert bool(torch.isfinite(y_u8).all()) and len(m.steps()) == steps
        m.set_topk(3)
        scores, classes = m.classify_u8(xd)
        want_s, want_c = ore.topk(gpu_ctx, y_u8, 3)
        torch.cuda.synchronize()
        assert torch.equal(scores, want_s) and torch.equal(classes, want_c)
        # a rejected geometry or filter leaves the current ones in place
        assert ore.load().ore_model_set_input_resize_ex(m.h, 150, 170, ctypes.byref(ore._lib.Resize(4, 96, 0, 0)), 1) == 1
        assert ore.load().ore_model_set_input_resize_ex(m.h, 150, 170, ctypes.byref(ore._lib.Resize(72, 96, 4, 16)), 5) == 1
        assert torch.equal(m.run_u8(xd), y_u8)
        # ore_model_set_input_resize means bilinear
        m.set_input_resize((150, 170), resized, origin)
        y_plain = m.run_u8(xd).clone()
        want_plain = m.run(ore.preprocess_resize_u8(gpu_ctx, xd, (64, 64), resized, origin, scale, shift)).clone()
        torch.cuda.synchronize()
        assert torch.equal(y_plain, want_plain) and not torch.equal(y_plain, y_u8)
        # an antialiased list through the _u8_list entries; the resize of the pointer entries is not theirs
        imgs = [x[0], images((64, 64, 3), seed=81), images((200, 90, 3), seed=82)]
        geoms = [(resized, origin), ((64, 64), (0, 0)), ((80, 64), (16, 0))]
        with _list(gpu_ctx, 4, (64, 64), 3) as lst:
            lst.set([_cuda(i) for i in imgs], geometries=geoms)
            want = m.run(_cuda(_ref(imgs, geoms, (64, 64), scale, shift))).clone()
            got = m.run_u8_list(lst).clone()
            torch.cuda.synchronize()
            assert torch.equal(got, want) and torch.equal(got[0], y_u8[0])
            scores, classes = m.classify_u8_list(lst)
            want_s, want_c = ore.topk(gpu_ctx, got, 3)
            torch.cuda.synchronize()
            assert torch.equal(scores, want_s) and torch.equal(classes, want_c)


def test_chunked_run_u8_antialiased(gpu_ctx):
    """On the pattern of test_chunked_run_u8_resized: chunk i0 must read from source image i0."""
    import torch
    import ore
    from ore import squeezenet
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        n = m.run_batch + 5
        assert n <= 2048
        g = torch.Generator(device="cuda").manual_seed(12)
        x = torch.randint(0, 256, (n, 250, 240, 3), dtype=torch.uint8, device="cuda", generator=g)
        scale, shift = _norm(3)
        m.set_input_norm(scale, shift)
        m.set_input_resize((250, 240), (226, 228), (1, 2), antialias=True)
        want = torch.empty((n, m.output_elems), device="cuda")
        m.run_into(ore.preprocess_resize_u8(gpu_ctx, x, (224, 224), (226, 228), (1, 2), scale, shift, antialias=True), want)
        got = m.run_u8(x)
        torch.cuda.synchronize()
        assert torch.equal(got, want)


def test_captures_keep_the_filter():
    """capture_u8 then launch on the buffer's current contents; capture_u8_list with a re-set of the same count.
    Graph capture needs a non-null context stream: a context of its own on a torch stream."""
    import torch
    import ore
    from ore import squeezenet
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    m = ore.Model(ctx, squeezenet.build(64), max_batch=1)
    lst = ore.ImageList(ctx, 2, (64, 64), 3, antialias=True)
    try:
        scale, shift = _norm(3)
        resized, origin = (72, 96), (4, 16)
        m.set_input_norm(scale, shift, reverse_channels=True)
        m.set_input_resize((150, 170), resized, origin, antialias=True)
        x1, x2 = images((1, 150, 170, 3), seed=83), images((1, 150, 170, 3), seed=84)
        x3, g3 = images((200, 90, 3), seed=85), ((80, 64), (16, 0))
        refs = [_cuda(resize_aa_ref(x, resized, origin, (64, 64), scale, shift, reverse=True)) for x in (x1, x2)]
        refs.append(_cuda(resize_aa_ref(x3[None], g3[0], g3[1], (64, 64), scale, shift, reverse=True)))
        d1, d2, d3 = _cuda(x1), _cuda(x2), _cuda(x3)
        buf = d1.clone()
        wants = [torch.empty((1, m.output_elems), device="cuda") for _ in refs]
        out = torch.empty_like(wants[0])
        torch.cuda.synchronize()
        for r, w in zip(refs, wants):
            m.run_into(r, w)
        s.synchronize()
        assert not torch.equal(wants[0], wants[1])
        m.capture_u8(buf, out)  # capture only: nothing runs yet
        m.set_input_resize((150, 170), resized, origin)  # the graph keeps the filter it was captured with
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[0])
        buf.copy_(d2)  # in place: the graph keeps the pointer
        torch.cuda.synchronize()
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[1])
        lst.set([d1[0]], geometries=[(resized, origin)])
        s.synchronize()
        m.capture_u8_list(lst, out)
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[0])
        lst.set([d3], geometries=[g3])  # the same count: a new image of a new size
        m.replay()
        s.synchronize()
        assert torch.equal(out, wants[2])
    finally:
        s.synchronize()
        lst.close()
        m.close()
        ctx.close()
