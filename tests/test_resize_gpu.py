"""GPU: resize + crop of uint8 NHWC batches in front of the graph (ore_preprocess_resize_u8,
ore_model_set_input_resize).

The arithmetic is fixed (include/ore.h: integer taps, every float32 operation rounded on its own), so numpy
reproduces it bit for bit (tests/_resize_ref.py) and every comparison here is exact: a tolerance would hide a
shifted tap.  There is one kernel (one thread per output pixel), so each case runs once."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from _resize_ref import images, resize_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

_MEAN = np.array([0.485, 0.456, 0.406, 0.5], np.float32)
_STD = np.array([0.229, 0.224, 0.225, 0.25], np.float32)


def _norms(c):
    """(name, scale, shift) for c channels: ImageNet style and Caffe style."""
    imagenet = ((np.float32(1.0) / (np.float32(255.0) * _STD[:c])).astype(np.float32),
                (-_MEAN[:c] / _STD[:c]).astype(np.float32))
    caffe = (np.ones(c, np.float32), -np.array([104.0, 117.0, 123.0, 110.0], np.float32)[:c])
    return [("imagenet",) + imagenet, ("caffe",) + caffe]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# (n, Hs, Ws, C), (Rh, Rw), (top, left), (H, W)
GEOMETRIES = [
    ((2, 7, 5, 3), (16, 12), (0, 0), (16, 12)),        # upscale, 15-byte rows
    ((2, 30, 40, 3), (17, 23), (2, 3), (11, 13)),      # odd W, unaligned stores
    ((2, 64, 64, 3), (64, 64), (3, 5), (20, 32)),      # a plain crop
    ((2, 3, 1, 1), (9, 4), (0, 0), (9, 4)),            # every tap clamped
    ((2, 97, 131, 3), (8, 8), (0, 0), (8, 8)),         # skipped rows
    ((2, 1, 1, 4), (4, 4), (0, 0), (4, 4)),
    ((2, 21, 34, 2), (12, 20), (0, 0), (12, 20)),
    ((2, 61, 83, 4), (40, 52), (1, 4), (36, 44)),
    ((2, 375, 500, 3), (256, 341), (16, 58), (224, 224)),  # the workload's geometry
    ((3, 200, 48, 3), (37, 24), (1, 0), (35, 24)),     # strong row downscale, three images
    ((1, 40, 36, 1), (80, 72), (7, 4), (66, 64)),      # upscale with a crop, one channel
]


def _gid(v):
    return "x".join(map(str, v))


@pytest.mark.parametrize("shape,resized,origin,out", GEOMETRIES, ids=_gid)
def test_resize_matches_numpy(gpu_ctx, shape, resized, origin, out):
    import ore
    c = shape[3]
    x = images(shape, seed=20)
    xd = _cuda(x)
    for name, scale, shift in _norms(c):
        y = ore.preprocess_resize_u8(gpu_ctx, xd, out, resized, origin, scale, shift)
        assert tuple(y.shape) == (shape[0], c) + tuple(out)
        np.testing.assert_array_equal(y.cpu().numpy(), resize_ref(x, resized, origin, out, scale, shift), err_msg=name)
    # defaults: scale 1, shift 0
    np.testing.assert_array_equal(ore.preprocess_resize_u8(gpu_ctx, xd, out, resized, origin).cpu().numpy(),
                                  resize_ref(x, resized, origin, out))


def test_identity_resize_equals_preprocess_u8_of_the_slice(gpu_ctx):
    """Rh, Rw = Hs, Ws: the cropped bytes, converted exactly as ore_preprocess_u8 converts them."""
    import ore
    x = images((2, 64, 64, 3), seed=21)
    _, scale, shift = _norms(3)[0]
    want = ore.preprocess_u8(gpu_ctx, _cuda(x[:, 3:23, 5:37]), scale, shift)
    got = ore.preprocess_resize_u8(gpu_ctx, _cuda(x), (20, 32), (64, 64), (3, 5), scale, shift)
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_plain_resize_default_geometry(gpu_ctx):
    import ore
    x = images((2, 30, 40, 3), seed=22)
    got = ore.preprocess_resize_u8(gpu_ctx, _cuda(x), (16, 24))
    np.testing.assert_array_equal(got.cpu().numpy(), resize_ref(x, (16, 24), (0, 0), (16, 24)))


def test_widest_rows(gpu_ctx):
    """Source rows of 16384 pixels x 4 channels, the widest the entry accepts: the largest column offsets."""
    import ore
    x = images((2, 3, 16384, 4), seed=26)
    got = ore.preprocess_resize_u8(gpu_ctx, _cuda(x), (2, 5), (2, 9), (0, 4))
    np.testing.assert_array_equal(got.cpu().numpy(), resize_ref(x, (2, 9), (0, 4), (2, 5)))


@pytest.mark.parametrize("shape,resized,origin,out", [((2, 7, 5, 3), (16, 12), (0, 0), (16, 12)),
                                                      ((2, 30, 40, 3), (17, 23), (2, 3), (11, 13)),
                                                      ((2, 45, 60, 3), (32, 43), (2, 5), (28, 32))], ids=_gid)
def test_resize_reverse_channels(gpu_ctx, shape, resized, origin, out):
    import ore
    x = images(shape, seed=23)
    for name, scale, shift in _norms(3):
        y = ore.preprocess_resize_u8(gpu_ctx, _cuda(x), out, resized, origin, scale, shift, reverse_channels=True)
        np.testing.assert_array_equal(y.cpu().numpy(), resize_ref(x, resized, origin, out, scale, shift, reverse=True), err_msg=name)


def test_resize_misaligned_input(gpu_ctx):
    """A uint8 view one byte into a larger buffer."""
    import torch
    import ore
    shape = (2, 30, 41, 3)
    x = images(shape, seed=24)
    buf = torch.zeros(x.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = _cuda(x).reshape(-1)
    view = buf[1:].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 4 == 1
    _, scale, shift = _norms(3)[0]
    ref = resize_ref(x, (24, 36), (2, 3), (20, 32), scale, shift)
    got = ore.preprocess_resize_u8(gpu_ctx, view, (20, 32), (24, 36), (2, 3), scale, shift)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


@pytest.mark.parametrize("gap", [8, 3], ids=["aligned-gap", "odd-gap"])
def test_resize_into_slice(gpu_ctx, gap):
    """y with an image stride above C*H*W (raw ABI): the elements between images keep their contents, whether
    the gap keeps the planes 16-byte aligned (8 floats) or not (3)."""
    import torch
    import ore
    from ore import _lib
    n, hs, ws, c = shape = (2, 30, 40, 3)
    h, w = 20, 32
    geom = _lib.Resize(24, 36, 2, 3)
    x = images(shape, seed=25)
    xd = _cuda(x)
    _, scale, shift = _norms(c)[0]
    ref = resize_ref(x, (24, 36), (2, 3), (h, w), scale, shift)
    per = c * h * w
    sentinel = -12345.0
    F = ctypes.c_float * c
    ybuf = torch.full((n, per + gap), sentinel, dtype=torch.float32, device="cuda")
    t = _lib.Tensor()
    t.data = ybuf.data_ptr()
    t.ndim = 4
    for i, d in enumerate((n, c, h, w)):
        t.dims[i] = d
    t.nstride = per + gap
    st = ore.load().ore_preprocess_resize_u8(gpu_ctx.h, ctypes.c_void_p(xd.data_ptr()), n, hs, ws, c, ctypes.byref(geom),
                                             F(*scale.tolist()), F(*shift.tolist()), 0, ctypes.byref(t))
    assert st == 0, ore.load().ore_last_error(gpu_ctx.h)
    got = ybuf.cpu().numpy()
    np.testing.assert_array_equal(got[:, :per].reshape(n, c, h, w), ref)
    np.testing.assert_array_equal(got[:, per:], np.full((n, gap), sentinel, np.float32))


def test_resize_errors(gpu_ctx):
    import torch
    import ore
    from ore import _lib
    x = torch.zeros((2, 30, 40, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ore.OreError, match="outside"):
        ore.preprocess_resize_u8(gpu_ctx, x, (20, 32), (24, 36), (5, 3))
    with pytest.raises(ore.OreError, match="outside"):
        ore.preprocess_resize_u8(gpu_ctx, x, (20, 32), (24, 36), (2, -1))
    with pytest.raises(ore.OreError, match="16384"):
        ore.preprocess_resize_u8(gpu_ctx, x, (20, 32), (16385, 36))
    with pytest.raises(ore.OreError):
        ore.preprocess_resize_u8(gpu_ctx, x.float(), (20, 32))
    with pytest.raises(ore.OreError):
        ore.preprocess_resize_u8(gpu_ctx, x[:, :, ::2], (20, 32))
    with pytest.raises(ore.OreError):  # reversal needs three channels
        ore.preprocess_resize_u8(gpu_ctx, torch.zeros((1, 4, 4, 1), dtype=torch.uint8, device="cuda"), (2, 2), reverse_channels=True)
    # an unknown flag bit through the raw ABI; n == 0 launches nothing and is fine
    L = ore.load()
    y = torch.empty((2, 3, 20, 32), device="cuda")
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = y.data_ptr(), 4, 0
    for i, d in enumerate(y.shape):
        t.dims[i] = d
    g = _lib.Resize(24, 36, 2, 3)
    xp = ctypes.c_void_p(x.data_ptr())
    for bad in (2, 4):  # the only flag is ORE_PRE_REVERSE_CHANNELS
        assert L.ore_preprocess_resize_u8(gpu_ctx.h, xp, 2, 30, 40, 3, ctypes.byref(g), None, None, bad, ctypes.byref(t)) == 1
        assert b"flags" in L.ore_last_error(gpu_ctx.h)
    t.dims[0] = 0
    assert L.ore_preprocess_resize_u8(gpu_ctx.h, xp, 0, 30, 40, 3, ctypes.byref(g), None, None, 0, ctypes.byref(t)) == 0
    torch.cuda.synchronize()


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


def _model_resize_checks(ctx, m, x, resized, origin, scale, shift):
    """run_u8 on the source batch == run(preprocess_resize_u8(...)) == run(the numpy tensor), bit for bit;
    classify_u8 == topk of those rows; clearing the resize restores the [n, H, W, C] entries."""
    import torch
    import ore
    c, h, w = m.input_dims
    n, hs, ws, _ = x.shape
    ref = resize_ref(x, resized, origin, (h, w), scale, shift)
    xd = _cuda(x)
    direct = _cuda(images((n, h, w, c), seed=30))
    m.set_input_norm(scale, shift)
    before = m.run_u8(direct).clone()
    steps = len(m.steps())

    m.set_input_resize((hs, ws), resized, origin)
    y_ref = m.run(_cuda(ref)).clone()
    y_pre = m.run(ore.preprocess_resize_u8(ctx, xd, (h, w), resized, origin, scale, shift)).clone()
    y_u8 = m.run_u8(xd).clone()
    torch.cuda.synchronize()
    assert torch.equal(y_u8, y_pre) and torch.equal(y_u8, y_ref)
    assert bool(torch.isfinite(y_u8).all())
    assert len(m.steps()) == steps  # the resize is not an exec step
    k = min(3, m.output_elems)
    m.set_topk(k)
    scores, classes = m.classify_u8(xd)
    want_s, want_c = ore.topk(ctx, y_u8, k)
    torch.cuda.synchronize()
    assert torch.equal(scores, want_s) and torch.equal(classes, want_c)
    with pytest.raises(ore.OreError):  # the model's own size is the wrong one now
        m.run_u8(direct)
    with pytest.raises(ore.OreError):
        m.classify_u8(direct)
    out = torch.empty((n, m.output_elems), device="cuda")
    assert ore.load().ore_model_set_input_resize(m.h, hs, ws, ctypes.byref(ore._lib.Resize(h, w, 1, 0))) == 1  # crop outside
    assert ore.load().ore_model_set_input_resize(m.h, 0, ws, ctypes.byref(ore._lib.Resize(h, w, 0, 0))) == 1
    assert torch.equal(m.run_u8_into(xd, out), y_u8)  # a rejected geometry leaves the current one in place

    m.set_input_resize(None)
    after = m.run_u8(direct)
    torch.cuda.synchronize()
    assert torch.equal(after, before)
    with pytest.raises(ore.OreError):
        m.run_u8(xd)
    return ref


def test_mnist_run_u8_resized(gpu_ctx):
    with open(os.path.join(GOLD, "mnist-8.onnx"), "rb") as f:
        onnx = f.read()
    x = images((3, 40, 50, 1), seed=31)
    with _model(gpu_ctx, onnx, max_batch=4) as m:
        assert m.input_dims == (1, 28, 28)
        _model_resize_checks(gpu_ctx, m, x, (32, 36), (2, 4), np.array([1.0 / 255.0], np.float32), np.array([-0.5], np.float32))


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_squeezenet_run_u8_resized(gpu_ctx, precision):
    from ore import squeezenet
    x = images((3, 90, 120, 3), seed=32)
    _, scale, shift = _norms(3)[0]
    with _model(gpu_ctx, squeezenet.build(64), max_batch=4, precision=precision) as m:
        _model_resize_checks(gpu_ctx, m, x, (72, 96), (4, 16), scale, shift)


def test_capture_u8_resized_replays_current_buffer():
    """Graph capture needs a non-null context stream: a context of its own on a torch stream, synchronised
    by hand against the default stream the test's tensors are made on."""
    import torch
    import ore
    from ore import squeezenet
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    m = ore.Model(ctx, squeezenet.build(64), max_batch=1)
    try:
        _, scale, shift = _norms(3)[1]
        m.set_input_norm(scale, shift, reverse_channels=True)
        m.set_input_resize((90, 120), (72, 96), (4, 16))
        x1 = images((1, 90, 120, 3), seed=33)
        x2 = images((1, 90, 120, 3), seed=34)
        refs = [_cuda(resize_ref(x, (72, 96), (4, 16), (64, 64), scale, shift, reverse=True)) for x in (x1, x2)]
        x1, x2 = _cuda(x1), _cuda(x2)
        buf = x1.clone()
        want1 = torch.empty((1, m.output_elems), device="cuda")
        want2, out = torch.empty_like(want1), torch.empty_like(want1)
        torch.cuda.synchronize()
        m.run_into(refs[0], want1)
        m.run_into(refs[1], want2)
        m.capture_u8(buf, out)  # capture only: nothing runs yet
        m.replay()
        s.synchronize()
        assert torch.equal(out, want1) and not torch.equal(want1, want2)
        buf.copy_(x2)  # in place: the graph keeps the pointer
        torch.cuda.synchronize()
        m.replay()
        s.synchronize()
        assert torch.equal(out, want2)
    finally:
        s.synchronize()
        m.close()
        ctx.close()


def test_chunked_run_u8_resized(gpu_ctx):
    """On the pattern of test_chunked_run_u8: a batch above run_batch goes in chunks, and chunk i0 must read
    from source image i0 -- the source images are not the size of the model's input."""
    import torch
    import ore
    from ore import squeezenet
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        n = m.run_batch + 5
        assert n <= 2048
        g = torch.Generator(device="cuda").manual_seed(9)
        x = torch.randint(0, 256, (n, 230, 236, 3), dtype=torch.uint8, device="cuda", generator=g)
        _, scale, shift = _norms(3)[0]
        m.set_input_norm(scale, shift)
        m.set_input_resize((230, 236), (226, 228), (1, 2))
        want = torch.empty((n, m.output_elems), device="cuda")
        m.run_into(ore.preprocess_resize_u8(gpu_ctx, x, (224, 224), (226, 228), (1, 2), scale, shift), want)
        got = m.run_u8(x)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
