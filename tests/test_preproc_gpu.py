"""GPU: uint8 NHWC input (ore_preprocess_u8, ore_model_run_u8, ore_model_graph_capture_u8).

The conversion's arithmetic is fixed -- float32(byte) * scale[c] + shift[c], the product and the sum rounded
separately -- so numpy reproduces it bit for bit and every comparison here is exact: a tolerance would
hide a layout bug (a swapped channel or a shifted pixel changes values by whole units, a fused multiply-add
by one ulp)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

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


def _images(shape, seed=0):
    """Seeded random bytes; where the batch has room for them, every one of the 256 byte values occurs."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=shape, dtype=np.uint8)
    if x.size >= 256:
        flat = x.reshape(-1)
        flat[rng.choice(x.size, 256, replace=False)] = np.arange(256, dtype=np.uint8)
        assert len(np.unique(x)) == 256
    return x


def _ref(x, scale, shift, reverse=False):
    """The documented arithmetic on the host: two float32 roundings per element."""
    if reverse:
        x = x[..., ::-1]
    xf = np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32)
    return (xf * scale.reshape(1, -1, 1, 1)) + shift.reshape(1, -1, 1, 1)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


SHAPES = [(1, 1, 1, 1), (2, 7, 5, 3), (2, 6, 6, 3), (2, 9, 3, 2), (1, 5, 4, 4), (3, 28, 28, 1), (1, 67, 61, 3),
          (2, 224, 224, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_preprocess_matches_numpy(gpu_ctx, shape):
    import ore
    x = _images(shape)
    xd = _cuda(x)
    for name, scale, shift in _norms(shape[3]):
        y = ore.preprocess_u8(gpu_ctx, xd, scale, shift)
        assert tuple(y.shape) == (shape[0], shape[3], shape[1], shape[2])
        np.testing.assert_array_equal(y.cpu().numpy(), _ref(x, scale, shift), err_msg=name)
    # defaults: scale 1, shift 0
    np.testing.assert_array_equal(ore.preprocess_u8(gpu_ctx, xd).cpu().numpy(),
                                  np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32))


@pytest.mark.parametrize("shape", [(2, 7, 5, 3), (2, 8, 8, 3)], ids=lambda s: "x".join(map(str, s)))
def test_preprocess_reverse_channels(gpu_ctx, shape):
    import ore
    x = _images(shape, seed=1)
    for name, scale, shift in _norms(3):
        y = ore.preprocess_u8(gpu_ctx, _cuda(x), scale, shift, reverse_channels=True)
        np.testing.assert_array_equal(y.cpu().numpy(), _ref(x, scale, shift, reverse=True), err_msg=name)


def test_preprocess_misaligned_input(gpu_ctx):
    """A uint8 view one byte into a larger buffer: not dword aligned, so the scalar kernel runs."""
    import torch
    import ore
    shape = (2, 8, 8, 3)
    x = _images(shape, seed=2)
    buf = torch.zeros(x.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = _cuda(x).reshape(-1)
    view = buf[1:].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 4 == 1
    for name, scale, shift in _norms(3):
        np.testing.assert_array_equal(ore.preprocess_u8(gpu_ctx, view, scale, shift).cpu().numpy(), _ref(x, scale, shift),
                                      err_msg=name)


@pytest.mark.parametrize("gap", [8, 3], ids=["aligned-gap", "odd-gap"])
def test_preprocess_into_slice(gpu_ctx, gap):
    """y with an image stride above C*H*W (raw ABI): the elements between images keep their contents.  A
    gap of 8 floats keeps every plane 16-byte aligned (vector kernel), a gap of 3 does not (scalar kernel)."""
    import torch
    import ore
    from ore import _lib
    n, h, w, c = shape = (2, 8, 8, 3)
    x = _images(shape, seed=3)
    xd = _cuda(x)
    _, scale, shift = _norms(c)[0]
    per = c * h * w
    sentinel = -12345.0
    ybuf = torch.full((n, per + gap), sentinel, dtype=torch.float32, device="cuda")
    t = _lib.Tensor()
    t.data = ybuf.data_ptr()
    t.ndim = 4
    for i, d in enumerate((n, c, h, w)):
        t.dims[i] = d
    t.nstride = per + gap
    F = ctypes.c_float * c
    st = ore.load().ore_preprocess_u8(gpu_ctx.h, ctypes.c_void_p(xd.data_ptr()), n, h, w, c, F(*scale.tolist()),
                                      F(*shift.tolist()), 0, ctypes.byref(t))
    assert st == 0, ore.load().ore_last_error(gpu_ctx.h)
    got = ybuf.cpu().numpy()
    np.testing.assert_array_equal(got[:, :per].reshape(n, c, h, w), _ref(x, scale, shift))
    np.testing.assert_array_equal(got[:, per:], np.full((n, gap), sentinel, np.float32))


@contextlib.contextmanager
def _model(ctx, onnx_bytes, **kw):
    """A model closed even when the test fails: it must not outlive the session's context."""
    import ore
    m = ore.Model(ctx, onnx_bytes, **kw)
    try:
        yield m
    finally:
        m.close()


def _same_three_ways(ctx, model, x, scale, shift):
    """run_u8(x) == run(preprocess_u8(x)) == run(the numpy tensor), bit for bit; returns the numpy tensor."""
    import torch
    import ore
    ref = _ref(x, scale, shift)
    xd = _cuda(x)
    model.set_input_norm(scale, shift)
    y_ref = model.run(_cuda(ref)).clone()
    y_pre = model.run(ore.preprocess_u8(ctx, xd, scale, shift)).clone()
    y_u8 = model.run_u8(xd)
    torch.cuda.synchronize()
    assert torch.equal(y_u8, y_pre) and torch.equal(y_u8, y_ref)
    assert bool(torch.isfinite(y_u8).all())
    return ref


def test_mnist_run_u8(gpu_ctx):
    with open(os.path.join(GOLD, "mnist-8.onnx"), "rb") as f:
        onnx = f.read()
    x = _images((3, 28, 28, 1), seed=4)
    with _model(gpu_ctx, onnx, max_batch=4) as m:
        assert m.input_dims == (1, 28, 28)
        _same_three_ways(gpu_ctx, m, x, np.array([1.0 / 255.0], np.float32), np.array([-0.5], np.float32))


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_squeezenet_run_u8(gpu_ctx, precision):
    from ore import squeezenet
    x = _images((3, 64, 64, 3), seed=5)
    _, scale, shift = _norms(3)[0]
    with _model(gpu_ctx, squeezenet.build(64), max_batch=4, precision=precision) as m:
        steps = len(m.steps())
        ref = _same_three_ways(gpu_ctx, m, x, scale, shift)
        assert len(m.steps()) == steps  # the conversion is not an exec step
        if precision == "f32":
            np.testing.assert_array_equal(m.read_value("data_0"), ref)  # the staged input of the last (uint8) run


def test_capture_u8_replays_current_buffer():
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
        x1 = _cuda(_images((1, 64, 64, 3), seed=6))
        x2 = _cuda(_images((1, 64, 64, 3), seed=7))
        buf = x1.clone()
        want1 = torch.empty((1, m.output_elems), device="cuda")
        want2, out = torch.empty_like(want1), torch.empty_like(want1)
        torch.cuda.synchronize()
        m.run_u8_into(x1, want1)
        m.run_u8_into(x2, want2)
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


def test_chunked_run_u8(gpu_ctx):
    """As test_config4_gpu.py::test_chunked_run_timing_and_read_value: a batch above run_batch goes in the
    chunks ore_model_run uses, each converted and then run."""
    import torch
    import ore
    from ore import squeezenet
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        n = m.run_batch + 5
        assert n <= 2048
        g = torch.Generator(device="cuda").manual_seed(8)
        x = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
        _, scale, shift = _norms(3)[0]
        m.set_input_norm(scale, shift)
        want = torch.empty((n, m.output_elems), device="cuda")
        m.run_into(ore.preprocess_u8(gpu_ctx, x, scale, shift), want)
        got = m.run_u8(x)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        with pytest.raises(ore.OreError, match="chunks"):
            m.read_value("data_0")


def test_u8_errors(gpu_ctx):
    import torch
    import ore
    from ore import _lib, squeezenet
    with _model(gpu_ctx, squeezenet.build(64), max_batch=2) as m:
        good = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
        m.run_u8(good)
        with pytest.raises(ore.OreError):  # wrong dtype
            m.run_u8(good.float())
        with pytest.raises(ore.OreError):
            ore.preprocess_u8(gpu_ctx, good.to(torch.int8))
        with pytest.raises(ore.OreError):  # non-contiguous
            m.run_u8(torch.zeros((2, 64, 3, 64), dtype=torch.uint8, device="cuda").permute(0, 1, 3, 2))
        with pytest.raises(ore.OreError):
            ore.preprocess_u8(gpu_ctx, good[:, :, ::2])
        with pytest.raises(ore.OreError):  # wrong C
            m.run_u8(torch.zeros((2, 64, 64, 4), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ore.OreError):
            ore.preprocess_u8(gpu_ctx, torch.zeros((1, 4, 4, 5), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ore.OreError):  # a norm whose length is not C
            m.set_input_norm([1.0, 1.0], [0.0, 0.0])
        assert ore.load().ore_model_set_input_norm(m.h, None, None, 1, 0) == 1  # ... and through the raw ABI
        with pytest.raises(ore.OreError):  # reversal needs three channels
            ore.preprocess_u8(gpu_ctx, torch.zeros((1, 4, 4, 1), dtype=torch.uint8, device="cuda"), reverse_channels=True)
        with pytest.raises(ore.OreError):  # n > max_batch
            m.run_u8(torch.zeros((3, 64, 64, 3), dtype=torch.uint8, device="cuda"))
        out = torch.empty((3, m.output_elems), device="cuda")
        three = torch.zeros((3, 64, 64, 3), dtype=torch.uint8, device="cuda")
        assert ore.load().ore_model_run_u8(m.h, ctypes.c_void_p(three.data_ptr()), 3, ctypes.c_void_p(out.data_ptr())) == 1
        # an unknown flag bit through the raw ABI
        y = torch.empty((2, 3, 64, 64), device="cuda")
        t = _lib.Tensor()
        t.data, t.ndim, t.nstride = y.data_ptr(), 4, 0
        for i, d in enumerate(y.shape):
            t.dims[i] = d
        L = ore.load()
        assert L.ore_preprocess_u8(gpu_ctx.h, ctypes.c_void_p(good.data_ptr()), 2, 64, 64, 3, None, None, 2, ctypes.byref(t)) == 1
        assert b"flags" in L.ore_last_error(gpu_ctx.h)
        assert L.ore_model_set_input_norm(m.h, None, None, 3, 4) == 1
        # y dims that are not [n,c,h,w]; n == 0 launches nothing and is fine
        assert L.ore_preprocess_u8(gpu_ctx.h, ctypes.c_void_p(good.data_ptr()), 2, 64, 32, 3, None, None, 0, ctypes.byref(t)) == 1
        t.dims[0] = 0
        assert L.ore_preprocess_u8(gpu_ctx.h, ctypes.c_void_p(good.data_ptr()), 0, 64, 64, 3, None, None, 0, ctypes.byref(t)) == 0
        torch.cuda.synchronize()
