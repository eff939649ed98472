"""GPU: row-wise top-k (ore_topk_f32) and the model classify entries (ore_model_classify, _classify_u8,
ore_model_graph_capture_classify, _capture_classify_u8).

The result is specified to the bit -- output j of a row is the element ranked j in "larger value first,
equal values by lower index, NaNs last by index", i.e. np.argsort(-x, axis=1, kind="stable")[:, :k], and
values are bit copies -- so every comparison here is exact, values as uint32: a tolerance could only hide an
off-by-one lane or a wrong tie."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

ROWS = (1, 3, 5, 130)  # a block not full of rows (4 per block), more than one block
DS = (1, 5, 63, 64, 65, 256, 257, 1000, 1024, 1025, 4100)  # both register kernels, their bounds, the long-row kernel
KINDS = ("normal", "softmax", "ties", "constant", "ramps", "zeros", "specials", "nans")


def _ref(x, k):
    """The host reference: stable descending argsort (NaNs last), values taken by index."""
    with np.errstate(invalid="ignore"):
        idx = np.argsort(-x, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(x, idx, 1), idx.astype(np.int32)


def _nan(rng, shape):
    """NaNs of both signs with random payloads."""
    bits = (rng.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31)) | np.uint32(0x7f800000) | \
        rng.integers(1, 1 << 23, shape, dtype=np.uint32)
    return bits.view(np.float32)


def _input(kind, rows, D, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((rows, D)).astype(np.float32)
    if kind == "softmax":
        e = np.exp(rng.standard_normal((rows, D)).astype(np.float32))
        return (e / e.sum(1, keepdims=True)).astype(np.float32)
    if kind == "ties":  # almost everything ties: the index rule decides
        return rng.integers(0, 4, (rows, D)).astype(np.float32)
    if kind == "constant":
        return np.full((rows, D), 0.25, np.float32)
    if kind == "ramps":  # even rows ascending (winners in the last lanes / registers), odd rows descending
        r = np.arange(D, dtype=np.float32) - np.float32(D // 2)
        return np.stack([r if i % 2 == 0 else r[::-1] for i in range(rows)]).astype(np.float32)
    if kind == "zeros":  # +0.0 and -0.0 compare equal, and keep their own sign in the output
        x = np.where(rng.random((rows, D)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        x[rng.random((rows, D)) < 0.05] = -1.0
        return x
    x = rng.standard_normal((rows, D)).astype(np.float32)
    if kind == "specials":  # NaN of both signs, +inf and -inf sprinkled in
        m = rng.random((rows, D))
        x = np.where(m < 0.1, _nan(rng, (rows, D)), x)
        x[(m >= 0.1) & (m < 0.2)] = np.inf
        x[(m >= 0.2) & (m < 0.3)] = -np.inf
        return x
    assert kind == "nans"  # row r: min(r, D) numbers, NaNs elsewhere -- NaNs must appear in the output, in index order
    y = _nan(rng, (rows, D))
    for r in range(rows):
        keep = rng.choice(D, min(r, D), replace=False)
        y[r, keep] = x[r, keep]
    return y


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DS)
def test_topk_matches_numpy(gpu_ctx, D, kind):
    import ore
    x = _input(kind, max(ROWS), D, seed=1000 * KINDS.index(kind) + D)
    kmax = min(D, 64)
    want_v, want_i = _ref(x, kmax)  # once for all rows and k: a prefix of the order
    xd = _cuda(x)
    for rows in ROWS:
        for k in sorted({1, min(5, D), kmax}):
            v, i = ore.topk(gpu_ctx, xd[:rows], k)
            assert tuple(v.shape) == tuple(i.shape) == (rows, k)
            assert str(v.dtype) == "torch.float32" and str(i.dtype) == "torch.int32"
            np.testing.assert_array_equal(i.cpu().numpy(), want_i[:rows, :k], err_msg=f"rows {rows} k {k}")
            np.testing.assert_array_equal(_u32(v.cpu().numpy()), _u32(want_v[:rows, :k]), err_msg=f"rows {rows} k {k}")


def test_topk_flattens_trailing_dims(gpu_ctx):
    """Rows are dims[0], the row the product of the rest (as ore_softmax_f32)."""
    import ore
    x = _input("normal", 3, 2 * 5 * 7, seed=1)
    v, i = ore.topk(gpu_ctx, _cuda(x.reshape(3, 2, 5, 7)), 4)
    want_v, want_i = _ref(x, 4)
    np.testing.assert_array_equal(i.cpu().numpy(), want_i)
    np.testing.assert_array_equal(_u32(v.cpu().numpy()), _u32(want_v))


@pytest.mark.parametrize("D", [1000, 1025])
def test_topk_row_stride(gpu_ctx, D):
    """x->nstride = D + 3 through the raw ABI: the 3 elements between rows would win every round if read."""
    import torch
    import ore
    from ore import _lib
    rows, gap, k = 5, 3, 64
    x = _input("ties", rows, D, seed=2)
    buf = np.full((rows, D + gap), np.float32(3e38), np.float32)
    buf[:, :D] = x
    xd = _cuda(buf)
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = xd.data_ptr(), 2, D + gap
    t.dims[0], t.dims[1] = rows, D
    v = torch.empty((rows, k), dtype=torch.float32, device="cuda")
    i = torch.empty((rows, k), dtype=torch.int32, device="cuda")
    st = ore.load().ore_topk_f32(gpu_ctx.h, ctypes.byref(t), k, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(i.data_ptr()))
    assert st == 0, ore.load().ore_last_error(gpu_ctx.h)
    want_v, want_i = _ref(x, k)
    np.testing.assert_array_equal(i.cpu().numpy(), want_i)
    np.testing.assert_array_equal(_u32(v.cpu().numpy()), _u32(want_v))


@contextlib.contextmanager
def _model(ctx, onnx_bytes, **kw):
    """A model closed even when the test fails: it must not outlive the session's context."""
    import ore
    m = ore.Model(ctx, onnx_bytes, **kw)
    try:
        yield m
    finally:
        m.close()


def _images(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _classify_equals_run(m, x_u8, scale, shift, k):
    """classify == top-k of run's downloaded rows, classify_u8 == the same of run_u8; steps and tiles
    unchanged; rows past n of a larger output buffer untouched."""
    import torch
    n = x_u8.shape[0]
    assert n < m.max_batch
    steps, tiles = len(m.steps()), m.tiles()
    m.set_input_norm(scale, shift)
    xd8 = _cuda(x_u8)
    xf = _cuda(np.ascontiguousarray(x_u8.transpose(0, 3, 1, 2)).astype(np.float32) * scale.reshape(1, -1, 1, 1)
               + shift.reshape(1, -1, 1, 1))
    rows = m.run(xf).cpu().numpy()
    rows8 = m.run_u8(xd8).cpu().numpy()
    m.set_topk(k)
    for got, r in ((m.classify(xf), rows), (m.classify_u8(xd8), rows8)):
        want_v, want_i = _ref(r, k)
        assert tuple(got[0].shape) == tuple(got[1].shape) == (n, k)
        np.testing.assert_array_equal(got[1].cpu().numpy(), want_i)
        np.testing.assert_array_equal(_u32(got[0].cpu().numpy()), _u32(want_v))
    assert len(m.steps()) == steps and m.tiles() == tiles  # the selection is not an exec step
    big_s = torch.full((m.max_batch, k), -7.0, dtype=torch.float32, device="cuda")
    big_c = torch.full((m.max_batch, k), -7, dtype=torch.int32, device="cuda")
    m.classify_into(xf, big_s[:n], big_c[:n])
    want_v, want_i = _ref(rows, k)
    np.testing.assert_array_equal(big_c.cpu().numpy(), np.concatenate([want_i, np.full((m.max_batch - n, k), -7, np.int32)]))
    np.testing.assert_array_equal(_u32(big_s.cpu().numpy()),
                                  _u32(np.concatenate([want_v, np.full((m.max_batch - n, k), -7.0, np.float32)])))
    return xf, rows


def test_mnist_classify(gpu_ctx):
    with open(os.path.join(GOLD, "mnist-8.onnx"), "rb") as f:
        onnx = f.read()
    with _model(gpu_ctx, onnx, max_batch=4) as m:
        assert m.output_elems == 10
        _classify_equals_run(m, _images((3, 28, 28, 1), seed=3), np.array([1.0 / 255.0], np.float32),
                             np.array([-0.5], np.float32), k=3)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_squeezenet_classify(gpu_ctx, precision):
    from ore import squeezenet
    scale = (np.float32(1.0) / (np.float32(255.0) * np.array([0.229, 0.224, 0.225], np.float32))).astype(np.float32)
    shift = (-np.array([0.485, 0.456, 0.406], np.float32) / np.array([0.229, 0.224, 0.225], np.float32)).astype(np.float32)
    with _model(gpu_ctx, squeezenet.build(64), max_batch=4, precision=precision) as m:
        xf, rows = _classify_equals_run(m, _images((3, 64, 64, 3), seed=4), scale, shift, k=5)
        # read_value after classify behaves as after run: the output rows and (f32) the input
        np.testing.assert_array_equal(m.read_value("softmaxout_1").reshape(rows.shape), rows)
        if precision == "f32":
            np.testing.assert_array_equal(m.read_value("data_0"), xf.cpu().numpy())


def _relu_dropout_onnx(dims):
    from ore import onnx_wire as w
    nodes = [w.encode_node("Relu", ["data_0"], ["r"], name="relu"),
             w.encode_node("Dropout", ["r"], ["out", "_mask"], name="drop", attrs=[w.encode_attr_float("ratio", 0.5)])]
    return w.encode_model("alias-out", nodes, [], [w.encode_value_info("data_0", (1,) + dims)],
                          [w.encode_value_info("out", (1,) + dims)], opset=8)


def test_classify_output_inside_the_arena(gpu_ctx):
    """A graph whose output is a view of another value (a final Dropout aliases its input): run copies it
    out of the arena, classify selects from it in place."""
    dims, n, k = (2, 4, 9), 3, 7
    x = _input("normal", n, 72, seed=5).reshape((n,) + dims)
    with _model(gpu_ctx, _relu_dropout_onnx(dims), max_batch=4) as m:
        assert m.output_elems == 72
        rows = m.run(_cuda(x)).cpu().numpy()
        np.testing.assert_array_equal(rows, np.maximum(x, 0).reshape(n, 72))
        m.set_topk(k)
        scores, classes = m.classify(_cuda(x))
        want_v, want_i = _ref(rows, k)
        np.testing.assert_array_equal(classes.cpu().numpy(), want_i)
        np.testing.assert_array_equal(_u32(scores.cpu().numpy()), _u32(want_v))
        np.testing.assert_array_equal(m.run(_cuda(x)).cpu().numpy(), rows)  # run after classify: unchanged


def test_capture_classify_u8_replays_current_buffer():
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
        k = 5
        m.set_input_norm(np.ones(3, np.float32), -np.array([104.0, 117.0, 123.0], np.float32), reverse_channels=True)
        m.set_topk(k)
        x1 = _cuda(_images((1, 64, 64, 3), seed=6))
        x2 = _cuda(_images((1, 64, 64, 3), seed=7))
        buf = x1.clone()
        torch.cuda.synchronize()
        want1 = m.classify_u8(x1)  # on the context's stream, into buffers of their own
        want2 = m.classify_u8(x2)
        scores = torch.empty((1, k), dtype=torch.float32, device="cuda")
        classes = torch.empty((1, k), dtype=torch.int32, device="cuda")
        s.synchronize()
        m.capture_classify_u8(buf, scores, classes)  # capture only: nothing runs yet
        m.replay()
        s.synchronize()
        assert torch.equal(classes, want1[1]) and torch.equal(scores.view(torch.int32), want1[0].view(torch.int32))
        assert not torch.equal(want1[0], want2[0])
        buf.copy_(x2)  # in place: the graph keeps the pointer
        torch.cuda.synchronize()
        m.replay()
        s.synchronize()
        assert torch.equal(classes, want2[1]) and torch.equal(scores.view(torch.int32), want2[0].view(torch.int32))
    finally:
        s.synchronize()
        m.close()
        ctx.close()


def test_chunked_classify(gpu_ctx):
    """As test_preproc_gpu.py::test_chunked_run_u8: a batch above run_batch goes in ore_model_run's chunks,
    each selected into rows [i0, i0 + nc) of the outputs."""
    import torch
    from ore import squeezenet
    k = 5
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        n = m.run_batch + 5
        assert n <= 2048
        g = torch.Generator(device="cuda").manual_seed(8)
        x = torch.rand((n, 3, 224, 224), dtype=torch.float32, device="cuda", generator=g)
        m.set_topk(k)
        rows = m.run(x).cpu().numpy()
        scores, classes = m.classify(x)
        want_v, want_i = _ref(rows, k)
        np.testing.assert_array_equal(classes.cpu().numpy(), want_i)
        np.testing.assert_array_equal(_u32(scores.cpu().numpy()), _u32(want_v))


def test_topk_errors(gpu_ctx):
    import torch
    import ore
    from ore import _lib, squeezenet
    L = ore.load()
    x = _cuda(_input("normal", 2, 10, seed=9))
    for k in (0, 65, 11):  # k = 0, k > 64, k > D
        with pytest.raises(ore.OreError):
            ore.topk(gpu_ctx, x if k != 65 else _cuda(_input("normal", 2, 100, seed=9)), k)
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = x.data_ptr(), 2, 0
    t.dims[0], t.dims[1] = 2, 10
    v = torch.empty((2, 64), dtype=torch.float32, device="cuda")
    i = torch.empty((2, 64), dtype=torch.int32, device="cuda")
    for k in (0, 65, 11):  # ... and through the raw ABI
        assert L.ore_topk_f32(gpu_ctx.h, ctypes.byref(t), k, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(i.data_ptr())) == 1
        assert b"top-k" in L.ore_last_error(gpu_ctx.h)
    t.nstride = 9  # a row stride below D
    assert L.ore_topk_f32(gpu_ctx.h, ctypes.byref(t), 1, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(i.data_ptr())) == 1
    t.nstride, t.dims[0] = 0, 0  # rows == 0 launches nothing and is fine
    assert L.ore_topk_f32(gpu_ctx.h, ctypes.byref(t), 1, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(i.data_ptr())) == 0
    with pytest.raises(ore.OreError):  # non-contiguous input
        ore.topk(gpu_ctx, _cuda(_input("normal", 4, 10, seed=9))[:, ::2], 1)
    with _model(gpu_ctx, squeezenet.build(64), max_batch=2) as m:
        good = torch.zeros((2, 3, 64, 64), device="cuda")
        good8 = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
        for k in (0, 65, 1001):
            with pytest.raises(ore.OreError):
                m.set_topk(k)
            assert L.ore_model_set_topk(m.h, k) == 1
        assert m.topk == 1
        m.set_topk(5)
        scores = torch.empty((2, 5), dtype=torch.float32, device="cuda")
        classes = torch.empty((2, 5), dtype=torch.int32, device="cuda")
        m.classify_into(good, scores, classes)
        for fn, x_ok in ((m.classify_into, good), (m.classify_u8_into, good8)):
            with pytest.raises(ore.OreError, match="int32"):  # wrong dtype for classes
                fn(x_ok, scores, classes.long())
            with pytest.raises(ore.OreError, match="float32"):
                fn(x_ok, scores.double(), classes)
            with pytest.raises(ore.OreError, match="contiguous"):  # non-contiguous outputs
                fn(x_ok, torch.empty((2, 10), device="cuda")[:, ::2], classes)
            with pytest.raises(ore.OreError, match="contiguous"):
                fn(x_ok, scores, torch.empty((5, 2), dtype=torch.int32, device="cuda").t())
            with pytest.raises(ore.OreError, match="shape"):  # [n, k] for another k
                fn(x_ok, torch.empty((2, 4), device="cuda"), torch.empty((2, 4), dtype=torch.int32, device="cuda"))
        with pytest.raises(ore.OreError):  # wrong input dtype
            m.classify(good8)
        with pytest.raises(ore.OreError):
            m.classify_u8(good)
        three = torch.zeros((3, 3, 64, 64), device="cuda")  # n > max_batch
        three8 = torch.zeros((3, 64, 64, 3), dtype=torch.uint8, device="cuda")
        with pytest.raises(ore.OreError, match="max_batch"):
            m.classify(three)
        with pytest.raises(ore.OreError, match="max_batch"):
            m.classify_u8(three8)
        s3 = torch.empty((3, 5), dtype=torch.float32, device="cuda")
        c3 = torch.empty((3, 5), dtype=torch.int32, device="cuda")
        for entry, xin in ((L.ore_model_classify, three), (L.ore_model_classify_u8, three8)):
            assert entry(m.h, ctypes.c_void_p(xin.data_ptr()), 3, ctypes.c_void_p(s3.data_ptr()), ctypes.c_void_p(c3.data_ptr())) == 1
            assert entry(m.h, ctypes.c_void_p(xin.data_ptr()), 0, ctypes.c_void_p(s3.data_ptr()), ctypes.c_void_p(c3.data_ptr())) == 0
        # the context and the model stay usable
        got = m.classify(good)
        want_v, want_i = _ref(m.run(good).cpu().numpy(), 5)
        np.testing.assert_array_equal(got[1].cpu().numpy(), want_i)
        np.testing.assert_array_equal(_u32(got[0].cpu().numpy()), _u32(want_v))
    torch.cuda.synchronize()
