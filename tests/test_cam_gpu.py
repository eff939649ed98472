"""GPU: class activation maps of the selected classes (ore_class_maps_f32, ore_model_set_cam; csrc/ore_cam.hip).

Per-op entry: against a float64 reference within the project's f32 bound 2e-6 * (sum |w x| + |b|), and bit for bit
against ore_conv2d_f32 (+ ore_relu_f32) of all M channels, gathered -- over the case table of _cam.op_cases(), every
call into a NaN-poisoned buffer whose guard bands must come back untouched; one case with x as a slice of a poisoned
buffer, Relu off and a NULL bias.

Model level: for every test graph and SqueezeNet at 64 and 224, on f32 direct, f32 Winograd and f16 models, under
ORE_FUSE_ALL, fusion 0 and two streams, the maps equal bit for bit the pool's input read from a fusion-0 +
ORE_KEEP_VALUES load of the same model, gathered by the returned classes; scores and classes equal those of a run
without the maps.  Independent anchors: the f32 maps against float64 of the pinned input (read_value), the f16 maps
through _convref.f16_layer_check (tests/test_cam.py holds the cap on ambiguous outputs on the CPU).  Then views, the
uint8 input paths, captures, chunks and the errors."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

import _cam
from _convref import F16_AMBIGUOUS_CAP

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON = np.int32(0x7FC5A5A5)  # a quiet NaN no kernel computes
GUARD = 96                     # poisoned floats on either side of the maps
F32_TOL = 2e-6                 # the project's f32 bound, as a fraction of sum |w x| + |b|
PRECISIONS = [("f32", False), ("f32", True), ("f16", True)]  # (precision, winograd)
PREC_IDS = ["f32-direct", "f32-wino", "f16"]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


@contextlib.contextmanager
def _model(ctx, onnx_bytes, **kw):
    import ore
    m = ore.Model(ctx, onnx_bytes, **kw)
    try:
        yield m
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ the per-op entry
def _class_maps_raw(ctx, x_t, dims, nstride, w_t, b_t, cls_t, relu, views):
    """ore_class_maps_f32 through ctypes into the middle of a poisoned buffer: (maps, guard words left intact?)"""
    import torch
    import ore
    from ore import _lib
    n, C, H, W = dims
    k = int(cls_t.shape[1])
    size = n * k * H * W
    buf = torch.full((GUARD + size + GUARD,), int(POISON), dtype=torch.int32, device="cuda")
    d = _lib.Tensor()
    d.data, d.ndim, d.nstride = x_t.data_ptr(), 4, nstride
    for i, v in enumerate(dims):
        d.dims[i] = v
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(ore.load().ore_class_maps_f32(ctx.h, ctypes.byref(d), p(w_t), p(b_t) if b_t is not None else None,
                                             int(w_t.shape[0]), 1 if relu else 0, p(cls_t), k, views,
                                             ctypes.c_void_p(buf.data_ptr() + 4 * GUARD)), ctx.h)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:GUARD] == POISON).all() and (host[GUARD + size:] == POISON).all())
    return host[GUARD:GUARD + size].view(np.float32).reshape(n, k, H, W).copy(), intact


@functools.lru_cache(maxsize=None)
def _op_result(ctx, case):
    """(maps from the kernel, guards intact, float64 maps, magnitudes, the full conv gathered) of a per-op case"""
    import ore
    C, M, H, W, k, n, views = case
    x, w, b, classes = _cam.op_inputs(case)
    xd, wd, bd, cd = _cuda(x), _cuda(w), _cuda(b), _cuda(classes)
    got, intact = _class_maps_raw(ctx, xd, (n, C, H, W), 0, wd, bd, cd, True, views)
    full = ore.relu(ctx, ore.convolution(ctx, xd, wd.reshape(M, C, 1, 1), bd, strides=(1, 1)))
    wrapped = ore.class_maps(ctx, xd, wd, bd, cd, relu=True, views=views)
    ref, mag = _cam.maps_f64(x, w, b, classes, True, views)
    return got, intact, ref, mag, _cam.gather(full.cpu().numpy(), classes, views), wrapped.cpu().numpy()


@pytest.mark.parametrize("case", _cam.op_cases(), ids=_cam.op_id)
def test_class_maps_against_float64(gpu_ctx, case):
    got, intact, ref, mag, _, wrapped = _op_result(gpu_ctx, case)
    assert intact, "the guard bands around maps were written"
    assert not (_bits(got) == np.uint32(POISON)).any(), "an element of maps was not written"
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(mag, 1e-300)).max())
    print(f"class maps {_cam.op_id(case)}: max |got - f64| / (sum |w x| + |b|) = {worst:.3g}")
    assert (err <= F32_TOL * mag).all(), worst
    _assert_bits(wrapped, got, "ore.class_maps against the raw entry")


@pytest.mark.parametrize("case", _cam.op_cases(), ids=_cam.op_id)
def test_class_maps_equal_the_conv_bit_for_bit(gpu_ctx, case):
    got, _, _, _, conv, _ = _op_result(gpu_ctx, case)
    _assert_bits(got, conv, "class maps against ore_conv2d_f32 + ore_relu_f32, gathered")


@pytest.mark.parametrize("misalign", [0, 1], ids=["aligned", "off1"])
def test_class_maps_of_a_slice(gpu_ctx, misalign):
    """x as a slice: nstride above one image, the gaps and the surroundings NaN; Relu off, bias NULL.  The maps
    hold no NaN, equal the conv of the dense copy bit for bit, and meet the float64 bound."""
    import ore
    n, C, M, H, W, k, views = 3, 48, 40, 13, 11, 17, 1
    rng = np.random.default_rng(77)
    x = rng.standard_normal((n, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((M, C)) * np.sqrt(2.0 / C)).astype(np.float32)
    classes = rng.integers(0, M, (n, k)).astype(np.int32)
    img, gap, lead = C * H * W, 7, 64 + misalign
    flat = np.full(lead + n * (img + gap) + 64, np.nan, np.float32)
    for i in range(n):
        flat[lead + i * (img + gap):lead + i * (img + gap) + img] = x[i].reshape(-1)
    fd, wd, cd = _cuda(flat), _cuda(w), _cuda(classes)
    got, intact = _class_maps_raw(gpu_ctx, fd[lead:], (n, C, H, W), img + gap, wd, None, cd, False, views)
    assert intact and np.isfinite(got).all()
    ref, mag = _cam.maps_f64(x, w, None, classes, False, views)
    assert (np.abs(got.astype(np.float64) - ref) <= F32_TOL * mag).all()
    assert (got < 0).any()  # Relu really off
    full = ore.convolution(gpu_ctx, _cuda(x), wd.reshape(M, C, 1, 1), None, strides=(1, 1)).cpu().numpy()
    _assert_bits(got, _cam.gather(full, classes, views))
    view = fd[lead:lead + n * (img + gap)].view(n, img + gap)[:, :img].view(n, C, H, W)  # the same slice as a tensor
    _assert_bits(ore.class_maps(gpu_ctx, view, wd, None, cd, relu=False).cpu().numpy(), got)


def test_class_maps_empty_batch(gpu_ctx):
    import torch
    import ore
    x = torch.empty((0, 8, 3, 3), device="cuda")
    w, c = torch.zeros((4, 8), device="cuda"), torch.zeros((0, 2), dtype=torch.int32, device="cuda")
    assert tuple(ore.class_maps(gpu_ctx, x, w, None, c).shape) == (0, 2, 3, 3)
    p = ctypes.c_void_p(0x1000)  # n == 0 launches nothing: never dereferenced
    from ore import _lib
    d = _lib.Tensor()
    d.data, d.ndim = 0x1000, 4
    d.dims[0], d.dims[1], d.dims[2], d.dims[3] = 0, 8, 3, 3
    assert ore.load().ore_class_maps_f32(gpu_ctx.h, ctypes.byref(d), p, None, 4, 1, p, 2, 1, p) == 0


# ------------------------------------------------------------------------------------------ model level
def _model_bytes(name):
    from ore import squeezenet
    return squeezenet.build(int(name[2:])) if name.startswith("sq") else _cam.graph_bytes(name)


def _model_input(name, n=_cam.BATCH):
    from ore import squeezenet
    if name.startswith("sq"):
        return squeezenet.synthetic_input(n, int(name[2:]), seed=_cam.SQ_SEED)
    return np.asarray(_cam.graph_input(name, n))


@functools.lru_cache(maxsize=None)
def _pool_input(ctx, name, precision, winograd, n=_cam.BATCH):
    """T [n, M, Hm, Wm]: the pool's input as the unfused plan stores it (fusion 0 + ORE_KEEP_VALUES), read back"""
    import ore
    with _model(ctx, _model_bytes(name), max_batch=n, precision=precision, winograd=winograd) as m:
        m.set_fusion(ore.KEEP_VALUES)
        m.run(_cuda(_model_input(name, n)))
        T = m.read_value(_cam.head(_model_bytes(name))["T"])
    T.setflags(write=False)
    return T


MODELS = sorted(_cam.GRAPHS) + ["sq64", "sq224"]


@pytest.mark.parametrize("precision,winograd", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("name", MODELS)
def test_model_maps(gpu_ctx, name, precision, winograd):
    import torch
    import ore
    mb, k, n = _model_bytes(name), _cam.TOPK, _cam.BATCH
    h = _cam.head(mb)
    T = _pool_input(gpu_ctx, name, precision, winograd)
    x = _cuda(_model_input(name))
    with _model(gpu_ctx, mb, max_batch=n, precision=precision, winograd=winograd) as m:
        assert m.cam_hw == T.shape[2:]
        m.set_topk(k)
        for fusion, streams in ((ore.FUSE_ALL, 1), (0, 1), (ore.FUSE_ALL, 2)):
            what = f"{name} {precision} wino={winograd} fusion={fusion} streams={streams}"
            m.set_fusion(fusion)
            m.set_streams(streams)
            plain_s, plain_c = m.classify(x)
            scores, classes, maps = m.classify_cam(x)
            torch.cuda.synchronize()
            assert tuple(maps.shape) == (n, k) + T.shape[2:]
            assert torch.equal(classes, plain_c) and torch.equal(scores.view(torch.int32), plain_s.view(torch.int32)), what
            cls, got = classes.cpu().numpy(), maps.cpu().numpy()
            _assert_bits(got, _cam.gather(T, cls), what)
            # the independent anchors, on the input the plan pinned for the kernel
            buf = torch.empty_like(maps)
            m.set_cam_output(buf)
            m.classify(x)
            x1 = m.read_value(h["x"])
            m.set_cam_output(None)
            _assert_bits(buf.cpu().numpy(), got, what + ": a second run into a buffer of the caller's")
            if precision == "f32":
                ref, mag = _cam.maps_f64(x1, h["w"], h["b"], cls, h["relu"])
                err = np.abs(got.astype(np.float64) - ref)
                print(f"{what}: max |maps - f64| / mag = {float((err / np.maximum(mag, 1e-300)).max()):.3g}")
                assert (err <= F32_TOL * mag).all(), what
            else:
                bad, amb = _cam.f16_maps_check(got, x1, h["w"], h["b"], cls, h["relu"])
                print(f"{what}: f16_layer_check bad {bad:.4f}, ambiguous {amb:.4f}")
                assert bad == 0.0 and amb <= F16_AMBIGUOUS_CAP, what


@pytest.mark.parametrize("precision,winograd", [("f32", True), ("f16", True)], ids=["f32", "f16"])
def test_views(gpu_ctx, precision, winograd):
    """views = 2 with n = 4: both images of a group carry the group's classes"""
    import torch
    name, n, k = "c32", 4, 3
    T = _pool_input(gpu_ctx, name, precision, winograd, n)
    x = _cuda(_model_input(name, n))
    with _model(gpu_ctx, _model_bytes(name), max_batch=n, precision=precision, winograd=winograd) as m:
        m.set_topk(k)
        m.set_views(2)
        plain = m.classify(x)
        scores, classes, maps = m.classify_cam(x)
        torch.cuda.synchronize()
        assert tuple(classes.shape) == (2, k) and tuple(maps.shape) == (n, k) + T.shape[2:]
        assert torch.equal(classes, plain[1]) and torch.equal(scores.view(torch.int32), plain[0].view(torch.int32))
        _assert_bits(maps.cpu().numpy(), _cam.gather(T, classes.cpu().numpy(), views=2))


def test_input_paths(gpu_ctx):
    """classify_cam_u8 and classify_cam_u8_list give the maps of classify_cam on the converted float input"""
    import torch
    import ore
    name, n, k = "c64r", 3, 4
    C, M, H, W = _cam.GRAPHS[name][:4]
    rng = np.random.default_rng(5)
    x8 = _cuda(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8))
    scale, shift = np.array([1 / 64.0, 1 / 32.0, 1 / 128.0], np.float32), np.array([-2.0, -4.0, -1.0], np.float32)
    with _model(gpu_ctx, _model_bytes(name), max_batch=n) as m:
        m.set_topk(k)
        m.set_input_norm(scale, shift)
        want = m.classify_cam(ore.preprocess_u8(gpu_ctx, x8, scale, shift))
        got8 = m.classify_cam_u8(x8)
        lst = ore.ImageList(gpu_ctx, n, (H, W), 3)
        try:  # list images of their own sizes, resized: against the list's own conversion
            srcs = [_cuda(rng.integers(0, 256, (H + 3 * i, W + 2 * i, 3), dtype=np.uint8)) for i in range(n)]
            lst.set(srcs)
            wantl = m.classify_cam(ore.preprocess_list_u8(gpu_ctx, lst, scale, shift))
            gotl = m.classify_cam_u8_list(lst)
            torch.cuda.synchronize()
        finally:
            lst.close()
        assert not torch.equal(wantl[2], want[2])
        for got, ref in ((got8, want), (gotl, wantl)):
            assert torch.equal(got[1], ref[1])
            for a, b in ((got[0], ref[0]), (got[2], ref[2])):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert tuple(want[2].shape) == (n, k, H, W) and float(want[2].abs().max()) > 0


def test_captures():
    """capture_classify with a buffer set: a replay on new input bytes gives the new maps; a capture taken with
    the maps off writes nothing to a poisoned buffer"""
    import torch
    import ore
    name, n, k = "c32", 3, 5
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    m = ore.Model(ctx, _model_bytes(name), max_batch=n)
    try:
        m.set_topk(k)
        xa, xb = _cuda(_model_input(name)), _cuda(_model_input(name)[::-1].copy() * np.float32(0.5))
        torch.cuda.synchronize()
        wants = [m.classify_cam(x) for x in (xa, xb)]
        s.synchronize()
        assert not torch.equal(wants[0][2], wants[1][2])
        x = xa.clone()
        scores = torch.empty((n, k), dtype=torch.float32, device="cuda")
        classes = torch.empty((n, k), dtype=torch.int32, device="cuda")
        maps = torch.full((n, k) + m.cam_hw, float("nan"), device="cuda")
        torch.cuda.synchronize()
        m.set_cam_output(maps)
        m.capture_classify(x, scores, classes)  # capture only: nothing runs yet
        for want, src in zip(wants, (xa, xb)):
            x.copy_(src)
            torch.cuda.synchronize()
            m.replay()
            s.synchronize()
            assert torch.equal(classes, want[1]) and torch.equal(maps.view(torch.int32), want[2].view(torch.int32))
        # another buffer does not reach the captured graph; off, a new capture writes no maps
        other = torch.full((n, k) + m.cam_hw, float("nan"), device="cuda")
        torch.cuda.synchronize()
        m.set_cam_output(other)
        m.replay()
        s.synchronize()
        assert torch.isnan(other).all() and torch.equal(maps.view(torch.int32), wants[1][2].view(torch.int32))
        m.set_cam_output(None)
        maps.fill_(float("nan"))
        torch.cuda.synchronize()
        m.capture_classify(x, scores, classes)
        m.replay()
        s.synchronize()
        assert torch.isnan(maps).all() and torch.isnan(other).all() and torch.equal(classes, wants[1][1])
    finally:
        s.synchronize()
        m.close()
        ctx.close()


def test_chunked_maps(gpu_ctx):
    """As test_views_gpu.py::test_chunked_views (views not dividing the run batch): the maps of all n images equal
    the unchunked model's on the same images, taken in two halves"""
    import torch
    from ore import squeezenet
    k = 5
    mb = squeezenet.build(224)
    with _model(gpu_ctx, mb, max_batch=2048) as m:
        views = min(v for v in range(2, 8) if m.run_batch % v)
        n = (m.run_batch // (2 * views) + 1) * 2 * views
        assert m.run_batch < n <= 2048 and n % (2 * views) == 0
        g = torch.Generator(device="cuda").manual_seed(9)
        x = torch.rand((n, 3, 224, 224), dtype=torch.float32, device="cuda", generator=g)
        m.set_topk(k)
        m.set_views(views)
        scores, classes, maps = m.classify_cam(x)
        torch.cuda.synchronize()
    half = n // 2
    with _model(gpu_ctx, mb, max_batch=half) as m:
        assert m.run_batch == half
        m.set_topk(k)
        m.set_views(views)
        for j in range(2):
            s2, c2, m2 = m.classify_cam(x[j * half:(j + 1) * half])
            torch.cuda.synchronize()
            g0, g1 = j * half // views, (j + 1) * half // views
            assert torch.equal(c2, classes[g0:g1]) and torch.equal(s2.view(torch.int32), scores[g0:g1].view(torch.int32))
            assert torch.equal(m2.view(torch.int32), maps[j * half:(j + 1) * half].view(torch.int32))


def _plan_state(m):
    arena = [b for b in m.scratch_buffers() if b[0] == "arena"]
    return [(s["op"], s["name"]) for s in m.steps()], m.tiles(), int(m.run_batch), arena[0][2] if arena else 0


def test_errors(gpu_ctx):
    import torch
    import warnings
    import ore
    L = ore.load()
    name, n, k = "c32", 3, 5
    x = _cuda(_model_input(name))
    # a model without a map conv
    with open(os.path.join(GOLD, "mnist-8.onnx"), "rb") as f:
        mnist = f.read()
    with _model(gpu_ctx, mnist, max_batch=2) as m:
        buf = torch.zeros(64, device="cuda")
        for call in (lambda: m.cam_hw, lambda: m.set_cam_output(buf)):
            with pytest.raises(ore.OreError, match="no map conv") as e:
                call()
            assert e.value.status == 2  # ORE_ERR_UNSUPPORTED
        assert "Add" in str(e.value) or "MatMul" in str(e.value)  # names what it found
        m.set_cam_output(None)  # off is always fine
        y = m.run(torch.zeros((1, 1, 28, 28), device="cuda"))
        torch.cuda.synchronize()
        assert tuple(y.shape) == (1, 10)
    with _model(gpu_ctx, _model_bytes(name), max_batch=n) as m:
        m.set_topk(k)
        before = _plan_state(m)
        want = m.classify_cam(x)
        torch.cuda.synchronize()
        assert _plan_state(m) == before  # classify_cam restored the setting
        hw = m.cam_hw
        # the buffer too small: before any device call, for every classify entry
        small = torch.zeros(n * k * hw[0] * hw[1] - 1, device="cuda")
        m.set_cam_output(small)
        on = _plan_state(m)
        s = torch.empty((n, k), dtype=torch.float32, device="cuda")
        c = torch.empty((n, k), dtype=torch.int32, device="cuda")
        for fn in (m.classify_into, m.capture_classify):
            with pytest.raises(ore.OreError, match="class maps") as e:
                fn(x, s, c)
            assert e.value.status == 1
        assert float(small.abs().max()) == 0.0
        assert tuple(m.run(x).shape) == (n, m.output_elems)  # run* ignores the setting
        # inside a stream capture of the caller's: turning the maps off would replan
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        ctx2 = ore.Context(0, use_torch_stream=False)
        ctx2.set_stream(side.cuda_stream)
        m2 = ore.Model(ctx2, _model_bytes(name), max_batch=n)
        try:
            full = torch.zeros((n, k) + hw, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                g.capture_begin()
                try:
                    with pytest.raises(ore.OreError, match="capture") as refused:
                        m2.set_cam_output(full)
                finally:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")  # torch remarks that the captured graph is empty
                        g.capture_end()
            assert refused.value.status == 1
            m2.set_topk(k)
            got = m2.classify_cam(x)  # the model stays usable
            side.synchronize()
            assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))
        finally:
            side.synchronize()
            m2.close()
            ctx2.close()
        # the first model stays usable after its errors, on a buffer that is large enough
        full = torch.zeros((n, k) + hw, device="cuda")
        m.set_cam_output(full)
        assert _plan_state(m) == on  # another pointer does not replan
        m.classify_into(x, s, c)
        torch.cuda.synchronize()
        assert torch.equal(full.view(torch.int32), want[2].view(torch.int32)) and torch.equal(c, want[1])
        m.set_cam_output(None)
        assert _plan_state(m) == before  # the step list, tiles, run batch and arena size from before it was enabled
        _assert_bits(m.classify(x)[0].cpu().numpy(), want[0].cpu().numpy())
