"""GPU: localisation from class activation maps (ore_upsample_maps_f32, ore_cam_boxes_f32, ore_model_set_cam_boxes;
csrc/ore_cam_box.hip).  Everything here is exact: integers, or float32 bits (a NaN is compared as a NaN: the sign and
payload of a NaN that an operation produces, inf - inf, differ between processors and are not part of the contract).

Per-op entries, over the case table of _cam_boxes.cases(): the upsampled planes equal the numpy restatement bit for bit,
written into a NaN-poisoned buffer whose guard bands come back untouched and in which no element stays unwritten; the
boxes and areas equal the reference (numpy threshold + a pure-Python labelling, itself checked against scipy and the
library's host entry in tests/test_cam_boxes.py), with areas given and NULL, guard bands around both outputs; and they
equal the reference applied to the planes the GPU upsampled.

Model level, on the graphs of _cam.GRAPHS and SqueezeNet at 64, f32 direct, f32 Winograd and f16: classify_boxes
returns the scores, classes and maps of classify_cam bit for bit and the reference's boxes for those maps; the same
under views, through the uint8 entries, through a captured graph replayed on new input and on a chunked run; then the
errors, and that a model whose boxes were set and turned off answers as one that never had them."""
import contextlib
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest

import _cam
import _cam_boxes as cb

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON = np.int32(0x7FC5A5A5)  # a quiet NaN no kernel computes, and no box or area
GUARD = 96                     # poisoned words on either side of every output
PRECISIONS = [("f32", False), ("f32", True), ("f16", True)]  # (precision, winograd)
PREC_IDS = ["f32-direct", "f32-wino", "f16"]


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the case table's arrays are read-only


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same_floats(got, want, what=""):
    """Equal bits wherever the reference is a number, a NaN wherever it is a NaN: the payload and the sign of a NaN
    that an operation produces (inf - inf) differ between processors and are no part of the contract."""
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want.view(np.float32))
    np.testing.assert_array_equal(np.isnan(got.view(np.float32)), nan, err_msg=what)
    np.testing.assert_array_equal(got[~nan], want[~nan], err_msg=what)


def _poisoned(words):
    import torch
    return torch.full((GUARD + words + GUARD,), int(POISON), dtype=torch.int32, device="cuda")


def _split(buf, words):
    """(the payload, guard bands intact?) of a _poisoned buffer after a launch"""
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + words].copy(), bool((host[:GUARD] == POISON).all() and (host[GUARD + words:] == POISON).all())


def _ptr(buf):
    return ctypes.c_void_p(buf.data_ptr() + 4 * GUARD)


@contextlib.contextmanager
def _model(ctx, onnx_bytes, **kw):
    import ore
    m = ore.Model(ctx, onnx_bytes, **kw)
    try:
        yield m
    finally:
        m.close()


def _reference_boxes(maps, hw, frac):
    """(boxes [..., 4], areas [...]) of the numpy + pure-Python reference for float32 maps [..., Hm, Wm]"""
    maps = np.asarray(maps, dtype=np.float32)
    flat = maps.reshape((-1,) + maps.shape[-2:])
    res = [cb.box_of(cb.upsample(p, hw), frac) for p in flat]
    lead = maps.shape[:-2]
    return (np.array([r[0] for r in res], np.int32).reshape(lead + (4,)), np.array([r[1] for r in res], np.int32).reshape(lead))


# ------------------------------------------------------------------------------------------ the per-op entries
@functools.lru_cache(maxsize=None)
def _op_result(ctx, name):
    """Every launch of a case, once: (upsampled planes, guards intact), (boxes, areas, guards intact) with areas
    given, (boxes, guards intact) with areas NULL, and the wrappers' results"""
    import torch
    import ore
    from ore import _lib
    _, maps, (H, W), frac = next(c for c in cb.cases() if c[0] == name)
    planes, hm, wm = maps.shape
    L = ore.load()
    md = _cuda(maps)
    up = _poisoned(planes * H * W)
    _lib.check(L.ore_upsample_maps_f32(ctx.h, ctypes.c_void_p(md.data_ptr()), planes, hm, wm, H, W, _ptr(up)), ctx.h)
    bx, ar, bx2 = _poisoned(planes * 4), _poisoned(planes), _poisoned(planes * 4)
    _lib.check(L.ore_cam_boxes_f32(ctx.h, ctypes.c_void_p(md.data_ptr()), planes, hm, wm, H, W, frac, _ptr(bx), _ptr(ar)), ctx.h)
    _lib.check(L.ore_cam_boxes_f32(ctx.h, ctypes.c_void_p(md.data_ptr()), planes, hm, wm, H, W, frac, _ptr(bx2), None), ctx.h)
    wu = ore.upsample_maps(ctx, md, (H, W))
    wb, wa = ore.cam_boxes(ctx, md, (H, W), frac)
    torch.cuda.synchronize()
    u, u_ok = _split(up, planes * H * W)
    b, b_ok = _split(bx, planes * 4)
    a, a_ok = _split(ar, planes)
    b2, b2_ok = _split(bx2, planes * 4)
    return ((u.reshape(planes, H, W), u_ok), (b.reshape(planes, 4), a, b_ok and a_ok), (b2.reshape(planes, 4), b2_ok),
            (wu.cpu().numpy(), wb.cpu().numpy(), wa.cpu().numpy()))


@pytest.mark.parametrize("case", cb.cases(), ids=cb.case_id)
def test_upsample_is_the_numpy_restatement_bit_for_bit(gpu_ctx, case):
    (u, intact), _, _, (wu, _, _) = _op_result(gpu_ctx, case[0])
    want = cb.reference(case[0])[0]
    assert intact, "the guard bands around the upsampled planes were written"
    assert not (u == POISON).any(), "an element was not written"
    _assert_same_floats(u.view(np.float32), want)
    np.testing.assert_array_equal(_bits(wu), u.view(np.uint32), err_msg="ore.upsample_maps against the raw entry")


@pytest.mark.parametrize("case", cb.cases(), ids=cb.case_id)
def test_boxes_equal_the_reference(gpu_ctx, case):
    _, (b, a, intact), (b2, intact2), (_, wb, wa) = _op_result(gpu_ctx, case[0])
    _, boxes, areas = cb.reference(case[0])
    print(f"cam boxes {case[0]}: boxes {b.tolist()} areas {a.tolist()}")
    assert intact and intact2, "the guard bands around boxes or areas were written"
    np.testing.assert_array_equal(b, boxes)
    np.testing.assert_array_equal(a, areas)
    np.testing.assert_array_equal(b2, boxes, err_msg="with areas NULL")
    np.testing.assert_array_equal(wb, boxes, err_msg="ore.cam_boxes")
    np.testing.assert_array_equal(wa, areas, err_msg="ore.cam_boxes")


@pytest.mark.parametrize("case", cb.cases(), ids=cb.case_id)
def test_boxes_equal_the_reference_on_the_gpu_s_planes(gpu_ctx, case):
    (u, _), (b, a, _), _, _ = _op_result(gpu_ctx, case[0])
    frac = case[3]
    for p in range(len(u)):
        box, area = cb.box_of(u[p].view(np.float32), frac)
        assert (tuple(b[p]), int(a[p])) == (box, area), (case[0], p)


def test_wrappers_keep_leading_dims_and_empty_batches(gpu_ctx):
    import torch
    import ore
    maps = _cuda(np.random.default_rng(3).standard_normal((2, 3, 4, 5)).astype(np.float32))
    up = ore.upsample_maps(gpu_ctx, maps, (9, 11))
    boxes, areas = ore.cam_boxes(gpu_ctx, maps, (9, 11), 0.5)
    torch.cuda.synchronize()
    assert tuple(up.shape) == (2, 3, 9, 11) and tuple(boxes.shape) == (2, 3, 4) and tuple(areas.shape) == (2, 3)
    wb, wa = _reference_boxes(maps.cpu().numpy(), (9, 11), 0.5)
    assert np.array_equal(boxes.cpu().numpy(), wb) and np.array_equal(areas.cpu().numpy(), wa)
    empty = torch.empty((0, 4, 5), device="cuda")
    assert tuple(ore.upsample_maps(gpu_ctx, empty, (9, 11)).shape) == (0, 9, 11)
    assert tuple(ore.cam_boxes(gpu_ctx, empty, (9, 11))[0].shape) == (0, 4)
    p = ctypes.c_void_p(0x1000)  # planes == 0 launches nothing: never dereferenced
    assert ore.load().ore_upsample_maps_f32(gpu_ctx.h, p, 0, 4, 5, 9, 11, p) == 0
    assert ore.load().ore_cam_boxes_f32(gpu_ctx.h, p, 0, 4, 5, 9, 11, 0.2, p, None) == 0
    with pytest.raises(ore.OreError, match="ORE_CAM_BOX_MAX_SIDE"):
        ore.cam_boxes(gpu_ctx, maps, (513, 11))
    with pytest.raises(ore.OreError, match="below"):
        ore.upsample_maps(gpu_ctx, maps, (3, 11))


# ------------------------------------------------------------------------------------------ model level
def _model_bytes(name):
    from ore import squeezenet
    return squeezenet.build(int(name[2:])) if name.startswith("sq") else _cam.graph_bytes(name)


def _model_input(name, n=_cam.BATCH):
    from ore import squeezenet
    if name.startswith("sq"):
        return squeezenet.synthetic_input(n, int(name[2:]), seed=_cam.SQ_SEED)
    return np.asarray(_cam.graph_input(name, n))


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _assert_boxes_of(res, in_hw, frac, what=""):
    """boxes and areas of a classify_boxes result are the reference's for its own maps"""
    import torch
    torch.cuda.synchronize()
    scores, classes, maps, boxes, areas = res
    assert tuple(boxes.shape) == tuple(maps.shape[:2]) + (4,) and tuple(areas.shape) == tuple(maps.shape[:2]), what
    wb, wa = _reference_boxes(maps.cpu().numpy(), in_hw, frac)
    np.testing.assert_array_equal(boxes.cpu().numpy(), wb, err_msg=what)
    np.testing.assert_array_equal(areas.cpu().numpy(), wa, err_msg=what)


MODELS = sorted(_cam.GRAPHS) + ["sq64"]


@pytest.mark.parametrize("precision,winograd", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("name", MODELS)
def test_model_boxes(gpu_ctx, name, precision, winograd):
    import torch
    k, n = _cam.TOPK, _cam.BATCH
    x = _cuda(_model_input(name))
    with _model(gpu_ctx, _model_bytes(name), max_batch=n, precision=precision, winograd=winograd) as m:
        m.set_topk(k)
        in_hw = tuple(m.input_dims[1:])
        want = m.classify_cam(x)
        for frac in (0.2, 0.6):
            what = f"{name} {precision} wino={winograd} frac={frac}"
            got = m.classify_boxes(x, frac)
            torch.cuda.synchronize()
            assert torch.equal(got[1], want[1]) and _same_bits(got[0], want[0]) and _same_bits(got[2], want[2]), what
            assert tuple(got[2].shape) == (n, k) + m.cam_hw
            _assert_boxes_of(got, in_hw, frac, what)
        assert int(got[4].max()) > 0
        # set once, classify_into: the documented way for repeated calls; areas left out
        maps = torch.empty_like(want[2])
        boxes = torch.full((n, k, 4), int(POISON), dtype=torch.int32, device="cuda")
        s, c = torch.empty_like(want[0]), torch.empty_like(want[1])
        m.set_cam_output(maps)
        m.set_cam_boxes(boxes, None, 0.6)
        m.classify_into(x, s, c)
        torch.cuda.synchronize()
        assert _same_bits(maps, want[2]) and torch.equal(boxes, got[3])
        m.set_cam_output(None)


def test_views(gpu_ctx):
    """views = 3 with n = 6: boxes are per image, as the maps are"""
    import torch
    name, n, k = "c32", 6, 3
    x = _cuda(_model_input(name, n))
    with _model(gpu_ctx, _model_bytes(name), max_batch=n) as m:
        m.set_topk(k)
        m.set_views(3)
        want = m.classify_cam(x)
        got = m.classify_boxes(x)
        torch.cuda.synchronize()
        assert tuple(got[1].shape) == (2, k) and tuple(got[3].shape) == (n, k, 4) and tuple(got[4].shape) == (n, k)
        assert torch.equal(got[1], want[1]) and _same_bits(got[0], want[0]) and _same_bits(got[2], want[2])
        _assert_boxes_of(got, tuple(m.input_dims[1:]), 0.2)


def test_input_paths(gpu_ctx):
    """classify_boxes_u8 and classify_boxes_u8_list give the boxes of classify_boxes on the converted float input"""
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
        want = m.classify_boxes(ore.preprocess_u8(gpu_ctx, x8, scale, shift), 0.5)
        got8 = m.classify_boxes_u8(x8, 0.5)
        lst = ore.ImageList(gpu_ctx, n, (H, W), 3)
        try:
            srcs = [_cuda(rng.integers(0, 256, (H + 3 * i, W + 2 * i, 3), dtype=np.uint8)) for i in range(n)]
            lst.set(srcs)
            wantl = m.classify_boxes(ore.preprocess_list_u8(gpu_ctx, lst, scale, shift), 0.5)
            gotl = m.classify_boxes_u8_list(lst, 0.5)
            torch.cuda.synchronize()
        finally:
            lst.close()
        for got, ref in ((got8, want), (gotl, wantl)):
            assert torch.equal(got[1], ref[1]) and _same_bits(got[0], ref[0]) and _same_bits(got[2], ref[2])
            assert torch.equal(got[3], ref[3]) and torch.equal(got[4], ref[4])
            _assert_boxes_of(got, (H, W), 0.5)
        assert not torch.equal(wantl[2], want[2])


def test_captures():
    """capture_classify with maps and boxes set: a replay on new input bytes gives the new boxes; the captured graph
    keeps the setting it was captured with"""
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
        wants = [m.classify_boxes(x, 0.6) for x in (xa, xb)]
        s.synchronize()
        for w in wants:
            _assert_boxes_of(w, tuple(m.input_dims[1:]), 0.6)
        assert not torch.equal(wants[0][3], wants[1][3])
        x = xa.clone()
        scores = torch.empty((n, k), dtype=torch.float32, device="cuda")
        classes = torch.empty((n, k), dtype=torch.int32, device="cuda")
        maps = torch.full((n, k) + m.cam_hw, float("nan"), device="cuda")
        boxes = torch.full((n, k, 4), int(POISON), dtype=torch.int32, device="cuda")
        areas = torch.full((n, k), int(POISON), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.set_cam_output(maps)
        m.set_cam_boxes(boxes, areas, 0.6)
        m.capture_classify(x, scores, classes)  # capture only: nothing runs yet
        for want, src in zip(wants, (xa, xb)):
            x.copy_(src)
            torch.cuda.synchronize()
            m.replay()
            s.synchronize()
            assert torch.equal(classes, want[1]) and _same_bits(maps, want[2])
            assert torch.equal(boxes, want[3]) and torch.equal(areas, want[4])
        # other buffers and another fraction do not reach the captured graph
        other = torch.full((n, k, 4), int(POISON), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.set_cam_boxes(other, None, 0.2)
        boxes.fill_(int(POISON))
        torch.cuda.synchronize()
        m.replay()
        s.synchronize()
        assert (other == int(POISON)).all() and torch.equal(boxes, wants[1][3])
    finally:
        s.synchronize()
        m.close()
        ctx.close()


def test_chunked_boxes(gpu_ctx):
    """max_batch above run_batch, views not dividing the run batch (as test_cam_gpu.py::test_chunked_maps): every
    chunk's boxes land at its own planes.  All planes against the per-op kernel on the returned maps; the planes on
    both sides of the chunk boundary and at both ends against the reference."""
    import torch
    import ore
    from ore import squeezenet
    k = 5
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        views = min(v for v in range(2, 8) if m.run_batch % v)
        n = (m.run_batch // (2 * views) + 1) * 2 * views
        assert m.run_batch < n <= 2048
        g = torch.Generator(device="cuda").manual_seed(9)
        x = torch.rand((n, 3, 224, 224), dtype=torch.float32, device="cuda", generator=g)
        m.set_topk(k)
        m.set_views(views)
        scores, classes, maps, boxes, areas = m.classify_boxes(x)
        torch.cuda.synchronize()
        chunk = -(-(n // views) // 2) * views  # two chunks of whole groups
    wb, wa = ore.cam_boxes(gpu_ctx, maps, (224, 224), 0.2)
    torch.cuda.synchronize()
    assert torch.equal(boxes, wb) and torch.equal(areas, wa) and int(areas.min()) > 0
    for i in (0, chunk - 1, chunk, n - 1):
        rb, ra = _reference_boxes(maps[i, :2].cpu().numpy(), (224, 224), 0.2)
        assert np.array_equal(boxes[i, :2].cpu().numpy(), rb) and np.array_equal(areas[i, :2].cpu().numpy(), ra), i


def test_errors(gpu_ctx):
    import torch
    import ore
    name, n, k = "c32", 3, 5
    x = _cuda(_model_input(name))
    poison = lambda *shape: torch.full(shape, int(POISON), dtype=torch.int32, device="cuda")  # noqa: E731
    # a model without a map conv
    with open(os.path.join(GOLD, "mnist-8.onnx"), "rb") as f:
        mnist = f.read()
    with _model(gpu_ctx, mnist, max_batch=2) as m:
        with pytest.raises(ore.OreError, match="no map conv") as e:
            m.set_cam_boxes(poison(2, 1, 4))
        assert e.value.status == 2  # ORE_ERR_UNSUPPORTED
        m.set_cam_boxes(None)  # off is always fine
    with _model(gpu_ctx, _model_bytes(name), max_batch=n) as m:
        m.set_topk(k)
        want = m.classify_cam(x)
        torch.cuda.synchronize()
        hw = m.cam_hw
        boxes = poison(n, k, 4)
        # the boxes with the maps off
        with pytest.raises(ore.OreError, match="maps are off") as e:
            m.set_cam_boxes(boxes)
        assert e.value.status == 1
        maps = torch.zeros((n, k) + hw, device="cuda")
        m.set_cam_output(maps)
        for frac in (-0.1, 1.5, float("nan")):
            with pytest.raises(ore.OreError, match="frac"):
                m.set_cam_boxes(boxes, None, frac)
        for bad in (torch.zeros((n, k, 4), device="cuda"), torch.zeros((n, k, 4), dtype=torch.int32), boxes[:, :, :2]):
            with pytest.raises(ore.OreError, match="boxes"):
                m.set_cam_boxes(bad)
        # the buffers too small (boxes, then areas): before any device call, for every classify entry
        s = torch.empty((n, k), dtype=torch.float32, device="cuda")
        c = torch.empty((n, k), dtype=torch.int32, device="cuda")
        for small_b, small_a in ((poison(n * k * 4 - 1), None), (boxes, poison(n * k - 1))):
            m.set_cam_boxes(small_b, small_a)
            for fn in (m.classify_into, m.capture_classify):
                with pytest.raises(ore.OreError, match="ore_model_set_cam_boxes") as e:
                    fn(x, s, c)
                assert e.value.status == 1
            torch.cuda.synchronize()
            assert (small_b == int(POISON)).all() and float(maps.abs().max()) == 0.0
        assert tuple(m.run(x).shape) == (n, m.output_elems)  # run* ignores the setting
        # the maps turned off while the boxes are set: the boxes go with them, a later classify writes none
        m.set_cam_boxes(boxes)
        m.set_cam_output(None)
        got = m.classify(x)
        torch.cuda.synchronize()
        assert (boxes == int(POISON)).all() and torch.equal(got[1], want[1]) and _same_bits(got[0], want[0])
        with pytest.raises(ore.OreError, match="maps are off"):
            m.set_cam_boxes(boxes)
        # a model whose boxes were set and turned off answers as one that never had them
        again = m.classify_cam(x)
        torch.cuda.synchronize()
        assert torch.equal(again[1], want[1]) and _same_bits(again[0], want[0]) and _same_bits(again[2], want[2])
    # inside a stream capture of the caller's
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    ctx2 = ore.Context(0, use_torch_stream=False)
    ctx2.set_stream(side.cuda_stream)
    m2 = ore.Model(ctx2, _model_bytes(name), max_batch=n)
    try:
        m2.set_topk(k)
        maps2 = torch.zeros((n, k) + hw, device="cuda")
        boxes2 = poison(n, k, 4)
        m2.set_cam_output(maps2)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            g.capture_begin()
            try:
                with pytest.raises(ore.OreError, match="capture") as refused:
                    m2.set_cam_boxes(boxes2)
            finally:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # torch remarks that the captured graph is empty
                    g.capture_end()
        assert refused.value.status == 1
        m2.set_cam_boxes(boxes2)  # the model stays usable
        m2.classify(x)
        side.synchronize()
        wb, wa = _reference_boxes(want[2].cpu().numpy(), tuple(m2.input_dims[1:]), 0.2)
        assert _same_bits(maps2, want[2]) and np.array_equal(boxes2.cpu().numpy(), wb)
    finally:
        side.synchronize()
        m2.close()
        ctx2.close()
