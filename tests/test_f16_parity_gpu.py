"""The fp16 conv kernels (ORE_LOAD_F16) against a float64 reference, layer by layer.

One fp16 conv layer computes  y = RNE_f16(relu?(sum_k f16(x_k) f16(w_k) [f32 accumulate] + b_f32)).
_convref.f16_layer_check holds every output to that: it must be the correctly rounded f16 of some value
within 2e-6 * (sum |w x| + |b|) of the float64 sum over the f16 operands -- for most outputs one f16
value, bit for bit.  Each layer is checked in isolation: the reference input of layer i is read_value
of layer i - 1's output (the GPU's own f16 values), of the first layer the f32 model input.  Every case
runs on each of the four block tiles and asserts that its convs report that tile.

This anchors the unfused conv_f16_kernel (tap-pair, f32 NCHW, per-element NHWC gathers) and
conv_f16_dma_kernel (16-B NHWC); test_f16_gpu.py's fused == unfused bit-identity tests carry it to the
fused kernels, and one launch of each fused fire kernel is held to the reference here as well.  Also
here: overflow to +-inf and f16 subnormal weights / activations / outputs, the scalar fp16 MaxPool
(channel counts that are no multiple of 8) and the unfused fp16 Concat.

Measured on MI355X over all layer cases: no output outside its interval, ambiguous share at most 0.1475
(cap 1/3), accumulation-error ratio at most 5.4e-8 (allowed 2e-6); every layer prints both."""
import contextlib

import numpy as np
import pytest

from _convref import F16_AMBIGUOUS_CAP, f16_layer_bounds, f16_layer_check
from _f16_models import FIRE_F16_CASES, FIRE_POOL_F16_CASES, _chain_model, _fire_model_f16
from _knobs import conv_tile

import oracle

pytestmark = pytest.mark.gpu

F16_MIN_NORMAL = 2.0 ** -14
MEASURED = {"acc_ratio": 0.0, "ambiguous": 0.0}  # running maxima over the layers checked so far (printed)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@contextlib.contextmanager
def _loaded(gpu_ctx, model_bytes, max_batch, fusion, tile=-1):
    """An f16 model planned on block tile `tile`, closed on the way out also when the test fails: a model
    must not outlive the session's context (ore_model_destroy reads it)."""
    import ore
    with conv_tile(gpu_ctx, tile):
        m = ore.Model(gpu_ctx, model_bytes, max_batch=max_batch, precision="f16")
    try:
        m.set_fusion(fusion)
        yield m
    finally:
        m.close()


def _weights(rng, M, C, k, bias, scale=1.0):
    w = (rng.standard_normal((M, C, k, k)) * np.sqrt(2.0 / (C * k * k)) * scale).astype(np.float32)
    b = (rng.uniform(-0.1, 0.1, M) * scale).astype(np.float32) if bias else None
    return w, b


def _check_layers(m, x, layers, tag):
    """f16_layer_check on every conv of a _chain_model run (m holds the values of a run on x)."""
    inp = x
    for i, (w, b, pads, strides, relu) in enumerate(layers):
        out = m.read_value(f"r{i}" if relu else f"c{i}")
        if i > 0:  # the GPU's own f16 values: they survive the reference's cast to f16 unchanged
            assert np.array_equal(inp.astype(np.float16).astype(np.float32), inp)
        res = f16_layer_check(out, inp, w, b, pads, strides, relu)
        MEASURED["acc_ratio"] = max(MEASURED["acc_ratio"], res["acc_ratio"])
        MEASURED["ambiguous"] = max(MEASURED["ambiguous"], res["ambiguous"])
        print(f"f16 parity {tag} layer {i} K={w[0].size}: ambiguous {res['ambiguous']:.4f} acc_ratio "
              f"{res['acc_ratio']:.3e} bad {res['bad']:.5f} | max so far: ambiguous {MEASURED['ambiguous']:.4f} "
              f"acc_ratio {MEASURED['acc_ratio']:.3e}")
        assert res["ambiguous"] <= F16_AMBIGUOUS_CAP
        bad = np.argwhere(~res["ok"])
        assert bad.size == 0, (f"{tag} layer {i}: {len(bad)} of {out.size} outputs outside the f16 contract; first "
                               f"(n, m, oh, ow): got / nearest f16 = "
                               + ", ".join(f"{tuple(j)}: {out[tuple(j)]!r} / {res['ref'][tuple(j)]!r}" for j in bad[:8]))
        inp = out
    return inp


# id, (N, C, H, W), [(M, k, stride, pads t l b r, bias, relu)]: the last conv is the layer under test, a
# leading 1x1 puts its input into the f16 NHWC layout (and is itself a conv on the f32 NCHW input)
LAYER_CASES = [
    ("pair-7x7s2", (2, 3, 23, 23), [(96, 7, 2, [0, 0, 0, 0], True, True)]),     # conv1 geometry, padded 8th tap, 96-row tile
    ("pair-5x5", (1, 4, 12, 13), [(24, 5, 1, [2, 2, 2, 2], True, False)]),      # odd kw: the padding tap; all four pads
    ("pair-c1", (2, 1, 9, 9), [(20, 3, 2, [1, 0, 0, 1], False, False)]),        # C = 1, M % 8 != 0 (scalar store), uneven pads
    ("nchw-3x3", (2, 5, 17, 19), [(64, 3, 1, [1, 1, 1, 1], True, True)]),       # per-element f32 gather rounded while staging
    ("nchw-k117", (1, 13, 11, 7), [(33, 3, 2, [0, 1, 1, 0], False, False)]),    # K = 117: ragged last k stage, ragged M
    ("nchw-1x1", (3, 8, 9, 9), [(20, 1, 1, [0, 0, 0, 0], True, False)]),        # 1x1 on the f32 input
    ("vec-k576", (2, 8, 13, 13), [(64, 1, 1, [0] * 4, True, True), (64, 3, 1, [1, 1, 1, 1], True, True)]),   # fire9's expand3x3
    ("vec-k16", (2, 8, 12, 12), [(16, 1, 1, [0] * 4, True, True), (64, 1, 1, [0] * 4, True, True)]),         # less than one k stage
    ("vec-k512", (1, 8, 6, 6), [(512, 1, 1, [0] * 4, True, True), (200, 1, 1, [0] * 4, True, True)]),        # conv10-like, M % 128 != 0
    ("vec-k216s2", (2, 8, 15, 14), [(24, 1, 1, [0] * 4, True, True), (40, 3, 2, [0, 0, 1, 1], False, False)]),  # ragged stage, stride 2
    ("vec-k72", (3, 8, 9, 9), [(8, 1, 1, [0] * 4, True, True), (130, 3, 1, [1, 1, 1, 1], True, False)]),     # K = 72, M % 8 != 0
    ("elem-3x3", (2, 8, 9, 9), [(20, 1, 1, [0] * 4, True, True), (130, 3, 1, [1, 1, 1, 1], True, True)]),    # C % 8 != 0 gather
    ("elem-tiny", (2, 8, 7, 5), [(12, 1, 1, [0] * 4, True, True), (7, 1, 1, [0] * 4, False, False)]),        # tiny M, < one tile of columns
]


def _case_layers(idx):
    _, (N, C, H, W), spec = LAYER_CASES[idx]
    rng = np.random.default_rng(1000 + idx)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    layers, cin = [], C
    for M, k, s, pads, bias, relu in spec:
        w, b = _weights(rng, M, cin, k, bias)
        layers.append((w, b, pads, [s, s], relu))
        cin = M
    return x, layers


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("idx", range(len(LAYER_CASES)), ids=[c[0] for c in LAYER_CASES])
def test_f16_conv_layer_vs_float64(gpu_ctx, idx, cfg):
    import ore
    x, layers = _case_layers(idx)
    mb = _chain_model((1,) + x.shape[1:], layers)
    with _loaded(gpu_ctx, mb, x.shape[0], ore.FUSE_ALL | ore.KEEP_VALUES, tile=cfg) as m:
        _np(m.run(_t(x)))
        assert [t for t in m.tiles() if t >= 0] == [cfg] * len(layers), m.tiles()  # no silent fall-back to another tile
        _check_layers(m, x, layers, f"{LAYER_CASES[idx][0]} tile {ore.Model.TILE_NAMES[cfg]}")


def _special_chain(gpu_ctx, s1, s2, bias2, tag):
    """2 x 8 x 6 x 6 -> 1x1 -> 16 (bias, Relu; weights and bias x s1) -> 1x1 -> 16 (weights x s2), both layers
    through the sharp check: (layers, first layer's output, second layer's output)."""
    import ore
    rng = np.random.default_rng(77)
    x = rng.standard_normal((2, 8, 6, 6)).astype(np.float32)
    w1, b1 = _weights(rng, 16, 8, 1, True, s1)
    w2, b2 = _weights(rng, 16, 16, 1, bias2, s2)
    layers = [(w1, b1, [0] * 4, [1, 1], True), (w2, b2, [0] * 4, [1, 1], False)]
    with _loaded(gpu_ctx, _chain_model((1, 8, 6, 6), layers), 2, ore.FUSE_ALL | ore.KEEP_VALUES) as m:
        _np(m.run(_t(x)))
        out = _check_layers(m, x, layers, tag)
        return layers, m.read_value("r0"), out


def test_f16_conv_overflow_is_inf(gpu_ctx):
    """Outputs past 65504 in magnitude are +-inf, numpy's float16 cast: the kernels round with a plain
    (_Float16) cast and do not clamp."""
    layers, r0, out = _special_chain(gpu_ctx, 2.0 ** 6, 2.0 ** 9, True, "overflow")
    S = f16_layer_check(out, r0, *layers[1])["ref"]
    assert (S == np.inf).sum() >= 3 and (S == -np.inf).sum() >= 3 and np.isfinite(S).sum() >= 3
    np.testing.assert_array_equal(out[np.isinf(S)], S[np.isinf(S)].astype(np.float32))
    assert not np.isnan(out).any()


def test_f16_conv_subnormal_weights(gpu_ctx):
    """Weights whose f16 values are all subnormal (x 2^-16) on activations of ~2^8: normal outputs that
    exist only if the matrix cores read subnormal A operands as they are."""
    layers, _, out = _special_chain(gpu_ctx, 2.0 ** 8, 2.0 ** -16, False, "subnormal weights")
    wh = np.abs(layers[1][0].astype(np.float16).astype(np.float64))
    assert (wh < F16_MIN_NORMAL).all() and (wh > 0).mean() > 0.9
    assert (np.abs(out) >= F16_MIN_NORMAL).mean() > 0.5


def test_f16_conv_subnormal_activations_and_outputs(gpu_ctx):
    """The first layer x 2^-18: its outputs -- the second layer's B operands -- are f16 subnormals, and so are
    the second layer's outputs (gradual underflow, as the float64 reference keeps it).  read_value converts
    them through half_bits_to_float's renormalising branch."""
    _, r0, out = _special_chain(gpu_ctx, 2.0 ** -18, 1.0, False, "subnormal outputs")
    for v in (r0, out):
        a = np.abs(v)
        assert (a < F16_MIN_NORMAL).all() and (a > 0).mean() > 0.3, (a.max(), (a > 0).mean())


def _pool_model(x_shape, w, b, kernel, strides, auto_pad, pads):
    from ore import onnx_wire as wr
    attrs = [wr.encode_attr_ints("kernel_shape", kernel), wr.encode_attr_ints("strides", strides),
             wr.encode_attr_string("auto_pad", auto_pad)]
    if pads is not None:
        attrs.append(wr.encode_attr_ints("pads", pads))
    nodes = [wr.encode_node("Conv", ["x", "w", "b"], ["c0"], attrs=[wr.encode_attr_ints("pads", [0] * 4),
                                                                     wr.encode_attr_ints("strides", [1, 1])]),
             wr.encode_node("MaxPool", ["c0"], ["p0"], attrs=attrs),
             wr.encode_node("GlobalAveragePool", ["p0"], ["y"])]
    vinfo = [wr.encode_value_info("x", x_shape), wr.encode_value_info("w", w.shape), wr.encode_value_info("b", b.shape)]
    return wr.encode_model("p", nodes, [wr.encode_tensor("w", w), wr.encode_tensor("b", b)], vinfo,
                           [wr.encode_value_info("y", (1, 1, 1, 1))])


@pytest.mark.parametrize("case", [
    # channels, H, W, kernel, strides, auto_pad, pads
    # plane sizes at which the last window of a padded side does reach the padding
    (20, 20, 16, [3, 3], [2, 2], "NOTSET", [0, 0, 1, 1]),   # SqueezeNet's pools (ceil mode as bottom / right pads)
    (20, 14, 10, [2, 2], [2, 2], "NOTSET", [0, 0, 0, 0]),
    (20, 9, 11, [3, 3], [1, 1], "SAME_UPPER", None),
    (20, 13, 8, [3, 2], [2, 1], "NOTSET", [1, 0, 0, 1]),
    (24, 20, 16, [3, 3], [2, 2], "NOTSET", [0, 0, 1, 1]),   # the 16-B vector kernel on the same pool (control)
], ids=["3x3s2-c20", "2x2s2-c20", "3x3s1-same-c20", "3x2s21-c20", "3x3s2-c24"])
def test_f16_maxpool_standalone_exact(gpu_ctx, case):
    """The separate fp16 MaxPool kernel -- its per-channel form at 20 channels, its 16-B form at 24 -- equals
    the reference's MaxPool of the pool's own input bit for bit.  The conv's bias of -2 makes most values
    negative, so a padding tap (read as 0) decides the windows whose own values are all negative."""
    import ore
    C, H, W, kernel, strides, auto_pad, pads = case
    rng = np.random.default_rng(C + H + W)
    x = rng.standard_normal((2, 8, H, W)).astype(np.float32)
    w, _ = _weights(rng, C, 8, 1, False)
    b = np.full(C, -2.0, np.float32)
    mb = _pool_model((1, 8, H, W), w, b, kernel, strides, auto_pad, pads)
    # without ORE_FUSE_CONV_POOL the pool stays a launch of its own
    with _loaded(gpu_ctx, mb, 2, (ore.FUSE_ALL & ~ore.FUSE_CONV_POOL) | ore.KEEP_VALUES) as m:
        _np(m.run(_t(x)))
        assert [s["op"] for s in m.steps()].count("MaxPool") == 1
        c0, p0 = m.read_value("c0"), m.read_value("p0")
    assert c0.shape == (2, C, H, W) and (c0 < 0).mean() > 0.8
    want = oracle.maxpool2d(c0, kernel, strides, auto_pad=auto_pad, pads=pads)
    np.testing.assert_array_equal(p0, want)
    assert (want < 0).any()
    if auto_pad != "NOTSET" or any(pads):
        assert (want == 0).any()  # windows that the zero padding won


def _concat_model(x_shape, wa, ba, wb, bb):
    from ore import onnx_wire as wr
    conv = lambda w, o: wr.encode_node("Conv", ["x", w, "b" + w], [o], attrs=[
        wr.encode_attr_ints("pads", [0] * 4), wr.encode_attr_ints("strides", [1, 1])])
    nodes = [conv("wa", "a"), conv("wb", "b"),
             wr.encode_node("Concat", ["a", "b"], ["cat"], attrs=[wr.encode_attr_int("axis", 1)]),
             wr.encode_node("GlobalAveragePool", ["cat"], ["y"])]
    inits, vinfo = [], [wr.encode_value_info("x", x_shape)]
    for n, t in (("wa", wa), ("bwa", ba), ("wb", wb), ("bwb", bb)):
        inits.append(wr.encode_tensor(n, t))
        vinfo.append(wr.encode_value_info(n, t.shape))
    return wr.encode_model("cc", nodes, inits, vinfo, [wr.encode_value_info("y", (1, 1, 1, 1))])


@pytest.mark.parametrize("chans", [(20, 12), (24, 40)])
def test_f16_concat_unfused_exact(gpu_ctx, chans):
    """The fp16 Concat kernel at channel counts that are no multiple of 64 (20 + 12: slices that are not 16-B
    aligned) equals np.concatenate of its inputs bit for bit, and the in-place Concat of ORE_FUSE_CONCAT
    (the convs store channel slices) equals it."""
    import ore
    ca, cb = chans
    rng = np.random.default_rng(ca * 100 + cb)
    x = rng.standard_normal((3, 8, 9, 7)).astype(np.float32)
    (wa, ba), (wb, bb) = _weights(rng, ca, 8, 1, True), _weights(rng, cb, 8, 1, True)
    mb = _concat_model((1, 8, 9, 7), wa, ba, wb, bb)
    vals = []
    for fusion in (ore.KEEP_VALUES, ore.FUSE_ALL | ore.KEEP_VALUES):
        with _loaded(gpu_ctx, mb, 3, fusion) as m:
            y = _np(m.run(_t(x)))
            assert ("Concat" in [s["op"] for s in m.steps()]) == (fusion == ore.KEEP_VALUES)
            a, b, cat = m.read_value("a"), m.read_value("b"), m.read_value("cat")
        assert a.shape == (3, ca, 9, 7) and b.shape == (3, cb, 9, 7)
        np.testing.assert_array_equal(cat, np.concatenate([a, b], axis=1))
        vals.append((cat, y))
    np.testing.assert_array_equal(vals[0][0], vals[1][0])
    np.testing.assert_array_equal(vals[0][1], vals[1][1])
    assert np.abs(vals[0][0]).min() > 0 and (vals[0][0] < 0).any()  # real data in every slot


def _gap_f32(v):
    """GlobalAveragePool as the f16 path computes it: the pixels summed in order in f32, / their count.  Every
    step is a rounded, hence monotone, operation: the GAP of an elementwise bound bounds the GAP."""
    n, c = v.shape[:2]
    px = v.reshape(n, c, -1).astype(np.float32)
    s = np.zeros((n, c), np.float32)
    for i in range(px.shape[2]):
        s = s + px[:, :, i]
    return s / np.float32(px.shape[2])


@pytest.mark.parametrize("pooled", [False, True], ids=["fire", "fire-pool"])
def test_f16_fused_fire_anchor(gpu_ctx, pooled):
    """One fused kernel against the float64 reference directly (the fused == unfused tests carry the rest):
    expand 1x1 + expand 3x3 + Concat (+ MaxPool) + the next squeeze in one fire_f16_kernel /
    fire_pool_f16_kernel launch, real-valued weights.  From the f16 values the launch reads, the reference
    gives each expand output's admissible f16 interval; MaxPool and Concat carry intervals as they are, and
    f16_layer_bounds pushes them through the squeeze.  The squeeze output and the model output (its GAP)
    must lie within."""
    import ore
    case = FIRE_POOL_F16_CASES[0] if pooled else FIRE_F16_CASES[0]
    C, H, W = case[:3]
    pool = case[7] if pooled else None
    n = 1 if pooled else 2
    mb, prm = _fire_model_f16(*case[:7], pool=pool)
    x = np.random.default_rng(sum(case[:7])).standard_normal((n, C, H, W)).astype(np.float32)
    with _loaded(gpu_ctx, mb, n, ore.FUSE_ALL | ore.FUSE_EAGER | ore.KEEP_VALUES) as m:
        y = _np(m.run(_t(x)))
        assert "fire f16" in [ore.Model.TILE_NAMES[t] for t in m.tiles() if t >= 0]
        with pytest.raises(ore.OreError):
            m.read_value("cat")  # inside the launch
        qr, nr = m.read_value("qr"), m.read_value("nr")
    one, same = ([0] * 4, (1, 1), True), ([1] * 4, (1, 1), True)
    assert f16_layer_check(qr, x, *prm["wq"], *one)["ok"].all()  # the squeeze in front reads the f32 input
    lo1, hi1 = f16_layer_bounds(qr, qr, *prm["w1"], *one)
    lo3, hi3 = f16_layer_bounds(qr, qr, *prm["w3"], *same)
    lo, hi = (np.concatenate(p, axis=1).astype(np.float32) for p in ((lo1, lo3), (hi1, hi3)))
    if pooled:  # the max of lower bounds bounds the max
        lo, hi = (oracle.maxpool2d(v, (3, 3), (2, 2), auto_pad="NOTSET", pads=pool) for v in (lo, hi))
    nlo, nhi = f16_layer_bounds(lo, hi, *prm["wn"], *one)
    print(f"f16 fused anchor {'fire-pool' if pooled else 'fire'}: expand outputs with two admissible values "
          f"{(lo1 != hi1).mean():.4f} / {(lo3 != hi3).mean():.4f}, squeeze outputs with more than one {(nlo != nhi).mean():.4f}")
    nh = nr.astype(np.float16)
    assert np.array_equal(nh.astype(np.float32), nr) and nr.max() > 0
    bad = np.argwhere(~((nlo <= nh) & (nh <= nhi)))
    assert bad.size == 0, (len(bad), [(tuple(j), nr[tuple(j)], nlo[tuple(j)], nhi[tuple(j)]) for j in bad[:8]])
    y = y.reshape(n, -1)
    assert (_gap_f32(nlo) <= y).all() and (y <= _gap_f32(nhi)).all()
    np.testing.assert_array_equal(y, _gap_f32(nr))
