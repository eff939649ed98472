"""Sliced and misaligned tensors through the per-op C ABI, every surrounding element poisoned (tests/_slices.py).

include/ore.h lets ore_conv2d_f32 and ore_maxpool2d_f32 take an x or a y that is a slice: images `nstride`
elements apart, a channel range of a wider tensor, a base of any 4-byte alignment.  Here every conv kernel family
(LDS-staged, streaming, Winograd) and every MaxPool variant gets such tensors on both sides, with a quiet NaN
(+inf for MaxPool, whose fmaxf drops a NaN) in every element of the input buffer that is not the tensor's -- the
lead, the gaps between images, the tail, the parent's other channels -- and one NaN bit pattern over the whole
output buffer.  A tap that is multiplied by a zero instead of being selected away, a pad column read from the
neighbouring plane, an epilogue that stores one element past its slice: each shows as a NaN (+inf) in the result
or as changed bits outside it.  The contiguous-only ops run at a base that is 4-byte but not 16-byte aligned.

Which kernel ran.  The per-op ABI does not report the tile.  A Winograd result differs in bits from the direct one
(asserted where H * W > 1), so a Winograd kernel ran; its tile is not visible (run_conv takes the first tile that
is eligible when the forced one is not).  For the streaming family NOTHING in the results shows which kernel ran:
its tiles are bit-identical to the LDS-staged ones by design, and a layout its predicates refuse falls back to
the LDS-staged kernel.  The layouts are chosen, by reading the predicates, so that the forced family stays
eligible on the aligned ones:
  * stream_mode (ore_conv_stream.hip) needs vec_out -- y's plane a multiple of 4 (every STREAM case), y->nstride
    % 4 == 0 and a 16-byte aligned y -- K % 16 == 0 and N * plane % 4 == 0; a 1x1 conv also needs a 16-byte
    aligned x with x_ps % 4 == 0 and x->nstride % 4 == 0; a 3x3 conv only a 4-byte aligned x with x_guard >=
    stream_lead, i.e. (W + 1) * 4 rounded up to 16 bytes (<= 64 here) of x's 4 KiB page in front of it:
    device_place puts every first image 256 bytes into its page.
    So dense, gap4, chan_a and chan_b (the STREAM planes are multiples of 4: both channel offsets are aligned)
    keep the streaming kernel on either side; gap_odd and off1 on y, or on the x of a 1x1 conv, send the call to
    the LDS-staged kernel, and on the x of a 3x3 conv stay with the streaming kernel (4-byte aligned taps).
    conv_stream_eligible adds (K / 4) % depth == 0: tile 18 (depth 8) takes K = 96 and 64 only.
  * conv_wino_eligible (ore_conv_wino.hip) asks of the layout only a 4-byte aligned x and extents below 2 GiB:
    every layout here keeps every Winograd tile.
  * launch_maxpool_t: variant 5 needs evenly spaced planes (nstride == C * plane on both sides), a plane that is
    a multiple of 4 and a 16-byte aligned x, else it runs the direct kernel; variant 4 checks each plane's
    alignment inside the kernel; 2 and 3 load single elements.

No bound here is new: bit-identity with the dense call on tile 0 (include/ore.h: "Results never depend on it"),
2e-6 * (sum |x||w| + |b|) against oracle.conv2d (test_conv2d) and against _convref.conv_f64 (test_wino_conv_vs_f64),
exact equality for MaxPool and the elementwise ops, 2e-7 for Softmax (test_ops_gpu.py)."""
import zlib

import numpy as np
import pytest

import _slices as sl
from _convref import conv_f64
from _knobs import conv_tile, pool_variant
from _slices import DENSE, LAYOUTS, OFF1, ref

import oracle

pytestmark = pytest.mark.gpu

ORE_OK, ORE_ERR_INVALID = 0, 1

# x alone, y alone, both; dense / dense is the control
COMBOS = [(DENSE, DENSE)] + [c for l in LAYOUTS[1:] for c in ((l, DENSE), (DENSE, l), (l, l))]
COMBO_IDS = [f"x_{a}-y_{b}" for a, b in COMBOS]

# N, C, H, W, M, kh, kw, auto_pad, pads, strides: from CONV_CASES / STREAM_CASES (test_ops_gpu.py) and CASES
# (test_wino_gpu.py), each family's ragged edges
_P1 = (1, 1, 1, 1)
LDS_CASES = [
    (2, 5, 16, 16, 40, 3, 3, "SAME_UPPER", None, (1, 1)),
    (2, 3, 11, 9, 33, 2, 3, "NOTSET", (2, 0, 1, 3), (3, 1)),
    (2, 7, 23, 23, 96, 7, 7, "VALID", None, (2, 2)),
    (5, 17, 7, 7, 130, 3, 3, "NOTSET", _P1, (1, 1)),
    (2, 33, 6, 10, 48, 1, 1, "NOTSET", (1, 0, 0, 1), (1, 2)),
]
STREAM_CASES = [
    (3, 96, 12, 12, 16, 1, 1, "NOTSET", (0, 0, 0, 0), (1, 1)),
    (2, 64, 4, 6, 200, 1, 1, "NOTSET", (0, 0, 0, 0), (1, 1)),
    (2, 48, 7, 4, 48, 1, 1, "NOTSET", (0, 0, 0, 0), (1, 1)),
    (2, 16, 12, 12, 64, 3, 3, "NOTSET", _P1, (1, 1)),
    (1, 48, 7, 8, 192, 3, 3, "NOTSET", _P1, (1, 1)),
]
WINO_CASES = [(N, C, H, W, M, 3, 3, "NOTSET", _P1, (1, 1))
              for N, C, H, W, M in ((2, 16, 5, 7, 40), (3, 16, 1, 1, 32), (5, 32, 6, 6, 33), (2, 16, 12, 12, 64))]
CONV_CASES = LDS_CASES + STREAM_CASES + [c for c in WINO_CASES if c not in STREAM_CASES]
DIRECT_TILES = [-1, 0, 1, 2, 3, 12, 18, 46]  # the heuristic, the LDS-staged tiles, one of each streaming group
RELU_BIAS = [(False, True), (True, True), (False, False), (True, False)]


def _case_id(c):
    return "x".join(str(v) for v in c[:7]) + ("s" + "".join(map(str, c[9])) if c[9] != (1, 1) else "")


def _wino_geometry(case):
    N, C, H, W, M, kh, kw, auto_pad, pads, strides = case
    return kh == 3 and kw == 3 and strides == (1, 1) and pads == _P1 and C % 16 == 0


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _conv_attrs(auto_pad, pads, strides, relu):
    from ore import _lib
    a = _lib.ConvAttrs()
    a.auto_pad = _lib.PAD[auto_pad]
    a.n_pads = 4 if pads is not None else 0
    for i in range(a.n_pads):
        a.pads[i] = pads[i]
    a.strides[0], a.strides[1] = strides
    a.dilations[0] = a.dilations[1] = 1
    a.group = 1
    a.fuse_relu = 1 if relu else 0
    return a


def _pool_attrs(kernel, strides, auto_pad, pads):
    from ore import _lib
    a = _lib.PoolAttrs()
    a.auto_pad = _lib.PAD[auto_pad]
    a.n_pads = 4 if pads is not None else 0
    for i in range(a.n_pads):
        a.pads[i] = pads[i]
    a.kernel[0], a.kernel[1] = kernel
    a.strides[0], a.strides[1] = strides
    return a


def _err(ctx):
    import ore
    m = ore.load().ore_last_error(ctx.h)
    return m.decode() if m else ""


class _Slot:
    """One tensor on the device inside its poisoned buffer."""

    def __init__(self, shape, layout, data=None, poison=None):
        self.placed, self.buf = sl.device_place(shape, layout)
        self.desc = sl.descriptor(self.placed, self.buf)
        if data is None:
            sl.poison_output(self.buf)
        else:
            sl.upload(self.buf, self.placed.input_buffer(data, poison))

    def repoison(self):
        sl.poison_output(self.buf)

    def result(self, poison=sl.NAN_POISON):
        """The tensor after the call; the surroundings and the absence of poison checked on the way."""
        bits = sl.download(self.buf)
        sl.check_surroundings(self.placed, bits)
        got = self.placed.inside(bits)
        sl.check_no_poison(got, poison)
        return got


# ------------------------------------------------------------------------------------------------ Conv
_conv_data = {}
_conv_refs = {}


def _conv_case_data(case):
    if case not in _conv_data:
        N, C, H, W, M, kh, kw, auto_pad, pads, strides = case
        rng = np.random.default_rng(zlib.crc32(repr(case).encode()) ^ 0x51ce)
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)
        w = rng.standard_normal((M, C, kh, kw)).astype(np.float32)
        b = rng.standard_normal((M,)).astype(np.float32)
        eff = "NOTSET" if pads is not None and any(p > 0 for p in pads) else auto_pad
        p, Ho, Wo = oracle.resolve_window(eff, pads, H, W, kh, kw, strides[0], strides[1])
        _conv_data[case] = (x, w, b, _t(w), _t(b), [int(v) for v in p], (N, M, Ho, Wo))
    return _conv_data[case]


def _conv_ref(ctx, case, relu, bias, wino):
    """The same call on dense, unpoisoned tensors with conv_tile(0) (Winograd: the algorithm's default tile),
    held to the project's bound against the CPU reference once, then shared and never changed."""
    import ore
    import torch
    key = (case, relu, bias, wino)
    if key not in _conv_refs:
        N, C, H, W, M, kh, kw, auto_pad, pads, strides = case
        x, w, b, wd, bd, ptlbr, yshape = _conv_case_data(case)
        xd, y = _t(x), torch.empty(yshape, dtype=torch.float32, device="cuda")
        a = _conv_attrs(auto_pad, pads, strides, relu)
        descs = [sl.dense_descriptor(t) for t in (xd, wd, bd, y)]
        ctx.set_conv_algo(ore.CONV_ALGO_WINOGRAD if wino else ore.CONV_ALGO_DIRECT)
        try:
            with conv_tile(ctx, -1 if wino else 0):
                st = ore.load().ore_conv2d_f32(ctx.h, ref(descs[0]), ref(descs[1]), ref(descs[2]) if bias else None, ref(a),
                                               ref(descs[3]))
        finally:
            ctx.set_conv_algo(ore.CONV_ALGO_DIRECT)
        assert st == ORE_OK, _err(ctx)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        f64, mag = conv_f64(x, w, b if bias else None, ptlbr, strides)
        f64, mag = f64[:, :, :yshape[2], :yshape[3]], mag[:, :, :yshape[2], :yshape[3]]
        if wino:  # test_wino_conv_vs_f64's bound
            want = np.maximum(f64, 0) if relu else f64
            err = np.abs(got.astype(np.float64) - want) / (mag + 1e-30)
            assert err.max() <= 2e-6, err.max()
        else:     # test_conv2d's bound and reference
            want = oracle.conv2d(x, w, b if bias else None, auto_pad=auto_pad, pads=pads, strides=strides)
            if relu:
                want = oracle.relu(want)
            assert want.shape == got.shape
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            assert np.all(err <= 2e-6 * mag + 1e-30), f"max err {err.max()} vs bound {(2e-6 * mag).max()}"
        got.setflags(write=False)
        _conv_refs[key] = got
    return _conv_refs[key]


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("case", CONV_CASES, ids=_case_id)
def test_conv_slices(gpu_ctx, case, combo):
    """Every conv family on sliced x and y: ORE_OK, y's surroundings keep the poison bits, no output is NaN, and
    the outputs are the bits of the dense call -- direct: on tile 0, whatever tile is forced; Winograd: of the
    dense Winograd call, on every Winograd tile, and not the direct call's bits (a Winograd kernel ran).  Which
    streaming kernel ran is not visible in the results (module docstring)."""
    import ore
    N, C, H, W, M, kh, kw, auto_pad, pads, strides = case
    xl, yl = combo
    x, w, b, wd, bd, ptlbr, yshape = _conv_case_data(case)
    xs = _Slot(x.shape, xl, x, sl.NAN_POISON)
    ys = _Slot(yshape, yl)
    wdesc, bdesc = sl.dense_descriptor(wd), sl.dense_descriptor(bd)
    L = ore.load()
    base = ore.Model.TILE_NAMES.index("wino 32x32 d4")
    algos = [(False, DIRECT_TILES)] + ([(True, [base + t for t in range(5)])] if _wino_geometry(case) else [])
    for wino, tiles in algos:
        try:
            for relu, bias in RELU_BIAS:
                direct = _conv_ref(gpu_ctx, case, relu, bias, False)
                want = _conv_ref(gpu_ctx, case, relu, bias, True) if wino else direct
                gpu_ctx.set_conv_algo(ore.CONV_ALGO_WINOGRAD if wino else ore.CONV_ALGO_DIRECT)
                a = _conv_attrs(auto_pad, pads, strides, relu)
                for tile in tiles:
                    what = f"{'winograd' if wino else 'direct'} tile {tile} relu {relu} bias {bias}"
                    ys.repoison()
                    with conv_tile(gpu_ctx, tile):
                        st = L.ore_conv2d_f32(gpu_ctx.h, ref(xs.desc), ref(wdesc), ref(bdesc) if bias else None, ref(a),
                                              ref(ys.desc))
                    assert st == ORE_OK, (what, _err(gpu_ctx))
                    try:
                        got = ys.result()
                    except AssertionError as e:
                        raise AssertionError(f"{what}: {e}") from None
                    np.testing.assert_array_equal(got, want, err_msg=what)
                    if wino and H * W > 1:
                        assert not np.array_equal(got, direct), what
        finally:
            gpu_ctx.set_conv_algo(ore.CONV_ALGO_DIRECT)


def test_matmul_off1(gpu_ctx):
    """MatMul shares run_conv: (37, 256, 10) with a, b and y at a 4-byte aligned base between poison."""
    import ore
    m, k, n = 37, 256, 10
    rng = np.random.default_rng(m * 7 + n)
    a = rng.standard_normal((m, k)).astype(np.float32)
    b = rng.standard_normal((k, n)).astype(np.float32)
    want = oracle.matmul(a, b)
    bound = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    import torch
    yd = torch.empty((m, n), dtype=torch.float32, device="cuda")
    descs = [sl.dense_descriptor(t) for t in (_t(a), _t(b), yd)]
    with conv_tile(gpu_ctx, 0):
        assert ore.load().ore_matmul_f32(gpu_ctx.h, ref(descs[0]), ref(descs[1]), ref(descs[2])) == ORE_OK, _err(gpu_ctx)
    torch.cuda.synchronize()
    dense = yd.cpu().numpy()
    sa, sb = _Slot(a.shape, OFF1, a, sl.NAN_POISON), _Slot(b.shape, OFF1, b, sl.NAN_POISON)
    sy = _Slot((m, n), OFF1)
    for s in (sa, sb, sy):
        assert s.desc.data % 16 == 4
    for tile in (-1, 0, 1, 2, 3, 12, 46):
        sy.repoison()
        with conv_tile(gpu_ctx, tile):
            st = ore.load().ore_matmul_f32(gpu_ctx.h, ref(sa.desc), ref(sb.desc), ref(sy.desc))
        assert st == ORE_OK, (tile, _err(gpu_ctx))
        got = sy.result()
        np.testing.assert_array_equal(got, dense, err_msg=f"tile {tile}")
        assert np.all(np.abs(got - want) <= 2e-6 * bound + 1e-30)


# ------------------------------------------------------------------------------------------------ MaxPool
POOL_CASES = [
    # N, C, H, W, k, s, auto_pad, pads: from POOL_CASES (test_ops_gpu.py)
    (2, 5, 9, 9, (3, 3), (2, 2), "VALID", None),
    (2, 16, 54, 54, (3, 3), (2, 2), "NOTSET", (0, 0, 1, 1)),
    (3, 4, 10, 7, (3, 2), (2, 1), "SAME_UPPER", None),
    (3, 7, 27, 27, (3, 3), (2, 2), "NOTSET", (0, 0, 0, 0)),
    (2, 5, 35, 30, (3, 3), (2, 3), "NOTSET", (1, 2, 1, 0)),
    (1, 8, 28, 28, (2, 2), (2, 2), "NOTSET", (0, 0, 0, 0)),
]
_pool_data = {}


def _pool_case_data(case):
    if case not in _pool_data:
        N, C, H, W, k, s, auto_pad, pads = case
        x = (np.random.default_rng(3).standard_normal((N, C, H, W)) - 2.0).astype(np.float32)  # mostly negative: zero padding shows
        want = oracle.maxpool2d(x, k, s, auto_pad=auto_pad, pads=pads)
        want.setflags(write=False)
        _pool_data[case] = (x, want)
    return _pool_data[case]


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_maxpool_slices(gpu_ctx, case, combo):
    """Every MaxPool variant on sliced x and y, +inf around x: the oracle's values exactly, no +inf in the
    result, y's surroundings untouched.  (Variant 5 runs the direct kernel when the planes are not evenly
    spaced: the contract is the result.)"""
    import ore
    N, C, H, W, k, s, auto_pad, pads = case
    xl, yl = combo
    x, want = _pool_case_data(case)
    xs = _Slot(x.shape, xl, x, sl.INF_POISON)
    ys = _Slot(want.shape, yl)
    a = _pool_attrs(k, s, auto_pad, pads)
    for variant in (0, 2, 3, 4, 5):
        ys.repoison()
        with pool_variant(gpu_ctx, variant):
            st = ore.load().ore_maxpool2d_f32(gpu_ctx.h, ref(xs.desc), ref(a), ref(ys.desc))
        assert st == ORE_OK, (variant, _err(gpu_ctx))
        try:
            got = ys.result(sl.INF_POISON)
        except AssertionError as e:
            raise AssertionError(f"variant {variant}: {e}") from None
        np.testing.assert_array_equal(got, want, err_msg=f"variant {variant}")


# ------------------------------------------------------------------------------------------------ nstride rules
def _conv_reject_setup():
    N, C, H, W, M = 2, 4, 6, 5, 8
    x = np.zeros((N, C, H, W), np.float32)
    xs = _Slot(x.shape, sl.GAP4, x, sl.NAN_POISON)
    ys = _Slot((N, M, H, W), sl.GAP4)
    w = _t(np.zeros((M, C, 3, 3), np.float32))
    return xs, ys, w, _conv_attrs("NOTSET", _P1, (1, 1), False)


@pytest.mark.parametrize("side,delta", [("x", -1), ("y", -1), ("x", "neg"), ("y", "neg"), ("x", "range"), ("y", "range")])
def test_conv_rejects_overlapping_images(gpu_ctx, side, delta):
    """ore_conv2d_f32: a non-zero nstride below the image size (C*H*W for x, M*Ho*Wo for y) would make images
    overlap: ORE_ERR_INVALID naming the tensor, nothing launched (y keeps its poison).  Negative strides and
    strides past 32-bit indexing likewise."""
    import ore
    xs, ys, w, a = _conv_reject_setup()
    slot = xs if side == "x" else ys
    image = slot.placed.image
    bad = image + delta if delta == -1 else -image if delta == "neg" else (1 << 31) // 2
    d = sl.descriptor(slot.placed, slot.buf, nstride=bad)
    xd, yd = (d, ys.desc) if side == "x" else (xs.desc, d)
    st = ore.load().ore_conv2d_f32(gpu_ctx.h, ref(xd), ref(sl.dense_descriptor(w)), None, ref(a), ref(yd))
    assert st == ORE_ERR_INVALID
    assert f"Conv: {side}" in _err(gpu_ctx), _err(gpu_ctx)
    bits = sl.download(ys.buf)
    assert (bits == sl.OUT_POISON_BITS).all()
    # exactly the image size is accepted (the contiguous tensor, stated explicitly)
    if delta == -1:
        good = sl.descriptor(slot.placed, slot.buf, nstride=image)
        xd, yd = (good, ys.desc) if side == "x" else (xs.desc, good)
        assert ore.load().ore_conv2d_f32(gpu_ctx.h, ref(xd), ref(sl.dense_descriptor(w)), None, ref(a), ref(yd)) == ORE_OK
        gpu_ctx.sync()


@pytest.mark.parametrize("side,delta", [("x", -1), ("y", -1), ("x", "neg"), ("y", "neg"), ("x", "range"), ("y", "range")])
def test_maxpool_rejects_overlapping_images(gpu_ctx, side, delta):
    """ore_maxpool2d_f32: the same rule (C*H*W for x, C*Ho*Wo for y), and the sign and 32-bit range checks Conv
    has (nstride * N + 256 < 2^31)."""
    import ore
    N, C, H, W = 2, 3, 9, 9
    x = np.zeros((N, C, H, W), np.float32)
    xs = _Slot(x.shape, sl.GAP4, x, sl.INF_POISON)
    ys = _Slot((N, C, 4, 4), sl.GAP4)
    a = _pool_attrs((3, 3), (2, 2), "VALID", None)
    slot = xs if side == "x" else ys
    image = slot.placed.image
    bad = image + delta if delta == -1 else -image if delta == "neg" else (1 << 31) // 2
    d = sl.descriptor(slot.placed, slot.buf, nstride=bad)
    xd, yd = (d, ys.desc) if side == "x" else (xs.desc, d)
    st = ore.load().ore_maxpool2d_f32(gpu_ctx.h, ref(xd), ref(a), ref(yd))
    assert st == ORE_ERR_INVALID
    assert f"MaxPool: {side}" in _err(gpu_ctx), _err(gpu_ctx)
    assert (sl.download(ys.buf) == sl.OUT_POISON_BITS).all()
    if delta == -1:
        good = sl.descriptor(slot.placed, slot.buf, nstride=image)
        xd, yd = (good, ys.desc) if side == "x" else (xs.desc, good)
        assert ore.load().ore_maxpool2d_f32(gpu_ctx.h, ref(xd), ref(a), ref(yd)) == ORE_OK
        gpu_ctx.sync()


# ------------------------------------------------------------------------------------------------ contiguous-only ops
def _run_off1(ctx, fn, inputs, out_shape, want, atol=None):
    """fn(ctx.h, *input descriptors, output descriptor) with every operand at an off1 base between poison."""
    ins = [_Slot(a.shape, OFF1, a, sl.NAN_POISON) for a in inputs]
    out = _Slot(out_shape, OFF1)
    for s in ins + [out]:
        assert s.desc.data % 16 == 4 and s.desc.nstride == s.placed.image
    st = fn(ctx.h, *[ref(s.desc) for s in ins], ref(out.desc))
    assert st == ORE_OK, _err(ctx)
    got = out.result()
    if atol is None:
        np.testing.assert_array_equal(got, np.asarray(want).reshape(out_shape))
    else:
        assert np.abs(got - np.asarray(want).reshape(out_shape)).max() <= atol
    return ins, out


def _refuses_non_contiguous(ctx, fn, ins, out):
    """nstride other than the product of the inner dims, on each operand in turn: ORE_ERR_INVALID, nothing
    launched (the output buffer keeps its poison everywhere)."""
    slots = ins + [out]
    for i, s in enumerate(slots):
        out.repoison()
        descs = [t.desc for t in slots]
        descs[i] = sl.descriptor(s.placed, s.buf, nstride=s.placed.image + 1)
        st = fn(ctx.h, *[ref(d) for d in descs])
        assert st == ORE_ERR_INVALID, f"operand {i}: status {st}"
        assert (sl.download(out.buf) == sl.OUT_POISON_BITS).all(), f"operand {i}: something was launched"


@pytest.mark.parametrize("n", [7, 4099])
def test_relu_off1(gpu_ctx, n):
    """launch_relu takes the scalar kernel when x or y is not 16-byte aligned."""
    import ore
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32).reshape(1, 1, 1, n)
    ins, out = _run_off1(gpu_ctx, ore.load().ore_relu_f32, [x], x.shape, oracle.relu(x))
    _refuses_non_contiguous(gpu_ctx, ore.load().ore_relu_f32, ins, out)


def test_add_off1(gpu_ctx):
    import ore
    rng = np.random.default_rng(11)
    a = rng.standard_normal((3, 8, 5, 6)).astype(np.float32)
    b = rng.standard_normal((8, 1, 1)).astype(np.float32)
    ins, out = _run_off1(gpu_ctx, ore.load().ore_add_f32, [a, b], a.shape, oracle.add(a, b))
    _refuses_non_contiguous(gpu_ctx, ore.load().ore_add_f32, ins, out)
    a2 = rng.standard_normal((4, 10)).astype(np.float32)
    b2 = rng.standard_normal((1, 10)).astype(np.float32)
    _run_off1(gpu_ctx, ore.load().ore_add_f32, [a2, b2], a2.shape, oracle.add(a2, b2))


@pytest.mark.parametrize("rows,d", [(3, 7), (3, 257), (5, 1025)])
def test_softmax_off1(gpu_ctx, rows, d):
    """One wave per row, single-element loads: rows in registers (d <= 1024) and the long-row kernel, which stages
    e in y."""
    import ore
    x = (np.random.default_rng(d).standard_normal((rows, d, 1, 1)) * 5).astype(np.float32)
    ins, out = _run_off1(gpu_ctx, ore.load().ore_softmax_f32, [x], (rows, d), oracle.softmax(x), atol=2e-7)
    _refuses_non_contiguous(gpu_ctx, ore.load().ore_softmax_f32, ins, out)


@pytest.mark.parametrize("shape", [(3, 7, 1, 1), (2, 5, 129, 130)])
def test_gap_off1(gpu_ctx, shape):
    """The LDS-staged kernel (1 x 1 planes) and the one-thread-per-row kernel (129 x 130)."""
    import ore
    x = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
    ins, out = _run_off1(gpu_ctx, ore.load().ore_gap_f32, [x], shape[:2] + (1, 1), oracle.gap(x))
    _refuses_non_contiguous(gpu_ctx, ore.load().ore_gap_f32, ins, out)


@pytest.mark.parametrize("axis", [1, 2, 3, 0])
def test_concat_off1(gpu_ctx, axis):
    import ore
    rng = np.random.default_rng(axis)
    sa = [2, 3, 4, 5]
    sb = list(sa)
    sb[axis] = 6
    a = rng.standard_normal(sa).astype(np.float32)
    b = rng.standard_normal(sb).astype(np.float32)
    want = oracle.concat(a, b, axis)

    def fn(h, da, db, dy):
        return ore.load().ore_concat_f32(h, da, db, axis, dy)
    ins, out = _run_off1(gpu_ctx, fn, [a, b], want.shape, want)
    _refuses_non_contiguous(gpu_ctx, fn, ins, out)


def test_dropout_off1(gpu_ctx):
    import ore
    x = np.random.default_rng(1).standard_normal((4, 2, 2, 3)).astype(np.float32)
    ins, out = _run_off1(gpu_ctx, ore.load().ore_dropout_f32, [x], x.shape, x)
    _refuses_non_contiguous(gpu_ctx, ore.load().ore_dropout_f32, ins, out)


def test_matmul_refuses_non_contiguous(gpu_ctx):
    import ore
    rng = np.random.default_rng(2)
    a = rng.standard_normal((5, 16)).astype(np.float32)
    b = rng.standard_normal((16, 3)).astype(np.float32)
    want = oracle.matmul(a, b)
    ins = [_Slot(t.shape, OFF1, t, sl.NAN_POISON) for t in (a, b)]
    out = _Slot((5, 3), OFF1)
    assert ore.load().ore_matmul_f32(gpu_ctx.h, ref(ins[0].desc), ref(ins[1].desc), ref(out.desc)) == ORE_OK, _err(gpu_ctx)
    got = out.result()
    bound = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    assert np.all(np.abs(got - want) <= 2e-6 * bound + 1e-30)
    _refuses_non_contiguous(gpu_ctx, ore.load().ore_matmul_f32, ins, out)
