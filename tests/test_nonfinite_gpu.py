"""Non-finite activations through every plan: ore.h promises that a model's result does not depend on the
fusion flags, and an f16 model produces +-inf by overflow and NaN from inf x 0 or inf - inf by itself.  So
with NaN and +-inf in the input every plan must still return one result, the oracle's (the reference's
semantics: Relu is f32::max, so Relu(NaN) = +0; MaxPool folds f32::max from f32::MIN over a zero-padded
window, so it ignores NaN; Conv, GlobalAveragePool and Softmax propagate NaN, and inf x 0 is NaN under a zero
weight as under any other).  Winograd is exempt (its input transform mixes neighbouring pixels): f32 models
load with winograd=False.

Catalogue subset in ints mode: every finite intermediate is still a small integer, so the oracle's f32 result is
exact for the f32 and the f16 model alike.  NaN positions are compared exactly, every other element bit for
bit; NaN payloads are not compared."""
import functools

import numpy as np
import pytest

from ore import FUSE_ALL, KEEP_VALUES

import oracle
from _knobs import C1_POOL_F16, EPOOL_PATCH, EPOOL_WINDOW, force_tiles, pool_variant
from _topologies import BATCH, BY_NAME, CATALOGUE
from test_topologies_gpu import E, PLANS

gpu = pytest.mark.gpu
FIRST_CONV_TILES = (EPOOL_PATCH, C1_POOL_F16, EPOOL_WINDOW, 51, 52)  # patches; one-launch f16; f32 window; the band walkers f32 / f16

PREFIXES = ("base-", "f2-", "f6-", "f8-", "f9-", "f10-")  # base- covers base-pool-
ENTRIES = [e.name for e in CATALOGUE if e.name.startswith(PREFIXES)] + [f"f12-seed{i}" for i in range(4)]
SPECIALS = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)  # +inf, -inf, NaN, -NaN


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    import torch
    try:
        torch.cuda.synchronize()
        return t.cpu().numpy()
    except RuntimeError as err:  # a device error: nothing more runs on a GPU that has faulted
        pytest.exit(f"device error, stopping: {err}", returncode=3)


def poke(x, seed):
    """a copy of x with four elements per image replaced by +inf, -inf, a NaN with the sign bit clear and one
    with it set, at positions drawn by seed"""
    rng = np.random.default_rng(seed)
    y = np.array(x, dtype=np.float32, copy=True)
    per = y[0].size
    for img in range(y.shape[0]):
        y[img].reshape(-1)[rng.choice(per, size=4, replace=False)] = SPECIALS
    return y


def mismatches(got, want):
    """elements where got is not want: NaN exactly where want is NaN, every other element the same bits"""
    if got.shape != want.shape:
        return max(got.size, want.size)
    gn, wn = np.isnan(got), np.isnan(want)
    bits = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    return int(((gn != wn) | (bits & ~wn)).sum())


# Entries in which a NaN or inf anywhere in an image reaches every output element of that image, whatever the
# seed: a 1x1 conv without Relu straight into GlobalAveragePool spreads a pixel's NaN over all its channels
# (NaN x 0 under the zero weights), and the average over the plane keeps it.  With specials in every image no
# seed can leave an output element finite, so these run on seed 0 and the CPU test below holds them to exactly
# that: all-NaN for every seed tried.
ALL_NAN = ("f9-first-q-norelu",)
SEEDS = 64


def starved_pool(mb, x):
    """True when some MaxPool window of the oracle's run of x holds nothing but NaN.  Its result is then the fold's
    start value f32::MIN, a finite intermediate that is no small integer: an f16 model stores it as -inf (ore.h:
    outputs past 65504 are +-inf), and the oracle's f32 result is no longer what an exact f16 run returns."""
    from ore import onnx_wire
    model = onnx_wire.decode_model(mb)
    inits = {t.name: t.to_numpy() for t in model.graph.initializer}
    v = {"x": x}  # every catalogue graph's one input
    for node in model.graph.node:
        a, i0 = node.attrs(), v[node.input[0]]
        if node.op_type == "Conv":
            bias = inits[node.input[2]] if len(node.input) > 2 else None
            y = oracle.conv2d(i0, inits[node.input[1]], bias, pads=a["pads"].ints, strides=a["strides"].ints)
        elif node.op_type == "Relu":
            y = oracle.relu(i0)
        elif node.op_type == "MaxPool":
            y = oracle.maxpool2d(i0, a["kernel_shape"].ints, a["strides"].ints, auto_pad=a["auto_pad"].s.decode(), pads=a["pads"].ints)
            if (y == -np.finfo(np.float32).max).any():
                return True
        elif node.op_type == "Concat":
            y = oracle.concat(i0, v[node.input[1]], 1)
        elif node.op_type == "Dropout":
            y = i0
        elif node.op_type == "GlobalAveragePool":
            y = oracle.gap(i0)
        else:
            raise AssertionError(node.op_type)
        v[node.output[0]] = y
    return False


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, expected, seed) of an entry.  The seed is the first whose oracle output is at least a quarter finite
    and holds something non-finite too, with no MaxPool window of NaN alone (starved_pool); without one, the first that is at least a quarter finite; for ALL_NAN
    entries, and where 64 seeds give neither (the CPU test fails then), seed 0"""
    entry = BY_NAME[name]
    mb, b = entry.model("ints")
    elems = int(np.prod(b.shape[b.out]))
    ref = oracle.Model(mb)
    try:
        runs = []
        for seed in range(SEEDS):
            x = poke(entry.inputs("ints"), 1000 * seed + len(name))
            want = ref.run(x, elems)
            if np.isfinite(want).mean() >= 0.25 and starved_pool(mb, x):
                continue  # a condition on the seed, like the quarter: see starved_pool
            runs.append((x, want, seed))
            if np.isfinite(want).mean() >= 0.25 and not np.isfinite(want).all():
                return x, want, seed
    finally:
        ref.close()
    if name in ALL_NAN:
        assert all(np.isnan(w).all() for _, w, _ in runs), f"{name} is listed in ALL_NAN but some seed leaves a number"
        return runs[0]
    return next((r for r in runs if np.isfinite(r[1]).mean() >= 0.25), runs[0])


@pytest.mark.parametrize("name", ENTRIES)
def test_oracle_outputs_not_all_nan(name):
    """CPU, the oracle alone: at least a quarter of every case's expected output is finite (ALL_NAN: see there)"""
    x, want, seed = case(name)
    assert (~np.isfinite(x)).sum() == 4 * BATCH
    print(f"{name}: seed {seed}, {int(np.isfinite(want).sum())} of {want.size} finite, {int(np.isnan(want).sum())} NaN")
    if name in ALL_NAN:
        assert np.isnan(want).all()
    else:
        assert np.isfinite(want).mean() >= 0.25, f"{name}: no seed below {SEEDS} leaves a quarter of the oracle's output finite"


@gpu
@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("name", ENTRIES)
def test_topology_nonfinite(gpu_ctx, name, prec):
    """every plan of PLANS equals the oracle on an input with +-inf and NaN"""
    import ore
    entry = BY_NAME[name]
    mb, _ = entry.model("ints")
    x, want, _ = case(name)
    try:
        m = ore.Model(gpu_ctx, mb, max_batch=BATCH, precision=prec, winograd=False)
    except ore.OreError as err:
        assert err.status == 2 and prec == "f16" and entry.f16_refused is not None, err
        return
    problems = []
    try:
        xt = _t(x)
        for plan in PLANS:
            m.set_fusion(plan)
            y = _np(m.run(xt))
            bad = mismatches(y, want)
            print(f"{name} {prec} plan {plan}: {bad} of {want.size} differ")
            if bad:
                gn, wn = np.isnan(y), np.isnan(want)
                problems.append(f"plan {plan}: {bad} of {want.size} differ from the oracle ({int((gn & ~wn).sum())} NaN where it has "
                                f"none, {int((wn & ~gn).sum())} numbers where it has NaN)")
        # the fully fused plan again on every first-conv kernel the step takes (the plans above run the planner's pick)
        for tile in FIRST_CONV_TILES:
            m.set_fusion(E)
            if force_tiles(m, tile):
                try:
                    y = _np(m.run(xt))
                except ore.OreError as err:  # the forced kernel declines this geometry
                    assert err.status != 3, err
                    continue
                bad = mismatches(y, want)
                print(f"{name} {prec} tile {tile} ({ore.Model.TILE_NAMES[tile]}): {bad} of {want.size} differ")
                if bad:
                    problems.append(f"forced tile {tile} ({ore.Model.TILE_NAMES[tile]}): {bad} of {want.size} differ from the oracle")
    finally:
        m.close()
    assert not problems, f"{name} {prec}:\n  " + "\n  ".join(problems)


# ------------------------------------------------------------------------------------ per op
def _special_tensor(shape, seed, share=0.05):
    """standard-normal data shifted down (so that zero padding shows) with `share` of the elements each of +inf,
    -inf, NaN and NaN with the sign set"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) - 1.0).astype(np.float32)
    flat = x.reshape(-1)
    k = max(1, int(share * flat.size))
    idx = rng.choice(flat.size, size=4 * k, replace=False)
    for j, v in enumerate(SPECIALS):
        flat[idx[j * k:(j + 1) * k]] = v
    return x


@gpu
@pytest.mark.parametrize("n", [7, 4099])
def test_relu_nonfinite(gpu_ctx, n):
    import ore
    x = _special_tensor((1, 1, 1, n), n)
    got, want = _np(ore.relu(gpu_ctx, _t(x))), oracle.relu(x)
    assert not np.isnan(want).any()  # Relu(NaN) = +0
    assert mismatches(got, want) == 0


POOLS = [
    # N, C, H, W, k, s, auto_pad, pads: rows of test_ops_gpu.py's POOL_CASES that reach every kernel
    (2, 5, 9, 9, (3, 3), (2, 2), "VALID", None),
    (2, 16, 54, 54, (3, 3), (2, 2), "NOTSET", [0, 0, 1, 1]),
    (3, 4, 10, 7, (4, 4), (3, 2), "SAME_LOWER", None),
    (3, 7, 27, 27, (3, 3), (2, 2), "NOTSET", [0, 0, 0, 0]),
    (2, 5, 35, 30, (3, 3), (2, 3), "NOTSET", [1, 2, 1, 0]),
]


@gpu
@pytest.mark.parametrize("variant", [0, 2, 3, 4, 5])
@pytest.mark.parametrize("pool", POOLS)
def test_maxpool_nonfinite(gpu_ctx, pool, variant):
    import ore
    N, C, H, W, k, s, auto_pad, pads = pool
    x = _special_tensor((N, C, H, W), H * W + C, share=0.1)
    want = oracle.maxpool2d(x, k, s, auto_pad=auto_pad, pads=pads)
    assert not np.isnan(want).any()  # the fold drops NaN
    with pool_variant(gpu_ctx, variant):
        got = _np(ore.max_pool(gpu_ctx, _t(x), k, s, auto_pad=auto_pad, pads=pads))
    assert mismatches(got, want) == 0


@gpu
def test_softmax_nonfinite(gpu_ctx):
    """a row with a NaN, or with +inf (inf - inf), is all NaN, as the oracle's; -inf alone is a zero; rows
    without specials keep the op's bar (2e-7, test_ops_gpu.py)"""
    import ore
    rng = np.random.default_rng(9)
    x = rng.standard_normal((6, 37)).astype(np.float32)
    x[1, 5] = np.nan
    x[2, 7] = np.inf
    x[3, 9] = -np.inf
    x[4, 0], x[4, 36] = -np.inf, SPECIALS[3]
    got, want = _np(ore.softmax(gpu_ctx, _t(x))), oracle.softmax(x)
    assert np.isnan(want[[1, 2, 4]]).all() and np.isfinite(want[[0, 3, 5]]).all() and want[3, 9] == 0
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.abs(got[[0, 3, 5]] - want[[0, 3, 5]]).max() <= 2e-7 and got[3, 9] == 0


@gpu
@pytest.mark.parametrize("shape", [(2, 9, 4, 4), (3, 7, 13, 13)])
def test_gap_nonfinite(gpu_ctx, shape):
    import ore
    x = np.random.default_rng(shape[1]).standard_normal(shape).astype(np.float32)
    last = shape[2] * shape[3] - 1
    for (n, c), vals in {(0, 1): SPECIALS[2:3], (1, 2): SPECIALS[:1], (1, 3): SPECIALS[1:2], (0, 4): SPECIALS[:2],
                         (1, 5): SPECIALS[3:]}.items():  # NaN; +inf; -inf; +inf and -inf (NaN); -NaN: at both ends of a plane
        x[n, c].reshape(-1)[[0, last][:len(vals)]] = vals
    want = oracle.gap(x)
    assert np.isnan(want[0, 1]) and np.isposinf(want[1, 2]) and np.isneginf(want[1, 3]) and np.isnan(want[0, 4]) and np.isnan(want[1, 5])
    assert np.isnan(want).any() and np.isfinite(want).any()
    assert mismatches(_np(ore.global_average_pool(gpu_ctx, _t(x))), want) == 0


def _one_node_f16(op, C, H, W, attrs=()):
    """x -> 1x1 Conv (identity weights, no bias) -> op -> GlobalAveragePool: the op as a launch of its own in
    an f16 model, on the conv's output c0"""
    from ore import onnx_wire as wr
    w = np.eye(C, dtype=np.float32).reshape(C, C, 1, 1)
    nodes = [wr.encode_node("Conv", ["x", "w"], ["c0"], attrs=[wr.encode_attr_ints("pads", [0] * 4),
                                                                wr.encode_attr_ints("strides", [1, 1])]),
             wr.encode_node(op, ["c0"], ["v"], attrs=list(attrs)),
             wr.encode_node("GlobalAveragePool", ["v"], ["y"])]
    vinfo = [wr.encode_value_info("x", (1, C, H, W)), wr.encode_value_info("w", w.shape)]
    return wr.encode_model("one", nodes, [wr.encode_tensor("w", w)], vinfo, [wr.encode_value_info("y", (1, C, 1, 1))])


@gpu
@pytest.mark.parametrize("C", [20, 24])  # the per-channel and the 16-B forms of the f16 kernels
@pytest.mark.parametrize("op", ["Relu", "MaxPool"])
def test_f16_standalone_nonfinite(gpu_ctx, op, C):
    """the separate f16 Relu / MaxPool kernels (plan 0: nothing fused) on a conv output with NaN and +-inf equal
    the oracle's op of that output"""
    import ore
    from ore import onnx_wire as wr
    H, W = 13, 10
    attrs = () if op == "Relu" else (wr.encode_attr_ints("kernel_shape", [3, 3]), wr.encode_attr_ints("strides", [2, 2]),
                                     wr.encode_attr_string("auto_pad", "NOTSET"), wr.encode_attr_ints("pads", [0, 0, 1, 1]))
    rng = np.random.default_rng(C)
    x = (rng.integers(-6, 3, (2, C, H, W))).astype(np.float32)
    for img in range(2):  # an inf at a pixel makes its other channels NaN (inf x 0) behind the identity conv
        px = rng.choice(H * W, size=8, replace=False)
        for j, p in enumerate(px):
            x[img, rng.integers(C), p // W, p % W] = SPECIALS[j % 4]
    m = ore.Model(gpu_ctx, _one_node_f16(op, C, H, W, attrs), max_batch=2, precision="f16")
    try:
        m.set_fusion(KEEP_VALUES)
        _np(m.run(_t(x)))
        assert [s["op"] for s in m.steps()].count(op) == 1
        c0, v = m.read_value("c0"), m.read_value("v")
    finally:
        m.close()
    assert np.isnan(c0).any() and np.isposinf(c0).any() and np.isneginf(c0).any() and np.isfinite(c0).mean() > 0.5
    want = oracle.relu(c0) if op == "Relu" else oracle.maxpool2d(c0, (3, 3), (2, 2), auto_pad="NOTSET", pads=[0, 0, 1, 1])
    assert not np.isnan(want).any()
    assert mismatches(v, want) == 0, mismatches(v, want)


@gpu
def test_f16_fused_relu_negative_zero(gpu_ctx):
    """Negative conv outputs too small for f16 round to -0, and the fused f16 epilogues do their Relu after that
    rounding: it has to give +0.  A -0 would show at once, because the pooled epilogue behind it takes its maxima
    on the bit patterns, where 0x8000 beats every positive number.  One-launch first conv + Relu + pool + squeeze
    against the unfused plan, value by value and bit for bit."""
    import ore
    from _f16_models import _chain_model
    rng = np.random.default_rng(4)
    # f16-exact operands around 2^-14: the conv's outputs are around 2^-24, that is -0, +0 and the first subnormals
    x = (rng.standard_normal((2, 3, 37, 35)) * 2.0 ** -14).astype(np.float16).astype(np.float32)
    w1 = (rng.standard_normal((64, 3, 7, 7)) * 2.0 ** -14).astype(np.float16).astype(np.float32)
    w2 = rng.standard_normal((16, 64, 1, 1)).astype(np.float32)
    mb = _chain_model((1, 3, 37, 35), [(w1, None, [0] * 4, [2, 2], True), (w2, None, [0] * 4, [1, 1], True)], pool=[0, 0, 1, 1])
    got = {}
    for plan in (KEEP_VALUES, FUSE_ALL | ore.FUSE_EAGER | KEEP_VALUES, (FUSE_ALL & ~ore.FUSE_FIRST_SQUEEZE) | ore.FUSE_EAGER | KEEP_VALUES):
        m = ore.Model(gpu_ctx, mb, max_batch=2, precision="f16")
        try:
            m.set_fusion(plan)
            y = _np(m.run(_t(x)))
            vals = {"y": y}
            for vn in ("c0", "p0", "r1"):
                try:
                    vals[vn] = m.read_value(vn)
                except ore.OreError as err:  # elided by the plan
                    assert err.status != 3, err
            got[plan] = vals
            names = [ore.Model.TILE_NAMES[t] for t in m.tiles() if t >= 0]
            print(plan, names)
        finally:
            m.close()
    base = got[KEEP_VALUES]
    c0 = oracle.conv2d(x, w1, None, pads=[0] * 4, strides=[2, 2]).astype(np.float16)
    assert (np.signbit(c0) & (c0 == 0)).mean() > 0.1 and (c0 > 0).mean() > 0.1, "the conv has to produce -0 and positive outputs"
    assert (base["p0"] > 0).mean() > 0.5, (base["p0"] > 0).mean()
    for plan, vals in got.items():
        for vn, v in vals.items():
            if vn != "c0":
                assert mismatches(v, base[vn]) == 0, (plan, vn, mismatches(v, base[vn]))
