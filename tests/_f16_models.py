"""Model builders shared by the fp16 tests (no GPU): a Conv (+ Relu) chain ending in GlobalAveragePool
and a fire module with the next squeeze, as ONNX bytes, and the fire-module shapes the fused kernels are
tested at."""
import numpy as np


def _chain_model(x_shape, layers, pool=None):
    """Conv(+Relu) layers [(w, b, pads, strides, relu)], optional MaxPool after the first, then
    GlobalAveragePool (an f16 model's output must be f32)."""
    from ore import onnx_wire as w
    nodes, inits, vinfo = [], [], [w.encode_value_info("x", x_shape)]
    cur = "x"
    for i, (wt, b, pads, strides, relu) in enumerate(layers):
        ins = [cur, f"w{i}"] + ([f"b{i}"] if b is not None else [])
        inits.append(w.encode_tensor(f"w{i}", wt))
        vinfo.append(w.encode_value_info(f"w{i}", wt.shape))
        if b is not None:
            inits.append(w.encode_tensor(f"b{i}", b))
            vinfo.append(w.encode_value_info(f"b{i}", b.shape))
        nodes.append(w.encode_node("Conv", ins, [f"c{i}"], attrs=[w.encode_attr_ints("pads", pads),
                                                                   w.encode_attr_ints("strides", strides)]))
        cur = f"c{i}"
        if relu:
            nodes.append(w.encode_node("Relu", [cur], [f"r{i}"]))
            cur = f"r{i}"
        if i == 0 and pool is not None:
            nodes.append(w.encode_node("MaxPool", [cur], ["p0"], attrs=[
                w.encode_attr_ints("kernel_shape", [3, 3]), w.encode_attr_ints("strides", [2, 2]),
                w.encode_attr_string("auto_pad", "NOTSET"), w.encode_attr_ints("pads", pool)]))
            cur = "p0"
    nodes.append(w.encode_node("GlobalAveragePool", [cur], ["y"]))
    return w.encode_model("t", nodes, inits, vinfo, [w.encode_value_info("y", (1, 1, 1, 1))])


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def _sparse(rng, shape, nonzeros):
    """weights in {-1, 0, 1} with ~`nonzeros` non-zero taps per output channel, so every conv
    output stays a small integer (exact in f16 up to 2048)."""
    fan_in = int(np.prod(shape[1:]))
    keep = rng.random(shape) < min(1.0, nonzeros / fan_in)
    return (rng.choice([-1.0, 1.0], size=shape) * keep).astype(np.float32)


def _fire_model_f16(C, H, W, S1, E1, E3, S2, ints=False, seed=0, pool=None):
    # S2 None: no squeeze after the Concat (GAP reads it)
    """squeeze (C -> S1) -> expand 1x1 (E1) / 3x3 pad 1 (E3) -> Concat [-> 3x3 / stride-2 MaxPool with
    pads `pool`] -> squeeze (S2) -> GAP, all Relu; ints: sparse {-1, 0, 1} weights and small integer
    biases (every value exact in f16).  Returns (model bytes, {name: (w, b)})."""
    from ore import onnx_wire as wr
    rng = np.random.default_rng(seed + C * 7 + H + W + S1 + E1 + E3 + (S2 or 0))
    shapes = {"wq": (S1, C, 1, 1), "w1": (E1, S1, 1, 1), "w3": (E3, S1, 3, 3)}
    if S2 is not None:
        shapes["wn"] = (S2, E1 + E3, 1, 1)
    params, inits, vinfo = {}, [], [wr.encode_value_info("x", (1, C, H, W))]
    for n, shp in shapes.items():
        if ints:
            w, b = _sparse(rng, shp, 8), _ints(rng, -4, 4, (shp[0],))
        else:
            fan = shp[1] * shp[2] * shp[3]
            w = (rng.standard_normal(shp) * np.sqrt(2.0 / fan)).astype(np.float32)
            b = rng.uniform(-0.1, 0.1, shp[0]).astype(np.float32)
        params[n] = (w, b)
        inits += [wr.encode_tensor(n, w), wr.encode_tensor("b" + n, b)]
        vinfo += [wr.encode_value_info(n, w.shape), wr.encode_value_info("b" + n, b.shape)]
    conv = lambda i, w, o, pads: wr.encode_node("Conv", [i, w, "b" + w], [o], attrs=[
        wr.encode_attr_ints("pads", pads), wr.encode_attr_ints("strides", [1, 1])])
    nodes = [conv("x", "wq", "q", [0] * 4), wr.encode_node("Relu", ["q"], ["qr"]),
             conv("qr", "w1", "e1", [0] * 4), wr.encode_node("Relu", ["e1"], ["e1r"]),
             conv("qr", "w3", "e3", [1] * 4), wr.encode_node("Relu", ["e3"], ["e3r"]),
             wr.encode_node("Concat", ["e1r", "e3r"], ["cat"], attrs=[wr.encode_attr_int("axis", 1)])]
    if pool is not None:
        nodes.append(wr.encode_node("MaxPool", ["cat"], ["pc"], attrs=[
            wr.encode_attr_ints("kernel_shape", [3, 3]), wr.encode_attr_ints("strides", [2, 2]),
            wr.encode_attr_string("auto_pad", "NOTSET"), wr.encode_attr_ints("pads", pool)]))
    if S2 is None:  # the Concat read by something other than a squeeze (GAP): fire_f16_kernel's Concat form
        nodes.append(wr.encode_node("GlobalAveragePool", ["cat"], ["y"]))
        return wr.encode_model("fire", nodes, inits, vinfo, [wr.encode_value_info("y", (1, E1 + E3, 1, 1))]), params
    nodes += [conv("pc" if pool is not None else "cat", "wn", "n", [0] * 4), wr.encode_node("Relu", ["n"], ["nr"]),
              wr.encode_node("GlobalAveragePool", ["nr"], ["y"])]
    return wr.encode_model("fire", nodes, inits, vinfo, [wr.encode_value_info("y", (1, S2, 1, 1))]), params


FIRE_F16_CASES = [
    # C, H, W, S1, E1, E3, S2 -> fire_f16_kernel<S1 / 16, ceil(S2 / 32)>
    (16, 12, 12, 16, 64, 64, 16),     # fire2 -> squeeze3 family, one tile per image
    (32, 9, 8, 32, 128, 128, 48),     # fire5 -> squeeze6 (48 of 64 squeeze rows), W = 8
    (24, 8, 7, 48, 192, 192, 64),     # fire7 -> squeeze8, W = 7
    (16, 13, 13, 64, 64, 128, 32),    # C = 64, unequal expands, 13 x 13
    (8, 54, 54, 16, 64, 64, 32),      # SqueezeNet fire3 plane: 12 tiles per image, tile edges mid-row
    (16, 27, 27, 48, 192, 192, 48),   # fire6 plane: 3 tiles, the last partial
]

FIRE_POOL_F16_CASES = [
    # C, H, W, S1, E1, E3, S2, pool pads
    (16, 54, 54, 32, 128, 128, 32, [0, 0, 1, 1]),   # SqueezeNet fire4 -> pool3 -> fire5
    (32, 27, 27, 64, 256, 256, 64, [0, 0, 1, 1]),   # fire8 -> pool5 -> fire9
    (8, 13, 15, 16, 64, 96, 48, [1, 1, 1, 1]),      # padded on all sides, unequal expands, 48 squeeze rows
    (8, 9, 8, 48, 32, 64, 16, [0, 0, 0, 0]),        # floor-mode pool, C = 48
    (8, 38, 33, 32, 64, 64, 24, [0, 0, 1, 1]),      # 4 bands of 5 pooled rows, the last 4
]
