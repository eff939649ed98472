"""Shared by tests/test_cam.py (CPU) and tests/test_cam_gpu.py: the graphs, seeded inputs and host references of
the class activation map tests (ore_class_maps_f32, ore_model_set_cam).

A graph is  x [3, H, W] -> 3x3 Conv (pad 1) -> Relu -> 1x1 map conv (C -> M) -> [Relu] -> GlobalAveragePool ->
[Dropout] -> Softmax (or -> Reshape, the output), weights He-scaled normal, inputs standard normal (the "real" mode of _topologies.Builder).
head() walks any model's bytes back from its output as the library does and names what the tests read: the map
conv's input, its weights and bias, whether a Relu follows, and the pool's input T."""
import functools

import numpy as np

from _convref import conv_f64, f16_layer_check
from _topologies import Builder

BATCH = 3
TOPK = 5
SQ_SEED = 21  # of squeezenet.synthetic_input in the SqueezeNet model-level tests

# name -> (C, M, H, W, relu behind the map conv, a Reshape behind the pool in place of the Softmax, seed)
#   c32: C % 32 == 0 at 143 <= 256 pixels: the f32 conv + GAP fusion takes the map conv, T is never stored
#   c48: C % 32 != 0: it does not (nor does the f16 one, C % 64 != 0); no Relu, so the maps hold negative values
#   c64r: C % 64 == 0: the f16 conv + GAP fusion applies too; the pool's rows leave through a Reshape (no Softmax:
#         the loader takes a Softmax of 4-D values only, so no graph with a Reshape in front of one loads)
#   c20: C % 8 != 0: the f16 kernels read the pixels element by element; C % 32 != 0: a padded last k-step; a Dropout in front of the Softmax
GRAPHS = {
    "c32": (32, 40, 13, 11, True, False, 11),
    "c48": (48, 23, 9, 8, False, False, 12),
    "c64r": (64, 40, 13, 13, True, True, 13),
    "c20": (20, 17, 7, 5, True, False, 14),
}


@functools.lru_cache(maxsize=None)
def graph_bytes(name):
    from ore import onnx_wire as wr
    C, M, H, W, relu, reshape, seed = GRAPHS[name]
    b = Builder(3, H, W, "real", seed, 0)
    v = b.conv("x", C, k=3, pads=1, name="c1")
    v = b.conv(v, M, k=1, relu=relu, name="map")
    v = b.gap(v, "gap")
    if reshape:
        b.inits.append(wr.encode_tensor("shape", np.array([1, M], np.int64)))
        b.vinfo.append(wr.encode_value_info("shape", (2,)))
        v = b._node("Reshape", [v, "shape"], "flat", (M,))  # the graph's output: the engine's Softmax takes 4-D values only
    else:
        if name == "c20":
            v = b.dropout(v, "drop")
        v = b._node("Softmax", [v], "prob", (M,))
    return b.finish(v)


@functools.lru_cache(maxsize=None)
def graph_input(name, n=BATCH):
    C, M, H, W, relu, reshape, seed = GRAPHS[name]
    x = np.random.default_rng(1000 + seed).standard_normal((n, 3, H, W)).astype(np.float32)
    x.setflags(write=False)
    return x


def head(model_bytes):
    """{"x": the map conv's input, "T": the pool's input, "w": [M, C], "b": [M] or None, "relu": bool} of a model
    with a map conv; None where the walk back from the output does not find one."""
    from ore import onnx_wire as wr
    g = wr.decode_model(model_bytes).graph
    inits = {t.name: t.to_numpy() for t in g.initializer}
    prod = {n.output[0]: n for n in g.node}
    v = g.output[0].name
    softmax = False
    while v in prod and (prod[v].op_type in ("Dropout", "Reshape") or (prod[v].op_type == "Softmax" and not softmax)):
        softmax = softmax or prod[v].op_type == "Softmax"
        v = prod[v].input[0]
    if v not in prod or prod[v].op_type != "GlobalAveragePool":
        return None
    T = prod[v].input[0]
    v, relu = T, False
    if v in prod and prod[v].op_type == "Relu":
        v, relu = prod[v].input[0], True
    if v not in prod or prod[v].op_type != "Conv":
        return None
    n = prod[v]
    w = inits[n.input[1]]
    if w.shape[2:] != (1, 1):
        return None
    return {"x": n.input[0], "T": T, "w": w.reshape(w.shape[0], -1), "b": inits[n.input[2]] if len(n.input) > 2 else None,
            "relu": relu}


def gather(T, classes, views=1):
    """maps[i, j] = T[i, classes[i // views, j]]"""
    T, classes = np.asarray(T), np.asarray(classes)
    return np.stack([T[i, classes[i // views]] for i in range(T.shape[0])])


def maps_f64(x, w, b, classes, relu, views=1):
    """(float64 maps, sum |w x| + |b|) of the gathered 1x1 conv, [n, k, H, W] each."""
    ys, mags = [], []
    for i in range(x.shape[0]):
        c = np.asarray(classes)[i // views]
        y, mag = conv_f64(x[i:i + 1], w[c][:, :, None, None], None if b is None else b[c], (0, 0, 0, 0), (1, 1))
        ys.append(np.maximum(y[0], 0.0) if relu else y[0])
        mags.append(mag[0])
    return np.stack(ys), np.stack(mags)


def f16_maps_check(maps, x, w, b, classes, relu, views=1):
    """f16_layer_check of the maps, image by image (each has its own weight rows): (bad share, ambiguous share)
    over all outputs."""
    bad = amb = 0.0
    n = x.shape[0]
    for i in range(n):
        c = np.asarray(classes)[i // views]
        res = f16_layer_check(maps[i:i + 1], x[i:i + 1], w[c][:, :, None, None], None if b is None else b[c], (0, 0, 0, 0),
                              (1, 1), relu)
        bad += res["bad"] / n
        amb += res["ambiguous"] / n
    return bad, amb


def f16_exact_head(name):
    """The f16 contract of graph `name` walked on the CPU (as _sizes.f16_exact_forward does for SqueezeNet): the
    first layer's nearest-f16 outputs, then the map conv over ALL M classes of them -> its ambiguous share."""
    from ore import onnx_wire as wr
    C, M, H, W, relu, reshape, seed = GRAPHS[name]
    inits = {t.name: t.to_numpy() for t in wr.decode_model(graph_bytes(name)).graph.initializer}
    x = graph_input(name)
    w1, b1 = inits["w_c1"], inits["b_c1"]
    ref = f16_layer_check(np.zeros((x.shape[0], C, H, W), np.float32), x, w1, b1, (1, 1, 1, 1), (1, 1), True)["ref"]
    x1 = ref.astype(np.float32)
    w2, b2 = inits["w_map"], inits["b_map"]
    got = f16_layer_check(np.zeros((x.shape[0], M, H, W), np.float32), x1, w2, b2, (0, 0, 0, 0), (1, 1), relu)["ref"]
    return f16_layer_check(got.astype(np.float32), x1, w2, b2, (0, 0, 0, 0), (1, 1), relu)["ambiguous"]


# ---- the per-op cases: (C, M, H, W) x k x (n, views)
# (13, 9, 5, 3) is there for C % 4 != 0: the tail k-step of the f32 kernel multiplies zeros on both sides
SHAPES = [(32, 40, 13, 11), (20, 17, 1, 1), (48, 40, 4, 4), (512, 1000, 13, 13), (64, 33, 17, 17), (13, 9, 5, 3)]
KS = (1, 5, 17, 33)
NV = [(1, 1), (3, 1), (3, 3)]  # n in {1, 3} x views in {1, 3}, n a multiple of views


def op_cases():
    cases = []
    for shp in SHAPES:
        kmax = min(shp[1], 64)
        for k in sorted({k for k in KS if k <= kmax} | {kmax}):
            for n, views in NV:
                cases.append(shp + (k, n, views))
    return cases


def op_id(case):
    C, M, H, W, k, n, views = case
    return f"C{C}-M{M}-{H}x{W}-k{k}-n{n}-v{views}"


def op_inputs(case):
    """(x [n, C, H, W], w [M, C], b [M], classes [n / views, k]) of a per-op case: ids with a duplicate, 0 and M - 1."""
    C, M, H, W, k, n, views = case
    rng = np.random.default_rng(sum(v * p for v, p in zip(case, (3, 5, 7, 11, 13, 17, 19))))  # a seed per case
    x = rng.standard_normal((n, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((M, C)) * np.sqrt(2.0 / C)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, M).astype(np.float32)
    classes = rng.integers(0, M, (n // views, k)).astype(np.int32)
    classes[0, 0] = 0
    classes[-1, -1] = M - 1
    if k >= 4:
        classes[0, 2] = classes[0, 1]
    return x, w, b, classes
