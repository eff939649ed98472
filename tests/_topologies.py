"""A catalogue of small graphs around the planner's patterns (no GPU): for every fusion pass of
csrc/ore_plan.cpp the graph it matches and the near-misses of each of its guards (operand order and
kinds, a missing Relu or bias, a second reader, a graph output, channel counts off the multiples, pool
geometry, other strided writers into a Concat, aliases), plus seeded compositions of them.

Every graph has one 4-D input "x" and one output, batch 3.  Base module: squeeze S1 -> expand1x1 E1 /
expand3x3 E3 (pad 1) -> Concat -> [3x3 / stride-2 MaxPool] -> squeeze S2 -> GlobalAveragePool, all with
Relu and bias.  A second reader of a value is a GlobalAveragePool joined into the output by a final
Concat.  Planes are the smallest that reach the kernels' edges: 12 x 12 (16-B planes), 9 x 8 and 8 x 7
(rows wrap inside a pixel group), 13 x 13 (169 -> 172 padded), 7 x 7 (cannot be padded: the f32 fire
passes decline), 21 x 20 and 20 x 21 in front of a pool (ceil pads, a short last band).

Weights come in two modes.  "ints", the anchor: _sparse weights in {-1, 0, 1} with ~`taps` non-zero
taps per output channel, integer biases in [-3, 1], integer inputs in [-4, 4], so every intermediate is a
small integer (tests/test_topologies.py holds each entry to |v| <= 2048): exact in f16 and through the
Winograd transforms in f32, whatever the summation order.  "real": He-scaled normal weights, uniform
+-0.1 biases, standard-normal inputs.

An entry names the passes that MUST fire under FUSE_ALL | FUSE_EAGER per precision (`must`, possibly
none; a near-miss declares none and only its values are checked) and, where the f16 loader refuses the
graph, the loader's message (`f16_refused`)."""
import functools

import numpy as np

from _f16_models import _ints, _sparse

BATCH = 3
INT_LIMIT = 2048  # integers up to here are exact in f16

# the eleven pattern-matching passes of ore_plan.cpp
PASSES = ("conv_pool", "fire_pool_f32", "concat_pool", "fire_f32", "fire_f16", "fire_f16_concat", "first_squeeze",
          "pool_squeeze", "pool_expand", "conv_gap", "concat_in_place")

F16_OUTPUT = "f16 model: graph output '%s' must be f32 (end with GlobalAveragePool / Softmax)"


class Builder:
    """ONNX bytes over ore.onnx_wire, node by node.  Values carry their (C, H, W); a node has no name, so a
    plan step is called after its node's first output (a conv's pre-Relu value)."""

    def __init__(self, C, H, W, mode, seed, taps):
        assert mode in ("ints", "real")
        self.mode, self.taps = mode, taps
        self.rng = np.random.default_rng(seed)
        self.shape = {"x": (C, H, W)}
        self.kind = {"x": "input"}   # value -> the op that made it
        self.ins = {"x": []}         # value -> the activations that op read
        self.nodes, self.inits, self.vinfo = [], [], []
        self.extras = []             # GlobalAveragePool outputs to join into the output
        self.nconv = 0

    def _node(self, op, ins, out, shape, attrs=()):
        from ore import onnx_wire as wr
        assert out not in self.shape, out
        self.nodes.append(wr.encode_node(op, ins, [out], attrs=list(attrs)))
        self.shape[out] = tuple(int(d) for d in shape)
        self.kind[out] = op
        self.ins[out] = [i for i in ins if i in self.shape]
        return out

    def conv(self, x, M, k=1, pads=0, stride=1, relu=True, bias=True, name=None):
        from ore import onnx_wire as wr
        C, H, W = self.shape[x]
        name = name or f"c{self.nconv}"
        self.nconv += 1
        pads = [pads] * 4 if isinstance(pads, int) else list(pads)
        shp = (M, C, k, k)
        if self.mode == "ints":
            w, b = _sparse(self.rng, shp, self.taps), _ints(self.rng, -3, 1, (M,))
        else:
            w = (self.rng.standard_normal(shp) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
            b = self.rng.uniform(-0.1, 0.1, M).astype(np.float32)
        ins = [x, "w_" + name]
        self.inits.append(wr.encode_tensor("w_" + name, w))
        self.vinfo.append(wr.encode_value_info("w_" + name, w.shape))
        if bias:
            ins.append("b_" + name)
            self.inits.append(wr.encode_tensor("b_" + name, b))
            self.vinfo.append(wr.encode_value_info("b_" + name, b.shape))
        Ho = (H + pads[0] + pads[2] - k) // stride + 1
        Wo = (W + pads[1] + pads[3] - k) // stride + 1
        out = self._node("Conv", ins, name, (M, Ho, Wo), [wr.encode_attr_ints("pads", pads),
                                                           wr.encode_attr_ints("strides", [stride, stride])])
        return self._node("Relu", [out], name + "r", self.shape[out]) if relu else out

    def pool(self, x, k=3, stride=2, pads=(0, 0, 1, 1), name="p"):
        from ore import onnx_wire as wr
        C, H, W = self.shape[x]
        pads = list(pads)
        Ho = (H + pads[0] + pads[2] - k) // stride + 1
        Wo = (W + pads[1] + pads[3] - k) // stride + 1
        return self._node("MaxPool", [x], name, (C, Ho, Wo), [
            wr.encode_attr_ints("kernel_shape", [k, k]), wr.encode_attr_ints("strides", [stride, stride]),
            wr.encode_attr_string("auto_pad", "NOTSET"), wr.encode_attr_ints("pads", pads)])

    def concat(self, a, b, name):
        from ore import onnx_wire as wr
        (Ca, H, W), (Cb, Hb, Wb) = self.shape[a], self.shape[b]
        assert (H, W) == (Hb, Wb), (a, b, self.shape[a], self.shape[b])
        return self._node("Concat", [a, b], name, (Ca + Cb, H, W), [wr.encode_attr_int("axis", 1)])

    def gap(self, x, name):
        return self._node("GlobalAveragePool", [x], name, (self.shape[x][0], 1, 1))

    def dropout(self, x, name):
        return self._node("Dropout", [x], name, self.shape[x])

    def also_read(self, x):
        """a second reader of x: its GlobalAveragePool, joined into the output by finish()"""
        self.extras.append(self.gap(x, "g_" + x))

    def finish(self, out):
        from ore import onnx_wire as wr
        for i, g in enumerate(self.extras):
            out = self.concat(out, g, f"y{i}")
        self.out = out
        vinfo = [wr.encode_value_info("x", (1,) + self.shape["x"])] + self.vinfo
        return wr.encode_model("topo", self.nodes, self.inits, vinfo, [wr.encode_value_info(out, (1,) + self.shape[out])])


POOL = (3, 2, (0, 0, 1, 1))  # SqueezeNet's pools: 3x3 / stride 2, ceil mode as bottom / right pads


def module(b, x, p, S=16, E1=64, E3=64, pool=None, swap=False, e1=(1, 0), e3=(3, 1), relu=(1, 1, 1), bias=(1, 1, 1),
           split=False, extra=None, drop=None):
    """One fire module on x, values prefixed p: squeeze (S) -> e1 (E1, (kernel, pad)) / e3 (E3) -> Concat
    [-> pool (kernel, stride, pads)]; returns the value the next squeeze reads.  relu / bias: of (squeeze, e1,
    e3).  swap: Concat(e3, e1).  split: e3 reads a squeeze of its own.  e3 = (3, 0): a 3x3 without pads, so x
    is a plane two larger and e1 reads a 3x3 / pad-0 squeeze of x instead.  extra: one of "s", "e1", "e3", "cat",
    "pool" is read a second time.  drop: a Dropout behind "e1" or "cat"."""
    s = b.conv(x, S, relu=relu[0], bias=bias[0], name=p + "s")
    s1 = s
    if e3 == (3, 0):
        s1 = b.conv(x, S, k=3, pads=0, relu=relu[0], bias=bias[0], name=p + "t")
    elif split:
        s = b.conv(x, S, relu=relu[0], bias=bias[0], name=p + "t")
    a = b.conv(s1, E1, k=e1[0], pads=e1[1], relu=relu[1], bias=bias[1], name=p + "e1")
    c = b.conv(s, E3, k=e3[0], pads=e3[1], relu=relu[2], bias=bias[2], name=p + "e3")
    if extra == "s":
        b.also_read(s)
    if extra == "e1":
        b.also_read(a)
    if extra == "e3":
        b.also_read(c)
    if drop == "e1":
        a = b.dropout(a, p + "d")
    v = b.concat(c, a, p + "cat") if swap else b.concat(a, c, p + "cat")
    if extra == "cat":
        b.also_read(v)
    if drop == "cat":
        v = b.dropout(v, p + "d")
    if pool is not None:
        v = b.pool(v, *pool, name=p + "p")
        if extra == "pool":
            b.also_read(v)
    return v


def tail(b, v, S2=16, relu=True, bias=True, drop=False):
    """the squeeze behind the last module ("n") -> [Dropout] -> GlobalAveragePool; S2 None: GAP of v itself"""
    if S2 is not None:
        v = b.conv(v, S2, relu=relu, bias=bias, name="n")
    if drop:
        v = b.dropout(v, "nd")
    return b.finish(b.gap(v, "y"))


def fire_graph(S2=16, s2_relu=True, s2_bias=True, gap_drop=False, out=None, **kw):
    """the base module + tail; out "cat" / "pool": that value is the 4-D graph output instead"""
    def build(b):
        v = module(b, "x", "m", **kw)
        return b.finish(v) if out else tail(b, v, S2, s2_relu, s2_bias, gap_drop)
    return build


class Entry:
    def __init__(self, name, build, dims, must_f32=(), must_f16=(), f16_refused=None, taps=4, seed=0):
        self.name, self.build, self.dims = name, build, dims
        self.must = {"f32": tuple(must_f32), "f16": tuple(must_f16)}
        self.f16_refused = f16_refused
        self.taps, self.seed = taps, seed
        assert set(self.must["f32"]) | set(self.must["f16"]) <= set(PASSES), name

    @functools.lru_cache(maxsize=None)
    def model(self, mode):
        """(ONNX bytes, builder) in weight mode `mode`"""
        b = Builder(*self.dims, mode, 7919 * self.seed + sum(ord(c) for c in self.name), self.taps)
        return self.build(b), b

    def inputs(self, mode, which=0):
        """the batch of BATCH images (which: another draw)"""
        rng = np.random.default_rng(50021 + 7919 * self.seed + 101 * which + len(self.name))
        shape = (BATCH,) + tuple(self.dims)
        return _ints(rng, -4, 4, shape) if mode == "ints" else rng.standard_normal(shape).astype(np.float32)

    def __repr__(self):
        return self.name


def gap_f32(v):
    """GlobalAveragePool as the kernels reduce it: the pixels summed in order in f32, / their f32 count"""
    n, c = v.shape[:2]
    px = v.reshape(n, c, -1).astype(np.float32)
    s = np.zeros((n, c), np.float32)
    for i in range(px.shape[2]):
        s = s + px[:, :, i]
    return s / np.float32(px.shape[2])


@functools.lru_cache(maxsize=None)
def ints_reference(entry):
    """The float64 run of the entry in ints mode on inputs(0): (output [BATCH, elems] as float32, {value:
    float64 array}).  GlobalAveragePool by gap_f32, so the output is what an exact kernel returns."""
    from golden import f64_ref
    mb, _ = entry.model("ints")
    out, vals = f64_ref.run(mb, entry.inputs("ints"), intermediates=True, gap=gap_f32)
    return out.astype(np.float32), vals


# ---------------------------------------------------------------------------------- the catalogue
CATALOGUE = []
_PLANES = [(12, 12), (9, 8), (8, 7), (13, 13)]
_POOLED = [(21, 20), (20, 21)]
_turn = [0, 0]


def _plane(pooled):
    """the next plane in turn, so that every family sees every plane"""
    lst = _POOLED if pooled else _PLANES
    _turn[pooled] += 1
    return lst[_turn[pooled] % len(lst)]


def add(name, build, dims, **kw):
    assert name not in [e.name for e in CATALOGUE], name
    CATALOGUE.append(Entry(name, build, dims, **kw))


def both(name, must=None, C=16, grow=0, **kw):
    """the unpooled and the pooled form of a base-module variant; grow: the input plane is that much larger"""
    must = must or {}
    for pooled in (False, True):
        H, W = _plane(pooled)
        m = must.get("pool" if pooled else "plain", ((), ()))
        add(name + ("-pool" if pooled else ""), fire_graph(pool=POOL if pooled else None, **kw), (C, H + grow, W + grow),
            must_f32=m[0], must_f16=m[1])


FIRE = {"plain": (["fire_f32"], ["fire_f16"]), "pool": (["fire_pool_f32"], ["fire_f16"])}

# the base module on every plane
for _h, _w in _PLANES:
    add(f"base-{_h}x{_w}", fire_graph(), (16, _h, _w), must_f32=["fire_f32"], must_f16=["fire_f16"])
add("base-7x7", fire_graph(), (16, 7, 7), must_f16=["fire_f16"])  # 49-float planes cannot be 16-B padded: f32 declines
for _h, _w in _POOLED:
    add(f"base-pool-{_h}x{_w}", fire_graph(pool=POOL), (16, _h, _w), must_f32=["fire_pool_f32"], must_f16=["fire_f16"])

# F1: operand order and kinds
both("f1-swapped", swap=True)
both("f1-two-1x1", e3=(1, 0), must={"plain": (["concat_in_place"], ["concat_in_place"]), "pool": (["concat_pool"], [])})
both("f1-two-3x3", e1=(3, 1))
both("f1-e3-pad0", e3=(3, 0), grow=2)
both("f1-e3-5x5", e3=(5, 2))
both("f1-two-squeezes", split=True)

# F2: one Relu or one bias missing (squeeze, e1, e3 of the module; s2: the squeeze behind it)
both("f2-e1-norelu", relu=(1, 0, 1))
both("f2-e3-norelu", relu=(1, 1, 0))
both("f2-s2-norelu", s2_relu=False)
both("f2-e1-nobias", bias=(1, 0, 1))
both("f2-e3-nobias", bias=(1, 1, 0))
both("f2-s2-nobias", s2_bias=False)
# ... and with 32 squeeze channels, where the pooled squeeze recomputes e1 (pool + squeeze, pool + expand)
add("f2-e3-norelu-s32-pool", fire_graph(S=32, relu=(1, 1, 0), pool=POOL), (16, 20, 21),
    must_f32=["pool_squeeze", "pool_expand"])

# F3: a second reader of each value between the module's kernels
for _x in ("s", "e1", "e3"):
    both(f"f3-{_x}-read-twice", extra=_x)
both("f3-cat-read-twice", extra="cat", must={"plain": ([], ["fire_f16_concat"]), "pool": ([], ["fire_f16_concat"])})
add("f3-cat-read-twice-concat-pool", fire_graph(E1=48, E3=80, pool=POOL, extra="cat"), (16, 21, 20))
add("f3-pool-read-twice", fire_graph(pool=POOL, extra="pool"), (16, 20, 21))

# F4: 4-D graph outputs (f32 only: an f16 model's output must be f32)
add("f4-cat-output", fire_graph(out="cat"), (16, 12, 12), must_f32=["concat_in_place"], f16_refused=F16_OUTPUT % "mcat")
add("f4-pool-output", fire_graph(out="pool", pool=POOL), (16, 21, 20), must_f32=["concat_in_place"],
    f16_refused=F16_OUTPUT % "mp")
add("f4-conv-pool-output", lambda b: b.finish(b.pool(b.conv("x", 32, k=3, pads=1, name="c"), *POOL)), (16, 20, 21),
    must_f32=["conv_pool"], f16_refused=F16_OUTPUT % "p")

# F5: channel counts off the kernels' multiples
both("f5-e48-e80", E1=48, E3=80, must={"pool": (["concat_pool"], [])})
both("f5-e32-e96", E1=32, E3=96, must={"plain": ([], ["fire_f16"]), "pool": (["concat_pool"], ["fire_f16"])})
both("f5-s2-24", S2=24, must=FIRE)
both("f5-s2-72", S2=72)
both("f5-s1-8", S=8)
both("f5-s1-24", S=24)
both("f5-s1-80", S=80)  # above the f16 kernels' 64

# F6: pool geometry behind the module
for _pads in ([0, 0, 0, 0], [0, 0, 1, 1], [1, 1, 1, 1], [2, 2, 0, 0], [0, 0, 2, 2]):
    add("f6-pads-" + "".join(map(str, _pads)), fire_graph(pool=(3, 2, _pads)), (16,) + _plane(True))
add("f6-pool-2x2s2", fire_graph(pool=(2, 2, [0, 0, 0, 0])), (16, 21, 20))
add("f6-pool-3x3s1", fire_graph(pool=(3, 1, [1, 1, 1, 1])), (16, 12, 12))


# F7: other strided writers into a Concat
def _pool_concat(pool_first):
    def build(b):
        s = b.conv("x", 16, name="s")
        p = b.pool(s, 3, 1, [1, 1, 1, 1])
        c = b.conv(s, 32, k=3, pads=1, name="c")
        return tail(b, b.concat(p, c, "cat") if pool_first else b.concat(c, p, "cat"))
    return build


def _nested(S2):
    def build(b):
        s = b.conv("x", 16, name="s")
        e1, e3 = b.conv(s, 64, name="e1"), b.conv(s, 64, k=3, pads=1, name="e3")
        e5 = b.conv(s, 32, k=5, pads=2, name="e5")
        return tail(b, b.concat(b.concat(e1, e3, "cat"), e5, "cat2"), S2)
    return build


add("f7-concat-pool-conv", _pool_concat(True), (16, 13, 13), must_f32=["concat_in_place"])
add("f7-concat-conv-pool", _pool_concat(False), (16, 9, 8), must_f32=["concat_in_place"])
add("f7-nested-squeeze", _nested(16), (16, 12, 12), must_f16=["fire_f16_concat"])
add("f7-nested-gap", _nested(None), (16, 13, 13), must_f16=["fire_f16_concat"])


# F8: pool + squeeze and pool + expand
def _standing_pool(C=32, M=64, stride=1, pads=0, from_input=False):
    """a pool that no producer can take (its input has a second reader, or is the model input) -> 1x1 conv"""
    def build(b):
        v = "x"
        if not from_input:
            v = b.conv("x", C, name="c")
            b.also_read(v)
        n = b.conv(b.pool(v, *POOL), M, stride=stride, pads=pads, name="n")
        return b.finish(b.gap(n, "y"))
    return build


add("f8-pool-squeeze-m64", _standing_pool(), (16, 21, 20), must_f32=["pool_squeeze"])
add("f8-pool-squeeze-m72", _standing_pool(M=72), (16, 20, 21))
add("f8-pool-squeeze-c48", _standing_pool(C=48), (16, 21, 20))
add("f8-pool-squeeze-stride2", _standing_pool(stride=2), (16, 20, 21))
add("f8-pool-squeeze-pads0011", _standing_pool(pads=[0, 0, 1, 1]), (16, 21, 20))
add("f8-pool-of-input", _standing_pool(from_input=True), (32, 20, 21), must_f32=["pool_squeeze"])
for _s in (32, 64, 48):
    add(f"f8-fire-pool-s{_s}", fire_graph(S=_s, pool=POOL), (16,) + _plane(True), must_f32=["fire_pool_f32"],
        must_f16=["fire_f16"])


# F9: the first conv
def _first(C=3, M=96, k=7, Q=16, q_relu=True, twice=False, q_pads=0):
    def build(b):
        p = b.pool(b.conv("x", M, k=k, stride=2, name="c1"), *POOL)
        if twice:
            b.also_read(p)
        return b.finish(b.gap(b.conv(p, Q, pads=q_pads, relu=q_relu, name="n"), "y"))
    return build, (C, 37, 35)


add("f9-first-q16", *_first(), must_f32=["conv_pool", "first_squeeze"], must_f16=["conv_pool", "first_squeeze"])
add("f9-first-q24", *_first(Q=24), must_f32=["conv_pool"], must_f16=["conv_pool", "first_squeeze"])
add("f9-first-q-norelu", *_first(q_relu=False), must_f32=["conv_pool"], must_f16=["conv_pool"])
add("f9-first-q-pads0011", *_first(q_pads=[0, 0, 1, 1]), must_f32=["conv_pool"], must_f16=["conv_pool"])
add("f9-first-pool-read-twice", *_first(twice=True), must_f32=["conv_pool"], must_f16=["conv_pool"])
add("f9-first-c4-m64", *_first(C=4, M=64), must_f32=["conv_pool"], must_f16=["conv_pool", "first_squeeze"])
add("f9-first-5x5", *_first(k=5), must_f32=["conv_pool"], must_f16=["conv_pool"])


# F10: conv + GAP (a conv in front puts its input into the arena, f16: into the 16-B NHWC layout)
def _conv_gap(C=64, relu=True, twice=False):
    def build(b):
        g = b.conv(b.conv("x", C, name="c"), 32, relu=relu, name="cg")
        if twice:
            b.extras.append(b.gap(b.conv(g, 16, name="c2"), "g2"))
        return b.finish(b.gap(g, "y"))
    return build


add("f10-conv-gap-c64", _conv_gap(), (16, 13, 13), must_f32=["conv_gap"], must_f16=["conv_gap"])
add("f10-conv-gap-c48", _conv_gap(C=48), (16, 13, 13))
add("f10-conv-gap-17x17", _conv_gap(), (16, 17, 17))  # more than 256 pixels
add("f10-conv-read-twice", _conv_gap(twice=True), (16, 13, 13))
add("f10-conv-gap-norelu", _conv_gap(relu=False), (16, 12, 12), must_f32=["conv_gap"], must_f16=["conv_gap"])

# F11: aliases
both("f11-dropout-cat", drop="cat")
both("f11-dropout-e1", drop="e1")
both("f11-dropout-gap", gap_drop=True, must=FIRE)

# F12: seeded compositions of two or three modules, at most one pool between two of them
_VARIANTS = [{}, {}, {"swap": True}, {"e3": (5, 2)}, {"e3": (1, 0)}, {"e1": (3, 1)}, {"split": True}, {"relu": (1, 1, 0)},
             {"relu": (1, 0, 1)}, {"bias": (1, 0, 1)}, {"bias": (0, 1, 1)}, {"E1": 48, "E3": 80}, {"E1": 32, "E3": 96},
             {"S": 32}, {"S": 24}, {"S": 64}, {"drop": "cat"}, {"drop": "e1"}, {"extra": "cat"}, {"extra": "e1"},
             {"extra": "s"}]
_POOLS = [None, POOL, (3, 2, (1, 1, 1, 1)), (3, 2, (0, 0, 0, 0)), (2, 2, (0, 0, 0, 0))]


def _composition(seed):
    """deterministic in seed: (build, dims, description)"""
    rng = np.random.default_rng(4242 + seed)
    H, W = [(21, 20), (20, 21), (13, 13), (12, 12)][int(rng.integers(4))]
    mods, h = [], min(H, W)
    for i in range(int(rng.integers(2, 4))):
        kw = dict(_VARIANTS[int(rng.integers(len(_VARIANTS)))])
        pool = _POOLS[int(rng.integers(len(_POOLS)))] if h >= 12 else None
        if pool is not None:
            h = (h + pool[2][0] + pool[2][2] - pool[0]) // pool[1] + 1
        mods.append((kw, pool))
    S2 = [16, 16, 24, 64][int(rng.integers(4))]

    def build(b):
        v = "x"
        for i, (kw, pool) in enumerate(mods):
            v = module(b, v, f"m{i}", pool=pool, **kw)
        return tail(b, v, S2)
    return build, (16, H, W), f"{H}x{W} " + " | ".join(f"{kw}{' pool ' + str(p) if p else ''}" for kw, p in mods) + f" | S2={S2}"


for _seed in range(16):
    _b, _d, _ = _composition(_seed)
    add(f"f12-seed{_seed}", _b, _d, seed=_seed, taps=3)

BY_NAME = {e.name: e for e in CATALOGUE}
