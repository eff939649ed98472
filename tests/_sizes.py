"""Shared by tests/test_sizes.py (CPU) and tests/test_sizes_gpu.py: SqueezeNet-1.0 at input sizes other
than 64 and 224, square and not, and the image counts of the partial-batch runs on the 256-image plan.

Per size the model bytes, the seeded images and their two references -- the float64 executor
(tests/golden/f64_ref.py) and the oracle -- are computed once and shared (lru_cache); callers do not write
into them.  test_sizes.py holds the caps on the references alone (float64 top-2 gap, |oracle - f64|), so
no GPU test can hide behind a loose reference."""
import functools

import numpy as np

from _convref import f16_layer_check
from _wino_groups import dump

# conv1 / pool1 / pool3 / pool5 planes: 131 63/31/15/7 (pool1 plane 961 < FIRE_POOL_MIN_HW), 139 67/33/16/7,
# 163 79/39/19/9, 194 94/46/23/11 (even conv1 width), 226 110/54/27/13 (224's planes behind an even conv1
# width), 227 111/55/27/13 (the Caffe size), 256 125/62/31/15, 288 141/70/35/17 (conv10 on 289 pixels).
# 220 107/53/26/12 is there for the first conv's band walkers: they take input widths that are a multiple of 4
# (so never an even conv width), f32 from 212 to 224, f16 up to 224, and only behind the conv + pool fusion,
# whose patch rule (EPOOL_MAX_WORK) holds at 220 and 224 but not at 212 and 216 -- no other square size than
# 224 reaches them on the 256-image plan.
SIZES = [131, 139, 163, 194, 220, 226, 227, 256, 288, (163, 226), (227, 139)]
F16_EXACT_SIZES = [131, 163, 227]  # the CPU f16 forward pass (test_sizes.py)
SEED = 8  # of synthetic_input, every size; test_sizes.py asserts what it must give (seeds 0, 1, 2 do not)
NCU = 256  # an MI355X: the LDS Winograd kernel's grouping rule takes the CU count
PARTIAL_HW = 227  # part 3: partial batches on the 256-image plan
PARTIAL_MAX = 256
PARTIAL_BASE = [1, 2, 3, 5, 8, 17, 64, 65, 129, 255]


def size_id(hw):
    return str(hw) if isinstance(hw, int) else f"{hw[0]}x{hw[1]}"


def hw_pair(hw):
    return (hw, hw) if isinstance(hw, int) else tuple(hw)


def image_count(hw):
    """3 images per size below 224, 2 from 224 up (a non-square size by its smaller side)."""
    return 3 if min(hw_pair(hw)) < 224 else 2


def planes(hw):
    """[(H, W)] of the conv1, pool1, pool3 and pool5 outputs."""
    def out(v, k, s, hi):
        return (v + hi - k) // s + 1
    res = []
    h, w = hw_pair(hw)
    for k, s, hi in ((7, 2, 0), (3, 2, 0), (3, 2, 1), (3, 2, 0)):
        h, w = out(h, k, s, hi), out(w, k, s, hi)
        res.append((h, w))
    return res


@functools.lru_cache(maxsize=None)
def model_bytes(hw):
    from ore import squeezenet
    return squeezenet.build(hw)


@functools.lru_cache(maxsize=None)
def graph(hw):
    """(nodes, {initializer name: array}) of the size's model."""
    from ore import onnx_wire
    g = onnx_wire.decode_model(model_bytes(hw)).graph
    return list(g.node), {t.name: t.to_numpy() for t in g.initializer}


@functools.lru_cache(maxsize=None)
def images(hw):
    from ore import squeezenet
    x = squeezenet.synthetic_input(image_count(hw), hw, seed=SEED)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def references(hw):
    """(float64 rows, oracle rows) of the size's images, [n, 1000] each."""
    import oracle
    from golden import f64_ref
    mb = model_bytes(hw)
    r64 = f64_ref.run(mb, images(hw))
    om = oracle.Model(mb)
    try:
        ro = om.run(images(hw), r64.shape[1])
    finally:
        om.close()
    r64.setflags(write=False)
    ro.setflags(write=False)
    return r64, ro


def margins(y, hw):
    """test_config4_gpu.py's margins of GPU rows y against the size's references, per image."""
    r64, ro = references(hw)
    return [{"image": i, "vs_oracle": float(np.abs(y[i] - ro[i]).max()), "vs_f64": float(np.abs(y[i] - r64[i]).max()),
             "oracle_vs_f64": float(np.abs(ro[i] - r64[i]).max())} for i in range(len(y))]


def conv_nodes(hw):
    """[(node, w, b, pads, strides)] of the model's 26 convs, in graph order."""
    nodes, inits = graph(hw)
    res = []
    for n in nodes:
        if n.op_type == "Conv":
            a = n.attrs()
            res.append((n, inits[n.input[1]], inits[n.input[2]], list(a["pads"].ints), list(a["strides"].ints)))
    return res


def f16_exact_forward(hw, x):
    """The f16 model's contract walked on the CPU: every conv + Relu output is f16_layer_check's `ref` (the
    nearest f16 of the float64 sum over the f16 operands, Relu applied) of the layer's own input; MaxPool and
    Concat are exact on those values.  -> [(conv name, ambiguous share, max |y|)] over the 26 convs."""
    import oracle
    nodes, inits = graph(hw)
    env = {"data_0": np.asarray(x, dtype=np.float32)}
    rows = []
    for n in nodes:
        a = n.attrs()
        v = env[n.input[0]]
        if n.op_type == "Conv":  # every conv of the graph feeds a Relu: checked as one layer, as the GPU sweep does
            w, b = inits[n.input[1]], inits[n.input[2]]
            pads, strides = list(a["pads"].ints), list(a["strides"].ints)
            ho = (v.shape[2] + pads[0] + pads[2] - w.shape[2]) // strides[0] + 1
            wo = (v.shape[3] + pads[1] + pads[3] - w.shape[3]) // strides[1] + 1
            # ref and ambiguous depend on the layer's input alone: a first pass for ref, then ref as `got`
            ref = f16_layer_check(np.zeros((v.shape[0], w.shape[0], ho, wo), np.float32), v, w, b, pads, strides, True)["ref"]
            y = ref.astype(np.float32)
            res = f16_layer_check(y, v, w, b, pads, strides, True)
            assert res["ok"].all() and res["acc_ratio"] == 0.0, n.name
            rows.append((n.name, res["ambiguous"], float(np.abs(y).max())))
        elif n.op_type == "Relu":
            y = np.maximum(v, np.float32(0))  # of a conv: already applied
        elif n.op_type == "MaxPool":
            y = oracle.maxpool2d(v, a["kernel_shape"].ints, a["strides"].ints, auto_pad=a["auto_pad"].s.decode(),
                                 pads=a["pads"].ints)
        elif n.op_type == "Concat":
            y = np.concatenate([v, env[n.input[1]]], axis=1)
        elif n.op_type == "Dropout":
            y = v
        else:  # GlobalAveragePool, Softmax: behind the last conv
            break
        env[n.output[0]] = y
    return rows


# ---- part 3: the image counts of the partial-batch runs ----

def expand3x3_layers(hw=PARTIAL_HW):
    """(H, W, M) of the eight expand3x3 convs: the layers a plan may run on the LDS Winograd kernel."""
    from ore import squeezenet
    p = planes(hw)
    res = []
    plane = p[1]
    for name, _, e in squeezenet.FIRES:
        res.append((plane[0], plane[1], e))
        if name == "fire4":
            plane = p[2]
        elif name == "fire8":
            plane = p[3]
    return res


@functools.lru_cache(maxsize=None)
def _groups(n, layer):
    g = dump(NCU, [(n,) + layer])[0]
    assert g is not None, (n, layer)
    return g["mbs"], g["nsmall"]


def mbs_changes(layer, nmax=PARTIAL_MAX):
    """Every n in 2..nmax at which the grouping rule's `mbs` of `layer` (H, W, M) differs from its value at
    n - 1.  mbs does not decrease with n (wm_groups: a block count b qualifies once ntg * (mtiles / b) reaches
    WM_MIN_WG, and ntg grows with n), so equal ends hold no change between them."""
    def walk(lo, hi):
        if _groups(lo, layer)[0] == _groups(hi, layer)[0]:
            return []
        if hi == lo + 1:
            return [hi]
        mid = (lo + hi) // 2
        return walk(lo, mid) + walk(mid, hi)
    return walk(1, nmax)


def nsmall_count(layer, nmax=PARTIAL_MAX):
    """The largest n < nmax at which `layer` has single-block tail groups (nsmall > 0), or None.  Only groups of
    two or more blocks have a tail, and mbs does not decrease with n."""
    if _groups(nmax - 1, layer)[0] == 1:
        return None
    gs = dump(NCU, [(n,) + layer for n in range(1, nmax)])
    tails = [n for n, g in zip(range(1, nmax), gs) if g is not None and g["nsmall"] > 0]
    return max(tails) if tails else None


def has_nsmall(layer, counts):
    return any(_groups(n, layer)[1] > 0 for n in counts)


@functools.lru_cache(maxsize=None)
def partial_counts(layers=None):
    """The image counts part 3 runs on the 256-image plan: PARTIAL_BASE, and for every layer of `layers`
    ((H, W, M) tuples; default: all eight expand3x3 layers at PARTIAL_HW, a superset of any plan's Winograd
    layers) each n at which mbs changes with the n - 1 before it, and one n with nsmall > 0 where one exists."""
    layers = tuple(dict.fromkeys(expand3x3_layers() if layers is None else layers))
    counts = set(PARTIAL_BASE)
    for layer in layers:
        for n in mbs_changes(layer):
            counts.update((n, n - 1))
    for layer in layers:
        if not has_nsmall(layer, [n for n in counts if n < PARTIAL_MAX]):
            n = nsmall_count(layer)
            if n is not None:
                counts.add(n)
    return tuple(sorted(n for n in counts if 1 <= n < PARTIAL_MAX))
