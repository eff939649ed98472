"""The topology catalogue (tests/_topologies.py) and its two references, without a GPU: before either
reference judges a kernel, every ints-mode graph decodes, stays in small integers throughout (exact in
f16 and through the f32 Winograd transforms), has a non-degenerate output, and the C oracle agrees with
the float64 executor on it bit for bit."""
import numpy as np
import pytest

import oracle
from _topologies import BATCH, BY_NAME, CATALOGUE, INT_LIMIT, PASSES, Builder, _composition, gap_f32, ints_reference

NAMES = [e.name for e in CATALOGUE]


def test_catalogue_shape():
    assert len(NAMES) == len(set(NAMES)) and len(CATALOGUE) >= 70
    assert [n for n in NAMES if n.startswith("f12-")] == [f"f12-seed{s}" for s in range(16)]
    refused = [e.name for e in CATALOGUE if e.f16_refused]
    assert len(refused) <= 8, refused
    # every matching pass has an entry that declares it under FUSE_ALL | FUSE_EAGER
    declared = {p for e in CATALOGUE for prec in ("f32", "f16") if not (prec == "f16" and e.f16_refused) for p in e.must[prec]}
    assert declared == set(PASSES), set(PASSES) - declared


def test_compositions_deterministic():
    from ore import onnx_wire
    for seed in (0, 7, 15):
        assert _composition(seed)[2] == _composition(seed)[2]
        e = BY_NAME[f"f12-seed{seed}"]
        assert e.build(Builder(*e.dims, "ints", 1, 3)) == e.build(Builder(*e.dims, "ints", 1, 3))  # the same bytes
    descs = {_composition(s)[2] for s in range(16)}
    assert len(descs) >= 14, descs  # the seeds draw different graphs
    for s in range(16):
        n = sum(1 for nd in onnx_wire.decode_model(BY_NAME[f"f12-seed{s}"].model("ints")[0]).graph.node if nd.op_type == "Concat")
        assert n >= 2  # two or three modules


@pytest.mark.parametrize("name", NAMES)
def test_ints_reference(name):
    from ore import onnx_wire
    e = BY_NAME[name]
    mb, b = e.model("ints")
    g = onnx_wire.decode_model(mb).graph
    assert [v.name for v in g.input if v.name == "x"] == ["x"] and len(g.output) == 1 and g.output[0].name == b.out
    x = e.inputs("ints")
    assert x.shape == (BATCH,) + tuple(e.dims) and np.array_equal(x, np.round(x)) and np.abs(x).max() <= 4
    out, vals = ints_reference(e)
    averaged = set()  # GlobalAveragePool outputs and what joins them: means, not integers
    for nd in g.node:
        if nd.op_type == "GlobalAveragePool" or any(i in averaged for i in nd.input):
            averaged.update(nd.output)
    biggest = 0.0
    for vname, v in vals.items():
        assert v.shape[1:] == b.shape[vname], (vname, v.shape, b.shape[vname])
        if vname in averaged:
            continue
        assert np.array_equal(v, np.round(v)), vname
        biggest = max(biggest, float(np.abs(v).max()))
    print(f"{name}: max |intermediate| {biggest:.0f}, non-zero outputs {np.mean(out != 0):.2f}")
    assert biggest <= INT_LIMIT, biggest
    assert np.mean(out != 0) >= 0.10 and len(np.unique(out)) > 1
    assert out.shape == (BATCH, int(np.prod(b.shape[b.out])))
    # the oracle (f32, the reference's summation order) is exact on integers: the same bits
    ref = oracle.Model(mb).run(x, out.shape[1])
    np.testing.assert_array_equal(ref, out)


@pytest.mark.parametrize("name", NAMES[::9])
def test_real_mode_builds(name):
    """the real-valued weights of an entry: the same graph (node for node), other initializers"""
    from ore import onnx_wire
    e = BY_NAME[name]
    gi, gr = (onnx_wire.decode_model(e.model(m)[0]).graph for m in ("ints", "real"))
    assert [(n.op_type, list(n.input), list(n.output)) for n in gi.node] == [(n.op_type, list(n.input), list(n.output)) for n in gr.node]
    w = next(t for t in gr.initializer if t.name.startswith("w_")).to_numpy()
    assert not np.array_equal(w, np.round(w))
    assert e.inputs("real").dtype == np.float32 and not np.array_equal(e.inputs("real"), e.inputs("real", 1))


def test_gap_f32_matches_sequential_sum():
    v = np.arange(2 * 3 * 4 * 8, dtype=np.float64).reshape(2, 3, 4, 8) % 11 - 4  # 32 pixels: the division is exact
    np.testing.assert_array_equal(gap_f32(v), (v.reshape(2, 3, -1).sum(-1) / 32).astype(np.float32))
