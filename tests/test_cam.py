"""The references of tests/test_cam_gpu.py on their own (no GPU): what its checks lean on is asserted here, on the
CPU, so that no GPU test can hide behind a loose reference.

The f16 anchor of the GPU tests is _convref.f16_layer_check with bad == 0, which says something only while few
outputs have two admissible f16 values: for every test graph, and for SqueezeNet's conv10 at 64 on the seeded
images, an exact f16 forward pass keeps the map conv's ambiguous share under F16_AMBIGUOUS_CAP.  The per-op case
table reaches the edges it is there for, and head() finds the map conv where there is one."""
import os

import numpy as np
import pytest

import _cam
import _sizes
from _convref import F16_AMBIGUOUS_CAP

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", sorted(_cam.GRAPHS))
def test_graph_f16_reference_within_cap(name):
    amb = _cam.f16_exact_head(name)
    print(f"cam graph {name}: ambiguous share of the map conv over all classes {amb:.4f}")
    assert amb <= F16_AMBIGUOUS_CAP


def test_squeezenet_f16_reference_within_cap():
    from ore import squeezenet
    rows = _sizes.f16_exact_forward(64, squeezenet.synthetic_input(_cam.BATCH, 64, seed=_cam.SQ_SEED))
    name, amb, peak = rows[-1]
    print(f"cam squeezenet 64: {name} ambiguous {amb:.4f}, max |y| {peak:.1f}")
    assert name.startswith("conv10") and amb <= F16_AMBIGUOUS_CAP and peak < 65504.0


def test_op_cases_reach_their_edges():
    cases = _cam.op_cases()
    assert len(cases) == len(set(cases))
    assert {c[2] * c[3] for c in cases} == {1, 15, 16, 143, 169, 289}  # one block, a tail, more than 256 pixels
    assert any(c[0] % 4 for c in cases) and any(c[0] % 32 and not c[0] % 4 for c in cases)
    ks = {c[4] for c in cases}
    assert {1, 5, 9, 17, 33, 64} <= ks and 40 in ks  # across the 16- and the 32-row tiles, and min(M, 64) of each M
    assert {(c[5], c[6]) for c in cases} == {(1, 1), (3, 1), (3, 3)}
    for case in cases:
        x, w, b, classes = _cam.op_inputs(case)
        C, M, H, W, k, n, views = case
        assert classes.shape == (n // views, k) and classes.min() >= 0 and classes.max() < M
        assert (classes == M - 1).any() and (k == 1 and n // views == 1 or (classes == 0).any())
        if k >= 4:
            assert classes[0, 1] == classes[0, 2]


def test_head_finds_the_map_conv():
    from ore import squeezenet
    for name, (C, M, H, W, relu, reshape, seed) in _cam.GRAPHS.items():
        h = _cam.head(_cam.graph_bytes(name))
        assert h["w"].shape == (M, C) and h["b"].shape == (M,) and h["relu"] == relu and h["x"] == "c1r"
        assert h["T"] == ("mapr" if relu else "map")
    h = _cam.head(squeezenet.build(64))
    assert h["w"].shape == (1000, 512) and h["relu"]
    with open(os.path.join(GOLD, "mnist-8.onnx"), "rb") as f:
        assert _cam.head(f.read()) is None


def test_gather_and_f64_reference():
    rng = np.random.default_rng(3)
    T = rng.standard_normal((4, 7, 2, 3))
    cls = np.array([[6, 0, 6], [1, 2, 3]])
    g = _cam.gather(T, cls, views=2)
    assert g.shape == (4, 3, 2, 3)
    assert np.array_equal(g[1, 2], T[1, 6]) and np.array_equal(g[2, 0], T[2, 1]) and np.array_equal(g[3, 2], T[3, 3])
    x = rng.standard_normal((4, 5, 2, 3)).astype(np.float32)
    w = rng.standard_normal((7, 5)).astype(np.float32)
    b = rng.standard_normal(7).astype(np.float32)
    y, mag = _cam.maps_f64(x, w, b, cls, relu=True, views=2)
    want = np.maximum(np.einsum("mc,nchw->nmhw", w.astype(np.float64), x.astype(np.float64)) + b[None, :, None, None], 0.0)
    assert np.allclose(y, _cam.gather(want, cls, views=2), rtol=0, atol=1e-12) and (mag > 0).all()
