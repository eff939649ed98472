"""The references of tests/test_sizes_gpu.py on their own (no GPU): what the size sweep's checks lean on is
asserted here, on the CPU, so that no GPU test can hide behind a loose reference.

Per size of _sizes.SIZES, on the seeded images: the float64 top-2 gap is >= 1e-3 on every image (the argmax
check skips nothing) and the oracle is within 1e-5 of float64 (the allowance `1e-5 + |oracle - f64|` of the
Winograd plan check at most doubles the north_star bound).  Measured: gap >= 0.11, |oracle - f64| <= 8.9e-6
(226; 6.3e-6 at 131, 5.5e-6 at 227).  At 131, 163 and 227 an exact f16 forward pass stays within
f16_layer_check's cap on ambiguous outputs and far from the f16 range's end.  The image counts of the
partial-batch runs hold the grouping rule's change points.  build(int) == build((int, int))."""
import numpy as np
import pytest

import _sizes
from _convref import F16_AMBIGUOUS_CAP

IDS = [_sizes.size_id(hw) for hw in _sizes.SIZES]


def test_sizes_reach_what_they_claim():
    """The planes the size table lists, from the pads and strides of the graph."""
    want = {131: (63, 31, 15, 7), 139: (67, 33, 16, 7), 163: (79, 39, 19, 9), 194: (94, 46, 23, 11),
            220: (107, 53, 26, 12), 226: (110, 54, 27, 13), 227: (111, 55, 27, 13), 256: (125, 62, 31, 15), 288: (141, 70, 35, 17)}
    for hw, sides in want.items():
        assert _sizes.planes(hw) == [(s, s) for s in sides], hw
    assert _sizes.planes((163, 226)) == [(79, 110), (39, 54), (19, 27), (9, 13)]
    assert _sizes.planes((227, 139)) == [(111, 67), (55, 33), (27, 16), (13, 7)]
    assert [hw for hw in _sizes.SIZES if isinstance(hw, int) and _sizes.planes(hw)[0][1] % 2 == 0] == [194, 226]
    assert [_sizes.image_count(hw) for hw in _sizes.SIZES] == [3, 3, 3, 3, 3, 2, 2, 2, 2, 3, 3]
    for hw in _sizes.SIZES:
        h, w = _sizes.hw_pair(hw)
        x = _sizes.images(hw)
        assert x.shape == (_sizes.image_count(hw), 3, h, w) and x.dtype == np.float32


@pytest.mark.parametrize("hw", _sizes.SIZES, ids=IDS)
def test_reference_caps(hw):
    r64, ro = _sizes.references(hw)
    assert r64.shape == ro.shape == (_sizes.image_count(hw), 1000)
    top = np.sort(r64, axis=1)[:, -2:]
    gap = float((top[:, 1] - top[:, 0]).min())
    d = float(np.abs(ro - r64).max())
    print(f"sizes reference {_sizes.size_id(hw)}: float64 top-2 gap {gap:.4f}, |oracle - f64| {d:.3g}")
    assert gap >= 1e-3
    assert d <= 1e-5
    assert np.array_equal(ro.argmax(1), r64.argmax(1))
    assert np.abs(r64.sum(1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("hw", _sizes.F16_EXACT_SIZES)
def test_f16_exact_forward_within_caps(hw):
    """An exact f16 forward pass: every layer's ambiguous share <= 1/3 and no |value| near 65504, so the GPU
    sweep's f16_layer_check has room on these sizes' data.  Measured: ambiguous at most 0.115
    (fire9/squeeze1x1, at each of the three sizes), max |y| 299."""
    rows = _sizes.f16_exact_forward(hw, _sizes.images(hw))
    assert len(rows) == 26
    name, amb, _ = max(rows, key=lambda r: r[1])
    peak = max(r[2] for r in rows)
    print(f"sizes f16 exact {hw}: worst ambiguous {amb:.4f} at {name}, max |y| {peak:.1f}")
    assert amb <= F16_AMBIGUOUS_CAP
    assert peak < 65504.0


def test_partial_counts_hold_the_change_points():
    counts = _sizes.partial_counts()
    assert set(_sizes.PARTIAL_BASE) <= set(counts)
    assert all(1 <= n < _sizes.PARTIAL_MAX for n in counts) and list(counts) == sorted(set(counts))
    layers = [(27, 27, 256), (27, 27, 192), (13, 13, 256)]
    assert set(layers) <= set(_sizes.expand3x3_layers())
    for layer in dict.fromkeys(layers + _sizes.expand3x3_layers()):
        # the change points by the rule itself, every n of 1..256 in one dump
        gs = _sizes.dump(_sizes.NCU, [(n,) + layer for n in range(1, _sizes.PARTIAL_MAX + 1)])
        mbs = [g["mbs"] for g in gs]
        changes = [n for n in range(2, _sizes.PARTIAL_MAX + 1) if mbs[n - 1] != mbs[n - 2]]
        assert changes == _sizes.mbs_changes(layer), layer
        for n in changes:
            assert n in counts or n == _sizes.PARTIAL_MAX, (layer, n)
            assert n - 1 in counts, (layer, n)
        tails = [n for n in range(1, _sizes.PARTIAL_MAX) if gs[n - 1]["nsmall"] > 0]
        assert not tails or set(tails) & set(counts), layer
    # 27 x 27 / M = 256 and M = 192 do change below 256 images; 13 x 13 stays on single blocks
    assert _sizes.mbs_changes((27, 27, 256)) and _sizes.mbs_changes((27, 27, 192))
    assert _sizes.mbs_changes((13, 13, 256)) == []


def test_int_and_pair_build_the_same_bytes():
    from ore import squeezenet
    assert squeezenet.build(224) == squeezenet.build((224, 224))
    assert squeezenet.build_calibrated(224) == squeezenet.build_calibrated((224, 224))
    assert np.array_equal(squeezenet.synthetic_input(2, 64, seed=5), squeezenet.synthetic_input(2, (64, 64), seed=5))
    a, b = squeezenet.build((163, 226)), squeezenet.build((226, 163))
    assert a != b and len(a) == len(b)  # the same weights behind another input shape
    assert squeezenet.synthetic_input(1, (5, 7)).shape == (1, 3, 5, 7)
