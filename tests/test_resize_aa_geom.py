"""CPU: the tap map of the antialiased resize (ore_resize_aa_taps, csrc/ore_resize_geom.h) against the set
definition by brute force, and the numpy restatement of the arithmetic (tests/_resize_aa_ref.py) against
torch's float64 antialias=True on the CPU.  No kernel is launched here."""
import numpy as np
import pytest

import ore
from _resize_aa_ref import MAX_TAPS, aa_taps_ref, resize_aa_ref
from _resize_ref import images, resize_ref


def _check_axis(S, D, origin, count):
    first, ntaps, total, weights = ore.resize_aa_taps(S, D, origin, count)
    assert weights.shape == (count, MAX_TAPS)
    for k, (f, u) in enumerate(aa_taps_ref(S, D, origin, count)):  # aa_taps_ref asserts a contiguous, non-empty run
        assert len(u) <= MAX_TAPS
        assert (int(first[k]), int(ntaps[k]), int(total[k])) == (f, len(u), int(u.sum())), (S, D, origin + k)
        np.testing.assert_array_equal(weights[k, :len(u)], u)
        assert not weights[k, len(u):].any()
        assert 0 < u.min() and u.max() < 1 << 15 and u.sum() <= 1 << 21


def test_taps_every_small_axis():
    """Every (S, D) with 1 <= D < S <= 40 within the ratio rule, all resized indices."""
    seen = 0
    for S in range(2, 41):
        for D in range(1, S):
            if S > 32 * D:
                with pytest.raises(ore.OreError, match="32"):
                    ore.resize_aa_taps(S, D, 0, D)
                continue
            _check_axis(S, D, 0, D)
            seen += 1
    assert seen > 700


@pytest.mark.parametrize("S,D", [(16384, 512), (16384, 16383), (500, 341), (1080, 224)])
def test_taps_large_axes(S, D):
    """Both edges and the middle; origins and counts at the far edge."""
    _check_axis(S, D, 0, min(D, 40))
    _check_axis(S, D, D - min(D, 40), min(D, 40))
    _check_axis(S, D, D // 2, 3)
    _check_axis(S, D, D - 1, 1)


def test_taps_ratio_rule_and_arguments():
    ore.resize_aa_taps(64, 2, 0, 2)  # exactly 32
    ore.resize_aa_taps(16384, 512, 511, 1)
    with pytest.raises(ore.OreError, match="32"):
        ore.resize_aa_taps(66, 2, 0, 2)  # 33
    with pytest.raises(ore.OreError, match="32"):
        ore.resize_aa_taps(33, 1, 0, 1)
    with pytest.raises(ore.OreError, match="32"):
        ore.resize_aa_taps(16384, 511, 0, 1)
    for S, D in [(8, 8), (5, 9)]:
        with pytest.raises(ore.OreError, match="does not shrink.*ore_resize_taps"):
            ore.resize_aa_taps(S, D, 0, 1)
    for S, D, origin, count in [(0, 4, 0, 4), (16385, 4000, 0, 4), (8, 4, -1, 2), (8, 4, 2, 3), (8, 4, 0, 0), (8, 4, 0, 5)]:
        with pytest.raises(ore.OreError, match="resize taps"):
            ore.resize_aa_taps(S, D, origin, count)


# (n, Hs, Ws, C), (Rh, Rw), (top, left), (H, W): the four axis combinations
TORCH_CASES = [
    ((1, 7, 5, 3), (20, 15), (0, 0), (20, 15)),        # neither axis shrinks
    ((2, 33, 64, 3), (18, 20), (0, 0), (18, 20)),      # both shrink
    ((1, 96, 96, 1), (3, 3), (0, 0), (3, 3)),          # ratio 32: 64 taps
    ((1, 64, 33, 3), (40, 50), (3, 7), (30, 40)),      # rows shrink, columns are upscaled; a crop
    ((1, 31, 17, 4), (31, 5), (0, 0), (31, 5)),        # columns only
    ((1, 7, 5, 2), (3, 2), (0, 0), (3, 2)),            # clipped edge taps
    ((1, 75, 100, 3), (51, 68), (3, 6), (45, 45)),     # the workload's ratios at a fifth of its size
]


@pytest.mark.parametrize("shape,resized,origin,out", TORCH_CASES, ids=lambda v: "x".join(map(str, v)))
def test_reference_matches_torch_float64(shape, resized, origin, out):
    """Bound, in grey levels: 255 (T + 8) 2^-24 with T the largest row-tap count (2 on a plain axis): every
    float32 step of the chain -- the conversion of the column sum, T multiplies and T adds of the vertical
    step or the lerp's three, two divisions -- errs by at most half an ulp of a value of at most 255 (after
    the divisions; relative to it before), against float64 arithmetic that is exact at this scale."""
    import torch
    import torch.nn.functional as F
    x = images(shape, seed=40)
    (rh, rw), (top, left), (h, w) = resized, origin, out
    hs = shape[1]
    T = max(len(u) for _, u in aa_taps_ref(hs, rh, top, h)) if hs > rh else 2
    got = resize_aa_ref(x, resized, origin, out)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).double()
    want = F.interpolate(xt, size=(rh, rw), mode="bilinear", align_corners=False, antialias=True)
    want = want[:, :, top:top + h, left:left + w].numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    bound = 255.0 * (T + 8) * 2.0 ** -24
    print(f"max |ref - torch float64| = {err:.3g} grey levels, bound {bound:.3g} (T = {T})")
    assert err <= bound


@pytest.mark.parametrize("shape,resized,origin,out", [((2, 7, 5, 3), (20, 15), (2, 1), (16, 12)),
                                                      ((2, 30, 40, 3), (30, 40), (2, 3), (11, 13)),
                                                      ((1, 9, 9, 4), (9, 12), (0, 0), (9, 12))],
                         ids=lambda v: "x".join(map(str, v)))
def test_reference_without_a_shrinking_axis_is_the_plain_reference(shape, resized, origin, out):
    x = images(shape, seed=41)
    scale, shift = np.float32([0.5, 2, 3, 4][:shape[3]]), np.float32([1, -2, 0.25, 7][:shape[3]])
    np.testing.assert_array_equal(resize_aa_ref(x, resized, origin, out, scale, shift),
                                  resize_ref(x, resized, origin, out, scale, shift))
