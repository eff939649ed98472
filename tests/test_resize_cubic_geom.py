"""CPU: the cubic filters' taps (ore_resize_cubic_taps, the table the kernels use) against the brute-force definition
and the numpy restatement (_resize_cubic_ref.py), and the restatement against torch's bicubic interpolation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ore
from _resize_cubic_ref import cubic_aa_taps_ref, cubic_taps_ref, resize_cubic_ref

GRID = range(1, 81)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_aa_axis(S, D):
    first, ntaps, weights, total = ore.resize_cubic_taps(S, D, 0, D, antialias=True)
    ref = cubic_aa_taps_ref(S, D, 0, D)
    cap = min(64, -(-4 * max(S, D) // D))  # the bound the launches size their weight table by
    for o, (f, w, W) in enumerate(ref):
        assert (first[o], ntaps[o]) == (f, len(w)), (S, D, o)
        assert 1 <= len(w) <= cap and f + len(w) <= S, (S, D, o)
        assert np.array_equal(_bits(weights[o, :len(w)]), _bits(w)), (S, D, o)
        assert not weights[o, len(w):].any()
        assert _bits(total[o:o + 1])[0] == _bits(np.array([W]))[0], (S, D, o)
    return int(ntaps.max())


def test_aa_runs_equal_brute_force_on_the_grid():
    """Closed-form first tap and count, the weights and their sum, for every resized index of every S, D in 1..80
    with S <= 16 D; an axis that does not shrink has at most 4 taps."""
    for S in GRID:
        for D in GRID:
            if S > 16 * D:
                continue
            n = _check_aa_axis(S, D)
            if S <= D:
                assert n <= 4, (S, D)


@pytest.mark.parametrize("S,D", [(16384, 1024), (1024, 16384), (16, 1), (80, 5), (1600, 100), (16383, 1024), (15, 1), (1, 16384)])
def test_aa_runs_at_the_extremes(S, D):
    n = _check_aa_axis(S, D)
    assert n <= 64
    if S == 16 * D and D > 4:
        assert n == 64  # an interior run at ratio exactly 16 is full


def test_plain_taps_equal_the_restatement():
    for S in GRID:
        for D in GRID:
            first, ntaps, weights, total = ore.resize_cubic_taps(S, D, 0, D)
            f, w = cubic_taps_ref(S, D, 0, D)
            assert np.array_equal(first, f) and (ntaps == 4).all() and (total == 1.0).all(), (S, D)
            assert np.array_equal(_bits(weights[:, :4]), _bits(w)), (S, D)
            assert not weights[:, 4:].any()
            assert first.min() >= -2 and first.max() <= S - 2
    # 16384 -> 1 has no ratio rule; a window with an origin
    first, ntaps, weights, total = ore.resize_cubic_taps(16384, 1, 0, 1)
    assert first[0] == 8190 and ntaps[0] == 4
    first, _, weights, _ = ore.resize_cubic_taps(37, 91, 50, 30)
    f, w = cubic_taps_ref(37, 91, 50, 30)
    assert np.array_equal(first, f) and np.array_equal(_bits(weights[:, :4]), _bits(w))
    # growing far enough that the first coordinate lies below -1/2: the floor is -1
    first, _, _, _ = ore.resize_cubic_taps(2, 9, 0, 9)
    assert first[0] == -2


def test_identity_weights():
    """S == D: the plain weights are (0, 1, 0, 0) and the antialiased run is a single 1 among zeros, sum 1, exactly."""
    for S in (1, 2, 3, 7, 80, 16384):
        n = min(S, 200)
        first, ntaps, weights, total = ore.resize_cubic_taps(S, S, S - n, n)
        assert np.array_equal(first, np.arange(S - n, S) - 1)
        assert np.array_equal(_bits(weights[:, :4]), _bits(np.tile(np.float32([0, 1, 0, 0]), (n, 1))))
        first, ntaps, weights, total = ore.resize_cubic_taps(S, S, S - n, n, antialias=True)
        assert np.array_equal(_bits(total), _bits(np.ones(n, np.float32)))
        for i in range(n):
            o = S - n + i
            w = weights[i, :ntaps[i]]
            assert w[o - first[i]] == 1.0 and np.count_nonzero(w) == 1, (S, o)
            assert not np.signbit(w).any()


def test_identity_returns_the_bytes():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (2, 12, 20, 3), dtype=np.uint8)
    want = np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32)
    for aa in (False, True):
        assert np.array_equal(resize_cubic_ref(x, (12, 20), (0, 0), (12, 20), aa), want)
        assert np.array_equal(resize_cubic_ref(x, (12, 20), (3, 5), (4, 6), aa), want[:, :, 3:7, 5:11])


# (source hw, resized hw, origin, out hw): the six geometries whole, then windows with a non-zero origin
TORCH_CASES = [((13, 17), (9, 23), (0, 0), (9, 23)), ((7, 5), (7, 5), (0, 0), (7, 5)), ((31, 40), (8, 11), (0, 0), (8, 11)),
               ((5, 6), (20, 3), (0, 0), (20, 3)), ((64, 33), (4, 33), (0, 0), (4, 33)), ((1, 9), (3, 4), (0, 0), (3, 4)),
               ((13, 17), (9, 23), (2, 5), (6, 11)), ((31, 40), (8, 11), (3, 4), (5, 7)), ((5, 6), (20, 3), (9, 1), (11, 2)),
               ((64, 33), (4, 33), (1, 20), (3, 13))]
# 4 x the largest difference measured over TORCH_CASES (see the docstring below)
TORCH_BOUND = {False: 4 * 2.97e-4, True: 4 * 9.6e-5}


@pytest.mark.parametrize("aa", [False, True])
def test_restatement_against_torch_float64(aa):
    """The float32 restatement against F.interpolate(mode="bicubic", align_corners=False, antialias=aa) in float64
    on bytes 0..255.  Measured max abs difference over TORCH_CASES: 2.97e-4 plain, 9.6e-5 antialiased (torch's own
    float32 sits up to 1.5 x that from its float64, hence a bound of 4 x the measured value)."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for (hs, ws), (rh, rw), (top, left), (h, w) in TORCH_CASES:
        x = rng.integers(0, 256, (2, hs, ws, 3), dtype=np.uint8)
        got = resize_cubic_ref(x, (rh, rw), (top, left), (h, w), aa)
        t = torch.from_numpy(x).permute(0, 3, 1, 2).to(torch.float64)
        ref = F.interpolate(t, size=(rh, rw), mode="bicubic", align_corners=False, antialias=aa)
        ref = ref[:, :, top:top + h, left:left + w].numpy()
        worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
    print(f"restatement vs torch float64, antialias={aa}: max abs {worst:.3g}")
    assert worst <= TORCH_BOUND[aa]
