"""CPU: the numpy side of tests/test_nearest_select_gpu.py and of the slab case.  image() and keys() restate
ore_topk_key.h; here the c largest keys by np.sort are held against bins_ref(), which never sees a key, and every input
of tests/_nearest_select.py is shown, by select_passes() on the reference's winners, to end the radix select on the pass
it is meant for."""
import numpy as np
import pytest

import _nearest_select as sel
from _nearest_i8 import bin_winners, bins_fast, bins_ref, image, keys, quant, scores, select_last_shift, select_passes


def test_image():
    x = np.float32([np.nan, -np.nan, -np.inf, -1, -2.0 ** -149, -0.0, 0.0, 2.0 ** -149, 1, np.inf])
    assert image(x).tolist() == [0, 0, 0x007FFFFF, 0x407FFFFF, 0x7FFFFFFE, 0x80000000, 0x80000000, 0x80000001,
                                 0xBF800000, 0xFF800000]
    assert keys(np.float32([1, np.nan]), [0, 2 ** 31 - 1]).tolist() == [0xBF800000FFFFFFFF, 0x80000000]


@pytest.mark.parametrize("seed", [0, 1])
def test_keys_order_is_bins_ref(seed, n=5, G=1000, B=32):
    """Random int8 scores with ties, NaNs, infinities of both signs and both zeros, a last bin of eight rows"""
    rng = np.random.default_rng(seed)
    q = rng.integers(-8, 9, (n, 4)).astype(np.float32)
    q[:, 0] = 127
    t = np.exp2(rng.integers(-2, 3, G)).astype(np.float32)
    t[rng.integers(0, G, 60)] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0]), 60)
    t[32:64], t[64:96] = np.nan, 0.0  # an all-NaN bin, and a bin of zeros of either sign
    s = scores(*quant(q), rng.integers(-3, 4, (G, 4)).astype(np.int8), t)
    for c in (1, 5, 32):
        for got, want in zip(bins_fast(s, B, c), bins_ref(s, B, c)):
            np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("variant", sel.VARIANTS)
@pytest.mark.parametrize("name", sel.CASES)
def test_construction(name, variant):
    q, codes, t, s, B, ends = sel.build(name, variant)
    win = sel.winners(name, variant)
    assert len(np.unique(win[0])) == win.shape[1] and win.min() > 0
    desc = np.sort(win, axis=1)[:, ::-1][:, :max(sel.CS)]
    for c in sel.CS:
        assert tuple(select_last_shift(k, c) for k in win) == sel.ends_at(ends, c), (name, variant, c)
        if name not in sel.LARGE:  # there the keys are the reference: test_keys_order_is_bins_ref
            v, i = bins_ref(s, B, c)
            np.testing.assert_array_equal(~desc[:, :c].astype(np.uint32), i.astype(np.uint32))
            np.testing.assert_array_equal(desc[:, :c] >> np.uint64(32), image(v.view(np.float32)))
    if variant == "same":
        assert (sel.want(name, variant, 5)[1][2] == B * np.arange(5)).all()  # the NaN query: the bins' first rows


def test_cap_is_met_exactly():
    """shift16_cap: the pass at shift 16 leaves 512 keys, NBS_CAP, and the passes above it all 1000"""
    for variant in sel.VARIANTS:
        s, B = sel.build("shift16_cap", variant)[3:5]
        for k in bin_winners(s, B):
            for c in sel.CS:
                assert [p[2] for p in select_passes(k, c)] == [1000] * 5 + [512]
                assert select_last_shift(k, c, cap=511) == 8


def test_wanted_ranks_shrink_in_three_passes():
    """want3 at c = 256: keys rise above the cut at shifts 48, 40 and 32, and the passes between do not end it"""
    s, B = sel.build("want3", "same")[3:5]
    # at shift 32 the top bucket holds 4 bins and 20 more hold 6 each above the cut's
    assert select_passes(bin_winners(s, B)[0], 256) == [(56, 0, 1501), (48, 29, 1501), (40, 100, 1501), (32, 124, 259)]


def test_wanted_ranks_decide_the_cut():
    """want_cut at c = 256: 200 keys rise above the cut at shift 48, and the 56 ranks left end the select at shift 40"""
    s, B = sel.build("want_cut", "one")[3:5]
    assert select_passes(bin_winners(s, B)[0], 256) == [(56, 0, 1501), (48, 200, 1501), (40, 0, 400)]


def test_row_top_byte_ends_a_select():
    """shift24: 600 keys of the best image pass the image's four passes together, and the top byte of the complemented
    row parts them into the 300 (for the negated query 400) below row 2^24 and the rest"""
    for variant in sel.VARIANTS:
        win = sel.winners("shift24", variant)
        for c in sel.CS:
            for k, low in zip(win[:2], (300, 400)):
                assert select_passes(k, c)[3:] == [(32, 0, 600), (24, 0, low)]


def test_passes_covered():
    """The constructions end on every pass but the last, which ends no select: when the pass at shift 8 has run, its cut
    bucket holds the bins of 256 consecutive rows, at most 8 -- shown on the inputs that get that far."""
    ends = {e for case in sel.CASES.values() for c in sel.CS for e in sel.ends_at(case[4], c)}
    assert ends == {48, 40, 32, 24, 16, 8}
    for name in ("shift8", "shift48"):
        for k in sel.winners(name, "one"):
            for c in sel.CS:
                passes = select_passes(k, c)
                if passes[-1][0] == 8:
                    assert 1 <= passes[-1][2] - sum(p[1] for p in passes) <= 8
