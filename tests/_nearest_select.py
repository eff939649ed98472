"""Inputs that take nearest_bins' radix select (csrc/ore_nearest_bins.hip) through every pass it can end on, shared by
tests/test_nearest_select_ref.py (numpy alone) and tests/test_nearest_select_gpu.py.

int8 galleries of D = 2 whose every row is (1, 1).  The query (127, 1) has the codes (127, 1) and the scale 1, so a
row's score is 128 t_j, exact: the scales set the 32 bits of every score, t = (bits - (7 << 23)).view(float32).  Three
queries: that one; its negation, whose scores are negative (the flipped-bit branch of the image, and the order of the
bins reversed); and one holding +inf, whose every score is a NaN (image 0: the complemented rows alone decide).

A bin gets one chosen score.  Variant "same": all its rows have it, so the bin's winner is decided by the row.
Variant "one": one row has it, at a place that moves with the bin, and the others have a NaN scale, which loses to
every number under either sign of the query (a smaller scale would win the negated query), so the running best is
replaced in the middle of a bin."""
import functools

import numpy as np

from _nearest_i8 import bin_winners, bins_fast, bins_ref, quant, scores

ONE = 0x3F800000
QUERIES = np.float32([[127, 1], [-127, -1], [np.inf, 1]])


def _perm(NB, seed):
    return np.random.default_rng(seed).permutation(NB)


def _want3(NB):
    """Score bits of the case whose ranks still wanted shrink in three passes at c = 256: 29 bins one step up in the
    second byte, 100 bins in the top bucket of the third byte below them, the rest six to an image under it."""
    r = np.arange(NB)
    bits = np.where(r < 29, 0x10000 + r, np.where(r < 129, 0xFF00 + (r - 29), 0xFE00 + (r - 129) // 6))
    return ONE + bits[_perm(NB, 5)]


def _want_cut(NB):
    """Score bits of the case in which the ranks wanted after a pass decide the next cut bucket: 200 bins one step up in
    the second byte, 200 in the top bucket of the third byte below them and the rest six to an image under it.  At
    c = 256 the 56 ranks left after the second byte end the select in those 200; with 256 still wanted it would go on
    into the bucket of 1101."""
    r = np.arange(NB)
    bits = np.where(r < 200, 0x10000 + r, np.where(r < 400, 0xFF00 + (r - 200), 0xFE00 + (r - 400) // 6))
    return ONE + bits[_perm(NB, 6)]


LOW24 = (1 << 24) // 32  # the bins of 32 rows below row 2^24


def _shift24(NB):
    """Score bits of the case that ends on the top byte of the complemented row: a gallery past 2^24 rows, all bins one
    image but 600 above it -- 300 below row 2^24, every 1747th bin, and 300 of the 600 bins past it -- and 600 under it,
    400 below row 2^24 and 200 past it.  More than 512 keys share the top image (the lowest, for the negated query), so
    the image's passes end nothing, and the byte at shift 24 splits them 300 : 300 (400 : 200)."""
    r = np.arange(NB)
    h = r - LOW24
    bits = np.full(NB, ONE + 1)
    bits[((r < LOW24) & (r % 1301 == 5) & (r // 1301 < 400)) | ((h >= 0) & (h % 2 == 1) & (h < 400))] = ONE
    bits[((r < LOW24) & (r % 1747 == 0) & (r // 1747 < 300)) | ((h >= 0) & (h % 2 == 0))] = ONE + 2
    return bits


# name: (B, NB, rows the last bin lacks, score bits per bin, the shift the select ends on per query -- per c where it
# depends on c)
CASES = {
    # one top byte; 256 keys to a bucket of the second byte
    "shift48": (32, 1501, 5, lambda NB: ONE + (_perm(NB, 1) << 8), (48, 48, 8)),
    # the same in the third byte
    "shift40": (32, 1501, 5, lambda NB: ONE + _perm(NB, 2), (40, 40, 8)),
    # two buckets of 1024 in the third byte, four bins to an image: the cut falls inside a tie class
    "shift32": (32, 2048, 5, lambda NB: ONE + _perm(NB, 4) // 4, (32, 32, 8)),
    # the 29 bins end c <= 29 at shift 48 for the first query; the negated query has the bins six to an image on top
    "want3": (32, 1501, 5, _want3, {1: (48, 32, 8), 5: (48, 32, 8), 256: (32, 32, 8)}),
    "want_cut": (32, 1501, 5, _want_cut, {1: (48, 32, 8), 5: (48, 32, 8), 256: (40, 32, 8)}),
    # all scores equal: the rows alone, 8 bins to a bucket of the byte at shift 8, 2048 to one at shift 16
    "shift8": (32, 2100, 0, lambda NB: np.full(NB, ONE), (8, 8, 8)),
    # all scores equal and B = 128: the 512 bins below row 65536 fill the cut bucket at shift 16 -- NBS_CAP exactly
    "shift16_cap": (128, 1000, 0, lambda NB: np.full(NB, ONE), (16, 16, 16)),
    # past 2^24 rows: the byte of ~row at shift 24 takes two values
    "shift24": (32, LOW24 + 600, 5, _shift24, (24, 24, 8)),
}
LARGE = ("shift24",)  # too many bins for an argsort per bin: bins_fast() is the reference
VARIANTS = ("same", "one")
CS = (1, 5, 256)


def ends_at(ends, c):
    return ends[c] if isinstance(ends, dict) else ends


@functools.lru_cache(maxsize=4)  # shift24 is 300 MB a variant: the cases run one after the other
def build(name, variant):
    """(q [3, 2] float32, codes [G, 2] int8, scales [G] float32, scores [3, G] float32, B, ends)"""
    B, NB, lack, bits, ends = CASES[name]
    G = B * NB - lack
    t = (np.repeat(bits(NB).astype(np.uint32), B)[:G] - np.uint32(7 << 23)).view(np.float32).copy()
    if variant == "one":
        j = np.arange(G)
        rows = np.minimum(B, G - j // B * B)  # the rows of j's bin
        t[j % B != (7 * (j // B) + 3) % rows] = np.nan
    codes = np.ones((G, 2), np.int8)
    s = scores(*quant(QUERIES), codes, t)
    for arr in (t, codes, s):
        arr.setflags(write=False)
    return QUERIES, codes, t, s, B, ends


@functools.lru_cache(maxsize=4)
def winners(name, variant):
    """bin_winners() of the case's scores, uint64 [3, NB]"""
    w = bin_winners(build(name, variant)[3], build(name, variant)[4])
    w.setflags(write=False)
    return w


def want(name, variant, c):
    """The reference's (value bits, indices) of the case at c"""
    s, B = build(name, variant)[3:5]
    return bins_fast(s, B, c, winners(name, variant)) if name in LARGE else bins_ref(s, B, c)
