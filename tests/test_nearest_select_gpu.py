"""GPU: every pass nearest_bins' radix select (nearest_bins_select_kernel, csrc/ore_nearest_bins.hip) can end on, and
the query slabs of nearest_bins_run (csrc/ore_ops.cpp).

The select stops as soon as at most NBS_CAP = 512 keys stand at or above the cut, which random scores reach in its
first or second pass.  tests/_nearest_select.py sets the bits of every score through the int8 scales, so that the select
has to go on to the pass named: the low bytes of the image, the bytes of the complemented row (its top byte on a
gallery past 2^24 rows), 512 survivors exactly, ranks that shrink in three passes.  Which pass an input ends on is
asserted on the numpy reference's winners (select_passes), never read from the kernel.  Every comparison is on the bits
of the values and on the indices."""
import numpy as np
import pytest
import torch

import _nearest_select as sel
import ore
from _nearest_i8 import bins_fast, bins_ref, quant, scores, select_last_shift
from _poison import make_ctx

pytestmark = pytest.mark.gpu


def _bins(ctx, q, g, t, B, c):
    v, i = ore.nearest_bins(ctx, q, g, c, B, scales=t)
    torch.cuda.synchronize()
    return v.cpu().numpy().view(np.uint32), i.cpu().numpy()


def _exact(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])


@pytest.mark.parametrize("variant", sel.VARIANTS)
@pytest.mark.parametrize("name", sel.CASES)
def test_pass(gpu_ctx, name, variant):
    q, codes, t, s, B, ends = sel.build(name, variant)
    win = sel.winners(name, variant)
    qd, gd, td = (torch.from_numpy(np.array(a)).cuda() for a in (q, codes, t))  # the cached arrays are read-only
    for c in sel.CS:
        assert tuple(select_last_shift(k, c) for k in win) == sel.ends_at(ends, c)
        _exact(_bins(gpu_ctx, qd, gd, td, B, c), sel.want(name, variant, c))


def test_query_slabs(n=129, G=8388609, B=32, c=5):
    """The smallest gallery whose winners pass 256 MiB at 128 queries: 262145 bins, the last of one row, slabs of 64, 64
    and 1 queries.  q is a slice at a row stride of 8 of a NaN-filled buffer and query i is pattern i % 5 of five, so
    the rows on either side of a slab's edge differ.  Codes and scales are periodic in the row with periods that are
    no multiple of a bin: scores rise and fall along the gallery and tie across bins; the best stand past row 5 000 000
    and in the last bin.  Pattern 4 is the zero query: 262145 equal scores, the select's deepest input.  Then a call of
    5 bins on the same context, whose buffer is full of the large call's keys."""
    j = np.arange(G)
    codes = np.stack([j % 251 - 125, j // 7 % 17 - 8], 1).astype(np.int8)
    t = np.exp2(j // 1000 % 5 - 2).astype(np.float32)
    t[5_000_000:5_090_000], t[G - 1], codes[G - 1] = 8, 16, (125, 8)  # the best rows: a stretch far out, the last bin's
    pats = np.float32([[127, 1], [-127, 2], [3, 127], [-5, -127], [0, 0]])
    s = scores(*quant(pats), codes, t)
    want = [np.concatenate(r) for r in zip(*(bins_fast(s[p:p + 1], B, c) for p in range(5)))]
    assert (want[1][4] == B * np.arange(c)).all() and want[1][0, 0] == G - 1 and want[1][:4].min() > 5_000_000
    assert all(len(set(v.tolist())) < c - 1 for v in want[0])  # ties at the top
    ctx, stream = make_ctx()
    try:
        assert ore.nearest_bins_segments(ctx, n, G, B)[1] == 262145
        pick = np.arange(n) % 5
        qd = torch.full((n, 8), float("nan"), device="cuda")[:, :2]
        qd.copy_(torch.from_numpy(pats[pick]))
        gd, td = torch.from_numpy(codes).cuda(), torch.from_numpy(t).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            got = _bins(ctx, qd, gd, td, B, c)
            small = _bins(ctx, qd[:, :2], gd[:129], td[:129], B, c)
        _exact(got, (want[0][pick], want[1][pick]))
        _exact(small, bins_ref(s[pick, :129], B, c))
    finally:
        ctx.close()
