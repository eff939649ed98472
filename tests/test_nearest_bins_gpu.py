"""GPU: ore_nearest_bins_f16 / ore_nearest_bins_i8 (csrc/ore_nearest_bins.h, ore_nearest_bins.hip) against include/ore.h's
definition in numpy: the per-bin first of best()'s order, then best() over the winners.  int8 scores are
tests/_nearest_i8.py's; f16 data are integers of |x| <= 8, whose products and f32 sums are exact (64 D < 2^24), so a
float64 matmul gives the bits.  Every comparison is on the bits of the values and on the indices."""
import numpy as np
import pytest
import torch

import ore
from _nearest_i8 import bins_ref, quant, scores

pytestmark = pytest.mark.gpu
NAN = 0x7FC00000


def _given(fmt, seed, n, G, D):
    """(q, gallery, scales or None, scores).  int8: any code, scales 2^-6 .. 2^6, integer queries with a +-127 per row
    (tq = 1); f16: integers in -8 .. 8.  Ties everywhere."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-8, 9, (n, D)).astype(np.float32)
    if fmt == "f16":
        g = rng.integers(-8, 9, (G, D)).astype(np.float16)
        return q, g, None, (q.astype(np.float64) @ g.astype(np.float64).T).astype(np.float32)
    q[np.arange(n), rng.integers(0, D, n)] = rng.choice(np.float32([-127, 127]), n)
    g, t = rng.integers(-128, 128, (G, D)).astype(np.int8), np.exp2(rng.integers(-6, 7, G)).astype(np.float32)
    return q, g, t, scores(*quant(q), g, t)


def _dev(a, off=0):
    """a on the device, `off` elements past a 16-byte boundary"""
    t = torch.empty((off + a.size,), dtype=torch.from_numpy(a).dtype, device="cuda")[off:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == off * a.itemsize
    return t


def _bins(ctx, q, g, t, B, c, goff=0, soff=0):
    qd = q if isinstance(q, torch.Tensor) else _dev(np.ascontiguousarray(q, np.float32))
    v, i = ore.nearest_bins(ctx, qd, _dev(g, goff), c, B, scales=None if t is None else _dev(t, soff))
    torch.cuda.synchronize()
    return v.cpu().numpy().view(np.uint32), i.cpu().numpy()


def _exact(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])


# G of {B (one bin), 4 B - 1, 4 B + 1 (a last bin of one row, wave ranges that are all padding), 4099, 40000 (several
# segments)}; D of {1, 16, 63, 512}, chunked (520 f16, 1040 int8) and odd (element loads); n of one row, a partial tile, two
@pytest.mark.parametrize("fmt, n, G, D, B, c", [
    ("i8", 1, 32, 1, 32, 1), ("f16", 1, 1024, 1, 1024, 1), ("f16", 17, 511, 16, 128, 1), ("i8", 65, 513, 63, 128, 5),
    ("f16", 1, 4097, 63, 1024, 5), ("f16", 65, 4099, 512, 32, 65), ("i8", 17, 4099, 512, 32, 64),
    ("i8", 17, 40000, 1040, 128, 256), ("f16", 17, 40000, 520, 32, 256), ("i8", 65, 40000, 17, 1024, 5)])
def test_given(gpu_ctx, fmt, n, G, D, B, c):
    segments, bins = ore.nearest_bins_segments(gpu_ctx, n, G, B)
    assert bins == -(-G // B) and 1 <= segments <= -(-G // (4 * B))
    if G == 40000:
        assert segments > 1
    q, g, t, s = _given(fmt, n * G + D, n, G, D)
    _exact(_bins(gpu_ctx, q, g, t, B, c), bins_ref(s, B, c))


@pytest.mark.parametrize("collide", [False, True])
def test_collision_by_construction(gpu_ctx, collide, B=128):
    """Scores 10 .. 5 in six rows, every other row 0.  In six bins the five best are the exact search's; with the second
    and the third in one bin the third is absent and the sixth takes the last rank."""
    rows = [700, 130 if collide else 300, 140, 1500, 5, 1100]
    g, q = np.zeros((2048, 16), np.float16), np.zeros((3, 16), np.float32)
    g[rows, 0], q[:, 0] = [10, 9, 8, 7, 6, 5], [1, 2, 3]
    gd = _dev(g)
    v, i = _bins(gpu_ctx, q, g, None, B, 5)
    ev, ei = ore.nearest(gpu_ctx, _dev(q), gd, 5)
    assert ei.cpu().numpy().tolist() == [rows[:5]] * 3
    if collide:
        assert i.tolist() == [rows[:2] + rows[3:]] * 3 and (v.view(np.float32) == np.outer([1, 2, 3], [10, 9, 7, 6, 5])).all()
    else:
        _exact((v, i), (ev.cpu().numpy().view(np.uint32), ei.cpu().numpy()))


@pytest.fixture(scope="module")
def sorted_scores():
    """test_nearest_i8_gpu.test_sorted_gallery's data: the score rises with row // 100, eight distinct queries."""
    j = np.arange(300000)
    codes, q = np.zeros((len(j), 16), np.int8), np.zeros((8, 16), np.float32)
    codes[:, 0], codes[:, 1], codes[:, 2] = j // 10000, j // 100 % 100, j % 100
    q[:, :3] = np.outer(1 + np.arange(8), np.float32([10000, 100, 1]))
    return q, codes, scores(*quant(q), codes, np.ones(len(j), np.float32))


@pytest.mark.parametrize("order", ["rising", "falling"])
@pytest.mark.parametrize("c", [256, 5])
def test_sorted_gallery(gpu_ctx, sorted_scores, order, c, n=65, B=32):
    """The running best is replaced at every row or never, and the radix cut falls among equal images."""
    q, codes, s = sorted_scores
    if order == "falling":
        codes, s = codes[::-1].copy(), s[:, ::-1].copy()
    segments, bins = ore.nearest_bins_segments(gpu_ctx, n, len(codes), B)
    assert -(-bins // (4 * segments)) >= 8, segments  # steps of a wave's range
    want = bins_ref(s, B, c)
    pick = np.arange(n) % 8
    _exact(_bins(gpu_ctx, q[pick], codes, np.ones(len(codes), np.float32), B, c), (want[0][pick], want[1][pick]))


@pytest.mark.parametrize("fmt, qoff, goff", [("i8", 1, 0), ("i8", 0, 1), ("f16", 1, 1), ("i8", 1, 1)])
def test_sliced_misaligned(gpu_ctx, fmt, qoff, goff, D=64):
    """q in a NaN-filled buffer at a row stride of 80, 4 bytes off; the gallery one element off; the scales 4 bytes."""
    q, g, t, s = _given(fmt, 3, 17, 1000, D)
    qd = torch.full((qoff + 17 * 80,), float("nan"), device="cuda")[qoff:].view(17, 80)[:, :D]
    qd.copy_(torch.from_numpy(q))
    assert qd.data_ptr() % 16 == 4 * qoff and qd.stride(0) == 80
    _exact(_bins(gpu_ctx, qd, g, t, 32, 5, goff, 1), bins_ref(s, 32, 5))


def test_non_finite(gpu_ctx, B=32, c=5):
    """A query holding +inf: every score NaN, the winners are the bins' first rows.  A gallery row of NaN scale in a
    finite bin loses to every number, the infinite scores of an infinite scale included."""
    q, g, t, _ = _given("i8", 7, 2, 300, 8)
    q[0, 3], t[[32, 40, 64]] = np.inf, [np.nan, -np.inf, np.nan]
    s = scores(*quant(q), g, t)
    assert np.isnan(s[0]).all() and np.isnan(s[1, [32, 64]]).all()
    v, i = _bins(gpu_ctx, q, g, t, B, c)
    assert i[0].tolist() == [0, 32, 64, 96, 128] and (v[0] == NAN).all() and 32 not in i[1] and 64 not in i[1]
    _exact((v, i), bins_ref(s, B, c))
    _exact(_bins(gpu_ctx, q, g, t, B, 10), bins_ref(s, B, 10))  # every bin: the NaN bins' neighbours and -inf's rank


def test_two_stage(gpu_ctx, n=17, G=40000, D=64, k=5):
    rng = np.random.default_rng(11)
    g32 = rng.standard_normal((G, D)).astype(np.float32)
    q = g32[rng.permutation(G)[:n]] + 0.1 * rng.standard_normal((n, D)).astype(np.float32)
    qd, gd = _dev(q), _dev(g32)
    codes, t = ore.gallery_i8(gpu_ctx, gd)
    cand = bins_ref(scores(*quant(q), codes.cpu().numpy(), t.cpu().numpy()), 128, 128)[1].astype(np.int32)
    got = ore.nearest(gpu_ctx, qd, codes, k, scales=t, rerank=gd, candidates=128, bin_rows=128)
    want, exact = ore.rerank(gpu_ctx, qd, gd, _dev(cand), k), ore.nearest(gpu_ctx, qd, gd, k)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    distinct = [len(set((r // 128).tolist())) == k and set(r.tolist()) <= set(cr.tolist())
                for r, cr in zip(exact[1].cpu().numpy(), cand)]
    # include/ore.h's estimate: a query shares a bin with chance 10 * 128 / 40000 = 3.2 %, three of 17 with about 2 %
    assert sum(distinct) >= n - 2
    for a, b in zip(got, exact):
        assert torch.equal(a.view(torch.int32)[distinct], b.view(torch.int32)[distinct])
    with pytest.raises(ore.OreError, match="candidates = 128 outside"):
        ore.nearest(gpu_ctx, qd, codes, k, scales=t, rerank=gd, candidates=128)
