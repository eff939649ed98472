"""GPU: ore.rerank (csrc/ore_nearest_rerank.hip) against float64 on integer data, against the bits of ore.nearest on the
same gallery, past 2^32 bytes, on sliced and misaligned operands, and as the second stage of ore.nearest."""
import numpy as np
import pytest
import torch

import ore

pytestmark = pytest.mark.gpu
DTYPES = ["float32", "float16"]


def _dev(a, dtype="float32", off=0):  # a on the device as dtype, `off` elements past a 16-byte boundary
    t = torch.empty((off + a.size,), dtype=getattr(torch, dtype), device="cuda")[off:].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def _bits(v, i):
    torch.cuda.synchronize()
    return v.cpu().numpy().view(np.uint32), i.cpu().numpy()


def _same(got, want):  # (value bits, indices) pairs
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])


def _expect(q, rows, cand, G, k):
    """Stable argsort of -score over the distinct valid candidates in ascending index, padded with (NaN bits, -1)."""
    v, i = np.full((len(q), k), 0x7fc00000, np.uint32), np.full((len(q), k), -1, np.int32)
    for r, c in enumerate(cand):
        valid = np.unique(c[(c >= 0) & (c < G)])
        if valid.size:
            s = np.stack([rows[j] for j in valid]).astype(np.float64) @ q[r].astype(np.float64)
            o = np.argsort(-s, kind="stable")[:k]
            i[r, :o.size], v[r, :o.size] = valid[o], s[o].astype(np.float32).view(np.uint32)
    return v, i


# (n, G, (D for f32, D for f16), C, k, candidates): the load paths, group and chunk boundaries, the chunked query (520);
# the block edges and wave ownership in C; G = 1; a row that is all padding; rows with k - 1 distinct valid candidates
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n, G, D, C, k, how", [
    (1, 1, (1, 1), 1, 1, ""), (5, 1000, (3, 7), 15, 5, ""), (5, 1000, (4, 8), 16, 16, ""), (1, 1000, (17, 9), 17, 1, ""),
    (5, 1000, (33, 33), 64, 64, ""), (1, 1000, (520, 520), 65, 5, ""), (5, 1000, (520, 520), 256, 64, ""),
    (5, 1, (4, 8), 17, 5, ""), (5, 1000, (33, 33), 17, 5, "allpad"), (5, 1000, (17, 9), 64, 5, "short")])
def test_exact_with_ties(gpu_ctx, dtype, n, G, D, C, k, how):
    D = D[dtype == "float16"]
    rng = np.random.default_rng(n * G + D + C)
    q, g = rng.integers(-8, 9, (n, D)).astype(np.float32), rng.integers(-8, 9, (G, D)).astype(np.float32)
    cand = rng.integers(-G // 4 - 1, G + G // 4 + 1, (n, C)).astype(np.int32)  # a fifth below 0, a fifth at G or above
    cand[:, 0] %= G  # one valid row at least
    cand[:, -1], cand[0, C // 2] = cand[:, 0], cand[0, C // 2] if C < 3 else -1  # a repeat in every row, a -1 in the first
    if how == "allpad":
        cand[0] = np.where(np.arange(C) % 2, -1, G + np.arange(C))
    if how == "short":  # k - 1 distinct valid rows per query, each many times, between pads
        pool = np.stack([np.sort(rng.choice(G, k - 1, replace=False)) for _ in range(n)])
        cand = np.where(rng.random((n, C)) < 0.3, -1, np.take_along_axis(pool, rng.integers(0, k - 1, (n, C)), 1)).astype(np.int32)
        cand[:, :k - 1] = pool
    _same(_bits(*ore.rerank(gpu_ctx, _dev(q), _dev(g, dtype), _dev(cand, "int32"), k)), _expect(q, g, cand, G, k))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [5, 512])
def test_bits_of_the_search(gpu_ctx, dtype, D, n=33, G=4099):
    """The search's 64 indices per row, permuted, with 8 pads and 8 repeats (C = 80), come back as it returned them"""
    rng = np.random.default_rng(D)
    q, g = _dev(rng.standard_normal((n, D)).astype(np.float32)), _dev(rng.standard_normal((G, D)).astype(np.float32), dtype)
    wv, wi = _bits(*ore.nearest(gpu_ctx, q, g, 64))
    cand = np.full((n, 80), -1, np.int32)
    for r in range(n):
        pos = rng.permutation(80)
        cand[r, pos[:64]], cand[r, pos[64:72]] = rng.permutation(wi[r]), wi[r, rng.integers(0, 64, 8)]
    for k in (64, 5):
        _same(_bits(*ore.rerank(gpu_ctx, q, g, _dev(cand, "int32"), k)), (wv[:, :k], wi[:, :k]))


@pytest.mark.parametrize("dtype, G", [("float32", 2_100_000), ("float16", 4_200_000)])
def test_rows_past_4_gib(gpu_ctx, dtype, G, D=520):
    """A gallery past 2^32 bytes, zeros but for integer rows below and above that mark: the row offset is 64-bit."""
    first = 2**32 // (D * (4 if dtype == "float32" else 2)) + 1  # the first row that lies wholly above the mark
    rng = np.random.default_rng(G)
    idx = np.array([0, 5, 1000, first, first + 1, first + 7, G - 2, G - 1])
    rows, q = dict(zip(idx.tolist(), rng.integers(-8, 9, (idx.size, D)).astype(np.float32))), rng.integers(-8, 9, (2, D)).astype(np.float32)
    g = torch.zeros((G, D), dtype=getattr(torch, dtype), device="cuda")
    g[torch.from_numpy(idx).cuda()] = _dev(np.stack([rows[j] for j in idx.tolist()]), dtype)
    cand = np.stack([np.append(idx, -1), np.append(idx[::-1], G)]).astype(np.int32)
    _same(_bits(*ore.rerank(gpu_ctx, _dev(q), g, _dev(cand, "int32"), 8)), _expect(q, rows, cand, G, 8))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sliced_misaligned_inputs(gpu_ctx, dtype, n=5, G=1000, D=40, C=20, k=5):
    """q a slice of a NaN-filled buffer, the gallery one element past a 16-byte boundary, the candidates a column slice"""
    rng = np.random.default_rng(7)
    q, g = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((G, D)).astype(np.float32)
    cand = rng.integers(-3, G + 3, (n, C)).astype(np.int32)
    want = _bits(*ore.rerank(gpu_ctx, _dev(q), _dev(g, dtype), _dev(cand, "int32"), k))
    qd = torch.full((1 + n * 80,), float("nan"), device="cuda")[1:].view(n, 80)[:, :D]
    qd.copy_(torch.from_numpy(q))
    wide = _dev(rng.integers(G, 2**31 - 1, (n, C + 7)).astype(np.int32) * rng.choice([-1, 1], (n, C + 7)).astype(np.int32), "int32")
    wide[:, 3:3 + C] = torch.from_numpy(cand).cuda()
    gd = _dev(g, dtype, off=1)
    assert qd.data_ptr() % 16 == 4 and gd.data_ptr() % 16 in (2, 4) and wide[:, 3:3 + C].stride(0) == C + 7
    _same(_bits(*ore.rerank(gpu_ctx, qd, gd, wide[:, 3:3 + C], k)), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_stage_nearest(gpu_ctx, dtype, n=17, G=4099, D=64):
    rng = np.random.default_rng(11)
    q, g32 = _dev(rng.standard_normal((n, D)).astype(np.float32)), _dev(rng.standard_normal((G, D)).astype(np.float32))
    codes, s = ore.gallery_i8(gpu_ctx, g32)
    gr = g32 if dtype == "float32" else ore.gallery_f16(gpu_ctx, g32)
    v, i = ore.nearest(gpu_ctx, q, codes, 5, scales=s, rerank=gr, candidates=32)
    gv, gi = _bits(v, i)
    _same((gv, gi), _bits(*ore.rerank(gpu_ctx, q, gr, ore.nearest(gpu_ctx, q, codes, 32, scales=s)[1], 5)))
    assert (gi >= 0).all()
    for r in range(n):  # the search of the rerank gallery's five returned rows: the same values (bits of two rows alone)
        sv, si = _bits(*ore.nearest(gpu_ctx, q[r:r + 1], gr[i[r].long()].contiguous(), 5))
        _same((sv[0], gi[r][si[0]]), (gv[r], gi[r]))
