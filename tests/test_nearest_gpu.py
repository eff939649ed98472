"""GPU: ore_nearest_f32 (csrc/ore_nearest.hip) against a float64 matmul and np.argsort(kind="stable"): exact on
integer data with ties, within the derived f32 bound on normal data, bit for bit under a permutation of the gallery
and a smaller batch, and the special values of the order."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _nearest(ctx, q, g, k):
    import torch
    import ore
    qd = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    v, i = ore.nearest(ctx, qd, torch.from_numpy(np.ascontiguousarray(g, np.float32)).cuda(), k)
    torch.cuda.synchronize()
    return v.cpu().numpy(), i.cpu().numpy()


def _exact(ctx, q, g, k, qd=None):
    s = q.astype(np.float64) @ g.astype(np.float64).T
    want = np.argsort(-s, axis=1, kind="stable")[:, :k]
    v, i = _nearest(ctx, q if qd is None else qd, g, k)
    np.testing.assert_array_equal(i, want)
    np.testing.assert_array_equal(v.astype(np.float64), np.take_along_axis(s, want, 1))


def _ints(seed, n, G, D):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (n, D)).astype(np.float32), rng.integers(-8, 9, (G, D)).astype(np.float32)


# (n, G, D, k): every D of {1, 3, 4, 5, 67, 512}, n of {1, 15, 17, 65}, G of {1, 15, 17, 63, 65, 1000, 4099} and
# k of {1, 5, min(G, 64)} at least once; the last case runs on several segments of several steps each
@pytest.mark.parametrize("n, G, D, k", [(1, 1, 1, 1), (15, 15, 3, 15), (17, 17, 4, 5), (65, 63, 5, 63), (17, 65, 67, 64),
                                        (1, 1000, 512, 5), (65, 4099, 67, 64), (15, 4099, 512, 1), (17, 1000, 5, 64),
                                        (65, 40000, 8, 5)])
def test_exact_with_ties(gpu_ctx, n, G, D, k):
    import ore
    segments = ore.nearest_segments(gpu_ctx, n, G)
    assert 1 <= segments <= (G + 63) // 64
    if G == 40000:
        assert 1 < segments <= (G + 63) // 64 // 2, segments  # a merge launch, and two steps or more per workgroup
    _exact(gpu_ctx, *_ints(n * G + D, n, G, D), k)


@pytest.mark.parametrize("order", ["rising", "falling"])
@pytest.mark.parametrize("k", [5, 64])
def test_sorted_gallery(gpu_ctx, order, k):
    """Every workgroup walks eight steps or more.  Scores that rise strictly with the index bring 64 survivors per
    query and step, so every query is compacted at every step and its threshold rises each time; falling ones
    compact in a segment's first step only.  Row j is (j // 1024, j % 1024, 0 ...) and query i is c (1024, 1, 0 ...)
    with c = 1 + i % 8: the score c j < 2^22 and both products are integers, exact in f32."""
    import ore
    n, G, D = 17, 300000, 4 if k == 64 else 3  # 16-byte and 4-byte gallery loads
    segments = ore.nearest_segments(gpu_ctx, n, G)
    assert (G + 63) // 64 >= 8 * segments, segments
    j = np.arange(G) if order == "rising" else np.arange(G)[::-1]
    g, q = np.zeros((G, D), np.float32), np.zeros((n, D), np.float32)
    g[:, 0], g[:, 1] = j // 1024, j % 1024
    q[:, 0], q[:, 1] = 1024 * (1 + np.arange(n) % 8), 1 + np.arange(n) % 8
    _exact(gpu_ctx, q, g, k)


def test_sliced_misaligned_queries(gpu_ctx):
    """q as rows of a wider NaN-filled buffer, 4 bytes past a 16-byte boundary: nstride 80 > D = 67."""
    import torch
    q, g = _ints(3, 17, 1000, 67)
    buf = torch.full((1 + 17 * 80,), float("nan"), device="cuda")
    qd = buf[1:].view(17, 80)[:, :67]
    qd.copy_(torch.from_numpy(q))
    assert qd.data_ptr() % 16 == 4 and qd.stride(0) == 80
    _exact(gpu_ctx, q, g, 5, qd)


@functools.lru_cache(maxsize=None)
def _normal(D, n=33, G=4099):
    rng = np.random.default_rng(D)
    q, g = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((G, D)).astype(np.float32)
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    return q, g, q64 @ g64.T, D * 2.0 ** -24 * (np.abs(q64) @ np.abs(g64).T)


@pytest.mark.parametrize("D", [5, 512])
def test_against_float64(gpu_ctx, D, k=5):
    """b[i, j] = D 2^-24 sum_d |q g|: the bound of an f32 sum of D products, each within half an ulp, in any order."""
    q, g, s64, b = _normal(D)
    v, i = _nearest(gpu_ctx, q, g, k)
    err = np.abs(v - np.take_along_axis(s64, i, 1))
    print(f"D = {D}: max err / bound = {(err / np.take_along_axis(b, i, 1)).max():.3g}")
    assert (err <= np.take_along_axis(b, i, 1)).all()
    assert all(len(set(r)) == k for r in i), "indices repeat within a row"
    assert (np.diff(v, axis=1) <= 0).all(), "values increase along a row"
    assert (np.sort(s64, axis=1)[:, -k] <= v[:, k - 1] + b.max(axis=1)).all(), "a row misses a score by more than the bound"


@pytest.mark.parametrize("D", [5, 512])
def test_position_independence(gpu_ctx, D, k=5):
    q, g, s64, _ = _normal(D)
    top = -np.sort(-s64, axis=1)[:, :k + 1]
    assert (np.diff(top, axis=1) < 0).all(), "the input has a float64 tie at rank k"
    v, i = _nearest(gpu_ctx, q, g, k)
    perm = np.random.default_rng(1).permutation(len(g))
    vp, ip = _nearest(gpu_ctx, q, g[perm], k)
    v7, i7 = _nearest(gpu_ctx, q[:7], g, k)
    np.testing.assert_array_equal(vp.view(np.uint32), v.view(np.uint32))
    np.testing.assert_array_equal(perm[ip], i)
    np.testing.assert_array_equal(v7.view(np.uint32), v[:7].view(np.uint32))
    np.testing.assert_array_equal(i7, i[:7])


def test_special_values(gpu_ctx):
    q, g = _ints(4, 3, 17, 5)
    q = np.abs(q) + 1
    g[3, 2], g[5] = np.nan, np.inf
    v, i = _nearest(gpu_ctx, q, g, 17)
    assert (i[:, -1] == 3).all() and np.isnan(v[:, -1]).all() and not np.isnan(v[:, :-1]).any()  # the NaN row last
    assert (i[:, 0] == 5).all() and np.isposinf(v[:, 0]).all()                                # the +inf row first
    v, i = _nearest(gpu_ctx, np.zeros((2, 5), np.float32), _ints(5, 1, 65, 5)[1], 5)          # a zero query
    assert (i == np.arange(5)).all() and (v.view(np.uint32) == 0).all()
    v, i = _nearest(gpu_ctx, np.ones((1, 1), np.float32), np.float32([[-0.0], [0.0], [-0.0], [0.0], [-1.0]]), 4)
    assert (i == np.arange(4)).all() and (v == 0).all()                                      # -0 ties with +0 by index
