"""GPU: ore_nearest_f16 and ore_gallery_f16 (csrc/ore_nearest_f16.hip) against float64 matmuls of the f16-rounded
operands, np.argsort(kind="stable") and astype(np.float16)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _nearest(ctx, q, g, k, off=0):
    import torch
    import ore
    qd = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    gd = torch.empty((off + g.size,), dtype=torch.float16, device="cuda")[off:].view(g.shape)
    gd.copy_(torch.from_numpy(g.astype(np.float16)))
    assert gd.data_ptr() % 16 == 2 * off
    v, i = ore.nearest(ctx, qd, gd, k)
    torch.cuda.synchronize()
    return v.cpu().numpy(), i.cpu().numpy()


def _exact(ctx, q, g, k, qd=None, off=0):
    s = q.astype(np.float64) @ g.astype(np.float64).T
    want, (v, i) = np.argsort(-s, axis=1, kind="stable")[:, :k], _nearest(ctx, q if qd is None else qd, g, k, off)
    np.testing.assert_array_equal(i, want)
    np.testing.assert_array_equal(v.astype(np.float64), np.take_along_axis(s, want, 1))


def _ints(seed, n, G, D):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (n, D)).astype(np.float32), rng.integers(-8, 9, (G, D)).astype(np.float32)


# (n, G, D, k): every D of {1, 7, 8, 9, 33, 520} and 513 (one past the resident tile, two chunks), n of {1, 15, 17, 65},
# G of {1, step - 1, step + 1, 1000, 4099} and k of {1, 5, min(G, 64)} at least once; D = 1025 is three chunks of the
# staged tile (512 + 512 + 1) on 2-byte gallery loads, every sum at most 64 * 1025 < 2^24; the last on several segments
@pytest.mark.parametrize("n, G, D, k", [(1, 1, 1, 1), (15, 127, 7, 64), (17, 129, 8, 5), (65, 1000, 9, 64), (17, 4099, 33, 1),
                                        (1, 1000, 520, 5), (15, 4099, 513, 64), (65, 129, 520, 1), (17, 1000, 1025, 5),
                                        (65, 40000, 8, 5)])
def test_exact_with_ties(gpu_ctx, n, G, D, k):
    import ore
    segments, step = ore.nearest_segments_f16(gpu_ctx, n, G)
    steps = (G + step - 1) // step
    assert step == 128 and 1 <= segments <= steps  # the cases' 127 and 129 are step - 1 and step + 1
    if G == 40000:  # a merge launch, and ceil(steps / segments) >= 2 steps per workgroup (the last takes the rest of 313)
        assert segments > 1 and -(-steps // segments) >= 2, segments
    _exact(gpu_ctx, *_ints(n * G + D, n, G, D), k)


@pytest.mark.parametrize("order", ["rising", "falling"])
@pytest.mark.parametrize("k", [5, 64])
def test_sorted_gallery(gpu_ctx, order, k):
    """test_nearest_gpu.py's construction, every operand exact in f16: row j is (j // 1024, j % 1024, 0 ...), query i is
    c (1024, 1, 0 ...), c = 1 + i % 8, the score c j < 2^22.  Two query tiles: a workgroup walks eight steps or more."""
    import ore
    n, G, D = 65, 300000, 8 if k == 64 else 3  # 16-byte and 2-byte gallery loads
    segments, step = ore.nearest_segments_f16(gpu_ctx, n, G)
    assert (G + step - 1) // step >= 8 * segments, segments
    j = np.arange(G) if order == "rising" else np.arange(G)[::-1]
    g, q = np.zeros((G, D), np.float32), np.zeros((n, D), np.float32)
    g[:, 0], g[:, 1] = j // 1024, j % 1024
    q[:, 0], q[:, 1] = 1024 * (1 + np.arange(n) % 8), 1 + np.arange(n) % 8
    _exact(gpu_ctx, q, g, k)


@pytest.mark.parametrize("D", [40, 67])
def test_sliced_misaligned_queries(gpu_ctx, D):
    """q as rows of a wider NaN-filled buffer at nstride 80 > D, the gallery 2 bytes past a 16-byte boundary."""
    import torch
    q, g = _ints(3, 17, 1000, D)
    qd = torch.full((1 + 17 * 80,), float("nan"), device="cuda")[1:].view(17, 80)[:, :D]
    qd.copy_(torch.from_numpy(q))
    assert qd.data_ptr() % 16 == 4 and qd.stride(0) == 80
    _exact(gpu_ctx, q, g, 5, qd, off=1)


@functools.lru_cache(maxsize=None)
def _normal(D, n=33, G=4099):
    rng = np.random.default_rng(D)
    q, g = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((G, D)).astype(np.float32)
    q64, g64 = q.astype(np.float16).astype(np.float64), g.astype(np.float16).astype(np.float64)
    return q, g, q64 @ g64.T, 2e-6 * (np.abs(q64) @ np.abs(g64).T)


@pytest.mark.parametrize("D", [5, 512])
def test_against_float64(gpu_ctx, D, k=5):
    """b[i, j] = 2e-6 sum_d |q^ g^|: include/ore.h's accumulation contract of the f16 matrix cores."""
    q, g, s64, b = _normal(D)
    v, i = _nearest(gpu_ctx, q, g, k)
    err = np.abs(v - np.take_along_axis(s64, i, 1))
    print(f"D = {D}: max err / bound = {(err / np.take_along_axis(b, i, 1)).max():.3g}")
    assert (err <= np.take_along_axis(b, i, 1)).all()
    assert all(len(set(r)) == k for r in i) and (np.diff(v, axis=1) <= 0).all(), "indices repeat or values increase in a row"
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


@pytest.mark.parametrize("D", [8, 7])  # 16-byte loads and stores; one element per thread
def test_packer(gpu_ctx, D):
    """Halfway cases to even (1 + 2^-11, 1 + 3 2^-11, 65520: inf, 2^-25: 0), 65504, subnormals and values below them."""
    import torch
    import ore
    a = np.float32([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504, 65519.996, 65520, 1e6, 2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25,
                    1.5 * 2.0 ** -25, 1e-10, 0.0, np.inf, 1 / 3, 1000.5])
    x = np.resize(np.concatenate([a, -a, np.float32([np.nan])]), (37, D))
    got = ore.gallery_f16(gpu_ctx, torch.from_numpy(x).cuda())
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint16), x.astype(np.float16).view(np.uint16))


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
    v, i = _nearest(gpu_ctx, np.float32([[1e6, 1]]), np.float32([[1, 0], [0, 1], [-1, 0]]), 3)  # 1e6 -> inf; inf 0 = NaN last
    assert (i == [0, 2, 1]).all() and np.isposinf(v[0, 0]) and np.isneginf(v[0, 1]) and v.view(np.uint32)[0, 2] == 0x7fc00000
