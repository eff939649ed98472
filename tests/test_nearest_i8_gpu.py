"""GPU: ore_nearest_i8 and ore_gallery_i8 (csrc/ore_nearest_i8.hip) against tests/_nearest_i8.py, the numpy
restatement of include/ore.h's definition.  The dot product is an exact integer, so every comparison is on the bits."""
import numpy as np
import pytest
import torch

import ore
from _nearest_i8 import best, normal, quant, scores

pytestmark = pytest.mark.gpu
EDGE_ROWS = [[0.0], [np.nan, 1, -2], [np.inf, 1, -2], [1e-40, 0, -1e-40], [127, 0.5, -0.5, 1.5, -1.5, 126.5, -126.5]]


def _nearest(ctx, q, codes, scales, k, goff=0, soff=0):
    qd = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    gd = torch.empty((goff + codes.size,), dtype=torch.int8, device="cuda")[goff:].view(codes.shape)
    sd = torch.empty((soff + len(scales),), dtype=torch.float32, device="cuda")[soff:]
    gd.copy_(torch.from_numpy(codes))
    sd.copy_(torch.from_numpy(scales))
    assert gd.data_ptr() % 16 == goff and sd.data_ptr() % 16 == 4 * soff
    v, i = ore.nearest(ctx, qd, gd, k, scales=sd)
    torch.cuda.synchronize()
    return v.cpu().numpy().view(np.uint32), i.cpu().numpy()


def _exact(ctx, q, codes, scales, k, qd=None, **off):
    want_v, want_i = best(scores(*quant(q), codes, scales), k)
    v, i = _nearest(ctx, q if qd is None else qd, codes, scales, k, **off)
    np.testing.assert_array_equal(i, want_i)
    np.testing.assert_array_equal(v, want_v)


def _given(seed, n, G, D):
    """Any code, scales 2^-6 .. 2^6, small integer queries with a +-127 in every row (tq = 1): ties everywhere."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-8, 9, (n, D)).astype(np.float32)
    q[np.arange(n), rng.integers(0, D, n)] = rng.choice(np.float32([-127, 127]), n)
    return q, rng.integers(-128, 128, (G, D)).astype(np.int8), np.exp2(rng.integers(-6, 7, G)).astype(np.float32)


# (n, G, D, k): D of {1 .. 512}, 1040 (past the resident 1024: two chunks, 16-byte loads) and 2049 (three chunks, 1-byte
# loads); n of {1, 15, 17, 65}; G of {1, step - 1, step + 1, 1000, 4099}; k of {1, 5, min(G, 64)}; the last on several segments
@pytest.mark.parametrize("n, G, D, k", [(1, 1, 1, 1), (15, 127, 15, 64), (17, 129, 16, 5), (65, 1000, 17, 64), (17, 4099, 63, 1),
                                        (1, 1000, 65, 5), (15, 4099, 512, 64), (65, 129, 1040, 1), (17, 1000, 2049, 5),
                                        (65, 40000, 16, 5)])
def test_given_codes(gpu_ctx, n, G, D, k):
    segments, step = ore.nearest_segments_i8(gpu_ctx, n, G)
    steps = (G + step - 1) // step
    assert step == 128 and 1 <= segments <= steps  # the cases' 127 and 129 are step - 1 and step + 1
    if G == 40000:  # a merge launch, and ceil(steps / segments) >= 2 steps per workgroup (the last takes the rest)
        assert segments > 1 and -(-steps // segments) >= 2, segments
    q, codes, scales = _given(n * G + D, n, G, D)
    assert (quant(q)[1] == 1).all()
    _exact(gpu_ctx, q, codes, scales, k)


@pytest.mark.parametrize("D", [5, 512])
def test_float_queries_and_packed_gallery(gpu_ctx, D, k=5):
    q, g = normal(D)  # through the packer and the in-kernel query quantiser
    codes, scales = (t.cpu().numpy() for t in ore.gallery_i8(gpu_ctx, torch.from_numpy(g).cuda()))
    want_c, want_t = quant(g)
    np.testing.assert_array_equal(codes, want_c)
    np.testing.assert_array_equal(scales.view(np.uint32), want_t.view(np.uint32))
    _exact(gpu_ctx, q, codes, scales, k)


@pytest.mark.parametrize("order", ["rising", "falling"])
@pytest.mark.parametrize("k, D", [(64, 16), (5, 3)])  # 16-byte and 1-byte gallery loads
def test_sorted_gallery(gpu_ctx, order, k, D):
    """Row j holds the three base-100 digits of j, query i is c (10000, 100, 1), c = 1 + i % 8: its codes are (127, 1, 0),
    the score rises with j // 100.  Rising: a compaction at every step; falling: none after the first.  Two query tiles."""
    n, G = 65, 300000
    segments, step = ore.nearest_segments_i8(gpu_ctx, n, G)
    assert (G + step - 1) // step >= 8 * segments, segments
    j = np.arange(G) if order == "rising" else np.arange(G)[::-1]
    codes, q = np.zeros((G, D), np.int8), np.zeros((n, D), np.float32)
    codes[:, 0], codes[:, 1], codes[:, 2] = j // 10000, j // 100 % 100, j % 100
    q[:, :3] = np.outer(1 + np.arange(n) % 8, np.float32([10000, 100, 1]))
    assert (quant(q)[0][:, :3] == [127, 1, 0]).all()
    _exact(gpu_ctx, q, codes, np.ones(G, np.float32), k)


@pytest.mark.parametrize("D", [64, 67])
def test_sliced_misaligned(gpu_ctx, D):
    """q in a NaN-filled buffer at nstride 80 > D, 4 bytes past a 16-byte boundary; the gallery 1 byte, the scales 4."""
    q, (codes, scales) = normal(D, 17, 1)[0], _given(3, 1, 1000, D)[1:]
    qd = torch.full((1 + 17 * 80,), float("nan"), device="cuda")[1:].view(17, 80)[:, :D]
    qd.copy_(torch.from_numpy(q))
    assert qd.data_ptr() % 16 == 4 and qd.stride(0) == 80
    _exact(gpu_ctx, q, codes, scales, 5, qd, goff=1, soff=1)


@pytest.mark.parametrize("D", [8, 7])  # 16-byte loads with packed stores; one element per thread
def test_packer_edge_rows(gpu_ctx, D):
    """A zero row, a NaN (code 0, skipped by the maximum), +inf (t = inf, codes 0), subnormals, ties to even."""
    x = np.float32([r + [0.0] * (D - len(r)) for r in EDGE_ROWS])
    codes, scales = ore.gallery_i8(gpu_ctx, torch.from_numpy(x).cuda())
    want_c, want_t = quant(x)
    assert want_c[1, :3].tolist() == [0, 64, -127] and want_c[4, :7].tolist() == [127, 0, 0, 2, -2, 126, -126]
    assert not want_c[[0, 2]].any() and want_t[0] == 0 and np.isposinf(want_t[2]) and want_c.min() == -127
    np.testing.assert_array_equal(codes.cpu().numpy(), want_c)
    np.testing.assert_array_equal(scales.cpu().numpy().view(np.uint32), want_t.view(np.uint32))


def test_query_edges(gpu_ctx):
    """A NaN element (code 0), an all-zero query (scores 0), a query holding +inf (every score NaN, indices 0 .. k - 1)."""
    _, codes, scales = _given(7, 1, 300, 8)
    q = np.float32([r + [0.0] * (8 - len(r)) for r in EDGE_ROWS[:3]])[[1, 0, 2]]
    s = scores(*quant(q), codes, scales)
    assert not np.isnan(s[:2]).any() and not s[1].any() and np.isnan(s[2]).all()
    _exact(gpu_ctx, q, codes, scales, 5)
