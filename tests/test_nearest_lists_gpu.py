"""GPU: ore.nearest_lists (csrc/ore_nearest_lists.hip) against float64 on integer data, against the bits of ore.nearest
on the same float16 gallery, under a permutation of the lists, through ore.ivf_build / IvfIndex.search, and captured."""
import numpy as np
import pytest
import torch

import ore
from _poison import make_ctx

pytestmark = pytest.mark.gpu
R = ore.IVF_CHUNK_ROWS
NAN = 0x7fc00000


def _dev(a, dtype, off=0):  # a on the device as dtype, `off` elements past a 16-byte boundary
    t = torch.empty((off + a.size,), dtype=dtype, device="cuda")[off:].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _expect(q, g, offsets, probes, k):
    """float64 matmul of the f16-rounded operands, masked to the union of the probed lists, stable argsort"""
    L = len(offsets) - 1
    s = (q.astype(np.float16).astype(np.float64) @ g.astype(np.float16).astype(np.float64).T).astype(np.float32) + np.float32(0)
    v, i = np.full((len(q), k), NAN, np.uint32), np.full((len(q), k), -1, np.int32)
    for r, row in enumerate(probes):
        rows = np.concatenate([np.arange(offsets[l], offsets[l + 1]) for l in np.unique(row[(row >= 0) & (row < L)])] + [np.arange(0)])
        o = rows[np.argsort(-s[r, rows], kind="stable")[:k]].astype(np.int64)
        i[r, :o.size], v[r, :o.size] = o, s[r, o].view(np.uint32)
    return v, i, s


def _run(ctx, q, g, offsets, probes, k, off=0, qd=None):
    chunks = ore.ivf_chunks(torch.from_numpy(offsets)).cuda()
    v, i = ore.nearest_lists(ctx, _dev(q, torch.float32) if qd is None else qd, _dev(g, torch.float16, off), torch.from_numpy(offsets).cuda(),
                             chunks, _dev(probes, torch.int32), k, max(int(np.diff(offsets).max()), 1))
    torch.cuda.synchronize()
    return v.cpu().numpy().view(np.uint32), i.cpu().numpy()


SIZES5 = [0, 1, R - 1, R, R + 1]


def _probes(how, rng, n, P, L):
    p = rng.integers(-1 if L > 1 else 0, L + 1 if L > 1 else 1, (n, P)).astype(np.int32)  # -1 and L are padding
    if how == "one":  # 49 pairs on list 2 (four B blocks), then unions of one row and of none: below k
        p[:49, 0], p[49:64, 0], p[64:, 0] = 2, 1, 0
    if how == "groups":  # list 4 by all 17 (two blocks), list 3 by 16 (one); a duplicate, a -1 and an entry >= L
        p[:, 0], p[:, 1], p[:, 2] = rng.integers(0, 3, n), np.where(np.arange(n) < 16, 3, -1), 4
        p[0, 0], p[1, 0], p[2, 0] = 3, -1, L + 4
    if how == "all":  # list 7 by all 130: three groups, the last of 2 pairs; duplicates come by themselves at P = 64
        p[:, 0] = 7
    return p


@pytest.mark.parametrize("n, D, k, P, sizes, how, off", [
    (1, 1, 1, 1, [5], "", 0), (17, 7, 5, 3, SIZES5, "", 0), (65, 8, 64, 1, SIZES5, "one", 1),
    (17, 512, 5, 3, [0, 1, R - 1, R, 3 * R + 32], "groups", 0), (130, 33, 5, 64, None, "all", 0)])
def test_exact_with_ties(gpu_ctx, n, D, k, P, sizes, how, off):
    rng = np.random.default_rng(n * D + k)
    if sizes is None:  # L = 300: short lists, empty ones among them, and one of more than 3 R rows
        sizes = rng.integers(0, 40, 300)
        sizes[7] = 3 * R + 5
    offsets = _offsets(sizes)
    q, g = rng.integers(-8, 9, (n, D)).astype(np.float32), rng.integers(-8, 9, (offsets[-1], D)).astype(np.float32)
    probes = _probes(how, rng, n, P, len(sizes))
    qd = None
    if how == "all":  # q as a slice at stride 80 of a NaN-filled buffer
        qd = torch.full((n, 80), float("nan"), device="cuda")[:, 3:3 + D]
        qd.copy_(torch.from_numpy(q))
    v, i = _run(gpu_ctx, q, g, offsets, probes, k, off, qd)
    wv, wi, _ = _expect(q, g, offsets, probes, k)
    np.testing.assert_array_equal(i, wi)
    np.testing.assert_array_equal(v, wv)
    assert how != "one" or (i[49:] == -1).sum() == 15 * 63 + 64


def _normals(D, n=33, seed=5):
    rng = np.random.default_rng(seed)
    sizes = [700, 0, 1, 300, R, 2000, 4099 - 3001 - R]
    return rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((4099, D)).astype(np.float16), _offsets(sizes)


@pytest.mark.parametrize("D", [5, 512])
def test_all_lists_is_full_search(gpu_ctx, D):
    q, g, offsets = _normals(D)
    probes = np.stack([np.random.default_rng(r).permutation(7) for r in range(len(q))]).astype(np.int32)
    v, i = _run(gpu_ctx, q, g, offsets, probes, 5)
    fv, fi = ore.nearest(gpu_ctx, _dev(q, torch.float32), _dev(g, torch.float16), 5)
    np.testing.assert_array_equal(i, fi.cpu().numpy())
    np.testing.assert_array_equal(v, fv.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("D", [5, 512])
def test_position_independence(gpu_ctx, D, k=5):
    q, g, offsets = _normals(D)
    rng = np.random.default_rng(11)
    probes = np.stack([rng.permutation(7)[:3] for _ in range(len(q))]).astype(np.int32)
    _, wi, s = _expect(q, g, offsets, probes, k + 1)
    top = np.take_along_axis(s.astype(np.float64), wi.astype(np.int64), 1)
    assert (wi >= 0).all() and (np.diff(top, axis=1) < 0).all()  # no tie at ranks <= k + 1 in any of the 33 rows
    v, i = _run(gpu_ctx, q, g, offsets, probes, k)
    v7, i7 = _run(gpu_ctx, q[:7], g, offsets, probes[:7], k)
    np.testing.assert_array_equal(i7, i[:7])
    np.testing.assert_array_equal(v7, v[:7])
    perm = rng.permutation(7)  # the new gallery holds the old lists perm[0], perm[1], ...
    old_rows = np.concatenate([np.arange(offsets[l], offsets[l + 1]) for l in perm])
    new_of = np.empty(len(g), np.int64)
    new_of[old_rows] = np.arange(len(g))
    vp, ip = _run(gpu_ctx, q, g[old_rows], _offsets(np.diff(offsets)[perm]), np.argsort(perm)[probes].astype(np.int32), k)
    np.testing.assert_array_equal(vp, v)
    np.testing.assert_array_equal(ip, new_of[i])


def test_index(gpu_ctx, G=2000, D=16, L=9, n=8, k=5):
    rng = np.random.default_rng(3)
    g, c, q = (rng.integers(-8, 9, (m, D)).astype(np.float32) for m in (G, L, n))
    gd, qd = _dev(g, torch.float32), _dev(q, torch.float32)
    index = ore.ivf_build(gpu_ctx, gd, _dev(c, torch.float32))
    ids, offsets = index.ids.cpu().numpy(), index.offsets.cpu().numpy()
    assert np.array_equal(np.sort(ids), np.arange(G)) and offsets[0] == 0 and offsets[-1] == G and (np.diff(offsets) >= 0).all()
    assert index.max_list_rows == np.diff(offsets).max() and index.gallery.dtype == torch.float16
    assign = np.argmax(g.astype(np.float64) @ c.astype(np.float64).T, axis=1)  # the first of equal maxima
    np.testing.assert_array_equal(np.repeat(np.arange(L), np.diff(offsets)), assign[ids])
    assert all((np.diff(ids[offsets[l]:offsets[l + 1]]) > 0).all() for l in range(L))  # by original row inside a list
    s = q.astype(np.float64) @ g.astype(np.float64).T
    top = -np.sort(-s, axis=1)
    assert (top[:, k - 1] > top[:, k]).all()  # no tie across rank k: the index sets are determined
    _, fi = ore.nearest(gpu_ctx, qd, ore.gallery_f16(gpu_ctx, gd), k)
    v, i = index.search(qd, k, nprobe=L)
    np.testing.assert_array_equal(np.sort(i.cpu().numpy(), axis=1), np.sort(fi.cpu().numpy(), axis=1))
    np.testing.assert_array_equal(v.cpu().numpy(), top[:, :k].astype(np.float32))
    rv, _ = index.search(qd, k, nprobe=L, rerank=gd)
    np.testing.assert_array_equal(rv.cpu().numpy().view(np.uint32), ore.nearest(gpu_ctx, qd, gd, k)[0].cpu().numpy().view(np.uint32))


def test_capture_replay(k=5):
    """After one warm call of the shape the call is captured and replayed on new queries and new probes; a shape whose
    scratch must grow inside the capture is refused"""
    offsets = _normals(16)[2]
    g = np.random.default_rng(0).integers(-8, 9, (4099, 16)).astype(np.float16)
    gd, od = _dev(g, torch.float16), torch.from_numpy(offsets).cuda()
    chunks, rows = ore.ivf_chunks(torch.from_numpy(offsets)).cuda(), int(np.diff(offsets).max())
    qd, pd = torch.zeros((33, 16), device="cuda"), torch.zeros((33, 3), dtype=torch.int32, device="cuda")
    big = torch.zeros((33, 64), dtype=torch.int32, device="cuda")
    ctx, stream = make_ctx()
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            ore.nearest_lists(ctx, qd, gd, od, chunks, pd, k, rows)  # the warm call
            stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            with pytest.raises(ore.OreError, match="inside a stream capture"):
                ore.nearest_lists(ctx, qd, gd, od, chunks, big, k, rows)
            cv, ci = ore.nearest_lists(ctx, qd, gd, od, chunks, pd, k, rows)
        for seed in (1, 2):
            rng = np.random.default_rng(seed)
            probes = rng.integers(-1, 8, (33, 3)).astype(np.int32)
            with torch.cuda.stream(stream):
                qd.copy_(torch.from_numpy(rng.integers(-8, 9, (33, 16)).astype(np.float32)))
                pd.copy_(torch.from_numpy(probes))
                graph.replay()
                stream.synchronize()
                got = cv.cpu().numpy().view(np.uint32), ci.cpu().numpy()
                ev, ei = ore.nearest_lists(ctx, qd, gd, od, chunks, pd, k, rows)
                eager = ev.cpu().numpy().view(np.uint32), ei.cpu().numpy()
            np.testing.assert_array_equal(got[1], eager[1])
            np.testing.assert_array_equal(got[0], eager[0])
            want = _expect(qd.cpu().numpy(), g, offsets, probes, k)
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(got[0], want[0])
    finally:
        ctx.close()
