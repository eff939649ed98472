"""GPU: ore.kmeans_step (csrc/ore_kmeans.hip) against float64 on integer data -- assignment and scores to the bit,
ties included, and the bits of ore.nearest on the same float16 centroids; the update within 1 ulp; poisoned scratch;
ore.ivf_train against a float64 Lloyd loop on planted clusters; and captured."""
import functools

import numpy as np
import pytest
import torch

import ore
from _poison import NAN, make_ctx

pytestmark = pytest.mark.gpu
CASES = [(1, 1, 1), (63, 7, 127), (65, 8, 129), (200, 33, 300), (130, 512, 257)]


@functools.lru_cache(maxsize=None)
def _case(S, D, L):
    """Integers in [-8, 8]: exact in f16, sums exact in f32 and f64.  Where the shape allows: no centroid uses the last
    d; centroid 0 is all -0.0, so it scores 0 everywhere and wins exactly the rows that score 0 against every centroid
    (the lowest index among equals), which are v and -v along the last d: a zero sum; the last centroid repeats
    centroid 1 and so never wins: an empty list.  Returns the inputs and the float64 results, never written again."""
    rng = np.random.default_rng(S * D + L)
    x, c = rng.integers(-8, 9, (S, D)).astype(np.float32), rng.integers(-8, 9, (L, D)).astype(np.float32)
    if min(S, D, L) >= 3:
        c[:, D - 1], c[0], c[L - 1] = 0, -0.0, c[1]
        x[S - 2], x[S - 2, D - 1] = 0, 5
        x[S - 1] = -x[S - 2]
    s = x.astype(np.float64) @ c.astype(np.float64).T
    assign = s.argmax(1)  # the first of equal maxima
    counts = np.bincount(assign, minlength=L)
    sums = np.zeros((L, D))
    np.add.at(sums, assign, x.astype(np.float64))
    n2 = (sums * sums).sum(1, keepdims=True)
    keep = (counts[:, None] == 0) | (n2 == 0)
    new = np.where(keep, c, (sums / np.sqrt(np.where(keep, 1, n2))).astype(np.float32))
    if min(S, D, L) >= 3:
        assert counts[0] == 2 and keep[0] and counts[L - 1] == 0 and (~keep).any()
    return dict(x=x, c=c, assign=assign.astype(np.int32), scores=s[np.arange(S), assign].astype(np.float32) + np.float32(0),
                counts=counts.astype(np.int32), new=new, keep=keep[:, 0])


def _upload(r, sliced):
    """x and the centroids on the device; sliced: x 1 element past a 16-byte boundary at a row stride of D + 4 in NaNs"""
    S, D = r["x"].shape
    xd = torch.full((S, D + 4), float("nan"), device="cuda")[:, 1:1 + D] if sliced else torch.empty((S, D), device="cuda")
    xd.copy_(torch.from_numpy(r["x"]))
    return xd, torch.from_numpy(r["c"]).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("S, D, L", CASES)
def test_exact_assignment(gpu_ctx, S, D, L):
    r = _case(S, D, L)
    xd, cd = _upload(r, sliced=(S, D, L) == (65, 8, 129))
    _, assign, scores, counts = ore.kmeans_step(gpu_ctx, xd, cd)
    np.testing.assert_array_equal(assign.cpu().numpy(), r["assign"])
    np.testing.assert_array_equal(_bits(scores), r["scores"].view(np.uint32))
    np.testing.assert_array_equal(counts.cpu().numpy(), r["counts"])
    v, i = ore.nearest(gpu_ctx, xd, ore.gallery_f16(gpu_ctx, cd), 1)
    np.testing.assert_array_equal(assign.cpu().numpy(), i.cpu().numpy()[:, 0])
    np.testing.assert_array_equal(_bits(scores), _bits(v)[:, 0])


@pytest.mark.parametrize("S, D, L", CASES)
def test_update(gpu_ctx, S, D, L):
    r = _case(S, D, L)
    xd, cd = _upload(r, sliced=(S, D, L) == (65, 8, 129))
    first = ore.kmeans_step(gpu_ctx, xd, cd)
    got, want = first[0].cpu().numpy(), r["new"]
    np.testing.assert_array_equal(got[r["keep"]].view(np.uint32), r["c"][r["keep"]].view(np.uint32))  # -0.0 stays -0.0
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32))[~r["keep"]]
    print(f"kmeans update S={S} D={D} L={L}: largest difference {ulps.max(initial=0)} ulp")
    assert ulps.max(initial=0) <= 1 and (np.signbit(got) == np.signbit(want))[~r["keep"]].all()
    inplace = cd.clone()
    for other in (ore.kmeans_step(gpu_ctx, xd, cd), ore.kmeans_step(gpu_ctx, xd, inplace, out=inplace)):
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, other))
    assert inplace.data_ptr() == other[0].data_ptr()


def test_poisoned_scratch(gpu_ctx, S=200, D=33, L=300):
    """the scratch freshly allocated under ore_ctx_set_alloc_fill: what it held before is never read"""
    r = _case(S, D, L)
    xd, cd = _upload(r, sliced=False)
    want = _bits(ore.kmeans_step(gpu_ctx, xd, cd)[0])
    ctx, stream = make_ctx()
    try:
        ctx.set_alloc_fill(True, NAN)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            new, assign, scores, counts = ore.kmeans_step(ctx, xd, cd)
            stream.synchronize()
        np.testing.assert_array_equal(assign.cpu().numpy(), r["assign"])
        np.testing.assert_array_equal(_bits(scores), r["scores"].view(np.uint32))
        np.testing.assert_array_equal(counts.cpu().numpy(), r["counts"])
        np.testing.assert_array_equal(_bits(new), want)
    finally:
        ctx.close()


def _planted(seed=7, L=12, D=48, per=40):
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((L, D))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    x = np.repeat(dirs, per, 0) + 0.05 * rng.standard_normal((L * per, D))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    extra = -dirs.mean(0) / np.linalg.norm(dirs.mean(0))  # wins no row: an empty list from the first step on
    return dirs, x, np.concatenate([x[::per], extra[None].astype(np.float32)])


def _lloyd64(x, c, iters):
    """float64 Lloyd with ivf_train's rule for empty lists; also the smallest best-minus-second score of any row and the
    smallest gap between a row that seeds an empty list and the next row in line, over all iterations"""
    x, c, margin, gap = x.astype(np.float64), c.astype(np.float64), np.inf, np.inf
    for _ in range(iters):
        s = x @ c.T
        top = np.sort(s, axis=1)
        assign, best = s.argmax(1), top[:, -1]
        counts = np.bincount(assign, minlength=len(c))
        sums = np.zeros_like(c)
        np.add.at(sums, assign, x)
        c = np.where(counts[:, None] > 0, sums / np.maximum(np.linalg.norm(sums, axis=1, keepdims=True), 1e-300), c)
        empty, order = np.flatnonzero(counts == 0), np.argsort(best, kind="stable")
        c[empty] = x[order[:len(empty)]] / np.linalg.norm(x[order[:len(empty)]], axis=1, keepdims=True)
        margin, gap = min(margin, (top[:, -1] - top[:, -2]).min()), min([gap, *np.diff(best[order[:len(empty) + 1]])])
    return c, margin, gap


def test_ivf_train(gpu_ctx):
    dirs, x, init = _planted()
    assert (dirs @ dirs.T - np.eye(len(dirs))).max() <= 0.5
    want, margin, gap = _lloyd64(x, init, 3)
    # conditions on the inputs: f16 rounding moves a score by at most 2^-10 |x| |c|, about 0.001, so two rows' order by
    # score is safe from 0.002 on; and the extra centroid wins no row
    assert margin > 0.01 and gap > 0.002 and (x.astype(np.float64) @ init[-1] < (x.astype(np.float64) @ init[:-1].T).max(1)).all(), (margin, gap)
    xd = torch.from_numpy(x).cuda()
    got = ore.ivf_train(gpu_ctx, xd, len(init), iters=3, init=torch.from_numpy(init).cuda()).cpu().numpy()
    print(f"ivf_train: largest difference {np.abs(got - want).max():.3g}, norm off by {np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max():.3g}")
    assert np.abs(got - want).max() <= 2.0 ** -20
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    a, b = (ore.ivf_train(gpu_ctx, xd, 13, iters=2, seed=7) for _ in range(2))
    assert a.shape == (13, 48) and np.array_equal(_bits(a), _bits(b))


def test_capture_replay(S=200, D=33, L=300):
    """After one warm call of the shape a step is captured and replayed on new samples: the eager result, twice"""
    r = _case(S, D, L)
    xd, cd = _upload(r, sliced=False)
    ctx, stream = make_ctx()
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            ore.kmeans_step(ctx, xd, cd)  # the warm call
            stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            captured = ore.kmeans_step(ctx, xd, cd)
        for seed in (1, 2):
            with torch.cuda.stream(stream):
                xd.copy_(torch.from_numpy(np.random.default_rng(seed).integers(-8, 9, (S, D)).astype(np.float32)))
                graph.replay()
                stream.synchronize()
                got = [_bits(t) for t in captured]
                eager = [_bits(t) for t in ore.kmeans_step(ctx, xd, cd)]
            assert all(np.array_equal(a, b) for a, b in zip(got, eager))
            assert seed == 1 or not np.array_equal(got[1], first_assign)
            first_assign = got[1]
    finally:
        ctx.close()
