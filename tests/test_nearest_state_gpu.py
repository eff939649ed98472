"""GPU: what lies between the calls of the retrieval family -- the context-owned partial buffer (ctx->nearest_part,
csrc/ore_ops.cpp) and the capture rule of include/ore.h.

The three searches keep their segments' keys [n][S][k] in that buffer and nearest_bins its winners [n][NB]; it grows on
demand, is never cleared, and is freed behind a stream synchronise.  A kernel that read one slot its own call did not
write would pass on a fresh allocation, which is usually zero, the empty key.  So here every call runs on a buffer
that ore_ctx_set_alloc_fill has just filled with a chosen word, or that holds the keys of an earlier call of another
layout, on contexts of their own (tests/_poison.py make_ctx: what another test left behind must not matter).  Growth
inside a stream capture is refused before any device call; after one call of the shape outside, the searches are
captured and replayed on new queries.  References: tests/_nearest_i8.py for int8, a float64 matmul on integers of
|x| <= 8 for f32 and f16 (products and f32 sums exact).  Every comparison is on the bits of the values and on the
indices."""
import functools

import numpy as np
import pytest
import torch

import ore
from _nearest_i8 import best, bins_ref, quant, scores
from _poison import make_ctx

pytestmark = pytest.mark.gpu
TORCH = {"f32": torch.float32, "f16": torch.float16, "i8": torch.int8}


@functools.lru_cache(maxsize=None)
def _data(fmt, n, G, D, seed=0, inf_scales=False):
    """(q, gallery, scales or None, scores): integers in -8 .. 8; int8: any code, scales 2^-6 .. 2^6 (a third +inf on
    request) and a +-127 in every query row (tq = 1)"""
    rng = np.random.default_rng([seed, n, G, D])
    q = rng.integers(-8, 9, (n, D)).astype(np.float32)
    if fmt != "i8":
        g = rng.integers(-8, 9, (G, D)).astype(np.float16 if fmt == "f16" else np.float32)
        return q, g, None, (q.astype(np.float64) @ g.astype(np.float64).T).astype(np.float32)
    q[np.arange(n), rng.integers(0, D, n)] = rng.choice(np.float32([-127, 127]), n)
    g, t = rng.integers(-128, 128, (G, D)).astype(np.int8), np.exp2(rng.integers(-6, 7, G)).astype(np.float32)
    if inf_scales:
        t[rng.permutation(G)[:G // 3]] = np.inf
    return q, g, t, scores(*quant(q), g, t)


class Call:
    """One search -- op "nearest" (m = k) or "bins" (m = c, bins of B rows) -- with its operands and its reference"""

    def __init__(self, op, fmt, n, G, D, m, B=32, seed=0, inf_scales=False):
        self.op, self.fmt, self.n, self.G, self.m, self.B = op, fmt, n, G, m, B
        self.q, self.g, self.t, self.s = _data(fmt, n, G, D, seed, inf_scales)
        self.want = best(self.s, m) if op == "nearest" else bins_ref(self.s, B, m)

    def upload(self):
        self.qd, self.gd = torch.from_numpy(self.q).cuda(), torch.from_numpy(self.g).cuda()
        self.td = None if self.t is None else torch.from_numpy(self.t).cuda()
        return self

    def segments(self, ctx):
        if self.op == "bins":
            return ore.nearest_bins_segments(ctx, self.n, self.G, self.B)[0]
        return {"f32": lambda *a: ore.nearest_segments(*a), "f16": lambda *a: ore.nearest_segments_f16(*a)[0],
                "i8": lambda *a: ore.nearest_segments_i8(*a)[0]}[self.fmt](ctx, self.n, self.G)

    def bytes(self, ctx):
        """what the call needs of the buffer: nearest_partial_bytes / nearest_bins_bytes (no slabs at these sizes)"""
        if self.op == "bins":
            return self.n * -(-self.G // self.B) * 8
        S = self.segments(ctx)
        return self.n * S * self.m * 8 if S > 1 else 0

    def run(self, ctx, q=None):
        q = self.qd if q is None else q
        if self.op == "bins":
            return ore.nearest_bins(ctx, q, self.gd, self.m, self.B, scales=self.td)
        return ore.nearest(ctx, q, self.gd, self.m, scales=self.td)


def _np(out):
    return out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy()


def _exact(got, want, what=""):
    np.testing.assert_array_equal(got[1], want[1], what)
    np.testing.assert_array_equal(got[0], want[0], what)


def _eager(ctx, stream, call):
    with torch.cuda.stream(stream):
        out = call.run(ctx)
        stream.synchronize()
        return _np(out)


# as 64-bit keys: empty; the largest key there is (index 0); a NaN's bits above a NaN's bits; +inf's
@pytest.mark.parametrize("pattern", [0x00000000, 0xFFFFFFFF, 0x7FC00000, 0x7F800000])
def test_alloc_fill(pattern):
    """Every call finds the buffer freshly grown, so filled: the calls run in ascending size, and one that would fit
    what the context already has gets a new context."""
    calls = [Call("nearest", "f32", 17, 4099, 8, 5), Call("nearest", "f32", 17, 4099, 8, 64)]
    calls += [Call("nearest", fmt, 17, 4099, 16, k) for fmt in ("f16", "i8") for k in (5, 64)]
    calls += [Call("bins", "i8", 17, 4 * 32 + 1, 16, 5), Call("bins", "f16", 65, 4099, 16, 65)]
    ctx, stream = make_ctx()
    try:
        ctx.set_alloc_fill(True, pattern)
        for c in calls[2:6]:
            assert c.segments(ctx) > 1
        held, grown = 0, 0
        for c in sorted(calls, key=lambda c: c.bytes(ctx)):
            need = c.bytes(ctx)
            assert need > 0
            if need <= held:
                ctx.close()
                ctx, stream = make_ctx()
                ctx.set_alloc_fill(True, pattern)
            else:
                grown += held > 0
            held = need
            c.upload()
            torch.cuda.synchronize()
            _exact(_eager(ctx, stream, c), c.want, f"{c.op} {c.fmt} m = {c.m}, pattern {pattern:#x}")
        assert grown >= 3  # free and reallocate under fill, several times on one context
    finally:
        ctx.close()


def test_stale_contents():
    """One context; every call reads a buffer that holds the keys of the calls before it, in another layout"""
    big = Call("bins", "i8", 65, 40000, 16, 256, inf_scales=True)
    assert np.isinf(big.s).mean() > 0.3
    calls = [big, Call("nearest", "i8", 17, 4099, 16, 64), Call("nearest", "f32", 1, 4099, 8, 5),
             Call("bins", "f16", 17, 4 * 32 + 1, 16, 5), Call("nearest", "f32", 17, 17, 8, 5), big]
    ctx, stream = make_ctx()
    try:
        assert calls[4].bytes(ctx) == 0 and all(c.bytes(ctx) < big.bytes(ctx) for c in calls[1:5])
        for c in calls:
            c.upload()
        torch.cuda.synchronize()
        for step, c in enumerate(calls):
            _exact(_eager(ctx, stream, c), c.want, f"step {step + 1}")
    finally:
        ctx.close()


def test_growth_with_work_in_flight():
    """A small call and then a larger one of another format, nothing between them: the buffer the first call's kernels
    read is freed only behind them"""
    small, large = Call("nearest", "f16", 17, 4099, 16, 5).upload(), Call("bins", "i8", 65, 40000, 16, 256).upload()
    ctx, stream = make_ctx()
    try:
        assert 0 < small.bytes(ctx) < large.bytes(ctx)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            a = small.run(ctx)
            b = large.run(ctx)
            stream.synchronize()
            _exact(_np(a), small.want)
            _exact(_np(b), large.want)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ capture and replay
def _rerank_ref(q, g32, cand, k):
    """ore.rerank in numpy: the k best of each row's candidates (distinct here), scored in float64 on integers, ties by
    the lower row"""
    v, i = np.empty((len(q), k), np.uint32), np.empty((len(q), k), np.int64)
    for r, c in enumerate(cand):
        rows = np.sort(c)
        s = (g32[rows].astype(np.float64) @ q[r].astype(np.float64)).astype(np.float32)
        o = np.argsort(-s, kind="stable")[:k]
        v[r], i[r] = (s[o] + np.float32(0)).view(np.uint32), rows[o]
    return v, i


def test_capture_cold():
    """On a fresh context a search that needs the buffer is refused inside a capture and runs after it; rerank and a
    search of one segment are captured with no call before them"""
    f16 = Call("nearest", "f16", 17, 4099, 16, 5).upload()
    one = Call("nearest", "f32", 17, 17, 8, 5).upload()
    rng = np.random.default_rng(3)
    cand = np.stack([rng.permutation(4099)[:32] for _ in range(17)]).astype(np.int32)
    g32 = f16.g.astype(np.float32)
    candd, g32d = torch.from_numpy(cand).cuda(), torch.from_numpy(g32).cuda()
    ctx, stream = make_ctx()
    try:
        assert f16.segments(ctx) > 1 and one.segments(ctx) == 1
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            with pytest.raises(ore.OreError, match="inside a stream capture") as refused:
                f16.run(ctx)
            rr = ore.rerank(ctx, f16.qd, g32d, candd, 5)
            single = one.run(ctx)
        assert refused.value.status == 1  # ORE_ERR_INVALID
        _exact(_eager(ctx, stream, f16), f16.want)
        with torch.cuda.stream(stream):
            g.replay()
            stream.synchronize()
            _exact(_np(rr), _rerank_ref(f16.q, g32, cand, 5))
            _exact(_np(single), one.want)
    finally:
        ctx.close()


def test_capture_warm(n=17, G=4099, D=16, k=5):
    """The three searches, nearest_bins and the binned two-stage form in one graph on a static q; two replays on new
    queries against the eager calls and numpy"""
    sets = []
    for seed in (0, 1, 2):  # the warm-up's queries and two more; the galleries are seed 0's
        sets.append({fmt: _data(fmt, n, G, D, seed) for fmt in TORCH})
    base = sets[0]
    g32 = base["i8"][1].astype(np.float32)  # the two-stage form's exact gallery: the int8 codes as numbers
    gal = {fmt: torch.from_numpy(base[fmt][1]).cuda() for fmt in TORCH}
    td, g32d = torch.from_numpy(base["i8"][2]).cuda(), torch.from_numpy(g32).cuda()
    qs = {fmt: torch.from_numpy(base[fmt][0]).cuda() for fmt in TORCH}  # static

    def run_all(ctx):
        out = {fmt: ore.nearest(ctx, qs[fmt], gal[fmt], k, scales=td if fmt == "i8" else None) for fmt in TORCH}
        out["bins"] = ore.nearest_bins(ctx, qs["i8"], gal["i8"], 32, 32, scales=td)
        out["two"] = ore.nearest(ctx, qs["i8"], gal["i8"], k, scales=td, rerank=g32d, candidates=32, bin_rows=32)
        return out

    def want(s):
        q8 = s["i8"][0]
        s8 = scores(*quant(q8), base["i8"][1], base["i8"][2])
        w = {"f32": best((s["f32"][0].astype(np.float64) @ base["f32"][1].astype(np.float64).T).astype(np.float32), k),
             "f16": best((s["f16"][0].astype(np.float64) @ base["f16"][1].astype(np.float64).T).astype(np.float32), k),
             "i8": best(s8, k), "bins": bins_ref(s8, 32, 32)}
        w["two"] = _rerank_ref(q8, g32, w["bins"][1], k)
        return w

    ctx, stream = make_ctx()
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            run_all(ctx)  # one call of each shape outside the capture
            stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            captured = run_all(ctx)
        for s in sets[1:]:
            with torch.cuda.stream(stream):
                for fmt in TORCH:
                    qs[fmt].copy_(torch.from_numpy(s[fmt][0]))
                g.replay()
                stream.synchronize()
                got = {name: _np(o) for name, o in captured.items()}
                eager = {name: _np(o) for name, o in run_all(ctx).items()}  # .cpu() waits for the stream
            w = want(s)
            for name in got:
                _exact(got[name], eager[name], f"{name}: replay against eager")
                _exact(got[name], w[name], f"{name}: replay against numpy")
        # a shape that needs fewer bytes than an earlier call, of another n and k, is captured with no call of its own
        small = Call("nearest", "i8", 5, G, D, 7, seed=4).upload()
        assert 0 < small.bytes(ctx) < Call("bins", "i8", n, G, D, 32).bytes(ctx)
        torch.cuda.synchronize()
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=stream):
            out = small.run(ctx)
        with torch.cuda.stream(stream):
            g2.replay()
            stream.synchronize()
            _exact(_np(out), small.want)
    finally:
        ctx.close()
