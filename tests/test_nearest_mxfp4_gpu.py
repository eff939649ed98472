"""GPU: ore_gallery_mxfp4 / ore_nearest_bins_mxfp4 (csrc/ore_nearest_fp4.hip) against include/ore.h's format restated in
numpy; the references are float64 products of ore.mxfp4_decode()'s values."""
import ctypes

import numpy as np
import pytest
import torch

import ore
from _nearest_i8 import bins_ref, normal

pytestmark = pytest.mark.gpu
KAPPA = 0.0  # include/ore.h's ORE_MXFP4_KAPPA


def quant(x):
    """include/ore.h's block rule: (codes uint8 [G, 16 nb], scale bytes uint8 [G, nb])."""
    G, D = x.shape
    nb = -(-D // 32)
    p = np.zeros((G, 32 * nb), np.float32)
    p[:, :D] = x
    p = p.reshape(G, nb, 32)
    with np.errstate(all="ignore"):
        a = np.minimum(np.fmax.reduce(np.abs(p), axis=2, initial=np.float32(0)), np.finfo(np.float32).max)
        b = np.clip((a.view(np.uint32) >> 23).astype(np.int64) - 2, 0, 254)
        m = np.ldexp(np.abs(p).astype(np.float64), (127 - b)[:, :, None])
        c = np.where(m < 2, np.rint(2 * m), np.where(m < 4, 2 + np.rint(m), np.minimum(4 + np.rint(m / 2), 7)))
    c = np.where(np.isnan(p), 0, np.nan_to_num(c).astype(np.uint8) | np.signbit(p).astype(np.uint8) << 3).astype(np.uint8)
    return (c[:, :, 0::2] | c[:, :, 1::2] << 4).reshape(G, 16 * nb), b.astype(np.uint8)


def _pack(ctx, x):
    out = ore.gallery_mxfp4(ctx, torch.from_numpy(np.ascontiguousarray(x)).cuda())
    torch.cuda.synchronize()
    return out


def _bins(ctx, q, codes, scales, B, c):
    qd = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    codes, scales = (x if isinstance(x, torch.Tensor) else torch.from_numpy(x).cuda() for x in (codes, scales))
    v, i = ore.nearest_bins(ctx, qd, codes, c, B, scales=scales)
    torch.cuda.synchronize()
    return v.cpu().numpy().view(np.uint32), i.cpu().numpy()


def _s64(qh, codes, scales, D):  # (float64 scores, sum_d |q^ g^|) of the decoded operands
    g = ore.mxfp4_decode(np.asarray(codes), np.asarray(scales), D).astype(np.float64)
    return qh.astype(np.float64) @ g.T, np.abs(qh).astype(np.float64) @ np.abs(g).T


@pytest.mark.parametrize("D", [1, 31, 32, 33, 512])
def test_packer_bits(gpu_ctx, D, G=67):
    rng = np.random.default_rng(D)
    nb = -(-D // 32)
    x = (rng.standard_normal((G, 32 * nb)) * np.exp2(rng.integers(-20, 21, (G, nb))).repeat(32, axis=1)).astype(np.float32)[:, :D]
    x[1, 0], x[2, D // 2], x[3, D - 1], x[4, 0] = np.nan, np.inf, -np.inf, np.nan
    x[5, :32], x[6, :32] = 0, np.float32(1e-41) * rng.integers(-3, 4, min(D, 32))  # an all-zero and a subnormal-only block
    x[7, :32], x[7, 0] = 0, 4  # scale byte 127: a tie that goes to the even code of 2, a negative that rounds to -0
    if D > 2:
        x[7, 1], x[7, 2] = 2.5, -0.2
    x[4, D - 1] = 3
    codes, scales = _pack(gpu_ctx, x)
    want = quant(x)
    np.testing.assert_array_equal(scales.cpu().numpy(), want[1])
    np.testing.assert_array_equal(codes.cpu().numpy(), want[0])
    dec = ore.mxfp4_decode(codes, scales, D).cpu().numpy()
    assert dec[7, 0] == 4 and dec[5, 0] == 0 and want[1][5, 0] == 0 and (D < 3 or (dec[7, 1] == 2 and dec[7, 2] == 0 and np.signbit(dec[7, 2])))


def _exact_operands(seed, n, G, D):
    """Codes under per-block scales 2^(-2 .. 2) on both sides; a query block starts with a magnitude of 4 or 6, so the
    kernel's quantiser returns exactly these codes and scales.  Any other operand layout or nibble order fails."""
    rng = np.random.default_rng(seed)
    nb = -(-D // 32)

    def side(rows):
        c = rng.integers(0, 16, (rows, 32 * nb)).astype(np.uint8)
        c[:, D:] = 0
        return c, (127 + rng.integers(-2, 3, (rows, nb))).astype(np.uint8)
    cq, tq = side(n)
    cq[:, 0::32] = rng.choice(np.uint8([6, 7, 14, 15]), (n, nb))
    cg, tg = side(G)
    pack = lambda c: c[:, 0::2] | c[:, 1::2] << 4
    return ore.mxfp4_decode(pack(cq), tq, D), pack(cg), tg


# D takes every path: 1, 2 (200) and 4 k-groups with byte (400) and 16-byte (512) scale loads, any number (160, 544, 4096)
@pytest.mark.parametrize("n, G, D, B, c", [
    (1, 1, 1, 32, 1), (17, 127, 33, 32, 4), (65, 129, 128, 128, 1), (17, 4099, 160, 32, 5), (1, 4099, 512, 1024, 5),
    (17, 4099, 200, 128, 33), (17, 4099, 400, 32, 5), (65, 40000, 512, 32, 256), (17, 40000, 544, 128, 5), (1, 4099, 4096, 32, 5)])
def test_exact_with_ties(gpu_ctx, n, G, D, B, c):
    segments, bins = ore.nearest_bins_segments_mxfp4(gpu_ctx, n, G, B)
    assert bins == -(-G // B) and 1 <= segments <= -(-G // (4 * B)) and c <= min(bins, 256)
    assert segments > 1 or G < 40000
    q, cg, tg = _exact_operands(n * G + D, n, G, D)
    s = _s64(q, cg, tg, D)[0]
    assert np.array_equal(s, s.astype(np.float32))
    got, want = _bins(gpu_ctx, q, cg, tg, B, c), bins_ref(s.astype(np.float32), B, c)
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])


@pytest.mark.parametrize("D", [33, 512])
def test_against_float64(gpu_ctx, D):
    q, g = normal(D)
    codes, scales = _pack(gpu_ctx, g)
    qh = ore.mxfp4_decode(*_pack(gpu_ctx, q), D).cpu().numpy()  # the kernel quantises q by the packer's rule
    s, mag = _s64(qh, codes.cpu(), scales.cpu(), D)
    v, i = _bins(gpu_ctx, q, codes, scales, 32, 5)
    err = np.abs(v.view(np.float32).astype(np.float64) - np.take_along_axis(s, i, 1)) / np.take_along_axis(mag, i, 1)
    print(f"mxfp4 D={D}: max error / sum|q^ g^| = {err.max():.3g}")
    assert err.max() <= KAPPA


def _no_tie(s, B, c):
    """per query: no float64 tie among the first c + 1 winners, each alone at its bin's top (FP4 scores are coarse)"""
    v, i = bins_ref(s.astype(np.float32), B, min(c + 1, -(-s.shape[1] // B)))
    top = np.take_along_axis(s, i, 1)
    lo = i // B * B
    alone = np.array([all((s[r, lo[r, k]:lo[r, k] + B] == top[r, k]).sum() == 1 for k in range(i.shape[1])) for r in range(s.shape[0])])
    return alone & (np.diff(top, axis=1) < 0).all(axis=1)


def test_position_independence(gpu_ctx, B=32, c=5):
    (q, g), G = normal(512), 4099
    codes, scales = _pack(gpu_ctx, g)
    qh = ore.mxfp4_decode(*_pack(gpu_ctx, q), 512).cpu().numpy()
    ok = _no_tie(_s64(qh, codes.cpu(), scales.cpu(), 512)[0], B, c)  # a tie may go to another row once the rows move
    assert ok.sum() >= 24
    v, i = _bins(gpu_ctx, q, codes, scales, B, c)
    rng, full = np.random.default_rng(1), G // B  # whole bins move and their rows move inside them; the partial bin stays
    perm = np.concatenate([(B * rng.permutation(full)[:, None] + rng.permuted(np.tile(np.arange(B), (full, 1)), axis=1)).ravel(),
                           np.arange(B * full, G)])
    pm = torch.from_numpy(perm).cuda()
    vp, ip = _bins(gpu_ctx, q, codes[pm].contiguous(), scales[pm].contiguous(), B, c)
    np.testing.assert_array_equal(vp, v)
    np.testing.assert_array_equal(perm[ip][ok], i[ok])
    v7, i7 = _bins(gpu_ctx, q[:7], codes, scales, B, c)
    np.testing.assert_array_equal(v7, v[:7])
    np.testing.assert_array_equal(i7, i[:7])
    c64, t64 = _pack(gpu_ctx, g[:, :64])
    buf = torch.full((q.shape[0] + 1, 80), float("nan"), device="cuda")
    qs = buf[:-1, 5:69]
    qs.copy_(torch.from_numpy(np.ascontiguousarray(q[:, :64])))
    assert qs.stride(0) == 80 and qs.data_ptr() % 16 == 4
    dense, sliced = _bins(gpu_ctx, q[:, :64], c64, t64, B, c), _bins(gpu_ctx, qs, c64, t64, B, c)
    np.testing.assert_array_equal(sliced[0], dense[0])
    np.testing.assert_array_equal(sliced[1], dense[1])


def test_two_stage(gpu_ctx, n=17, G=40000, D=64, k=5, c=64, B=32):
    rng = np.random.default_rng(7)
    centres = rng.standard_normal((64, D)).astype(np.float32)
    g = centres[rng.integers(0, 64, G)] + np.float32(0.5) * rng.standard_normal((G, D)).astype(np.float32)
    q = g[rng.integers(0, G, n)] + np.float32(0.2) * rng.standard_normal((n, D)).astype(np.float32)
    gd, qd = torch.from_numpy(g).cuda(), torch.from_numpy(q).cuda()
    codes, scales = ore.gallery_mxfp4(gpu_ctx, gd)
    exact = ore.nearest(gpu_ctx, qd, gd, k)[1].cpu().numpy()
    qh = ore.mxfp4_decode(*_pack(gpu_ctx, q), D).cpu().numpy()
    cand = bins_ref(_s64(qh, codes.cpu(), scales.cpu(), D)[0].astype(np.float32), B, c)[1]
    kept = np.array([set(exact[r]) <= set(cand[r]) for r in range(n)])  # from the reference alone
    assert kept.mean() >= 0.9
    v, i = ore.nearest(gpu_ctx, qd, codes, k, scales=scales, rerank=gd, candidates=c, bin_rows=B)
    vr, ir = ore.rerank(gpu_ctx, qd, gd, ore.nearest_bins(gpu_ctx, qd, codes, c, B, scales=scales)[1], k)
    assert torch.equal(i, ir) and torch.equal(v.view(torch.int32), vr.view(torch.int32))
    np.testing.assert_array_equal(i.cpu().numpy()[kept], exact[kept])
    with pytest.raises(ore.OreError, match="first stage only"):
        ore.nearest(gpu_ctx, qd, codes, k, scales=scales)
    P, d = ctypes.c_void_p(codes.data_ptr()), ore._lib.Tensor()
    d.data, d.ndim, d.dims[0], d.dims[1] = qd.data_ptr(), 2, 0, D
    assert ore.load().ore_nearest_bins_mxfp4(gpu_ctx.h, ctypes.byref(d), P, ctypes.c_void_p(scales.data_ptr()), G, B, c, P, P) == 0
