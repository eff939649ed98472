"""CPU: ore_gallery_i8, ore_nearest_i8 and ore_nearest_segments_i8 judge their arguments in include/ore.h's order with no
context and fake pointers that are never dereferenced; the Python messages about scales; the definition against float64."""
import ctypes

import numpy as np
import pytest
import torch

import ore
from ore import _lib
from _nearest_i8 import normal, quant, scores

INVALID = 1  # ORE_ERR_INVALID
P, L = ctypes.c_void_p(0x1000), ore.load()


def _tensor(dims, nstride=0):
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = 0x1000, len(dims), nstride
    t.dims[:len(dims)] = dims
    return t


# every case breaks its own rule and every later one too (a null context is the last): the message names the first
@pytest.mark.parametrize("kw, word", [
    (dict(q=None, scales=None, G=0, k=0), b"null"),
    (dict(q=_tensor((2, 8)), gallery=None, G=0, k=0), b"null"),
    (dict(q=_tensor((8,)), scales=None, G=0, k=0), b"dims"),
    (dict(q=_tensor((2, 4, 0, 3), nstride=-1), scales=None, G=0, k=0), b"D, the row length"),
    (dict(q=_tensor((2, 131073), nstride=-1), scales=None, G=0, k=0), b"G = 0"),
    (dict(q=_tensor((2, 131073), nstride=-1), scales=None, G=100, k=65), b"k = 65"),
    (dict(q=_tensor((2, 131073), nstride=7), scales=None, G=100, k=5), b"nstride 7"),
    (dict(q=_tensor((2, 131073)), scales=None, G=100, k=5), b"null"),
    (dict(q=_tensor((2, 131073)), G=100, k=5), b"D = 131073"),
    (dict(q=_tensor((2, 131072)), G=100, k=64), b"null"),  # all in range: now the context is missed
])
def test_nearest_i8_checks_in_order(kw, word):
    a = dict(dict(gallery=P, scales=P, G=100, k=5), **kw)
    st = L.ore_nearest_i8(None, ctypes.byref(a["q"]) if a["q"] is not None else None, a["gallery"], a["scales"], a["G"], a["k"], P, P)
    assert st == INVALID and word in L.ore_last_error(None), L.ore_last_error(None)


@pytest.mark.parametrize("src, G, D, dst, scales, word", [
    (None, 0, 0, P, P, b"null"), (P, 0, 0, None, P, b"null"), (P, 0, 0, P, None, b"null"), (P, 0, 1 << 31, P, P, b"G = 0"),
    (P, 4, 1 << 31, P, P, b"D = 2147483648"), (P, 4, 8, P, P, b"null"),
])
def test_gallery_i8_checks_in_order(src, G, D, dst, scales, word):
    assert L.ore_gallery_i8(None, src, G, D, dst, scales) == INVALID and word in L.ore_last_error(None), L.ore_last_error(None)


def test_segments_entry_binding_and_messages():
    s = ctypes.c_int32()
    assert L.ore_nearest_segments_i8(None, 1, 1, ctypes.byref(s), ctypes.byref(s)) == INVALID
    assert all(name in _lib.EXPORTED and hasattr(L, name) for name in ("ore_gallery_i8", "ore_nearest_i8", "ore_nearest_segments_i8"))
    ctx = type("C", (), {"h": None, "device": 0})()
    q, codes = torch.zeros((2, 8)), torch.zeros((4, 8), dtype=torch.int8)
    with pytest.raises(ore.OreError, match="scales: an int8 gallery needs its scales"):
        ore.nearest(ctx, q, codes, 1)
    for gallery in (torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.float16)):
        with pytest.raises(ore.OreError, match="scales: given with a float(32|16) gallery"):
            ore.nearest(ctx, q, gallery, 1, scales=torch.ones(4))
    for bad in (torch.ones(4, dtype=torch.float64), torch.ones(5), torch.ones((4, 1)), torch.ones(8)[::2]):
        with pytest.raises(ore.OreError, match=r"scales: expected a contiguous float32 \[4\] CUDA tensor"):
            ore.nearest(ctx, q, codes, 1, scales=bad)
    with pytest.raises(ore.OreError, match="q: expected a 2-D float32 CUDA"):  # without scales: the existing messages
        ore.nearest(ctx, q, torch.zeros((4, 8)), 1)
    with pytest.raises(ore.OreError, match="gallery: expected a contiguous, non-empty 2-D float32 CUDA"):
        ore.gallery_i8(ctx, torch.zeros((4, 8)))


@pytest.mark.parametrize("D", [5, 512])
def test_definition_against_float64(D):
    """The restated score lies within 0.51 (tg[j] sum|q_i| + tq[i] sum|g^_j|) + 2^-22 |s64| of the float64 inner product
    of the original rows, g^ the dequantised gallery: half a step per code, and the three float roundings of the score."""
    q, g = normal(D)
    (cq, tq), (cg, tg) = quant(q), quant(g)
    s = scores(cq, tq, cg, tg).astype(np.float64)
    q64, g64, tq64, tg64 = q.astype(np.float64), g.astype(np.float64), tq.astype(np.float64), tg.astype(np.float64)
    s64, ghat = q64 @ g64.T, cg * tg64[:, None]
    bound = 0.51 * (np.abs(q64).sum(1)[:, None] * tg64[None, :] + tq64[:, None] * np.abs(ghat).sum(1)[None, :]) + 2.0 ** -22 * np.abs(s64)
    print(f"D = {D}: max err / bound = {(np.abs(s - s64) / bound).max():.3g}")
    assert (np.abs(s - s64) <= bound).all()
