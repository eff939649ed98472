"""CPU: ore_nearest_bins_f16 / _i8 / _segments judge their arguments in include/ore.h's order with no context and fake
pointers that are never dereferenced; the Python messages of nearest_bins() and of nearest(..., bin_rows=)."""
import ctypes

import pytest
import torch

import ore
from ore import _lib

INVALID = 1  # ORE_ERR_INVALID
P, L = ctypes.c_void_p(0x1000), ore.load()


def _tensor(dims, nstride=0):
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = 0x1000, len(dims), nstride
    t.dims[:len(dims)] = dims
    return t


# every case breaks its own rule and every later one too (a null context is the last): the message names the first
@pytest.mark.parametrize("kw, word", [
    (dict(q=None, scales=None, G=0, B=0, c=0), b"null"),
    (dict(q=_tensor((8,)), scales=None, G=0, B=0, c=0), b"dims"),
    (dict(q=_tensor((2, 131073), nstride=-1), scales=None, G=0, B=0, c=0), b"G = 0"),
    (dict(q=_tensor((2, 131073), nstride=7), scales=None, B=0, c=0), b"nstride 7"),  # no k between G and the stride
    (dict(q=_tensor((2, 131073)), scales=None, B=0, c=0), b"null"),
    (dict(q=_tensor((2, 131073)), B=0, c=0), b"D = 131073"),
    (dict(B=0, c=0), b"bin_rows = 0"), (dict(B=48, c=0), b"bin_rows = 48"), (dict(B=2048, c=0), b"bin_rows = 2048"),
    (dict(c=0), b"c = 0"), (dict(G=1000, c=9), b"c = 9 outside 1..8"), (dict(c=257), b"c = 257 outside 1..256"),
    (dict(c=256), b"null"),  # all in range: now the context is missed
])
def test_nearest_bins_checks_in_order(kw, word):
    a = dict(dict(q=_tensor((2, 512)), gallery=P, scales=P, G=100000, B=128, c=5), **kw)
    q = ctypes.byref(a["q"]) if a["q"] is not None else None
    assert L.ore_nearest_bins_i8(None, q, a["gallery"], a["scales"], a["G"], a["B"], a["c"], P, P) == INVALID
    assert word in L.ore_last_error(None), L.ore_last_error(None)
    if a["scales"] is not None and a["q"] is not None and a["q"].dims[1] <= 131072:  # the f16 entry: the same but for the int8 rules
        assert L.ore_nearest_bins_f16(None, q, a["gallery"], a["G"], a["B"], a["c"], P, P) == INVALID
        assert word in L.ore_last_error(None), L.ore_last_error(None)


def test_bindings_and_python_messages():
    s = ctypes.c_int32()
    assert L.ore_nearest_bins_segments(None, 1, 1, 32, ctypes.byref(s), ctypes.byref(s)) == INVALID
    assert all(name in _lib.EXPORTED and hasattr(L, name) for name in ("ore_nearest_bins_f16", "ore_nearest_bins_i8", "ore_nearest_bins_segments"))
    ctx = type("C", (), {"h": None, "device": 0})()
    q, codes, g16 = torch.zeros((2, 8)), torch.zeros((4, 8), dtype=torch.int8), torch.zeros((4, 8), dtype=torch.float16)
    with pytest.raises(ore.OreError, match=r"gallery: .*gallery_f16\(\), gallery_i8\(\)"):
        ore.nearest_bins(ctx, q, torch.zeros((4, 8)), 1)
    with pytest.raises(ore.OreError, match="scales: an int8 gallery needs its scales"):
        ore.nearest_bins(ctx, q, codes, 1)
    with pytest.raises(ore.OreError, match="q: expected a 2-D float32 CUDA"):  # nearest()'s tensor checks
        ore.nearest_bins(ctx, q, g16, 1)
    with pytest.raises(ore.OreError, match="bin_rows: given without rerank"):
        ore.nearest(ctx, q, g16, 1, bin_rows=32)
    for B in (0, 48, 2048):
        with pytest.raises(ore.OreError, match=f"bin_rows = {B} is no power of two"):
            ore.nearest(ctx, q, g16, 1, rerank=torch.zeros((4, 8)), bin_rows=B)
    with pytest.raises(ore.OreError, match=r"candidates = 2 outside 1\.\.1 \(k\.\.min\(bins, 256\)\)"):
        ore.nearest(ctx, q, g16, 1, rerank=torch.zeros((4, 8)), candidates=2, bin_rows=32)
