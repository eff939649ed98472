"""CPU: ore_gallery_f16, ore_nearest_f16 and ore_nearest_segments_f16 judge their arguments in the order include/ore.h
states, from the arguments alone: no context, fake non-null pointers that are never dereferenced, no launch."""
import ctypes

import pytest

import ore
from ore import _lib

INVALID = 1  # ORE_ERR_INVALID
P = ctypes.c_void_p(0x1000)


def _tensor(dims, data=0x1000, nstride=0):
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = data, len(dims), nstride
    for i, d in enumerate(dims):
        t.dims[i] = d
    return t


# every case breaks its own rule and every later one too (a null context is the last): the message names the first
@pytest.mark.parametrize("kw, word", [
    (dict(q=None, G=0, k=0), b"null"),
    (dict(q=_tensor((2, 8)), gallery=None, G=0, k=0), b"null"),
    (dict(q=_tensor((2, 8)), values=None, G=0, k=0), b"null"),
    (dict(q=_tensor((8,)), G=0, k=0), b"dims"),
    (dict(q=_tensor((2, 4, 0, 3), nstride=-1), G=0, k=0), b"D, the row length"),
    (dict(q=_tensor((2, 8), nstride=-1), G=0, k=0), b"G = 0"),
    (dict(q=_tensor((2, 8), nstride=-1), G=100, k=65), b"k = 65"),
    (dict(q=_tensor((2, 8), nstride=7), G=100, k=5), b"nstride 7"),
    (dict(q=_tensor((2, 8), nstride=12), G=100, k=64), b"null"),  # all in range: now the context is missed
])
def test_nearest_f16_checks_in_order(kw, word):
    a = dict(dict(gallery=P, G=100, k=5, values=P, indices=P), **kw)
    L = ore.load()
    st = L.ore_nearest_f16(None, ctypes.byref(a["q"]) if a["q"] is not None else None, a["gallery"], a["G"], a["k"],
                           a["values"], a["indices"])
    assert st == INVALID and word in L.ore_last_error(None), L.ore_last_error(None)


@pytest.mark.parametrize("src, G, D, dst, word", [
    (None, 0, 0, P, b"null"), (P, 0, 0, None, b"null"), (P, 0, 1 << 31, P, b"G = 0"), (P, 4, 0, P, b"D = 0"),
    (P, 1 << 31, 1 << 31, P, b"G = 2147483648"), (P, 4, 1 << 31, P, b"D = 2147483648"), (P, 4, 8, P, b"null"),
])
def test_gallery_f16_checks_in_order(src, G, D, dst, word):
    L = ore.load()
    assert L.ore_gallery_f16(None, src, G, D, dst) == INVALID and word in L.ore_last_error(None), L.ore_last_error(None)


def test_segments_entry_and_binding():
    L = ore.load()
    s = ctypes.c_int32()
    assert L.ore_nearest_segments_f16(None, 1, 1, ctypes.byref(s), ctypes.byref(s)) == INVALID
    for name in ("ore_gallery_f16", "ore_nearest_f16", "ore_nearest_segments_f16"):
        assert name in _lib.EXPORTED and hasattr(L, name)
    import torch
    ctx = type("C", (), {"h": None, "device": 0})()
    with pytest.raises(ore.OreError, match="q: expected a 2-D float32 CUDA"):  # a float16 gallery leaves q float32
        ore.nearest(ctx, torch.zeros((2, 8)), torch.zeros((4, 8), dtype=torch.float16), 1)
    with pytest.raises(ore.OreError, match="gallery: expected a contiguous, non-empty 2-D float32 CUDA"):
        ore.gallery_f16(ctx, torch.zeros((4, 8)))
