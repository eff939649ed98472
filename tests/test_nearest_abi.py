"""CPU: ore_nearest_f32 and ore_model_set_embed judge their arguments in the order include/ore.h states, from the
arguments alone -- no context and fake non-null pointers that are never dereferenced -- and the binding lists the
new entries.  No kernel is launched here."""
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


def _nearest(q, gallery=P, G=100, k=5, values=P, indices=P):
    L = ore.load()
    st = L.ore_nearest_f32(None, ctypes.byref(q) if q is not None else None, gallery, G, k, values, indices)
    return st, L.ore_last_error(None)


# every case breaks its own rule and every later one too (a null context is the last): the message names the first
@pytest.mark.parametrize("kw, word", [
    (dict(q=None, G=0, k=0), b"null"),
    (dict(q=_tensor((2, 8), data=0), G=0, k=0), b"null"),
    (dict(q=_tensor((2, 8)), gallery=None, G=0, k=0), b"null"),
    (dict(q=_tensor((2, 8)), values=None, G=0, k=0), b"null"),
    (dict(q=_tensor((2, 8)), indices=None, G=0, k=0), b"null"),
    (dict(q=_tensor((8,)), G=0, k=0), b"dims"),
    (dict(q=_tensor((2, 0), nstride=-1), G=0, k=0), b"D, the row length"),
    (dict(q=_tensor((2, 4, 0, 3), nstride=-1), G=0, k=0), b"D, the row length"),
    (dict(q=_tensor((2, 8), nstride=-1), G=0, k=0), b"G = 0"),
    (dict(q=_tensor((2, 8), nstride=-1), G=1 << 31, k=0), b"G = 2147483648"),
    (dict(q=_tensor((2, 8), nstride=-1), G=100, k=0), b"k = 0"),
    (dict(q=_tensor((2, 8), nstride=-1), G=100, k=65), b"k = 65"),
    (dict(q=_tensor((2, 8), nstride=-1), G=3, k=4), b"k = 4 outside 1..3"),
    (dict(q=_tensor((2, 8), nstride=7), G=100, k=5), b"nstride 7"),
    (dict(q=_tensor((2, 8), nstride=(1 << 31) // 2), G=100, k=5), b"nstride"),
    (dict(q=_tensor((2, 8), nstride=12), G=100, k=64), b"null"),  # all in range: now the context is missed
    (dict(q=_tensor((0, 2, 2, 2)), G=(1 << 31) - 1, k=1), b"null"),
])
def test_nearest_checks_in_order(kw, word):
    st, msg = _nearest(**kw)
    assert st == INVALID and word in msg, msg


def test_embed_entries_need_a_model_and_the_binding_lists_them():
    L = ore.load()
    dim = ctypes.c_int64()
    for st in (L.ore_model_set_embed(None, P, 10, _lib.EMBED_L2), L.ore_model_set_embed(None, None, 0, 0),
               L.ore_model_embed_dim(None, ctypes.byref(dim)), L.ore_nearest_segments(None, 1, 1, None)):
        assert st == INVALID and b"null" in L.ore_last_error(None)
    for name in ("ore_nearest_f32", "ore_nearest_segments", "ore_model_embed_dim", "ore_model_set_embed"):
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert ore.EMBED_L2 == 1 and callable(ore.nearest) and callable(ore.Model.classify_embed)


def test_nearest_host_checks():
    import torch
    ctx = type("C", (), {"h": None, "device": 0})()
    with pytest.raises(ore.OreError, match="q: expected a 2-D float32 CUDA"):
        ore.nearest(ctx, torch.zeros((2, 8)), torch.zeros((4, 8)), 1)
