"""CPU: ore_nearest_rerank_f32 / _f16 judge their arguments in the order include/ore.h states, from the arguments alone
(no context, fake pointers that are never dereferenced), and ore.rerank / ore.nearest name the argument they refuse."""
import ctypes

import pytest

import ore
from ore import _lib
from test_nearest_abi import P, _tensor


# every case breaks its own rule and every later one too (a null context is the last): the message names the first
@pytest.mark.parametrize("entry", ["ore_nearest_rerank_f32", "ore_nearest_rerank_f16"])
@pytest.mark.parametrize("kw, word", [
    (dict(q=None, G=0, C=0, k=0), b"null"), (dict(q=_tensor((2, 8), data=0), G=0, C=0, k=0), b"null"),
    (dict(gallery=None, G=0, C=0, k=0), b"null"), (dict(cand=None, G=0, C=0, k=0), b"null"),
    (dict(values=None, G=0, C=0, k=0), b"null"), (dict(indices=None, G=0, C=0, k=0), b"null"),
    (dict(q=_tensor((8,)), G=0, C=0, k=0), b"dims"), (dict(q=_tensor((2, 4, 0, 3), nstride=-1), G=0, C=0, k=0), b"D, the row length"),
    (dict(G=0, C=0, k=0), b"G = 0"), (dict(G=1 << 31, C=0, k=0), b"G = 2147483648"),
    (dict(C=0, stride=-1, k=0), b"C = 0"), (dict(C=257, stride=256, k=0), b"C = 257"),
    (dict(C=32, stride=31, k=0), b"cand_stride 31"), (dict(C=32, stride=32, k=0), b"k = 0"),
    (dict(C=256, stride=256, k=65), b"k = 65"), (dict(G=1, C=3, stride=3, k=4), b"k = 4 outside 1..3"),
    (dict(q=_tensor((2, 8), nstride=7), C=32, stride=40, k=32), b"nstride 7"),
    (dict(q=_tensor((2, 8), nstride=12), G=1, C=256, stride=1 << 40, k=64), b"null"),  # all in range: the context is missed
    (dict(q=_tensor((0, 2, 2, 2)), G=(1 << 31) - 1, C=1, stride=1, k=1), b"null")])
def test_rerank_checks_in_order(entry, kw, word):
    L = ore.load()
    a = dict(dict(q=_tensor((2, 8), nstride=-1), gallery=P, G=100, cand=P, stride=0, C=32, k=5, values=P, indices=P), **kw)
    st = getattr(L, entry)(None, ctypes.byref(a["q"]) if a["q"] is not None else None, a["gallery"], a["G"], a["cand"],
                           a["stride"], a["C"], a["k"], a["values"], a["indices"])
    assert st == 1 and word in L.ore_last_error(None) and entry in _lib.EXPORTED, L.ore_last_error(None)  # ORE_ERR_INVALID


def test_rerank_host_messages():
    import torch
    ctx = type("C", (), {"h": None, "device": 0})()
    q, g = torch.zeros((2, 8)), torch.zeros((100, 8))
    for kw, msg in ((dict(candidates=8), "candidates: given without rerank"),
                    (dict(rerank=torch.zeros((100, 8), dtype=torch.int8)), "rerank: expected a 2-D float32 or float16"),
                    (dict(rerank=torch.zeros((99, 8))), r"rerank: expected the gallery's \[G, D\]"),
                    (dict(rerank=g, candidates=65), r"candidates = 65 outside 5\.\.64"),
                    (dict(rerank=g), "q: expected a 2-D float32 CUDA")):  # the default 40 passes; the search's checks follow
        with pytest.raises(ore.OreError, match=msg):
            ore.nearest(ctx, q, g, 5, **kw)
    with pytest.raises(ore.OreError, match="q: expected a 2-D float32 CUDA"):
        ore.rerank(ctx, q, g, torch.zeros((2, 8), dtype=torch.int32), 5)
