"""CPU: ore_nearest_lists_f16 judges its arguments in the order include/ore.h states, from the arguments alone (no
context, fake pointers that are never dereferenced); ore_ivf_chunks against a restatement in Python."""
import ctypes

import numpy as np
import pytest
import torch

import ore
from ore import _lib
from test_nearest_abi import P, _tensor

R = ore.IVF_CHUNK_ROWS


# every case breaks its own rule and every later one too (a null context is the last): the message names the first
@pytest.mark.parametrize("kw, word", [
    (dict(q=None, G=0, k=0, L=0), b"null"), (dict(gallery=None, G=0, k=0, L=0), b"null"), (dict(values=None, G=0, L=0), b"null"),
    (dict(indices=None, G=0, L=0), b"null"), (dict(q=_tensor((8,)), G=0, k=0, L=0), b"dims"), (dict(G=0, k=0, L=0), b"G = 0"),
    (dict(k=0, L=0), b"k = 0"), (dict(k=65, L=0), b"k = 65"), (dict(q=_tensor((2, 8), nstride=7), L=0), b"nstride 7"),
    (dict(q=_tensor((2, 513)), offsets=None, L=0), b"D = 513"), (dict(offsets=None, L=0), b"offsets"),
    (dict(L=0, chunks=None), b"L = 0"), (dict(chunks=None, n_chunks=0), b"chunks"),
    (dict(n_chunks=0, rows=0), b"n_chunks = 0"), (dict(n_chunks=1000 // R + 4 + 1, rows=0), b"n_chunks"),
    (dict(rows=0, probes=None), b"max_list_rows = 0"), (dict(rows=1001, probes=None), b"max_list_rows = 1001"),
    (dict(probes=None, stride=0), b"probes"), (dict(stride=0, Pn=0), b"probe_stride = 0"), (dict(Pn=0), b"P = 0"),
    (dict(Pn=65, stride=100), b"P = 65"), (dict(Pn=9, stride=8), b"P = 9 outside 1..8"),
    (dict(q=_tensor(((1 << 31) - 1, 8)), Pn=2), b"n P"),
    (dict(q=_tensor((2, 512), nstride=600), Pn=64, stride=1 << 20, k=64), b"null"),  # all in range: the context is missed
    (dict(q=_tensor((0, 2, 2, 2))), b"null")])
def test_lists_checks_in_order(kw, word):
    L = ore.load()
    a = dict(dict(q=_tensor((2, 8)), gallery=P, G=1000, offsets=P, L=4, chunks=P, n_chunks=5, rows=300, probes=P, stride=8, Pn=3,
                  k=5, values=P, indices=P), **kw)
    st = L.ore_nearest_lists_f16(None, ctypes.byref(a["q"]) if a["q"] is not None else None, a["gallery"], a["G"], a["offsets"], a["L"],
                                 a["chunks"], a["n_chunks"], a["rows"], a["probes"], a["stride"], a["Pn"], a["k"], a["values"], a["indices"])
    assert st == 1 and word in L.ore_last_error(None) and "ore_nearest_lists_f16" in _lib.EXPORTED, L.ore_last_error(None)


def test_ivf_chunks():
    """empty lists, a list of exactly R rows and one of R + 1; the count-only call; offsets that are no offsets"""
    sizes = [0, 5, R, 0, R + 1, 3 * R + 7, 0]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    want = [(l, r) for l in range(len(sizes)) for r in range(offsets[l], offsets[l + 1], R)]
    assert len(want) <= offsets[-1] // R + len(sizes)
    got = ore.ivf_chunks(torch.from_numpy(offsets))
    assert got.dtype == torch.int32 and got.tolist() == [list(w) for w in want]
    L, count = ore.load(), ctypes.c_int32(-1)
    assert L.ore_ivf_chunks(offsets.ctypes.data, len(sizes), None, ctypes.byref(count)) == 0 and count.value == len(want)
    for bad, word in ((np.array([1, 2], np.int32), b"offsets[0]"), (np.array([0, 5, 4], np.int32), b"offsets[2] = 4 below")):
        assert L.ore_ivf_chunks(bad.ctypes.data, len(bad) - 1, None, ctypes.byref(count)) == 1 and word in L.ore_last_error(None)
    assert L.ore_ivf_chunks(None, 1, None, ctypes.byref(count)) == 1 and L.ore_ivf_chunks(offsets.ctypes.data, 0, None, ctypes.byref(count)) == 1


def test_lists_host_messages():
    ctx = type("C", (), {"h": None, "device": 0})()
    with pytest.raises(ore.OreError, match="q: expected a 2-D float32 CUDA"):
        ore.nearest_lists(ctx, torch.zeros((2, 8)), None, None, None, None, 5, 1)
    with pytest.raises(ore.OreError, match="offsets: expected a 1-D int32 CPU"):
        ore.ivf_chunks(torch.zeros(3))
