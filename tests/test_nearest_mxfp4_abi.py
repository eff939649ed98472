"""CPU: the three MXFP4 entries are exported as include/ore.h declares them and judge their arguments in its order, with
no context and fake pointers that are never dereferenced; the Python messages, and ore.mxfp4_decode() on the host."""
import ctypes
import os
import re

import numpy as np
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


@pytest.mark.parametrize("kw, word", [
    (dict(q=None, scales=None, codes=0x1008, B=0, c=0), b"null"),
    (dict(q=_tensor((2, 0)), scales=None, codes=0x1008, B=0, c=0), b"D, the row length"),
    (dict(q=_tensor((2, 4097)), scales=None, codes=0x1008, B=0, c=0), b"null"),
    (dict(q=_tensor((2, 4097)), codes=0x1008, B=0, c=0), b"D = 4097"),
    (dict(codes=0x1008, B=0, c=0), b"codes"),
    (dict(B=0, c=0), b"bin_rows = 0"), (dict(B=48, c=0), b"bin_rows = 48"),
    (dict(c=0), b"c = 0"), (dict(G=1000, c=9), b"c = 9 outside 1..8"), (dict(c=257), b"c = 257 outside 1..256"),
    (dict(c=256), b"null"),                      # all in range: now the context is missed
    (dict(q=_tensor((0, 4096)), c=256), b"null"),  # and so it is with no queries: n == 0 is no error of the arguments
])
def test_checks_in_order(kw, word):
    a = dict(dict(q=_tensor((2, 512)), codes=0x1000, scales=P, G=100000, B=128, c=5), **kw)
    q = ctypes.byref(a["q"]) if a["q"] is not None else None
    assert L.ore_nearest_bins_mxfp4(None, q, ctypes.c_void_p(a["codes"]), a["scales"], a["G"], a["B"], a["c"], P, P) == INVALID
    assert word in L.ore_last_error(None), L.ore_last_error(None)


def test_exports_and_python_messages():
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "ore.h")) as f:
        declared = set(re.findall(r"^ore_status (\w+)\(", f.read(), re.M))
    assert all(n in declared and n in _lib.EXPORTED and hasattr(L, n)
               for n in ("ore_gallery_mxfp4", "ore_nearest_bins_mxfp4", "ore_nearest_bins_segments_mxfp4"))
    s = ctypes.c_int32()
    assert L.ore_nearest_bins_segments_mxfp4(None, 1, 1, 32, ctypes.byref(s), ctypes.byref(s)) == INVALID
    assert L.ore_gallery_mxfp4(None, P, 1, 1, ctypes.c_void_p(0x1002), P) == INVALID and b"codes" in L.ore_last_error(None)
    ctx = type("C", (), {"h": None, "device": 0})()
    q, codes = torch.zeros((2, 40)), torch.zeros((4, 32), dtype=torch.uint8)
    with pytest.raises(ore.OreError, match="first stage only"):
        ore.nearest(ctx, q, codes, 1, scales=torch.zeros((4, 2), dtype=torch.uint8))
    with pytest.raises(ore.OreError, match="scales: an MXFP4 gallery needs its scale bytes"):
        ore.nearest_bins(ctx, q, codes, 1)
    with pytest.raises(ore.OreError, match=r"scales: expected a contiguous uint8 \[4, 2\]"):
        ore.nearest_bins(ctx, q, codes, 1, scales=torch.zeros((4, 1), dtype=torch.uint8))
    with pytest.raises(ore.OreError, match="rerank: expected the gallery's"):
        ore.nearest(ctx, q, codes, 1, scales=torch.zeros((4, 2), dtype=torch.uint8), rerank=torch.zeros((4, 70)), bin_rows=32)
    codes = np.zeros((1, 32), np.uint8)
    codes[0, :2], codes[0, 16] = [0x21, 0xF9], 0x07
    want = np.zeros((1, 40), np.float32)
    want[0, :4], want[0, 32] = [1, 2, -1, -12], 3  # 0.5, 1, -0.5, -6 under 2^1; 6 under 2^-1
    np.testing.assert_array_equal(ore.mxfp4_decode(codes, np.uint8([[128, 126]]), 40), want)
