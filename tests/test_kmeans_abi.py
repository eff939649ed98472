"""CPU: ore_kmeans_step_f32 judges its arguments in the order include/ore.h states, from the arguments alone (no
context, fake pointers that are never dereferenced), and ore.kmeans_step refuses its tensors before the library."""
import ctypes

import pytest
import torch

import ore
from ore import _lib
from test_abi import declared_functions
from test_nearest_abi import P, _tensor

BAD = _tensor((2, 8), nstride=7)  # breaks the last rule before the context


# every case breaks its own rule and every later one too (a null context is the last): the message names the first
@pytest.mark.parametrize("kw, word", [
    (dict(x=None, L=0), b"null"), (dict(x=_tensor((1 << 31, 0), data=0), L=0), b"null"), (dict(centroids=None, L=0), b"null"),
    (dict(out=None, L=0), b"null"), (dict(assign=None, L=0), b"null"), (dict(counts=None, L=0), b"null"),
    (dict(x=_tensor((8,)), L=0), b"dims"), (dict(x=_tensor((1 << 31, 0)), L=0), b"D = 0"),
    (dict(x=_tensor((1 << 31, 513)), L=0), b"D = 513"), (dict(x=_tensor(((1 << 31) - 64, 8), nstride=7), L=0), b"S = 2147483584"),
    (dict(x=BAD, L=0), b"L = 0"), (dict(x=BAD, L=65537), b"L = 65537"), (dict(x=BAD), b"nstride 7"),
    (dict(x=_tensor(((1 << 31) - 65, 512), nstride=0), L=65536, scores=None), b"null"),  # all in range: the context is missed
    (dict(x=_tensor((0, 2, 2, 2))), b"null")])
def test_kmeans_checks_in_order(kw, word):
    L = ore.load()
    a = dict(dict(x=_tensor((2, 8)), centroids=P, L=4, out=P, assign=P, scores=P, counts=P), **kw)
    st = L.ore_kmeans_step_f32(None, ctypes.byref(a["x"]) if a["x"] is not None else None, a["centroids"], a["L"], a["out"], a["assign"],
                               a["scores"], a["counts"])
    assert st == 1 and word in L.ore_last_error(None), L.ore_last_error(None)
    assert "ore_kmeans_step_f32" in _lib.EXPORTED and "ore_kmeans_step_f32" in declared_functions()
    assert (ore.KMEANS_MAX_D, ore.KMEANS_MAX_L) == (512, 65536)


def test_kmeans_host_messages():
    ctx = type("C", (), {"h": None, "device": 0})()
    with pytest.raises(ore.OreError, match="x: expected a 2-D float32 CUDA"):
        ore.kmeans_step(ctx, torch.zeros((2, 8)), torch.zeros((4, 8)))
    with pytest.raises(ore.OreError, match=r"centroids: expected a contiguous \[L, 8\]"):
        ore.kmeans_step(ctx, torch.zeros((2, 8)), torch.zeros((4, 7)))
    with pytest.raises(ore.OreError, match="x: expected a 2-D float32 CUDA"):
        ore.ivf_train(ctx, torch.zeros((9, 8)), 4, iters=1)
