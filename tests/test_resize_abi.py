"""CPU: the resize entry points (ore_resize_taps, ore_preprocess_resize_u8, ore_model_set_input_resize) are
exported, the binding's flag mirrors the header, and every argument check answers ORE_ERR_INVALID with a
message before any device call.  No kernel is launched here."""
import ctypes
import os
import re

import pytest

import ore
from ore import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID
P = ctypes.c_void_p(0x1000)  # never dereferenced: the checks come first


def _tensor(dims, data=0x1000, nstride=0):
    t = _lib.Tensor()
    t.data = data
    t.ndim = 4
    for i, d in enumerate(dims):
        t.dims[i] = d
    t.nstride = nstride
    return t


def _fails(status, word=None):
    assert status == INVALID
    msg = ore.load().ore_last_error(None)
    assert msg  # a message, also without a context
    if word:
        assert word in msg, msg


def test_exports_and_flags():
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", open(HEADER).read()))
    assert int(defs["ORE_PRE_REVERSE_CHANNELS"]) == ore.PRE_REVERSE_CHANNELS == 1
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.load().ore_abi_version()  # added without an ABI bump
    for name in ("ore_resize_taps", "ore_preprocess_resize_u8", "ore_model_set_input_resize"):
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)
    assert ctypes.sizeof(_lib.Resize) == 32


def test_null_arguments_are_invalid():
    L = ore.load()
    g = _lib.Resize(8, 8, 0, 0)
    y = _tensor((1, 3, 4, 4))
    _fails(L.ore_model_set_input_resize(None, 8, 8, ctypes.byref(g)), b"null")
    _fails(L.ore_model_set_input_resize(None, 8, 8, None), b"null")
    _fails(L.ore_preprocess_resize_u8(None, P, 1, 8, 8, 3, ctypes.byref(g), None, None, 0, ctypes.byref(y)), b"null")
    i0, t = (ctypes.c_int32 * 4)(), (ctypes.c_float * 4)()
    _fails(L.ore_resize_taps(8, 4, 0, 4, None, i0, t), b"null")
    _fails(L.ore_resize_taps(8, 4, 0, 4, i0, None, t), b"null")
    _fails(L.ore_resize_taps(8, 4, 0, 4, i0, i0, None), b"null")


def test_taps_argument_checks():
    for src, resized, origin, count in [(0, 4, 0, 4), (8, 0, 0, 1), (16385, 4, 0, 4), (8, 16385, 0, 4), (8, 4, -1, 2),
                                        (8, 4, 2, 3), (8, 4, 4, 1), (8, 4, 0, 0), (8, 4, 0, -1), (8, 4, 0, 5),
                                        (8, 4, 1 << 62, 1 << 62)]:
        with pytest.raises(ore.OreError, match="resize taps"):
            ore.resize_taps(src, resized, origin, count)
    i0, i1, t = ore.resize_taps(16384, 16384, 16383, 1)
    assert (int(i0[0]), int(i1[0]), float(t[0])) == (16383, 16383, 0.0)


def _call(g, hs=8, ws=8, c=3, n=1, ydims=(1, 3, 4, 4), flags=0, nstride=0):
    """ore_preprocess_resize_u8 without a context: the pointers and the geometry are checked first, so a bad
    geometry is reported as such and a good one ends at "null context", all before any device call."""
    y = _tensor(ydims, nstride=nstride)
    return ore.load().ore_preprocess_resize_u8(None, P, n, hs, ws, c, ctypes.byref(_lib.Resize(*g)), None, None, flags,
                                               ctypes.byref(y))


def test_geometry_checks_before_any_device_call():
    _fails(_call((8, 8, 0, 0)), b"null context")  # a valid call: only the context is missing
    _fails(_call((8, 8, 4, 4)), b"null context")
    _fails(_call((16384, 16384, 16380, 16380), hs=16384, ws=16384), b"null context")
    _fails(_call((8, 8, 0, 0), flags=ore.PRE_REVERSE_CHANNELS), b"null context")
    _fails(_call((8, 8, 0, 0), nstride=3 * 4 * 4 + 3), b"null context")
    # a crop outside the resized image
    for g in [(8, 8, 5, 0), (8, 8, 0, 5), (8, 8, -1, 0), (8, 8, 0, -1), (3, 8, 0, 0), (8, 3, 0, 0), (8, 8, 1 << 62, 0)]:
        _fails(_call(g), b"outside")
    # a size above 16384, a size of 0
    _fails(_call((8, 8, 0, 0), hs=16385), b"1..16384")
    _fails(_call((8, 8, 0, 0), ws=16385), b"1..16384")
    _fails(_call((16385, 8, 0, 0)), b"1..16384")
    _fails(_call((8, 16385, 0, 0)), b"1..16384")
    _fails(_call((8, 8, 0, 0), hs=0), b"1..16384")
    _fails(_call((8, 8, 0, 0), ws=0), b"1..16384")
    _fails(_call((0, 8, 0, 0)), b"1..16384")
    _fails(_call((8, 0, 0, 0)), b"1..16384")
    _fails(_call((8, 8, 0, 0), ydims=(1, 3, 0, 4)), b"image of")
    _fails(_call((8, 8, 0, 0), ydims=(1, 3, 4, 0)), b"image of")
    # channels, flags, the output view, the batch
    _fails(_call((8, 8, 0, 0), c=5, ydims=(1, 5, 4, 4)), b"channels")
    _fails(_call((8, 8, 0, 0), c=0, ydims=(1, 0, 4, 4)), b"channels")
    _fails(_call((8, 8, 0, 0), flags=4), b"flags")
    _fails(_call((8, 8, 0, 0), flags=2), b"flags")
    _fails(_call((8, 8, 0, 0), c=1, ydims=(1, 1, 4, 4), flags=ore.PRE_REVERSE_CHANNELS), b"3 channels")
    _fails(_call((8, 8, 0, 0), ydims=(2, 3, 4, 4)), b"[n,c,H,W]")
    _fails(_call((8, 8, 0, 0), ydims=(1, 4, 4, 4)), b"[n,c,H,W]")
    _fails(_call((8, 8, 0, 0), nstride=3 * 4 * 4 - 1), b"stride")
    _fails(_call((8, 8, 0, 0), n=-1, ydims=(-1, 3, 4, 4)), b"negative")
    # null pointers
    L = ore.load()
    y = _tensor((1, 3, 4, 4))
    g = _lib.Resize(8, 8, 0, 0)
    _fails(L.ore_preprocess_resize_u8(None, None, 1, 8, 8, 3, ctypes.byref(g), None, None, 0, ctypes.byref(y)), b"null argument")
    _fails(L.ore_preprocess_resize_u8(None, P, 1, 8, 8, 3, None, None, None, 0, ctypes.byref(y)), b"null argument")
    _fails(L.ore_preprocess_resize_u8(None, P, 1, 8, 8, 3, ctypes.byref(g), None, None, 0, None), b"null argument")
    _fails(L.ore_preprocess_resize_u8(None, P, 1, 8, 8, 3, ctypes.byref(g), None, None, 0,
                                      ctypes.byref(_tensor((1, 3, 4, 4), data=0))), b"null argument")


def test_python_checks_host():
    """preprocess_resize_u8 / Model.set_input_resize / the _u8 entries reject on the host what they would
    hand to the library as raw pointers (on the pattern of test_model_u8_io_checks_host)."""
    import torch
    ctx = type("C", (), {"device": 0, "h": None})()
    x = torch.zeros((2, 9, 12, 3), dtype=torch.uint8)
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        ore.preprocess_resize_u8(ctx, x, (4, 4))
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        ore.preprocess_resize_u8(ctx, x.float(), (4, 4))
    m = object.__new__(ore.Model)
    m.ctx = ctx
    m.input_dims = (3, 8, 8)
    m.output_elems = 10
    m.max_batch = 2
    m.topk = 1
    m.input_src_hw = (9, 12)
    out = torch.zeros((2, 10))
    for fn in (m.run_u8_into, m.capture_u8):
        with pytest.raises(ore.OreError, match="uint8 CUDA"):
            fn(x, out)
    # the size the entries compare against is the source's once a resize is set, the model's otherwise
    assert m._check_u8_dims(x) == 2
    with pytest.raises(ore.OreError, match="source size"):
        m._check_u8_dims(torch.zeros((2, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(ore.OreError, match="source size"):
        m._check_u8_dims(torch.zeros((2, 9, 12, 4), dtype=torch.uint8))
    m.input_src_hw = None
    assert m._check_u8_dims(torch.zeros((1, 8, 8, 3), dtype=torch.uint8)) == 1
    with pytest.raises(ore.OreError, match="model"):
        m._check_u8_dims(x)
