"""CPU: the uint8-input entry points (ore_preprocess_u8, ore_model_set_input_norm, ore_model_run_u8,
ore_model_graph_capture_u8) reject null arguments before touching a device, and the binding's flag
mirrors the header.  No kernel is launched here."""
import ctypes
import os
import re

import pytest

import ore
from ore import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID


def _tensor(dims, data=0x1000):
    t = _lib.Tensor()
    t.data = data
    t.ndim = 4
    for i, d in enumerate(dims):
        t.dims[i] = d
    return t


def _fails(status):
    assert status == INVALID
    assert ore.load().ore_last_error(None)  # a message, also without a context


def test_null_model_is_invalid():
    L = ore.load()
    p = ctypes.c_void_p(0x1000)  # never dereferenced: the model is checked first
    _fails(L.ore_model_set_input_norm(None, None, None, 3, 0))
    _fails(L.ore_model_run_u8(None, p, 1, p))
    _fails(L.ore_model_graph_capture_u8(None, p, 1, p))


def test_preprocess_null_arguments_are_invalid():
    L = ore.load()
    p = ctypes.c_void_p(0x1000)
    y = _tensor((1, 3, 4, 4))
    _fails(L.ore_preprocess_u8(None, p, 1, 4, 4, 3, None, None, 0, ctypes.byref(y)))  # no context
    _fails(L.ore_preprocess_u8(None, None, 1, 4, 4, 3, None, None, 0, ctypes.byref(y)))
    _fails(L.ore_preprocess_u8(None, p, 1, 4, 4, 3, None, None, 0, None))
    assert b"null" in L.ore_last_error(None)


def test_flag_matches_header():
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", open(HEADER).read()))
    assert int(defs["ORE_PRE_REVERSE_CHANNELS"]) == ore.PRE_REVERSE_CHANNELS == _lib.PRE_REVERSE_CHANNELS
    assert int(defs["ORE_ABI_VERSION"]) == 2  # the entries were added without an ABI bump
    for name in ("ore_preprocess_u8", "ore_model_set_input_norm", "ore_model_run_u8", "ore_model_graph_capture_u8"):
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)


def test_model_u8_io_checks_host():
    """run_u8_into / capture_u8 hand raw pointers to the walker, so they reject anything but a contiguous
    uint8 CUDA tensor (checked here on CPU tensors, before any device call), as run_into does for float32."""
    import torch
    m = object.__new__(ore.Model)
    m.ctx = type("C", (), {"device": 0})()
    m.input_dims = (3, 8, 8)
    m.output_elems = 10
    m.max_batch = 2
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    out = torch.zeros((2, 10))
    for fn in (m.run_u8_into, m.capture_u8):
        with pytest.raises(ore.OreError, match="uint8 CUDA"):
            fn(x, out)
        with pytest.raises(ore.OreError, match="uint8 CUDA"):
            fn(x.float(), out)
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        m.run_u8(x)
    with pytest.raises(ore.OreError, match="2 values for 3 channels"):
        m.set_input_norm([1.0, 1.0], None)
