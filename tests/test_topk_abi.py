"""CPU: the top-k entry points (ore_topk_f32, ore_model_set_topk, ore_model_classify, _classify_u8,
ore_model_graph_capture_classify, _capture_classify_u8) reject null arguments and a k out of range before
touching a device, and the binding lists them.  No kernel is launched here."""
import ctypes
import os
import re

import pytest

import ore
from ore import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID
NAMES = ("ore_topk_f32", "ore_model_set_topk", "ore_model_classify", "ore_model_classify_u8",
         "ore_model_graph_capture_classify", "ore_model_graph_capture_classify_u8")


def _tensor(dims, data=0x1000):
    t = _lib.Tensor()
    t.data = data
    t.ndim = len(dims)
    for i, d in enumerate(dims):
        t.dims[i] = d
    return t


def _fails(status):
    assert status == INVALID
    assert ore.load().ore_last_error(None)  # a message, also without a context


def test_null_model_is_invalid():
    L = ore.load()
    p = ctypes.c_void_p(0x1000)  # never dereferenced: the model is checked first
    _fails(L.ore_model_set_topk(None, 1))
    assert b"null" in L.ore_last_error(None)
    for entry in (L.ore_model_classify, L.ore_model_classify_u8, L.ore_model_graph_capture_classify,
                  L.ore_model_graph_capture_classify_u8):
        _fails(entry(None, p, 1, p, p))
        _fails(entry(None, p, 1, p, None))  # ... and a null classes pointer with it
        assert b"null" in L.ore_last_error(None)


def test_topk_null_arguments_are_invalid():
    L = ore.load()
    p = ctypes.c_void_p(0x1000)
    x = _tensor((2, 10))
    _fails(L.ore_topk_f32(None, ctypes.byref(x), 1, p, p))  # no context
    _fails(L.ore_topk_f32(None, None, 1, p, p))
    assert b"null" in L.ore_last_error(None)


def test_topk_k_range_is_checked_before_any_device_call():
    """No context and fake non-null pointers that are never dereferenced: the answer names k, so the range
    was judged from the tensor's dims alone, before the context or the device was needed."""
    L = ore.load()
    p = ctypes.c_void_p(0x1000)
    x = _tensor((2, 10))
    for k in (0, -1, 11, 65):
        _fails(L.ore_topk_f32(None, ctypes.byref(x), k, p, p))
        assert b"top-k k" in L.ore_last_error(None)
    _fails(L.ore_topk_f32(None, ctypes.byref(_tensor((2, 5, 20))), 65, p, p))  # k <= D = 100 but above 64
    assert b"top-k k" in L.ore_last_error(None)
    _fails(L.ore_topk_f32(None, ctypes.byref(_tensor((2, 5, 20))), 64, p, p))  # in range: now the context is missed
    assert b"null" in L.ore_last_error(None)
    for args in ((None, p), (p, None)):
        _fails(L.ore_topk_f32(None, ctypes.byref(x), 1, *args))
        assert b"null" in L.ore_last_error(None)
    _fails(L.ore_topk_f32(None, ctypes.byref(_tensor((2, 10), data=0)), 1, p, p))
    assert b"null" in L.ore_last_error(None)


def test_names_and_abi_version():
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", open(HEADER).read()))
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.ABI_VERSION  # the entries were added without an ABI bump
    for name in NAMES:
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)
    assert callable(ore.topk)


def _host_model(k=5):
    m = object.__new__(ore.Model)
    m.ctx = type("C", (), {"device": 0})()
    m.input_dims = (3, 8, 8)
    m.output_elems = 10
    m.max_batch = 2
    m.topk = k
    return m


def test_model_classify_io_checks_host():
    """classify*_into / capture_classify* hand raw pointers to the walker, so they reject anything but
    contiguous CUDA tensors of the right dtype (checked here on CPU tensors, before any device call)."""
    import torch
    m = _host_model()
    xf = torch.zeros((2, 3, 8, 8))
    x8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    scores = torch.zeros((2, 5))
    classes = torch.zeros((2, 5), dtype=torch.int32)
    for fn in (m.classify_into, m.capture_classify):
        with pytest.raises(ore.OreError, match="x: expected a float32 CUDA"):
            fn(xf, scores, classes)
        with pytest.raises(ore.OreError, match="x: expected a float32 CUDA"):
            fn(x8, scores, classes)
    for fn in (m.classify_u8_into, m.capture_classify_u8):
        with pytest.raises(ore.OreError, match="uint8 CUDA"):
            fn(x8, scores, classes)
        with pytest.raises(ore.OreError, match="uint8 CUDA"):
            fn(xf, scores, classes)
    with pytest.raises(ore.OreError, match="float32 CUDA"):
        m.classify(xf)
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        m.classify_u8(x8)


def test_model_classify_output_checks_host():
    import torch
    m = _host_model()
    scores = torch.zeros((2, 5))
    classes = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(ore.OreError, match="scores: expected a float32 CUDA"):
        m._check_classify_out(2, scores, classes)
    with pytest.raises(ore.OreError, match="scores: expected a float32 CUDA"):
        m._check_classify_out(2, scores.double(), classes)
    with pytest.raises(ore.OreError, match="1..10"):  # set_topk's range is min(output elems, 64)
        m.set_topk(11)
    with pytest.raises(ore.OreError, match="1..10"):
        m.set_topk(0)
    assert m.topk == 5
