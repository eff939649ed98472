"""CPU: the image-list entry points (ore_image_check, ore_image_list_*, ore_preprocess_list_u8 and the model's
_u8_list entries) are exported, the descriptor is 64 bytes, and every host check answers ORE_ERR_INVALID with a
message before any device call (on the pattern of tests/test_resize_abi.py).  No kernel is launched here."""
import ctypes
import os
import re

import pytest

import ore
from ore import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID
P = 0x1000  # never dereferenced: ore_image_check is host only

NEW = ["ore_image_check", "ore_image_list_create", "ore_image_list_destroy", "ore_image_list_set", "ore_image_list_count",
       "ore_preprocess_list_u8", "ore_model_run_u8_list", "ore_model_classify_u8_list", "ore_model_graph_capture_u8_list",
       "ore_model_graph_capture_classify_u8_list"]


def _img(hs=8, ws=8, row_stride=0, g=(8, 8, 0, 0), data=P):
    d = _lib.ImageU8()
    d.data = data
    d.hs, d.ws, d.row_stride = hs, ws, row_stride
    d.g = _lib.Resize(*g)
    return d


def _check(imgs, c=3, h=4, w=4, n=None):
    """ore_image_check -> (status, bad_index, message); bad_index stays -7 where the library does not set it."""
    arr = (_lib.ImageU8 * max(len(imgs), 1))(*imgs)
    bad = ctypes.c_int64(-7)
    st = ore.load().ore_image_check(arr, len(imgs) if n is None else n, c, h, w, ctypes.byref(bad))
    return st, bad.value, ore.load().ore_last_error(None)


def _ok(img, **kw):
    st, bad, msg = _check([img], **kw)
    assert st == 0 and bad == -7, msg


def _bad(img, word, **kw):
    st, bad, msg = _check([img], **kw)
    assert st == INVALID and bad == 0
    assert msg and word in msg and b"image 0" in msg, msg


def test_exports_and_descriptor_size():
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", open(HEADER).read()))
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.load().ore_abi_version() == ore.ABI_VERSION  # added without an ABI bump
    assert len(NEW) == 10
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)
    assert ctypes.sizeof(_lib.ImageU8) == 64
    for name in ("ImageList", "preprocess_list_u8"):
        assert hasattr(ore, name)
    for name in ("run_u8_list", "run_u8_list_into", "classify_u8_list", "classify_u8_list_into", "capture_u8_list",
                 "capture_classify_u8_list"):
        assert hasattr(ore.Model, name)


def test_image_check_accepts():
    _ok(_img())
    _ok(_img(row_stride=0))
    _ok(_img(row_stride=24))            # exactly ws*c
    _ok(_img(row_stride=4096))
    _ok(_img(g=(8, 8, 4, 4)))           # the crop at the far corner
    _ok(_img(16384, 16384, 0, (16384, 16384, 16380, 16380)), c=4)  # 2^30 bytes, dense
    _ok(_img(16384, 16384, 65536, (16384, 16384, 0, 0)), c=4)


def test_image_check_rejects():
    _bad(_img(data=None), b"null")
    for kw in (dict(hs=0), dict(ws=0), dict(g=(0, 8, 0, 0)), dict(g=(8, 0, 0, 0)),
               dict(hs=16385), dict(ws=16385), dict(g=(16385, 8, 0, 0)), dict(g=(8, 16385, 0, 0))):
        _bad(_img(**kw), b"1..16384")
    # a crop outside the resized image: the tuples of test_geometry_checks_before_any_device_call
    for g in [(8, 8, 5, 0), (8, 8, 0, 5), (8, 8, -1, 0), (8, 8, 0, -1), (3, 8, 0, 0), (8, 3, 0, 0), (8, 8, 1 << 62, 0)]:
        _bad(_img(g=g), b"outside")
    _bad(_img(row_stride=8 * 3 - 1), b"row stride")
    _bad(_img(row_stride=-24), b"row stride")
    _bad(_img(row_stride=-(1 << 62)), b"row stride")
    _bad(_img(row_stride=1 << 62), b"2^31")
    # the output shape and the channel count are the list's, checked once
    for kw in (dict(c=0), dict(c=5)):
        st, _, msg = _check([_img()], **kw)
        assert st == INVALID and b"channels" in msg
    for kw in (dict(h=0), dict(w=0)):
        st, _, msg = _check([_img()], **kw)
        assert st == INVALID and b"image of" in msg


def test_image_check_extent_bound():
    """(hs-1)*row_stride + ws*c must stay below 2^31: rejected at 2^31 exactly, accepted one byte below."""
    for hs, ws, c, g in [(2, 1, 1, (4, 4, 0, 0)), (2, 8, 3, (4, 4, 0, 0)), (16384, 16384, 4, (4, 4, 0, 0)), (1025, 7, 3, (4, 4, 0, 0))]:
        rows = hs - 1
        stride = ((1 << 31) - ws * c) // rows  # the largest with rows * stride + ws*c <= 2^31
        if rows * stride + ws * c == 1 << 31:
            _bad(_img(hs, ws, stride, g), b"2^31", c=c)
            _ok(_img(hs, ws, stride - 1, g), c=c)
        else:
            assert rows * stride + ws * c < 1 << 31 < rows * (stride + 1) + ws * c
            _ok(_img(hs, ws, stride, g), c=c)
            _bad(_img(hs, ws, stride + 1, g), b"2^31", c=c)
    # the exact pair the bound is stated with: one row step of 2^31 - 1 bytes plus one byte, and one byte less
    _bad(_img(2, 1, (1 << 31) - 1, (4, 4, 0, 0)), b"2^31", c=1)
    _ok(_img(2, 1, (1 << 31) - 2, (4, 4, 0, 0)), c=1)
    # a one-row image never steps a row
    _ok(_img(1, 8, 1 << 40, (4, 4, 0, 0)))


def test_bad_index_is_the_first_bad_descriptor():
    good = _img()
    st, bad, msg = _check([good, good, _img(g=(8, 8, 5, 0)), good, _img(hs=0)])
    assert st == INVALID and bad == 2 and b"image 2" in msg and b"outside" in msg
    st, bad, msg = _check([good, good, good, _img(data=None)])
    assert st == INVALID and bad == 3 and b"image 3" in msg
    st, bad, _ = _check([good, good, good])
    assert st == 0 and bad == -7
    # a null bad_index is allowed
    arr = (_lib.ImageU8 * 2)(good, _img(ws=0))
    assert ore.load().ore_image_check(arr, 2, 3, 4, 4, None) == INVALID
    assert ore.load().ore_image_check(arr, 1, 3, 4, 4, None) == 0


def test_empty_and_null_lists():
    L = ore.load()
    assert L.ore_image_check(None, 0, 3, 4, 4, None) == 0
    st, bad, _ = _check([], n=0)
    assert st == 0 and bad == -7
    assert L.ore_image_check(None, 1, 3, 4, 4, None) == INVALID and b"null" in L.ore_last_error(None)
    assert L.ore_image_check(None, -1, 3, 4, 4, None) == INVALID


def _fails_null(status):
    assert status == INVALID
    msg = ore.load().ore_last_error(None)
    assert msg and b"null" in msg, msg


def test_null_arguments_are_invalid():
    L = ore.load()
    q = ctypes.c_void_p(P)
    y = _lib.Tensor()
    y.data, y.ndim = P, 4
    out = ctypes.c_void_p()
    _fails_null(L.ore_image_list_create(None, 4, 3, 4, 4, ctypes.byref(out)))
    assert not out.value
    _fails_null(L.ore_image_list_set(None, (_lib.ImageU8 * 1)(_img()), 1))
    _fails_null(L.ore_preprocess_list_u8(None, None, None, None, 0, ctypes.byref(y)))
    _fails_null(L.ore_model_run_u8_list(None, None, q))
    _fails_null(L.ore_model_classify_u8_list(None, None, q, q))
    _fails_null(L.ore_model_classify_u8_list(None, None, q, None))
    _fails_null(L.ore_model_graph_capture_u8_list(None, None, q))
    _fails_null(L.ore_model_graph_capture_classify_u8_list(None, None, q, q))
    _fails_null(L.ore_model_graph_capture_classify_u8_list(None, None, q, None))
    assert L.ore_image_list_count(None) == 0
    assert L.ore_image_list_destroy(None) == 0  # as ore_ctx_destroy / ore_model_destroy of a null handle


def _host_list(capacity=4, c=3, out_hw=(4, 4)):
    """An ImageList without a library object behind it: set() must raise before it would need one."""
    lst = object.__new__(ore.ImageList)
    lst.ctx = type("C", (), {"device": 0, "h": None})()
    lst.capacity, lst.channels, lst.out_hw = capacity, c, out_hw
    lst.h = None
    lst._images = ()
    return lst


def test_python_checks_host():
    import torch
    lst = _host_list()
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        lst.set([torch.zeros((9, 12, 3), dtype=torch.uint8)])  # a CPU tensor
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        lst.set([torch.zeros((9, 12, 3), dtype=torch.float32)])
    with pytest.raises(ore.OreError, match="not both"):
        lst.set([], geometries=[], short=8)
    with pytest.raises(ore.OreError, match="capacity"):
        lst.set([None] * 5)
    with pytest.raises(ore.OreError, match="geometries"):
        lst.set([None], geometries=[])
    with pytest.raises(ore.OreError, match="ImageList"):
        ore.preprocess_list_u8(lst.ctx, lst)  # not open
    with pytest.raises(ore.OreError, match="ImageList"):
        ore.preprocess_list_u8(lst.ctx, None)
    m = object.__new__(ore.Model)
    m.ctx, m.input_dims, m.max_batch, m.output_elems, m.topk = lst.ctx, (3, 4, 4), 2, 10, 1
    for fn in (m.run_u8_list, m.classify_u8_list):
        for bad in (None, lst, torch.zeros((1, 4, 4, 3), dtype=torch.uint8)):  # not a list, a closed one, a batch
            with pytest.raises(ore.OreError, match="ImageList"):
                fn(bad)
    for fn in (m.run_u8_list_into, m.capture_u8_list):
        with pytest.raises(ore.OreError, match="ImageList"):
            fn(lst, torch.zeros((1, 10)))

    # shape and strides, through set() itself: CPU views standing in for CUDA ones (_as_cuda)
    x = torch.zeros((9, 12, 3), dtype=torch.uint8)
    for bad, word in [(x[:, :, 0], r"\[Hs, Ws, C\]"),            # [Hs, Ws] without channels
                      (x[:, ::2], "strides"),                    # stride(1) != C
                      (x.permute(1, 0, 2), "strides"),           # rows and columns swapped
                      (x[:, :, :2], "channels"),                 # two of three channels
                      (x[:0], "empty")]:
        with pytest.raises(ore.OreError, match=word):
            lst.set([_as_cuda(x), _as_cuda(bad)])
    with pytest.raises(ore.OreError, match="cuda:1"):
        lst.set([_as_cuda(x, index=1)])
    # what set() would hand to the library: pointer, size, row stride and the three kinds of geometry
    win = x[3:8, 5:11]
    _, arr = lst._descriptors([_as_cuda(x), _as_cuda(win)], None, None)
    assert (arr[0].data, arr[0].hs, arr[0].ws, arr[0].row_stride) == (x.data_ptr(), 9, 12, 36)
    assert (arr[1].data, arr[1].hs, arr[1].ws, arr[1].row_stride) == (x.data_ptr() + 3 * 36 + 5 * 3, 5, 6, 36)
    assert [(d.g.rh, d.g.rw, d.g.top, d.g.left) for d in arr] == [(4, 4, 0, 0)] * 2
    _, arr = lst._descriptors([_as_cuda(x)], [((6, 7), (1, 2))], None)
    assert (arr[0].g.rh, arr[0].g.rw, arr[0].g.top, arr[0].g.left) == (6, 7, 1, 2)
    _, arr = lst._descriptors([_as_cuda(x), _as_cuda(win)], None, 5)
    want = [ore.center_crop_geometry(hw, 5, (4, 4)) for hw in ((9, 12), (5, 6))]
    assert [((d.g.rh, d.g.rw), (d.g.top, d.g.left)) for d in arr] == want
    assert ore.load().ore_image_check(arr, 2, 3, 4, 4, None) == 0


def _as_cuda(x, index=0):
    """A CPU tensor that reports itself as a CUDA tensor on cuda:<index>, for the host checks that come before
    any library call: they read its dtype, shape and strides, never its bytes."""
    import torch

    class AsCuda(torch.Tensor):
        is_cuda = True
        device = type("D", (), {"index": index})()

    return x.as_subclass(AsCuda)
