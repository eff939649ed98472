"""CPU: the class activation map entries (ore_class_maps_f32, ore_model_cam_dims, ore_model_set_cam) exist, the
binding lists them, and every argument check of ore_class_maps_f32 answers ORE_ERR_INVALID with its message from
the arguments alone: no context, pointers that are never dereferenced, no device call.  No kernel is launched here."""
import ctypes
import os
import re

import ore
from ore import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID
NAMES = ("ore_class_maps_f32", "ore_model_cam_dims", "ore_model_set_cam")
P = ctypes.c_void_p(0x1000)  # never dereferenced


def _tensor(dims, data=0x1000):
    t = _lib.Tensor()
    t.data = data
    t.ndim = len(dims)
    for i, d in enumerate(dims):
        t.dims[i] = d
    return t


def _fails(status):
    assert status == INVALID
    msg = ore.load().ore_last_error(None)
    assert msg  # a message, also without a context
    return msg


def _maps(x, w=P, bias=P, M=40, relu=1, classes=P, k=5, views=1, maps=P, ctx=None):
    return ore.load().ore_class_maps_f32(ctx, None if x is None else ctypes.byref(x), w, bias, M, relu, classes, k, views, maps)


def test_names_and_abi_version():
    text = open(HEADER).read()
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", text))
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.ABI_VERSION  # additions only, no ABI bump
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)
    assert callable(ore.class_maps)
    for attr in ("cam_hw", "set_cam_output", "classify_cam", "classify_cam_u8", "classify_cam_u8_list"):
        assert hasattr(ore.Model, attr), attr


def test_null_arguments_are_invalid():
    x = _tensor((3, 32, 13, 11))
    assert b"null" in _fails(_maps(None))
    assert b"null" in _fails(_maps(_tensor((3, 32, 13, 11), data=0)))
    for name in ("w", "classes", "maps"):
        assert b"null" in _fails(_maps(x, **{name: None})), name
    # a null bias is allowed, and with everything in range only the context is missed
    assert b"null" in _fails(_maps(x, bias=None))
    assert b"null" in _fails(_maps(x))


def test_ranges_are_checked_before_any_device_call():
    """Each answer names its argument, so it was judged before the context or the device was needed."""
    x = _tensor((6, 32, 13, 11))
    for dims in ((6, 32), (6, 32, 13), (6,)):
        assert b"dims" in _fails(_maps(_tensor(dims)))
    for bad in ((6, 0, 13, 11), (6, 32, 0, 11), (6, 32, 13, 0), (-1, 32, 13, 11)):
        assert b"class maps: x" in _fails(_maps(_tensor(bad)))
    assert b"M = 0" in _fails(_maps(x, M=0))
    for M, k in ((40, 0), (40, -1), (40, 41), (1000, 65), (3, 4)):
        msg = _fails(_maps(x, M=M, k=k))
        assert b"k = " in msg and b"min(M, 64)" in msg
    for views in (0, -1, 65):
        assert b"views" in _fails(_maps(x, views=views))
    for n, views in ((5, 2), (7, 3), (1, 2)):
        msg = _fails(_maps(_tensor((n, 32, 13, 11)), views=views))
        assert b"views" in msg and b"multiple" in msg
    # the nstride rule of include/ore.h: 0 or at least one image, and 32-bit indexing
    img = 32 * 13 * 11
    for ns in (img - 1, 1, -img):
        t = _tensor((6, 32, 13, 11))
        t.nstride = ns
        assert b"nstride" in _fails(_maps(t))
    t = _tensor((6, 32, 13, 11))
    t.nstride = 1 << 29
    assert b"32-bit" in _fails(_maps(t))
    t.nstride = img + 3  # a slice: in range, the context is missed
    assert b"null" in _fails(_maps(t, k=40, views=6))
    assert b"null" in _fails(_maps(_tensor((0, 32, 13, 11))))  # n == 0 still needs a context


def test_model_entries_with_a_null_model():
    L = ore.load()
    hw = (ctypes.c_int64 * 2)()
    assert b"null" in _fails(L.ore_model_cam_dims(None, hw))
    assert b"null" in _fails(L.ore_model_cam_dims(None, None))
    assert b"null" in _fails(L.ore_model_set_cam(None, P, 100))
    assert b"null" in _fails(L.ore_model_set_cam(None, None, 0))
