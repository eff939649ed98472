"""CPU: the antialiased-resize entry points (ore_resize_aa_taps, ore_preprocess_resize_u8_ex, ore_image_check_ex,
ore_image_list_create_ex / _filter, ore_model_set_input_resize_ex, ore_ctx_set_resize_variant) are exported, the
binding mirrors the header's constants, and every argument check answers ORE_ERR_INVALID with a message before
any device call.  No kernel is launched here."""
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
AA = 1


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
    assert msg
    if word:
        assert word in msg, msg


def test_exports_and_constants():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", src))
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.load().ore_abi_version()  # added without an ABI bump
    assert int(defs["ORE_AA_MAX_RATIO"]) == ore.AA_MAX_RATIO == 32
    assert int(defs["ORE_AA_MAX_TAPS"]) == ore.AA_MAX_TAPS == 64
    enum = re.search(r"typedef enum \{([^}]*)\} ore_resize_filter;", src).group(1)
    assert dict(re.findall(r"(ORE_FILTER_\w+) = (\d+)", enum)) == {"ORE_FILTER_BILINEAR": "0", "ORE_FILTER_BILINEAR_AA": "1"}
    assert (ore.FILTER_BILINEAR, ore.FILTER_BILINEAR_AA) == (0, 1)
    for name in ("ore_resize_aa_taps", "ore_preprocess_resize_u8_ex", "ore_image_check_ex", "ore_image_list_create_ex",
                 "ore_image_list_filter", "ore_model_set_input_resize_ex", "ore_ctx_set_resize_variant"):
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)


def _call(g, filt=AA, hs=64, ws=64, c=3, n=1, ydims=(1, 3, 2, 2), flags=0, nstride=0):
    """ore_preprocess_resize_u8_ex without a context: a good call ends at "null context"."""
    y = _tensor(ydims, nstride=nstride)
    return ore.load().ore_preprocess_resize_u8_ex(None, P, n, hs, ws, c, ctypes.byref(_lib.Resize(*g)), filt, None, None, flags,
                                                  ctypes.byref(y))


def test_preprocess_ex_check_order():
    _fails(_call((2, 2, 0, 0)), b"null context")  # ratio exactly 32 on both axes
    _fails(_call((2, 2, 0, 0), filt=0, hs=16384, ws=16384), b"null context")  # the plain filter has no ratio rule
    _fails(_call((80, 90, 3, 4)), b"null context")  # nothing shrinks
    _fails(_call((2, 2, 0, 0), flags=ore.PRE_REVERSE_CHANNELS), b"null context")
    # an unknown filter
    for filt in (2, -1, 7):
        _fails(_call((2, 2, 0, 0), filt=filt), b"filter")
    # a ratio above 32, the axis named
    _fails(_call((2, 2, 0, 0), hs=65), b"rows")
    _fails(_call((2, 2, 0, 0), ws=65), b"columns")
    _fails(_call((2, 64, 0, 0), hs=66, ydims=(1, 3, 2, 64)), b"rows")
    _fails(_call((512, 2, 0, 0), hs=16384, ws=16384, ydims=(1, 3, 2, 2)), b"columns")
    _fails(_call((511, 600, 0, 0), hs=16384, ws=16384), b"rows go 16384 -> 511")
    # the checks of the plain entry come first, unchanged
    _fails(_call((2, 2, 1, 0)), b"outside")
    _fails(_call((2, 2, 0, 0), hs=16385), b"1..16384")
    _fails(_call((2, 2, 0, 0), flags=2), b"flags")
    _fails(_call((2, 2, 0, 0), flags=4), b"flags")
    _fails(_call((2, 2, 0, 0), c=5, ydims=(1, 5, 2, 2)), b"channels")
    _fails(_call((2, 2, 0, 0), ydims=(2, 3, 2, 2)), b"[n,c,H,W]")
    _fails(_call((2, 2, 0, 0), nstride=11), b"stride")
    _fails(_call((2, 2, 0, 0), n=-1, ydims=(-1, 3, 2, 2)), b"negative")
    # a bad ratio is reported before the missing context and before the output stride
    _fails(_call((2, 2, 0, 0), hs=65, nstride=11), b"rows")
    # null pointers
    L = ore.load()
    y, g = _tensor((1, 3, 2, 2)), _lib.Resize(2, 2, 0, 0)
    _fails(L.ore_preprocess_resize_u8_ex(None, None, 1, 64, 64, 3, ctypes.byref(g), AA, None, None, 0, ctypes.byref(y)), b"null argument")
    _fails(L.ore_preprocess_resize_u8_ex(None, P, 1, 64, 64, 3, None, AA, None, None, 0, ctypes.byref(y)), b"null argument")
    _fails(L.ore_preprocess_resize_u8_ex(None, P, 1, 64, 64, 3, ctypes.byref(g), AA, None, None, 0, None), b"null argument")
    _fails(L.ore_preprocess_resize_u8_ex(None, P, 1, 64, 64, 3, ctypes.byref(g), AA, None, None, 0,
                                         ctypes.byref(_tensor((1, 3, 2, 2), data=0))), b"null argument")


def _descs(items):
    arr = (_lib.ImageU8 * len(items))()
    for i, (hs, ws, g) in enumerate(items):
        arr[i].data, arr[i].hs, arr[i].ws, arr[i].row_stride = 0x1000, hs, ws, 0
        arr[i].g = _lib.Resize(*g)
    return arr


def test_image_check_ex():
    L = ore.load()
    items = [(64, 64, (2, 2, 0, 0)), (9, 9, (20, 20, 3, 3)), (40, 66, (2, 2, 0, 0)), (67, 40, (2, 2, 0, 0))]
    arr = _descs(items)
    bad = ctypes.c_int64(-1)
    _fails(L.ore_image_check_ex(arr, 4, 3, 2, 2, AA, ctypes.byref(bad)), b"image 2")
    assert bad.value == 2 and b"columns" in L.ore_last_error(None)
    assert L.ore_image_check_ex(arr, 2, 3, 2, 2, AA, ctypes.byref(bad)) == 0
    _fails(L.ore_image_check_ex(_descs(items[3:]), 1, 3, 2, 2, AA, None), b"rows")
    # the plain filter, and ore_image_check itself, still accept them -- and 16384 -> 1
    far = _descs(items + [(16384, 16384, (2, 2, 0, 0))])
    assert L.ore_image_check_ex(far, 5, 3, 2, 2, 0, ctypes.byref(bad)) == 0
    assert L.ore_image_check(far, 5, 3, 2, 2, ctypes.byref(bad)) == 0
    one = _descs([(16384, 16384, (1, 1, 0, 0))])
    assert L.ore_image_check(one, 1, 3, 1, 1, None) == 0
    _fails(L.ore_image_check_ex(one, 1, 3, 1, 1, AA, ctypes.byref(bad)), b"image 0")
    # the earlier checks, unchanged, and the arguments
    _fails(L.ore_image_check_ex(_descs([(64, 64, (2, 2, 1, 0))]), 1, 3, 2, 2, AA, ctypes.byref(bad)), b"outside")
    _fails(L.ore_image_check_ex(arr, 1, 3, 2, 2, 2, None), b"filter")
    _fails(L.ore_image_check_ex(None, 1, 3, 2, 2, AA, None), b"null")
    _fails(L.ore_image_check_ex(arr, -1, 3, 2, 2, AA, None), b"negative")
    assert L.ore_image_check_ex(None, 0, 3, 2, 2, AA, None) == 0


def test_null_arguments():
    L = ore.load()
    g = _lib.Resize(2, 2, 0, 0)
    _fails(L.ore_model_set_input_resize_ex(None, 64, 64, ctypes.byref(g), AA), b"null")
    _fails(L.ore_ctx_set_resize_variant(None, 1), b"null")
    out = ctypes.c_void_p()
    _fails(L.ore_image_list_create_ex(None, 4, 3, 2, 2, AA, ctypes.byref(out)), b"null")
    assert L.ore_image_list_filter(None) == 0
    a, w = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 256)()
    _fails(L.ore_resize_aa_taps(8, 4, 0, 4, None, a, a, w), b"null")
    _fails(L.ore_resize_aa_taps(8, 4, 0, 4, a, None, a, w), b"null")
    _fails(L.ore_resize_aa_taps(8, 4, 0, 4, a, a, None, w), b"null")
    f, n, s = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    assert L.ore_resize_aa_taps(8, 4, 0, 4, f, n, s, None) == 0  # the weights are optional
    assert list(f) == [0, 1, 3, 5] and list(n) == [3, 4, 4, 3]


def test_aa_taps_on_an_axis_that_does_not_shrink():
    L = ore.load()
    a = (ctypes.c_int32 * 8)()
    for src, resized in [(8, 8), (4, 8)]:
        _fails(L.ore_resize_aa_taps(src, resized, 0, 4, a, a, a, None), b"does not shrink")
        assert b"ore_resize_taps" in L.ore_last_error(None)
    _fails(L.ore_resize_aa_taps(66, 2, 0, 2, a, a, a, None), b"32")


def test_python_checks_host():
    """The keyword reaches the host checks: a ratio over 32 is refused with the axis named before any library
    call (a context that is no context would fail there)."""
    import torch
    ctx = type("C", (), {"device": 0, "h": None})()
    m = object.__new__(ore.Model)
    m.ctx, m.input_dims, m.h = ctx, (3, 2, 2), None
    with pytest.raises(ore.OreError, match="rows go 65 -> 2"):
        m.set_input_resize((65, 64), antialias=True)
    with pytest.raises(ore.OreError, match="columns go 67 -> 2"):
        m.set_input_resize((64, 67), (2, 2), antialias=True)
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        ore.preprocess_resize_u8(ctx, torch.zeros((1, 65, 64, 3), dtype=torch.uint8), (2, 2), antialias=True)
