"""CPU: the cubic filters through the C ABI without a device.  Filter words 256 / 257 pass every check a host can
make (a good call ends at the missing context, list or model), every other word but 0 and 1 is rejected; the
16-times rule of 257 sits where the 32-times rule of 1 does; ore_resize_cubic_taps checks its arguments in the
documented order.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import ore
from ore import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID
P = ctypes.c_void_p(0x1000)  # never dereferenced: the checks come first
CUBIC, CUBIC_AA = 256, 257
UNKNOWN = (2, -1, 7, 258, 512)


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
    assert int(defs["ORE_FILTER_CUBIC_BIT"]) == _lib.FILTER_CUBIC_BIT == 256
    assert int(defs["ORE_FILTER_BICUBIC"]) == ore.FILTER_BICUBIC == 256
    assert int(defs["ORE_FILTER_BICUBIC_AA"]) == ore.FILTER_BICUBIC_AA == 257
    assert int(defs["ORE_CUBIC_AA_MAX_RATIO"]) == ore.CUBIC_AA_MAX_RATIO == 16
    assert ore.CUBIC_AA_MAX_RATIO * 4 == ore.AA_MAX_TAPS  # a run at the limit is 64 taps
    assert "ore_resize_cubic_taps" in _lib.EXPORTED and hasattr(ore.load(), "ore_resize_cubic_taps")
    from ore import engine
    assert [engine._filter(a, c) for a in (False, True) for c in (False, True)] == [0, 256, 1, 257]


def _call(g, filt, hs=64, ws=64, c=3, n=1, ydims=(1, 3, 2, 2), flags=0, nstride=0):
    """ore_preprocess_resize_u8_ex without a context: a good call ends at "null context"."""
    y = _tensor(ydims, nstride=nstride)
    return ore.load().ore_preprocess_resize_u8_ex(None, P, n, hs, ws, c, ctypes.byref(_lib.Resize(*g)), filt, None, None, flags,
                                                  ctypes.byref(y))


def test_preprocess_ex():
    for filt in (CUBIC, CUBIC_AA):
        _fails(_call((4, 4, 1, 2), filt), b"null context")  # ratio exactly 16 on both axes
        _fails(_call((80, 90, 3, 4), filt), b"null context")  # nothing shrinks
        _fails(_call((4, 4, 0, 0), filt, flags=ore.PRE_REVERSE_CHANNELS), b"null context")
        # the checks of the plain entry come first, unchanged
        _fails(_call((4, 4, 3, 0), filt), b"outside")
        _fails(_call((4, 4, 0, 0), filt, hs=16385), b"1..16384")
        _fails(_call((4, 4, 0, 0), filt, nstride=11), b"stride")
    for filt in UNKNOWN:
        _fails(_call((4, 4, 0, 0), filt), b"filter")
    # ratio 17: the axis named, before the missing context and the output stride
    _fails(_call((4, 4, 0, 0), CUBIC_AA, hs=65), b"at most 16 times, the rows go 65 -> 4")
    _fails(_call((4, 4, 0, 0), CUBIC_AA, ws=68), b"at most 16 times, the columns go 68 -> 4")
    _fails(_call((4, 4, 0, 0), CUBIC_AA, hs=65, nstride=11), b"rows")
    _fails(_call((1023, 2000, 0, 0), CUBIC_AA, hs=16384, ws=16384), b"rows go 16384 -> 1023")
    _fails(_call((1024, 1024, 0, 0), CUBIC_AA, hs=16384, ws=16384), b"null context")
    # the plain cubic filter has no ratio rule
    _fails(_call((1, 1, 0, 0), CUBIC, hs=16384, ws=16384, ydims=(1, 3, 1, 1)), b"null context")
    _fails(_call((1, 1, 0, 0), CUBIC_AA, hs=16384, ws=16384, ydims=(1, 3, 1, 1)), b"at most 16")
    # the 32-times rule of filter 1 is where it was
    _fails(_call((2, 2, 0, 0), 1, hs=64), b"null context")
    _fails(_call((2, 2, 0, 0), 1, hs=65), b"at most 32 times, the rows go 65 -> 2")


def _u8(items):
    arr = (_lib.ImageU8 * len(items))()
    for i, (hs, ws, g) in enumerate(items):
        arr[i].data, arr[i].hs, arr[i].ws, arr[i].row_stride = 0x1000, hs, ws, 0
        arr[i].g = _lib.Resize(*g)
    return arr


def _nv12(items):
    arr = (_lib.ImageNv12 * len(items))()
    for i, (hs, ws, g) in enumerate(items):
        arr[i].y, arr[i].uv, arr[i].hs, arr[i].ws = 0x1000, 0x2000, hs, ws
        arr[i].g = _lib.Resize(*g)
    return arr


def _yuv(items):
    arr = (_lib.ImageYuv * len(items))()
    for i, (hs, ws, g) in enumerate(items):
        arr[i].plane[0], arr[i].plane[1], arr[i].plane[2] = 0x1000, 0x2000, 0x3000
        arr[i].hs, arr[i].ws, arr[i].format = hs, ws, _lib.YUV_FORMATS["i420"]
        arr[i].g = _lib.Resize(*g)
    return arr


def _checks():
    L = ore.load()
    return [("ex", _u8, lambda a, n, filt, bad: L.ore_image_check_ex(a, n, 3, 2, 2, filt, bad)),
            ("nv12", _nv12, lambda a, n, filt, bad: L.ore_image_check_nv12(a, n, 2, 2, filt, bad)),
            ("yuv", _yuv, lambda a, n, filt, bad: L.ore_image_check_yuv(a, n, 2, 2, filt, bad))]


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["ex", "nv12", "yuv"])
def test_image_checks(kind):
    _, make, check = _checks()[kind]
    items = [(32, 32, (2, 2, 0, 0)), (9, 9, (20, 20, 3, 3)), (20, 34, (2, 2, 0, 0)), (35, 20, (2, 2, 0, 0))]
    arr = make(items)
    bad = ctypes.c_int64(-1)
    for filt in (CUBIC, CUBIC_AA):
        assert check(arr, 2, filt, ctypes.byref(bad)) == 0  # ratio 16 passes
    _fails(check(arr, 4, CUBIC_AA, ctypes.byref(bad)), b"image 2")
    assert bad.value == 2 and b"at most 16 times, the columns go 34 -> 2" in ore.load().ore_last_error(None)
    _fails(check(make(items[3:]), 1, CUBIC_AA, None), b"at most 16 times, the rows go 35 -> 2")
    assert check(arr, 4, CUBIC, ctypes.byref(bad)) == 0  # no ratio rule under 256
    far = make([(16384, 16384, (1, 1, 0, 0))])
    L = ore.load()
    one = [lambda f: L.ore_image_check_ex(far, 1, 3, 1, 1, f, None), lambda f: L.ore_image_check_nv12(far, 1, 1, 1, f, None),
           lambda f: L.ore_image_check_yuv(far, 1, 1, 1, f, None)][kind]
    assert one(CUBIC) == 0  # 16384 -> 1
    _fails(one(CUBIC_AA), b"at most 16")
    for filt in UNKNOWN:
        _fails(check(arr, 1, filt, None), b"filter")
    # the earlier checks, unchanged
    _fails(check(make([(32, 32, (2, 2, 1, 0))]), 1, CUBIC_AA, ctypes.byref(bad)), b"outside")
    assert check(None, 0, CUBIC_AA, None) == 0


def test_entries_that_need_a_handle():
    """The list constructors and the model entry look at their handle first: without one they answer "null"
    whatever the filter, as they do for the filters of the enum."""
    L = ore.load()
    g = _lib.Resize(2, 2, 0, 0)
    out = ctypes.c_void_p()
    for filt in (CUBIC, CUBIC_AA) + UNKNOWN:
        _fails(L.ore_model_set_input_resize_ex(None, 64, 64, ctypes.byref(g), filt), b"null")
        _fails(L.ore_image_list_create_ex(None, 4, 3, 2, 2, filt, ctypes.byref(out)), b"null")
        _fails(L.ore_image_list_create_nv12(None, 4, 2, 2, filt, 0, ctypes.byref(out)), b"null")
        _fails(L.ore_image_list_create_yuv(None, 4, 2, 2, filt, 0, ctypes.byref(out)), b"null")
    assert L.ore_image_list_filter(None) == 0


def _taps(src, resized, origin, count, filt, first=True, ntaps=True, weights=True, total=True):
    n = max(count, 1)
    f, k, s = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)(), (ctypes.c_float * n)()
    w = (ctypes.c_float * (64 * n))()
    st = ore.load().ore_resize_cubic_taps(src, resized, origin, count, filt, f if first else None, k if ntaps else None,
                                          w if weights else None, s if total else None)
    return st, list(f), list(k), list(s)


def test_cubic_taps_arguments():
    for missing in ("first", "ntaps", "total"):
        _fails(_taps(8, 4, 0, 4, CUBIC, **{missing: False})[0], b"null")
    st, f, k, s = _taps(8, 4, 0, 4, CUBIC, weights=False)  # the weights are optional
    assert st == 0 and f == [-1, 1, 3, 5] and k == [4] * 4 and s == [1.0] * 4
    st, f, k, s = _taps(8, 4, 0, 4, CUBIC_AA, weights=False)
    assert st == 0 and f == [0, 0, 1, 3] and k == [5, 7, 7, 5]
    # null pointers, then the filter, then the axis, then the ratio
    _fails(_taps(0, 4, 0, 4, 1, first=False)[0], b"null")
    for filt in (0, 1) + UNKNOWN:
        _fails(_taps(8, 4, 0, 4, filt)[0], b"filter")
    _fails(_taps(0, 4, 0, 4, 7)[0], b"filter")
    for bad in [(0, 4, 0, 4), (8, 0, 0, 1), (16385, 4, 0, 4), (8, 4, 1, 4), (8, 4, -1, 2), (8, 4, 0, 0), (8, 16385, 0, 4)]:
        for filt in (CUBIC, CUBIC_AA):
            _fails(_taps(*bad, filt)[0], b"resize taps")
    _fails(_taps(68, 4, 2, 4, CUBIC_AA)[0], b"resize taps: 68 samples")  # the axis before the ratio
    _fails(_taps(65, 4, 0, 4, CUBIC_AA)[0], b"at most 16")
    assert _taps(64, 4, 0, 4, CUBIC_AA)[0] == 0
    assert _taps(16384, 1, 0, 1, CUBIC)[0] == 0
    _fails(_taps(16384, 1, 0, 1, CUBIC_AA)[0], b"at most 16")
    # the Python wrapper returns the same table
    first, ntaps, weights, total = ore.resize_cubic_taps(8, 4, 0, 4, antialias=True)
    assert list(first) == [0, 0, 1, 3] and list(ntaps) == [5, 7, 7, 5] and weights.shape == (4, 64)
    assert weights.dtype == np.float32 and total.dtype == np.float32
    with pytest.raises(ore.OreError, match="at most 16"):
        ore.resize_cubic_taps(65, 4, 0, 4, antialias=True)


def test_python_checks_host():
    """The keyword reaches the host checks: a ratio over 16 is refused with the axis named before any library call
    (a context that is no context would fail there); under cubic alone there is no ratio rule."""
    import torch
    ctx = type("C", (), {"device": 0, "h": None})()
    m = object.__new__(ore.Model)
    m.ctx, m.input_dims, m.h = ctx, (3, 2, 2), None
    with pytest.raises(ore.OreError, match="at most 16 times, the rows go 33 -> 2"):
        m.set_input_resize((33, 32), antialias=True, cubic=True)
    with pytest.raises(ore.OreError, match="columns go 35 -> 2"):
        m.set_input_resize((32, 35), (2, 2), antialias=True, cubic=True)
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        ore.preprocess_resize_u8(ctx, torch.zeros((1, 33, 32, 3), dtype=torch.uint8), (2, 2), cubic=True)
