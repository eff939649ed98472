"""CPU: the oriented image-list entries (include/ore.h: ore_image_check_oriented and its NV12 / YUV forms,
ore_image_list_set_oriented ..., ore_orient_geometry, ore_image_list_oriented) are declared, exported and bound; the
host-only checks judge the crop in displayed space and the ratio rules in stored space; and the Python layer rejects
bad arguments before any library call.  No kernel is launched here."""
import ctypes
import inspect
import re
import os

import pytest

import ore
from ore import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID
NAMES = ("ore_orient_geometry", "ore_image_check_oriented", "ore_image_check_nv12_oriented", "ore_image_check_yuv_oriented",
         "ore_image_list_set_oriented", "ore_image_list_set_nv12_oriented", "ore_image_list_set_yuv_oriented",
         "ore_image_list_oriented")
FAKE = 0x1000  # a non-null pointer that is never dereferenced


def _codes(*c):
    return (ctypes.c_uint8 * len(c))(*c)


def _u8(hs, ws, g, n=1):
    arr = (_lib.ImageU8 * n)()
    for d in arr:
        d.data, d.hs, d.ws, d.row_stride = FAKE, hs, ws, 0
        d.g = _lib.Resize(*g)
    return arr


def _nv12(hs, ws, g, n=1):
    arr = (_lib.ImageNv12 * n)()
    for d in arr:
        d.y, d.uv, d.hs, d.ws = FAKE, FAKE, hs, ws
        d.g = _lib.Resize(*g)
    return arr


def _yuv(hs, ws, g, n=1):
    arr = (_lib.ImageYuv * n)()
    for d in arr:
        d.plane[0], d.plane[1], d.plane[2] = FAKE, FAKE, FAKE
        d.hs, d.ws, d.format = hs, ws, _lib.YUV_FORMATS["i420"]
        d.g = _lib.Resize(*g)
    return arr


def _checks(h, w, filt):
    """The three check entries over one (hs, ws, g) under one signature: (make, check(arr, n, codes, bad))."""
    L = ore.load()
    return [
        (_u8, lambda a, n, c, b: L.ore_image_check_oriented(a, n, 3, h, w, filt, c, b)),
        (_nv12, lambda a, n, c, b: L.ore_image_check_nv12_oriented(a, n, h, w, filt, c, b)),
        (_yuv, lambda a, n, c, b: L.ore_image_check_yuv_oriented(a, n, h, w, filt, c, b)),
    ]


def _err():
    return ore.load().ore_last_error(None)


def test_names_and_abi_version():
    text = open(HEADER).read()
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", text))
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.ABI_VERSION  # additions only, no ABI bump
    assert re.search(r"#define ORE_IMAGE_FLIP_H 1u", text) and ore.IMAGE_FLIP_H == 1  # still the only flag bit
    assert int(defs["ORE_AA_MAX_RATIO"]) == ore.AA_MAX_RATIO and int(defs["ORE_CUBIC_AA_MAX_RATIO"]) == ore.CUBIC_AA_MAX_RATIO
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)
    for fn in (ore.oriented_hw, ore.apply_orientation, ore.rotation_orientation, ore.orient_geometry):
        assert callable(fn)
    # the descriptors did not grow: the codes travel in an array of their own
    assert ctypes.sizeof(_lib.ImageU8) == 64 and ctypes.sizeof(_lib.ImageNv12) == 80 and ctypes.sizeof(_lib.ImageYuv) == 104
    assert "mark" in text and "re-capture" in text  # the capture rule is in the header


def test_bad_codes_name_the_descriptor_before_its_geometry():
    for make, check in _checks(5, 7, _lib.FILTER_BILINEAR):
        arr = make(20, 30, (5, 7, 0, 0), n=3)
        arr[1].g = _lib.Resize(0, 0, -1, -1)  # descriptor 1's geometry is bad too: the code is judged first
        for code in (0, 9, 255):
            bad = ctypes.c_int64(-1)
            assert check(arr, 3, _codes(1, code, 8), ctypes.byref(bad)) == INVALID
            assert b"image 1" in _err() and b"orientation" in _err() and bad.value == 1
        bad = ctypes.c_int64(-1)
        assert check(arr, 3, _codes(1, 6, 0), ctypes.byref(bad)) == INVALID  # a good code: now its geometry
        assert b"image 1" in _err() and b"orientation" not in _err() and bad.value == 1
        for code in range(1, 9):
            assert check(arr, 1, _codes(code, 0, 0), None) == 0, _err()  # only n codes are read
        assert check(arr, 0, _codes(0), None) == 0  # n == 0
        assert check(None, 0, None, None) == 0
        assert check(arr, 1, None, None) == 0  # NULL: all 1


def test_crop_is_checked_in_displayed_space():
    h, w = 5, 7
    for make, check in _checks(h, w, _lib.FILTER_BILINEAR):
        # displayed 6 x 40 at (1, 30): fits displayed space (1 + 5 <= 6, 30 + 7 <= 40); read as a stored-space window
        # it would not (30 + 7 > 6).  Stored image 30 x 20, displayed 20 x 30 under the transposing codes.
        fits = make(30, 20, (6, 40, 1, 30))
        for code in (5, 6, 7, 8):
            assert check(fits, 1, _codes(code), None) == 0, _err()
        # the converse: displayed 40 x 6 at (0, 30) would fit if its numbers were held against the stored-space sizes
        # (0 + 5 <= 6, 30 + 7 <= 40), and does not fit the displayed image (30 + 7 > 6)
        for code in (5, 6, 7, 8):
            bad = ctypes.c_int64(-1)
            assert check(make(30, 20, (40, 6, 0, 30)), 1, _codes(code), ctypes.byref(bad)) == INVALID
            assert b"image 0" in _err() and b"crop" in _err() and bad.value == 0
        for code in (1, 2, 3, 4):
            assert check(make(30, 20, (40, 6, 0, 30)), 1, _codes(code), None) == INVALID
            assert check(make(30, 20, (40, 8, 30, 1)), 1, _codes(code), None) == 0
        # one past each border, every code
        for code in range(1, 9):
            assert check(make(30, 20, (9, 12, 4, 5)), 1, _codes(code), None) == 0  # the far corner
            assert check(make(30, 20, (9, 12, 5, 5)), 1, _codes(code), None) == INVALID
            assert check(make(30, 20, (9, 12, 4, 6)), 1, _codes(code), None) == INVALID
            assert check(make(30, 20, (9, 12, -1, 0)), 1, _codes(code), None) == INVALID
            assert check(make(30, 20, (9, 12, 0, -1)), 1, _codes(code), None) == INVALID


def test_ratio_rule_is_judged_on_the_stored_axes():
    # a 40 x 2000 stored image under code 6 is displayed 2000 x 40.  Displayed geometry 50 x 5: stored-space resized
    # size 5 x 50, so the stored rows go 40 -> 5 (8 times) and the stored columns 2000 -> 50 (40 times > 32).
    h, w = 5, 5
    for make, check in _checks(h, w, _lib.FILTER_BILINEAR_AA):
        bad = ctypes.c_int64(-1)
        assert check(make(40, 2000, (50, 5, 0, 0)), 1, _codes(6), ctypes.byref(bad)) == INVALID
        assert b"image 0" in _err() and b"columns go 2000 -> 50" in _err() and bad.value == 0
        # displayed 5 x 63: stored 63 x 5, 40 -> 63 grows, 2000 -> 5 ... 400 times
        assert check(make(40, 2000, (5, 63, 0, 0)), 1, _codes(6), None) == INVALID and b"columns go 2000 -> 5" in _err()
        # displayed 63 x 5: stored columns 2000 -> 63 is within 32 times, stored rows 40 -> 5 within 32 times.  Judged on
        # displayed axes against the displayed sizes as if they were stored ones (40 -> 63, 2000 -> 5) it would fail.
        assert check(make(40, 2000, (63, 5, 0, 0)), 1, _codes(6), None) == 0, _err()
        assert check(make(40, 2000, (63, 5, 0, 0)), 1, _codes(1), None) == INVALID and b"columns go 2000 -> 5" in _err()
        assert check(make(40, 2000, (63, 5, 0, 0)), 1, None, None) == INVALID
    for make, check in _checks(h, w, _lib.FILTER_BICUBIC_AA):  # 16 times: 2000 -> 63 is 31.7
        assert check(make(40, 2000, (63, 5, 0, 0)), 1, _codes(6), None) == INVALID and b"columns go 2000 -> 63" in _err()
        assert check(make(40, 2000, (125, 5, 0, 0)), 1, _codes(8), None) == 0, _err()
    for make, check in _checks(h, w, _lib.FILTER_BILINEAR):  # no rule without antialiasing
        assert check(make(40, 2000, (50, 5, 0, 0)), 1, _codes(6), None) == 0


def test_null_lists_and_unknown_filters():
    L = ore.load()
    for fn in (L.ore_image_list_set_oriented, L.ore_image_list_set_nv12_oriented, L.ore_image_list_set_yuv_oriented):
        assert fn(None, None, None, None, 0) == INVALID and b"null" in _err()
        assert fn(None, None, None, _codes(6), 1) == INVALID and b"null" in _err()
    assert L.ore_image_list_oriented(None) == 0
    for make, check in _checks(5, 7, 2):
        assert check(make(20, 30, (5, 7, 0, 0)), 1, _codes(1), None) == INVALID and b"filter" in _err()


def _host_list(cls=None, capacity=4, out_hw=(4, 4)):
    lst = object.__new__(cls or ore.ImageList)
    lst.ctx = type("C", (), {"device": 0, "h": None})()
    lst.capacity, lst.channels, lst.out_hw = capacity, 3, out_hw
    lst.h = None
    lst._images = ()
    return lst


def test_set_oriented_argument_errors_come_before_the_library():
    import torch
    for cls in (ore.ImageList, ore.Nv12ImageList, ore.YuvImageList):
        names = list(inspect.signature(cls.set_oriented).parameters)
        assert names[1:] == [names[1], "orientations", "geometries", "short", "flips"]
        assert all(inspect.signature(cls.set_oriented).parameters[k].default is None for k in names[3:])
        assert list(inspect.signature(cls._descriptors).parameters)[2:] == ["geometries", "short", "codes"]
        assert inspect.signature(cls._descriptors).parameters["codes"].default is None  # positional callers unchanged
        lst = _host_list(cls)
        with pytest.raises(ore.OreError, match="2 orientations for 0 images"):
            lst.set_oriented([], [6, 6])
        with pytest.raises(ore.OreError, match="orientations is None"):
            lst.set_oriented([], None)
        for bad in (0, 9, -1, 6.0, True, "6"):
            with pytest.raises(ore.OreError, match=r"orientations\[0\].*EXIF code"):
                lst.set_oriented([None], [bad])  # the code is judged before the image
        with pytest.raises(ore.OreError, match="not both"):
            lst.set_oriented([], [], geometries=[], short=8)
        with pytest.raises(ore.OreError, match="1 flips for 0 images"):
            lst.set_oriented([], [], flips=[True])
        with pytest.raises(ore.OreError, match="exceed the list's capacity"):
            lst.set_oriented([None] * 5, [1] * 5)
        assert lst._images == () and not hasattr(lst, "_codes")  # nothing was kept: the codes travel as an argument
    lst = _host_list()
    with pytest.raises(ore.OreError, match="uint8 CUDA"):  # the images' own checks still run
        lst.set_oriented([torch.zeros((4, 4, 3), dtype=torch.uint8)], [6])
    assert not hasattr(lst, "_codes") and set(vars(lst)) == {"ctx", "capacity", "channels", "out_hw", "h", "_images"}
