"""CPU: the orientation map of the oriented image lists (include/ore.h: ore_orient_geometry).

ore_orient_geometry against a numpy restatement over a grid of windows; ore.apply_orientation against the pixel
table (and PIL's exif_transpose where PIL is installed); the window form of the definition against its table form;
and, with the numpy references of the four filters, what the definition is NOT: a resize of the rotated bytes.  The
two agree to rounding, and an image that is not resized comes out as the oriented bytes exactly."""
import ctypes
import itertools

import numpy as np
import pytest

import ore
from ore import _lib

from _orient_ref import (CODES, FILTERS, REV_COLS, REV_ROWS, TRANSPOSE, apply_orientation_ref, check_table_against_definition,
                         displayed_hw, orient_geometry_ref, oriented_ref, stored_index)
from _resize_ref import images

# (displayed resized size, output shape): windows at every combination of the borders and one strictly inside
SHAPES = [((5, 7), (5, 7)), ((9, 12), (5, 7)), ((40, 50), (17, 33)), ((17, 40), (17, 33)), ((20, 33), (17, 33))]


def _windows(resized, out):
    tops = sorted({0, (resized[0] - out[0]) // 2, resized[0] - out[0]})
    lefts = sorted({0, (resized[1] - out[1]) // 2, resized[1] - out[1]})
    return list(itertools.product(tops, lefts))


def test_orient_geometry_matches_the_restatement():
    seen = set()
    for code in CODES:
        for resized, out in SHAPES:
            for origin in _windows(resized, out):
                got = ore.orient_geometry(code, resized, origin, out)
                want = orient_geometry_ref(code, resized, origin, out)
                assert got == want, (code, resized, origin, out)
                (rh_s, rw_s), (top_s, left_s), (hz, wz), rr, rc, tr = got
                assert (rr, rc, tr) == (code in REV_ROWS, code in REV_COLS, code in TRANSPOSE)
                assert 0 <= top_s <= rh_s - hz and 0 <= left_s <= rw_s - wz  # the stored window is inside iff the displayed one is
                seen.add((top_s == 0, top_s == rh_s - hz, left_s == 0, left_s == rw_s - wz))
                # the window form is the table form: element (i, j) reads resized stored (a, b) of the table
                (a, b), (wa, wb) = check_table_against_definition(code, resized, origin, out)
                np.testing.assert_array_equal(a, wa)
                np.testing.assert_array_equal(b, wb)
    assert {(True, False, True, False), (False, True, False, True), (False, False, False, False)} <= seen  # all four borders, and none


def test_orient_geometry_raw_entry():
    L = ore.load()
    g = _lib.Resize(9, 12, 1, 2)
    sg = _lib.Resize()
    for bad in (0, 9, -1, 256 + 6):
        assert L.ore_orient_geometry(bad, ctypes.byref(g), 5, 7, ctypes.byref(sg), None, None, None, None, None) == 1
        assert b"orientation" in L.ore_last_error(None)
    assert L.ore_orient_geometry(6, None, 5, 7, ctypes.byref(sg), None, None, None, None, None) == 1
    assert L.ore_orient_geometry(6, ctypes.byref(g), 5, 7, None, None, None, None, None, None) == 0  # every output is optional
    tr = ctypes.c_int32(-1)
    assert L.ore_orient_geometry(6, ctypes.byref(g), 5, 7, ctypes.byref(sg), None, None, None, None, ctypes.byref(tr)) == 0
    assert tr.value == 1 and (sg.rh, sg.rw, sg.top, sg.left) == (12, 9, 12 - 7 - 2, 1)
    with pytest.raises(ore.OreError, match="orientation"):
        ore.orient_geometry(0, (9, 12), (1, 2), (5, 7))


def test_apply_orientation_is_the_table():
    import torch
    x = images((5, 9, 3), seed=1)
    for code in CODES:
        want = apply_orientation_ref(x, code)
        assert want.shape[:2] == ore.oriented_hw((5, 9), code) == displayed_hw((5, 9), code)
        got = ore.apply_orientation(x, code)
        np.testing.assert_array_equal(got, want)
        assert np.shares_memory(got, x)  # a view
        np.testing.assert_array_equal(ore.apply_orientation(torch.from_numpy(x), code).numpy(), want)
        np.testing.assert_array_equal(ore.apply_orientation(x[..., 0], code), want[..., 0])  # [H, W] alone
        for r, c in ((0, 0), (1, 3), (want.shape[0] - 1, want.shape[1] - 1)):
            a, b = stored_index(code, r, c, 5, 9)
            assert tuple(got[r, c]) == tuple(x[a, b])
    for bad in (0, 9, True, 6.0, None, "6"):
        with pytest.raises(ore.OreError, match="orientation"):
            ore.apply_orientation(x, bad)
        with pytest.raises(ore.OreError, match="orientation"):
            ore.oriented_hw((5, 9), bad)


def test_apply_orientation_is_exif_transpose():
    PIL = pytest.importorskip("PIL")
    from PIL import Image, ImageOps
    del PIL
    x = images((5, 9, 3), seed=2)
    for code in CODES:
        im = Image.fromarray(x)
        exif = im.getexif()
        exif[0x0112] = code
        im.info["exif"] = exif.tobytes()
        shown = np.asarray(ImageOps.exif_transpose(im))
        np.testing.assert_array_equal(ore.apply_orientation(x, code), shown, err_msg=f"code {code}")


def test_rotation_orientation():
    assert [ore.rotation_orientation(d) for d in (0, 90, 180, 270)] == [1, 6, 3, 8]
    assert ore.rotation_orientation(360) == 1 and ore.rotation_orientation(-90) == 8 and ore.rotation_orientation(450) == 6
    for bad in (45, 1, 90.0, None, True):
        with pytest.raises(ore.OreError, match="rotation_orientation"):
            ore.rotation_orientation(bad)
    # a frame to be rotated 90 degrees clockwise: its first stored column, bottom to top, becomes the first displayed row
    x = np.arange(6).reshape(2, 3)
    np.testing.assert_array_equal(ore.apply_orientation(x, ore.rotation_orientation(90)), np.rot90(x, -1))
    np.testing.assert_array_equal(ore.apply_orientation(x, ore.rotation_orientation(180)), np.rot90(x, 2))
    np.testing.assert_array_equal(ore.apply_orientation(x, ore.rotation_orientation(270)), np.rot90(x, 1))


# ---------------------------------------------------------------------------------- the definition and the rotated resize
# (stored size, output shape, displayed resized size, origin)
CASES = [((23, 31), (5, 7), (5, 7), (0, 0)), ((23, 31), (5, 7), (9, 12), (4, 5)), ((9, 13), (17, 33), (40, 50), (2, 3)),
         ((37, 53), (17, 33), (20, 36), (1, 2))]
# max |definition - reference resize of apply_orientation(x)| over CASES x CODES on 0..255 values, measured with the
# numpy references alone.  It is rounding (t against 1 - t, and the passes in the other order), so it
# depends on the inputs: the test allows twice the measured value.  A wrong index would show as whole grey levels.
MEASURED = {"bilinear": 3.06e-5, "aa": 3.06e-5, "bicubic": 1.99e-4, "bicubic_aa": 9.16e-5}


@pytest.mark.parametrize("name", list(FILTERS))
def test_definition_against_the_resize_of_the_rotated_bytes(name):
    fn = FILTERS[name][1]
    worst, differs = 0.0, False
    for k, (src, out, resized, origin) in enumerate(CASES):
        x = images(src + (3,), seed=900 + k)
        for code in CODES:
            shown = np.ascontiguousarray(apply_orientation_ref(x, code))
            got = oriented_ref(fn, x, code, resized, origin, out)
            want = fn(shown[None], resized, origin, out)[0]
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            differs |= code != 1 and err > 0
            assert err <= 2 * MEASURED[name], (name, code, k, err)
            if code == 1:
                assert err == 0.0
            # not resized: exactly the oriented bytes
            hw = displayed_hw(src, code)
            same = oriented_ref(fn, x, code, hw, (0, 0), hw)
            np.testing.assert_array_equal(same, shown.transpose(2, 0, 1).astype(np.float32))
    print(f"{name}: max difference {worst:.3g} (measured {MEASURED[name]:.3g})")
    assert differs  # it IS a different computation: the permutation of the resize, not the resize of the permutation
    assert worst >= MEASURED[name] / 2  # the recorded figure is this test's, not a stale one
