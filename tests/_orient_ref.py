"""The orientation semantics of include/ore.h (ore_image_list_set_oriented) restated in numpy, for the orientation
tests: the pixel table by explicit index arrays, the displayed -> stored geometry map, and the defined result of an
oriented descriptor -- the numpy reference resize of the STORED image over the stored-space window, permuted."""
import numpy as np

from _resize_aa_ref import resize_aa_ref
from _resize_cubic_ref import resize_cubic_ref
from _resize_ref import resize_ref

CODES = (1, 2, 3, 4, 5, 6, 7, 8)
REV_ROWS, REV_COLS, TRANSPOSE = (3, 4, 6, 7), (2, 3, 7, 8), (5, 6, 7, 8)

# filter name -> (antialias, cubic) as the lists take them, and the numpy reference of the unoriented resize
FILTERS = {
    "bilinear": ((False, False), resize_ref),
    "aa": ((True, False), resize_aa_ref),
    "bicubic": ((False, True), lambda x, *a, **k: resize_cubic_ref(x, *a, antialias=False, **k)),
    "bicubic_aa": ((True, True), lambda x, *a, **k: resize_cubic_ref(x, *a, antialias=True, **k)),
}


def stored_index(code, r, c, hs, ws):
    """The table: displayed pixel (r, c) of a stored hs x ws image is stored pixel (a, b)."""
    return {1: (r, c), 2: (r, ws - 1 - c), 3: (hs - 1 - r, ws - 1 - c), 4: (hs - 1 - r, c),
            5: (c, r), 6: (hs - 1 - c, r), 7: (hs - 1 - c, ws - 1 - r), 8: (c, ws - 1 - r)}[code]


def displayed_hw(src_hw, code):
    return (src_hw[1], src_hw[0]) if code in TRANSPOSE else tuple(src_hw)


def apply_orientation_ref(x, code):
    """x [hs, ws, ...] -> the displayed image, by the table alone (a gather, no flips or transposes)."""
    hs, ws = x.shape[:2]
    dh, dw = displayed_hw((hs, ws), code)
    r, c = np.meshgrid(np.arange(dh), np.arange(dw), indexing="ij")
    a, b = stored_index(code, r, c, hs, ws)
    return x[a, b]


def orient_geometry_ref(code, resized_hw, origin, out_hw):
    """((rh_s, rw_s), (top_s, left_s), (hz, wz), rev_rows, rev_cols, transpose) of a displayed-space geometry."""
    (rh, rw), (top, left), (h, w) = resized_hw, origin, out_hw
    rr, rc, tr = code in REV_ROWS, code in REV_COLS, code in TRANSPOSE
    rh_s, rw_s = (rw, rh) if tr else (rh, rw)
    hz, wz = (w, h) if tr else (h, w)
    a0, b0 = (left, top) if tr else (top, left)
    return (rh_s, rw_s), (rh_s - hz - a0 if rr else a0, rw_s - wz - b0 if rc else b0), (hz, wz), rr, rc, tr


def permute(z, rev_rows, rev_cols, transpose):
    """[..., hz, wz] of the stored window -> [..., h, w] of the displayed one: reverse, then transpose."""
    if rev_rows:
        z = z[..., ::-1, :]
    if rev_cols:
        z = z[..., :, ::-1]
    return np.swapaxes(z, -1, -2) if transpose else z


def oriented_ref(fn, x, code, resized_hw, origin, out_hw, flip=False, **kw):
    """The definition: x uint8 [hs, ws, C] stored -> float32 [C, h, w].  fn is a FILTERS reference."""
    rs, os_, hzwz, rr, rc, tr = orient_geometry_ref(code, resized_hw, origin, out_hw)
    y = permute(fn(x[None], rs, os_, hzwz, **kw)[0], rr, rc, tr)
    assert y.shape[1:] == tuple(out_hw)
    return np.ascontiguousarray(y[..., ::-1] if flip else y)


def check_table_against_definition(code, resized_hw, origin, out_hw):
    """The stored-window form equals the table form of the issue: element (i, j), r = top + i, c = left + j, reads
    resized stored (a, b) = stored_index(code, r, c, rh_s, rw_s).  Returns the two index grids for comparison."""
    (rh_s, rw_s), (top_s, left_s), (hz, wz), rr, rc, tr = orient_geometry_ref(code, resized_hw, origin, out_hw)
    i, j = np.meshgrid(np.arange(out_hw[0]), np.arange(out_hw[1]), indexing="ij")
    a, b = stored_index(code, origin[0] + i, origin[1] + j, rh_s, rw_s)
    u, v = np.meshgrid(np.arange(hz), np.arange(wz), indexing="ij")
    wa, wb = permute(top_s + u, rr, rc, tr), permute(left_s + v, rr, rc, tr)
    return (a, b), (wa, wb)
