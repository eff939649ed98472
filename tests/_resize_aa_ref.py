"""The antialiased resize of include/ore.h (ore_preprocess_resize_u8_ex, ORE_FILTER_BILINEAR_AA) restated in
numpy, for the resize_aa tests.  The taps come from the set definition by brute force, not from the library's
closed form; the column sums are exact in int64, everything after them is float32 array arithmetic, one
rounding per operation (numpy never contracts a multiply and an add), and the row taps are accumulated by a
Python loop in ascending order: this is the definition bit for bit.  Axes that do not shrink fall back to
_resize_ref.taps_ref."""
import numpy as np

from _resize_ref import taps_ref

MAX_RATIO, MAX_TAPS = 32, 64


def aa_taps_ref(S, D, origin, count):
    """One shrinking axis (S > D): per resized index origin .. origin + count - 1 the first tap and the int64
    weights of its taps: every j of [0, S - 1] with |(2 j + 1) D - (2 o + 1) S| < 2 S, u_j = 2 S - |...|."""
    assert S > D
    j = np.arange(S, dtype=np.int64)
    out = []
    for o in range(origin, origin + count):
        u = 2 * S - np.abs((2 * j + 1) * D - (2 * o + 1) * S)
        idx = np.nonzero(u > 0)[0]
        assert len(idx) >= 1 and np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx)))  # contiguous, not empty
        out.append((int(idx[0]), u[idx]))
    return out


def resize_aa_ref(x, resized_hw, origin, out_hw, scale=None, shift=None, reverse=False):
    """x uint8 [n, Hs, Ws, C] -> float32 [n, C, H, W]."""
    n, hs, ws, c = x.shape
    (rh, rw), (top, left), (h, w) = resized_hw, origin, out_hw
    if reverse:
        x = x[..., ::-1]
    # 1. horizontal, for every source row: g [n, Hs, W, C] float32
    if ws > rw:
        cols = aa_taps_ref(ws, rw, left, w)
        x64 = x.astype(np.int64)
        g = np.stack([np.tensordot(x64[:, :, f:f + len(u)], u, axes=([2], [0])) for f, u in cols], axis=2).astype(np.float32)
        usum = np.array([int(u.sum()) for _, u in cols], np.float32).reshape(1, 1, w, 1)
    else:
        x0, x1, tx = taps_ref(ws, rw, left, w)
        xf = x.astype(np.float32)
        a, b = xf[:, :, x0], xf[:, :, x1]
        g = a + (b - a) * tx.reshape(1, 1, w, 1)
    assert g.dtype == np.float32 and g.shape == (n, hs, w, c)
    # 2. vertical: v [n, H, W, C]
    if hs > rh:
        v = np.empty((n, h, w, c), np.float32)
        for r, (f, u) in enumerate(aa_taps_ref(hs, rh, top, h)):
            acc = np.zeros((n, w, c), np.float32)
            for i, ui in enumerate(u):  # ascending source row
                acc = acc + np.float32(ui) * g[:, f + i]
            v[:, r] = acc / np.float32(int(u.sum()))
    else:
        y0, y1, ty = taps_ref(hs, rh, top, h)
        up, lo = g[:, y0], g[:, y1]
        v = up + (lo - up) * ty.reshape(1, h, 1, 1)
    # 3. the column weight sum
    if ws > rw:
        v = v / usum
    assert v.dtype == np.float32
    v = np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    scale = np.ones(c, np.float32) if scale is None else np.asarray(scale, np.float32)
    shift = np.zeros(c, np.float32) if shift is None else np.asarray(shift, np.float32)
    out = (v * scale.reshape(1, c, 1, 1)) + shift.reshape(1, c, 1, 1)
    assert out.dtype == np.float32
    return out
