"""The cubic resize filters of include/ore.h (ORE_FILTER_BICUBIC = 256, ORE_FILTER_BICUBIC_AA = 257) restated in
numpy, for the resize_cubic tests.  The taps come from the definitions (a floor and a clamp; a brute-force scan of
every source sample), not from the library's closed forms.  Everything is float32 array arithmetic, one rounding
per operation in the order the header fixes (numpy never contracts a multiply and an add), and the taps are
accumulated by Python loops in ascending order: this is the definition bit for bit."""
import numpy as np

BICUBIC, BICUBIC_AA = 256, 257
AA_MAX_RATIO, MAX_TAPS = 16, 64
f32 = np.float32


def _near(a, b, z):
    """((a z + b) z) z + 1, left to right"""
    r = f32(a) * z
    r = r + f32(b)
    r = r * z
    r = r * z
    return r + f32(1)


def _far(a, b, c, d, z):
    """((a z + b) z + c) z + d, left to right"""
    r = f32(a) * z
    r = r + f32(b)
    r = r * z
    r = r + f32(c)
    r = r * z
    return r + f32(d)


def cubic_taps_ref(S, D, origin, count):
    """Plain cubic, one axis: (first int64 [count], w float32 [count, 4]); tap k of index i reads sample
    clamp(first[i] + k, 0, S - 1)."""
    o = np.arange(origin, origin + count, dtype=np.int64)
    num = (2 * o + 1) * S - D
    i = num // (2 * D)  # numpy floors
    assert (i >= -1).all() and (i <= S - 1).all()
    rem = num - 2 * D * i
    t = rem.astype(f32) / f32(2 * D)
    s = f32(1) - t
    w = np.stack([_far(-0.75, 3.75, -6, 3, t + f32(1)), _near(1.25, -2.25, t), _near(1.25, -2.25, s),
                  _far(-0.75, 3.75, -6, 3, s + f32(1))], axis=1)
    assert w.dtype == f32
    return i - 1, w


def cubic_aa_taps_ref(S, D, origin, count):
    """Antialiased cubic, one axis: per resized index (first, w float32 [ntaps], W float32) over every j of [0, S - 1]
    with |(2 j + 1) D - (2 o + 1) S| < 4 max(S, D)."""
    G = 2 * max(S, D)
    j = np.arange(S, dtype=np.int64)
    out = []
    for o in range(origin, origin + count):
        a = np.abs((2 * j + 1) * D - (2 * o + 1) * S)
        idx = np.nonzero(a < 2 * G)[0]
        assert len(idx) >= 1 and np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx)))  # contiguous, not empty
        a = a[idx]
        z = a.astype(f32) / f32(G)
        w = np.where(a < G, _near(1.5, -2.5, z), _far(-0.5, 2.5, -4, 2, z)).astype(f32)
        W = f32(0)
        for wj in w:
            W = W + wj
        out.append((int(idx[0]), w, f32(W)))
    return out


def _finish(v, c, scale, shift):
    assert v.dtype == f32
    v = np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    scale = np.ones(c, f32) if scale is None else np.asarray(scale, f32)
    shift = np.zeros(c, f32) if shift is None else np.asarray(shift, f32)
    out = (v * scale.reshape(1, c, 1, 1)) + shift.reshape(1, c, 1, 1)
    assert out.dtype == f32
    return out


def _cubic_plain(xf, resized_hw, origin, out_hw):
    n, hs, ws, c = xf.shape
    (rh, rw), (top, left), (h, w) = resized_hw, origin, out_hw
    fx, wx = cubic_taps_ref(ws, rw, left, w)
    fy, wy = cubic_taps_ref(hs, rh, top, h)
    # horizontal, for every source row: g [n, Hs, W, C]
    g = None
    for j in range(4):
        term = wx[:, j].reshape(1, 1, w, 1) * xf[:, :, np.clip(fx + j, 0, ws - 1)]
        g = term if g is None else g + term
    v = None
    for k in range(4):
        term = wy[:, k].reshape(1, h, 1, 1) * g[:, np.clip(fy + k, 0, hs - 1)]
        v = term if v is None else v + term
    return v


def _cubic_aa(xf, resized_hw, origin, out_hw):
    n, hs, ws, c = xf.shape
    (rh, rw), (top, left), (h, w) = resized_hw, origin, out_hw
    cols = cubic_aa_taps_ref(ws, rw, left, w)
    rows = cubic_aa_taps_ref(hs, rh, top, h)
    g = np.empty((n, hs, w, c), f32)
    for q, (f, u, _) in enumerate(cols):
        acc = np.zeros((n, hs, c), f32)
        for j, uj in enumerate(u):  # ascending source column
            acc = acc + uj * xf[:, :, f + j]
        g[:, :, q] = acc
    U = np.array([t[2] for t in cols], f32).reshape(1, w, 1)
    v = np.empty((n, h, w, c), f32)
    for r, (f, vv, V) in enumerate(rows):
        acc = np.zeros((n, w, c), f32)
        for i, vi in enumerate(vv):  # ascending source row
            acc = acc + vi * g[:, f + i]
        v[:, r] = (acc / V) / U
    return v


def resize_cubic_ref(x, resized_hw, origin, out_hw, antialias=False, scale=None, shift=None, reverse=False):
    """x uint8 [n, Hs, Ws, C] -> float32 [n, C, H, W] under filter 256 (antialias False) or 257."""
    if reverse:
        x = x[..., ::-1]
    xf = x.astype(f32)
    v = (_cubic_aa if antialias else _cubic_plain)(xf, resized_hw, origin, out_hw)
    return _finish(v, x.shape[3], scale, shift)
