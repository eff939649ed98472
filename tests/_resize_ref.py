"""The resize arithmetic of include/ore.h (ore_preprocess_resize_u8) restated in numpy, for the resize tests.
Integer tap map per axis, then four float32 operations per lerp, each rounded on its own: numpy's float32
array arithmetic never contracts a multiply and an add, so this is the definition bit for bit."""
import numpy as np


def taps_ref(S, D, origin, count):
    """One axis: S source samples resized to D, resized indices origin .. origin + count - 1."""
    o = origin + np.arange(count, dtype=np.int64)
    num = np.maximum((2 * o + 1) * S - D, 0)
    i0, rem = num // (2 * D), num % (2 * D)
    last = i0 >= S - 1
    i0, rem = np.where(last, S - 1, i0), np.where(last, 0, rem)
    i1 = np.minimum(i0 + 1, S - 1)
    t = rem.astype(np.float32) / np.float32(2 * D)
    assert t.dtype == np.float32
    return i0.astype(np.int32), i1.astype(np.int32), t


def resize_ref(x, resized_hw, origin, out_hw, scale=None, shift=None, reverse=False):
    """x uint8 [n, Hs, Ws, C] -> float32 [n, C, H, W]."""
    n, hs, ws, c = x.shape
    (rh, rw), (top, left), (h, w) = resized_hw, origin, out_hw
    y0, y1, ty = taps_ref(hs, rh, top, h)
    x0, x1, tx = taps_ref(ws, rw, left, w)
    if reverse:
        x = x[..., ::-1]
    xf = x.astype(np.float32)
    r0, r1 = xf[:, y0], xf[:, y1]
    a, b, cc, d = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]  # [n, H, W, C]
    tx, ty = tx.reshape(1, 1, w, 1), ty.reshape(1, h, 1, 1)
    up = a + (b - a) * tx
    lo = cc + (d - cc) * tx
    v = np.ascontiguousarray((up + (lo - up) * ty).transpose(0, 3, 1, 2))
    scale = np.ones(c, np.float32) if scale is None else np.asarray(scale, np.float32)
    shift = np.zeros(c, np.float32) if shift is None else np.asarray(shift, np.float32)
    out = (v * scale.reshape(1, c, 1, 1)) + shift.reshape(1, c, 1, 1)
    assert out.dtype == np.float32
    return out


def images(shape, seed=0):
    """Seeded random bytes; where the batch has room for them, every one of the 256 byte values occurs."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=shape, dtype=np.uint8)
    if x.size >= 256:
        flat = x.reshape(-1)
        flat[rng.choice(x.size, 256, replace=False)] = np.arange(256, dtype=np.uint8)
        assert len(np.unique(x)) == 256
    return x
