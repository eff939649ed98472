"""numpy restatement of the NV12 colour conversion (include/ore.h, csrc/ore_yuv.h), written from the formula and
sharing no code with the library: int64 arithmetic, floor shifts, nearest chroma."""
import numpy as np

# {yoff, cy, cvr, cug, cvg, cub}: round(k * 2^20) of the three-decimal constants
MATRICES = {
    "bt601": (16, 1220542, 1673527, 409993, 852492, 2116026),
    "bt709": (16, 1220542, 1880097, 223347, 558891, 2214593),
    "bt601_full": (0, 1048576, 1470104, 360853, 748826, 1858077),
}
# the constants themselves, for the float64 formula
CONSTANTS = {
    "bt601": (16, 1.164, 1.596, 0.391, 0.813, 2.018),
    "bt709": (16, 1.164, 1.793, 0.213, 0.533, 2.112),
    "bt601_full": (0, 1.0, 1.402, 0.344, 0.714, 1.772),
}
NAMES = list(MATRICES)


def yuv_to_rgb_ref(y, u, v, matrix):
    """uint8 arrays of one shape -> uint8 [..., 3], and the largest accumulator magnitude met."""
    yoff, cy, cvr, cug, cvg, cub = MATRICES[matrix]
    y, u, v = (np.asarray(a).astype(np.int64) for a in (y, u, v))
    u, v = u - 128, v - 128
    luma = np.maximum(y - yoff, 0) * cy + (1 << 19)
    acc = np.stack([luma + cvr * v, luma - cug * u - cvg * v, luma + cub * u], axis=-1)
    return np.clip(acc >> 20, 0, 255).astype(np.uint8), int(np.abs(acc).max())  # >> on int64 floors


def yuv_to_rgb_float(y, u, v, matrix):
    """clamp(floor(the float64 formula + 0.5)) per channel, as int64 [..., 3]."""
    yoff, ky, kvr, kug, kvg, kub = CONSTANTS[matrix]
    y, u, v = (np.asarray(a).astype(np.float64) for a in (y, u, v))
    u, v = u - 128.0, v - 128.0
    luma = np.maximum(y - yoff, 0.0) * ky
    f = np.stack([luma + kvr * v, luma - kug * u - kvg * v, luma + kub * u], axis=-1)
    return np.clip(np.floor(f + 0.5), 0, 255).astype(np.int64)


def nv12_to_rgb_ref(y_plane, uv_plane, matrix):
    """[Hs, Ws] and [ceil(Hs/2), ceil(Ws/2), 2] -> [Hs, Ws, 3]: pixel (r, j) takes the pair at (r >> 1, j >> 1)."""
    hs, ws = y_plane.shape
    assert uv_plane.shape == ((hs + 1) // 2, (ws + 1) // 2, 2)
    uv = np.repeat(np.repeat(uv_plane, 2, axis=0), 2, axis=1)[:hs, :ws]
    return yuv_to_rgb_ref(y_plane, uv[..., 0], uv[..., 1], matrix)[0]
