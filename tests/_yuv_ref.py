"""numpy restatement of the YUV image lists' pixel rule (include/ore.h, ore_yuv_format), sharing no code with the
library: each format's planes expanded to [hs, ws, 3] with nearest chroma -- source pixel (r, j) takes the sample at
(r >> sy, j >> sx) -- through the integer conversion of tests/_nv12_ref.py.  The result feeds tests/_resize_ref.py and
tests/_resize_aa_ref.py.  Also the plane makers the tests share."""
import numpy as np

from _nv12_ref import yuv_to_rgb_ref
from _resize_ref import images

# format -> (ore_yuv_format id, sx, sy); sx, sy are None where the format has no chroma
FORMATS = {"nv12": (0, 1, 1), "yuyv": (1, 1, 0), "i444": (2, 0, 0), "i440": (3, 0, 1), "i422": (4, 1, 0),
           "i420": (5, 1, 1), "i411": (6, 2, 0), "gray": (7, None, None)}
NAMES = list(FORMATS)


def _ceil_shift(n, s):
    return (n + (1 << s) - 1) >> s


def plane_shapes(fmt, hs, ws):
    """The planes of an hs x ws frame, as ore.YuvImageList.set and ore.yuv_planes_to_rgb take them."""
    _, sx, sy = FORMATS[fmt]
    if fmt == "gray":
        return [(hs, ws)]
    hc, wc = _ceil_shift(hs, sy), _ceil_shift(ws, sx)
    if fmt == "yuyv":
        return [(hs, wc, 4)]
    if fmt == "nv12":
        return [(hs, ws), (hc, wc, 2)]
    return [(hs, ws), (hc, wc), (hc, wc)]


def yuv_split(fmt, planes, ws=None):
    """The planes of a frame -> full-resolution uint8 (Y, U, V), each [hs, ws]; ws states the width of a YUYV frame
    when it is odd."""
    if fmt == "yuyv":
        g = planes[0]
        hs, wc = g.shape[:2]
        ws = 2 * wc if ws is None else ws
        assert ws in (2 * wc, 2 * wc - 1)
        y = np.stack([g[..., 0], g[..., 2]], axis=-1).reshape(hs, 2 * wc)[:, :ws]
        u = np.repeat(g[..., 1], 2, axis=1)[:, :ws]
        v = np.repeat(g[..., 3], 2, axis=1)[:, :ws]
        return y, u, v
    y = planes[0]
    hs, ws = y.shape
    if fmt == "gray":
        grey = np.full((hs, ws), 128, np.uint8)
        return y, grey, grey
    _, sx, sy = FORMATS[fmt]
    if fmt == "nv12":
        cu, cv = planes[1][..., 0], planes[1][..., 1]
    else:
        cu, cv = planes[1], planes[2]
    assert cu.shape == cv.shape == (_ceil_shift(hs, sy), _ceil_shift(ws, sx))
    up = lambda c: np.repeat(np.repeat(c, 1 << sy, axis=0), 1 << sx, axis=1)[:hs, :ws]  # noqa: E731
    return y, up(cu), up(cv)


def yuv_planes_to_rgb_ref(fmt, planes, matrix, ws=None):
    y, u, v = yuv_split(fmt, planes, ws)
    return yuv_to_rgb_ref(y, u, v, matrix)[0]


def make_planes(fmt, hs, ws, seed):
    """Seeded random planes of an hs x ws frame; bytes cover 0..255 where there is room, so the clamps are met."""
    return [images(shape, seed=seed + 1000 * k) for k, shape in enumerate(plane_shapes(fmt, hs, ws))]


def extremes(fmt):
    """A 4 x 6 frame in quadrants: Y = 255 in the upper rows and 0 in the lower, U = V = 0 in the left chroma columns
    and 255 in the right.  The triples (255, 0, 0), (255, 255, 255), (0, 0, 0) and (0, 255, 255) drive R, G and B
    each past both clamps."""
    hs, ws = 4, 6
    out = []
    for k, shape in enumerate(plane_shapes(fmt, hs, ws)):
        rows, cols = shape[:2]
        lum = np.where(np.arange(rows)[:, None] < rows // 2, 255, 0)   # [rows, 1]
        chroma = np.where(np.arange(cols)[None, :] < cols // 2, 0, 255)  # [1, cols]
        p = np.empty(shape, np.uint8)
        if fmt == "yuyv":
            p[..., 0::2] = lum[:, :, None]
            p[..., 1::2] = chroma[:, :, None]
        elif k == 0:
            p[...] = lum
        else:
            p[...] = chroma.reshape((1, cols) + (1,) * (len(shape) - 2))
        out.append(p)
    return out


def frame(fmt, planes, ws=None):
    """The tuple ore.YuvImageList.set takes for planes (any array or tensor type): the width rides along where a
    YUYV frame's is odd."""
    return (fmt, *planes) if ws is None else (fmt, *planes, int(ws))


def yuyv_width(fmt, ws):
    """The ws argument of a frame of this format and width: stated for an odd YUYV frame alone."""
    return ws if fmt == "yuyv" and ws % 2 else None
