"""Shared by tests/test_cam_boxes.py (CPU) and tests/test_cam_boxes_gpu.py: the numpy restatement of the upsampled
class activation map and its threshold (include/ore.h, "Localisation from class activation maps"), an independent
pure-Python 8-connected labelling with the tie rule, and the case table.

Everything here is exact: float32 numpy arrays round every -, * and + on their own, as the kernels do, and the rest is
integers.  A case is (name, maps [planes, Hm, Wm] float32, (H, W), frac).  At identity scale (H = Hm, W = Wm) the
upsampled plane is the plane, so a 0 / 1 plane under 0 < frac <= 1 states an arbitrary mask."""
import collections
import functools

import numpy as np


# ------------------------------------------------------------------------------------------ the arithmetic
def taps(S, D):
    """(i0, i1, t) of ore_resize_taps(S, D, 0, D), restated: the source coordinate ((2 o + 1) S - D) / 2 D clamped at
    0, its floor and its fraction as one float32 division; at and past the last sample both taps are S - 1."""
    o = np.arange(D, dtype=np.int64)
    num = np.maximum((2 * o + 1) * S - D, 0)
    i0, rem = num // (2 * D), num % (2 * D)
    last = i0 >= S - 1
    i0, rem = np.where(last, S - 1, i0), np.where(last, 0, rem)
    t = rem.astype(np.float32) / np.float32(2 * D)
    return i0, np.minimum(i0 + 1, S - 1), t.astype(np.float32)


def lerp(a, b, t):
    """a + (b - a) t in float32, three roundings"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.subtract(b, a, dtype=np.float32)
        p = np.multiply(d, t, dtype=np.float32)
        return np.add(a, p, dtype=np.float32)


def upsample(m, hw):
    """one plane [Hm, Wm] -> [H, W]"""
    m = np.asarray(m, dtype=np.float32)
    H, W = hw
    y0, y1, ty = taps(m.shape[0], H)
    x0, x1, tx = taps(m.shape[1], W)
    top = lerp(m[y0][:, x0], m[y0][:, x1], tx[None, :])
    bot = lerp(m[y1][:, x0], m[y1][:, x1], tx[None, :])
    return lerp(top, bot, ty[:, None])


def threshold(u, frac):
    """thr = lo + frac (hi - lo) over the non-NaN elements (NaN when there is none), in float32"""
    with np.errstate(invalid="ignore"):
        lo, hi = np.fmin.reduce(u.ravel()), np.fmax.reduce(u.ravel())
    return lerp(np.float32(lo), np.float32(hi), np.float32(frac))


def mask_of(u, frac):
    with np.errstate(invalid="ignore"):
        return u >= threshold(u, frac)  # a NaN on either side is False


def components(mask):
    """The 8-connected components of a boolean mask in the order of their first pixels in raster order: a list of
    (count, (top, left, bottom, right)), half-open.  A plain breadth-first search, independent of the library."""
    H, W = mask.shape
    todo = mask.copy()
    out = []
    for s in np.flatnonzero(mask.ravel()):
        r, q = divmod(int(s), W)
        if not todo[r, q]:
            continue
        todo[r, q] = False
        queue = collections.deque([(r, q)])
        n, t, l, b, rt = 0, r, q, r, q
        while queue:
            r, q = queue.popleft()
            n += 1
            t, l, b, rt = min(t, r), min(l, q), max(b, r), max(rt, q)
            for r2 in range(max(r - 1, 0), min(r + 2, H)):
                for q2 in range(max(q - 1, 0), min(q + 2, W)):
                    if todo[r2, q2]:
                        todo[r2, q2] = False
                        queue.append((r2, q2))
        out.append((n, (t, l, b + 1, rt + 1)))
    return out


def largest(mask):
    """((top, left, bottom, right), area) of the largest component; the first of equals; (0, 0, 0, 0), 0 when empty"""
    best = (0, (0, 0, 0, 0))
    for comp in components(mask):
        if comp[0] > best[0]:
            best = comp
    return best[1], best[0]


def box_of(u, frac):
    return largest(mask_of(np.asarray(u, dtype=np.float32), frac))


# ------------------------------------------------------------------------------------------ the masks at 64 x 64
def spiral(n=64):
    """a one-pixel-wide path wound inwards with one empty pixel between its arms: one component whose flood fill
    has to walk its whole length"""
    g = np.zeros((n, n), np.float32)
    r = c = 0
    dr, dc = 0, 1
    g[0, 0] = 1
    while True:
        for _ in range(2):  # straight on, or one turn to the right
            nr, nc, ar, ac = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if 0 <= nr < n and 0 <= nc < n and not g[nr, nc] and not (0 <= ar < n and 0 <= ac < n and g[ar, ac]):
                r, c = nr, nc
                g[r, c] = 1
                break
            dr, dc = dc, -dr
        else:
            return g


def tie_blobs(n=64):
    """two 4 x 4 blobs: the upper one lies to the right, so it is first in raster order and second in column order"""
    g = np.zeros((n, n), np.float32)
    g[5:9, 40:44] = 1
    g[20:24, 3:7] = 1
    return g


def diagonal_blobs(n=64):
    """two 5 x 5 blobs touching at one corner (50 pixels under 8-connectivity, 25 + 25 under 4) and one of 30"""
    g = np.zeros((n, n), np.float32)
    g[10:15, 10:15] = 1
    g[15:20, 15:20] = 1
    g[40:45, 30:36] = 1
    return g


def dots(n=64):
    g = np.zeros((n, n), np.float32)
    g[::2, ::2] = 1
    return g


def frame(n=64):
    """a frame two pixels thick whose hole holds a smaller blob"""
    g = np.zeros((n, n), np.float32)
    g[4:60, 4:60] = 1
    g[6:58, 6:58] = 0
    g[20:31, 22:33] = 1
    return g


MASKS = {"spiral": spiral, "tie": tie_blobs, "diagonal": diagonal_blobs, "dots": dots, "full": lambda n=64: np.ones((n, n), np.float32),
         "frame": frame}


# ------------------------------------------------------------------------------------------ the case table
def _rand(seed, planes, hm, wm):
    return np.random.default_rng(seed).standard_normal((planes, hm, wm)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        ("1x1-id", np.full((1, 1, 1), 3.0, np.float32), (1, 1), 0.2),
        ("1x1-7x5", np.full((1, 1, 1), -2.0, np.float32), (7, 5), 0.2),
        ("3x2-id", _rand(1, 1, 3, 2), (3, 2), 0.2),
        ("4x5-33x70", _rand(2, 7, 4, 5), (33, 70), 0.2),           # W crosses two bitmap words; seven workgroups
        ("4x5-33x70-frac0", _rand(2, 7, 4, 5), (33, 70), 0.0),     # everything that is not NaN
        ("4x5-33x70-frac1", _rand(2, 7, 4, 5), (33, 70), 1.0),     # the maxima alone
        ("17x17-64x65", _rand(3, 1, 17, 17), (64, 65), 0.2),       # one bit in the last word
        ("2x9-40x512", _rand(4, 1, 2, 9), (40, 512), 0.2),         # the side cap, 16 words per row
        ("9x2-512x40", _rand(5, 1, 9, 2), (512, 40), 0.2),
        ("13x13-224x224", _rand(6, 1, 13, 13), (224, 224), 0.2),   # the product's shapes
        ("17x17-288x288", _rand(7, 1, 17, 17), (288, 288), 0.2),
        ("64x64-512x512", _rand(11, 1, 64, 64), (512, 512), 0.9),  # all three caps at once: the most LDS; few pixels pass
        # a higher threshold cuts random planes into several components: the choice among them
        ("13x13-224x224-frac06", _rand(6, 1, 13, 13), (224, 224), 0.6),
        ("4x5-33x70-frac06", _rand(2, 7, 4, 5), (33, 70), 0.6),
    ]
    for name in sorted(MASKS):
        out.append((f"64x64-{name}", MASKS[name]()[None], (64, 64), 0.5))
    out.append(("constant", np.full((1, 5, 4), 2.5, np.float32), (20, 16), 0.2))
    nans = _rand(8, 7, 6, 6)
    nans[:, 1, 2] = np.nan
    nans[3, 4:, :3] = np.nan
    out.append(("nans", nans, (24, 24), 0.2))
    out.append(("all-nan", np.full((1, 3, 3), np.nan, np.float32), (8, 8), 0.2))
    inf = _rand(9, 1, 5, 5)
    inf[0, 2, 3] = np.inf
    out.append(("inf", inf, (20, 20), 0.2))
    out.append(("inf-frac0", inf, (20, 20), 0.0))  # thr = lo + 0 * inf is NaN: an empty mask
    out.append(("negative", -np.abs(_rand(10, 1, 6, 7)) - np.float32(1), (30, 29), 0.2))  # no Relu in front
    for c in out:
        c[1].setflags(write=False)
    return tuple(out)


def case_id(case):
    return case[0]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(upsampled planes [planes, H, W], boxes int32 [planes, 4], areas int32 [planes]) of a case, computed once"""
    _, maps, hw, frac = next(c for c in cases() if c[0] == name)
    u = np.stack([upsample(m, hw) for m in maps])
    res = [box_of(p, frac) for p in u]
    boxes, areas = np.array([r[0] for r in res], np.int32), np.array([r[1] for r in res], np.int32)
    for a in (u, boxes, areas):
        a.setflags(write=False)
    return u, boxes, areas
