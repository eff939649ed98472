"""include/ore.h's int8 search in numpy, every float32 operation rounded on its own: quant() is the row quantiser of the
packer and of the kernel's query path, scores() the two-multiply score, best() the k first of ore_topk_f32's order."""
import functools

import numpy as np


def quant(x):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        a = np.fmax.reduce(np.abs(x), axis=1, initial=np.float32(0))  # fmax skips NaNs
        t, inv = a / np.float32(127), np.float32(127) / a
        r = x * inv[:, None]
        codes = np.where(np.isnan(r), 0, np.rint(np.clip(r, -127, 127))).astype(np.int8)
    return codes, t.astype(np.float32)


def scores(cq, tq, cg, tg):
    dot = cq.astype(np.int64) @ cg.astype(np.int64).T
    with np.errstate(all="ignore"):
        return (dot.astype(np.float32) * tq[:, None].astype(np.float32)) * tg[None, :].astype(np.float32)


def best(s, k):
    idx = np.argsort(-s, axis=1, kind="stable")[:, :k]  # NaNs last, ties by index
    v = np.take_along_axis(s, idx, 1) + np.float32(0)   # -0 comes back as +0
    v[np.isnan(v)] = np.float32(np.nan)                 # and a NaN as 0x7fc00000
    return v.view(np.uint32), idx


@functools.lru_cache(maxsize=None)
def normal(D, n=33, G=4099):
    rng = np.random.default_rng(D)
    return rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((G, D)).astype(np.float32)
