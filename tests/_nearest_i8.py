"""include/ore.h's int8 search in numpy, every float32 operation rounded on its own: quant() is the row quantiser of the
packer and of the kernel's query path, scores() the two-multiply score, best() the k first of ore_topk_f32's order.
bins_ref() is the candidate search on any scores; image() and keys() are ore_topk_key.h's 64-bit keys, bin_winners() and
bins_fast() the candidate search through them, and select_passes() says, from the keys alone, on which pass a radix
select over them ends."""
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


def bins_ref(s, B, c):
    """include/ore.h's candidate search: the per-bin first of best()'s order, then best() over the winners."""
    n, G = s.shape
    NB = -(-G // B)
    p = np.full((n, NB * B), np.nan, np.float32)  # absent rows: NaNs behind every row of their bin
    p[:, :G] = s
    rows = (best(p.reshape(n * NB, B), 1)[1][:, 0] + B * (np.arange(n * NB) % NB)).reshape(n, NB)
    v, i = best(np.take_along_axis(s, rows, 1), c)  # the winners stand in row order: ties by lower row
    return v, np.take_along_axis(rows, i, 1)


def image(s):
    """ore_topk_key.h's order image of float32 scores as uint32: 0 for a NaN, -0 folded to +0, the sign bit set for
    x >= 0, every bit flipped for x < 0."""
    s = np.asarray(s, np.float32)
    b = (s + np.float32(0)).view(np.uint32)  # -0 + 0 = +0
    return np.where(np.isnan(s), np.uint32(0), np.where(b >> 31 != 0, ~b, b | np.uint32(1 << 31))).astype(np.uint32)


def keys(s, rows):
    """The 64-bit keys image << 32 | ~row as uint64: larger is better, equal images by the lower row."""
    return image(s).astype(np.uint64) << np.uint64(32) | (~np.asarray(rows).astype(np.uint32)).astype(np.uint64)


def bin_winners(s, B):
    """The winner key of every bin, uint64 [n, NB], by a reshape and a max: keys are unique, so the largest key of a
    bin is its best image at the lowest row.  Absent rows have key 0, below every key of a row."""
    n, G = s.shape
    NB = -(-G // B)
    k = np.zeros((n, NB * B), np.uint64)
    k[:, :G] = keys(s, np.arange(G))
    return k.reshape(n, NB, B).max(axis=2)


def bins_fast(s, B, c, win=None):
    """bins_ref() through the keys, for galleries on which an argsort per bin is slow: (value bits, indices).  `win`:
    bin_winners(s, B), where the caller has them."""
    top = np.sort(bin_winners(s, B) if win is None else win, axis=1)[:, ::-1][:, :c]
    idx = (~top.astype(np.uint32)).astype(np.int64)
    v = np.take_along_axis(s, idx, 1) + np.float32(0)  # as best(): -0 comes back as +0, a NaN as 0x7fc00000
    v[np.isnan(v)] = np.float32(np.nan)
    return v.view(np.uint32), idx


def select_passes(keys_row, c, cap=512):
    """The passes a radix select from the top byte down makes over one query's keys before at most `cap` keys are
    left at or above the cut, restated from the rule and not from the kernel: at the byte at `shift` the cut is the
    c-th largest key's prefix through that byte.  [(shift, keys that rose above the cut in this pass, keys at or above
    the cut)], the last entry being the pass the select ends on."""
    k = np.asarray(keys_row, np.uint64)
    kc = np.sort(k)[len(k) - c]
    out, above = [], 0
    for shift in range(56, -8, -8):
        p = k >> np.uint64(shift)
        now = int((p > kc >> np.uint64(shift)).sum())
        out.append((shift, now - above, int((p >= kc >> np.uint64(shift)).sum())))
        above = now
        if out[-1][2] <= cap:
            break
    return out


def select_last_shift(keys_row, c, cap=512):
    return select_passes(keys_row, c, cap)[-1][0]


@functools.lru_cache(maxsize=None)
def normal(D, n=33, G=4099):
    rng = np.random.default_rng(D)
    return rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((G, D)).astype(np.float32)
