"""The fp16 layer checker (_convref.f16_layer_check) has teeth: on one 3x3 layer (K = 576, bias, Relu)
it accepts a k-ordered f32 accumulation rounded to nearest even, and rejects the same sums rounded
toward zero and a float16 accumulation.  No GPU: the three "kernels" are numpy emulations."""
import numpy as np

from _convref import F16_AMBIGUOUS_CAP, f16_layer_bounds, f16_layer_check


def _layer():
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((2, 64, 6, 6)).astype(np.float32)
    w = (rng.standard_normal((32, 64, 3, 3)) * np.sqrt(2.0 / 576)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, 32).astype(np.float32)
    return x, w, b


def _columns(x):
    """im2col of a 3x3 pad-1 stride-1 conv, k = (c, r, s): [N, K, H * W] of the f16 operands."""
    N, C, H, W = x.shape
    xp = np.zeros((N, C, H + 2, W + 2), np.float16)
    xp[:, :, 1:-1, 1:-1] = x.astype(np.float16)
    cols = np.stack([xp[:, :, r:r + H, s:s + W] for r in range(3) for s in range(3)], axis=2)
    return cols.reshape(N, C * 9, H * W)


def _accumulate(x, w, b, acc_t):
    """sum_k f16(w) f16(x) one k at a time in acc_t, + bias, Relu; [N, M, H, W] of acc_t."""
    cols = _columns(x).astype(acc_t)
    wm = w.astype(np.float16).reshape(w.shape[0], -1).astype(acc_t)
    acc = np.zeros((x.shape[0], w.shape[0], cols.shape[2]), acc_t)
    for k in range(wm.shape[1]):
        acc = (acc + wm[None, :, k, None] * cols[:, None, k, :]).astype(acc_t)
    acc = (acc + b.astype(acc_t)[None, :, None]).astype(acc_t)
    return np.maximum(acc, acc_t(0)).reshape(x.shape[0], w.shape[0], x.shape[2], x.shape[3])


def _toward_zero(v):
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h)


def test_f16_checker_accepts_rne_rejects_truncation_and_f16_accumulation():
    x, w, b = _layer()
    v32 = _accumulate(x, w, b, np.float32)
    args = (x, w, b, [1, 1, 1, 1], (1, 1), True)

    good = f16_layer_check(v32.astype(np.float16).astype(np.float32), *args)
    print(f"rne: bad {good['bad']:.4f} ambiguous {good['ambiguous']:.4f} acc_ratio {good['acc_ratio']:.3e}")
    assert good["ok"].all()
    assert 0.0 < good["ambiguous"] <= F16_AMBIGUOUS_CAP
    assert good["acc_ratio"] <= 2e-6
    assert (v32 > 0).mean() > 0.3  # not a dead layer: the Relu leaves a rounding to check

    # truncation keeps the nearest f16 only where it lies toward zero: half of the non-zero outputs
    # differ, fewer by the ambiguous ones
    trunc = f16_layer_check(_toward_zero(v32).astype(np.float32), *args)
    print(f"toward zero: bad {trunc['bad']:.4f} of all, {trunc['bad'] / (v32 > 0).mean():.4f} of the non-zero outputs")
    assert trunc["bad"] / (v32 > 0).mean() >= 0.3

    half = f16_layer_check(_accumulate(x, w, b, np.float16).astype(np.float32), *args)
    print(f"f16 accumulation: bad {half['bad']:.4f} acc_ratio {half['acc_ratio']:.3e}")
    assert half["bad"] >= 0.3 and half["acc_ratio"] > 2e-6


def test_f16_checker_overflow_and_subnormals():
    """+-inf past 65504 and gradual underflow are what the reference expects; a flushed subnormal fails."""
    x = np.array([1.0, 3.0, 2.0 ** -10], np.float32).reshape(1, 3, 1, 1)
    w = np.array([[60000.0, 4000.0, 0.0], [-60000.0, -4000.0, 0.0], [0.0, 0.0, 2.0 ** -8]], np.float32).reshape(3, 3, 1, 1)
    args = (x, w, None, [0, 0, 0, 0], (1, 1), False)
    want = np.array([np.inf, -np.inf, 2.0 ** -18], np.float32).reshape(1, 3, 1, 1)
    assert f16_layer_check(want, *args)["ok"].all()
    flushed = want.copy()
    flushed[0, 2] = 0.0
    assert f16_layer_check(flushed, *args)["ok"].reshape(-1).tolist() == [True, True, False]
    clamped = want.copy()
    clamped[0, 0] = 65504.0
    assert f16_layer_check(clamped, *args)["ok"].reshape(-1).tolist() == [False, True, True]


def test_f16_layer_bounds_contain_the_exact_input_case():
    """A point interval gives f16_layer_check's own [lo, hi]; widening the input by an f16 ulp either way only
    widens the output interval, and it still holds the output of any input inside."""
    x, w, b = _layer()
    xh = x.astype(np.float16)
    args = (w, b, [1, 1, 1, 1], (1, 1), True)
    good = f16_layer_check(_accumulate(x, w, b, np.float32).astype(np.float16).astype(np.float32), x, *args)
    lo, hi = f16_layer_bounds(xh, xh, *args)
    assert np.array_equal(lo, good["lo"]) and np.array_equal(hi, good["hi"])
    xlo, xhi = np.nextafter(xh, np.float16(-np.inf)), np.nextafter(xh, np.float16(np.inf))
    wlo, whi = f16_layer_bounds(xlo, xhi, *args)
    assert (wlo <= lo).all() and (hi <= whi).all() and (wlo < lo).any() and (hi < whi).any()
    inside = np.where(np.random.default_rng(3).random(x.shape) < 0.5, xlo, xhi)
    got = _accumulate(inside.astype(np.float32), w, b, np.float32).astype(np.float16)
    assert ((wlo <= got) & (got <= whi)).all()
