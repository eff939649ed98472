"""Float64 reference helpers for the conv parity tests (no GPU): a direct convolution with the
per-output magnitude sum |w x| that the f32 tolerance 2e-6 * sum|w x| is written against, the per-output
check of one fp16 conv layer against its contract (f16_layer_check, f16_layer_bounds), and a one-Conv ONNX
model builder."""
import numpy as np


def conv_f64(x, w, b, pads, strides):
    """Direct convolution in float64 (zero padding, pads t, l, b, r) and sum |w x| per output."""
    x = x.astype(np.float64)
    w = w.astype(np.float64)
    N, C, H, W = x.shape
    M, _, kh, kw = w.shape
    pt, pl, pb, pr = pads
    sh, sw = strides
    xp = np.zeros((N, C, H + pt + pb, W + pl + pr))
    xp[:, :, pt:pt + H, pl:pl + W] = x
    Ho = (H + pt + pb - kh) // sh + 1
    Wo = (W + pl + pr - kw) // sw + 1
    cols = np.empty((N, C, kh, kw, Ho, Wo))
    for r in range(kh):
        for s in range(kw):
            cols[:, :, r, s] = xp[:, :, r:r + sh * (Ho - 1) + 1:sh, s:s + sw * (Wo - 1) + 1:sw]
    cols = cols.reshape(N, C * kh * kw, Ho * Wo)
    wm = w.reshape(M, -1)
    y = np.einsum("mk,nkp->nmp", wm, cols).reshape(N, M, Ho, Wo)
    mag = np.einsum("mk,nkp->nmp", np.abs(wm), np.abs(cols)).reshape(N, M, Ho, Wo)
    if b is not None:
        y += b.astype(np.float64)[None, :, None, None]
        mag += np.abs(b.astype(np.float64))[None, :, None, None]
    return y, mag


F16_ACC_TOL = 2e-6        # f32 accumulation error allowed, as a fraction of sum |w x| + |b| (test_ops_gpu.py's)
F16_AMBIGUOUS_CAP = 1 / 3  # largest share of outputs a case may leave with two admissible f16 values


def _f16(a):
    with np.errstate(over="ignore"):  # past 65504: +-inf, the cast the kernels do
        return np.asarray(a).astype(np.float16)


def f16_layer_check(got, x, w, b, pads, strides, relu):
    """One fp16 conv layer against its contract
        y = RNE_f16(relu?(sum_k f16(x_k) f16(w_k) [f32 accumulate] + b_f32)):
    products of two f16 values are exact in f32, so with S the float64 value of the sum over the f16
    operands and e = F16_ACC_TOL * mag (mag = sum |w x| + |b|), `got` must lie in
    [f16(relu?(S - e)), f16(relu?(S + e))] -- RNE is monotone, so that is "the correctly rounded f16 of
    some value within e of S"; where the two ends agree (most outputs) it is one f16 value, bit for bit.

    got: the layer's output, [N, M, Ho, Wo], every value an f16.  Returns a dict:
      ok         bool array, got within [lo, hi]
      bad        share of outputs outside
      ambiguous  share of outputs with lo != hi (depends on the reference alone)
      acc_ratio  over the outputs where got != f16(relu?(S)): the largest distance from S to the
                 rounding boundary got lies behind, / mag -- a lower bound on the accumulation error
                 of whatever produced got (0.0 when every output is the nearest f16)
      ref, lo, hi  f16(relu?(S)), f16(relu?(S - e)), f16(relu?(S + e))"""
    got = np.asarray(got)
    gh = _f16(got)
    assert np.array_equal(gh.astype(np.float64), got.astype(np.float64), equal_nan=True), "got holds non-f16 values"
    S, mag = conv_f64(_f16(x), _f16(w), b, pads, strides)
    assert S.shape == got.shape, (S.shape, got.shape)
    act = (lambda v: np.maximum(v, 0.0)) if relu else (lambda v: v)
    e = F16_ACC_TOL * mag
    lo, hi, ref = _f16(act(S - e)), _f16(act(S + e)), _f16(act(S))
    ok = (lo <= gh) & (gh <= hi)  # NaN fails both
    # the boundary between got and the f16 next to it on S's side: v rounds to got only from beyond it
    g64 = np.clip(gh.astype(np.float64), -65536.0, 65536.0)  # +-inf: as the f16 after 65504, boundary 65520
    with np.errstate(over="ignore", invalid="ignore"):
        toward = np.where(gh > ref, -np.inf, np.inf).astype(np.float16)
        nb = np.clip(np.nextafter(gh, toward).astype(np.float64), -65536.0, 65536.0)
    off = (gh != ref) & ~np.isnan(gh)
    dist = np.abs(0.5 * (g64 + nb) - act(S))
    ratio = np.where(off & (mag > 0), dist / np.where(mag > 0, mag, 1.0), 0.0)
    return {"ok": ok, "bad": float(1.0 - ok.mean()), "ambiguous": float((lo != hi).mean()),
            "acc_ratio": float(ratio.max()) if ratio.size else 0.0, "ref": ref, "lo": lo, "hi": hi}


def f16_layer_bounds(xlo, xhi, w, b, pads, strides, relu):
    """f16_layer_check's [lo, hi] for a layer whose input is only known elementwise within [xlo, xhi] (f16
    values; equal: exactly its lo / hi): the interval of S by the signs of the weights, e from the larger
    |x|.  Pushes one layer's admissible outputs through the next."""
    xlo, xhi, wh = (_f16(a).astype(np.float64) for a in (xlo, xhi, w))
    wpos, wneg = np.maximum(wh, 0.0), np.minimum(wh, 0.0)
    s_lo = conv_f64(xlo, wpos, b, pads, strides)[0] + conv_f64(xhi, wneg, None, pads, strides)[0]
    s_hi = conv_f64(xhi, wpos, b, pads, strides)[0] + conv_f64(xlo, wneg, None, pads, strides)[0]
    e = F16_ACC_TOL * conv_f64(np.maximum(np.abs(xlo), np.abs(xhi)), wh, b, pads, strides)[1]
    act = (lambda v: np.maximum(v, 0.0)) if relu else (lambda v: v)
    return _f16(act(s_lo - e)), _f16(act(s_hi + e))


def _conv_model(x_shape, w, b, pads, strides):
    from ore import onnx_wire as wr
    ins = ["x", "w"] + (["b"] if b is not None else [])
    nodes = [wr.encode_node("Conv", ins, ["y"], attrs=[wr.encode_attr_ints("pads", pads),
                                                       wr.encode_attr_ints("strides", strides)])]
    inits = [wr.encode_tensor("w", w)] + ([wr.encode_tensor("b", b)] if b is not None else [])
    vinfo = [wr.encode_value_info("x", x_shape), wr.encode_value_info("w", w.shape)]
    if b is not None:
        vinfo.append(wr.encode_value_info("b", b.shape))
    return wr.encode_model("c", nodes, inits, vinfo, [wr.encode_value_info("y", (1, 1, 1, 1))])
