"""The poison detector's own test (tests/_slices.py), on numpy arrays: no GPU.

Two numpy models of kernels run over a flat buffer the way a HIP kernel runs over device memory -- by flat
offsets from the tensor's base, never through the logical array -- in a correct form and in the forms the
detector exists for:
  * a 3-tap 'same' row filter whose out-of-row taps are SELECTED away (ok ? v : 0), against the form that
    multiplies them by a 0 / 1 mask (v * ok): with finite neighbours both give the same numbers, with a NaN
    next to the row the second gives NaN;
  * a row max whose out-of-row taps are selected away, against the form that reads them unmasked (+inf wins);
  * an epilogue that stores the tensor's elements, against forms whose bound is one too wide: one element into
    the gap behind an image, the lead in front of the tensor, the tail behind it, the neighbouring channel.
Every wrong form must be flagged and every correct one must pass, on every layout the GPU tests use."""
import numpy as np
import pytest

import _slices as sl
from _slices import Layout, Placed

SHAPE = (3, 5, 4, 6)
LAYOUTS = sl.LAYOUTS + [Layout("lead_only", lead=5), Layout("chan_gap", lead=3, gap=5, chan=(2, 1))]


def _x(shape=SHAPE, seed=0):
    return (np.random.default_rng(seed).standard_normal(shape) - 2.0).astype(np.float32)


def _flat_taps(placed, buf):
    """Per element of the tensor: the buffer's values at flat offsets -1, 0, +1 from it (clamped into the buffer,
    as a masked lane's load is clamped into the allocation) and whether each tap lies inside the element's row."""
    W = placed.shape[-1]
    w = np.arange(W).reshape((1,) * (len(placed.shape) - 1) + (W,))
    taps = []
    for d in (-1, 0, 1):
        ok = np.broadcast_to((w + d >= 0) & (w + d < W), placed.shape)
        v = buf[np.clip(placed.index + d, 0, placed.total - 1)]
        taps.append((v, ok))
    return taps


def filter_select(placed, buf):
    """y = x[w-1] + 2 x[w] + x[w+1] with zero padding: masked taps are selected away."""
    (l, lok), (c, _), (r, rok) = _flat_taps(placed, buf)
    return np.where(lok, l, np.float32(0)) + np.float32(2) * c + np.where(rok, r, np.float32(0))


def filter_multiply(placed, buf):
    """The same filter with the mask as a factor: 0 * NaN is NaN."""
    (l, lok), (c, _), (r, rok) = _flat_taps(placed, buf)
    with np.errstate(invalid="ignore"):
        return l * lok.astype(np.float32) + np.float32(2) * c + r * rok.astype(np.float32)


def rowmax_select(placed, buf):
    """y = max(x[w-1], x[w], x[w+1], 0 where a tap is padding), fmaxf-style (NaN dropped)."""
    (l, lok), (c, _), (r, rok) = _flat_taps(placed, buf)
    return np.fmax(np.fmax(np.where(lok, l, np.float32(0)), c), np.where(rok, r, np.float32(0)))


def rowmax_unmasked(placed, buf):
    (l, _), (c, _), (r, _) = _flat_taps(placed, buf)
    return np.fmax(np.fmax(l, c), r)


def store(placed, out_bits, y, extra=()):
    """The epilogue: y to the tensor's elements, plus one stray element at each flat position of `extra`."""
    out = out_bits.view(np.float32)
    out[placed.index] = y
    for i in extra:
        out[i] = np.float32(1.5)


def _ref_filter(x):
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(1, 1)])
    return xp[..., :-2] + np.float32(2) * xp[..., 1:-1] + xp[..., 2:]


def _ref_rowmax(x):
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(1, 1)])
    return np.maximum(np.maximum(xp[..., :-2], xp[..., 1:-1]), xp[..., 2:])


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_layout_geometry(layout):
    """Every element of the tensor has its own flat position at base + n * nstride + the dense inner offset; lead,
    gaps, tail and the parent's other channels are all outside and named correctly."""
    p = Placed.of(SHAPE, layout)
    N, C, H, W = SHAPE
    assert np.unique(p.index).size == p.index.size
    for n, c, h, w in ((0, 0, 0, 0), (1, 2, 3, 4), (N - 1, C - 1, H - 1, W - 1)):
        assert p.index[n, c, h, w] == p.base + n * p.nstride + (c * H + h) * W + w
    ctot = C if layout.chan is None else layout.chan[0] + C + layout.chan[1]
    assert p.nstride == ctot * H * W + layout.gap and p.lead == layout.lead
    assert p.total - p.index.max() - 1 >= sl.TAIL_MIN
    mask = p.outside_mask()
    assert mask.sum() == p.total - p.index.size
    regions = {p.region(int(i)) for i in np.flatnonzero(mask)}
    want = {"tail"} | ({"lead"} if layout.lead else set()) | ({"gap"} if layout.gap else set()) | \
        ({"channel"} if layout.chan else set())
    assert regions == want
    assert {p.region(int(i)) for i in p.index.ravel()} == {"inside"}
    # the input buffer: data inside, poison everywhere else, bit for bit
    x = _x()
    buf = p.input_buffer(x, sl.NAN_POISON)
    np.testing.assert_array_equal(p.inside(buf), x)
    assert np.isnan(buf[mask]).all() and not np.isnan(buf[~mask]).any()
    out = p.output_buffer()
    assert (out == sl.OUT_POISON_BITS).all() and np.isnan(out.view(np.float32)).all()


def test_layout_rejects_overlap_and_short_tail():
    with pytest.raises(AssertionError):
        Placed(SHAPE, 0, nstride=5 * 4 * 6 - 1)
    with pytest.raises(AssertionError):
        Placed(SHAPE, 0, total=3 * 5 * 4 * 6 + sl.TAIL_MIN - 1)


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_correct_ops_pass(layout):
    p = Placed.of(SHAPE, layout)
    x = _x()
    for op, ref, poison in ((filter_select, _ref_filter, sl.NAN_POISON), (rowmax_select, _ref_rowmax, sl.INF_POISON)):
        out = p.output_buffer()
        store(p, out, op(p, p.input_buffer(x, poison)))
        sl.check_surroundings(p, out)
        got = p.inside(out)
        sl.check_no_poison(got, poison)
        np.testing.assert_array_equal(got, ref(x))


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_poisoned_read_is_flagged(layout):
    """A masked tap that is multiplied by zero, and a pool tap that is not masked at all, read the element in front
    of the tensor's first row or behind its last: lead, gap, tail or a neighbouring channel, poison in each."""
    p = Placed.of(SHAPE, layout)
    x = _x()
    got = filter_multiply(p, p.input_buffer(x, sl.NAN_POISON))
    with pytest.raises(AssertionError, match="hold poison"):
        sl.check_no_poison(got, sl.NAN_POISON)
    # finite surroundings hide exactly this: over finite garbage the same op gives the right numbers
    np.testing.assert_array_equal(filter_multiply(p, p.input_buffer(x, np.float32(7.0))), _ref_filter(x))
    got = rowmax_unmasked(p, p.input_buffer(x, sl.INF_POISON))
    with pytest.raises(AssertionError, match="hold poison"):
        sl.check_no_poison(got, sl.INF_POISON)
    # ... and a NaN poison would not show it: fmaxf drops the NaN
    sl.check_no_poison(rowmax_unmasked(p, p.input_buffer(x, sl.NAN_POISON)), sl.NAN_POISON)


def test_single_poisoned_read_is_flagged():
    """One tap of one output reading one poisoned element is enough."""
    p = Placed.of(SHAPE, sl.GAP_ODD)
    x = _x()
    buf = p.input_buffer(x, sl.NAN_POISON)
    y = filter_select(p, buf)
    sl.check_no_poison(y, sl.NAN_POISON)
    y[1, 0, 0, 0] += np.float32(0) * buf[p.index[1, 0, 0, 0] - 1]  # the gap in front of image 1, under a zero weight
    with pytest.raises(AssertionError, match=r"1 of 360 outputs.*\(1, 0, 0, 0\)"):
        sl.check_no_poison(y, sl.NAN_POISON)


def _stray_positions(p):
    """One flat position per kind of surroundings the layout has: an epilogue bound one too wide lands there."""
    N, C, H, W = p.shape
    pos = {"tail": int(p.index[N - 1, C - 1, H - 1, W - 1]) + 1 if p.chan is None else p.lead + p.extent}
    if p.lead:
        pos["lead"] = p.lead - 1 if p.chan is None else p.base - p.chan_off - 1
    if p.nstride > p.parent_image:
        pos["gap"] = p.lead + p.parent_image  # one past the first (parent) image
    if p.chan is not None:
        pos["channel"] = int(p.index[0, C - 1, H - 1, W - 1]) + 1  # the first element of channel c0 + C
        pos["channel_before"] = p.base - 1
    return pos


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_stray_write_is_flagged(layout):
    p = Placed.of(SHAPE, layout)
    x = _x()
    y = filter_select(p, p.input_buffer(x, sl.NAN_POISON))
    strays = _stray_positions(p)
    assert set(strays) >= {"tail"} | ({"lead"} if layout.lead else set()) | ({"gap"} if layout.gap else set()) | \
        ({"channel"} if layout.chan else set())
    for kind, i in strays.items():
        assert p.region(i) == kind.split("_")[0], (kind, i, p.region(i))
        out = p.output_buffer()
        store(p, out, y, extra=[i])
        with pytest.raises(AssertionError, match=rf"1 element\(s\) outside the tensor were written: {i} \({p.region(i)}"):
            sl.check_surroundings(p, out)
        # the parity check alone does not see it
        np.testing.assert_array_equal(p.inside(out), _ref_filter(x))


def test_stray_write_of_the_poison_value_as_a_float_is_flagged():
    """A stray store of a NaN with other bits than the poison's is a write: the comparison is on the bits."""
    p = Placed.of(SHAPE, sl.GAP4)
    out = p.output_buffer()
    out.view(np.float32)[p.lead + p.parent_image] = np.float32(np.nan)
    with pytest.raises(AssertionError, match="gap"):
        sl.check_surroundings(p, out)


def test_unwritten_output_is_flagged():
    """An epilogue whose bound is one too NARROW leaves the output poison inside the tensor."""
    p = Placed.of(SHAPE, sl.DENSE)
    x = _x()
    out = p.output_buffer()
    store(p, out, filter_select(p, p.input_buffer(x, sl.NAN_POISON)))
    out[p.index[2, 4, 3, 5]] = sl.OUT_POISON_BITS
    sl.check_surroundings(p, out)
    for poison in (sl.NAN_POISON, sl.INF_POISON):
        with pytest.raises(AssertionError, match=r"\(2, 4, 3, 5\)"):
            sl.check_no_poison(p.inside(out), poison)


def test_2d_contiguous_placement():
    """MatMul's and the elementwise ops' operands: contiguous, only base and surroundings vary."""
    p = Placed.of((37, 10), sl.OFF1)
    assert p.nstride == 10 and p.base == p.lead == 8 and p.index[36, 9] == 8 + 369
    a = _x((37, 10))
    np.testing.assert_array_equal(p.inside(p.input_buffer(a, sl.NAN_POISON)), a)
    with pytest.raises(AssertionError):
        Placed.of((37, 10), sl.CHAN_A)
