"""Poisoned surroundings for the per-op slice tests (tests/test_slices_gpu.py; the detector's own test is
tests/test_slices.py, on numpy arrays).

A tensor handed to the C ABI is `data`, `dims` and `nstride`: element (n, c, h, w) of an [N, C, H, W] tensor
lies at data + n * nstride + (c * H + h) * W + w, and nothing else of the memory around it is the op's.  The
helper here lays a logical array out inside ONE buffer --

    lead | image 0 | gap | image 1 | gap | ... | image N-1 | tail (>= 64 elements)

where an image is the tensor's own C * H * W elements or, for a channel slice, channels [c0, c0 + C) of a
parent image of Ctot channels -- and fills every element that is not the tensor's with a poison:

  inputs   NAN_POISON for arithmetic ops (Conv, MatMul, the elementwise ops): a poisoned element that reaches a
           multiply or an add makes the output NaN, also under a zero weight or a 0 / 1 mask; INF_POISON for
           MaxPool, whose fmaxf drops a NaN but never a +inf.
  outputs  OUT_POISON_BITS, one NaN bit pattern written through an int32 view over the WHOLE buffer, the
           tensor's own elements included: afterwards every element outside must still hold those bits
           (check_surroundings, compared as int32) and every element inside must be a computed value
           (check_no_poison + the caller's comparison with its reference).

Placed is numpy only.  device_place / upload / download / descriptor put one on the GPU and build the
ore_tensor through ctypes, with the tensor's base at a chosen offset inside a 4 KiB page (torch allocations are
256-byte aligned, so a misaligned or mid-page base has to be made)."""
import ctypes
from typing import NamedTuple, Optional, Tuple

import numpy as np

OUT_POISON_BITS = np.int32(0x7FC5A5A5)                                  # a quiet NaN no kernel computes
NAN_POISON = np.array([0x7FC0BAD0], np.int32).view(np.float32)[0]      # input poison: a quiet NaN
INF_POISON = np.float32(np.inf)                                          # input poison for MaxPool
TAIL_MIN = 64
PAGE = 4096
PAGE_OFF = 256  # bytes into its 4 KiB page at which device_place puts the buffer's first image


class Layout(NamedTuple):
    """lead: poisoned elements in front of the first (parent) image, at least; gap: nstride minus the (parent)
    image size; chan: (c0, after) -- the tensor is channels [c0, c0 + C) of a parent with Ctot = c0 + C + after
    channels; misalign: floats by which device_place shifts the first image off its 16-byte aligned base."""
    name: str
    lead: int = 0
    gap: int = 0
    chan: Optional[Tuple[int, int]] = None
    misalign: int = 0

    def __str__(self):
        return self.name


# S = the dense image size; `dense` is the control (today's call, with poison before and after)
DENSE = Layout("dense")
GAP4 = Layout("gap4", lead=8, gap=8)                       # nstride = S + 8, base 16-byte aligned
GAP_ODD = Layout("gap_odd", lead=8, gap=3)                 # nstride = S + 3
OFF1 = Layout("off1", lead=8, misalign=1)                  # base 4-byte but not 16-byte aligned, nstride = S
CHAN_A = Layout("chan_a", lead=8, chan=(4, 3))             # c0 * plane % 4 == 0 whatever the plane
CHAN_B = Layout("chan_b", lead=8, chan=(1, 2))             # c0 * plane % 4 == plane % 4: != 0 on odd planes
LAYOUTS = [DENSE, GAP4, GAP_ODD, OFF1, CHAN_A, CHAN_B]


class Placed:
    """A logical array of `shape` (1 to 4 dims; dims[0] steps by nstride, the rest is dense) inside a flat
    buffer of `total` elements.  index[...] is the flat position of every element of the tensor."""

    def __init__(self, shape, lead=0, nstride=None, chan=None, total=None):
        self.shape = tuple(int(s) for s in shape)
        n = self.shape[0]
        self.image = int(np.prod(self.shape[1:], dtype=np.int64))
        if chan is not None:
            assert len(self.shape) == 4, "a channel slice is of a 4-D tensor"
            c0, ctot = chan
            plane = self.shape[2] * self.shape[3]
            assert c0 >= 0 and c0 + self.shape[1] <= ctot
            self.parent_image = ctot * plane
            self.chan_off = c0 * plane
        else:
            self.parent_image = self.image
            self.chan_off = 0
        self.chan = chan
        self.lead = int(lead)
        self.nstride = self.parent_image if nstride is None else int(nstride)
        assert self.nstride >= self.parent_image, "images would overlap"
        self.base = self.lead + self.chan_off  # flat position of element [0, 0, ...]
        extent = (n - 1) * self.nstride + self.parent_image if n else 0
        self.total = self.lead + extent + TAIL_MIN if total is None else int(total)
        assert self.total >= self.lead + extent + TAIL_MIN, "the tail is at least TAIL_MIN elements"
        self.extent = extent
        inner = np.arange(self.image, dtype=np.int64).reshape(self.shape[1:] or (1,))
        idx = self.base + np.arange(n, dtype=np.int64).reshape((n,) + (1,) * inner.ndim) * self.nstride + inner[None]
        self.index = idx.reshape(self.shape)

    @classmethod
    def of(cls, shape, layout, extra_lead=0, total=None):
        shape = tuple(int(s) for s in shape)
        chan = None
        if layout.chan is not None:
            chan = (layout.chan[0], layout.chan[0] + shape[1] + layout.chan[1])
        probe = cls(shape, 0, None, chan)
        return cls(shape, layout.lead + extra_lead, probe.parent_image + layout.gap, chan, total)

    # ---- buffers
    def input_buffer(self, arr, poison):
        """float32 [total]: arr at the tensor's positions, `poison` everywhere else."""
        arr = np.asarray(arr, np.float32)
        assert arr.shape == self.shape, (arr.shape, self.shape)
        buf = np.full(self.total, poison, np.float32)
        buf[self.index] = arr
        return buf

    def output_buffer(self):
        """int32 [total], every element OUT_POISON_BITS (view it as float32 for the op)."""
        return np.full(self.total, OUT_POISON_BITS, np.int32)

    def inside(self, buf):
        """The tensor's elements of a [total] buffer, as float32 of the tensor's shape."""
        return np.asarray(buf).view(np.float32)[self.index]

    def outside_mask(self):
        m = np.ones(self.total, bool)
        m[self.index] = False
        return m

    def region(self, i):
        """Where flat position i lies: 'lead', 'tail', 'gap' (between two images), 'channel' (another channel of the
        parent image) or 'inside'."""
        if i < self.lead:
            return "lead"
        if i >= self.lead + self.extent:
            return "tail"
        n, r = divmod(i - self.lead, self.nstride)
        if r >= self.parent_image:
            return "gap"
        if r < self.chan_off or r >= self.chan_off + self.image:
            return "channel"
        return "inside"


def _bits(buf):
    buf = np.asarray(buf)
    assert buf.dtype in (np.int32, np.float32), buf.dtype
    return buf.view(np.int32)


def check_surroundings(placed, buf_after):
    """Surroundings untouched: every element of the output buffer outside the tensor still holds
    OUT_POISON_BITS, compared as int32 (a NaN never equals itself as a float)."""
    bits = _bits(buf_after)
    assert bits.shape == (placed.total,), (bits.shape, placed.total)
    bad = np.flatnonzero((bits != OUT_POISON_BITS) & placed.outside_mask())
    if bad.size:
        where = ", ".join(f"{int(i)} ({placed.region(int(i))}, base{int(i) - placed.base:+d}) = 0x{int(bits[i]) & 0xffffffff:08x}"
                          for i in bad[:8])
        raise AssertionError(f"{bad.size} element(s) outside the tensor were written: {where}")


def check_no_poison(result, poison):
    """No poison in the result: no NaN where the inputs' surroundings were NaN (also catches an output element
    the op never wrote: it still holds the output poison, a NaN), no +inf where they were +inf."""
    r = np.asarray(result, np.float32)
    bad = np.isnan(r) if np.isnan(poison) else (np.isnan(r) | (r == poison))
    if bad.any():
        first = [tuple(int(v) for v in ix) for ix in np.argwhere(bad)[:8]]
        raise AssertionError(f"{int(bad.sum())} of {r.size} outputs hold poison (an element outside the input was read, "
                             f"or the output was not written); first at {first}")


# ---------------------------------------------------------------------------------------------- device side
def device_place(shape, layout, page_off=PAGE_OFF):
    """-> (Placed, buf): a float32 CUDA buffer and the layout of `shape` in it, the first (parent) image
    page_off + 4 * layout.misalign bytes into a 4 KiB page.  At least layout.lead elements and at least page_off
    bytes of the buffer lie in front of it: what a kernel reads of its page before the tensor is poison too."""
    import torch
    slack = 2 * PAGE // 4
    probe = Placed.of(shape, layout)
    buf = torch.empty(probe.total + slack, dtype=torch.float32, device="cuda")
    want = page_off + 4 * layout.misalign
    adj = ((want - (buf.data_ptr() + 4 * layout.lead)) % PAGE) // 4
    if 4 * (layout.lead + adj) < page_off:
        adj += PAGE // 4
    placed = Placed.of(shape, layout, extra_lead=adj, total=probe.total + slack)
    assert (buf.data_ptr() + 4 * placed.lead) % PAGE == want
    return placed, buf


def upload(buf, host):
    """host: float32 or int32 [total]; copied bit for bit."""
    import torch
    host = np.ascontiguousarray(host)
    if host.dtype == np.int32:
        buf.view(torch.int32).copy_(torch.from_numpy(host))
    else:
        buf.copy_(torch.from_numpy(host.astype(np.float32, copy=False)))


def poison_output(buf):
    import torch
    buf.view(torch.int32).fill_(int(OUT_POISON_BITS))


def download(buf):
    """The whole buffer as int32 bits (view as float32 through Placed.inside)."""
    import torch
    torch.cuda.synchronize()
    return buf.view(torch.int32).cpu().numpy()


def descriptor(placed, buf, nstride=None):
    """ore_tensor of the placed tensor: data at its element [0, 0, ...], its dims and its nstride."""
    from ore import _lib
    t = _lib.Tensor()
    t.data = buf.data_ptr() + 4 * placed.base
    t.ndim = len(placed.shape)
    for i, s in enumerate(placed.shape):
        t.dims[i] = s
    t.nstride = placed.nstride if nstride is None else nstride
    return t


def dense_descriptor(t):
    """ore_tensor of a contiguous float32 CUDA tensor (weights, bias)."""
    from ore import _lib
    d = _lib.Tensor()
    d.data = t.data_ptr()
    d.ndim = t.dim()
    for i, s in enumerate(t.shape):
        d.dims[i] = int(s)
    d.nstride = 0
    return d


def ref(d):
    return ctypes.byref(d)
