"""Poisoned library memory (no GPU needed to import): the patterns and helpers of
tests/test_scratch_poison_gpu.py.

The library never initialises the device memory it allocates for itself, and its kernels read parts of it by
design (padded channel planes, the 256-B tails of the arena slots, the arena's lead, the slots of the images
a smaller run does not use, what an earlier value left in a reused slot).  With ordinary finite junk there, a
pad element that reaches a multiply under a zero weight, a 0 / 1 mask or a max changes nothing (tests/_slices.py
makes the same point for the per-op slices).  So the junk is chosen: NAN survives every multiply and add, BIG
wins every max (which drops a NaN).

A model is loaded on a context with ore_ctx_set_alloc_fill on, its activation memory is filled again
(ore_model_fill_scratch) before every run, and the caller's output tensor starts as the pattern too; the
result must hold no pattern word and equal a reference that never saw the poisoned code."""
import ctypes

import numpy as np

NAN = 0x7FC07FC0  # a quiet NaN as f32 and in both f16 halves
BIG = {"f32": 0x7F800000, "f16": 0x7C007C00}  # +inf as f32; +inf in both f16 halves (2.66e36 as f32)


def patterns(precision):
    """[(name, 32-bit word)] every case runs under: NaN, and the +inf of the model's activation type"""
    return [("nan", NAN), ("big", BIG[precision])]


def make_ctx():
    """an ore.Context on a torch stream of its own (alloc fill is per context): (ctx, stream)"""
    import torch
    import ore
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    return ctx, s


def filled(shape, pattern, dtype=None):
    """a CUDA tensor of `shape` (float32, or int32 with dtype) whose every 32-bit word is the pattern"""
    import torch
    t = torch.full(tuple(shape), int(np.uint32(pattern).view(np.int32)), dtype=torch.int32, device="cuda")
    return t if dtype is torch.int32 else t.view(torch.float32)


def words(a):
    """the 32-bit words of a float32 / int32 / uint32 array"""
    return np.ascontiguousarray(a).view(np.uint32)


def count_words(a, pattern):
    return int((words(a) == np.uint32(pattern)).sum())


def download(ctx, ptr, nbytes):
    """`nbytes` of device memory at ptr as uint32 words (ore_download; a tail of nbytes % 4 is dropped)"""
    from ore import _lib
    n = nbytes // 4
    host = np.empty(n, np.uint32)
    _lib.check(_lib.load().ore_download(ctx.h, host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), n * 4), ctx.h)
    return host


def poisoned_run(m, stream, x, pattern, entry="run_into", out=None):
    """fill_scratch(pattern), then m.<entry>(x, out) into an output that starts as the pattern: the output as
    numpy.  The context has a stream of its own: torch's work is joined before, the stream after."""
    import pytest
    import torch
    import ore
    try:
        if out is None:
            out = filled((x.shape[0], m.output_elems), pattern)
        torch.cuda.synchronize()
        m.fill_scratch(pattern)
        getattr(m, entry)(x, out)
        stream.synchronize()
        return out.cpu().numpy()
    except (RuntimeError, ore.OreError) as err:  # a device error: nothing more runs on a GPU that has faulted
        if isinstance(err, ore.OreError) and err.status != 3:
            raise
        pytest.exit(f"device error, stopping: {err}", returncode=3)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(words(a), words(b))
