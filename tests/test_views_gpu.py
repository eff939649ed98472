"""GPU: several views of one subject -- mirrored list images (ore_image_list_set_ex / _set_nv12_ex), the
view-mean top-k (ore_topk_mean_f32) and the model's views (ore_model_set_views).

Both pieces are specified to the bit.  A flipped image is the unflipped one with its columns reversed; the
mean of a group is the float32 sum of its rows in ascending order divided by float32(views), every operation
rounded on its own, and the selection is ore_topk_f32's order over it.  So every comparison here is exact,
values as uint32 (a NaN mean compares by NaN-ness: its payload is unspecified)."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

from _nv12_ref import NAMES
from _resize_aa_ref import resize_aa_ref
from _resize_ref import images, resize_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

GROUPS = (1, 3, 5)  # a block not full of groups (4 per block), more than one block
VIEWS = (1, 2, 3, 10, 64)
DS = (1, 63, 64, 65, 256, 257, 1000, 1024, 1025, 4100)  # both register kernels, their bounds, the long-row kernel
KINDS = ("normal", "softmax", "ties", "zeros", "subnormals", "specials")

_MEAN = np.array([0.485, 0.456, 0.406, 0.5], np.float32)
_STD = np.array([0.229, 0.224, 0.225, 0.25], np.float32)


def _norm(c):
    return ((np.float32(1.0) / (np.float32(255.0) * _STD[:c])).astype(np.float32), (-_MEAN[:c] / _STD[:c]).astype(np.float32))


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------ topk_mean
def _mean_ref(x, views):
    """The definition: acc = row 0; acc = acc + row v for v ascending; m = acc / float32(views), in float32."""
    xv = x.reshape(x.shape[0] // views, views, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = xv[:, 0].copy()
        for v in range(1, views):
            acc = acc + xv[:, v]
        m = acc / np.float32(views)
    assert m.dtype == np.float32
    return m


def _topk_ref(m, k):
    with np.errstate(invalid="ignore"):
        idx = np.argsort(-m, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(m, idx, 1), idx.astype(np.int32)


def _nan(rng, shape):
    """NaNs of both signs with random payloads."""
    bits = (rng.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31)) | np.uint32(0x7f800000) | \
        rng.integers(1, 1 << 23, shape, dtype=np.uint32)
    return bits.view(np.float32)


def _input(kind, rows, D, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((rows, D)).astype(np.float32)
    if kind == "softmax":
        e = np.exp(rng.standard_normal((rows, D)).astype(np.float32))
        return (e / e.sum(1, keepdims=True)).astype(np.float32)
    if kind == "ties":  # small integers: the sums are exact and mostly tie, the index rule decides
        return rng.integers(0, 4, (rows, D)).astype(np.float32)
    if kind == "zeros":  # the mean of -0.0s alone is -0.0, one +0.0 among them makes it +0.0; all tie
        x = np.where(rng.random((rows, D)) < 0.35, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        x[:, rng.random(D) < 0.05] = -1.0
        return x
    if kind == "subnormals":  # 1e-44 .. 1e-38: neither the sum nor the division may flush
        x = (10.0 ** rng.uniform(-44.0, -38.0, (rows, D))).astype(np.float32)
        assert x.max() < np.finfo(np.float32).tiny and x.min() > 0
        return x
    assert kind == "specials"  # NaN of both signs, +inf and -inf sprinkled in: inf - inf and NaN make NaN means
    x = rng.standard_normal((rows, D)).astype(np.float32)
    m = rng.random((rows, D))
    x = np.where(m < 0.01, _nan(rng, (rows, D)), x)
    x[(m >= 0.01) & (m < 0.03)] = np.inf
    x[(m >= 0.03) & (m < 0.05)] = -np.inf
    return x


def _assert_topk(v, i, want_v, want_i, msg=""):
    """indices exactly; values bit for bit where the mean is a number, by NaN-ness where it is NaN"""
    np.testing.assert_array_equal(i, want_i, err_msg=msg)
    nan = np.isnan(want_v)
    np.testing.assert_array_equal(np.isnan(v), nan, err_msg=msg)
    np.testing.assert_array_equal(_u32(v)[~nan], _u32(want_v)[~nan], err_msg=msg)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DS)
def test_topk_mean_matches_numpy(gpu_ctx, D, kind):
    import ore
    x = _input(kind, max(GROUPS) * max(VIEWS), D, seed=1000 * KINDS.index(kind) + D)
    kmax = min(D, 64)
    xd = _cuda(x)
    for views in VIEWS:
        m = _mean_ref(x[:max(GROUPS) * views], views)  # once for all groups and k: prefixes of it
        if kind == "zeros" and views in (2, 3) and D >= 256:
            assert np.signbit(m[m == 0]).any() and not np.signbit(m[m == 0]).all()  # both signs of a zero mean occur
        if kind == "subnormals":
            assert (m < np.finfo(np.float32).tiny).any() and (m > 0).all()
        want_v, want_i = _topk_ref(m, kmax)
        for groups in GROUPS:
            for k in sorted({1, min(5, D), kmax}):
                v, i = ore.topk_mean(gpu_ctx, xd[:groups * views], views, k)
                assert tuple(v.shape) == tuple(i.shape) == (groups, k)
                assert str(v.dtype) == "torch.float32" and str(i.dtype) == "torch.int32"
                _assert_topk(v.cpu().numpy(), i.cpu().numpy(), want_v[:groups, :k], want_i[:groups, :k],
                             f"views {views} groups {groups} k {k}")


@pytest.mark.parametrize("D", [64, 1000, 1025])
def test_one_view_is_topk(gpu_ctx, D):
    """views == 1 is ore_topk_f32 itself: the payload of a NaN survives"""
    import torch
    import ore
    rng = np.random.default_rng(D)
    x = rng.standard_normal((5, D)).astype(np.float32)
    x = np.where(rng.random((5, D)) < 0.3, _nan(rng, (5, D)), x)
    x[4, 2:] = _nan(rng, (D - 2,))  # a row whose best 64 reach into the NaNs
    xd = _cuda(x)
    k = min(D, 64)
    v1, i1 = ore.topk_mean(gpu_ctx, xd, 1, k)
    v0, i0 = ore.topk(gpu_ctx, xd, k)
    torch.cuda.synchronize()
    assert torch.equal(i1, i0) and torch.equal(v1.view(torch.int32), v0.view(torch.int32))
    assert bool(torch.isnan(v1).any())
    np.testing.assert_array_equal(_u32(v1.cpu().numpy()), _u32(np.take_along_axis(x, i1.cpu().numpy().astype(np.int64), 1)))


@pytest.mark.parametrize("D", [1000, 1025])
def test_topk_mean_row_stride(gpu_ctx, D):
    """x->nstride = D + 3 through the raw ABI: the 3 elements between rows would win every round if read."""
    import torch
    import ore
    from ore import _lib
    views, groups, gap, k = 3, 2, 3, 64
    rows = views * groups
    x = _input("ties", rows, D, seed=2)
    buf = np.full((rows, D + gap), np.float32(3e38), np.float32)
    buf[:, :D] = x
    xd = _cuda(buf)
    t = _lib.Tensor()
    t.data, t.ndim, t.nstride = xd.data_ptr(), 2, D + gap
    t.dims[0], t.dims[1] = rows, D
    v = torch.empty((groups, k), dtype=torch.float32, device="cuda")
    i = torch.empty((groups, k), dtype=torch.int32, device="cuda")
    L = ore.load()
    st = L.ore_topk_mean_f32(gpu_ctx.h, ctypes.byref(t), views, k, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(i.data_ptr()))
    assert st == 0, L.ore_last_error(gpu_ctx.h)
    want_v, want_i = _topk_ref(_mean_ref(x, views), k)
    _assert_topk(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
    t.dims[0] = 0  # no rows: fine, nothing launched
    assert L.ore_topk_mean_f32(gpu_ctx.h, ctypes.byref(t), views, k, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(i.data_ptr())) == 0
    t.dims[0] = rows - 1  # with a context too: not whole groups
    assert L.ore_topk_mean_f32(gpu_ctx.h, ctypes.byref(t), views, k, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(i.data_ptr())) == 1
    assert b"views" in L.ore_last_error(gpu_ctx.h)
    for bad in (0, 65):
        with pytest.raises(ore.OreError, match="views"):
            ore.topk_mean(gpu_ctx, xd, bad, 1)
    with pytest.raises(ore.OreError, match="multiple"):
        ore.topk_mean(gpu_ctx, xd, 4, 1)


# ------------------------------------------------------------------------------------------ mirrored list images
# (1,1), (5,7), (8,8); (3,64) and (2,65) put a wave boundary inside a row; (9,31) is 279 pixels, two blocks
OUTS = [(1, 1), (5, 7), (8, 8), (3, 64), (2, 65), (9, 31)]


def _geoms(out_hw):
    """A plain resize, the window in the far corner of a larger resized image (left + W == rw) and one inside."""
    h, w = out_hw
    return [((h, w), (0, 0)), ((h + 3, w + 5), (3, 5)), ((h + 4, w + 9), (1, 3))]


def _aa_ok(hs, ws, g):
    return hs <= 32 * g[0][0] and ws <= 32 * g[0][1]


@functools.lru_cache(maxsize=None)
def _sources(c):
    """Host arrays and how to cut them from device tensors: 37 x 53 (odd) and 64 x 48 (even) dense, and three
    windows of a 70 x 80 image (odd base address, a row stride above ws * c)."""
    a, b, big = images((37, 53, c), seed=500 + c), images((64, 48, c), seed=510 + c), images((70, 80, c), seed=520 + c)
    cuts = [(slice(3, 40), slice(5, 58)), (slice(6, 70), slice(31, 79)), (slice(1, 21), slice(2, 31))]
    return a, b, big, cuts


def _source_views(c):
    a, b, big, cuts = _sources(c)
    ad, bd, bigd = _cuda(a), _cuda(b), _cuda(big)
    dev = [ad, bd] + [bigd[r, q] for r, q in cuts]
    host = [a, b] + [np.ascontiguousarray(big[r, q]) for r, q in cuts]
    assert not dev[2].is_contiguous() and dev[2].stride(0) == 80 * c
    return dev, host


@contextlib.contextmanager
def _closing(*lists):
    try:
        yield lists
    finally:
        import torch
        torch.cuda.synchronize()  # the launches that read the tables have finished
        for lst in lists:
            lst.close()


def _doubled(items, seed):
    """Every item twice, once flipped and once not, in a mixed order of flags: two descriptors over the same bytes."""
    flips = [bool(b) for b in np.random.default_rng(seed).integers(0, 2, len(items))]
    if len(set(flips)) == 1:
        flips[0] = not flips[0]
    return items + items, flips + [not f for f in flips]


def _mirrored(y, flips):
    """The definition: image i with its columns reversed where flips[i]."""
    import torch
    return torch.stack([y[i].flip(-1) if f else y[i] for i, f in enumerate(flips)])


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_flipped_is_the_unflipped_mirrored(gpu_ctx, antialias, c):
    import torch
    import ore
    dev, host = _source_views(c)
    scale, shift = _norm(c)
    for out_hw in OUTS:
        items = [(d, g) for d, x in zip(dev, host) for g in _geoms(out_hw) if not antialias or _aa_ok(x.shape[0], x.shape[1], g)]
        assert len(items) >= 5 and len({id(d) for d, _ in items}) >= 3, out_hw
        items, flips = _doubled(items, seed=c + 10 * out_hw[1])
        srcs, geoms = [d for d, _ in items], [g for _, g in items]
        with _closing(ore.ImageList(gpu_ctx, len(items), out_hw, c, antialias)) as (lst,):
            for reverse in ((False, True) if c == 3 else (False,)):
                lst.set(srcs, geometries=geoms)  # the old entry
                plain = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift, reverse_channels=reverse)
                lst.set(srcs, geometries=geoms, flips=[False] * len(items))  # flags of zero: the same
                zero = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift, reverse_channels=reverse)
                lst.set(srcs, geometries=geoms, flips=flips)
                got = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift, reverse_channels=reverse)
                torch.cuda.synchronize()
                assert tuple(got.shape) == (len(items), c) + out_hw
                assert torch.equal(zero, plain), (out_hw, reverse)
                assert torch.equal(got, _mirrored(plain, flips)), (out_hw, reverse)
                if out_hw[1] > 1:
                    assert not torch.equal(got, plain)


@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_flipped_against_the_numpy_reference(gpu_ctx, antialias):
    """Directly against tests/_resize_ref.py / _resize_aa_ref.py with the columns reversed."""
    import ore
    dev, host = _source_views(3)
    out_hw = (9, 31)
    geoms = [_geoms(out_hw)[i % 3] for i in range(len(dev))]
    flips = [True, False, True, True, False]
    scale, shift = _norm(3)
    fn = resize_aa_ref if antialias else resize_ref
    with _closing(ore.ImageList(gpu_ctx, len(dev), out_hw, 3, antialias)) as (lst,):
        lst.set(dev, geometries=geoms, flips=flips)
        for reverse in (False, True):
            got = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift, reverse_channels=reverse).cpu().numpy()
            for i, (x, g, f) in enumerate(zip(host, geoms, flips)):
                want = fn(x[None], g[0], g[1], out_hw, scale, shift, reverse)[0]
                np.testing.assert_array_equal(got[i], want[..., ::-1] if f else want, err_msg=f"image {i}")


def _nv12_frames():
    """Odd frame sizes, an even one, and a region of interest of it at an even origin (views with pitches)."""
    def frame(hs, ws, seed):
        return images((hs, ws), seed=seed), images(((hs + 1) // 2, (ws + 1) // 2, 2), seed=seed + 1000)
    f = [frame(33, 47, 600), frame(7, 9, 602), frame(64, 96, 604)]
    y, uv = f[2]
    return f, (y[2:, 4:], uv[1:, 2:])


@pytest.mark.parametrize("matrix", NAMES)
@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_nv12_flipped(gpu_ctx, antialias, matrix):
    """A flipped NV12 image is the unflipped one mirrored, and what a flipped interleaved list gives for the
    converted bytes."""
    import torch
    import ore
    frames, (ry, ruv) = _nv12_frames()
    dev = [(_cuda(y), _cuda(uv)) for y, uv in frames]
    dev.append((dev[2][0][2:, 4:], dev[2][1][1:, 2:]))
    assert not dev[3][0].is_contiguous() and tuple(dev[3][1].shape) == (31, 46, 2)
    rgbs = [_cuda(ore.nv12_to_rgb(y, uv, matrix)) for y, uv in frames + [(ry, ruv)]]
    for out_hw in [(5, 7), (3, 64), (2, 65), (9, 31)]:
        items = [(i, g) for i in range(4) for g in _geoms(out_hw)]
        items, flips = _doubled(items, seed=out_hw[1])
        geoms = [g for _, g in items]
        nv = ore.Nv12ImageList(gpu_ctx, len(items), out_hw, matrix, antialias)
        il = ore.ImageList(gpu_ctx, len(items), out_hw, 3, antialias)
        with _closing(nv, il):
            for reverse in (False, True):
                nv.set([dev[i] for i, _ in items], geometries=geoms)
                plain = ore.preprocess_list_u8(gpu_ctx, nv, *_norm(3), reverse_channels=reverse)
                nv.set([dev[i] for i, _ in items], geometries=geoms, flips=flips)
                il.set([rgbs[i] for i, _ in items], geometries=geoms, flips=flips)
                got = ore.preprocess_list_u8(gpu_ctx, nv, *_norm(3), reverse_channels=reverse)
                want = ore.preprocess_list_u8(gpu_ctx, il, *_norm(3), reverse_channels=reverse)
                torch.cuda.synchronize()
                assert torch.equal(got, _mirrored(plain, flips)), (out_hw, reverse)
                assert torch.equal(got, want), (out_hw, reverse)
                assert not torch.equal(got, plain)


@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_flipped_into_slice(gpu_ctx, antialias):
    """y with an image stride above C*H*W (raw ABI), interleaved and NV12: the poisoned elements between the
    images stay poisoned."""
    import torch
    import ore
    from ore import _lib
    out_hw, gap, sentinel = (3, 64), 3, -12345.0
    per = 3 * out_hw[0] * out_hw[1]
    dev, _ = _source_views(3)
    frames, _ = _nv12_frames()
    fdev = [(_cuda(y), _cuda(uv)) for y, uv in frames]
    geoms = _geoms(out_hw)
    flips = [True, False, True]
    il = ore.ImageList(gpu_ctx, 3, out_hw, 3, antialias)
    nv = ore.Nv12ImageList(gpu_ctx, 3, out_hw, "bt709", antialias)
    L = ore.load()
    with _closing(il, nv):
        for lst, srcs in ((il, dev[:3]), (nv, fdev)):
            lst.set(srcs, geometries=geoms)
            plain = ore.preprocess_list_u8(gpu_ctx, lst)
            lst.set(srcs, geometries=geoms, flips=flips)
            ybuf = torch.full((3, per + gap), sentinel, dtype=torch.float32, device="cuda")
            t = _lib.Tensor()
            t.data, t.ndim, t.nstride = ybuf.data_ptr(), 4, per + gap
            for i, d in enumerate((3, 3) + out_hw):
                t.dims[i] = d
            st = L.ore_preprocess_list_u8(gpu_ctx.h, lst.h, None, None, 0, ctypes.byref(t))
            assert st == 0, L.ore_last_error(gpu_ctx.h)
            torch.cuda.synchronize()
            assert torch.equal(ybuf[:, :per].reshape((3, 3) + out_hw), _mirrored(plain, flips))
            assert bool((ybuf[:, per:] == sentinel).all())


@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "aa"])
def test_ten_crop(gpu_ctx, antialias):
    """multi_crop_geometries end to end: each of the ten list outputs is its window of the whole resized image
    (the dense entry with the window equal to the resized image), mirrored for the last five."""
    import torch
    import ore
    src_hw, short, out_hw = (40, 52), 32, (24, 24)
    x = _cuda(images(src_hw + (3,), seed=700))
    scale, shift = _norm(3)
    ten = ore.multi_crop_geometries(src_hw, short, out_hw, 10)
    resized = ten[0][0]
    assert resized == (32, 41)
    full = ore.preprocess_resize_u8(gpu_ctx, x[None], resized, resized, (0, 0), scale, shift, antialias=antialias)[0]
    with _closing(ore.ImageList(gpu_ctx, 10, out_hw, 3, antialias)) as (lst,):
        lst.set([x] * 10, geometries=[(r, o) for r, o, _ in ten], flips=[f for _, _, f in ten])
        got = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift)
        torch.cuda.synchronize()
        for i, (_, (top, left), flip) in enumerate(ten):
            want = full[:, top:top + 24, left:left + 24]
            assert torch.equal(got[i], want.flip(-1) if flip else want), i
        assert torch.equal(got[5], got[1].flip(-1)) and torch.equal(got[9], got[4].flip(-1))


def _fill(arr, tensors, geoms):
    from ore import _lib
    for i, (x, g) in enumerate(zip(tensors, geoms)):
        arr[i].data = x.data_ptr()
        arr[i].hs, arr[i].ws, arr[i].row_stride = int(x.shape[0]), int(x.shape[1]), int(x.stride(0))
        arr[i].g = _lib.Resize(g[0][0], g[0][1], g[1][0], g[1][1])


def test_unknown_flag_keeps_the_list(gpu_ctx):
    import torch
    import ore
    from ore import _lib
    L = ore.load()
    dev, _ = _source_views(3)
    out_hw = (5, 7)
    geoms = _geoms(out_hw)
    frames, _ = _nv12_frames()
    fdev = [(_cuda(y), _cuda(uv)) for y, uv in frames]
    il = ore.ImageList(gpu_ctx, 3, out_hw, 3)
    nv = ore.Nv12ImageList(gpu_ctx, 3, out_hw)
    with _closing(il, nv):
        il.set(dev[:3], geometries=geoms, flips=[True, False, True])
        before = ore.preprocess_list_u8(gpu_ctx, il).clone()
        arr = (_lib.ImageU8 * 3)()
        _fill(arr, dev[2:5], geoms)
        W = ctypes.c_uint32 * 3
        for bad in (W(0, 2, 0), W(1, 3, 1), W(0, 0x80000000, 1)):
            assert L.ore_image_list_set_ex(il.h, arr, bad, 3) == 1
            assert b"image 1" in L.ore_last_error(gpu_ctx.h) and b"flag" in L.ore_last_error(gpu_ctx.h)
        assert L.ore_image_list_set_ex(il.h, arr, W(0, 0, 2), 2) == 0  # only n words are read
        assert il.count == 2
        il.set(dev[:3], geometries=geoms, flips=[True, False, True])
        assert L.ore_image_list_set_ex(il.h, arr, W(4, 0, 0), 3) == 1 and b"image 0" in L.ore_last_error(gpu_ctx.h)
        assert il.count == 3
        torch.cuda.synchronize()
        assert torch.equal(ore.preprocess_list_u8(gpu_ctx, il), before)  # the previous content, flips included
        # the entry of the other format, with or without flags
        narr = (_lib.ImageNv12 * 3)()
        assert L.ore_image_list_set_nv12_ex(il.h, narr, W(0, 0, 0), 3) == 1 and b"interleaved" in L.ore_last_error(gpu_ctx.h)
        assert L.ore_image_list_set_ex(nv.h, arr, None, 3) == 1 and b"NV12" in L.ore_last_error(gpu_ctx.h)
        nv.set(fdev, geometries=geoms, flips=[False, True, True])
        nbefore = ore.preprocess_list_u8(gpu_ctx, nv).clone()
        for i, (y, uv) in enumerate(fdev):
            narr[i].y, narr[i].uv = y.data_ptr(), uv.data_ptr()
            narr[i].hs, narr[i].ws = int(y.shape[0]), int(y.shape[1])
            narr[i].g = _lib.Resize(out_hw[0], out_hw[1], 0, 0)
        assert L.ore_image_list_set_nv12_ex(nv.h, narr, W(0, 0, 6), 3) == 1 and b"image 2" in L.ore_last_error(gpu_ctx.h)
        torch.cuda.synchronize()
        assert nv.count == 3 and torch.equal(ore.preprocess_list_u8(gpu_ctx, nv), nbefore)
        assert L.ore_image_list_set_nv12_ex(nv.h, narr, W(1, 1, 1), 0) == 0 and nv.count == 0  # n == 0 empties


# ------------------------------------------------------------------------------------------ models
@contextlib.contextmanager
def _model(ctx, onnx_bytes, **kw):
    """A model closed even when the test fails: it must not outlive the session's context."""
    import ore
    m = ore.Model(ctx, onnx_bytes, **kw)
    try:
        yield m
    finally:
        m.close()


def _want(rows, views, k):
    return _topk_ref(_mean_ref(rows, views), k)


def _equal(got, want):
    assert tuple(got[0].shape) == tuple(got[1].shape) == want[1].shape
    np.testing.assert_array_equal(got[1].cpu().numpy(), want[1])
    np.testing.assert_array_equal(_u32(got[0].cpu().numpy()), _u32(want[0]))


def _list_inputs(c, out_hw, n, seed):
    """n list images of their own sizes with a window each and mixed flips"""
    h, w = out_hw
    sizes = [(h + 9, w + 20), (h, w), (h // 2 + 1, w + 3), (2 * h, 2 * w), (h + 1, w // 2), (h + 30, w + 30)]
    geoms = [((h + 4, w + 8), (2, 4)), ((h, w), (0, 0)), ((h, w + 2), (0, 2)), ((h + 2, w), (1, 0)), ((h, w), (0, 0)),
             ((h + 6, w + 6), (6, 6))]
    flips = [True, False, False, True, True, False]
    return [_cuda(images(s + (c,), seed=seed + i)) for i, s in enumerate(sizes[:n])], geoms[:n], flips[:n]


def _views_equal_run(ctx, m, x_u8, scale, shift, views, k):
    """classify* under set_views == the numpy mean / top-k of run*'s downloaded rows; steps and tiles unchanged;
    rows past n / views of a larger output buffer untouched."""
    import torch
    import ore
    n, c = x_u8.shape[0], x_u8.shape[3]
    groups = n // views
    assert n % views == 0 and groups < n <= m.max_batch
    steps, tiles = len(m.steps()), m.tiles()
    m.set_input_norm(scale, shift)
    xd8 = _cuda(x_u8)
    xf = _cuda(np.ascontiguousarray(x_u8.transpose(0, 3, 1, 2)).astype(np.float32) * scale.reshape(1, -1, 1, 1)
               + shift.reshape(1, -1, 1, 1))
    srcs, geoms, flips = _list_inputs(c, tuple(m.input_dims[1:]), n, seed=800)
    assert m.views == 1
    m.set_topk(k)
    with _closing(ore.ImageList(ctx, n, tuple(m.input_dims[1:]), c)) as (lst,):
        lst.set(srcs, geometries=geoms, flips=flips)
        one = m.classify(xf)  # one view: today's classify
        m.set_views(views)
        assert m.views == views
        rows, rows8, rowsl = m.run(xf).cpu().numpy(), m.run_u8(xd8).cpu().numpy(), m.run_u8_list(lst).cpu().numpy()
        assert rows.shape == rows8.shape == rowsl.shape == (n, m.output_elems)  # the runs ignore the views
        _equal(one, _topk_ref(rows, k))
        _equal(m.classify(xf), _want(rows, views, k))
        _equal(m.classify_u8(xd8), _want(rows8, views, k))
        _equal(m.classify_u8_list(lst), _want(rowsl, views, k))
        lst.set(srcs, geometries=geoms)  # without the flips the rows, and so the means, differ
        assert not np.array_equal(m.run_u8_list(lst).cpu().numpy(), rowsl)
    assert len(m.steps()) == steps and m.tiles() == tiles  # the selection is not an exec step
    big_s = torch.full((m.max_batch, k), -7.0, dtype=torch.float32, device="cuda")
    big_c = torch.full((m.max_batch, k), -7, dtype=torch.int32, device="cuda")
    m.classify_into(xf, big_s[:groups], big_c[:groups])
    want_v, want_i = _want(rows, views, k)
    rest = m.max_batch - groups
    np.testing.assert_array_equal(big_c.cpu().numpy(), np.concatenate([want_i, np.full((rest, k), -7, np.int32)]))
    np.testing.assert_array_equal(_u32(big_s.cpu().numpy()), _u32(np.concatenate([want_v, np.full((rest, k), -7.0, np.float32)])))


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_squeezenet_views(gpu_ctx, precision):
    from ore import squeezenet
    scale, shift = _norm(3)
    with _model(gpu_ctx, squeezenet.build(64), max_batch=8, precision=precision) as m:
        _views_equal_run(gpu_ctx, m, images((6, 64, 64, 3), seed=801), scale, shift, views=2, k=5)


def test_mnist_views(gpu_ctx):
    with open(os.path.join(GOLD, "mnist-8.onnx"), "rb") as f:
        onnx = f.read()
    with _model(gpu_ctx, onnx, max_batch=8) as m:
        assert m.output_elems == 10
        _views_equal_run(gpu_ctx, m, images((6, 28, 28, 1), seed=802), np.array([1.0 / 255.0], np.float32),
                         np.array([-0.5], np.float32), views=3, k=3)


def test_capture_classify_u8_list_with_views():
    """Captured once with views = 2, replayed after a set with the same count, new images and new flips: the
    graph reads the table, flags included, at replay and keeps its views."""
    import torch
    import ore
    from ore import squeezenet
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    m = ore.Model(ctx, squeezenet.build(64), max_batch=4)
    lst = ore.ImageList(ctx, 4, (64, 64), 3)
    try:
        k = 5
        m.set_input_norm(*_norm(3))
        m.set_topk(k)
        m.set_views(2)
        a, ga, fa = _list_inputs(3, (64, 64), 4, seed=810)
        b, gb, fb = _list_inputs(3, (64, 64), 4, seed=820)
        b, gb, fb = b[::-1], gb[::-1], [True, True, False, True]
        fa = [False] * 4  # captured on a list without a flip: the replay must still read the flags of the next set
        torch.cuda.synchronize()
        wants = []
        for srcs, geoms, flips in ((a, ga, fa), (b, gb, fb)):
            lst.set(srcs, geometries=geoms, flips=flips)
            wants.append(m.classify_u8_list(lst))  # eager, on the context's stream, into buffers of their own
        s.synchronize()
        assert not torch.equal(wants[0][0], wants[1][0])
        scores = torch.empty((2, k), dtype=torch.float32, device="cuda")
        classes = torch.empty((2, k), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        lst.set(a, geometries=ga, flips=fa)
        m.capture_classify_u8_list(lst, scores, classes)  # capture only: nothing runs yet
        m.replay()
        s.synchronize()
        assert torch.equal(classes, wants[0][1]) and torch.equal(scores.view(torch.int32), wants[0][0].view(torch.int32))
        lst.set(b, geometries=gb, flips=fb)
        m.set_views(1)  # the graph keeps the views it was captured with
        m.replay()
        s.synchronize()
        assert torch.equal(classes, wants[1][1]) and torch.equal(scores.view(torch.int32), wants[1][0].view(torch.int32))
    finally:
        s.synchronize()
        lst.close()
        m.close()
        ctx.close()


def test_views_errors(gpu_ctx):
    import torch
    import ore
    from ore import squeezenet
    L = ore.load()
    with _model(gpu_ctx, squeezenet.build(64), max_batch=4) as m:
        assert 2 <= m.run_batch <= 4
        for bad in (0, -1, 65, m.run_batch + 1):  # the last: within ORE_MAX_VIEWS but above the run batch
            with pytest.raises(ore.OreError, match="views"):
                m.set_views(bad)
            assert L.ore_model_set_views(m.h, bad) == 1 and b"views" in L.ore_last_error(gpu_ctx.h)
        assert m.views == 1
        m.set_topk(5)
        m.set_views(2)
        x3 = torch.zeros((3, 3, 64, 64), device="cuda")
        x38 = torch.zeros((3, 64, 64, 3), dtype=torch.uint8, device="cuda")
        x4 = torch.rand((4, 3, 64, 64), device="cuda")
        s = torch.empty((4, 5), dtype=torch.float32, device="cuda")
        c = torch.empty((4, 5), dtype=torch.int32, device="cuda")
        with pytest.raises(ore.OreError, match="multiple of views"):
            m.classify(x3)
        with pytest.raises(ore.OreError, match="multiple of views"):
            m.classify_u8(x38)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        for entry, xin in ((L.ore_model_classify, x3), (L.ore_model_classify_u8, x38),
                           (L.ore_model_graph_capture_classify, x3), (L.ore_model_graph_capture_classify_u8, x38)):
            assert entry(m.h, p(xin), 3, p(s), p(c)) == 1
            assert b"multiple of views" in L.ore_last_error(gpu_ctx.h)
        for fn in (m.classify_into, m.capture_classify):
            with pytest.raises(ore.OreError, match="shape"):  # [n, k] where [n / views, k] is expected
                fn(x4, s, c)
        with _closing(ore.ImageList(gpu_ctx, 4, (64, 64), 3)) as (lst,):
            srcs, geoms, flips = _list_inputs(3, (64, 64), 3, seed=830)
            lst.set(srcs, geometries=geoms, flips=flips)
            with pytest.raises(ore.OreError, match="multiple of views"):
                m.classify_u8_list(lst)
            for entry in (L.ore_model_classify_u8_list, L.ore_model_graph_capture_classify_u8_list):
                assert entry(m.h, lst.h, p(s), p(c)) == 1 and b"multiple of views" in L.ore_last_error(gpu_ctx.h)
            with pytest.raises(ore.OreError, match="shape"):
                m.classify_u8_list_into(lst.set(srcs + srcs[:1], geometries=geoms + geoms[:1]), s, c)
            assert tuple(m.run_u8_list(lst).shape) == (4, m.output_elems)
        # the model stays usable
        _equal(m.classify(x4), _want(m.run(x4).cpu().numpy(), 2, 5))
    torch.cuda.synchronize()


def test_chunked_views(gpu_ctx):
    """As test_topk_gpu.py::test_chunked_classify with groups that do not divide the run batch: the chunks hold
    whole groups, and chunk c's results go to rows [g0, g0 + gc)."""
    import torch
    from ore import squeezenet
    k = 5
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        views = min(v for v in range(2, 8) if m.run_batch % v)
        n = (m.run_batch // views + 1) * views
        assert m.run_batch < n <= 2048 and n % views == 0
        g = torch.Generator(device="cuda").manual_seed(9)
        x = torch.rand((n, 3, 224, 224), dtype=torch.float32, device="cuda", generator=g)
        m.set_topk(k)
        m.set_views(views)
        rows = m.run(x).cpu().numpy()
        _equal(m.classify(x), _want(rows, views, k))
