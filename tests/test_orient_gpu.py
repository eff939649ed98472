"""GPU: oriented image lists (ore_image_list_set_oriented and its NV12 / YUV forms).

An oriented descriptor is specified to the bit: the unoriented descriptor of the stored-space window
ore_orient_geometry gives, over a list of shape (hz, wz), with its rows and / or columns reversed and then transposed
(and mirrored on top where it carries ORE_IMAGE_FLIP_H).  So every comparison here is exact, twice over: against
today's kernels through the unoriented lists, and against the numpy references of tests/_orient_ref.py.

Output shapes: (5, 7), the suite's usual one, and (17, 33), which is no multiple of any tile and crosses tile edges in
both directions.  Sources: windows of 9 .. 90 pixels a side with odd sizes, cut from one larger image, so each has a
row stride of its own and most an odd base address."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

from _nv12_ref import NAMES as MATRICES
from _orient_ref import CODES, FILTERS, TRANSPOSE, displayed_hw, orient_geometry_ref, oriented_ref
from _resize_ref import images
from _yuv_ref import NAMES as FORMATS, frame, make_planes, yuyv_width

pytestmark = pytest.mark.gpu

OUTS = [(5, 7), (17, 33)]
_MEAN = np.array([0.485, 0.456, 0.406, 0.5], np.float32)
_STD = np.array([0.229, 0.224, 0.225, 0.25], np.float32)
# (row, column, hs, ws) of the sources inside a 97 x 103 image
CUTS = [(1, 2, 9, 13), (3, 5, 37, 53), (6, 31, 89, 61), (40, 1, 23, 31), (51, 11, 45, 90)]
RATIO = {"bilinear": None, "aa": 32, "bicubic": None, "bicubic_aa": 16}


def _norm(c):
    return ((np.float32(1.0) / (np.float32(255.0) * _STD[:c])).astype(np.float32), (-_MEAN[:c] / _STD[:c]).astype(np.float32))


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _big(c):
    return images((97, 103, c), seed=1100 + c)


def _source_views(c):
    big = _big(c)
    bigd = _cuda(big)
    dev = [bigd[r:r + hs, q:q + ws] for r, q, hs, ws in CUTS]
    host = [np.ascontiguousarray(big[r:r + hs, q:q + ws]) for r, q, hs, ws in CUTS]
    assert all(d.stride(0) == 103 * c and not d.is_contiguous() for d in dev)
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


def _geoms(out_hw):
    """Displayed space: a plain resize, the window in the far corner of a larger resized image, and one inside."""
    h, w = out_hw
    return [((h, w), (0, 0)), ((h + 3, w + 5), (3, 5)), ((h + 4, w + 9), (1, 3))]


def _ratio_ok(name, src_hw, code, g, out_hw):
    """The ratio rule, on the stored axes against the stored-space resized size."""
    if RATIO[name] is None:
        return True
    (rh_s, rw_s) = orient_geometry_ref(code, g[0], g[1], out_hw)[0]
    return src_hw[0] <= RATIO[name] * rh_s and src_hw[1] <= RATIO[name] * rw_s


def _items(name, sizes, out_hw, rounds=2):
    """[(source index, code, geometry, flip)]: every code `rounds` times over mixed sources and geometries, some flagged."""
    out = []
    for k in range(8 * rounds):
        code, src, flip = CODES[k % 8], (3 * k + k // 8) % len(sizes), (k + k // 8) % 3 == 1
        for t in range(3):  # the first of the three geometries the filter's ratio rule accepts for this source
            g = _geoms(out_hw)[(k + k // 8 + t) % 3]
            if _ratio_ok(name, sizes[src], code, g, out_hw):
                out.append((src, code, g, flip))
                break
    assert {i[1] for i in out} == set(CODES) and len({i[0] for i in out}) >= 4
    assert {(i[1] in TRANSPOSE, i[3]) for i in out} == {(False, False), (False, True), (True, False), (True, True)}
    return out


def _permuted(z, code, flip):
    """The definition in torch: z [C, hz, wz] of the stored window -> the displayed [C, h, w]."""
    _, _, _, rr, rc, tr = orient_geometry_ref(code, (1, 1), (0, 0), (1, 1))
    if rr:
        z = z.flip(-2)
    if rc:
        z = z.flip(-1)
    if tr:
        z = z.transpose(-1, -2)
    return z.flip(-1) if flip else z


def _unoriented(ctx, make_list, srcs, items, out_hw, **kw):
    """Today's kernels as the yardstick: every item through an unoriented list of shape (hz, wz) with the stored-space
    window ore_orient_geometry gives, then permuted in torch.  make_list(n, out_hw) -> a list of the kind under test."""
    import torch
    import ore
    want = [None] * len(items)
    for tr in (False, True):
        idx = [i for i, it in enumerate(items) if (it[1] in TRANSPOSE) == tr]
        shape = (out_hw[1], out_hw[0]) if tr else out_hw
        stored = [ore.orient_geometry(items[i][1], items[i][2][0], items[i][2][1], out_hw) for i in idx]
        assert all(s[2] == shape and s[:3] == orient_geometry_ref(items[i][1], items[i][2][0], items[i][2][1], out_hw)[:3]
                   for s, i in zip(stored, idx))
        with _closing(make_list(len(idx), shape)) as (lst,):
            lst.set([srcs[items[i][0]] for i in idx], geometries=[(s[0], s[1]) for s in stored])
            assert not lst.oriented
            z = ore.preprocess_list_u8(ctx, lst, **kw)
            torch.cuda.synchronize()
            for j, i in enumerate(idx):
                want[i] = _permuted(z[j], items[i][1], items[i][3]).contiguous()
    return torch.stack(want)


def _set_oriented(lst, srcs, items):
    return lst.set_oriented([srcs[i[0]] for i in items], [i[1] for i in items], geometries=[i[2] for i in items],
                            flips=[i[3] for i in items])


# ------------------------------------------------------------------------------------------ interleaved lists
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("name", list(FILTERS))
def test_oriented_is_the_unoriented_permuted(gpu_ctx, name, c):
    import torch
    import ore
    (aa, cubic), fn = FILTERS[name]
    dev, host = _source_views(c)
    scale, shift = _norm(c)
    for out_hw in OUTS:
        items = _items(name, [x.shape[:2] for x in host], out_hw)
        make = lambda n, hw: ore.ImageList(gpu_ctx, n, hw, c, aa, cubic)  # noqa: E731
        with _closing(make(len(items), out_hw)) as (lst,):
            assert not lst.oriented
            _set_oriented(lst, dev, items)
            assert lst.oriented and lst.count == len(items)
            for reverse in ((False, True) if c == 3 else (False,)):
                kw = dict(scale=scale, shift=shift, reverse_channels=reverse)
                got = ore.preprocess_list_u8(gpu_ctx, lst, **kw)
                want = _unoriented(gpu_ctx, make, dev, items, out_hw, **kw)
                assert tuple(got.shape) == (len(items), c) + out_hw
                for i, it in enumerate(items):
                    assert torch.equal(got[i], want[i]), (out_hw, reverse, i, it[1:])
                gh = got.cpu().numpy()
                for i, (src, code, g, flip) in enumerate(items):
                    ref = oriented_ref(fn, host[src], code, g[0], g[1], out_hw, flip, scale=scale, shift=shift, reverse=reverse)
                    np.testing.assert_array_equal(gh[i], ref, err_msg=f"{out_hw} reverse {reverse} image {i} code {code}")


def test_short_and_plain_resize_use_the_displayed_size(gpu_ctx):
    """short= and the default geometry of set_oriented are those of the displayed image: a portrait photo stored
    landscape (code 6) is cropped as the portrait it shows."""
    import torch
    import ore
    dev, host = _source_views(3)
    x, xh = dev[4], host[4]  # 45 x 90 stored, 90 x 45 displayed
    out_hw = (17, 33)
    resized, origin = ore.center_crop_geometry((90, 45), 40, out_hw)
    assert resized == (80, 40)
    with _closing(ore.ImageList(gpu_ctx, 2, out_hw, 3)) as (lst,):
        lst.set_oriented([x, x], [6, 8], short=40)
        a = ore.preprocess_list_u8(gpu_ctx, lst).cpu().numpy()
        lst.set_oriented([x, x], [6, 8])
        b = ore.preprocess_list_u8(gpu_ctx, lst).cpu().numpy()
        torch.cuda.synchronize()
        fn = FILTERS["bilinear"][1]
        for i, code in enumerate((6, 8)):
            np.testing.assert_array_equal(a[i], oriented_ref(fn, xh, code, resized, origin, out_hw))
            np.testing.assert_array_equal(b[i], oriented_ref(fn, xh, code, out_hw, (0, 0), out_hw))
        with pytest.raises(ore.OreError, match="crop"):  # 17 + 33 > 40 columns of the displayed image; 80 stored ones would do
            lst.set_oriented([x], [6], geometries=[(resized, (0, 17))])
        assert lst.count == 2


# ------------------------------------------------------------------------------------------ NV12 and YUV lists
NV12_SIZES = [(33, 47), (7, 9), (45, 61), (62, 92)]  # the last: a window of a 64 x 96 frame at (2, 4)


@functools.lru_cache(maxsize=None)
def _nv12_host():
    def fr(hs, ws, seed):
        return images((hs, ws), seed=seed), images(((hs + 1) // 2, (ws + 1) // 2, 2), seed=seed + 1000)
    f = [fr(33, 47, 1200), fr(7, 9, 1202), fr(45, 61, 1204), fr(64, 96, 1206)]
    return f[:3] + [(f[3][0][2:, 4:], f[3][1][1:, 2:])], f[3]


def _nv12_dev():
    frames, whole = _nv12_host()
    dev = [(_cuda(y), _cuda(uv)) for y, uv in frames[:3]]
    wy, wuv = _cuda(whole[0]), _cuda(whole[1])
    dev.append((wy[2:, 4:], wuv[1:, 2:]))
    assert not dev[3][0].is_contiguous() and tuple(dev[3][1].shape) == (31, 46, 2)
    return dev


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("name", list(FILTERS))
def test_nv12_oriented_equals_the_interleaved_oriented(gpu_ctx, name, matrix):
    import torch
    import ore
    aa, cubic = FILTERS[name][0]
    frames, _ = _nv12_host()
    dev = _nv12_dev()
    rgbs = [_cuda(ore.nv12_to_rgb(np.ascontiguousarray(y), np.ascontiguousarray(uv), matrix)) for y, uv in frames]
    for out_hw in OUTS:
        items = _items(name, NV12_SIZES, out_hw)
        nv = ore.Nv12ImageList(gpu_ctx, len(items), out_hw, matrix, aa, cubic)
        il = ore.ImageList(gpu_ctx, len(items), out_hw, 3, aa, cubic)
        with _closing(nv, il):
            _set_oriented(nv, dev, items)
            _set_oriented(il, rgbs, items)
            for reverse in (False, True):
                kw = dict(scale=_norm(3)[0], shift=_norm(3)[1], reverse_channels=reverse)
                got = ore.preprocess_list_u8(gpu_ctx, nv, **kw)
                want = ore.preprocess_list_u8(gpu_ctx, il, **kw)
                torch.cuda.synchronize()
                assert torch.equal(got, want), (out_hw, reverse)
            if name == "bilinear":  # and against today's NV12 kernels directly
                make = lambda n, hw: ore.Nv12ImageList(gpu_ctx, n, hw, matrix, aa, cubic)  # noqa: E731
                assert torch.equal(ore.preprocess_list_u8(gpu_ctx, nv), _unoriented(gpu_ctx, make, dev, items, out_hw))


YUV_SIZES = [(33, 47), (7, 9)]


@functools.lru_cache(maxsize=None)
def _yuv_host():
    """One frame per format and size, odd sizes: the last row and column have a chroma sample of their own."""
    return [(fmt, make_planes(fmt, hs, ws, 1300 + 10 * k + j), hs, ws) for k, fmt in enumerate(FORMATS)
            for j, (hs, ws) in enumerate(YUV_SIZES)]


@pytest.mark.parametrize("name", list(FILTERS))
def test_yuv_oriented_equals_the_interleaved_oriented(gpu_ctx, name):
    import torch
    import ore
    aa, cubic = FILTERS[name][0]
    host = _yuv_host()
    assert len(host) == 16 and {f[0] for f in host} == set(FORMATS)
    dev = [frame(fmt, [_cuda(p) for p in planes], yuyv_width(fmt, ws)) for fmt, planes, hs, ws in host]
    matrix = "bt601_full"
    rgbs = [_cuda(ore.yuv_planes_to_rgb(fmt, planes, matrix, ws=yuyv_width(fmt, ws))) for fmt, planes, hs, ws in host]
    for out_hw in OUTS:
        # every frame under two codes, one of them transposing: frame k meets codes k % 8 + 1 and (k + 4) % 8 + 1
        items = []
        for k in range(32):
            src, code = k % 16, CODES[(k + 4 * (k // 16)) % 8]
            g = next(g for t in range(3) for g in [_geoms(out_hw)[(k + t) % 3]] if _ratio_ok(name, host[src][2:], code, g, out_hw))
            items.append((src, code, g, k % 3 == 1))
        assert all({it[1] in TRANSPOSE for it in items if host[it[0]][0] == fmt} == {False, True} for fmt in FORMATS)
        yl = ore.YuvImageList(gpu_ctx, len(items), out_hw, matrix, aa, cubic)
        il = ore.ImageList(gpu_ctx, len(items), out_hw, 3, aa, cubic)
        with _closing(yl, il):
            _set_oriented(yl, dev, items)
            _set_oriented(il, rgbs, items)
            kw = dict(scale=_norm(3)[0], shift=_norm(3)[1], reverse_channels=True)
            got = ore.preprocess_list_u8(gpu_ctx, yl, **kw)
            want = ore.preprocess_list_u8(gpu_ctx, il, **kw)
            torch.cuda.synchronize()
            for i, it in enumerate(items):
                assert torch.equal(got[i], want[i]), (out_hw, i, host[it[0]][0], it[1:])


# ------------------------------------------------------------------------------------------ y as a slice
@pytest.mark.parametrize("name", list(FILTERS))
def test_oriented_into_a_poisoned_slice(gpu_ctx, name):
    """y through the raw ABI with an image stride above C*H*W and a base that is only 4-byte aligned, NaN everywhere
    first: under transposing codes at (17, 33) -- ragged in both directions -- the elements between the images, before
    the first and after the last stay NaN, and the images are the dense result."""
    import torch
    import ore
    from ore import _lib
    aa, cubic = FILTERS[name][0]
    out_hw, gap, lead = (17, 33), 5, 3
    per = 3 * out_hw[0] * out_hw[1]
    dev, host = _source_views(3)
    items = [(k % 5, code, _geoms(out_hw)[k % 3], k % 2 == 1) for k, code in enumerate((6, 8, 5, 7, 6, 3))]
    items = [it for it in items if _ratio_ok(name, host[it[0]].shape[:2], it[1], it[2], out_hw)]
    n = len(items)
    assert n >= 4
    nv_items = [(k % 4, code, _geoms(out_hw)[k % 3], k % 2 == 0) for k, code in enumerate((8, 6, 7, 5))]
    yuv_host = _yuv_host()
    yuv_dev = [frame(fmt, [_cuda(p) for p in planes], yuyv_width(fmt, ws)) for fmt, planes, hs, ws in yuv_host]
    yuv_items = [(2 * k, code, _geoms(out_hw)[k % 3], k % 2 == 1) for k, code in enumerate((6, 5, 8, 7, 6, 8, 5, 7))]
    il = ore.ImageList(gpu_ctx, n, out_hw, 3, aa, cubic)
    nv = ore.Nv12ImageList(gpu_ctx, 4, out_hw, "bt709", aa, cubic)
    yl = ore.YuvImageList(gpu_ctx, 8, out_hw, "bt601_full", aa, cubic)
    L = ore.load()
    nan_bits = torch.tensor(float("nan")).view(torch.int32).item()
    with _closing(il, nv, yl):
        for lst, srcs, its in ((il, dev, items), (nv, _nv12_dev(), nv_items), (yl, yuv_dev, yuv_items)):
            _set_oriented(lst, srcs, its)
            m = len(its)
            dense = ore.preprocess_list_u8(gpu_ctx, lst)
            buf = torch.full((lead + m * (per + gap) + 1,), float("nan"), dtype=torch.float32, device="cuda")
            t = _lib.Tensor()
            t.data, t.ndim, t.nstride = buf.data_ptr() + 4 * lead, 4, per + gap
            assert t.data % 16 != 0
            for i, d in enumerate((m, 3) + out_hw):
                t.dims[i] = d
            st = L.ore_preprocess_list_u8(gpu_ctx.h, lst.h, None, None, 0, ctypes.byref(t))
            assert st == 0, L.ore_last_error(gpu_ctx.h)
            torch.cuda.synchronize()
            body = buf[lead:lead + m * (per + gap)].reshape(m, per + gap)
            assert torch.equal(body[:, :per].reshape((m, 3) + out_hw), dense)
            assert not bool(torch.isnan(dense).any())
            bits = buf.view(torch.int32)
            assert bool((bits[:lead] == nan_bits).all()) and bool((bits[-1:] == nan_bits).all())
            assert bool((body[:, per:].contiguous().view(torch.int32) == nan_bits).all())


# ------------------------------------------------------------------------------------------ past the grid's rows
@pytest.mark.parametrize("name", ["bilinear", "bicubic_aa"])
def test_oriented_past_the_grid_limit(gpu_ctx, name):
    """65,539 oriented descriptors, more than a grid's 65,535 rows, so four blocks visit a second descriptor (on the
    pattern of test_image_list_gpu.py::test_past_the_grid_limit).  Codes cycle with period four, which does not divide
    65,535: descriptors i and i + 65,535 of a block differ, a transposing one (through the LDS tile) follows an upright
    one and the other way round.  bicubic_aa is the 128-thread kernel with its weights' dynamic LDS beside the tile."""
    import ore
    (aa, cubic), fn = FILTERS[name]
    n, out_hw = 65539, (2, 3)
    assert 65535 % 4 != 0
    codes, flips = (1, 6, 3, 5), (False, True, False, False)
    pool = [images(hw + (3,), seed=1900 + k) for k, hw in enumerate([(3, 5), (6, 4), (2, 7), (5, 5)])]  # stored sizes
    geoms = [((3, 5), (1, 1)), ((4, 4), (1, 0)), ((3, 4), (0, 1)), ((4, 5), (2, 2))]  # displayed space: resize and crop
    scale, shift = _norm(3)
    refs = np.stack([oriented_ref(fn, pool[k], codes[k], geoms[k][0], geoms[k][1], out_hw, flips[k], scale=scale, shift=shift)
                     for k in range(4)])
    assert len({r.tobytes() for r in refs}) == 4
    dev = [_cuda(x) for x in pool]
    idx = np.arange(n) % 4
    with _closing(ore.ImageList(gpu_ctx, n, out_hw, 3, aa, cubic)) as (lst,):
        lst.set_oriented([dev[k] for k in idx], [codes[k] for k in idx], geometries=[geoms[k] for k in idx],
                         flips=[flips[k] for k in idx])
        assert lst.oriented and lst.count == n
        y = ore.preprocess_list_u8(gpu_ctx, lst, scale=scale, shift=shift).cpu().numpy()
    np.testing.assert_array_equal(y, refs[idx])


# ------------------------------------------------------------------------------------------ the entries' contract
def _fill(arr, tensors, geoms):
    from ore import _lib
    for i, (x, g) in enumerate(zip(tensors, geoms)):
        arr[i].data = x.data_ptr()
        arr[i].hs, arr[i].ws, arr[i].row_stride = int(x.shape[0]), int(x.shape[1]), int(x.stride(0))
        arr[i].g = _lib.Resize(g[0][0], g[0][1], g[1][0], g[1][1])


@pytest.mark.parametrize("name", ["bilinear", "bicubic_aa"])
def test_all_one_codes_and_null_are_set_ex(gpu_ctx, name):
    import torch
    import ore
    from ore import _lib
    aa, cubic = FILTERS[name][0]
    dev, host = _source_views(3)
    out_hw = (17, 33)
    geoms = [_geoms(out_hw)[k % 3] for k in range(5)]
    flips = [True, False, False, True, True]
    L = ore.load()
    a = ore.ImageList(gpu_ctx, 5, out_hw, 3, aa, cubic)
    b = ore.ImageList(gpu_ctx, 5, out_hw, 3, aa, cubic)
    with _closing(a, b):
        want = ore.preprocess_list_u8(gpu_ctx, a.set(dev, geometries=geoms, flips=flips))
        ones = ore.preprocess_list_u8(gpu_ctx, b.set_oriented(dev, [1] * 5, geometries=geoms, flips=flips))
        assert b.oriented and not a.oriented
        torch.cuda.synchronize()
        assert torch.equal(ones, want)
        arr = (_lib.ImageU8 * 5)()
        _fill(arr, dev, geoms)
        words = (ctypes.c_uint32 * 5)(*[1 if f else 0 for f in flips])
        b.set_oriented(dev[:2], [6, 8])  # something else in between
        assert L.ore_image_list_set_oriented(b.h, arr, words, None, 5) == 0, L.ore_last_error(gpu_ctx.h)
        null = ore.preprocess_list_u8(gpu_ctx, b)
        assert L.ore_image_list_set_oriented(b.h, arr, None, None, 5) == 0
        bare = ore.preprocess_list_u8(gpu_ctx, b)
        want_bare = ore.preprocess_list_u8(gpu_ctx, a.set(dev, geometries=geoms))
        torch.cuda.synchronize()
        assert torch.equal(null, want) and torch.equal(bare, want_bare)
        assert L.ore_image_list_set_oriented(b.h, arr, None, None, 0) == 0 and b.count == 0  # n == 0 empties
        assert L.ore_image_list_set_oriented(a.h, None, None, None, 0) == 0 and a.oriented  # and marks


def test_rejected_oriented_set_keeps_the_list(gpu_ctx):
    import torch
    import ore
    from ore import _lib
    L = ore.load()
    dev, _ = _source_views(3)
    out_hw = (5, 7)
    geoms = _geoms(out_hw)
    frames = _nv12_dev()
    il = ore.ImageList(gpu_ctx, 3, out_hw, 3)
    nv = ore.Nv12ImageList(gpu_ctx, 3, out_hw)
    yl = ore.YuvImageList(gpu_ctx, 3, out_hw)
    U8 = ctypes.c_uint8 * 3
    with _closing(il, nv, yl):
        il.set_oriented(dev[:3], [6, 3, 8], geometries=geoms, flips=[True, False, True])
        before = ore.preprocess_list_u8(gpu_ctx, il).clone()
        arr = (_lib.ImageU8 * 3)()
        _fill(arr, dev[2:5], geoms)
        for bad in (U8(1, 0, 1), U8(6, 9, 6), U8(8, 200, 0)):  # a bad code at index 1 (and a later one: the first is named)
            assert L.ore_image_list_set_oriented(il.h, arr, None, bad, 3) == 1
            assert b"image 1" in L.ore_last_error(gpu_ctx.h) and b"orientation" in L.ore_last_error(gpu_ctx.h)
        _fill(arr, dev[2:5], [geoms[0], ((5, 7), (1, 0)), geoms[2]])  # a bad geometry at index 1
        assert L.ore_image_list_set_oriented(il.h, arr, None, U8(6, 6, 6), 3) == 1
        assert b"image 1" in L.ore_last_error(gpu_ctx.h) and b"crop" in L.ore_last_error(gpu_ctx.h)
        _fill(arr, dev[2:5], geoms)
        assert L.ore_image_list_set_oriented(il.h, arr, (ctypes.c_uint32 * 3)(0, 2, 0), U8(6, 6, 6), 3) == 1  # an unknown flag
        assert b"image 1" in L.ore_last_error(gpu_ctx.h) and b"flag" in L.ore_last_error(gpu_ctx.h)
        with pytest.raises(ore.OreError, match="crop"):
            il.set_oriented(dev[:3], [6, 6, 6], geometries=[geoms[0], ((5, 7), (1, 0)), geoms[2]])
        # the entries of the other kinds
        narr, yarr = (_lib.ImageNv12 * 3)(), (_lib.ImageYuv * 3)()
        assert L.ore_image_list_set_nv12_oriented(il.h, narr, None, U8(1, 1, 1), 3) == 1 and b"interleaved" in L.ore_last_error(gpu_ctx.h)
        assert L.ore_image_list_set_yuv_oriented(il.h, yarr, None, U8(1, 1, 1), 3) == 1 and b"interleaved" in L.ore_last_error(gpu_ctx.h)
        assert L.ore_image_list_set_oriented(nv.h, arr, None, U8(6, 6, 6), 3) == 1 and b"NV12" in L.ore_last_error(gpu_ctx.h)
        assert L.ore_image_list_set_oriented(yl.h, arr, None, U8(6, 6, 6), 3) == 1 and b"YUV" in L.ore_last_error(gpu_ctx.h)
        assert L.ore_image_list_set_yuv_oriented(nv.h, yarr, None, U8(6, 6, 6), 3) == 1
        assert not nv.oriented and not yl.oriented and nv.count == 0  # a rejected set marks nothing
        torch.cuda.synchronize()
        assert il.count == 3 and il.oriented
        assert torch.equal(ore.preprocess_list_u8(gpu_ctx, il), before)  # content, count and orientations
        # an NV12 list likewise
        nv.set_oriented(frames[:3], [8, 5, 2], geometries=geoms)
        nbefore = ore.preprocess_list_u8(gpu_ctx, nv).clone()
        for i, (y, uv) in enumerate(frames[:3]):
            narr[i].y, narr[i].uv = y.data_ptr(), uv.data_ptr()
            narr[i].hs, narr[i].ws = int(y.shape[0]), int(y.shape[1])
            narr[i].y_stride, narr[i].uv_stride = int(y.stride(0)), int(uv.stride(0))
            narr[i].g = _lib.Resize(out_hw[0], out_hw[1], 0, 0)
        assert L.ore_image_list_set_nv12_oriented(nv.h, narr, None, U8(1, 6, 0), 3) == 1 and b"image 2" in L.ore_last_error(gpu_ctx.h)
        torch.cuda.synchronize()
        assert nv.count == 3 and torch.equal(ore.preprocess_list_u8(gpu_ctx, nv), nbefore)
        assert L.ore_image_list_set_nv12_oriented(nv.h, narr, None, U8(1, 6, 7), 3) == 0
        assert not torch.equal(ore.preprocess_list_u8(gpu_ctx, nv), nbefore)


def test_sets_and_runs_are_stream_ordered(gpu_ctx):
    """set, run, set, run with no synchronisation in between: each run sees its own table."""
    import torch
    import ore
    dev, host = _source_views(3)
    out_hw = (17, 33)
    fn = FILTERS["bilinear"][1]
    a = [(k, code, _geoms(out_hw)[k % 3], False) for k, code in enumerate((6, 1, 8, 3, 5))]
    b = [(4 - k, code, _geoms(out_hw)[(k + 1) % 3], k % 2 == 0) for k, code in enumerate((2, 7, 1, 6, 4))]
    c = [(k, 1, _geoms(out_hw)[k % 3], False) for k in range(5)]  # all 1: back to the instances without orientation
    with _closing(ore.ImageList(gpu_ctx, 5, out_hw, 3)) as (lst,):
        outs = []
        for items in (a, b, c, a):
            _set_oriented(lst, dev, items)
            outs.append(ore.preprocess_list_u8(gpu_ctx, lst))
        torch.cuda.synchronize()
        for items, got in zip((a, b, c, a), outs):
            gh = got.cpu().numpy()
            for i, (src, code, g, flip) in enumerate(items):
                np.testing.assert_array_equal(gh[i], oriented_ref(fn, host[src], code, g[0], g[1], out_hw, flip))


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


def _model_items(n, out_hw, seed):
    """n stored images of their own sizes whose displayed image holds an out_hw window, with mixed codes and flips."""
    h, w = out_hw
    sizes = [(h + 9, w + 20), (h, w), (h // 2 + 1, w + 3), (2 * h, 2 * w), (h + 1, w // 2), (h + 30, w + 30), (h + 2, w + 1)]
    codes = [6, 1, 8, 3, 5, 2, 7]
    geoms = [((h + 4, w + 8), (2, 4)), ((h, w), (0, 0)), ((h, w + 2), (0, 2)), ((h + 2, w), (1, 0)), ((h, w), (0, 0)),
             ((h + 6, w + 6), (6, 6)), ((h + 1, w + 1), (1, 1))]
    flips = [True, False, False, True, True, False, False]
    srcs = []
    for i in range(7):
        hs, ws = sizes[i]
        stored = (ws, hs) if codes[i] in TRANSPOSE else (hs, ws)
        srcs.append(_cuda(images(stored + (3,), seed=seed + i)))
    pick = [i % 7 for i in range(n)]
    return [srcs[i] for i in pick], [codes[i] for i in pick], [geoms[i] for i in pick], [flips[i] for i in pick]


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_model_runs_an_oriented_list(gpu_ctx, precision):
    """run_u8_list on an oriented list is run on preprocess_list_u8 of it, bit for bit, and so are the views."""
    import torch
    import ore
    from ore import squeezenet
    scale, shift = _norm(3)
    with _model(gpu_ctx, squeezenet.build(64), max_batch=8, precision=precision) as m:
        m.set_input_norm(scale, shift)
        srcs, codes, geoms, flips = _model_items(6, (64, 64), seed=1400)
        with _closing(ore.ImageList(gpu_ctx, 6, (64, 64), 3)) as (lst,):
            lst.set_oriented(srcs, codes, geometries=geoms, flips=flips)
            x = ore.preprocess_list_u8(gpu_ctx, lst, scale, shift)
            want = m.run(x)
            got = m.run_u8_list(lst)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
            lst.set(srcs[1:2] * 6)  # the same list without orientations: other rows
            assert not torch.equal(m.run_u8_list(lst), want)
            lst.set_oriented(srcs, codes, geometries=geoms, flips=flips)
            m.set_topk(5)
            m.set_views(2)
            s0, c0 = m.classify(x)
            s1, c1 = m.classify_u8_list(lst)
            torch.cuda.synchronize()
            assert tuple(c1.shape) == (3, 5) and torch.equal(c1, c0) and torch.equal(s1.view(torch.int32), s0.view(torch.int32))


def test_chunked_run_of_an_oriented_list(gpu_ctx):
    """On the pattern of test_image_list_gpu.py::test_chunked_run_u8_list: a list above run_batch goes in chunks, and
    chunk i0 must start at descriptor i0 -- orientation included: the codes cycle with period seven."""
    import torch
    import ore
    from ore import squeezenet
    with _model(gpu_ctx, squeezenet.build(224), max_batch=2048) as m:
        n = m.run_batch + 5
        if ((n + 1) // 2) % 7 == 0:
            n += 1
        assert n <= 2048 and m.run_batch < n <= 2 * m.run_batch
        srcs, codes, geoms, flips = _model_items(n, (224, 224), seed=1500)
        scale, shift = _norm(3)
        m.set_input_norm(scale, shift)
        with _closing(ore.ImageList(gpu_ctx, n, (224, 224), 3)) as (lst,):
            lst.set_oriented(srcs, codes, geometries=geoms, flips=flips)
            want = torch.empty((n, m.output_elems), device="cuda")
            m.run_into(ore.preprocess_list_u8(gpu_ctx, lst, scale, shift), want)
            got = m.run_u8_list(lst)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
            assert not torch.equal(got[0], got[1])


def _own_stream_model(max_batch, n):
    import torch
    import ore
    from ore import squeezenet
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    m = ore.Model(ctx, squeezenet.build(64), max_batch=max_batch)
    lst = ore.ImageList(ctx, n, (64, 64), 3)
    m.set_input_norm(*_norm(3))
    return s, ctx, m, lst


def test_capture_on_a_marked_list_replays_later_orientations():
    import torch
    s, ctx, m, lst = _own_stream_model(4, 4)
    try:
        a = _model_items(4, (64, 64), seed=1600)
        b = tuple(v[::-1] for v in _model_items(4, (64, 64), seed=1700))
        ones = (a[0][1:2] * 4, [1] * 4, None, None)  # all codes 1: a marked capture, nothing oriented in the table
        torch.cuda.synchronize()
        wants = []
        for srcs, codes, geoms, flips in (ones, a, b):
            lst.set_oriented(srcs, codes, geometries=geoms, flips=flips)
            wants.append(m.run_u8_list(lst))  # eager, on the context's stream
        s.synchronize()
        assert not torch.equal(wants[1], wants[2])
        out = torch.empty((4, m.output_elems), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        lst.set_oriented(*ones[:2])
        assert lst.oriented
        m.capture_u8_list(lst, out)  # capture only: nothing runs yet
        for k, (srcs, codes, geoms, flips) in ((0, ones), (1, a), (2, b), (0, ones)):
            lst.set_oriented(srcs, codes, geometries=geoms, flips=flips)
            m.replay()
            s.synchronize()
            assert torch.equal(out, wants[k]), k
    finally:
        s.synchronize()
        lst.close()
        m.close()
        ctx.close()


def test_capture_on_an_unmarked_list_refuses_orientations():
    import torch
    import ore
    s, ctx, m, lst = _own_stream_model(4, 4)
    try:
        srcs, codes, geoms, flips = _model_items(4, (64, 64), seed=1800)
        plain = [x for x, c in zip(srcs, codes) if c not in TRANSPOSE][:1] * 4
        torch.cuda.synchronize()
        lst.set(plain, flips=[False, True, False, True])
        want = m.run_u8_list(lst)
        s.synchronize()
        out = torch.empty((4, m.output_elems), dtype=torch.float32, device="cuda")
        assert not lst.oriented
        m.capture_u8_list(lst, out)
        m.replay()
        s.synchronize()
        assert torch.equal(out, want)
        lst.set_oriented(plain, [1] * 4, flips=[False, True, False, True])  # all 1: the captured kernels still serve it
        m.replay()
        s.synchronize()
        assert torch.equal(out, want)
        lst.set_oriented(srcs, codes, geometries=geoms, flips=flips)
        with pytest.raises(ore.OreError, match="re-capture"):
            m.replay()
        assert ore.load().ore_model_graph_launch(m.h) == 1
        s.synchronize()
        assert torch.equal(out, want)  # nothing ran
        m.capture_u8_list(lst, out)  # the list is marked now: the new graph reads orientations
        m.replay()
        eager = m.run_u8_list(lst)
        s.synchronize()
        assert torch.equal(out, eager)
    finally:
        s.synchronize()
        lst.close()
        m.close()
        ctx.close()
