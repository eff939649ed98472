"""CPU: the NV12 entry points (ore_yuv_to_rgb, ore_image_check_nv12, ore_image_list_*_nv12) are exported, the
colour conversion equals its numpy restatement (tests/_nv12_ref.py) on every (Y, U, V) triple, and every host
check answers ORE_ERR_INVALID with the descriptor's index and the reason (on the pattern of
tests/test_image_list_abi.py).  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import ore
from ore import _lib

from _nv12_ref import NAMES, nv12_to_rgb_ref, yuv_to_rgb_float, yuv_to_rgb_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID
P = 0x1000  # never dereferenced: ore_image_check_nv12 is host only

NEW = ["ore_yuv_to_rgb", "ore_image_check_nv12", "ore_image_list_create_nv12", "ore_image_list_set_nv12",
       "ore_image_list_format", "ore_image_list_matrix"]


def test_exports_and_descriptor_size():
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", open(HEADER).read()))
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.load().ore_abi_version() == ore.ABI_VERSION  # added without an ABI bump
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)
    assert ctypes.sizeof(_lib.ImageNv12) == 80
    src = open(HEADER).read()
    for name, value in (("ORE_YUV_BT601", ore.YUV_BT601), ("ORE_YUV_BT709", ore.YUV_BT709), ("ORE_YUV_BT601_FULL", ore.YUV_BT601_FULL),
                        ("ORE_IMAGE_INTERLEAVED", ore.IMAGE_INTERLEAVED), ("ORE_IMAGE_NV12", ore.IMAGE_NV12)):
        assert re.search(rf"\b{name} = {value}\b", src), name
    assert [_lib.YUV_MATRICES[n] for n in NAMES] == [0, 1, 2]
    for name in ("Nv12ImageList", "yuv_to_rgb", "nv12_to_rgb"):
        assert hasattr(ore, name)
    assert issubclass(ore.Nv12ImageList, ore.ImageList)
    # the handle-less readers, as ore_image_list_count / _filter of a null list
    assert ore.load().ore_image_list_format(None) == 0 and ore.load().ore_image_list_matrix(None) == 0


# ------------------------------------------------------------------------------------------- the conversion
@pytest.mark.parametrize("matrix", NAMES)
def test_every_triple(matrix):
    """All 2^24 triples: the library equals the numpy restatement, every accumulator fits int32 (below 5.8e8), and
    every channel is within 1 of clamp(floor(float64 formula + 0.5)) -- the coefficient rounding moves a value by
    less than 2e-4, so the two can differ only next to a tie."""
    u, v = (a.astype(np.uint8).ravel() for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    peak, worst = 0, 0
    for y0 in range(0, 256, 16):  # 2^20 triples at a time
        yy = np.repeat(np.arange(y0, y0 + 16, dtype=np.uint8), u.size)
        uu, vv = np.tile(u, 16), np.tile(v, 16)
        got = ore.yuv_to_rgb(yy, uu, vv, matrix)
        want, acc = yuv_to_rgb_ref(yy, uu, vv, matrix)
        assert got.shape == (yy.size, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, want)
        peak = max(peak, acc)
        worst = max(worst, int(np.abs(got.astype(np.int64) - yuv_to_rgb_float(yy, uu, vv, matrix)).max()))
    print(f"{matrix}: largest accumulator {peak}, largest distance to the float64 formula {worst}")
    assert peak < 5.8e8
    assert worst <= 1


def test_spot_values_and_arguments():
    one = lambda y, u, v, m: ore.yuv_to_rgb(np.uint8([y]), np.uint8([u]), np.uint8([v]), m)[0].tolist()  # noqa: E731
    for m in ("bt601", "bt709"):
        assert one(16, 128, 128, m) == [0, 0, 0] and one(235, 128, 128, m) == [255, 255, 255]
        assert one(0, 128, 128, m) == [0, 0, 0] and one(255, 128, 128, m) == [255, 255, 255]  # outside the range: clamped
    assert one(0, 128, 128, "bt601_full") == [0, 0, 0] and one(255, 128, 128, "bt601_full") == [255, 255, 255]
    assert one(128, 128, 128, "bt601_full") == [128, 128, 128]
    # the id and the name are one matrix; shapes are kept
    y = np.arange(24, dtype=np.uint8).reshape(2, 3, 4) * 10
    assert np.array_equal(ore.yuv_to_rgb(y, y[::-1], y, "bt709"), ore.yuv_to_rgb(y, y[::-1], y, ore.YUV_BT709))
    assert ore.yuv_to_rgb(y, y, y).shape == (2, 3, 4, 3)
    L = ore.load()
    b = (ctypes.c_uint8 * 3)(1, 2, 3)
    for bad in (-1, 3, 99):
        assert L.ore_yuv_to_rgb(bad, b, b, b, 1, b) == INVALID and b"matrix" in L.ore_last_error(None)
    with pytest.raises(ore.OreError, match="matrix"):
        ore.yuv_to_rgb(y, y, y, "bt2020")
    with pytest.raises(ore.OreError, match="matrix"):
        ore.yuv_to_rgb(y, y, y, 7)
    assert L.ore_yuv_to_rgb(0, None, b, b, 1, b) == INVALID and b"null" in L.ore_last_error(None)
    assert L.ore_yuv_to_rgb(0, b, b, b, -1, b) == INVALID
    assert L.ore_yuv_to_rgb(0, None, None, None, 0, None) == 0
    with pytest.raises(ore.OreError, match="uint8"):
        ore.yuv_to_rgb(y.astype(np.int32), y, y)
    with pytest.raises(ore.OreError, match="differ"):
        ore.yuv_to_rgb(y, y[:1], y)


@pytest.mark.parametrize("hs,ws", [(1, 1), (2, 2), (3, 5), (6, 4)])
def test_nv12_to_rgb_takes_chroma_nearest(hs, ws):
    rng = np.random.default_rng(hs * 10 + ws)
    y = rng.integers(0, 256, (hs, ws), dtype=np.uint8)
    uv = rng.integers(0, 256, ((hs + 1) // 2, (ws + 1) // 2, 2), dtype=np.uint8)
    for m in NAMES:
        got = ore.nv12_to_rgb(y, uv, m)
        assert got.shape == (hs, ws, 3)
        np.testing.assert_array_equal(got, nv12_to_rgb_ref(y, uv, m))
    r, j = hs - 1, ws - 1  # the last row and column of an odd frame have a pair of their own
    assert ore.nv12_to_rgb(y, uv)[r, j].tolist() == ore.yuv_to_rgb(y[r, j], uv[r >> 1, j >> 1, 0], uv[r >> 1, j >> 1, 1]).tolist()
    with pytest.raises(ore.OreError, match="uv_plane"):
        ore.nv12_to_rgb(y, uv[:, :, :1])
    with pytest.raises(ore.OreError, match="y_plane"):
        ore.nv12_to_rgb(y[0], uv)


# ------------------------------------------------------------------------------------------- ore_image_check_nv12
def _img(hs=8, ws=8, y_stride=0, uv_stride=0, g=(8, 8, 0, 0), y=P, uv=P):
    d = _lib.ImageNv12()
    d.y, d.uv = y, uv
    d.hs, d.ws, d.y_stride, d.uv_stride = hs, ws, y_stride, uv_stride
    d.g = _lib.Resize(*g)
    return d


def _check(imgs, h=4, w=4, n=None, filter=0):
    """ore_image_check_nv12 -> (status, bad_index, message); bad_index stays -7 where the library does not set it."""
    arr = (_lib.ImageNv12 * max(len(imgs), 1))(*imgs)
    bad = ctypes.c_int64(-7)
    st = ore.load().ore_image_check_nv12(arr, len(imgs) if n is None else n, h, w, filter, ctypes.byref(bad))
    return st, bad.value, ore.load().ore_last_error(None)


def _ok(img, **kw):
    st, bad, msg = _check([img], **kw)
    assert st == 0 and bad == -7, msg


def _bad(img, word, **kw):
    st, bad, msg = _check([img], **kw)
    assert st == INVALID and bad == 0
    assert msg and word in msg and b"image 0" in msg, msg


def test_check_accepts():
    _ok(_img())
    _ok(_img(y_stride=0, uv_stride=0))        # dense, stated as 0
    _ok(_img(y_stride=8, uv_stride=8))        # exactly ws and 2 * ceil(ws / 2)
    _ok(_img(y_stride=4096, uv_stride=2048))
    _ok(_img(7, 8, g=(7, 8, 0, 0)))           # an odd height
    _ok(_img(8, 7, g=(8, 7, 0, 0)))           # an odd width: 4 pairs, 8 bytes a UV row
    _ok(_img(8, 7, 7, 8, (8, 7, 0, 0)))
    _ok(_img(1, 1, g=(4, 4, 0, 0)))
    _ok(_img(g=(8, 8, 4, 4)))                 # the crop at the far corner
    _ok(_img(16384, 16384, 0, 0, (16384, 16384, 16380, 16380)))


def test_check_rejects_one_rule_at_a_time():
    _bad(_img(y=None), b"null y")
    _bad(_img(uv=None), b"null uv")
    for kw in (dict(hs=0), dict(ws=0), dict(g=(0, 8, 0, 0)), dict(g=(8, 0, 0, 0)),
               dict(hs=16385), dict(ws=16385), dict(g=(16385, 8, 0, 0)), dict(g=(8, 16385, 0, 0))):
        _bad(_img(**kw), b"1..16384")
    for g in [(8, 8, 5, 0), (8, 8, 0, 5), (8, 8, -1, 0), (8, 8, 0, -1), (3, 8, 0, 0), (8, 3, 0, 0), (8, 8, 1 << 62, 0)]:
        _bad(_img(g=g), b"outside")
    _bad(_img(y_stride=7), b"y stride")
    _bad(_img(y_stride=-8), b"y stride")
    _bad(_img(uv_stride=7), b"uv stride")
    _bad(_img(8, 7, 7, 7, (8, 7, 0, 0)), b"uv stride")  # an odd width still needs 2 * ceil(7 / 2) = 8 bytes
    _bad(_img(uv_stride=-8), b"uv stride")
    _bad(_img(y_stride=1 << 62), b"y rows")
    _bad(_img(uv_stride=1 << 62), b"uv rows")
    # the output shape is the list's, checked once; so is the filter
    for kw in (dict(h=0), dict(w=0)):
        st, _, msg = _check([_img()], **kw)
        assert st == INVALID and b"image of" in msg
    st, _, msg = _check([_img()], filter=2)
    assert st == INVALID and b"filter" in msg


def test_check_extent_bounds():
    """(hs-1)*y_stride + ws and (ceil(hs/2)-1)*uv_stride + 2*ceil(ws/2) must stay below 2^31: rejected at 2^31
    exactly, accepted one byte below."""
    g = (4, 4, 0, 0)
    _bad(_img(2, 1, (1 << 31) - 1, 0, g), b"2^31")
    _ok(_img(2, 1, (1 << 31) - 2, 0, g))
    # three rows are two UV rows: one UV row step of 2^31 - 2 bytes plus the two bytes of a pair
    _bad(_img(3, 1, 0, (1 << 31) - 2, g), b"2^31")
    _ok(_img(3, 1, 0, (1 << 31) - 3, g))
    for hs, ws in [(16384, 16384), (1025, 7), (4, 6)]:
        rows, tail = (hs + 1) // 2 - 1, 2 * ((ws + 1) // 2)
        stride = ((1 << 31) - tail) // rows  # the largest with rows * stride + tail <= 2^31
        if rows * stride + tail == 1 << 31:
            _bad(_img(hs, ws, 0, stride, g), b"uv rows")
            _ok(_img(hs, ws, 0, stride - 1, g))
        else:
            _ok(_img(hs, ws, 0, stride, g))
            _bad(_img(hs, ws, 0, stride + 1, g), b"uv rows")
    # planes of one row never step a row: two source rows share one UV row
    _ok(_img(1, 8, 1 << 40, 1 << 40, g))
    _ok(_img(2, 8, 8, 1 << 40, g))
    _bad(_img(2, 8, 1 << 40, 8, g), b"y rows")


def test_check_aa_ratio_rule():
    _ok(_img(64, 64, g=(2, 2, 0, 0)), h=2, w=2, filter=1)        # 32 times
    _bad(_img(66, 64, g=(2, 2, 0, 0)), b"rows go 66 -> 2", h=2, w=2, filter=1)     # 33 times
    _bad(_img(64, 66, g=(2, 2, 0, 0)), b"columns go 66 -> 2", h=2, w=2, filter=1)
    _ok(_img(33, 33, g=(1, 1, 0, 0)), h=1, w=1, filter=0)        # the plain filter has no such rule
    _bad(_img(33, 33, g=(1, 1, 0, 0)), b"at most 32", h=1, w=1, filter=1)
    _ok(_img(32, 32, g=(1, 1, 0, 0)), h=1, w=1, filter=1)


def test_bad_index_and_empty_lists():
    good = _img()
    st, bad, msg = _check([good, good, _img(uv_stride=3), good, _img(hs=0)])
    assert st == INVALID and bad == 2 and b"image 2" in msg and b"uv stride" in msg
    st, bad, _ = _check([good, good, good])
    assert st == 0 and bad == -7
    L = ore.load()
    arr = (_lib.ImageNv12 * 2)(good, _img(ws=0))
    assert L.ore_image_check_nv12(arr, 2, 4, 4, 0, None) == INVALID  # a null bad_index is allowed
    assert L.ore_image_check_nv12(arr, 1, 4, 4, 0, None) == 0
    assert L.ore_image_check_nv12(None, 0, 4, 4, 0, None) == 0
    assert L.ore_image_check_nv12(None, 1, 4, 4, 0, None) == INVALID and b"null" in L.ore_last_error(None)
    assert L.ore_image_check_nv12(None, -1, 4, 4, 0, None) == INVALID


def test_null_arguments_are_invalid():
    L = ore.load()
    out = ctypes.c_void_p()
    assert L.ore_image_list_create_nv12(None, 4, 4, 4, 0, 0, ctypes.byref(out)) == INVALID and b"null" in L.ore_last_error(None)
    assert not out.value
    assert L.ore_image_list_set_nv12(None, (_lib.ImageNv12 * 1)(_img()), 1) == INVALID and b"null" in L.ore_last_error(None)


# ------------------------------------------------------------------------------------------- Python's own checks
def _as_cuda(x, index=0):
    """A CPU tensor that reports itself as a CUDA tensor on cuda:<index> (as in tests/test_image_list_abi.py): the
    host checks read its dtype, shape and strides, never its bytes."""
    import torch

    class AsCuda(torch.Tensor):
        is_cuda = True
        device = type("D", (), {"index": index})()

    return x.as_subclass(AsCuda)


def _host_list(capacity=4, out_hw=(4, 4)):
    """An Nv12ImageList without a library object behind it: set() must raise before it would need one."""
    lst = object.__new__(ore.Nv12ImageList)
    lst.ctx = type("C", (), {"device": 0, "h": None})()
    lst.capacity, lst.channels, lst.out_hw, lst.antialias, lst.matrix = capacity, 3, out_hw, False, 0
    lst.h = None
    lst._images = ()
    return lst


def test_python_checks_host():
    import torch
    lst = _host_list()
    y, uv = torch.zeros((9, 12), dtype=torch.uint8), torch.zeros((5, 6, 2), dtype=torch.uint8)
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        lst.set([(y, uv)])  # CPU tensors
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        lst.set([(_as_cuda(y), _as_cuda(uv.float()))])
    with pytest.raises(ore.OreError, match="pair"):
        lst.set([_as_cuda(y)])
    with pytest.raises(ore.OreError, match="not both"):
        lst.set([], geometries=[], short=8)
    with pytest.raises(ore.OreError, match="capacity"):
        lst.set([None] * 5)
    with pytest.raises(ore.OreError, match="geometries"):
        lst.set([(_as_cuda(y), _as_cuda(uv))], geometries=[])
    with pytest.raises(ore.OreError, match="cuda:1"):
        lst.set([(_as_cuda(y, index=1), _as_cuda(uv))])
    wide = torch.zeros((9, 12, 2), dtype=torch.uint8)
    for by, buv, word in [(y[0], uv, r"\[Hs, Ws\]"),                  # a row, not a plane
                          (y[:0], uv, "empty"),
                          (y, uv[:4], "uv: expected"),               # ceil(9 / 2) = 5 rows
                          (y, uv[:, :5], "uv: expected"),
                          (y[:, ::2], uv[:, :3], "y: strides"),      # a column stride of 2
                          (y.t()[:9, :9], torch.zeros((5, 5, 2), dtype=torch.uint8), "y: strides"),
                          (y, wide[:5, ::2], "uv: strides")]:        # pairs 4 bytes apart
        with pytest.raises(ore.OreError, match=word):
            lst.set([(_as_cuda(by), _as_cuda(buv))])
    # what set() would hand to the library: windows of a larger frame at an even origin
    fy, fuv = torch.zeros((20, 32), dtype=torch.uint8), torch.zeros((10, 16, 2), dtype=torch.uint8)
    wy, wuv = fy[4:13, 6:17], fuv[2:7, 3:9]  # 9 x 11 at (4, 6): 5 x 6 pairs at (2, 3)
    _, arr = lst._descriptors([(_as_cuda(fy), _as_cuda(fuv)), (_as_cuda(wy), _as_cuda(wuv))], None, None)
    assert (arr[0].y, arr[0].uv, arr[0].hs, arr[0].ws, arr[0].y_stride, arr[0].uv_stride) == (fy.data_ptr(), fuv.data_ptr(), 20, 32, 32, 32)
    assert (arr[1].y, arr[1].uv) == (fy.data_ptr() + 4 * 32 + 6, fuv.data_ptr() + 2 * 32 + 6)
    assert (arr[1].hs, arr[1].ws, arr[1].y_stride, arr[1].uv_stride) == (9, 11, 32, 32)
    assert [(d.g.rh, d.g.rw, d.g.top, d.g.left) for d in arr] == [(4, 4, 0, 0)] * 2
    _, arr = lst._descriptors([(_as_cuda(fy), _as_cuda(fuv))], None, 5)
    assert ((arr[0].g.rh, arr[0].g.rw), (arr[0].g.top, arr[0].g.left)) == ore.center_crop_geometry((20, 32), 5, (4, 4))
    assert ore.load().ore_image_check_nv12(arr, 1, 4, 4, 0, None) == 0
    # the model takes it where it takes an ImageList (closed here: the same refusal)
    m = object.__new__(ore.Model)
    m.ctx, m.input_dims, m.max_batch, m.output_elems, m.topk = lst.ctx, (3, 4, 4), 2, 10, 1
    with pytest.raises(ore.OreError, match="ImageList"):
        m.run_u8_list(lst)
    with pytest.raises(ore.OreError, match="matrix"):
        ore.Nv12ImageList(lst.ctx, 4, (4, 4), matrix="rec2020")
