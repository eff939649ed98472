"""CPU: the YUV image list entry points (ore_image_check_yuv, ore_image_list_create_yuv, ore_image_list_set_yuv /
_set_yuv_ex) are exported, ore.yuv_planes_to_rgb equals its numpy restatement (tests/_yuv_ref.py) for every format,
and every host check answers ORE_ERR_INVALID with the descriptor's index, the plane and the reason (on the pattern
of tests/test_nv12_abi.py).  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import ore
from ore import _lib

from _nv12_ref import NAMES as MATRICES
from _yuv_ref import FORMATS, NAMES, frame, make_planes, plane_shapes, yuv_planes_to_rgb_ref, yuyv_width

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID
P = 0x1000  # never dereferenced: ore_image_check_yuv is host only

NEW = ["ore_image_check_yuv", "ore_image_list_create_yuv", "ore_image_list_set_yuv", "ore_image_list_set_yuv_ex"]
PLANES = {"nv12": 2, "yuyv": 1, "i444": 3, "i440": 3, "i422": 3, "i420": 3, "i411": 3, "gray": 1}


def test_exports_and_descriptor_size():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", src))
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.load().ore_abi_version() == ore.ABI_VERSION  # added without an ABI bump
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)
    assert ctypes.sizeof(_lib.ImageYuv) == 104
    assert ctypes.sizeof(_lib.ImageNv12) == 80 and ctypes.sizeof(_lib.ImageU8) == 64  # the others are unchanged
    assert re.search(r"\bORE_IMAGE_YUV = 2\b", src) and ore.IMAGE_YUV == 2
    for name, (fid, _, _) in FORMATS.items():
        assert re.search(rf"\bORE_YUV_FMT_{name.upper()} = {fid}\b", src), name
        assert ore.YUV_FORMATS[name] == fid
    assert sorted(ore.YUV_FORMATS) == sorted(NAMES)
    for name in ("YuvImageList", "yuv_planes_to_rgb"):
        assert hasattr(ore, name)
    assert issubclass(ore.YuvImageList, ore.ImageList) and not issubclass(ore.YuvImageList, ore.Nv12ImageList)


# ------------------------------------------------------------------------------------------- the pixel rule
@pytest.mark.parametrize("fmt", NAMES)
@pytest.mark.parametrize("hs,ws", [(1, 1), (2, 2), (3, 5), (6, 4), (5, 9)])
def test_planes_to_rgb_takes_chroma_nearest(fmt, hs, ws):
    """(3, 5) and (5, 9) have a last row and column with a chroma sample of their own.  Across these sizes ws % 4 is
    1, 2 and 0; test_i411_covers_every_width_phase adds 3."""
    planes = make_planes(fmt, hs, ws, seed=hs * 100 + ws)
    w = yuyv_width(fmt, ws)
    for m in MATRICES:
        got = ore.yuv_planes_to_rgb(fmt, planes, m, ws=w)
        assert got.shape == (hs, ws, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, yuv_planes_to_rgb_ref(fmt, planes, m, w))
    # the rule itself at the far corner, by hand
    if fmt not in ("gray", "yuyv"):
        _, sx, sy = FORMATS[fmt]
        r, j = hs - 1, ws - 1
        if fmt == "nv12":
            u, v = planes[1][r >> sy, j >> sx]
        else:
            u, v = planes[1][r >> sy, j >> sx], planes[2][r >> sy, j >> sx]
        assert ore.yuv_planes_to_rgb(fmt, planes, "bt601")[r, j].tolist() == ore.yuv_to_rgb(planes[0][r, j], u, v, "bt601").tolist()


def test_i411_covers_every_width_phase():
    """ws % 4 in {1, 2, 3, 0}: the last chroma sample of a row serves 1, 2, 3 and 4 columns."""
    for ws in (5, 6, 7, 8):
        planes = make_planes("i411", 3, ws, seed=ws)
        assert planes[1].shape == (3, 2)
        np.testing.assert_array_equal(ore.yuv_planes_to_rgb("i411", planes), yuv_planes_to_rgb_ref("i411", planes, "bt601_full"))


def test_nv12_and_planes_agree():
    """An NV12 frame through the general entry is ore.nv12_to_rgb; I420 with the same samples is the same picture."""
    y, uv = make_planes("nv12", 5, 7, seed=3)
    for m in MATRICES:
        want = ore.nv12_to_rgb(y, uv, m)
        np.testing.assert_array_equal(ore.yuv_planes_to_rgb("nv12", [y, uv], m), want)
        np.testing.assert_array_equal(ore.yuv_planes_to_rgb("i420", [y, uv[..., 0], uv[..., 1]], m), want)
    g = make_planes("yuyv", 4, 6, seed=4)[0]
    want = ore.yuv_planes_to_rgb("i422", [g[..., 0::2].reshape(4, 6), g[..., 1], g[..., 3]])
    np.testing.assert_array_equal(ore.yuv_planes_to_rgb("yuyv", [g]), want)


@pytest.mark.parametrize("matrix", MATRICES)
def test_grey_is_grey(matrix):
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    rgb = ore.yuv_planes_to_rgb("gray", [y], matrix)
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 1], rgb[..., 2])
    np.testing.assert_array_equal(rgb, yuv_planes_to_rgb_ref("gray", [y], matrix))
    if matrix == "bt601_full":
        np.testing.assert_array_equal(rgb[..., 0], y)


def test_planes_to_rgb_arguments():
    y, u, v = make_planes("i420", 4, 6, seed=1)
    with pytest.raises(ore.OreError, match="format"):
        ore.yuv_planes_to_rgb("p010", [y, u, v])
    with pytest.raises(ore.OreError, match="3 plane"):
        ore.yuv_planes_to_rgb("i420", [y, u])
    with pytest.raises(ore.OreError, match="plane 2: expected"):
        ore.yuv_planes_to_rgb("i420", [y, u, v[:1]])
    with pytest.raises(ore.OreError, match="uint8"):
        ore.yuv_planes_to_rgb("i420", [y, u.astype(np.int16), v])
    with pytest.raises(ore.OreError, match="matrix"):
        ore.yuv_planes_to_rgb("i420", [y, u, v], "rec2020")
    g = make_planes("yuyv", 3, 6, seed=2)[0]
    assert ore.yuv_planes_to_rgb("yuyv", [g]).shape == (3, 6, 3) and ore.yuv_planes_to_rgb("yuyv", [g], ws=5).shape == (3, 5, 3)
    with pytest.raises(ore.OreError, match="groups"):
        ore.yuv_planes_to_rgb("yuyv", [g], ws=4)
    with pytest.raises(ore.OreError, match="plane 0: expected"):
        ore.yuv_planes_to_rgb("yuyv", [g[..., :2]])


# ------------------------------------------------------------------------------------------- ore_image_check_yuv
def _img(fmt="i420", hs=8, ws=8, stride=(0, 0, 0), g=(8, 8, 0, 0), planes=None, reserved=0):
    d = _lib.ImageYuv()
    fid = FORMATS[fmt][0] if isinstance(fmt, str) else fmt
    used = PLANES.get(fmt, 3) if isinstance(fmt, str) else 3
    planes = [P if k < used else None for k in range(3)] if planes is None else planes
    for k in range(3):
        d.plane[k] = planes[k]
        d.stride[k] = stride[k]
    d.hs, d.ws, d.format, d.reserved = hs, ws, fid, reserved
    d.g = _lib.Resize(*g)
    return d


def _check(imgs, h=4, w=4, n=None, filter=0):
    """ore_image_check_yuv -> (status, bad_index, message); bad_index stays -7 where the library does not set it."""
    arr = (_lib.ImageYuv * max(len(imgs), 1))(*imgs)
    bad = ctypes.c_int64(-7)
    st = ore.load().ore_image_check_yuv(arr, len(imgs) if n is None else n, h, w, filter, ctypes.byref(bad))
    return st, bad.value, ore.load().ore_last_error(None)


def _ok(img, **kw):
    st, bad, msg = _check([img], **kw)
    assert st == 0 and bad == -7, msg


def _bad(img, word, **kw):
    st, bad, msg = _check([img], **kw)
    assert st == INVALID and bad == 0
    assert msg and word in msg and b"image 0" in msg, msg


def _row_bytes(fmt, ws):
    """Bytes of a row of each plane in use, by the header's table."""
    return [int(np.prod(s[1:])) for s in plane_shapes(fmt, 8, ws)]


@pytest.mark.parametrize("fmt", NAMES)
def test_check_accepts(fmt):
    _ok(_img(fmt))
    for ws in (8, 7, 6, 5):  # every width phase
        rb = _row_bytes(fmt, ws) + [0, 0]
        _ok(_img(fmt, 8, ws, tuple(rb[:3]), (8, ws, 0, 0)))  # exactly the row bytes
        _ok(_img(fmt, 7, ws, (0, 0, 0), (7, ws, 0, 0)))
    _ok(_img(fmt, stride=tuple(4096 if k < PLANES[fmt] else 0 for k in range(3))))
    _ok(_img(fmt, stride=tuple(0 if k < PLANES[fmt] else -5 for k in range(3))))  # the stride of an unused plane is not read
    _ok(_img(fmt, 1, 1, g=(4, 4, 0, 0)))
    _ok(_img(fmt, g=(8, 8, 4, 4)))  # the crop at the far corner
    _ok(_img(fmt, 16384, 16384, (0, 0, 0), (16384, 16384, 16380, 16380)))


def test_row_bytes_of_the_header():
    assert _row_bytes("yuyv", 7) == [16] and _row_bytes("nv12", 7) == [7, 8] and _row_bytes("i411", 7) == [7, 2, 2]
    assert _row_bytes("i444", 7) == [7, 7, 7] and _row_bytes("i440", 7) == [7, 7, 7] and _row_bytes("i422", 7) == [7, 4, 4]
    assert _row_bytes("i420", 7) == [7, 4, 4] and _row_bytes("gray", 7) == [7]


@pytest.mark.parametrize("fmt", NAMES)
def test_check_rejects_one_rule_at_a_time(fmt):
    used = PLANES[fmt]
    # every plane in use must be there, every other must not
    for k in range(3):
        planes = [P if j < used else None for j in range(3)]
        planes[k] = None if k < used else P
        _bad(_img(fmt, planes=planes), b"null plane %d" % k if k < used else b"plane %d must be null" % k)
    _bad(_img(fmt, reserved=1), b"reserved")
    _bad(_img(fmt, reserved=-1), b"reserved")
    for kw in (dict(hs=0), dict(ws=0), dict(g=(0, 8, 0, 0)), dict(g=(8, 0, 0, 0)),
               dict(hs=16385), dict(ws=16385), dict(g=(16385, 8, 0, 0)), dict(g=(8, 16385, 0, 0))):
        _bad(_img(fmt, **kw), b"1..16384")
    for g in [(8, 8, 5, 0), (8, 8, 0, 5), (8, 8, -1, 0), (8, 8, 0, -1), (3, 8, 0, 0), (8, 3, 0, 0), (8, 8, 1 << 62, 0)]:
        _bad(_img(fmt, g=g), b"outside")
    for ws in (8, 7):
        rb = _row_bytes(fmt, ws)
        for k in range(used):
            for s in (rb[k] - 1, -rb[k]):
                stride = [0, 0, 0]
                stride[k] = s
                _bad(_img(fmt, 8, ws, tuple(stride), (8, ws, 0, 0)), b"plane %d stride" % k)
            stride = [0, 0, 0]
            stride[k] = 1 << 62
            _bad(_img(fmt, 8, ws, tuple(stride), (8, ws, 0, 0)), b"plane %d: " % k)


def test_check_rejects_unknown_formats_and_lists():
    for fid in (-1, 8, 99):
        _bad(_img(fid), b"format")
    # the output shape is the list's, checked once; so is the filter
    for kw in (dict(h=0), dict(w=0)):
        st, _, msg = _check([_img()], **kw)
        assert st == INVALID and b"image of" in msg
    st, _, msg = _check([_img()], filter=2)
    assert st == INVALID and b"filter" in msg
    # the order of the rules: format, reserved, planes, sizes
    _bad(_img(9, reserved=1, hs=0), b"format")
    _bad(_img("gray", reserved=1, planes=[None, None, None], hs=0), b"reserved")
    _bad(_img("gray", planes=[None, None, None], hs=0), b"null plane 0")


@pytest.mark.parametrize("fmt", NAMES)
def test_check_extent_bounds(fmt):
    """(rows - 1) * stride + row bytes must stay below 2^31 for every plane in use: rejected at 2^31 exactly, accepted
    one byte below; a plane of one row never steps a row."""
    g = (4, 4, 0, 0)
    _, sx, sy = FORMATS[fmt]
    for hs, ws in [(3, 1), (5, 6), (1025, 7)]:
        rb = _row_bytes(fmt, ws)
        for k in range(PLANES[fmt]):
            rows = hs if k == 0 else (hs + (1 << sy) - 1) >> sy
            assert rows > 1
            steps = rows - 1
            stride = ((1 << 31) - 1 - rb[k]) // steps  # the largest with steps * stride + row bytes <= 2^31 - 1
            s = [0, 0, 0]
            s[k] = stride
            _ok(_img(fmt, hs, ws, tuple(s), g))
            if steps == 1:
                assert stride + rb[k] == (1 << 31) - 1  # exactly 2^31 - 1 is accepted, exactly 2^31 is not
            s[k] = stride + 1
            st, bad, msg = _check([_img(fmt, hs, ws, tuple(s), g)])
            assert st == INVALID and bad == 0 and b"2^31" in msg and b"plane %d: " % k in msg, msg
    # planes of one row: any stride; two source rows share one chroma row where sy = 1
    _ok(_img(fmt, 1, 8, (1 << 40,) * PLANES[fmt] + (0,) * (3 - PLANES[fmt]), g))
    if sy == 1:
        s = [8 if fmt != "yuyv" else 16] + [1 << 40] * (PLANES[fmt] - 1) + [0] * (3 - PLANES[fmt])
        _ok(_img(fmt, 2, 8, tuple(s), g))
    _bad(_img(fmt, 2, 8, (1 << 40, 0, 0), g), b"plane 0: ")


def test_check_aa_ratio_rule():
    for fmt in NAMES:
        _ok(_img(fmt, 64, 64, g=(2, 2, 0, 0)), h=2, w=2, filter=1)        # 32 times
        _bad(_img(fmt, 66, 64, g=(2, 2, 0, 0)), b"rows go 66 -> 2", h=2, w=2, filter=1)     # 33 times
        _bad(_img(fmt, 64, 66, g=(2, 2, 0, 0)), b"columns go 66 -> 2", h=2, w=2, filter=1)
        _ok(_img(fmt, 33, 33, g=(1, 1, 0, 0)), h=1, w=1, filter=0)        # the plain filter has no such rule
        _bad(_img(fmt, 33, 33, g=(1, 1, 0, 0)), b"at most 32", h=1, w=1, filter=1)
        _ok(_img(fmt, 32, 32, g=(1, 1, 0, 0)), h=1, w=1, filter=1)


def test_bad_index_and_empty_lists():
    good = _img()
    st, bad, msg = _check([good, _img("gray"), _img("nv12", stride=(0, 3, 0)), good, _img(hs=0)])
    assert st == INVALID and bad == 2 and b"image 2" in msg and b"plane 1 stride" in msg
    st, bad, _ = _check([good, _img("yuyv"), _img("i411")])
    assert st == 0 and bad == -7
    L = ore.load()
    arr = (_lib.ImageYuv * 2)(good, _img(ws=0))
    assert L.ore_image_check_yuv(arr, 2, 4, 4, 0, None) == INVALID  # a null bad_index is allowed
    assert L.ore_image_check_yuv(arr, 1, 4, 4, 0, None) == 0
    assert L.ore_image_check_yuv(None, 0, 4, 4, 0, None) == 0
    assert L.ore_image_check_yuv(None, 1, 4, 4, 0, None) == INVALID and b"null" in L.ore_last_error(None)
    assert L.ore_image_check_yuv(None, -1, 4, 4, 0, None) == INVALID


def test_null_arguments_are_invalid():
    L = ore.load()
    out = ctypes.c_void_p()
    assert L.ore_image_list_create_yuv(None, 4, 4, 4, 0, 2, ctypes.byref(out)) == INVALID and b"null" in L.ore_last_error(None)
    assert not out.value
    arr = (_lib.ImageYuv * 1)(_img())
    assert L.ore_image_list_set_yuv(None, arr, 1) == INVALID and b"null" in L.ore_last_error(None)
    assert L.ore_image_list_set_yuv_ex(None, arr, None, 1) == INVALID and b"null" in L.ore_last_error(None)


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
    """A YuvImageList without a library object behind it: set() must raise before it would need one."""
    lst = object.__new__(ore.YuvImageList)
    lst.ctx = type("C", (), {"device": 0, "h": None})()
    lst.capacity, lst.channels, lst.out_hw, lst.antialias, lst.matrix = capacity, 3, out_hw, False, 2
    lst.h = None
    lst._images = ()
    return lst


def _z(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.uint8)


def test_python_checks_host():
    lst = _host_list()
    y, u, v = _z(9, 12), _z(5, 6), _z(5, 6)
    c = _as_cuda
    with pytest.raises(ore.OreError, match="uint8 CUDA"):
        lst.set([("i420", y, u, v)])  # CPU tensors
    with pytest.raises(ore.OreError, match="plane 1: expected a uint8 CUDA"):
        lst.set([("i420", c(y), c(u.float()), c(v))])
    with pytest.raises(ore.OreError, match="format"):
        lst.set([("i421", c(y), c(u), c(v))])
    with pytest.raises(ore.OreError, match="format"):
        lst.set([c(y)])
    with pytest.raises(ore.OreError, match="3 plane"):
        lst.set([("i420", c(y), c(u))])
    with pytest.raises(ore.OreError, match="1 plane"):
        lst.set([("gray", c(y), c(u))])
    with pytest.raises(ore.OreError, match="not both"):
        lst.set([], geometries=[], short=8)
    with pytest.raises(ore.OreError, match="capacity"):
        lst.set([None] * 5)
    with pytest.raises(ore.OreError, match="geometries"):
        lst.set([("i420", c(y), c(u), c(v))], geometries=[])
    with pytest.raises(ore.OreError, match="cuda:1"):
        lst.set([("i420", c(y, index=1), c(u), c(v))])
    wide = _z(9, 12, 2)
    for fr, word in [(("i420", y[0], u, v), r"\[Hs, Ws\]"),                     # a row, not a plane
                     (("i420", y[:0], u, v), "empty"),
                     (("i420", y, u[:4], v), "plane 1: expected"),               # ceil(9 / 2) = 5 rows
                     (("i420", y, u, v[:, :5]), "plane 2: expected"),
                     (("i444", y, u, v), "plane 1: expected"),                   # full-size chroma
                     (("i411", y, u, v), "plane 1: expected"),                   # 3 samples a row
                     (("i420", y[:, ::2], u[:, :3], v[:, :3]), "plane 0: strides"),   # a column stride of 2
                     (("i420", y, u, _z(6, 5).t()), "plane 2: strides"),
                     (("nv12", y, wide[:5, ::2]), "plane 1: strides"),           # pairs 4 bytes apart
                     (("nv12", y, u), "plane 1: expected"),
                     (("yuyv", y), "plane 0: expected"),
                     (("yuyv", _z(9, 6, 4), 10), "groups"),
                     (("yuyv", _z(9, 6, 8)[:, :, ::2]), "plane 0: strides")]:
        with pytest.raises(ore.OreError, match=word):
            lst.set([tuple([fr[0]] + [c(p) if not isinstance(p, int) else p for p in fr[1:]])])
    # what set() would hand to the library: one frame of every format, then windows of larger frames at legal origins
    hs, ws = 9, 11
    frames, tensors = [], []
    for fmt in NAMES:
        ts = [_z(*s) for s in plane_shapes(fmt, hs, ws)]
        tensors.append(ts)
        frames.append(frame(fmt, [c(t) for t in ts], yuyv_width(fmt, ws)))
    big = _host_list(capacity=8)
    _, arr = big._descriptors(frames, None, None)
    for d, fmt, ts in zip(arr, NAMES, tensors):
        assert d.format == FORMATS[fmt][0] and d.reserved == 0 and (d.hs, d.ws) == (hs, ws)
        assert [d.plane[k] for k in range(3)] == [t.data_ptr() for t in ts] + [None] * (3 - len(ts))
        assert [d.stride[k] for k in range(len(ts))] == [t.stride(0) for t in ts] == _row_bytes(fmt, ws)
        assert (d.g.rh, d.g.rw, d.g.top, d.g.left) == (4, 4, 0, 0)
    assert ore.load().ore_image_check_yuv(arr, len(NAMES), 4, 4, 0, None) == 0
    fy, fu, fv = _z(20, 32), _z(10, 16), _z(10, 16)
    _, arr = lst._descriptors([("i420", c(fy[4:13, 6:17]), c(fu[2:7, 3:9]), c(fv[2:7, 3:9]))], None, None)  # 9 x 11 at (4, 6)
    assert [arr[0].plane[k] for k in range(3)] == [fy.data_ptr() + 4 * 32 + 6, fu.data_ptr() + 2 * 16 + 3, fv.data_ptr() + 2 * 16 + 3]
    assert (arr[0].hs, arr[0].ws, [arr[0].stride[k] for k in range(3)]) == (9, 11, [32, 16, 16])
    fg = _z(20, 16, 4)
    _, arr = lst._descriptors([("yuyv", c(fg[3:12, 3:9]), 11)], None, 5)  # 9 x 11 at row 3, column 6
    assert arr[0].plane[0] == fg.data_ptr() + 3 * 64 + 12 and arr[0].plane[1] is None and (arr[0].hs, arr[0].ws) == (9, 11)
    assert ((arr[0].g.rh, arr[0].g.rw), (arr[0].g.top, arr[0].g.left)) == ore.center_crop_geometry((9, 11), 5, (4, 4))
    assert ore.load().ore_image_check_yuv(arr, 1, 4, 4, 0, None) == 0
    # the model takes it where it takes an ImageList (closed here: the same refusal)
    m = object.__new__(ore.Model)
    m.ctx, m.input_dims, m.max_batch, m.output_elems, m.topk = lst.ctx, (3, 4, 4), 2, 10, 1
    with pytest.raises(ore.OreError, match="ImageList"):
        m.run_u8_list(lst)
    with pytest.raises(ore.OreError, match="matrix"):
        ore.YuvImageList(lst.ctx, 4, (4, 4), matrix="rec2020")
