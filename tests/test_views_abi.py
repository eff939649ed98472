"""CPU: the multi-view entries (ore_image_list_set_ex, ore_image_list_set_nv12_ex, ore_topk_mean_f32,
ore_model_set_views) reject bad arguments before touching a device and the binding lists them; the Python
layer keeps what existing callers rely on (ImageList._descriptors, Model.views at class level,
_check_classify_out over output rows); multi_crop_geometries gives torchvision's FiveCrop / TenCrop order; the
classify entries' group chunking (csrc/ore_chunk.h: group_chunks) through a host dump; and classify_sharded
with views under gloo.  No kernel is launched here."""
import ctypes
import functools
import os
import re
import shutil
import socket
import subprocess
import tempfile

import numpy as np
import pytest
import torch.multiprocessing as mp

import ore
from ore import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "ore.h")
CSRC = os.path.join(os.path.dirname(HERE), "onnx-rusty-inference-engine_amd", "csrc")
INVALID = 1  # ORE_ERR_INVALID
NAMES = ("ore_image_list_set_ex", "ore_image_list_set_nv12_ex", "ore_topk_mean_f32", "ore_model_set_views")


def _tensor(dims, data=0x1000):
    t = _lib.Tensor()
    t.data = data
    t.ndim = len(dims)
    for i, d in enumerate(dims):
        t.dims[i] = d
    return t


def _fails(status):
    assert status == INVALID
    msg = ore.load().ore_last_error(None)
    assert msg  # a message, also without a context
    return msg


def test_names_and_abi_version():
    text = open(HEADER).read()
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", text))
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.ABI_VERSION  # additions only, no ABI bump
    assert int(defs["ORE_MAX_VIEWS"]) == 64 == ore.MAX_VIEWS
    assert re.search(r"#define ORE_IMAGE_FLIP_H 1u", text) and ore.IMAGE_FLIP_H == 1
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)
    assert callable(ore.topk_mean) and callable(ore.multi_crop_geometries)
    assert ctypes.sizeof(_lib.ImageU8) == 64 and ctypes.sizeof(_lib.ImageNv12) == 80  # the descriptors did not grow


def test_null_arguments_are_invalid():
    L = ore.load()
    p = ctypes.c_void_p(0x1000)  # never dereferenced
    x = _tensor((4, 10))
    assert b"null" in _fails(L.ore_image_list_set_ex(None, None, None, 0))
    assert b"null" in _fails(L.ore_image_list_set_nv12_ex(None, None, None, 0))
    assert b"null" in _fails(L.ore_model_set_views(None, 1))
    assert b"null" in _fails(L.ore_model_set_views(None, 0))
    assert b"null" in _fails(L.ore_topk_mean_f32(None, ctypes.byref(x), 2, 1, p, p))  # all in range: the context is missed
    assert b"null" in _fails(L.ore_topk_mean_f32(None, None, 2, 1, p, p))
    for args in ((None, p), (p, None)):
        assert b"null" in _fails(L.ore_topk_mean_f32(None, ctypes.byref(x), 2, 1, *args))
    assert b"null" in _fails(L.ore_topk_mean_f32(None, ctypes.byref(_tensor((4, 10), data=0)), 2, 1, p, p))


def test_topk_mean_ranges_are_checked_before_any_device_call():
    """No context and fake non-null pointers that are never dereferenced: each answer names its argument, so it
    was judged from the arguments alone, before the context or the device was needed."""
    L = ore.load()
    p = ctypes.c_void_p(0x1000)
    x = _tensor((128, 10))
    for views in (0, -1, 65):
        assert b"views" in _fails(L.ore_topk_mean_f32(None, ctypes.byref(x), views, 1, p, p))
    for rows, views in ((5, 2), (7, 3), (64, 10), (1, 2)):
        msg = _fails(L.ore_topk_mean_f32(None, ctypes.byref(_tensor((rows, 10))), views, 1, p, p))
        assert b"views" in msg and b"multiple" in msg
    for k in (0, 11, 65):
        for views in (1, 2, 64):
            assert b"top-k k" in _fails(L.ore_topk_mean_f32(None, ctypes.byref(x), views, k, p, p))
    assert b"null" in _fails(L.ore_topk_mean_f32(None, ctypes.byref(x), 64, 10, p, p))  # the largest of both


def _host_list(cls=None, capacity=4, out_hw=(4, 4)):
    lst = object.__new__(cls or ore.ImageList)
    lst.ctx = type("C", (), {"device": 0, "h": None})()
    lst.capacity, lst.channels, lst.out_hw = capacity, 3, out_hw
    lst.h = None
    lst._images = ()
    return lst


def test_image_list_python_layer_host():
    """_descriptors keeps its signature and its (images, array) result; flips are checked on the host, so a set
    on a list without a handle raises before any library call."""
    import inspect
    for cls in (ore.ImageList, ore.Nv12ImageList):
        names = list(inspect.signature(cls._descriptors).parameters)
        assert len(names) == 5 and names[2:] == ["geometries", "short", "codes"]  # codes: set_oriented's, optional
        assert inspect.signature(cls._descriptors).parameters["codes"].default is None
        assert list(inspect.signature(cls.set).parameters)[2:] == ["geometries", "short", "flips"]
        assert inspect.signature(cls.set).parameters["flips"].default is None
        lst = _host_list(cls)
        images, arr = lst._descriptors([], None, None)
        assert images == [] and len(arr) == 1
        for flips in ([True], [False, True], (1, 0, 1)):
            with pytest.raises(ore.OreError, match=f"{len(flips)} flips for 0 images"):
                lst.set([], flips=flips)
        assert lst._images == ()
    lst = _host_list()
    assert isinstance(lst._descriptors([], None, None)[1], ctypes.Array) and lst._descriptors([], None, None)[1]._type_ is _lib.ImageU8
    import torch
    with pytest.raises(ore.OreError, match="uint8 CUDA"):  # the images' own checks still come first
        lst.set([torch.zeros((4, 4, 3), dtype=torch.uint8)], flips=[True])
    words = ore.engine._flip_words([True, False, 1, 0, "x"], 5)
    assert list(words) == [1, 0, 1, 0, 1]


def test_model_python_layer_host():
    import torch
    m = object.__new__(ore.Model)
    m.ctx = type("C", (), {"device": 0})()
    m.input_dims, m.output_elems, m.max_batch, m.topk = (3, 8, 8), 10, 4, 5
    assert m.views == 1 and "views" not in vars(m) and ore.Model.views == 1
    scores = torch.zeros((2, 5))
    classes = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(ore.OreError, match="scores: expected a float32 CUDA"):
        m._check_classify_out(2, scores, classes)
    with pytest.raises(ore.OreError, match="scores: expected a float32 CUDA"):
        m._check_classify_out(2, scores.double(), classes)
    assert m._subjects(4) == 4
    m.views = 2
    assert m._subjects(4) == 2 and m._subjects(0) == 0
    with pytest.raises(ore.OreError, match="3 images are not a multiple of views = 2"):
        m._subjects(3)


def test_multi_crop_geometries():
    src, short, out = (375, 500), 256, (224, 224)
    resized, centre = ore.center_crop_geometry(src, short, out)
    assert resized == (256, 341) and centre == (16, 58)
    ten = ore.multi_crop_geometries(src, short, out, 10)
    assert len(ten) == 10 and [f for _, _, f in ten] == [False] * 5 + [True] * 5
    assert all(r == resized for r, _, _ in ten)
    assert [o for _, o, _ in ten[:5]] == [(0, 0), (0, 117), (32, 0), (32, 117), centre]  # tl, tr, bl, br, centre
    assert ten[4][:2] == (resized, centre)
    for mirrored, plain in zip((5, 6, 7, 8), (1, 0, 3, 2)):  # the mirrored image's tl is the tr window, flipped
        assert ten[mirrored][:2] == ten[plain][:2]
    assert ten[9][:2] == ten[4][:2]
    assert ore.multi_crop_geometries(src, short, out) == ten[:5] == ore.multi_crop_geometries(src, short, out, 5)
    tall = ore.multi_crop_geometries((500, 375), 256, (224, 200), 5)  # a tall source, a crop that is not square
    assert tall[0][0] == (341, 256) and [o for _, o, _ in tall] == [(0, 0), (0, 56), (117, 0), (117, 56), (58, 28)]
    with pytest.raises(ore.OreError, match="crops"):
        ore.multi_crop_geometries(src, short, out, 4)
    with pytest.raises(ore.OreError, match="larger"):
        ore.multi_crop_geometries((100, 100), 32, (64, 64), 10)


# ------------------------------------------------------------------------------ group chunking
RUN_BATCHES = (1, 7, 256)
VIEWS = (1, 2, 3, 10)


@functools.lru_cache(maxsize=None)
def _dumped():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tempfile.mkdtemp(prefix="views_chunk_"), "views_chunk_dump")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(HERE, "views_chunk_dump.cpp"), "-o", exe], check=True)
    cases = [(rb, v) for rb in RUN_BATCHES for v in VIEWS if v <= rb]
    args = [str(a) for rb, v in cases for a in (rb, v, 3 * rb)]
    txt = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    res = {}
    for line in txt.splitlines():
        f = line.split()
        if f[0] == "case":
            cur = res.setdefault((int(f[1]), int(f[2])), {})
        elif f[0] == "n":
            chunks = []
            cur[int(f[1])] = (int(f[2]), int(f[3]), chunks)
        else:
            chunks.append((int(f[0]), int(f[1])))
    assert sorted(res) == sorted(cases)
    return res


def test_group_chunks_at_one_view_are_todays():
    """views = 1: (nchunks, chunk) of the walker before views existed, for every n up to three run batches"""
    for rb in RUN_BATCHES:
        got = _dumped()[(rb, 1)]
        assert sorted(got) == list(range(1, 3 * rb + 1))
        for n, (nchunks, chunk, chunks) in got.items():
            want_n = -(-n // rb) if n > rb else 1
            assert (nchunks, chunk) == (want_n, -(-n // want_n)), (rb, n)
            assert chunks == [(i0, min(chunk, n - i0)) for i0 in range(0, n, chunk)] and len(chunks) == nchunks, (rb, n)


def test_group_chunks_hold_whole_groups():
    seen_many = 0
    for (rb, v), got in _dumped().items():
        if v == 1:
            continue
        assert sorted(got) == list(range(v, 3 * rb + 1, v))
        for n, (nchunks, chunk, chunks) in got.items():
            G, gb = n // v, rb // v
            assert nchunks == -(-G // gb) == len(chunks) and chunk == -(-G // nchunks) * v, (rb, v, n)
            at = 0
            for i0, nc in chunks:  # [0, n) once and in order, whole groups, a run batch at the most
                assert i0 == at and nc >= v and nc % v == 0 and nc <= rb, (rb, v, n, i0, nc)
                at += nc
            assert at == n, (rb, v, n)
            seen_many += nchunks > 1
    assert seen_many  # the cases reach past one chunk


# ------------------------------------------------------------------------------ classify_sharded(views=)
K = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rows(n, d=17):
    return np.random.default_rng(11).standard_normal((n, d)).astype(np.float32)


def _mean_topk(rows, views, k):
    acc = rows[0::views].copy()
    for v in range(1, views):
        acc = acc + rows[v::views]
    m = acc / np.float32(views)
    idx = np.argsort(-m, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(m, idx, 1), idx.astype(np.int32)


def _worker(rank, world, port, n, views, out_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "onnx-rusty-inference-engine_amd"))
    import torch
    import torch.distributed as dist
    from ore.parallel import classify_sharded
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x = torch.from_numpy(_rows(n))  # the "images" are their own output rows
    sizes = []

    def classify(xs):
        sizes.append(int(xs.shape[0]))
        v, i = _mean_topk(xs.numpy(), views, K) if xs.shape[0] else (np.zeros((0, K), np.float32), np.zeros((0, K), np.int32))
        return torch.from_numpy(v), torch.from_numpy(i)

    scores, classes = classify_sharded(classify, x, views=views)
    assert len(sizes) == 1 and sizes[0] % views == 0  # a whole number of groups on every rank
    assert classes.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(scores.shape) == tuple(classes.shape) == (n // views, K)
    gathered = [None] * world
    dist.all_gather_object(gathered, sizes[0])
    assert sum(gathered) == n
    if rank == 0:
        np.savez(out_path, scores=scores.numpy(), classes=classes.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n", [4, 6])
def test_classify_sharded_views_matches_single_process(tmp_path, n):
    out = str(tmp_path / "y.npz")
    mp.spawn(_worker, args=(2, _free_port(), n, 2, out), nprocs=2, join=True)
    got = np.load(out)
    want_v, want_i = _mean_topk(_rows(n), 2, K)
    assert got["classes"].dtype == np.int32
    np.testing.assert_array_equal(got["classes"], want_i)
    np.testing.assert_array_equal(got["scores"].view(np.uint32), want_v.view(np.uint32))


def test_classify_sharded_rejects_split_groups():
    from ore.parallel import classify_sharded
    import torch
    with pytest.raises(ValueError, match="multiple of views"):
        classify_sharded(lambda xs: None, torch.zeros((5, 3)), views=2)
