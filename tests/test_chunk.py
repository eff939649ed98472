"""The runners' image chunking (csrc/ore_chunk.h: image_chunk, chunk_at) on the host: tests/chunk_dump.cpp, a
plain host program around the header, against the rule restated here.  A batch whose input or output extent
passes the kernels' 32-bit buffer offsets (less 2 MiB of slack) is launched in image chunks that fit: the chunks
tile the batch once and in order, each fits on both sides, nb is 0 exactly when one image alone does not fit and
N when the whole batch does."""
import functools
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "onnx-rusty-inference-engine_amd", "csrc")

LIMIT = 2 ** 31 - 2 ** 21


def extent(n, side):
    """bytes from the first image's start to the end of the n-th: side = (nstride elements, image bytes, es)"""
    nstride, img, es = side
    return (n - 1) * nstride * es + img


def fits(n, x, y):
    return extent(n, x) < LIMIT and extent(n, y) < LIMIT


def rule(N, x, y):
    """the whole batch when it fits, else halved (rounding up) until a chunk does; 0: one image is too large"""
    if not fits(1, x, y):
        return 0
    nb = N
    while nb > 1 and not fits(nb, x, y):
        nb = (nb + 1) // 2
    return nb


def nchw(C, plane, es=4, ps=None, cn=None):
    """C planes of `plane` elements at plane stride ps, inside images of cn channels (a concat slice: cn > C)"""
    ps = ps or plane
    return ((cn or C) * ps, C * ps * es, es)


def nhwc(pixels, C, cs=None):
    """f16 pixels of C channels at pixel stride cs"""
    cs = cs or C
    return (pixels * cs, pixels * cs * 2, 2)


# the Winograd test's conv (test_wino_output_past_2gib: C 64, 27 x 27, M 256; 2.16 GB out at N 2900)
WINO_X, WINO_Y = nchw(64, 27 * 27), nchw(256, 27 * 27)
# the largest batch of it that fits whole
WINO_NMAX = max(n for n in range(2800, 2900) if fits(n, WINO_X, WINO_Y))

CASES = {
    "wino past 2 GiB": (2900, WINO_X, WINO_Y),
    # f32 expand3x3 writing channels 256..511 of a 512-channel concat, padded planes
    "f32 concat slice": (4000, nchw(64, 27 * 27, ps=736), nchw(256, 27 * 27, ps=736, cn=512)),
    # f16 NHWC on both sides, the output a slice of wider pixels
    "f16 nhwc": (9000, nhwc(55 * 55, 64), nhwc(55 * 55, 128, cs=256)),
    # f16 first conv from the f32 NCHW input: 4-byte elements in, 2-byte out
    "f16 from f32 nchw": (4000, nchw(3, 224 * 224), nhwc(109 * 109, 96)),
    # the fused first conv + pool + squeeze: the extent written is the squeeze's (16 planes of 54 x 54)
    "fused squeeze out": (5000, nchw(3, 224 * 224), nchw(16, 54 * 54)),
    "one image": (1, WINO_X, WINO_Y),
    "one image too large": (1, nchw(3, 16384 * 16384), nchw(16, 54 * 54)),
    "too large in a batch": (7, nchw(16, 54 * 54), nchw(64, 4096 * 4096)),
    "whole batch, the last that fits": (WINO_NMAX, WINO_X, WINO_Y),
    "one below": (WINO_NMAX - 1, WINO_X, WINO_Y),
    "one above: two chunks": (WINO_NMAX + 1, WINO_X, WINO_Y),
    "two full chunks": (2 * WINO_NMAX, WINO_X, WINO_Y),
    "one above two full chunks": (2 * WINO_NMAX + 1, WINO_X, WINO_Y),
    # 822 MB images: two fit, three do not
    "a last chunk of one image": (3, nchw(3, 1792 * 1792), nchw(64, 1792 * 1792)),
    "small": (5, WINO_X, WINO_Y),
}


@functools.lru_cache(maxsize=None)
def _dumped():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tempfile.mkdtemp(prefix="chunk_"), "chunk_dump")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(HERE, "chunk_dump.cpp"), "-o", exe], check=True)
    args = [str(v) for N, x, y in CASES.values() for v in (N, *x, *y)]
    txt = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    res = []
    for line in txt.splitlines():
        f = line.split()
        if f[0] == "case":
            res.append((int(f[1]), []))
        else:
            res[-1][1].append((int(f[0]), int(f[1])))
    assert len(res) == len(CASES)
    return dict(zip(CASES, res))


def test_cases_cover_the_rule():
    """the cases are what their names say, by the restated rule"""
    assert WINO_NMAX == 2873 and not fits(WINO_NMAX + 1, WINO_X, WINO_Y)
    assert rule(*CASES["wino past 2 GiB"]) == 1450  # 2.16 GB out: halved once
    assert extent(2900, WINO_Y) > LIMIT > extent(1450, WINO_Y)
    for name in ("f32 concat slice", "f16 nhwc", "f16 from f32 nchw", "fused squeeze out"):
        N, x, y = CASES[name]
        assert 1 < rule(N, x, y) < N, name
    N, x, y = CASES["f32 concat slice"]
    assert x[0] * x[2] == x[1] and y[0] * y[2] > y[1]  # the image stride above the slice's own bytes
    assert rule(*CASES["one image too large"]) == 0 and rule(*CASES["too large in a batch"]) == 0
    assert rule(*CASES["two full chunks"]) == WINO_NMAX
    assert rule(*CASES["one above two full chunks"]) == (WINO_NMAX + 2) // 2  # halved twice: four chunks


def test_chunks():
    for name, (N, x, y) in CASES.items():
        nb, chunks = _dumped()[name]
        assert nb == rule(N, x, y), name
        assert (nb == 0) == (not fits(1, x, y)), name
        if fits(N, x, y):
            assert nb == N, name
        if nb == 0:
            assert chunks == [], name
            continue
        # [0, N) exactly once, in order, nb at a time
        at = 0
        for i0, nc in chunks:
            assert i0 == at and 1 <= nc <= nb, (name, i0, nc)
            assert extent(nc, x) < LIMIT and extent(nc, y) < LIMIT, (name, i0, nc)
            at += nc
        assert at == N, name
        assert all(nc == nb for _, nc in chunks[:-1]), name
        assert len(chunks) == -(-N // nb), name


def test_more_than_one_chunk_past_2gib():
    nb, chunks = _dumped()["wino past 2 GiB"]
    assert nb == 1450 and chunks == [(0, 1450), (1450, 1450)]
    assert _dumped()["a last chunk of one image"] == (2, [(0, 2), (2, 1)])
    nb, chunks = _dumped()["one above: two chunks"]
    assert chunks == [(0, nb), (nb, 2874 - nb)] and nb == 1437
