"""The LDS Winograd kernel's workgroup geometry for the tests: builds tests/wino_geom_dump.cpp (a plain host
program around csrc/ore_wino_geom.h, the header the kernel and its launcher share) and parses its output."""
import functools
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "onnx-rusty-inference-engine_amd", "csrc")

WM_TILES, WM_CH = 64, 32

# (N, C, H, W, M) that force, by the grouping rule on a 256-CU device: large groups of >= 2 blocks and single-block
# groups in one launch, a partial last block, tile groups spanning images, an odd plane
# (test_wino_geom.py asserts all of that; test_wino_groups_gpu.py runs them)
GROUPED_CASES = [
    (11000, 16, 5, 7, 40),
    (11000, 16, 5, 7, 72),
]


@functools.lru_cache(maxsize=None)
def _binary():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = os.path.join(tempfile.mkdtemp(prefix="wino_geom_"), "wino_geom_dump")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(HERE, "wino_geom_dump.cpp"), "-o", out],
                   check=True)
    return out


def dump(ncu, cases):
    """cases: (N, H, W, M) tuples -> per case None (outside the kernel's range) or a dict of the WmGroups fields
    and `wgs`, the list of (tile group, mb0, mb1) by blockIdx."""
    args = [str(ncu)] + [str(v) for c in cases for v in c]
    txt = subprocess.run([_binary()] + args, check=True, capture_output=True, text=True).stdout
    res, cur = [], None
    for line in txt.splitlines():
        f = line.split()
        if f[0] == "case":
            ok, ntg, mtiles, mbs, nmg, nsmall, grid = (int(v) for v in f[5:12])
            cur = dict(ntg=ntg, mtiles=mtiles, mbs=mbs, nmg=nmg, nsmall=nsmall, grid=grid, wgs=[]) if ok else None
            res.append(cur)
        else:
            bid, tg, mb0, mb1 = (int(v) for v in f)
            assert bid == len(cur["wgs"])
            cur["wgs"].append((tg, mb0, mb1))
    assert len(res) == len(cases)
    return res


def properties(case, geo):
    """What a GROUPED_CASES shape must exercise, from its geometry."""
    N, C, H, W, M = case
    tpi = ((H + 1) // 2) * ((W + 1) // 2)
    sizes = {b - a for _, a, b in geo["wgs"] if b > a}
    return {
        "large groups of >= 2 blocks": geo["mbs"] >= 2 and geo["mbs"] in sizes,
        "both group sizes in one launch": geo["nsmall"] > 0 and 1 in sizes and len(sizes) >= 2,
        "partial last block": M % WM_CH != 0,
        "a tile group spans two images": WM_TILES % tpi != 0 and N * tpi > WM_TILES,
        "odd plane": H % 2 == 1 or W % 2 == 1,
    }
