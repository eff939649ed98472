#!/usr/bin/env python3
"""Cost of the cubic resize filters in front of the graph beside the two bilinear ones: prints one
JSON line and, with --out, writes it (profiles/ingest_resize_cubic.json).  bench_resize.py's method (medians of
--rounds windows of back-to-back calls timed by HIP events, the variants of one comparison alternating inside a
round), at its two geometries and over two lists:
   resize256   uint8 [256,375,500,3]  -> 256 x 341, centre crop 224
   hd224       uint8 [64,1080,1920,3] -> short side 224 (224 x 398), centre crop 224
   list256     the 256 images of resize256 as an image list
   nv12_hd     64 NV12 frames of 1080 x 1920 as an NV12 list, hd224's geometry
 (a) ore_preprocess_resize_u8_ex / ore_preprocess_list_u8 under each filter of --filters (bilinear = 0, aa = 1,
     cubic = 256, cubic_aa = 257);
 (b) the framework composition on the dense tensors: F.interpolate(x.float(), mode="bicubic", antialias=False / True),
     crop, mul_ / add_.
Before anything is timed each cubic result is compared with the framework's (they agree to float32 rounding), and the
list entry with the dense one on the same images (bit-equal).  --filters bilinear,aa runs on a library without the
cubic filters: the parent's numbers for the two filters whose code did not change.
Needs an MI355X (no fallback).
usage: python tools/bench_resize_cubic.py [--rounds 9] [--filters bilinear,aa,cubic,cubic_aa] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ingest import alternate  # noqa: E402
from bench_resize import GEOMETRIES, OUT  # noqa: E402

FILTERS = {"bilinear": 0, "aa": 1, "cubic": 256, "cubic_aa": 257}


def _list_kw(name):
    """Keywords of the list constructors; `cubic` only where it is needed, so that the bilinear filters also run
    against a binding that has no such keyword."""
    kw = {"antialias": bool(FILTERS[name] & 1)}
    if FILTERS[name] & 256:
        kw["cubic"] = True
    return kw


def _norm():
    import numpy as np
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    return (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)


def geometry(name, rounds, filters, with_list):
    import torch
    import torch.nn.functional as F
    import ore
    from ore._lib import Resize, check
    from ore.engine import _desc
    (B, HS, WS, C), short = GEOMETRIES[name]
    (rh, rw), (top, left) = ore.center_crop_geometry((HS, WS), short, (OUT, OUT))
    ctx = ore.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1000)
    x8 = torch.randint(0, 256, (B, HS, WS, C), dtype=torch.uint8, device="cuda", generator=g)
    scale, shift = _norm()
    sc_t, sh_t = (torch.from_numpy(v).cuda().view(1, 3, 1, 1) for v in (scale, shift))
    L = ore.load()
    Fl = ctypes.c_float * 3
    sc_c, sh_c = Fl(*scale.tolist()), Fl(*shift.tolist())
    xp = ctypes.c_void_p(x8.data_ptr())
    geom = Resize(rh, rw, top, left)
    y = {f: torch.empty((B, C, OUT, OUT), dtype=torch.float32, device="cuda") for f in filters}
    yd = {f: _desc(v) for f, v in y.items()}

    def dense(f):
        def run():
            check(L.ore_preprocess_resize_u8_ex(ctx.h, xp, B, HS, WS, C, ctypes.byref(geom), FILTERS[f], sc_c, sh_c, 0,
                                                ctypes.byref(yd[f])), ctx.h)
        return run

    def framework(aa):
        def run():
            t = F.interpolate(x8.permute(0, 3, 1, 2).float(), size=(rh, rw), mode="bicubic", align_corners=False, antialias=aa)
            return t[:, :, top:top + OUT, left:left + OUT].contiguous().mul_(sc_t).add_(sh_t)
        return run

    print(f"bench_resize_cubic: {name} dense", file=sys.stderr, flush=True)
    variants = {f: (dense(f), 30) for f in filters}
    variants["framework_bicubic"] = (framework(False), 5)
    variants["framework_bicubic_aa"] = (framework(True), 5)
    res = {"geometry": name, "shape": [B, HS, WS, C], "resized": [rh, rw], "origin": [top, left], "out": [OUT, OUT]}
    for f in filters:
        variants[f][0]()
    torch.cuda.synchronize()
    for f, aa in (("cubic", False), ("cubic_aa", True)):
        if f in filters:  # normalised units; the conventions agree to float32 rounding
            res[f"framework_max_abs_diff_{f}"] = float((framework(aa)() - y[f]).abs().max())
    res["dense"] = alternate(variants, rounds)
    for f, fw in (("cubic", "framework_bicubic"), ("cubic_aa", "framework_bicubic_aa")):
        if f in filters:
            res[f"framework_over_{f}"] = round(res["dense"][fw]["us"] / res["dense"][f]["us"], 2)

    if with_list:
        print(f"bench_resize_cubic: {name} list", file=sys.stderr, flush=True)
        lists, yl = {}, {}
        for f in filters:
            lists[f] = ore.ImageList(ctx, B, (OUT, OUT), C, **_list_kw(f))
            lists[f].set([x8[i] for i in range(B)], geometries=[((rh, rw), (top, left))] * B)
            yl[f] = torch.empty_like(y[f])

        def as_list(f):
            d = _desc(yl[f])

            def run():
                check(L.ore_preprocess_list_u8(ctx.h, lists[f].h, sc_c, sh_c, 0, ctypes.byref(d)), ctx.h)
            return run

        variants = {f: (as_list(f), 30) for f in filters}
        for f in filters:
            variants[f][0]()
        torch.cuda.synchronize()
        for f in filters:
            if not torch.equal(yl[f], y[f]):
                sys.exit(f"bench_resize_cubic.py: {name}: the list and the dense kernel differ under {f}")
        res["list"] = alternate(variants, rounds)
        res["list_bit_equal_dense"] = True
        torch.cuda.synchronize()
        for lst in lists.values():
            lst.close()
    ctx.close()
    return res


def nv12(rounds, filters):
    """64 NV12 frames of 1080 x 1920 under hd224's geometry."""
    import torch
    import ore
    from ore._lib import check
    from ore.engine import _desc
    B, HS, WS = 64, 1080, 1920
    (rh, rw), (top, left) = ore.center_crop_geometry((HS, WS), 224, (OUT, OUT))
    ctx = ore.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1001)
    yp = torch.randint(0, 256, (B, HS, WS), dtype=torch.uint8, device="cuda", generator=g)
    uvp = torch.randint(0, 256, (B, HS // 2, WS // 2, 2), dtype=torch.uint8, device="cuda", generator=g)
    scale, shift = _norm()
    L = ore.load()
    Fl = ctypes.c_float * 3
    sc_c, sh_c = Fl(*scale.tolist()), Fl(*shift.tolist())
    print("bench_resize_cubic: nv12_hd list", file=sys.stderr, flush=True)
    lists, out = {}, {}
    for f in filters:
        lists[f] = ore.Nv12ImageList(ctx, B, (OUT, OUT), "bt601", **_list_kw(f))
        lists[f].set([(yp[i], uvp[i]) for i in range(B)], geometries=[((rh, rw), (top, left))] * B)
        out[f] = torch.empty((B, 3, OUT, OUT), dtype=torch.float32, device="cuda")

    def as_list(f):
        d = _desc(out[f])

        def run():
            check(L.ore_preprocess_list_u8(ctx.h, lists[f].h, sc_c, sh_c, 0, ctypes.byref(d)), ctx.h)
        return run

    res = {"geometry": "nv12_hd", "frames": [B, HS, WS], "resized": [rh, rw], "origin": [top, left], "out": [OUT, OUT],
           "list": alternate({f: (as_list(f), 30) for f in filters}, rounds)}
    torch.cuda.synchronize()
    for lst in lists.values():
        lst.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--filters", default=",".join(FILTERS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    filters = [f for f in a.filters.split(",") if f]
    if not filters or any(f not in FILTERS for f in filters):
        sys.exit(f"bench_resize_cubic.py: --filters takes a comma-separated subset of {', '.join(FILTERS)}")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_resize_cubic.py: no GPU visible")
    res = {"tool": "bench_resize_cubic", "rounds": a.rounds, "filters": filters,
           "geometries": [geometry(n, a.rounds, filters, n == "resize256") for n in GEOMETRIES] + [nv12(a.rounds, filters)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
