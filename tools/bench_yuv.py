#!/usr/bin/env python3
"""Cost of a YUV image list of mixed layouts: prints one JSON line.  bench_nv12.py's method (medians
of --rounds windows of back-to-back calls timed by HIP events, the variants of one comparison alternating inside a
round, the reference variant timed twice a round so that its spread against itself stands beside every ratio).
 Short side to 256 then centre crop 224, each case under the plain and the antialiased filter:
   (a) mixed     --frames frames of 375 x 500 in a JPEG-like mix of all eight ore_yuv_format layouts, shuffled:
         yuv_list               ore_preprocess_list_u8 on the YUV list, one launch;
         rgb_list (+ _again)    the same call on the interleaved list of the same frames converted beforehand;
         convert_then_rgb_list  what a caller does without the YUV list: a conversion pass per layout on the device,
                                written in torch with the library's integer formula, then rgb_list.
   (b) generality  the same NV12 frames as ORE_YUV_FMT_NV12 descriptors of a YUV list (yuv_list) against the
         Nv12ImageList (nv12_list, + _again), at 375 x 500 and 1080 x 1920: the price of the general descriptor.
   (c) yuyv      1080 x 1920 YUYV frames (yuyv_list) against NV12 frames of the same pictures (nv12_list, + _again):
         the NV12 frame keeps the chroma of the even rows.
 Before anything is timed, every YUV list's output is compared bit for bit with the interleaved list of the converted
 frames (all frames in (a); the first 8 at 1080 x 1920, where 256 converted frames would be 1.6 GB), and the torch
 pass with the host conversion on one frame per layout.
 Needs an MI355X (no fallback).
usage: python tools/bench_yuv.py [--rounds 9] [--frames 256] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ingest import alternate  # noqa: E402

SHORT, OUT, CHUNK = 256, 224, 32
BT601_FULL = (0, 1048576, 1470104, 360853, 748826, 1858077)  # include/ore.h
SHIFTS = {"nv12": (1, 1), "yuyv": (1, 0), "i444": (0, 0), "i440": (0, 1), "i422": (1, 0), "i420": (1, 1), "i411": (2, 0),
          "gray": (0, 0)}
# of 256 files: what cameras and phones save (4:2:0, 4:2:2) ahead of editors (4:4:4), scanners (grey) and the rest
MIX = {"nv12": 96, "i420": 32, "yuyv": 48, "i422": 16, "i444": 32, "i440": 8, "i411": 8, "gray": 16}


def plane_shapes(fmt, hs, ws):
    sx, sy = SHIFTS[fmt]
    hc, wc = -(-hs // (1 << sy)), -(-ws // (1 << sx))
    return {"yuyv": [(hs, wc, 4)], "nv12": [(hs, ws), (hc, wc, 2)], "gray": [(hs, ws)]}.get(fmt, [(hs, ws), (hc, wc), (hc, wc)])


def yuv_views(fmt, planes, ws):
    """Batched planes [n, ...] of one layout -> (y [n, hs, ws], u, v [n, hc, wc] or None) views."""
    if fmt == "yuyv":
        g = planes[0]
        return g[..., 0::2].reshape(g.shape[0], g.shape[1], -1)[:, :, :ws], g[..., 1], g[..., 3]
    if fmt == "nv12":
        return planes[0], planes[1][..., 0], planes[1][..., 1]
    if fmt == "gray":
        return planes[0], None, None
    return planes


def torch_yuv_to_rgb(fmt, planes, rgb):
    """Batched planes of one layout -> rgb [n, hs, ws, 3] (uint8, on the device), CHUNK frames at a time: nearest
    chroma and the integer formula of include/ore.h under BT.601 full range, in torch tensor operations."""
    import torch
    yoff, cy, cvr, cug, cvg, cub = BT601_FULL
    n, hs, ws = rgb.shape[:3]
    sx, sy = SHIFTS[fmt]
    y, u, v = yuv_views(fmt, planes, ws)
    for i in range(0, n, CHUNK):
        luma = (y[i:i + CHUNK].to(torch.int32) - yoff).clamp_(min=0) * cy + (1 << 19)
        out = rgb[i:i + CHUNK]
        if u is None:
            g = (luma >> 20).clamp_(0, 255)
            out[..., 0], out[..., 1], out[..., 2] = g, g, g
            continue
        up = lambda c: (c[i:i + CHUNK].to(torch.int32) - 128).repeat_interleave(1 << sy, 1).repeat_interleave(1 << sx, 2)[:, :hs, :ws]  # noqa: E731
        uu, vv = up(u), up(v)
        out[..., 0] = ((luma + cvr * vv) >> 20).clamp_(0, 255)
        out[..., 1] = ((luma - cug * uu - cvg * vv) >> 20).clamp_(0, 255)
        out[..., 2] = ((luma + cub * uu) >> 20).clamp_(0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_yuv.py: no GPU visible")
    import ore
    from ore._lib import check
    from ore.engine import _desc
    ctx = ore.Context(0)
    L = ore.load()
    B = a.frames
    gen = torch.Generator(device="cuda").manual_seed(1000)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    Fl = ctypes.c_float * 3
    sc_c, sh_c = Fl(*scale.tolist()), Fl(*shift.tolist())
    y_a = torch.empty((B, 3, OUT, OUT), dtype=torch.float32, device="cuda")
    y_b = torch.empty_like(y_a)
    d_a, d_b = _desc(y_a), _desc(y_b)
    res = {"tool": "bench_yuv", "rounds": a.rounds, "frames": B, "short": SHORT, "out": [OUT, OUT], "matrix": "bt601_full",
           "cases": {}}

    def rand(shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)

    def run(lst, desc):
        check(L.ore_preprocess_list_u8(ctx.h, lst.h, sc_c, sh_c, 0, ctypes.byref(desc)), ctx.h)

    def equal(yl, il, n):
        """The outputs of two lists of n images, all elements."""
        run(yl, _desc(y_a[:n]))
        run(il, _desc(y_b[:n]))
        torch.cuda.synchronize()
        return bool(torch.equal(y_a[:n], y_b[:n]))

    def ratios(r, num, den, again):
        return {f"{num}_over_{den}": round(r[num]["us"] / r[den]["us"], 4), f"{again}_over_{den}": round(r[again]["us"] / r[den]["us"], 4)}

    # ------------------------------------------------------------------ (a) the mixed batch
    hs, ws = 375, 500
    counts = {f: max(1, round(c * B / 256)) for f, c in MIX.items()}
    counts["nv12"] += B - sum(counts.values())
    planes = {f: [rand((n,) + s) for s in plane_shapes(f, hs, ws)] for f, n in counts.items()}
    rgb = {f: torch.empty((n, hs, ws, 3), dtype=torch.uint8, device="cuda") for f, n in counts.items()}
    scratch = {f: torch.empty_like(t) for f, t in rgb.items()}
    same = True
    for f in counts:
        torch_yuv_to_rgb(f, planes[f], rgb[f])
        host = ore.yuv_planes_to_rgb(f, [p[0].cpu().numpy() for p in planes[f]], "bt601_full")
        same = same and bool(np.array_equal(rgb[f][0].cpu().numpy(), host))
    order = [(f, i) for f, n in counts.items() for i in range(n)]
    order = [order[k] for k in np.random.default_rng(0).permutation(len(order))]
    frames = [(f, *[p[i] for p in planes[f]]) for f, i in order]
    src_bytes = int(sum(p.numel() for ps in planes.values() for p in ps))
    for antialias in (False, True):
        name = f"mixed_{hs}x{ws}_{'aa' if antialias else 'bilinear'}"
        print(f"bench_yuv: {name}", file=sys.stderr, flush=True)
        yl = ore.YuvImageList(ctx, B, (OUT, OUT), "bt601_full", antialias).set(frames, short=SHORT)
        il = ore.ImageList(ctx, B, (OUT, OUT), 3, antialias).set([rgb[f][i] for f, i in order], short=SHORT)
        il2 = ore.ImageList(ctx, B, (OUT, OUT), 3, antialias).set([scratch[f][i] for f, i in order], short=SHORT)

        def convert_then_rgb_list():
            for f in counts:
                torch_yuv_to_rgb(f, planes[f], scratch[f])
            run(il2, d_b)

        eq = equal(yl, il, B)
        reps = 10 if antialias else 30
        r = alternate({"yuv_list": (lambda: run(yl, d_a), reps), "rgb_list": (lambda: run(il, d_b), reps),
                       "convert_then_rgb_list": (convert_then_rgb_list, 2), "rgb_list_again": (lambda: run(il, d_b), reps)}, a.rounds)
        res["cases"][name] = {"mix": counts, **r, "yuv_equals_rgb_list": eq, "torch_pass_equals_host_conversion": same,
                              "yuv_source_bytes": src_bytes, "rgb_source_bytes": int(B * hs * ws * 3),
                              **ratios(r, "yuv_list", "rgb_list", "rgb_list_again"),
                              "convert_then_rgb_list_over_yuv": round(r["convert_then_rgb_list"]["us"] / r["yuv_list"]["us"], 2)}
        torch.cuda.synchronize()
        for lst in (yl, il, il2):
            lst.close()
    del planes, rgb, scratch, frames

    # ------------------------------------------------------------------ (b) NV12 both ways, (c) YUYV against NV12
    for hs, ws in ((375, 500), (1080, 1920)):
        hc, wc = (hs + 1) // 2, (ws + 1) // 2
        yp, uvp = rand((B, hs, ws)), rand((B, hc, wc, 2))
        n_eq = B if hs < 1000 else 8
        rgb = torch.empty((n_eq, hs, ws, 3), dtype=torch.uint8, device="cuda")
        torch_yuv_to_rgb("nv12", [yp[:n_eq], uvp[:n_eq]], rgb)
        if hs > 1000:  # the same pictures as YUYV: full-height chroma whose even rows are the NV12 frame's
            gp = rand((B, hs, wc, 4))
            gp[..., 0::2] = yp.reshape(B, hs, wc, 2)
            gp[:, 0::2, :, 1] = uvp[..., 0]
            gp[:, 0::2, :, 3] = uvp[..., 1]
            rgb_g = torch.empty_like(rgb)
            torch_yuv_to_rgb("yuyv", [gp[:n_eq]], rgb_g)
        for antialias in (False, True):
            tag = f"{hs}x{ws}_{'aa' if antialias else 'bilinear'}"
            print(f"bench_yuv: nv12 {tag}", file=sys.stderr, flush=True)
            yl = ore.YuvImageList(ctx, B, (OUT, OUT), "bt601_full", antialias).set([("nv12", yp[i], uvp[i]) for i in range(B)], short=SHORT)
            nv = ore.Nv12ImageList(ctx, B, (OUT, OUT), "bt601_full", antialias).set([(yp[i], uvp[i]) for i in range(B)], short=SHORT)
            il = ore.ImageList(ctx, n_eq, (OUT, OUT), 3, antialias).set([rgb[i] for i in range(n_eq)], short=SHORT)
            run(yl, d_a)
            run(nv, d_b)
            torch.cuda.synchronize()
            eq_nv = bool(torch.equal(y_a, y_b))
            ys = ore.YuvImageList(ctx, n_eq, (OUT, OUT), "bt601_full", antialias).set([("nv12", yp[i], uvp[i]) for i in range(n_eq)], short=SHORT)
            eq = equal(ys, il, n_eq)
            reps = 10 if antialias or hs > 1000 else 30
            r = alternate({"yuv_list": (lambda: run(yl, d_a), reps), "nv12_list": (lambda: run(nv, d_b), reps),
                           "nv12_list_again": (lambda: run(nv, d_b), reps)}, a.rounds)
            res["cases"][f"nv12_{tag}"] = {**r, "yuv_equals_nv12_list": eq_nv, "yuv_equals_rgb_list": eq, "rgb_list_frames": n_eq,
                                           **ratios(r, "yuv_list", "nv12_list", "nv12_list_again")}
            torch.cuda.synchronize()
            ys.close()
            yl.close()
            if hs > 1000:
                print(f"bench_yuv: yuyv {tag}", file=sys.stderr, flush=True)
                yg = ore.YuvImageList(ctx, B, (OUT, OUT), "bt601_full", antialias).set([("yuyv", gp[i]) for i in range(B)], short=SHORT)
                ys = ore.YuvImageList(ctx, n_eq, (OUT, OUT), "bt601_full", antialias).set([("yuyv", gp[i]) for i in range(n_eq)], short=SHORT)
                ig = ore.ImageList(ctx, n_eq, (OUT, OUT), 3, antialias).set([rgb_g[i] for i in range(n_eq)], short=SHORT)
                eq = equal(ys, ig, n_eq)
                r = alternate({"yuyv_list": (lambda: run(yg, d_a), reps), "nv12_list": (lambda: run(nv, d_b), reps),
                               "nv12_list_again": (lambda: run(nv, d_b), reps)}, a.rounds)
                res["cases"][f"yuyv_{tag}"] = {**r, "yuv_equals_rgb_list": eq, "rgb_list_frames": n_eq,
                                               "yuyv_source_bytes": int(gp.numel()), "nv12_source_bytes": int(yp.numel() + uvp.numel()),
                                               **ratios(r, "yuyv_list", "nv12_list", "nv12_list_again")}
                torch.cuda.synchronize()
                for lst in (yg, ys, ig):
                    lst.close()
            nv.close()
            il.close()
        del yp, uvp, rgb
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
