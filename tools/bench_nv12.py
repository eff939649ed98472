#!/usr/bin/env python3
"""Cost of an NV12 image list against the interleaved list and against a colour-conversion pass in front of it
(DESIGN.md 3.8e): prints one JSON line.  bench_ragged.py's method (medians of --rounds windows of back-to-back
calls timed by HIP events, the variants of one comparison alternating inside a round).
 Two sets of 256 frames, short side to 256 then centre crop 224, each under the plain and the antialiased filter:
   1080 x 1920 (a decoder's 1080p surface) and 375 x 500.
 Each case three ways:
   (a) nv12_list      ore_preprocess_list_u8 on an NV12 list of the frames;
   (b) rgb_list       the same call on the interleaved list of the same frames converted beforehand -- the kernel
                      every earlier measurement was taken on; timed twice a round (rgb_list_again), so the spread
                      of one kernel against itself is in the result beside the difference it is compared with;
   (c) convert_then_rgb_list  what a caller does without (a): an NV12 -> RGB pass on the device, written in torch
                      with the library's integer formula (32 frames at a time), then (b).
 (a)'s output is compared with (b)'s, and (c)'s converted bytes with (b)'s input, before anything is timed.
 Needs an MI355X (no fallback).
usage: python tools/bench_nv12.py [--rounds 9] [--frames 256] [--out FILE]"""
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
BT601 = (16, 1220542, 1673527, 409993, 852492, 2116026)  # include/ore.h


def torch_nv12_to_rgb(y, uv, rgb):
    """y [n, Hs, Ws], uv [n, Hc, Wc, 2] -> rgb [n, Hs, Ws, 3] (all uint8, on the device), CHUNK frames at a time:
    the integer formula of include/ore.h in torch tensor operations."""
    import torch
    yoff, cy, cvr, cug, cvg, cub = BT601
    hs, ws = y.shape[1:]
    for i in range(0, y.shape[0], CHUNK):
        c = uv[i:i + CHUNK].to(torch.int32) - 128
        c = c.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :hs, :ws]
        u, v = c[..., 0], c[..., 1]
        luma = (y[i:i + CHUNK].to(torch.int32) - yoff).clamp_(min=0) * cy + (1 << 19)
        out = rgb[i:i + CHUNK]
        out[..., 0] = ((luma + cvr * v) >> 20).clamp_(0, 255)
        out[..., 1] = ((luma - cug * u - cvg * v) >> 20).clamp_(0, 255)
        out[..., 2] = ((luma + cub * u) >> 20).clamp_(0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_nv12.py: no GPU visible")
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
    y_nv = torch.empty((B, 3, OUT, OUT), dtype=torch.float32, device="cuda")
    y_rgb = torch.empty_like(y_nv)
    d_nv, d_rgb = _desc(y_nv), _desc(y_rgb)
    res = {"tool": "bench_nv12", "rounds": a.rounds, "frames": B, "short": SHORT, "out": [OUT, OUT], "matrix": "bt601", "cases": {}}

    for hs, ws in ((1080, 1920), (375, 500)):
        hc, wc = (hs + 1) // 2, (ws + 1) // 2
        yp = torch.randint(0, 256, (B, hs, ws), dtype=torch.uint8, device="cuda", generator=gen)
        uvp = torch.randint(0, 256, (B, hc, wc, 2), dtype=torch.uint8, device="cuda", generator=gen)
        rgb = torch.empty((B, hs, ws, 3), dtype=torch.uint8, device="cuda")
        torch_nv12_to_rgb(yp, uvp, rgb)
        # the torch pass states the library's formula: frame 0 against the host conversion
        same = bool(np.array_equal(rgb[0].cpu().numpy(), ore.nv12_to_rgb(yp[0].cpu().numpy(), uvp[0].cpu().numpy(), "bt601")))
        scratch = torch.empty_like(rgb)
        (rh, rw), (top, left) = ore.center_crop_geometry((hs, ws), SHORT, (OUT, OUT))
        for antialias in (False, True):
            name = f"{hs}x{ws}_{'aa' if antialias else 'bilinear'}"
            print(f"bench_nv12: {name}", file=sys.stderr, flush=True)
            nv = ore.Nv12ImageList(ctx, B, (OUT, OUT), "bt601", antialias).set([(yp[i], uvp[i]) for i in range(B)], short=SHORT)
            il = ore.ImageList(ctx, B, (OUT, OUT), 3, antialias).set([rgb[i] for i in range(B)], short=SHORT)
            il2 = ore.ImageList(ctx, B, (OUT, OUT), 3, antialias).set([scratch[i] for i in range(B)], short=SHORT)

            def nv12_list():
                check(L.ore_preprocess_list_u8(ctx.h, nv.h, sc_c, sh_c, 0, ctypes.byref(d_nv)), ctx.h)

            def rgb_list():
                check(L.ore_preprocess_list_u8(ctx.h, il.h, sc_c, sh_c, 0, ctypes.byref(d_rgb)), ctx.h)

            def convert_then_rgb_list():
                torch_nv12_to_rgb(yp, uvp, scratch)
                check(L.ore_preprocess_list_u8(ctx.h, il2.h, sc_c, sh_c, 0, ctypes.byref(d_rgb)), ctx.h)

            nv12_list()
            rgb_list()
            torch.cuda.synchronize()
            equal = bool(torch.equal(y_nv, y_rgb))
            reps = 10 if antialias or hs > 1000 else 30
            r = alternate({"nv12_list": (nv12_list, reps), "rgb_list": (rgb_list, reps), "convert_then_rgb_list": (convert_then_rgb_list, 2),
                           "rgb_list_again": (rgb_list, reps)}, a.rounds)
            res["cases"][name] = {
                "resized": [rh, rw], "origin": [top, left], **r,
                "nv12_equals_rgb_list": equal, "torch_pass_equals_host_conversion": same,
                "nv12_source_bytes": int(B * (hs * ws + hc * wc * 2)), "rgb_source_bytes": int(B * hs * ws * 3),
                "nv12_over_rgb_list": round(r["nv12_list"]["us"] / r["rgb_list"]["us"], 4),
                "rgb_list_again_over_rgb_list": round(r["rgb_list_again"]["us"] / r["rgb_list"]["us"], 4),
                "convert_then_rgb_list_over_nv12": round(r["convert_then_rgb_list"]["us"] / r["nv12_list"]["us"], 2)}
            torch.cuda.synchronize()
            for lst in (nv, il, il2):
                lst.close()
        del yp, uvp, rgb, scratch
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
