#!/usr/bin/env python3
"""Cost of the antialiased resize + crop in front of the graph: prints one JSON line and, with
--out, writes it (profiles/ingest_resize_aa.json).  bench_resize.py's method (medians of --rounds windows of
back-to-back calls timed by HIP events, the variants of one comparison alternating inside a round), at its two
geometries:
   resize256   uint8 [256,375,500,3]  -> 256 x 341, centre crop 224
   hd224       uint8 [64,1080,1920,3] -> short side 224 (224 x 398), centre crop 224
 (a) ore_preprocess_resize_u8_ex, ORE_FILTER_BILINEAR_AA (one thread per output pixel), and the list entry on
     the same images, with their GB/s over the bytes the filter must move: per image the source rows the crop's
     row taps touch, restricted to the byte span of its column taps, plus 4 C H W written; as a fraction of (d);
 (b) ore_preprocess_resize_u8, the plain filter: the floor;
 (c) the framework composition: F.interpolate(x.float(), antialias=True), crop, mul_ / add_;
 (d) a device-to-device copy of the float32 batch (ore_dropout_f32), the machine's own copy rate;
 (e) Model.run_u8_into with the plain and with the antialiased resize, f32 and f16, max_batch = n, autotuned,
     set_streams(2).
Before anything is timed the kernel's output is compared with the list entry's on the same images and with the
model's own conversion: all must be bit-equal.  (The band kernel DESIGN.md 3.8d speaks of was measured with an
earlier form of this tool, which timed both kernels in one round: profiles/ingest_resize_aa_band.json.)
Needs an MI355X (no fallback).
usage: python tools/bench_resize_aa.py [--rounds 9] [--no-model] [--out FILE]"""
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


def geometry(name, rounds, model):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import ore
    from ore import squeezenet
    from ore._lib import FILTER_BILINEAR_AA, Resize, check
    from ore.engine import _desc
    (B, HS, WS, C), short = GEOMETRIES[name]
    (rh, rw), (top, left) = ore.center_crop_geometry((HS, WS), short, (OUT, OUT))
    ctx = ore.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1000)
    x8 = torch.randint(0, 256, (B, HS, WS, C), dtype=torch.uint8, device="cuda", generator=g)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    sc_t, sh_t = (torch.from_numpy(v).cuda().view(1, 3, 1, 1) for v in (scale, shift))

    # the bytes the filter must move
    fy, ny, _, _ = ore.resize_aa_taps(HS, rh, top, OUT)
    fx, nx, _, _ = ore.resize_aa_taps(WS, rw, left, OUT)
    rows = int(fy[-1] + ny[-1] - fy[0])
    span = int(fx[-1] + nx[-1] - fx[0]) * C
    write_b, read_b = B * 4 * C * OUT * OUT, B * rows * span

    y = {k: torch.empty((B, C, OUT, OUT), dtype=torch.float32, device="cuda") for k in ("pixel", "list", "plain", "copy")}
    L = ore.load()
    yd = {k: _desc(v) for k, v in y.items()}
    Fl = ctypes.c_float * 3
    sc_c, sh_c = Fl(*scale.tolist()), Fl(*shift.tolist())
    xp = ctypes.c_void_p(x8.data_ptr())
    geom = Resize(rh, rw, top, left)

    def pixel():
        check(L.ore_preprocess_resize_u8_ex(ctx.h, xp, B, HS, WS, C, ctypes.byref(geom), FILTER_BILINEAR_AA, sc_c, sh_c, 0,
                                            ctypes.byref(yd["pixel"])), ctx.h)

    lst = ore.ImageList(ctx, B, (OUT, OUT), C, antialias=True)
    lst.set([x8[i] for i in range(B)], geometries=[((rh, rw), (top, left))] * B)

    def as_list():
        check(L.ore_preprocess_list_u8(ctx.h, lst.h, sc_c, sh_c, 0, ctypes.byref(yd["list"])), ctx.h)

    def plain():
        check(L.ore_preprocess_resize_u8(ctx.h, xp, B, HS, WS, C, ctypes.byref(geom), sc_c, sh_c, 0, ctypes.byref(yd["plain"])), ctx.h)

    def framework():
        t = F.interpolate(x8.permute(0, 3, 1, 2).float(), size=(rh, rw), mode="bilinear", align_corners=False, antialias=True)
        return t[:, :, top:top + OUT, left:left + OUT].contiguous().mul_(sc_t).add_(sh_t)

    def copy():
        check(L.ore_dropout_f32(ctx.h, ctypes.byref(yd["pixel"]), ctypes.byref(yd["copy"])), ctx.h)

    print(f"bench_resize_aa: {name} kernels", file=sys.stderr, flush=True)
    pixel()
    as_list()
    plain()
    torch.cuda.synchronize()
    kernels_equal = bool(torch.equal(y["pixel"], y["list"]))
    if not kernels_equal:
        sys.exit(f"bench_resize_aa.py: {name}: the dense and the list kernel differ")
    fw_diff = float((framework() - y["pixel"]).abs().max())  # normalised units; the conventions agree to float32 rounding
    plain_diff = float((y["plain"] - y["pixel"]).abs().max())  # what the filter changes
    r = alternate({"pixel": (pixel, 30), "list": (as_list, 30), "plain": (plain, 30), "framework": (framework, 5), "copy": (copy, 30)},
                  rounds)
    c = r["copy"]
    c["gbps_moved"] = round(2 * write_b / c["us"] / 1e3, 1)
    for k in ("pixel", "list"):
        r[k]["gbps"] = round((read_b + write_b) / r[k]["us"] / 1e3, 1)
        r[k]["rate_over_copy_rate"] = round(r[k]["gbps"] / c["gbps_moved"], 3)
    res = {"geometry": name, "shape": [B, HS, WS, C], "resized": [rh, rw], "origin": [top, left], "out": [OUT, OUT],
           "row_taps_max": int(ny.max()), "column_taps_max": int(nx.max()),
           "bytes_written": write_b, "bytes_read": read_b,
           "pixel": r["pixel"], "list": r["list"], "plain_filter": r["plain"], "framework": r["framework"], "copy_d2d": c,
           "kernels_bit_equal": kernels_equal, "framework_max_abs_diff": fw_diff, "plain_filter_max_abs_diff": plain_diff,
           "list_over_pixel": round(r["list"]["us"] / r["pixel"]["us"], 3),
           "pixel_over_plain": round(r["pixel"]["us"] / r["plain"]["us"], 2),
           "framework_over_pixel": round(r["framework"]["us"] / r["pixel"]["us"], 2)}
    torch.cuda.synchronize()
    lst.close()

    if model:
        onnx = squeezenet.build(OUT)
        res["model"] = {}
        for precision in ("f32", "f16"):
            print(f"bench_resize_aa: {name} model {precision}", file=sys.stderr, flush=True)
            m = ore.Model(ctx, onnx, max_batch=B, precision=precision)
            m.set_streams(2)
            m.set_input_norm(scale, shift)
            out_p = torch.empty((B, m.output_elems), device="cuda")
            out_a = torch.empty_like(out_p)
            m.autotune(y["plain"], out_p)

            def run_plain():
                m.set_input_resize((HS, WS), (rh, rw), (top, left))
                m.run_u8_into(x8, out_p)

            def run_aa():
                m.set_input_resize((HS, WS), (rh, rw), (top, left), antialias=True)
                m.run_u8_into(x8, out_a)

            run_aa()
            want = m.run(y["pixel"])
            torch.cuda.synchronize()
            equal = bool(torch.equal(want, out_a))
            if not equal:
                sys.exit(f"bench_resize_aa.py: {name} {precision}: run_u8_into differs from run of the converted batch")
            r = alternate({"run_u8_into_plain": (run_plain, 10), "run_u8_into_aa": (run_aa, 10)}, rounds)
            d = r["run_u8_into_aa"]["us"] - r["run_u8_into_plain"]["us"]
            res["model"][precision] = {"run_u8_into_plain": r["run_u8_into_plain"], "run_u8_into_aa": r["run_u8_into_aa"],
                                       "outputs_equal": equal, "added_us": round(d, 2),
                                       "added_share_of_aa_step": round(d / r["run_u8_into_aa"]["us"], 4),
                                       "img_per_s_plain": round(B / r["run_u8_into_plain"]["us"] * 1e6),
                                       "img_per_s_aa": round(B / r["run_u8_into_aa"]["us"] * 1e6)}
            m.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_resize_aa.py: no GPU visible")
    res = {"tool": "bench_resize_aa", "rounds": a.rounds, "geometries": [geometry(n, a.rounds, not a.no_model) for n in GEOMETRIES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
