#!/usr/bin/env python3
"""Cost of resize + crop in front of the graph: prints one JSON line.  bench_ingest.py's
method (medians of --rounds windows of back-to-back calls timed by HIP events, the variants of one
comparison alternating inside a round), at two geometries:
   resize256   uint8 [256,375,500,3]  -> 256 x 341, centre crop 224
   hd224       uint8 [64,1080,1920,3] -> short side 224 (224 x 398), centre crop 224
 (a) ore_preprocess_resize_u8, and its GB/s over the bytes it must move: per image the source rows its taps
     touch, restricted to the columns' byte span, plus 4 C H W written; also over the whole touched rectangle
     (the bounding rows, skipped ones included); both as a fraction of (e);
 (b) the framework composition a caller would write: F.interpolate of the float tensor, crop, mul_ / add_;
 (c) ore_preprocess_u8 at [n,224,224,3]: the floor (no resize, the same output);
 (d) Model.run_u8_into with the resize (source images) against without (224 x 224 images), f32 and f16,
     max_batch = n, autotuned, set_streams(2);
 (e) a device-to-device copy of the float32 batch (ore_dropout_f32), the machine's own copy rate.
(The LDS-staged second kernel DESIGN.md 3.8b speaks of was measured with an earlier form of this tool, which
timed both kernels in one round: profiles/ingest_resize_staged.json.)
Needs an MI355X (no fallback).
usage: python tools/bench_resize.py [--rounds 9] [--no-model] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ingest import alternate  # noqa: E402

GEOMETRIES = {"resize256": ((256, 375, 500, 3), 256), "hd224": ((64, 1080, 1920, 3), 224)}
OUT = 224


def geometry(name, rounds, model):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import ore
    from ore import squeezenet
    from ore._lib import Resize, check
    from ore.engine import _desc
    (B, HS, WS, C), short = GEOMETRIES[name]
    (rh, rw), (top, left) = ore.center_crop_geometry((HS, WS), short, (OUT, OUT))
    ctx = ore.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1000)
    x8 = torch.randint(0, 256, (B, HS, WS, C), dtype=torch.uint8, device="cuda", generator=g)
    x224 = torch.randint(0, 256, (B, OUT, OUT, C), dtype=torch.uint8, device="cuda", generator=g)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    sc_t, sh_t = (torch.from_numpy(v).cuda().view(1, 3, 1, 1) for v in (scale, shift))

    # the bytes the resize must move
    y0, y1, _ = ore.resize_taps(HS, rh, top, OUT)
    x0, x1, _ = ore.resize_taps(WS, rw, left, OUT)
    span = (int(x1[-1]) - int(x0[0]) + 1) * C
    rows_taps = len(set(y0.tolist()) | set(y1.tolist()))
    rows_rect = int(y1[-1]) - int(y0[0]) + 1
    write_b = B * 4 * C * OUT * OUT
    read_taps, read_rect = B * rows_taps * span, B * rows_rect * span

    y = torch.empty((B, C, OUT, OUT), dtype=torch.float32, device="cuda")
    y2 = torch.empty_like(y)  # the copy's destination
    L = ore.load()
    yd, y2d = _desc(y), _desc(y2)
    Fl = ctypes.c_float * 3
    sc_c, sh_c = Fl(*scale.tolist()), Fl(*shift.tolist())
    xp, xp224 = ctypes.c_void_p(x8.data_ptr()), ctypes.c_void_p(x224.data_ptr())
    geom = Resize(rh, rw, top, left)

    def kernel():
        check(L.ore_preprocess_resize_u8(ctx.h, xp, B, HS, WS, C, ctypes.byref(geom), sc_c, sh_c, 0, ctypes.byref(yd)), ctx.h)

    def framework():
        t = F.interpolate(x8.permute(0, 3, 1, 2).float(), size=(rh, rw), mode="bilinear", align_corners=False, antialias=False)
        return t[:, :, top:top + OUT, left:left + OUT].contiguous().mul_(sc_t).add_(sh_t)

    def floor():
        check(L.ore_preprocess_u8(ctx.h, xp224, B, OUT, OUT, C, sc_c, sh_c, 0, ctypes.byref(yd)), ctx.h)

    def copy():
        check(L.ore_dropout_f32(ctx.h, ctypes.byref(yd), ctypes.byref(y2d)), ctx.h)

    print(f"bench_resize: {name} kernels", file=sys.stderr, flush=True)
    kernel()
    fw_diff = float((framework() - y).abs().max())  # in normalised units; the conventions agree to float32 rounding
    r = alternate({"kernel": (kernel, 30), "framework": (framework, 5), "floor_u8_224": (floor, 30), "copy": (copy, 30)}, rounds)
    a, c = r["kernel"], r["copy"]
    c["gbps_moved"] = round(2 * write_b / c["us"] / 1e3, 1)
    a["gbps_tap_rows"] = round((read_taps + write_b) / a["us"] / 1e3, 1)
    a["gbps_rectangle"] = round((read_rect + write_b) / a["us"] / 1e3, 1)
    res = {"geometry": name, "shape": [B, HS, WS, C], "resized": [rh, rw], "origin": [top, left], "out": [OUT, OUT],
           "bytes_written": write_b, "bytes_read_tap_rows": read_taps, "bytes_read_rectangle": read_rect,
           "kernel": a, "framework": r["framework"], "floor_u8_224": r["floor_u8_224"], "copy_d2d": c,
           "framework_max_abs_diff": fw_diff,
           "framework_over_kernel": round(r["framework"]["us"] / a["us"], 2),
           "kernel_over_floor": round(a["us"] / r["floor_u8_224"]["us"], 2),
           "kernel_rate_over_copy_rate_tap_rows": round(a["gbps_tap_rows"] / c["gbps_moved"], 3),
           "kernel_rate_over_copy_rate_rectangle": round(a["gbps_rectangle"] / c["gbps_moved"], 3)}
    del y2

    if model:
        onnx = squeezenet.build(OUT)
        xf = ore.preprocess_u8(ctx, x224, scale, shift)
        res["model"] = {}
        for precision in ("f32", "f16"):
            print(f"bench_resize: {name} model {precision}", file=sys.stderr, flush=True)
            m = ore.Model(ctx, onnx, max_batch=B, precision=precision)
            m.set_streams(2)
            m.set_input_norm(scale, shift)
            out = torch.empty((B, m.output_elems), device="cuda")
            out_r = torch.empty_like(out)
            m.autotune(xf, out)

            def direct():
                m.set_input_resize(None)
                m.run_u8_into(x224, out)

            def resized():
                m.set_input_resize((HS, WS), (rh, rw), (top, left))
                m.run_u8_into(x8, out_r)

            resized()
            want = m.run(ore.preprocess_resize_u8(ctx, x8, (OUT, OUT), (rh, rw), (top, left), scale, shift))
            equal = bool(torch.equal(want, out_r))
            r = alternate({"run_u8_into": (direct, 10), "run_u8_into_resized": (resized, 10)}, rounds)
            d = r["run_u8_into_resized"]["us"] - r["run_u8_into"]["us"]
            res["model"][precision] = {"run_u8_into": r["run_u8_into"], "run_u8_into_resized": r["run_u8_into_resized"],
                                       "outputs_equal": equal, "added_us": round(d, 2),
                                       "added_share_of_resized_step": round(d / r["run_u8_into_resized"]["us"], 4),
                                       "img_per_s_u8_input": round(B / r["run_u8_into"]["us"] * 1e6),
                                       "img_per_s_resized_input": round(B / r["run_u8_into_resized"]["us"] * 1e6)}
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
        sys.exit("bench_resize.py: no GPU visible")
    res = {"tool": "bench_resize", "rounds": a.rounds, "geometries": [geometry(n, a.rounds, not a.no_model) for n in GEOMETRIES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
