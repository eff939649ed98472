#!/usr/bin/env python3
"""Cost of uint8 input on the GPU: prints one JSON line.  At a batch of uint8 [256,224,224,3]:
 (a) ore_preprocess_u8, and its GB/s over the bytes it must move (n*H*W*C read + 4x that written);
 (b) the framework equivalent a caller would write without it:
     x.permute(0,3,1,2).float().mul_(scale).add_(shift).contiguous();
 (c) a device-to-device hipMemcpyAsync of the float32 batch (ore_dropout_f32 is exactly that), as the
     machine's own copy rate: it moves 2x the float32 batch, (a)'s rate is reported as a fraction of it;
 (d) Model.run_u8_into against Model.run_into on the converted batch, f32 and f16, max_batch = batch,
     autotuned, set_streams(2).
Every figure is the median over --rounds windows of back-to-back calls timed by HIP events on the context
stream, with the smallest and largest window beside it; the variants of one comparison alternate inside a
round, so drift of the shared machine lands on all of them.  Needs an MI355X (no fallback).
usage: python tools/bench_ingest.py [--batch 256] [--hw 224] [--rounds 9] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))


def window_us(fn, reps):
    """Mean time of one call over `reps` back-to-back calls, in microseconds (HIP events)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1000.0


def alternate(variants, rounds, warmup=3):
    """variants: {name: (fn, reps)} -> {name: {"us": median, "min_us", "max_us"}} over `rounds` rounds, each
    timing every variant once, in turn."""
    import torch
    for fn, _ in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, reps) in variants.items():
            t[k].append(window_us(fn, reps))
    return {k: {"us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import ore
    from ore import squeezenet
    from ore._lib import check
    from ore.engine import _desc
    if not torch.cuda.is_available():
        sys.exit("bench_ingest.py: no GPU visible")
    B, S = a.batch, a.hw
    ctx = ore.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1000)
    x8 = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=g)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    sc_t, sh_t = (torch.from_numpy(v).cuda().view(1, 3, 1, 1) for v in (scale, shift))
    read_b, write_b = x8.numel(), x8.numel() * 4

    # (a) - (c)
    y = torch.empty((B, 3, S, S), dtype=torch.float32, device="cuda")
    y2 = torch.empty_like(y)
    L = ore.load()
    yd, y2d = _desc(y), _desc(y2)
    F = ctypes.c_float * 3
    sc_c, sh_c = F(*scale.tolist()), F(*shift.tolist())
    xp = ctypes.c_void_p(x8.data_ptr())

    def kernel():
        check(L.ore_preprocess_u8(ctx.h, xp, B, S, S, 3, sc_c, sh_c, 0, ctypes.byref(yd)), ctx.h)

    def framework():
        return x8.permute(0, 3, 1, 2).float().mul_(sc_t).add_(sh_t).contiguous()

    def copy():
        check(L.ore_dropout_f32(ctx.h, ctypes.byref(yd), ctypes.byref(y2d)), ctx.h)

    kernel()
    same = bool(torch.equal(y, framework()))
    r = alternate({"kernel": (kernel, 50), "framework": (framework, 10), "copy": (copy, 50)}, a.rounds)
    k, f, c = r["kernel"], r["framework"], r["copy"]
    k["gbps"] = round((read_b + write_b) / k["us"] / 1e3, 1)
    c["gbps_moved"] = round(2 * write_b / c["us"] / 1e3, 1)
    res = {"tool": "bench_ingest", "shape": [B, S, S, 3], "rounds": a.rounds, "bytes_read": read_b, "bytes_written": write_b,
           "kernel": k, "framework": f, "copy_d2d": c, "kernel_equals_framework": same,
           "kernel_vs_framework": round(f["us"] / k["us"], 2), "kernel_rate_over_copy_rate": round(k["gbps"] / c["gbps_moved"], 3)}

    # (d)
    onnx = squeezenet.build(S)
    xf = ore.preprocess_u8(ctx, x8, scale, shift)
    res["model"] = {}
    for precision in ("f32", "f16"):
        m = ore.Model(ctx, onnx, max_batch=B, precision=precision)
        m.set_streams(2)
        m.set_input_norm(scale, shift)
        out = torch.empty((B, m.output_elems), device="cuda")
        out8 = torch.empty_like(out)
        m.autotune(xf, out)
        m.run_u8_into(x8, out8)
        equal = bool(torch.equal(m.run_into(xf, out), out8))
        r = alternate({"run_into": (lambda: m.run_into(xf, out), 10), "run_u8_into": (lambda: m.run_u8_into(x8, out8), 10)},
                      a.rounds)
        d = r["run_u8_into"]["us"] - r["run_into"]["us"]
        res["model"][precision] = {"run_into": r["run_into"], "run_u8_into": r["run_u8_into"], "outputs_equal": equal,
                                   "added_us": round(d, 2), "added_share_of_u8_step": round(d / r["run_u8_into"]["us"], 4),
                                   "img_per_s_f32_input": round(B / r["run_into"]["us"] * 1e6),
                                   "img_per_s_u8_input": round(B / r["run_u8_into"]["us"] * 1e6)}
        m.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
