#!/usr/bin/env python3
"""Cost of the class activation maps on the GPU: prints one JSON line.
 (a) the map kernel alone (ore_class_maps_f32 on conv10's real input and weights, f32) against its floor: one
     read of the conv's input at the copy rate of DESIGN.md section 4 (6.29 TB/s);
 (b) Model.classify_into with and without a buffer set (set_cam_output) on the same model, f32 and f16,
     max_batch = batch, autotuned, set_streams(2), k = 5: the added microseconds are the cost of the feature;
 (c) what a caller did before: a fusion-0 + ORE_KEEP_VALUES model's run_into (which stores the [batch, 1000,
     13, 13] map), plus a torch gather of the k planes per image out of a device copy of that map.  Both are
     lower bounds on (c): the map lives in the model's arena, so a caller gets it only through read_value, a
     download of 176 MB at batch 256 that is not timed here; and f16 models store it as NHWC halves, which
     read_value converts on the host, so for f16 only the run_into of that plan is timed.
Every figure is the median over --rounds windows of back-to-back calls timed by HIP events on the context
stream, with the smallest and largest window beside it; the variants of one comparison alternate inside a
round, so drift of the shared machine lands on all of them.  Needs an MI355X (no fallback).
usage: python tools/bench_cam.py [--batch 256] [--hw 224] [--rounds 9] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_ingest import alternate  # noqa: E402  (the same windows and alternation)

K = 5
COPY_TBS = 6.29  # the device copy rate the floors are written against


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
    from ore import onnx_wire, squeezenet
    from ore._lib import check
    from ore.engine import _desc
    if not torch.cuda.is_available():
        sys.exit("bench_cam.py: no GPU visible")
    B, S = a.batch, a.hw
    ctx = ore.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1000)
    x8 = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=g)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    xf = ore.preprocess_u8(ctx, x8, scale, shift)
    onnx = squeezenet.build(S)
    graph = onnx_wire.decode_model(onnx).graph
    conv10 = [n for n in graph.node if n.op_type == "Conv"][-1]
    inits = {t.name: t.to_numpy() for t in graph.initializer}
    res = {"tool": "bench_cam", "batch": B, "hw": S, "rounds": a.rounds, "k": K, "kernel": {}, "model": {}}

    kernel_in = None
    for precision in ("f32", "f16"):
        m = ore.Model(ctx, onnx, max_batch=B, precision=precision)
        m.set_streams(2)
        m.set_topk(K)
        hm, wm = m.cam_hw
        out = torch.empty((B, m.output_elems), device="cuda")
        scores = torch.empty((B, K), dtype=torch.float32, device="cuda")
        classes = torch.empty((B, K), dtype=torch.int32, device="cuda")
        maps = torch.empty((B, K, hm, wm), dtype=torch.float32, device="cuda")
        m.autotune(xf, out)
        # the caller's way before: the unfused plan that stores the map, and a gather out of it
        old = ore.Model(ctx, onnx, max_batch=B, precision=precision)
        old.set_fusion(ore.KEEP_VALUES)
        old_out = torch.empty((B, old.output_elems), device="cuda")
        old.run_into(xf, old_out)
        m.classify_into(xf, scores, classes)
        torch.cuda.synchronize()
        variants = {}
        if precision == "f32":
            T = torch.from_numpy(old.read_value(_pool_input_name(graph))).cuda()
            idx = classes.to(torch.int64)[:, :, None, None].expand(B, K, hm, wm)

            def old_way():
                old.run_into(xf, old_out)
                return torch.gather(T, 1, idx)

            m.set_cam_output(maps)
            m.classify_into(xf, scores, classes)
            torch.cuda.synchronize()
            # against the unfused plan's stored map: equal bits where both plans feed conv10 the same input; on f32
            # Winograd models the fusion flags decide which 3x3 convs run Winograd, so the inputs differ in the last bits
            equal = float((torch.gather(T, 1, classes.to(torch.int64)[:, :, None, None].expand(B, K, hm, wm)) - maps).abs().max())
            kernel_in = torch.from_numpy(m.read_value(conv10.input[0])).cuda()
            m.set_cam_output(None)
            variants["keep_values_run_plus_gather"] = (old_way, 5)
        else:
            equal = None
            variants["keep_values_run_into"] = (lambda: old.run_into(xf, old_out), 5)

        def with_maps():
            m.classify_into(xf, scores, classes)

        # the two settings of one model cannot alternate inside a round without a replan between them: each is
        # measured against the unfused plan in rounds of its own, the plain one first
        plain = alternate(dict(variants, classify_into=(with_maps, 10)), a.rounds)
        m.set_cam_output(maps)
        cam = alternate(dict(variants, classify_into_cam=(with_maps, 10)), a.rounds)
        m.set_cam_output(None)
        old_key = next(iter(variants))
        d = cam["classify_into_cam"]["us"] - plain["classify_into"]["us"]
        res["model"][precision] = {
            "classify_into": plain["classify_into"], "classify_into_cam": cam["classify_into_cam"],
            old_key: cam[old_key], old_key + "_in_the_plain_rounds": plain[old_key],
            "added_us": round(d, 2), "added_pct_of_classify_into": round(100.0 * d / plain["classify_into"]["us"], 3),
            "old_way_over_classify_into_cam": round(cam[old_key]["us"] / cam["classify_into_cam"]["us"], 2),
            "maps_max_abs_diff_vs_unfused_plans_map": equal, "maps_bytes": B * K * hm * wm * 4,
            "stored_map_bytes": B * m.output_elems * hm * wm * (4 if precision == "f32" else 2)}
        old.close()
        m.close()

    # (a) the kernel alone on conv10's input (f32), against one read of that input at the copy rate
    w = torch.from_numpy(inits[conv10.input[1]].reshape(inits[conv10.input[1]].shape[0], -1).copy()).cuda()
    bias = torch.from_numpy(inits[conv10.input[2]]).cuda()
    L = ore.load()
    for n in (B, 1):
        xk = kernel_in[:n].contiguous()
        cls = torch.randint(0, w.shape[0], (n, K), dtype=torch.int32, device="cuda", generator=g)
        out = torch.empty((n, K) + tuple(xk.shape[2:]), dtype=torch.float32, device="cuda")
        xd = _desc(xk)
        ptr = [ctypes.c_void_p(t.data_ptr()) for t in (w, bias, cls, out)]

        def kernel():
            check(L.ore_class_maps_f32(ctx.h, ctypes.byref(xd), ptr[0], ptr[1], int(w.shape[0]), 1, ptr[2], K, 1, ptr[3]), ctx.h)

        kernel()
        equal = bool(torch.equal(out, ore.class_maps(ctx, xk, w, bias, cls)))
        r = alternate({"kernel": (kernel, 200)}, a.rounds)
        floor_us = xk.numel() * 4 / (COPY_TBS * 1e12) * 1e6
        res["kernel"][f"{n}x{xk.shape[1]}x{xk.shape[2]}x{xk.shape[3]}_k{K}"] = dict(
            r, input_bytes=xk.numel() * 4, floor_us=round(floor_us, 2), kernel_over_floor=round(r["kernel"]["us"] / floor_us, 2),
            equal_the_wrapper=equal)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def _pool_input_name(graph):
    return [n for n in graph.node if n.op_type == "GlobalAveragePool"][0].input[0]


if __name__ == "__main__":
    main()
