#!/usr/bin/env python3
"""Cost of top-k output on the GPU: prints one JSON line.
 (a) ore_topk_f32 alone against torch.topk(rows, k, dim=1, sorted=True) on the same device rows (what a
     caller would use today), at [batch,1000] with k = 1, 5, 64 and [1,1000] with k = 5; the rows are the
     output of a real SqueezeNet run;
 (b) Model.classify_into against Model.run_into on the same model, f32 and f16, max_batch = batch,
     autotuned, set_streams(2), k = 5: the added microseconds are the cost of the feature;
 (c) the same two end to end to pinned host memory: classify_into + download of [batch,5] scores and
     classes against run_into + download of [batch,1000];
 (d) bytes per step and rank of the multi-GPU gather before and after (derived: n*1000*4 against n*k*8).
Every figure is the median over --rounds windows of back-to-back calls timed by HIP events on the context
stream, with the smallest and largest window beside it; the variants of one comparison alternate inside a
round, so drift of the shared machine lands on all of them.  Needs an MI355X (no fallback).
usage: python tools/bench_classify.py [--batch 256] [--hw 224] [--rounds 9] [--out FILE]"""
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
        sys.exit("bench_classify.py: no GPU visible")
    B, S = a.batch, a.hw
    ctx = ore.Context(0)
    L = ore.load()
    g = torch.Generator(device="cuda").manual_seed(1000)
    x8 = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=g)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    xf = ore.preprocess_u8(ctx, x8, scale, shift)
    onnx = squeezenet.build(S)
    res = {"tool": "bench_classify", "batch": B, "hw": S, "rounds": a.rounds, "k": K, "kernel": {}, "model": {}}

    rows_all = None
    for precision in ("f32", "f16"):
        m = ore.Model(ctx, onnx, max_batch=B, precision=precision)
        m.set_streams(2)
        m.set_topk(K)
        D = m.output_elems
        out = torch.empty((B, D), device="cuda")
        scores = torch.empty((B, K), dtype=torch.float32, device="cuda")
        classes = torch.empty((B, K), dtype=torch.int32, device="cuda")
        h_out = torch.empty((B, D), dtype=torch.float32).pin_memory()
        h_scores = torch.empty((B, K), dtype=torch.float32).pin_memory()
        h_classes = torch.empty((B, K), dtype=torch.int32).pin_memory()
        m.autotune(xf, out)
        m.run_into(xf, out)
        m.classify_into(xf, scores, classes)
        tv, ti = torch.topk(out, K, dim=1, sorted=True)
        equal = bool(torch.equal(tv, scores))  # indices may differ from torch's where values tie
        if precision == "f32":
            rows_all = out.clone()

        def run_host():
            m.run_into(xf, out)
            h_out.copy_(out, non_blocking=True)

        def classify_host():
            m.classify_into(xf, scores, classes)
            h_scores.copy_(scores, non_blocking=True)
            h_classes.copy_(classes, non_blocking=True)

        r = alternate({"run_into": (lambda: m.run_into(xf, out), 10),
                       "classify_into": (lambda: m.classify_into(xf, scores, classes), 10),
                       "run_into_to_host": (run_host, 10), "classify_into_to_host": (classify_host, 10)}, a.rounds)
        d = r["classify_into"]["us"] - r["run_into"]["us"]
        dh = r["classify_into_to_host"]["us"] - r["run_into_to_host"]["us"]
        res["model"][precision] = dict(r, scores_equal_torch_topk_of_run=equal, added_us=round(d, 2),
                                       added_pct_of_run_into=round(100.0 * d / r["run_into"]["us"], 3),
                                       to_host_delta_us=round(dh, 2),
                                       to_host_delta_pct=round(100.0 * dh / r["run_into_to_host"]["us"], 3),
                                       download_bytes_run=B * D * 4, download_bytes_classify=B * K * 8)
        m.close()

    # (a) the kernel alone, on the f32 model's rows
    D = rows_all.shape[1]
    for n, k in ((B, 1), (B, 5), (B, 64), (1, 5)):
        rows = rows_all[:n].contiguous()
        rd = _desc(rows)
        v = torch.empty((n, k), dtype=torch.float32, device="cuda")
        i = torch.empty((n, k), dtype=torch.int32, device="cuda")
        vp, ip = ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(i.data_ptr())

        def kernel():
            check(L.ore_topk_f32(ctx.h, ctypes.byref(rd), k, vp, ip), ctx.h)

        def framework():
            return torch.topk(rows, k, dim=1, sorted=True)

        kernel()
        tv, ti = framework()
        r = alternate({"kernel": (kernel, 200), "torch_topk": (framework, 200)}, a.rounds)
        res["kernel"][f"{n}x{D}_k{k}"] = dict(r, values_equal=bool(torch.equal(tv, v)),
                                              indices_equal=bool(torch.equal(ti.to(torch.int32), i)),
                                              torch_over_kernel=round(r["torch_topk"]["us"] / r["kernel"]["us"], 2))
    res["gather_bytes_per_rank_step"] = {"rows": B * D * 4, "topk": B * K * 8, "ratio": round(B * D * 4 / (B * K * 8), 1)}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
