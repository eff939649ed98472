#!/usr/bin/env python3
"""Cost of one Lloyd iteration of spherical k-means: prints one JSON line and writes it to
profiles/kmeans.json.  S = 262144 unit-norm rows drawn from a mixture of L = 1024 Gaussians (tools/bench_nearest_ivf.py's
rows), the centroids L of those rows, at D = 512 and D = 64.  Alternating inside a round:
  step             ore.kmeans_step, the three launches;
  torch_step       the route without it: the f32 matmul + argmax in slabs, index_add_ and normalise of
                   tools/bench_nearest_ivf.py;
  nearest_search   ore.nearest(x, gallery_f16(centroids), 1) on centroids rounded beforehand: the assignment's operands;
  nearest_step     gallery_f16 + that search + index_add_ + normalise.
Every figure is the median over --rounds windows of back-to-back calls timed by HIP events, with the smallest and largest
window beside it (tools/bench_ingest.py's alternate).  The launches of a step alone (assign, update, the rounding of the
centroids) are kernel times from a run of its own under rocprofv3 --kernel-trace: a fresh child process per D that makes
--rounds steps after three warm ones; median, smallest and largest dispatch.  Needs an MI355X (no fallback).
usage: python tools/bench_kmeans.py [--rounds 9] [--S 262144] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_ingest import alternate  # noqa: E402  (the same windows and alternation)

L = 1024
KERNELS = {"assign": "kmeans_assign_kernel", "update": "kmeans_update_kernel", "round_centroids": "gallery_f16_kernel"}


def problem(S, D):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(1000 + D)
    norm = torch.nn.functional.normalize
    means = norm(torch.randn((L, D), device="cuda", generator=gen))
    comp = torch.randint(0, L, (S,), device="cuda", generator=gen)
    x = norm(means[comp] + torch.randn((S, D), device="cuda", generator=gen) / D ** 0.5)
    return x, x[torch.randperm(S, device="cuda", generator=gen)[:L]].clone()


def traced_steps(S, D, rounds):
    """the child under the profiler: three warm steps, then `rounds` more"""
    import torch
    import ore
    ctx = ore.Context(0)
    x, cent = problem(S, D)
    for _ in range(3 + rounds):
        ore.kmeans_step(ctx, x, cent)
    torch.cuda.synchronize()
    ctx.close()


def kernel_times(S, D, rounds):
    """{launch: {"us", "min_us", "max_us"}} of the last `rounds` dispatches of each kernel of a step"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--traced", str(D), "--S", str(S), "--rounds", str(rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not files:
            sys.exit(f"bench_kmeans.py: the traced run failed ({r.returncode}): {r.stderr[-2000:]}")
        rows = [row for f in files for row in csv.DictReader(open(f))]
    out = {}
    for name, part in KERNELS.items():
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rows if part in r["Kernel_Name"]][-rounds:]
        if len(us) != rounds:
            sys.exit(f"bench_kmeans.py: {len(us)} dispatches of {part} in the trace, expected {rounds}")
        out[name] = {"us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--S", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kmeans.json"))
    ap.add_argument("--traced", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    import ore
    if not torch.cuda.is_available():
        sys.exit("bench_kmeans.py: no GPU visible")
    if a.traced:
        return traced_steps(a.S, a.traced, a.rounds)
    ctx = ore.Context(0)
    norm = torch.nn.functional.normalize
    res = {"tool": "bench_kmeans", "S": a.S, "L": L, "rounds": a.rounds, "cells": {}}
    for D in (512, 64):
        x, cent = problem(a.S, D)
        c16 = ore.gallery_f16(ctx, cent)

        def finish(assign):
            sums = torch.zeros_like(cent).index_add_(0, assign, x)
            return torch.where(sums.norm(dim=1, keepdim=True) > 0, norm(sums), cent)

        def torch_step():
            return finish(torch.cat([(x[i:i + 65536] @ cent.T).argmax(1) for i in range(0, a.S, 65536)]))

        def nearest_step():
            return finish(ore.nearest(ctx, x, ore.gallery_f16(ctx, cent), 1)[1][:, 0].long())

        new, assign, scores, _ = ore.kmeans_step(ctx, x, cent)
        v, i = ore.nearest(ctx, x, c16, 1)
        same = bool(torch.equal(assign, i[:, 0]) and torch.equal(scores.view(torch.int32), v[:, 0].view(torch.int32)))
        reps = 5
        r = alternate({"step": (lambda: ore.kmeans_step(ctx, x, cent), reps), "torch_step": (torch_step, reps),
                       "nearest_search": (lambda: ore.nearest(ctx, x, c16, 1), reps), "nearest_step": (nearest_step, reps)}, a.rounds)
        r["same_bits_as_nearest"] = same
        r["max_diff_vs_nearest_step"] = float((new - nearest_step()).abs().max())
        r["assign_flops"], r["update_read_bytes"] = 2 * a.S * L * D, a.S * D * 4
        r["launches"] = kernel_times(a.S, D, a.rounds)
        res["cells"][f"D{D}"] = r
    line = json.dumps(res)
    ctx.close()
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
