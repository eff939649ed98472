#!/usr/bin/env python3
"""Cost and recall of the MXFP4 candidate search beside the int8 one: prints one JSON line.
Per cell of n in {1, 32, 256} x G in {10^4, 10^6} at D = 512, for B in {32, 128} and c in {32, 64}, alternating inside
a round: ore.nearest_bins on the MXFP4 gallery (ore.gallery_mxfp4) and on the int8 gallery (ore.gallery_i8), both
kernels each, and the two two-stage searches ore.nearest(..., rerank=g, candidates=c, bin_rows=B), k = 5, with the
share of queries whose five indices equal the f32 search's.  Beside them the read floors: one read of the gallery per
query tile of 64 at --hbm-tbs, 272 bytes a row for MXFP4 (256 of codes, 16 of scales) and 516 for int8.
Every figure is the median over --rounds windows of back-to-back calls timed by HIP events on the context stream, with
the smallest and largest window beside it (tools/bench_ingest.py's alternate).  Needs an MI355X (no fallback).
usage: python tools/bench_nearest_fp4.py [--rounds 9] [--out FILE]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_ingest import alternate  # noqa: E402  (the same windows and alternation)

D, K = 512, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import ore
    if not torch.cuda.is_available():
        sys.exit("bench_nearest_fp4.py: no GPU visible")
    ctx = ore.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(1000)
    res = {"tool": "bench_nearest_fp4", "D": D, "k": K, "rounds": a.rounds, "hbm_tbs": a.hbm_tbs, "cells": {}}
    for G in (10 ** 4, 10 ** 6):
        g = torch.nn.functional.normalize(torch.randn((G, D), device="cuda", generator=gen))
        gals = {"mxfp4": ore.gallery_mxfp4(ctx, g), "i8": ore.gallery_i8(ctx, g)}
        for n in (1, 32, 256):
            q = torch.nn.functional.normalize(torch.randn((n, D), device="cuda", generator=gen))
            reps = 20 if G * n <= 10 ** 7 else 3
            settings = [(f, B, c) for f in gals for B in (32, 128) for c in (32, 64)]
            v = {}
            for f, B, c in settings:
                gal, sc = gals[f]
                v[f"{f}_B{B}_c{c}_bins"] = (lambda gal=gal, sc=sc, B=B, c=c: ore.nearest_bins(ctx, q, gal, c, B, scales=sc), reps)
                v[f"{f}_B{B}_c{c}_two_stage"] = (lambda gal=gal, sc=sc, B=B, c=c: ore.nearest(ctx, q, gal, K, scales=sc, rerank=g,
                                                                                             candidates=c, bin_rows=B), reps)
            r = alternate(v, a.rounds)
            exact = ore.nearest(ctx, q, g, K)[1].sort(1)[0]
            for f, B, c in settings:
                gal, sc = gals[f]
                got = ore.nearest(ctx, q, gal, K, scales=sc, rerank=g, candidates=c, bin_rows=B)[1].sort(1)[0]
                r[f"{f}_B{B}_c{c}_two_stage"]["same_index_set_share_vs_f32"] = round(float((got == exact).all(1).float().mean()), 4)
            tiles = -(-n // 64)
            r["floor_read_us"] = {"mxfp4": round(tiles * G * 272 / (a.hbm_tbs * 1e6), 2), "i8": round(tiles * G * 516 / (a.hbm_tbs * 1e6), 2)}
            r["segments"] = {f"{f}_B{B}": (ore.nearest_bins_segments_mxfp4 if f == "mxfp4" else ore.nearest_bins_segments)(ctx, n, G, B)[0]
                             for f in gals for B in (32, 128)}
            res["cells"][f"n{n}_G{G}"] = r
        del g, gals
    line = json.dumps(res)
    ctx.close()
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
