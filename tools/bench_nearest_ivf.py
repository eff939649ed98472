#!/usr/bin/env python3
"""Cost and recall of the inverted-file search beside the full f16 search: prints one JSON line.
D = 512, k = 5, G = 10^6 rows drawn from a mixture of 1024 Gaussians and L2-normalised, the queries from the same
mixture; L = 1024 centroids from a few Lloyd iterations (torch, inner product) started on gallery rows.  Per cell of
nprobe in {8, 16, 32} x n in {1, 32, 256}, alternating inside a round: the whole IvfIndex.search, its coarse stage
(ore.nearest on the centroids) and its scan (ore.nearest_lists on the probes of that stage) alone, the search with
rerank=, and ore.nearest on the same rows as an f16 gallery.  Beside them the bytes the distinct probed lists hold, the
bytes the scan has to read (a list once per group of 64 queries that probe it), the read floor of the latter at
--hbm-tbs, and the recall of the f32 search's five indices with and without rerank.
Every figure is the median over --rounds windows of back-to-back calls timed by HIP events on the context stream, with
the smallest and largest window beside it (tools/bench_ingest.py's alternate).  Needs an MI355X (no fallback).
usage: python tools/bench_nearest_ivf.py [--rounds 9] [--out FILE]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_ingest import alternate  # noqa: E402  (the same windows and alternation)

D, K, L = 512, 5, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--G", type=int, default=10 ** 6)
    ap.add_argument("--lloyd", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import ore
    if not torch.cuda.is_available():
        sys.exit("bench_nearest_ivf.py: no GPU visible")
    ctx = ore.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(1000)
    norm = torch.nn.functional.normalize
    means = norm(torch.randn((L, D), device="cuda", generator=gen))

    def draw(m):  # a component's mean plus noise of about the same length, then onto the sphere
        comp = torch.randint(0, L, (m,), device="cuda", generator=gen)
        return norm(means[comp] + torch.randn((m, D), device="cuda", generator=gen) / D ** 0.5)

    g = draw(a.G)
    cent = g[torch.randperm(a.G, device="cuda", generator=gen)[:L]].clone()
    for _ in range(a.lloyd):
        assign = torch.cat([(g[i:i + 65536] @ cent.T).argmax(1) for i in range(0, a.G, 65536)])
        sums = torch.zeros_like(cent).index_add_(0, assign, g)
        cent = torch.where(sums.norm(dim=1, keepdim=True) > 0, norm(sums), cent).contiguous()
    index = ore.ivf_build(ctx, g, cent)
    sizes = (index.offsets[1:] - index.offsets[:-1]).long()
    res = {"tool": "bench_nearest_ivf", "D": D, "k": K, "G": a.G, "L": L, "rounds": a.rounds, "hbm_tbs": a.hbm_tbs,
           "chunk_rows": ore.IVF_CHUNK_ROWS, "chunks": int(index.chunks.shape[0]), "max_list_rows": index.max_list_rows,
           "empty_lists": int((sizes == 0).sum()), "cells": {}}
    for n in (1, 32, 256):
        q = draw(n)
        exact = ore.nearest(ctx, q, g, K)[1]
        for nprobe in (8, 16, 32):
            probes = ore.nearest(ctx, q, cent, nprobe)[1]
            reps = 10
            r = alternate({
                "search": (lambda: index.search(q, K, nprobe), reps),
                "coarse": (lambda: ore.nearest(ctx, q, cent, nprobe), reps),
                "scan": (lambda: ore.nearest_lists(ctx, q, index.gallery, index.offsets, index.chunks, probes, K, index.max_list_rows), reps),
                "search_rerank": (lambda: index.search(q, K, nprobe, rerank=g), reps),
                "full_f16": (lambda: ore.nearest(ctx, q, index.gallery, K), reps)}, a.rounds)
            pairs = torch.bincount(probes.flatten().long(), minlength=L)  # the coarse stage names no list twice
            held = int(sizes[pairs > 0].sum()) * D * 2
            read = int((sizes * ((pairs + 63) // 64)).sum()) * D * 2
            r["probed_lists"], r["probed_bytes"], r["scan_read_bytes"] = int((pairs > 0).sum()), held, read
            r["scan_floor_us"] = round(read / (a.hbm_tbs * 1e6), 2)
            for name, kw in (("recall_vs_f32", {}), ("recall_vs_f32_rerank", {"rerank": g})):
                got = index.search(q, K, nprobe, **kw)[1]
                r[name] = round(float((got[:, :, None] == exact[:, None, :]).any(2).float().mean()), 4)
            res["cells"][f"n{n}_nprobe{nprobe}"] = r
    line = json.dumps(res)
    ctx.close()
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
