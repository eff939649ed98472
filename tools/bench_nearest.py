#!/usr/bin/env python3
"""Cost of the nearest-neighbour search and of the embedding on the GPU: prints one JSON line.
 (a) ore.nearest for n in {1, 32, 256} queries against G in {10^4, 10^6} rows at D = 512, k = 5, beside what a
     caller did before on the same tensors: q @ g.T followed by torch.topk.  Each case with its two floors: one read
     of the gallery per query tile of 64 at --hbm-tbs, and 2 n G D FLOPs at --mfma-tflops (the f32 matrix peak); the
     larger is the floor that binds.  The share of rows on which both return the same index set is reported.
     Beside them the same search on the packed f16 copy of the gallery (ore.gallery_f16), the three alternating
     inside a round: its floors are the read at 2 bytes per element and the FLOPs at --mfma-f16-tflops (the f16
     matrix peak), with the share of rows on which the f16 and the f32 search return the same index set.
     And the same search on the int8 copy with a scale per row (ore.gallery_i8), the four alternating inside a round:
     its floors are the read of G D bytes of codes and 4 G bytes of scales per query tile, and the operations at
     --mfma-i8-tops (the dense int8 matrix peak of AMD's MI355X data sheet, 5.0 POPS: twice the f16 figure, as
     v_mfma_i32_16x16x64_i8 has twice the k-depth of v_mfma_f32_16x16x32_f16 at the same issue rate); with the share
     of rows on which the int8 and the f32 search return the same index set, the mean overlap of the two sets, and
     the ratio to the f16 search of the same rounds beside the two min - max spreads it has to exceed.
     And the two-stage search in the same rounds: the int8 search with 32 candidates, then ore.rerank of those against
     the f32 gallery (ore.nearest(..., rerank=g, candidates=32)), k = 5, and the rerank launch alone on the same
     candidates.  The rerank's floor is its gathered read, n 32 D 4 bytes at --hbm-tbs; the two-stage time stands
     against the f32 search of the same rounds, with the same index-set share and mean overlap against it.
 (b) Model.classify_into (SqueezeNet at --hw, --batch images, k = 5, f32 and f16, autotuned, set_streams(2)) with
     the normalised embedding on against off.
Every figure is the median over --rounds windows of back-to-back calls timed by HIP events on the context stream,
with the smallest and largest window beside it; the variants of one comparison alternate inside a round.  Needs an
MI355X (no fallback).
 (c) --bins, instead of (a) and (b): the binned candidate search, see bins_part().
usage: python tools/bench_nearest.py [--batch 256] [--hw 224] [--rounds 9] [--skip-model] [--bins] [--out FILE]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_ingest import alternate  # noqa: E402  (the same windows and alternation)

D, K, KC = 512, 5, 32  # KC: the candidates of the two-stage search


def bins_part(a, ctx, torch, ore, gen):
    """--bins: the binned candidate search.  Per cell of n x G, alternating inside a round: the f32
    search, the int8 search at k = 5 and at k = 32, and for the int8 and the f16 gallery, B in {32, 128}, c in {32,
    128}: ore.nearest_bins (both kernels) and the two-stage ore.nearest(..., rerank=g, candidates=c, bin_rows=B), with
    the share of queries whose five indices equal the f32 search's.  The read floors are those of part (a)."""
    res = {"tool": "bench_nearest --bins", "D": D, "k": K, "rounds": a.rounds, "hbm_tbs": a.hbm_tbs, "cells": {}}
    for G in (10 ** 4, 10 ** 6):
        g = torch.nn.functional.normalize(torch.randn((G, D), device="cuda", generator=gen))
        gh = ore.gallery_f16(ctx, g)
        gi, si = ore.gallery_i8(ctx, g)
        for n in (1, 32, 256):
            q = torch.nn.functional.normalize(torch.randn((n, D), device="cuda", generator=gen))
            reps = 20 if G * n <= 10 ** 7 else 3
            v = {"f32_k5": (lambda: ore.nearest(ctx, q, g, K), reps),
                 "i8_k5": (lambda: ore.nearest(ctx, q, gi, K, scales=si), reps),
                 "i8_k32": (lambda: ore.nearest(ctx, q, gi, KC, scales=si), reps),
                 "i8_k32_two_stage": (lambda: ore.nearest(ctx, q, gi, K, scales=si, rerank=g, candidates=KC), reps)}
            # c no larger than the bins there are: G = 10^4 at B = 128 has 79, and that setting is named c79
            settings = [(f, B, min(c, -(-G // B))) for f in ("i8", "f16") for B in (32, 128) for c in (32, 128)]
            for f, B, c in settings:
                gal, sc = (gi, si) if f == "i8" else (gh, None)
                v[f"{f}_B{B}_c{c}_bins"] = (lambda gal=gal, sc=sc, B=B, c=c: ore.nearest_bins(ctx, q, gal, c, B, scales=sc), reps)
                v[f"{f}_B{B}_c{c}_two_stage"] = (lambda gal=gal, sc=sc, B=B, c=c: ore.nearest(ctx, q, gal, K, scales=sc, rerank=g,
                                                                                             candidates=c, bin_rows=B), reps)
            r = alternate(v, a.rounds)
            exact = ore.nearest(ctx, q, g, K)[1].sort(1)[0]
            for f, B, c in settings:
                gal, sc = (gi, si) if f == "i8" else (gh, None)
                got = ore.nearest(ctx, q, gal, K, scales=sc, rerank=g, candidates=c, bin_rows=B)[1].sort(1)[0]
                r[f"{f}_B{B}_c{c}_two_stage"]["same_index_set_share_vs_f32"] = round(float((got == exact).all(1).float().mean()), 4)
            got = ore.nearest(ctx, q, gi, K, scales=si, rerank=g, candidates=KC)[1].sort(1)[0]
            r["i8_k32_two_stage"]["same_index_set_share_vs_f32"] = round(float((got == exact).all(1).float().mean()), 4)
            tiles = -(-n // 64)
            r["floor_read_us"] = {"i8": round(tiles * (G * D + 4 * G) / (a.hbm_tbs * 1e6), 2), "f16": round(tiles * G * D * 2 / (a.hbm_tbs * 1e6), 2)}
            r["segments"] = {f"B{B}": ore.nearest_bins_segments(ctx, n, G, B)[0] for B in (32, 128)}
            res["cells"][f"n{n}_G{G}"] = r
        del g, gh, gi, si
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", action="store_true", help="the binned candidate search only (DESIGN.md 3.13f)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--mfma-tflops", type=float, default=157.3)
    ap.add_argument("--mfma-f16-tflops", type=float, default=2500.0)
    ap.add_argument("--mfma-i8-tops", type=float, default=5000.0)
    ap.add_argument("--skip-model", action="store_true", help="part (a) only")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import ore
    from ore import squeezenet
    if not torch.cuda.is_available():
        sys.exit("bench_nearest.py: no GPU visible")
    ctx = ore.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(1000)
    if a.bins:
        line = json.dumps(bins_part(a, ctx, torch, ore, gen))
        ctx.close()
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
    res = {"tool": "bench_nearest", "D": D, "k": K, "rounds": a.rounds, "hbm_tbs": a.hbm_tbs, "mfma_tflops": a.mfma_tflops,
           "mfma_f16_tflops": a.mfma_f16_tflops, "mfma_i8_tops": a.mfma_i8_tops, "nearest": {}, "nearest_f16": {}, "nearest_i8": {},
           "nearest_rerank": {}, "rerank_candidates": KC, "model": {}}
    for G in (10 ** 4, 10 ** 6):
        g = torch.nn.functional.normalize(torch.randn((G, D), device="cuda", generator=gen))
        gh = ore.gallery_f16(ctx, g)
        gi, si = ore.gallery_i8(ctx, g)
        for n in (1, 32, 256):
            q = torch.nn.functional.normalize(torch.randn((n, D), device="cuda", generator=gen))
            reps = 20 if G * n <= 10 ** 7 else 3
            cand = ore.nearest(ctx, q, gi, min(G, KC), scales=si)[1]
            r = alternate({"ore_nearest": (lambda: ore.nearest(ctx, q, g, K), reps),
                           "ore_two_stage": (lambda: ore.nearest(ctx, q, gi, K, scales=si, rerank=g, candidates=KC), reps),
                           "ore_rerank": (lambda: ore.rerank(ctx, q, g, cand, K), reps),
                           "ore_nearest_f16": (lambda: ore.nearest(ctx, q, gh, K), reps),
                           "ore_nearest_i8": (lambda: ore.nearest(ctx, q, gi, K, scales=si), reps),
                           "matmul_topk": (lambda: torch.topk(q @ g.T, K, dim=1), reps)}, a.rounds)
            ours, theirs = ore.nearest(ctx, q, g, K)[1], torch.topk(q @ g.T, K, dim=1)[1]
            halves = ore.nearest(ctx, q, gh, K)[1]
            bytes_ = ore.nearest(ctx, q, gi, K, scales=si)[1]
            torch.cuda.synchronize()
            same = (ours.long().sort(1)[0] == theirs.sort(1)[0]).all(1).float().mean()
            same_h = (ours.sort(1)[0] == halves.sort(1)[0]).all(1).float().mean()
            same_i = (ours.sort(1)[0] == bytes_.sort(1)[0]).all(1).float().mean()
            overlap_i = (ours[:, :, None] == bytes_[:, None, :]).any(2).float().mean()
            h, b = r.pop("ore_nearest_f16"), r.pop("ore_nearest_i8")
            two, rr = r.pop("ore_two_stage"), r.pop("ore_rerank")
            staged = ore.nearest(ctx, q, gi, K, scales=si, rerank=g, candidates=KC)[1]
            torch.cuda.synchronize()
            gather_us = n * KC * D * 4 / (a.hbm_tbs * 1e6)
            res["nearest_rerank"][f"n{n}_G{G}"] = dict(
                two, rerank_alone=rr, floor_gather_us=round(gather_us, 3), rerank_share_of_floor=round(gather_us / rr["us"], 4),
                i8_search_us=b["us"], f32_search_us=r["ore_nearest"]["us"], speedup_vs_f32=round(r["ore_nearest"]["us"] / two["us"], 3),
                f32_window_spread_us=round(r["ore_nearest"]["max_us"] - r["ore_nearest"]["min_us"], 2),
                ahead_of_f32=bool(r["ore_nearest"]["min_us"] > two["max_us"]),
                same_index_set_share_vs_f32=round(float((ours.sort(1)[0] == staged.sort(1)[0]).all(1).float().mean()), 4),
                mean_overlap_vs_f32=round(float((ours[:, :, None] == staged[:, None, :]).any(2).float().mean()), 4))
            read_b, mfma_b = -(-n // 64) * (G * D + 4 * G) / (a.hbm_tbs * 1e6), 2.0 * n * G * D / (a.mfma_i8_tops * 1e6)
            segments_b, step_rows_b = ore.nearest_segments_i8(ctx, n, G)
            spread = max(h["max_us"] - h["min_us"], b["max_us"] - b["min_us"])
            res["nearest_i8"][f"n{n}_G{G}"] = dict(
                b, segments=segments_b, step_rows=step_rows_b, floor_read_us=round(read_b, 2), floor_mfma_us=round(mfma_b, 2),
                bound="mfma" if mfma_b > read_b else "read", share_of_floor=round(max(read_b, mfma_b) / b["us"], 4),
                gallery_gbs=round(-(-n // 64) * (G * D + 4 * G) / b["us"] / 1e3, 1), tops=round(2.0 * n * G * D / b["us"] / 1e6, 2),
                speedup_vs_f16=round(h["us"] / b["us"], 3), speedup_vs_f32=round(r["ore_nearest"]["us"] / b["us"], 3),
                f16_minus_i8_us=round(h["us"] - b["us"], 2), larger_window_spread_us=round(spread, 2),
                faster_than_f16=bool(h["us"] - b["us"] > spread),
                same_index_set_share_vs_f32=round(float(same_i), 4), mean_overlap_vs_f32=round(float(overlap_i), 4))
            read_h, mfma_h = -(-n // 64) * G * D * 2 / (a.hbm_tbs * 1e6), 2.0 * n * G * D / (a.mfma_f16_tflops * 1e6)
            segments_h, step_rows = ore.nearest_segments_f16(ctx, n, G)
            res["nearest_f16"][f"n{n}_G{G}"] = dict(
                h, segments=segments_h, step_rows=step_rows, floor_read_us=round(read_h, 2), floor_mfma_us=round(mfma_h, 2),
                bound="mfma" if mfma_h > read_h else "read", share_of_floor=round(max(read_h, mfma_h) / h["us"], 4),
                gallery_gbs=round(-(-n // 64) * G * D * 2 / h["us"] / 1e3, 1), tflops=round(2.0 * n * G * D / h["us"] / 1e6, 2),
                speedup_vs_f32=round(r["ore_nearest"]["us"] / h["us"], 3),
                f32_window_spread_us=round(r["ore_nearest"]["max_us"] - r["ore_nearest"]["min_us"], 2),
                same_index_set_share_vs_f32=round(float(same_h), 4))
            read_us = -(-n // 64) * G * D * 4 / (a.hbm_tbs * 1e6)
            mfma_us = 2.0 * n * G * D / (a.mfma_tflops * 1e6)
            us = r["ore_nearest"]["us"]
            res["nearest"][f"n{n}_G{G}"] = dict(
                r, segments=ore.nearest_segments(ctx, n, G), floor_read_us=round(read_us, 2), floor_mfma_us=round(mfma_us, 2),
                bound="mfma" if mfma_us > read_us else "read", share_of_floor=round(max(read_us, mfma_us) / us, 4),
                gallery_gbs=round(-(-n // 64) * G * D * 4 / us / 1e3, 1), tflops=round(2.0 * n * G * D / us / 1e6, 2),
                speedup=round(r["matmul_topk"]["us"] / us, 3), same_index_set_share=round(float(same), 4))
        del g, gh, gi, si
    B, S = a.batch, a.hw
    x = torch.randn((B, 3, S, S), device="cuda", generator=gen)
    for precision in () if a.skip_model else ("f32", "f16"):
        m = ore.Model(ctx, squeezenet.build(S), max_batch=B, precision=precision)
        m.set_streams(2)
        m.set_topk(K)
        m.autotune(x, torch.empty((B, m.output_elems), device="cuda"))
        scores = torch.empty((B, K), dtype=torch.float32, device="cuda")
        classes = torch.empty((B, K), dtype=torch.int32, device="cuda")
        emb = torch.empty((B, m.embed_dim), dtype=torch.float32, device="cuda")
        # on <-> off replans, so the two settings are timed one after the other, off - on - off
        off1 = alternate({"classify_into": (lambda: m.classify_into(x, scores, classes), 10)}, a.rounds)["classify_into"]
        m.set_embed_output(emb)
        on = alternate({"classify_into": (lambda: m.classify_into(x, scores, classes), 10)}, a.rounds)["classify_into"]
        m.set_embed_output(None)
        off2 = alternate({"classify_into": (lambda: m.classify_into(x, scores, classes), 10)}, a.rounds)["classify_into"]
        res["model"][precision] = {"embed_off": off1, "embed_on": on, "embed_off_again": off2,
                                   "added_us": round(on["us"] - (off1["us"] + off2["us"]) / 2, 2)}
        m.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
