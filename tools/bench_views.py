#!/usr/bin/env python3
"""Cost of multi-view classification on the GPU: prints one JSON line.  bench_classify.py's
method (medians of --rounds windows of back-to-back calls timed by HIP events, the variants of one comparison
alternating inside a round).
 (a) ten_view  Ten-crop classification of 25 sources of 375 x 500 (250 list images: short side to 256, the ten
               224 x 224 windows of multi_crop_geometries, the last five mirrored), SqueezeNet at 224, f32 and
               f16, max_batch = 256, autotuned, set_streams(2), k = 5:
                 classify_u8_list_into with set_views(10)   against
                 run_u8_list_into + rows.view(25, 10, D).mean(1) + torch.topk   on the same list
               (what a caller does without the feature).  The classes of the two are compared before timing;
               the download either way is [25, 5] scores and classes, so it is left out.
 (b) ingest    ore_preprocess_list_u8 on 256 images of 375 x 500 (short side to 256, centre crop 224) with
               every other descriptor flipped against the same list unflipped -- timed twice a round
               (unflipped_again), so the spread of one kernel against itself is beside the difference -- plain
               and antialiased, interleaved and NV12.  The flipped output is compared with the unflipped one
               mirrored before timing.
Needs an MI355X (no fallback).
usage: python tools/bench_views.py [--rounds 9] [--no-model] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_ingest import alternate  # noqa: E402  (the same windows and alternation)

K, VIEWS, SOURCES, SHORT, OUT, HS, WS = 5, 10, 25, 256, 224, 375, 500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_views.py: no GPU visible")
    import ore
    from ore import squeezenet
    from ore._lib import check
    from ore.engine import _desc
    ctx = ore.Context(0)
    L = ore.load()
    gen = torch.Generator(device="cuda").manual_seed(1000)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    res = {"tool": "bench_views", "rounds": a.rounds, "k": K, "views": VIEWS, "source": [HS, WS], "short": SHORT,
           "out": [OUT, OUT], "ten_view": {}, "ingest": {}}

    # ---- (a) ten-crop classification
    if not a.no_model:
        n = SOURCES * VIEWS
        src = torch.randint(0, 256, (SOURCES, HS, WS, 3), dtype=torch.uint8, device="cuda", generator=gen)
        ten = ore.multi_crop_geometries((HS, WS), SHORT, (OUT, OUT), VIEWS)
        lst = ore.ImageList(ctx, n, (OUT, OUT), 3).set([src[i // VIEWS] for i in range(n)],
                                                      geometries=[ten[i % VIEWS][:2] for i in range(n)],
                                                      flips=[ten[i % VIEWS][2] for i in range(n)])
        onnx = squeezenet.build(OUT)
        for precision in ("f32", "f16"):
            print(f"bench_views: ten_view {precision}", file=sys.stderr, flush=True)
            m = ore.Model(ctx, onnx, max_batch=256, precision=precision)
            m.set_streams(2)
            m.set_input_norm(scale, shift)
            m.set_topk(K)
            D = m.output_elems
            rows = torch.empty((n, D), device="cuda")
            m.autotune(ore.preprocess_list_u8(ctx, lst, scale, shift), rows)
            m.set_views(VIEWS)
            scores = torch.empty((SOURCES, K), dtype=torch.float32, device="cuda")
            classes = torch.empty((SOURCES, K), dtype=torch.int32, device="cuda")

            def views_classify():
                m.classify_u8_list_into(lst, scores, classes)

            def rows_mean_topk():
                m.run_u8_list_into(lst, rows)
                return torch.topk(rows.view(SOURCES, VIEWS, D).mean(1), K, dim=1, sorted=True)

            views_classify()
            tv, ti = rows_mean_topk()
            torch.cuda.synchronize()
            equal = bool(torch.equal(ti.to(torch.int32), classes))  # torch's mean sums in another order: the classes
            close = float((tv - scores).abs().max())                 # must agree, the scores to rounding
            r = alternate({"views_classify": (views_classify, 10), "rows_mean_topk": (rows_mean_topk, 10),
                           "run_u8_list_into": (lambda: m.run_u8_list_into(lst, rows), 10)}, a.rounds)
            res["ten_view"][precision] = dict(
                r, images=n, subjects=SOURCES, classes_equal=equal, scores_max_abs_diff=close,
                rows_mean_topk_over_views_classify=round(r["rows_mean_topk"]["us"] / r["views_classify"]["us"], 4),
                selection_added_us=round(r["views_classify"]["us"] - r["run_u8_list_into"]["us"], 2),
                framework_added_us=round(r["rows_mean_topk"]["us"] - r["run_u8_list_into"]["us"], 2))
            m.close()
        torch.cuda.synchronize()
        lst.close()
        del src

    # ---- (b) list ingest, every other descriptor flipped
    B = 256
    Fl = ctypes.c_float * 3
    sc_c, sh_c = Fl(*scale.tolist()), Fl(*shift.tolist())
    hc, wc = (HS + 1) // 2, (WS + 1) // 2
    rgb = torch.randint(0, 256, (B, HS, WS, 3), dtype=torch.uint8, device="cuda", generator=gen)
    yp = torch.randint(0, 256, (B, HS, WS), dtype=torch.uint8, device="cuda", generator=gen)
    uvp = torch.randint(0, 256, (B, hc, wc, 2), dtype=torch.uint8, device="cuda", generator=gen)
    y0 = torch.empty((B, 3, OUT, OUT), dtype=torch.float32, device="cuda")
    y1 = torch.empty_like(y0)
    d0, d1 = _desc(y0), _desc(y1)
    flips = [i % 2 == 1 for i in range(B)]
    for fmt in ("interleaved", "nv12"):
        srcs = [rgb[i] for i in range(B)] if fmt == "interleaved" else [(yp[i], uvp[i]) for i in range(B)]
        for antialias in (False, True):
            name = f"{fmt}_{'aa' if antialias else 'bilinear'}"
            print(f"bench_views: ingest {name}", file=sys.stderr, flush=True)
            make = (lambda: ore.ImageList(ctx, B, (OUT, OUT), 3, antialias)) if fmt == "interleaved" else \
                (lambda: ore.Nv12ImageList(ctx, B, (OUT, OUT), "bt601", antialias))
            plain = make().set(srcs, short=SHORT)
            mixed = make().set(srcs, short=SHORT, flips=flips)

            def unflipped():
                check(L.ore_preprocess_list_u8(ctx.h, plain.h, sc_c, sh_c, 0, ctypes.byref(d0)), ctx.h)

            def flipped_alternate():
                check(L.ore_preprocess_list_u8(ctx.h, mixed.h, sc_c, sh_c, 0, ctypes.byref(d1)), ctx.h)

            unflipped()
            flipped_alternate()
            torch.cuda.synchronize()
            equal = bool(torch.equal(y1[0::2], y0[0::2]) and torch.equal(y1[1::2], y0[1::2].flip(-1)))
            reps = 10 if antialias else 30
            r = alternate({"unflipped": (unflipped, reps), "flipped_alternate": (flipped_alternate, reps),
                           "unflipped_again": (unflipped, reps)}, a.rounds)
            res["ingest"][name] = dict(
                r, images=B, flipped_equals_unflipped_mirrored=equal,
                flipped_over_unflipped=round(r["flipped_alternate"]["us"] / r["unflipped"]["us"], 4),
                unflipped_again_over_unflipped=round(r["unflipped_again"]["us"] / r["unflipped"]["us"], 4))
            torch.cuda.synchronize()
            plain.close()
            mixed.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
