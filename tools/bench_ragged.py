#!/usr/bin/env python3
"""Cost of an image list against the dense resize and against one call per image: prints one
JSON line.  bench_resize.py's method (medians of --rounds windows of back-to-back calls timed by HIP events,
the variants of one comparison alternating inside a round).
 uniform   256 images of 375 x 500 x 3 -> 256 x 341, centre crop 224, all in one buffer:
   (a) ore_preprocess_list_u8 on a list of the 256 images;
   (b) ore_preprocess_resize_u8 on the same bytes as one dense batch;
   (c) what a caller without the list does: 256 calls of ore_preprocess_resize_u8 with n = 1 into slices of y.
 mixed     256 images with heights and widths drawn from 333..500 (seeded), geometry by short = 256:
   (a) and (c) again (no dense batch exists).
 model     Model.run_u8_into (dense, set_input_resize) against Model.run_u8_list_into on the uniform set, f32
           and f16, max_batch = 256, autotuned, set_streams(2).
Every variant's output is compared with (a)'s before it is timed.  Needs an MI355X (no fallback).
usage: python tools/bench_ragged.py [--rounds 9] [--no-model] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ingest import alternate  # noqa: E402

B, HS, WS, C, SHORT, OUT = 256, 375, 500, 3, 256, 224


def per_image_calls(ctx, L, imgs, geoms, y, sc_c, sh_c):
    """(c): one ore_preprocess_resize_u8 call per image, n = 1, into image i of y; the arguments are made once."""
    from ore._lib import Resize, Tensor, check
    calls = []
    for i, (x, (resized, origin)) in enumerate(zip(imgs, geoms)):
        t = Tensor()
        t.data, t.ndim, t.nstride = y[i].data_ptr(), 4, 0
        for k, d in enumerate((1, C, OUT, OUT)):
            t.dims[k] = d
        calls.append((ctypes.c_void_p(x.data_ptr()), int(x.shape[0]), int(x.shape[1]), Resize(*resized, *origin), t))

    def run():
        for xp, hs, ws, g, t in calls:
            check(L.ore_preprocess_resize_u8(ctx.h, xp, 1, hs, ws, C, ctypes.byref(g), sc_c, sh_c, 0, ctypes.byref(t)), ctx.h)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ragged.py: no GPU visible")
    import ore
    from ore import squeezenet
    from ore._lib import Resize, check
    from ore.engine import _desc
    ctx = ore.Context(0)
    L = ore.load()
    gen = torch.Generator(device="cuda").manual_seed(1000)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    Fl = ctypes.c_float * 3
    sc_c, sh_c = Fl(*scale.tolist()), Fl(*shift.tolist())
    y = torch.empty((B, C, OUT, OUT), dtype=torch.float32, device="cuda")
    y_other = torch.empty_like(y)
    yd, yod = _desc(y), _desc(y_other)
    res = {"tool": "bench_ragged", "rounds": a.rounds, "batch": B, "out": [OUT, OUT]}

    # ---- uniform set
    x8 = torch.randint(0, 256, (B, HS, WS, C), dtype=torch.uint8, device="cuda", generator=gen)
    geom = ore.center_crop_geometry((HS, WS), SHORT, (OUT, OUT))
    (rh, rw), (top, left) = geom
    g_c = Resize(rh, rw, top, left)
    xp = ctypes.c_void_p(x8.data_ptr())
    uni = ore.ImageList(ctx, B, (OUT, OUT), C).set([x8[i] for i in range(B)], short=SHORT)
    mixed = ore.ImageList(ctx, B, (OUT, OUT), C)

    def list_uniform():
        check(L.ore_preprocess_list_u8(ctx.h, uni.h, sc_c, sh_c, 0, ctypes.byref(yd)), ctx.h)

    def dense():
        check(L.ore_preprocess_resize_u8(ctx.h, xp, B, HS, WS, C, ctypes.byref(g_c), sc_c, sh_c, 0, ctypes.byref(yod)), ctx.h)

    calls_uniform = per_image_calls(ctx, L, [x8[i] for i in range(B)], [geom] * B, y_other, sc_c, sh_c)
    print("bench_ragged: uniform", file=sys.stderr, flush=True)
    list_uniform()
    dense()
    eq_dense = bool(torch.equal(y, y_other))
    y_other.zero_()
    calls_uniform()
    eq_calls = bool(torch.equal(y, y_other))
    r = alternate({"list": (list_uniform, 30), "dense": (dense, 30), "per_image_calls": (calls_uniform, 3)}, a.rounds)
    res["uniform"] = {"shape": [B, HS, WS, C], "resized": [rh, rw], "origin": [top, left], **r,
                      "list_equals_dense": eq_dense, "list_equals_per_image_calls": eq_calls,
                      "list_over_dense": round(r["list"]["us"] / r["dense"]["us"], 4),
                      "per_image_calls_over_list": round(r["per_image_calls"]["us"] / r["list"]["us"], 2)}

    # ---- mixed set: sizes 333..500, seeded; geometry by short = 256
    rng = np.random.default_rng(1000)
    sizes = [(int(h), int(w)) for h, w in rng.integers(333, 501, size=(B, 2))]
    imgs = [torch.randint(0, 256, (h, w, C), dtype=torch.uint8, device="cuda", generator=gen) for h, w in sizes]
    geoms = [ore.center_crop_geometry(s, SHORT, (OUT, OUT)) for s in sizes]
    mixed.set(imgs, short=SHORT)

    def list_mixed():
        check(L.ore_preprocess_list_u8(ctx.h, mixed.h, sc_c, sh_c, 0, ctypes.byref(yd)), ctx.h)

    calls_mixed = per_image_calls(ctx, L, imgs, geoms, y_other, sc_c, sh_c)
    print("bench_ragged: mixed", file=sys.stderr, flush=True)
    list_mixed()
    y_other.zero_()
    calls_mixed()
    eq_calls = bool(torch.equal(y, y_other))
    r = alternate({"list": (list_mixed, 30), "per_image_calls": (calls_mixed, 3)}, a.rounds)
    res["mixed"] = {"sizes": "333..500, numpy default_rng(1000)", "source_bytes": int(sum(h * w * C for h, w in sizes)), **r,
                    "list_equals_per_image_calls": eq_calls,
                    "per_image_calls_over_list": round(r["per_image_calls"]["us"] / r["list"]["us"], 2)}
    del y_other

    # ---- the model's step, dense against list, on the uniform set
    if not a.no_model:
        onnx = squeezenet.build(OUT)
        xf = ore.preprocess_resize_u8(ctx, x8, (OUT, OUT), (rh, rw), (top, left), scale, shift)
        res["model"] = {}
        for precision in ("f32", "f16"):
            print(f"bench_ragged: model {precision}", file=sys.stderr, flush=True)
            m = ore.Model(ctx, onnx, max_batch=B, precision=precision)
            m.set_streams(2)
            m.set_input_norm(scale, shift)
            m.set_input_resize((HS, WS), (rh, rw), (top, left))
            out = torch.empty((B, m.output_elems), device="cuda")
            out_l = torch.empty_like(out)
            m.autotune(xf, out)

            def run_dense():
                m.run_u8_into(x8, out)

            def run_list():
                m.run_u8_list_into(uni, out_l)

            run_dense()
            run_list()
            equal = bool(torch.equal(out, out_l))
            r = alternate({"run_u8_into": (run_dense, 10), "run_u8_list_into": (run_list, 10)}, a.rounds)
            d = r["run_u8_list_into"]["us"] - r["run_u8_into"]["us"]
            res["model"][precision] = {**r, "outputs_equal": equal, "list_added_us": round(d, 2),
                                       "list_over_dense": round(r["run_u8_list_into"]["us"] / r["run_u8_into"]["us"], 4)}
            m.close()
        del xf
    torch.cuda.synchronize()
    uni.close()
    mixed.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
