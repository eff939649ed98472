#!/usr/bin/env python3
"""Cost of oriented image lists on the GPU: prints one JSON line.  bench_views.py's method (medians
of --rounds windows of back-to-back ore_preprocess_list_u8 calls timed by HIP events, the variants of one comparison
alternating inside a round).  Two geometries -- 256 images of 375 x 500, short side to 256, centre crop 224; 64
frames of 1080 x 1920, short side to 224, centre crop 224 -- the four filters, interleaved RGB and NV12:
 unoriented   the list set through set() (`plain`, timed twice a round: `plain_again` is the spread of one kernel
              against itself) and, where the package has it, through set_oriented with every code 1 (`ones`), which
              must launch the same kernels.  --unoriented-only stops here, and --pkg points the tool at another
              checkout's package (the parent commit's, which has no set_oriented) for the same lists in the same
              session.
 oriented     every code 6 (`all6`: displayed 500 x 375 / 1920 x 1080, the short side and the crop in displayed space)
              and codes 6 and 1 alternating (`half6`), against what a caller does without the feature: a physical
              rotation of the source bytes in torch, x.transpose(1, 2).flip(2).contiguous() over the whole batch (one
              pass per plane for NV12), followed by the unoriented list of the rotated images (`rotate_then_list`;
              `list_of_rotated` is that list alone, the rotation already paid).  The oriented output is compared with
              the rotated list's before timing: they agree to rounding, not bit for bit -- and NV12
              with an odd height pairs its chroma differently after a rotation of the planes, so that figure is larger.
Needs an MI355X (no fallback).
usage: python tools/bench_orient.py [--rounds 9] [--unoriented-only] [--pkg DIR] [--label NAME] [--only photo|video] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_ingest import alternate  # noqa: E402  (the same windows and alternation)

OUT = 224
GEOMETRIES = {"photo": (256, 375, 500, 256), "video": (64, 1080, 1920, 224)}  # images, hs, ws, short side
FILTERS = {"bilinear": (False, False), "aa": (True, False), "bicubic": (False, True), "bicubic_aa": (True, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--unoriented-only", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
    ap.add_argument("--only", default="")
    ap.add_argument("--label", default="", help="what the result line calls the package (default: its path from the repository)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_orient.py: no GPU visible")
    import ore
    from ore._lib import check
    from ore.engine import _desc
    has_orient = hasattr(ore.ImageList, "set_oriented")
    if not has_orient and not a.unoriented_only:
        sys.exit("bench_orient.py: this package has no set_oriented (use --unoriented-only)")
    ctx = ore.Context(0)
    L = ore.load()
    gen = torch.Generator(device="cuda").manual_seed(1000)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    Fl = ctypes.c_float * 3
    sc_c, sh_c = Fl(*scale.tolist()), Fl(*shift.tolist())
    res = {"tool": "bench_orient", "rounds": a.rounds, "package": a.label or os.path.relpath(os.path.abspath(a.pkg), REPO), "set_oriented": has_orient,
           "out": [OUT, OUT], "geometries": {k: list(v) for k, v in GEOMETRIES.items()}, "results": {}}

    for gname, (B, HS, WS, SHORT) in GEOMETRIES.items():
        if a.only and a.only != gname:
            continue
        hc, wc = (HS + 1) // 2, (WS + 1) // 2
        rgb = torch.randint(0, 256, (B, HS, WS, 3), dtype=torch.uint8, device="cuda", generator=gen)
        yp = torch.randint(0, 256, (B, HS, WS), dtype=torch.uint8, device="cuda", generator=gen)
        uvp = torch.randint(0, 256, (B, hc, wc, 2), dtype=torch.uint8, device="cuda", generator=gen)
        y0 = torch.empty((B, 3, OUT, OUT), dtype=torch.float32, device="cuda")
        y1, y2 = torch.empty_like(y0), torch.empty_like(y0)
        d0, d1, d2 = _desc(y0), _desc(y1), _desc(y2)
        if not a.unoriented_only:  # the rotation's destination, allocated once as a caller's pipeline would
            rgb_r = torch.empty((B, WS, HS, 3), dtype=torch.uint8, device="cuda")
            yp_r = torch.empty((B, WS, HS), dtype=torch.uint8, device="cuda")
            uvp_r = torch.empty((B, wc, hc, 2), dtype=torch.uint8, device="cuda")
        for fmt in ("interleaved", "nv12"):
            srcs = [rgb[i] for i in range(B)] if fmt == "interleaved" else [(yp[i], uvp[i]) for i in range(B)]
            for fname, (antialias, cubic) in FILTERS.items():
                name = f"{gname}_{fmt}_{fname}"
                print(f"bench_orient: {name}", file=sys.stderr, flush=True)
                make = (lambda: ore.ImageList(ctx, B, (OUT, OUT), 3, antialias, cubic)) if fmt == "interleaved" else \
                    (lambda: ore.Nv12ImageList(ctx, B, (OUT, OUT), "bt601", antialias, cubic))

                def run(lst, d):
                    return lambda: check(L.ore_preprocess_list_u8(ctx.h, lst.h, sc_c, sh_c, 0, ctypes.byref(d)), ctx.h)

                reps = 10 if antialias else 30
                lists = [make().set(srcs, short=SHORT)]
                variants = {"plain": (run(lists[0], d0), reps)}
                out = {"images": B}
                if has_orient:
                    lists.append(make().set_oriented(srcs, [1] * B, short=SHORT))
                    variants["ones"] = (run(lists[-1], d1), reps)
                variants["plain_again"] = (run(lists[0], d0), reps)
                if has_orient:
                    variants["plain"][0]()
                    variants["ones"][0]()
                    torch.cuda.synchronize()
                    out["ones_equals_plain"] = bool(torch.equal(y1, y0))
                if not a.unoriented_only:
                    all6 = make().set_oriented(srcs, [6] * B, short=SHORT)
                    half = make().set_oriented(srcs, [6 if i % 2 == 0 else 1 for i in range(B)], short=SHORT)
                    if fmt == "interleaved":
                        def rotate():
                            rgb_r.copy_(rgb.transpose(1, 2).flip(2))
                        rotated = make().set([rgb_r[i] for i in range(B)], short=SHORT)
                    else:
                        def rotate():
                            yp_r.copy_(yp.transpose(1, 2).flip(2))
                            uvp_r.copy_(uvp.transpose(1, 2).flip(2))
                        rotated = make().set([(yp_r[i], uvp_r[i]) for i in range(B)], short=SHORT)
                    lists += [all6, half, rotated]
                    run_rot = run(rotated, d2)

                    def rotate_then_list():
                        rotate()
                        run_rot()

                    rotate_then_list()
                    run(all6, d1)()
                    torch.cuda.synchronize()
                    out["all6_vs_rotated_max_abs"] = float((y1 - y2).abs().max())
                    variants.update({"all6": (run(all6, d1), reps), "half6": (run(half, d1), reps),
                                     "rotate_then_list": (rotate_then_list, reps), "list_of_rotated": (run_rot, reps)})
                r = alternate(variants, a.rounds)
                out.update(r)
                out["plain_again_over_plain"] = round(r["plain_again"]["us"] / r["plain"]["us"], 4)
                if has_orient:
                    out["ones_over_plain"] = round(r["ones"]["us"] / r["plain"]["us"], 4)
                if not a.unoriented_only:
                    out["all6_over_plain"] = round(r["all6"]["us"] / r["plain"]["us"], 4)
                    out["half6_over_plain"] = round(r["half6"]["us"] / r["plain"]["us"], 4)
                    out["rotate_then_list_over_all6"] = round(r["rotate_then_list"]["us"] / r["all6"]["us"], 4)
                res["results"][name] = out
                torch.cuda.synchronize()
                for lst in lists:
                    lst.close()
        del rgb, yp, uvp, y0, y1, y2
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
