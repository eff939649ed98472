#!/usr/bin/env python3
"""Cost of the boxes of the class activation maps on the GPU: prints one JSON line.
SqueezeNet at --hw, --batch images, k = 5, f32 and f16:
 (a) the box kernel alone (ore_cam_boxes_f32, frac 0.2) on the model's own maps of a random uint8 batch, and on a
     worst-case set: planes of alternating coarse cells (a 13 x 13 checkerboard, whose upsampled mask is one
     component wound through the whole plane); the upsample kernel alone beside them, with its GB/s over the bytes
     it writes;
 (b) Model.classify_into with maps + boxes set against maps only, same model, max_batch = batch, autotuned,
     set_streams(2): the added microseconds are the cost of the feature;
 (c) what a caller did before, both from the maps on the device: a download of the maps plus F.interpolate,
     threshold and scipy.ndimage.label on the host; and F.interpolate + threshold on the device, a download of the
     masks and scipy.ndimage.label on the host.  Wall-clock, synchronised, --host-rounds times.
Every device figure is the median over --rounds windows of back-to-back calls timed by HIP events on the context
stream, with the smallest and largest window beside it; the variants of one comparison alternate inside a round, so
drift of the shared machine lands on all of them.  Needs an MI355X (no fallback); (c) needs scipy and is left out
without it.
usage: python tools/bench_cam_boxes.py [--batch 256] [--hw 224] [--rounds 9] [--host-rounds 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_ingest import alternate  # noqa: E402  (the same windows and alternation)

K = 5
FRAC = 0.2


def host_boxes(masks):
    """the largest 8-connected component's box per boolean mask, by scipy"""
    import numpy as np
    from scipy import ndimage
    out = np.zeros((len(masks), 4), np.int32)
    for i, mask in enumerate(masks):
        lab, n = ndimage.label(mask, np.ones((3, 3)))
        if n:
            best = int(np.argmax(np.bincount(lab.ravel())[1:])) + 1
            sl = ndimage.find_objects(lab, best)[best - 1]
            out[i] = (sl[0].start, sl[1].start, sl[0].stop, sl[1].stop)
    return out


def wall_us(fn, rounds):
    import torch
    t = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import ore
    from ore import squeezenet
    from ore._lib import check
    if not torch.cuda.is_available():
        sys.exit("bench_cam_boxes.py: no GPU visible")
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    B, S = a.batch, a.hw
    ctx = ore.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1000)
    x8 = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=g)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    scale, shift = (np.float32(1) / (np.float32(255) * std)).astype(np.float32), (-mean / std).astype(np.float32)
    xf = ore.preprocess_u8(ctx, x8, scale, shift)
    onnx = squeezenet.build(S)
    L = ore.load()
    res = {"tool": "bench_cam_boxes", "batch": B, "hw": S, "rounds": a.rounds, "host_rounds": a.host_rounds, "k": K, "frac": FRAC,
           "kernel": {}, "model": {}, "before": {}}

    own_maps = None
    for precision in ("f32", "f16"):
        m = ore.Model(ctx, onnx, max_batch=B, precision=precision)
        m.set_streams(2)
        m.set_topk(K)
        hm, wm = m.cam_hw
        out = torch.empty((B, m.output_elems), device="cuda")
        scores = torch.empty((B, K), dtype=torch.float32, device="cuda")
        classes = torch.empty((B, K), dtype=torch.int32, device="cuda")
        maps = torch.empty((B, K, hm, wm), dtype=torch.float32, device="cuda")
        boxes = torch.empty((B, K, 4), dtype=torch.int32, device="cuda")
        areas = torch.empty((B, K), dtype=torch.int32, device="cuda")
        m.autotune(xf, out)
        m.set_cam_output(maps)

        def classify():
            m.classify_into(xf, scores, classes)

        # the two settings of one model alternate inside a round: turning the boxes on or off does not replan
        def with_boxes():
            m.set_cam_boxes(boxes, areas, FRAC)
            m.classify_into(xf, scores, classes)
            m.set_cam_boxes(None)

        r = alternate({"classify_into_maps": (classify, 10), "classify_into_maps_boxes": (with_boxes, 10)}, a.rounds)
        d = r["classify_into_maps_boxes"]["us"] - r["classify_into_maps"]["us"]
        m.set_cam_boxes(boxes, areas, FRAC)
        classify()
        torch.cuda.synchronize()
        wb, wa = ore.cam_boxes(ctx, maps, (S, S), FRAC)
        res["model"][precision] = dict(r, added_us=round(d, 2), added_pct=round(100.0 * d / r["classify_into_maps"]["us"], 3),
                                       equal_the_kernel_alone=bool(torch.equal(wb, boxes) and torch.equal(wa, areas)),
                                       mean_area_share=round(float(areas.float().mean()) / (S * S), 4))
        if precision == "f32":
            own_maps = maps.clone()
        m.set_cam_output(None)
        m.close()

    # (a) the kernels alone
    hm, wm = own_maps.shape[2:]
    cells = (torch.arange(hm, device="cuda")[:, None] + torch.arange(wm, device="cuda")[None, :]) % 2
    worst = cells.to(torch.float32)[None, None].expand(B, K, hm, wm).contiguous()
    up = torch.empty((B, K, S, S), dtype=torch.float32, device="cuda")
    for name, mp in (("own_maps", own_maps), ("alternating_cells", worst)):
        bx = torch.empty((B, K, 4), dtype=torch.int32, device="cuda")
        ar = torch.empty((B, K), dtype=torch.int32, device="cuda")
        ptr = [ctypes.c_void_p(t.data_ptr()) for t in (mp, bx, ar, up)]

        def box_kernel():
            check(L.ore_cam_boxes_f32(ctx.h, ptr[0], B * K, hm, wm, S, S, FRAC, ptr[1], ptr[2]), ctx.h)

        def up_kernel():
            check(L.ore_upsample_maps_f32(ctx.h, ptr[0], B * K, hm, wm, S, S, ptr[3]), ctx.h)

        r = alternate({"cam_boxes": (box_kernel, 20), "upsample_maps": (up_kernel, 20)}, a.rounds)
        torch.cuda.synchronize()
        res["kernel"][name] = dict(r, planes=B * K, mean_area_share=round(float(ar.float().mean()) / (S * S), 4),
                                   upsample_write_gbs=round(up.numel() * 4 / r["upsample_maps"]["us"] / 1e3, 1))

    # (c) what a caller did before
    if have_scipy:
        flat = own_maps.reshape(B * K, 1, hm, wm)

        def masks_on_device():
            u = F.interpolate(flat, size=(S, S), mode="bilinear", align_corners=False)[:, 0]
            lo, hi = u.amin((1, 2), keepdim=True), u.amax((1, 2), keepdim=True)
            return u >= lo + FRAC * (hi - lo)

        def all_on_host():
            t = own_maps.cpu().reshape(B * K, 1, hm, wm)
            u = F.interpolate(t, size=(S, S), mode="bilinear", align_corners=False)[:, 0]
            lo, hi = u.amin((1, 2), keepdim=True), u.amax((1, 2), keepdim=True)
            return host_boxes((u >= lo + FRAC * (hi - lo)).numpy())

        def device_masks_host_labels():
            return host_boxes(masks_on_device().cpu().numpy())

        ours = ore.cam_boxes(ctx, own_maps, (S, S), FRAC)[0].reshape(-1, 4).cpu().numpy()
        theirs = device_masks_host_labels()
        res["before"] = {"download_interpolate_label_on_the_host": wall_us(all_on_host, a.host_rounds),
                         "interpolate_threshold_on_the_device_label_on_the_host": wall_us(device_masks_host_labels, a.host_rounds),
                         "device_part_alone": alternate({"interpolate_threshold": (masks_on_device, 5)}, a.rounds)["interpolate_threshold"],
                         # F.interpolate rounds differently from the stated arithmetic: a pixel at the threshold may flip
                         "boxes_equal_share": round(float((ours == theirs).all(1).mean()), 4)}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
