#!/usr/bin/env python3
"""SqueezeNet-1.0 fp32 images/s on MI355X (BASELINE.json metric), one process per GPU.

A step = one pass of the whole 66-node graph over one batch of 256 synthetic 3x224x224 images
already resident in HBM (per GPU: weak scaling), plus, for N > 1, the RCCL all-gather of the
[256, 1000] softmax rows (the only collective, BASELINE.json north_star).  Prints one JSON line
on rank 0.  A plain run sets up (model, seeded batch, per-layer tile autotune), warms up, times the
K steps and prints the headline figure; --full adds everything else: the roofline of the dominant
kernel (the MFMA implicit-GEMM conv) from a per-kernel HIP-event pass, the max-abs sample against
the oracle, the fp16 line, the batch-1 latency probe and the CPU baseline (the C restatement of
the reference's algorithm, timed on this host's cores).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
  python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N
"""
import argparse
import json
import os
import sys
import threading
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, REPO)

METRIC = "SqueezeNet-1.0 fp32 images/s at batch 256, 1/2/4/8 MI355X; max-abs diff vs CPU"
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: f32 MFMA dense peak (= f32 vector peak)
PEAK_F16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: f16/bf16 MFMA dense peak (no sparsity)
PEAK_HBM_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E spec peak
# achievable peaks ("measure achievable peaks (copy kernel, MFMA loop) and report
# both"): MI355X_MICROARCH.md's measured figures where it has one -- f32 MFMA 155 TF/s
# (v_mfma_f32_32x32x2_f32 / 16x16x4_f32 back to back, 99 % of spec) and 6.29 TB/s (float4 copy) --
# and this repo's probe for the f16 MFMA loop, which the guide does not measure (tools/peaks.sh,
# profiles/r01_peaks.txt); this repo's read / write streams for reference (profiles/r03k_hbm_probe.txt)
ACHIEVABLE = {"f32_mfma_TFLOP/s": 155.0, "f16_mfma_TFLOP/s": 2037.6, "hbm_copy_GB/s": 6290.0,
              "hbm_read_GB/s": 6149.0, "hbm_write_GB/s": 4634.0,
              "source": "MI355X_MICROARCH.md (f32 MFMA 155 TF/s, float4 copy 6.29 TB/s); f16 MFMA loop and "
                        "read / write streams: this repo's probes (profiles/r01_peaks.txt, r03k_hbm_probe.txt)"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="images per GPU per step (weak scaling)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="strong scaling: this many images per step split over the GPUs (SURVEY §8(d) B=2048)")
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--full", action="store_true",
                    help="also run the reporting legs after the timed steps: the per-kernel HIP-event pass (roofline, "
                         "breakdown, --layers), the max-abs sample vs the oracle, and at N = 1 the fp16 line, the batch-1 "
                         "latency probe and the CPU baseline (each leg has its own --no-... switch)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps write what the last timed step returned -- the [G, 1000] softmax rows "
                         "(gathered over the ranks for N > 1) -- as DIR/probs.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="0 = every CPU this process may use (affinity and cgroup quota; see usable_cpus)")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                    help="N > 1 collective: nccl = RCCL all_gather of the device rows (the product path); gloo = the "
                         "rows staged through host memory (exercises the N > 1 branch with several ranks on one GPU)")
    ap.add_argument("--dist", action="store_true",
                    help="take the N > 1 path (process group, per-step all-gather, max over ranks) even at N = 1: a "
                         "one-rank RCCL communicator runs the product collective on a one-GPU box")
    ap.add_argument("--no-step-timing", action="store_true",
                    help="--full: skip the per-kernel HIP-event pass (no roofline / breakdown)")
    ap.add_argument("--layers", action="store_true", help="--full: print per-kernel-step times to stderr")
    ap.add_argument("--no-b1", action="store_true", help="--full: skip the batch-1 latency probe")
    ap.add_argument("--graph", action="store_true", help="time one HIP-graph replay per step instead of plain launches")
    ap.add_argument("--no-autotune", action="store_true", help="keep the heuristic per-layer conv tiles")
    ap.add_argument("--tune-reps", type=int, default=3, help="timed launches per autotune candidate")
    ap.add_argument("--dump-steps", default="", help="write the plan's kernel steps (op, name, flops, bytes) as JSON")
    ap.add_argument("--streams", type=int, default=2,
                    help="ore_model_set_streams: 2 (default) runs independent neighbouring steps -- the split fire "
                         "modules' expand1x1 beside their Winograd expand3x3 -- on a side stream (bit-identical; "
                         "71.1 k vs 70.5 k img/s at B = 256); 1: one stream")
    ap.add_argument("--no-f16-line", action="store_true",
                    help="--full: skip the config-5 fp16 measurement reported under \"f16\" of the f32 line (run at N = 1 "
                         "only, like the batch-1 probe and the CPU baseline)")
    ap.add_argument("--no-winograd", action="store_true",
                    help="f32: 3x3 stride-1 convs on the direct kernels only (ORE_LOAD_NO_WINOGRAD)")
    ap.add_argument("--fusion", type=int, default=None, help="ore_model_set_fusion flags (experiments; default: the model's)")
    ap.add_argument("--precision", choices=["f32", "f16"], default="f32",
                    help="f32: convs on the f32-input MFMA (the headline); f16: the fp16 variant (SURVEY.md §8(f)3, "
                         "config 5)")
    return ap.parse_args()


def lib_sha256():
    """sha256 of the libore.so this process loaded (ties a PMC traffic file to the benched build)."""
    import hashlib
    from ore import _lib
    with open(_lib.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def roofline_8d(infos, per_step_ms, ms_per_step, peak_tflops, peak_gbs=PEAK_HBM_GBS, ach_tflops=None):
    """each launch is bound by its own FLOP:byte ratio, bound_time = max(MFMA FLOPs /
    MFMA peak, algorithmic bytes / HBM peak); frac = bound_time / measured time, per launch, per op
    class and for the whole network (against the timed ms_per_step, launch gaps included).  The FLOPs
    are the MFMA work the kernels issue ("issued"): a direct conv issues its algorithmic 2 C M kh kw
    per output, a Winograd F(2x2, 3x3) layer 16 C M per 2x2 tile instead of the direct 36 C M, so no
    frac can exceed 1.  `effective_frac` beside it credits every layer with the direct-conv FLOPs (a
    Winograd launch's can pass 1: it does less work than it is credited with)."""
    steps, classes = [], {}
    tot_bound = tot_ebound = tot_abound = 0.0
    for info, ms in zip(infos, per_step_ms):
        t_e = info["flops"] / (peak_tflops * 1e12) * 1e3                              # algorithmic (direct)
        t_i = info.get("mfma_flops", info["flops"]) / (peak_tflops * 1e12) * 1e3      # MFMA work issued
        t_b = info["bytes"] / (peak_gbs * 1e9) * 1e3
        bound, ebound = max(t_i, t_b), max(t_e, t_b)
        tot_bound += bound
        tot_ebound += ebound
        if ach_tflops:  # the same bound against the measured achievable peaks (MFMA loop, copy rate)
            tot_abound += max(info.get("mfma_flops", info["flops"]) / (ach_tflops * 1e12) * 1e3,
                              info["bytes"] / (ACHIEVABLE["hbm_copy_GB/s"] * 1e9) * 1e3)
        kind = "mfma" if t_i >= t_b else "hbm"
        steps.append({"name": info["name"], "op": info["op"], "bound": kind, "us": round(1000 * float(ms), 1),
                      "bound_us": round(1000 * bound, 1), "frac": round(bound / max(float(ms), 1e-9), 3),
                      "effective_frac": round(ebound / max(float(ms), 1e-9), 3)})
        c = classes.setdefault(info["op"], {"ms": 0.0, "bound_ms": 0.0, "ebound_ms": 0.0, "flops": 0.0,
                                            "mfma_flops": 0.0, "bytes": 0.0, "launches": 0})
        c["ms"] += float(ms)
        c["bound_ms"] += bound
        c["ebound_ms"] += ebound
        c["flops"] += info["flops"]
        c["mfma_flops"] += info.get("mfma_flops", info["flops"])
        c["bytes"] += info["bytes"]
        c["launches"] += 1
    per_class = {}
    for k, c in classes.items():
        per_class[k] = {"launches": c["launches"], "ms": round(c["ms"], 4), "bound_ms": round(c["bound_ms"], 4),
                        "frac": round(c["bound_ms"] / max(c["ms"], 1e-9), 4),
                        "effective_frac": round(c["ebound_ms"] / max(c["ms"], 1e-9), 4),
                        "issued_TFLOP/s": round(c["mfma_flops"] / (c["ms"] * 1e-3) / 1e12, 2) if c["flops"] else None,
                        "effective_TFLOP/s": round(c["flops"] / (c["ms"] * 1e-3) / 1e12, 2) if c["flops"] else None,
                        "GB/s": round(c["bytes"] / (c["ms"] * 1e-3) / 1e9, 1)}
    net = {"bound_ms": round(tot_bound, 4), "ms_per_step": round(ms_per_step, 4),
           "frac": round(tot_bound / ms_per_step, 4),
           "effective_bound_ms": round(tot_ebound, 4), "effective_frac": round(tot_ebound / ms_per_step, 4),
           "kernel_ms": round(float(sum(per_step_ms)), 4)}
    peaks = {"mfma_TFLOP/s": peak_tflops, "hbm_GB/s": peak_gbs}
    if ach_tflops:
        net["achievable_bound_ms"] = round(tot_abound, 4)
        net["achievable_frac"] = round(tot_abound / ms_per_step, 4)
        peaks["achievable"] = dict(ACHIEVABLE, used={"mfma_TFLOP/s": ach_tflops, "hbm_GB/s": ACHIEVABLE["hbm_copy_GB/s"]})
    return {"peaks": peaks, "network": net,
            "per_class": per_class, "per_launch": steps}, classes


def usable_cpus():
    """CPUs this process may run on: the affinity mask, capped by a cgroup CPU quota (v2 cpu.max or v1
    cfs_quota / cfs_period) -- on the GPU box os.cpu_count() shows the whole machine, far more than the
    share this job gets.  Returns (usable, details)."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
            if q != "max":
                quota = int(q) / int(p)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                p = int(f.read())
            if q > 0:
                quota = q / p
        except (OSError, ValueError):
            pass
    usable = aff if quota is None else max(1, min(aff, int(quota)))
    return usable, {"host_cpu_count": os.cpu_count(), "affinity_cpus": aff, "cgroup_cpu_quota": quota}


def cpu_baseline(model_bytes, hw, threads):
    """The oracle in the reference's cost structure (per-dot heap buffer, im2col, weights decoded
    per op call), one independent batch-1 image per thread — timed on this host."""
    import numpy as np
    import oracle
    from ore import squeezenet
    x = squeezenet.synthetic_input(threads, hw, seed=77)
    models = [oracle.Model(model_bytes) for _ in range(threads)]
    done = [0.0] * threads

    def work(i):
        t0 = time.perf_counter()
        models[i].run(x[i:i + 1], 1000, faithful=True)
        done[i] = time.perf_counter() - t0

    t0 = time.perf_counter()
    ths = [threading.Thread(target=work, args=(i,)) for i in range(threads)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    wall = time.perf_counter() - t0
    for m in models:
        m.close()
    return {"value": threads / wall, "unit": "images/s", "cores": threads, "kind": "port",
            "sample": f"{threads} SqueezeNet-1.0 224x224 images, one batch-1 inference() per thread, "
                      f"reference cost structure (oracle faithful mode); single-image latency "
                      f"{float(np.median(done)):.2f} s"}


def fixture_images(hw):
    """The 16 images of the strict-parity fixture (zoo image + 15 U(-50, 50) draws) at 224; else none."""
    import numpy as np
    from ore import onnx_wire, squeezenet
    if hw != 224:
        return np.zeros((16, 3, hw, hw), dtype=np.float32)
    # = tests/golden/make_golden.py squeezenet_inputs_calib16()
    zoo = onnx_wire.load_tensor(os.path.join(REPO, "tests", "golden", "squeezenet_data_0.pb")).to_numpy()
    return np.concatenate([zoo, squeezenet.synthetic_input(15, 224, seed=31)]).astype(np.float32)


def b1_latency(model_bytes, hw, local, precision, winograd=True, iters=200):
    """Batch-1 latency (SURVEY.md §8(d) B = 1 config): one image per synchronous call, issued
    as plain launches, as one HIP-graph replay, and as a graph with the fire modules' expand
    branches on two streams (ore_model_set_streams).  Milliseconds per image."""
    import torch
    import ore
    s = torch.cuda.Stream(device=f"cuda:{local}")
    ctx = ore.Context(local, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    x = (torch.rand((1, 3, hw, hw), device=f"cuda:{local}") * 100.0 - 50.0).contiguous()
    res = {}
    for label, streams, graph in (("plain_ms", 1, False), ("graph_ms", 1, True), ("graph_2streams_ms", 2, True)):
        m = ore.Model(ctx, model_bytes, max_batch=1, precision=precision, winograd=winograd)
        m.set_streams(streams)
        out = torch.empty((1, m.output_elems), device=f"cuda:{local}")
        torch.cuda.synchronize()
        m.autotune(x, out)  # batch-1 grids favour other tiles than batch 256
        if graph:
            m.capture(x, out)
        call = m.replay if graph else (lambda: m.run_into(x, out))
        for _ in range(10):
            call()
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
            s.synchronize()
        res[label] = round(1000.0 * (time.perf_counter() - t0) / iters, 4)
        m.close()
    ctx.close()
    return res


def f16_line(ctx, model_bytes, x, B, args, ref, pos):
    """Config 5 (SqueezeNet-1.0 fp16: f16 activations / weights, f32 accumulate) on the same input
    batch, measured like the headline: autotune, warmup, K timed steps, then a HIP-event pass for
    the conv class's TF/s against the 2.5 PF/s f16 peak; max-abs and top-1 against the f32 oracle
    sample.  Reported beside the f32 metric, never as its value."""
    import numpy as np
    import torch
    import ore
    m = ore.Model(ctx, model_bytes, max_batch=B, precision="f16")
    out = torch.empty((B, m.output_elems), dtype=torch.float32, device=x.device)
    m.autotune(x, out)
    for _ in range(args.warmup):
        m.run_into(x, out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        m.run_into(x, out)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    infos = m.steps()
    per = np.zeros(len(infos))
    m.enable_timing(True)
    for _ in range(args.steps):
        m.run_into(x, out)
        per += np.asarray(m.step_times_ms())
    torch.cuda.synchronize()
    m.enable_timing(False)
    per /= args.steps
    conv_ms = sum(p for p, i in zip(per, infos) if i["op"] == "Conv")
    conv_fl = sum(i["flops"] for i in infos if i["op"] == "Conv")
    achieved = conv_fl / (conv_ms * 1e-3) / 1e12
    r8d, _ = roofline_8d(infos, per, 1000.0 * elapsed / args.steps, PEAK_F16_MFMA_TFLOPS,
                         ach_tflops=ACHIEVABLE["f16_mfma_TFLOP/s"])
    y = out[pos].cpu().numpy()  # the fixture images' rows (N = 1: x is the whole global batch)
    res = {"value": round(B * args.steps / elapsed, 2), "unit": "images/s",
           "ms_per_step": round(1000.0 * elapsed / args.steps, 4), "dtype": "f16",
           "conv_TFLOP/s": round(achieved, 2), "roofline_frac": round(achieved / PEAK_F16_MFMA_TFLOPS, 4),
           "conv_launches": sum(1 for i in infos if i["op"] == "Conv"),
           "max_abs_diff_vs_cpu": float(np.abs(y - ref).max()),
           "top1_agrees_with_cpu": bool((y.argmax(1) == ref.argmax(1)).all()),
           "roofline_8d": {"network": r8d["network"], "per_class": r8d["per_class"]},
           "note": "config 5 (BASELINE.json configs[4]) on the same batch; fused f16 kernels, DESIGN.md 3.1.1"}
    m.close()
    return res


DUMP_MAX_BYTES = 64 << 20  # --dump-outputs writes at most this much


def dump_outputs(dirname, rows):
    """--dump-outputs: the rows the last timed step returned, as DIR/probs.npy (float32).  Past 64 MB
    (G > 16 k images) a fixed seeded sample of the rows, in batch order."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    y = np.ascontiguousarray(rows.detach().cpu().numpy(), dtype=np.float32)
    keep = (DUMP_MAX_BYTES - 4096) // y[0].nbytes  # 4096: room for the .npy header
    if len(y) > keep:
        y = y[np.sort(np.random.default_rng(1000).choice(len(y), size=keep, replace=False))]
    np.save(os.path.join(dirname, "probs.npy"), y)


def report_full(result, args, ctx, model_bytes, x, B, dev, world, gathered, sample_idx, x_sample, collective):
    """--full, after the timed steps: the max-abs sample against the oracle and, at N = 1, the fp16
    line, the batch-1 latency probe and the CPU baseline, added to the result line."""
    import numpy as np
    import torch
    import oracle
    f16 = args.precision == "f16"
    # max-abs vs the CPU restatement on a bounded sample: the fixture images at their global positions as
    # they come out of the timed steps (for N > 1 out of the gathered rows, i.e. through the collective)
    torch.cuda.synchronize()
    got = gathered[sample_idx].cpu().numpy()
    ref = oracle.Model(model_bytes).run(x_sample, 1000)
    per_img = np.abs(got - ref).max(axis=1)
    result["max_abs_diff_vs_cpu"] = float(per_img.max())
    result["max_abs_per_image"] = [float(v) for v in per_img]
    result["top1_agrees_with_cpu"] = bool((got.argmax(1) == ref.argmax(1)).all())
    result["max_abs_sample"] = (f"{len(sample_idx)} images at global positions {sample_idx} of the timed batch"
                                f"{' (gathered over ' + collective + ')' if collective else ''}: "
                                f"{'the strict-parity fixture (zoo image + 15 U(-50,50) draws; zoo-calibrated model, softmax max 0.074 on the zoo image)' if args.hw == 224 else 'seeded U(-50,50) images'}"
                                f" vs the oracle (C restatement of the reference, f32) run live on this host")
    result["max_abs_comparability"] = ("zoo-calibrated model (conv10 x ZOO_LOGIT_GAIN) since round 5; rounds 1-4 "
                                       "sampled the uncalibrated He-normal model, whose peakier logits put the "
                                       "same f32 roundings at up to ~1e-5 (DESIGN.md 5.1): not comparable across "
                                       "that change")
    # the reporting legs run at N = 1 only (the CPU baseline on rank 0 at N = 1), so no
    # rank waits on the others' collectives meanwhile
    if world == 1:
        if not f16 and not args.no_f16_line:
            result["f16"] = f16_line(ctx, model_bytes, x, B, args, ref, sample_idx)
        if not args.no_b1:
            result["b1_latency_ms"] = b1_latency(model_bytes, args.hw, dev, args.precision,
                                                 winograd=not args.no_winograd)
        if not args.no_cpu_baseline:
            usable, cpu_info = usable_cpus()
            threads = args.cpu_threads or usable
            result["cpu_baseline"] = cpu_baseline(model_bytes, args.hw, threads)
            result["cpu_baseline"].update(cpu_info, usable_cpus=usable)


def main():
    args = parse()
    import numpy as np
    import torch
    import torch.distributed as dist

    import ore
    from ore import parallel, squeezenet

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print(f"note: --gpus {args.gpus} but WORLD_SIZE {world}; using WORLD_SIZE", file=sys.stderr)
    use_dist = world > 1 or args.dist  # the process group and the per-step all-gather
    gloo = use_dist and args.dist_backend == "gloo"
    # gloo: ranks may share a GPU (the N > 1 branch rehearsed on a one-GPU box); nccl: one GPU per rank
    dev = local % max(1, torch.cuda.device_count()) if gloo else local
    torch.cuda.set_device(dev)
    # one non-default stream for everything (the model's launches, RCCL, torch ops): HIP-graph
    # capture needs a capturable stream
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    if use_dist:
        if gloo:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))

    # one seeded global batch of G images (config 4: --global-batch 2048 split over the GPUs; by
    # default weak scaling, G = world x --batch), generated identically on every rank; each rank
    # keeps its contiguous slice (ore.parallel.shard_bounds) resident in HBM
    strong = args.global_batch > 0
    G = args.global_batch if strong else world * args.batch
    if G % world:
        raise SystemExit(f"--global-batch {G} does not split evenly over {world} GPUs")
    lo, hi = parallel.shard_bounds(G, world, rank)
    B = hi - lo
    # the zoo-calibrated synthetic SqueezeNet (conv10 x ZOO_LOGIT_GAIN: the zoo image's softmax peaks at
    # 0.074 like squeezenet_output_0.pb), so the max-abs sample below sits well above the f32 noise floor
    model_bytes = squeezenet.build_calibrated(args.hw)
    ctx = ore.Context(dev)
    model = ore.Model(ctx, model_bytes, max_batch=B, precision=args.precision, winograd=not args.no_winograd)
    f16 = args.precision == "f16"
    g = torch.Generator(device=f"cuda:{dev}")
    g.manual_seed(1000)
    xg = torch.rand((G, 3, args.hw, args.hw), generator=g, device=f"cuda:{dev}") * 100.0 - 50.0
    # the max-abs sample: the strict-parity fixture images (tests/golden/make_golden.py calib16: the zoo
    # image squeezenet_data_0.pb + 15 U(-50, 50) draws) placed at evenly spread positions of the global
    # batch, so the check covers every rank's gathered rows; other sizes: the seeded images at those positions
    x_sample = fixture_images(args.hw)
    sample_idx = sorted({int(round(i * (G - 1) / max(1, min(G, len(x_sample)) - 1))) for i in range(min(G, len(x_sample)))})
    x_sample = x_sample[:len(sample_idx)]
    if args.hw == 224:
        xg[sample_idx] = torch.from_numpy(x_sample).to(xg.device)
    else:
        x_sample = xg[sample_idx].cpu().numpy()
    x = xg[lo:hi].contiguous()
    del xg
    torch.cuda.empty_cache()
    out = torch.empty((B, model.output_elems), dtype=torch.float32, device=f"cuda:{dev}")
    if not use_dist:
        gathered = out
    elif gloo:  # the rows staged through host memory for the gloo all-gather
        out_host = torch.empty((B, model.output_elems), dtype=torch.float32)
        gathered = torch.empty((G, model.output_elems), dtype=torch.float32)
    else:
        gathered = torch.empty((G, model.output_elems), dtype=torch.float32, device=f"cuda:{dev}")

    if args.fusion is not None:
        model.set_fusion(args.fusion)
    if args.streams != 1:
        model.set_streams(args.streams)
    if not args.no_autotune:  # per-layer conv tile search, outside the timed region
        model.autotune(x, out, reps=args.tune_reps)
    if args.dump_steps and rank == 0:  # kernel-step names for tools/pmc_report.py
        with open(args.dump_steps, "w") as f:
            json.dump(model.steps(), f)

    # --graph: the step's kernels as one HIP graph (ore_model_graph_capture), replayed per step.
    # Measured no faster at B = 256 (69.9 k vs 70.2 k img/s: the 21 launches queue ahead of the GPU),
    # so the default times plain launches
    use_graph = args.graph
    if use_graph:
        model.capture(x, out)

    def step(graph=use_graph):
        if graph:
            model.replay()
        else:
            model.run_into(x, out)
        if use_dist:
            if gloo:
                out_host.copy_(out)
                parallel.gather_rows_into(gathered, out_host)
            else:
                parallel.gather_rows_into(gathered, out)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()

    # the timed region: K steps back to back, nothing else on the stream
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if use_dist:  # the max over ranks
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if gloo else f"cuda:{dev}")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:  # the last timed step's rows, before any other pass writes `out` again
        dump_outputs(args.dump_outputs, gathered)

    # per-kernel durations (roofline, breakdown): the same K steps again with a HIP event on the
    # launch stream between consecutive kernels (ore_model_enable_timing).  A separate pass because
    # the events and the per-step read-back add ~0.12 ms of gaps per step (measured 5.22 vs
    # 5.10 ms) that are not part of the workload; the kernels inside are the same launches.
    timing = args.full and not args.no_step_timing
    infos = model.steps() if timing else []
    per_step_ms = np.zeros(len(infos)) if timing else None
    if timing:
        if args.streams != 1:
            model.set_streams(1)  # the events sit between consecutive launches of one stream
        model.enable_timing(True)
        for _ in range(args.steps):
            model.run_into(x, out)  # the event hooks run between plain launches
            per_step_ms += np.asarray(model.step_times_ms())  # waits on the step's last event only
        torch.cuda.synchronize()
        model.enable_timing(False)
        if args.streams != 1:
            model.set_streams(args.streams)

    if rank == 0:
        value = G * args.steps / elapsed
        result = {
            "metric": METRIC, "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1000.0 * elapsed / args.steps, 4), "higher_is_better": True,
            "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f16" if f16 else "f32",
            "data": "synthetic (seeded U(-50,50) 3x224x224 images with the 16 parity-fixture images inside; seeded "
                    "He-normal SqueezeNet-1.0 weights, conv10 scaled by ZOO_LOGIT_GAIN = "
                    f"{squeezenet.ZOO_LOGIT_GAIN} so the zoo image's softmax peaks at 0.074 as with the real weights)",
            "config": {"workload": f"SqueezeNet-1.0 (66 nodes, 818.9 MMAC/img) "
                                   f"{'fp16 (config 5: f16 activations/weights, f32 accumulate)' if f16 else 'fp32'} "
                                   f"inference, batch {B} per GPU, 3x{args.hw}x{args.hw}",
                       "model": "squeezenet1.0-8 topology, synthetic weights", "global_batch": G,
                       "per_gpu_batch": B, "run_batch": model.run_batch, "seq_len": None, "parallelism": f"dp{world}",
                       "collective": (f"{'gloo (host-staged)' if gloo else 'RCCL'} all_gather of [{B},1000] logits per step"
                                      if use_dist else None),
                       "launch": "one HIP-graph replay per step" if use_graph else "plain launches",
                       "streams": args.streams},
        }
        result["conv_tiles"] = {"autotuned": not args.no_autotune,
                                "tile_per_conv": [ore.Model.TILE_NAMES[t] for t in model.tiles() if t >= 0]}
        if timing:
            per_step_ms /= args.steps
            peak = PEAK_F16_MFMA_TFLOPS if f16 else PEAK_F32_MFMA_TFLOPS
            ach = ACHIEVABLE["f16_mfma_TFLOP/s"] if f16 else ACHIEVABLE["f32_mfma_TFLOP/s"]
            r8d, classes = roofline_8d(infos, per_step_ms, 1000.0 * elapsed / args.steps, peak, ach_tflops=ach)
            conv = classes.get("Conv", {"ms": 1e-9, "flops": 0.0, "mfma_flops": 0.0, "bytes": 0.0, "launches": 1})
            effective = conv["flops"] / (conv["ms"] * 1e-3) / 1e12
            issued = conv["mfma_flops"] / (conv["ms"] * 1e-3) / 1e12
            kname = ("Conv class: conv_band_pool_f16_kernel / conv_pair_pool_f16_kernel (conv1 + pool1 + fire2 "
                     "squeeze straight from the f32 input, band walker or patch kernel per the autotuned tile), "
                     "fire_f16_kernel / fire_pool_f16_kernel (fire module [+ MaxPool] + next squeeze) and "
                     "conv_f16_kernel (implicit GEMM), all MFMA 32x32x16 f16 with f32 accumulate" if f16 else
                     "Conv class: conv_band_pool_f32_kernel / conv_win_pool_f32_kernel (conv1 + pool1 + fire2 squeeze, autotuned), fire_kernel (fire "
                     "module + next squeeze), conv_winol_kernel (Winograd F(2x2,3x3) expand3x3, LDS-staged, MFMA "
                     "16x16x4 f32), conv_stream_kernel / conv_stream1x1_persist_kernel (LDS-free implicit GEMM, "
                     "MFMA 16x16x4 f32), pool_conv1x1_f32_kernel (pool3 / pool5 + the next squeeze) and "
                     "conv_gemm_kernel (LDS-staged, MFMA 32x32x2 f32) per the autotuned tile") + f", {conv['launches']} launches/step)"
            # HBM bytes per launch from the PMC passes of tools/pmc.sh (FETCH_SIZE x2 + WRITE_SIZE, separate
            # --pmc runs; counters cannot be read inside this timed run), per step and for the conv class
            tj, tsrc, tsame = None, None, None
            tfile = os.path.join(REPO, "profiles", f"pmc_traffic_{args.precision}.json")
            if os.path.exists(tfile):
                with open(tfile) as f:
                    tj = json.load(f)
                tsame = tj.get("lib_sha256") == lib_sha256()
                tsrc = (f"profiles/pmc_traffic_{args.precision}.json: PMC FETCH_SIZE/WRITE_SIZE passes "
                        f"({tj.get('source', 'tools/pmc.sh')}, commit {tj.get('commit', '?')}); "
                        f"{'the same libore.so build as this run' if tsame else 'an earlier libore.so build'}")
            # the dominant kernel: the launch with the largest share of the step (one kernel per launch)
            di = int(np.argmax(per_step_ms))
            dinfo, dms = infos[di], float(per_step_ms[di])
            tiles = model.tiles()
            dtile = ore.Model.TILE_NAMES[tiles[di]] if di < len(tiles) and tiles[di] >= 0 else None
            d_issued = dinfo.get("mfma_flops", dinfo["flops"])
            d_traffic = None
            if tj and tj.get("per_step") and len(tj["per_step"]) == len(infos) and tj["per_step"][di]["name"] == dinfo["name"]:
                d_traffic = round(tj["per_step"][di]["hbm_bytes"])
            d_bound_hbm = dinfo["bytes"] / (PEAK_HBM_GBS * 1e9) > d_issued / (peak * 1e12)
            result["roofline"] = {
                "bound": "hbm" if d_bound_hbm else "mfma",
                "kernel": f"step '{dinfo['name']}' ({dinfo['op']}), tile '{dtile}': the longest launch of the step "
                          f"({100.0 * dms / float(per_step_ms.sum()):.1f} % of the kernel time)",
                "achieved": round((dinfo["bytes"] / (dms * 1e-3) / 1e9) if d_bound_hbm else (d_issued / (dms * 1e-3) / 1e12), 2),
                "peak": PEAK_HBM_GBS if d_bound_hbm else peak, "unit": "GB/s" if d_bound_hbm else "TFLOP/s",
                "frac": round((dinfo["bytes"] / (PEAK_HBM_GBS * 1e9) if d_bound_hbm else d_issued / (peak * 1e12)) / (dms * 1e-3), 4),
                "traffic": d_traffic, "traffic_unit": "bytes/launch", "traffic_source": tsrc, "traffic_same_build": tsame,
                "algorithmic_flops_per_launch": d_issued, "algorithmic_bytes_per_launch": dinfo["bytes"],
                "launch_us": round(1000.0 * dms, 2),
                "achievable_peak": ach, "achievable_frac": round(d_issued / (ach * 1e12) / (dms * 1e-3), 4),
                "kernel_timing": f"HIP events between consecutive launches on the model stream, a separate ONE-STREAM pass of "
                                 f"the {args.steps} timed steps (events kept out of the value's timed loop; the value's loop runs "
                                 f"{args.streams} stream(s), so per-launch times describe the one-stream schedule)",
                # what the side stream hides: the one-stream pass's summed launch times minus the timed step
                "one_stream_kernel_ms": round(float(sum(per_step_ms)), 4),
                "side_stream_hides_ms": round(float(sum(per_step_ms)) - 1000.0 * elapsed / args.steps, 4),
                "conv_class": {
                    "kernel": kname, "launches": conv["launches"],
                    "achieved": round(issued, 2), "unit": "TFLOP/s", "peak": peak, "frac": round(issued / peak, 4),
                    "achieved_is": "MFMA work the conv launches issue / their measured time (direct convs: "
                                   "2*Cout*Ho*Wo*Cin*kh*kw; Winograd F(2x2,3x3) expand3x3: 16*C*M per 2x2 output tile)",
                    "effective_TFLOP/s": round(effective, 2), "effective_frac": round(effective / peak, 4),
                    "effective_is": "algorithmic direct-conv FLOPs (1.638 GFLOP/img) / the same time: credits Winograd "
                                    "layers with 2.25x the work they issue",
                    "achievable_frac": round(issued / ach, 4),
                    "traffic": round(tj["hbm_bytes_per_launch"]) if tj else None,
                    "algorithmic_bytes_per_launch": round(conv["bytes"] / max(conv["launches"], 1)),
                    "per_launch_avg_us": round(1000.0 * conv["ms"] / conv["launches"], 2)}}
            result["roofline_8d"] = r8d
            if args.layers:
                for info, ms in zip(infos, per_step_ms):
                    tf = info["flops"] / (ms * 1e-3) / 1e12 if info["flops"] else 0.0
                    gbs = info["bytes"] / (ms * 1e-3) / 1e9
                    print(f"{info['name']:24s} {info['op']:18s} {1000 * ms:9.1f} us {tf:7.1f} TF/s {gbs:8.1f} GB/s",
                          file=sys.stderr)
        if args.full:
            report_full(result, args, ctx, model_bytes, x, B, dev, world, gathered, sample_idx, x_sample,
                        "gloo" if gloo else "RCCL" if use_dist else None)
        print(json.dumps(result), flush=True)

    model.close()
    ctx.close()
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
