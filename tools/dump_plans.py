"""Dumps the planner's output for a fixed set of models and fusion flags: per configuration the launched
steps (`Model.steps()`: op, name, flops, bytes, mfma_flops), the tile ids (`Model.tiles()`) and
`ore_model_run_batch`.  tests/test_plan_golden_gpu.py compares these records, exactly, with
tests/golden/plans.json, which was written once from the library of the commit before the planner moved
to csrc/ore_plan.cpp and is never regenerated from the code under test.

Each model is loaded once and run once on one image (the step figures are per-image values times the last
run's batch); every record is then taken right after a `set_fusion`, so it shows the plan alone and not
what a launch left behind.  Many configurations share a plan: the file stores each distinct record once
and maps the configuration keys to it by index.

Usage (on the GPU): python tools/dump_plans.py OUT.json
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "onnx-rusty-inference-engine_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def fusion_sets():
    """(label, flags) in the order they are applied."""
    from ore import _lib as L
    eager = L.FUSE_ALL | L.FUSE_EAGER
    sets = [("all", L.FUSE_ALL), ("eager", eager)]
    for name in ("CONV_POOL", "FIRE", "CONCAT_POOL", "FIRE_POOL", "FIRST_SQUEEZE", "POOL_SQUEEZE", "CONV_GAP",
                 "POOL_EXPAND"):
        sets.append(("eager-" + name, eager & ~getattr(L, "FUSE_" + name)))
    sets += [("all+keep", L.FUSE_ALL | L.KEEP_VALUES), ("7", 7), ("0", 0)]
    return sets


def model_loads():
    """(label, onnx bytes, max_batch, precision, winograd): one load each."""
    from ore import squeezenet
    loads = []
    for label, size, batch in (("sq224/b256", 224, 256), ("sq224/b3", 224, 3), ("sq64/b3", 64, 3)):
        mb = squeezenet.build(size)
        loads += [(label + "/f32", mb, batch, "f32", True), (label + "/f32-nowino", mb, batch, "f32", False),
                  (label + "/f16", mb, batch, "f16", True)]
    with open(os.path.join(REPO, "tests", "golden", "mnist-8.onnx"), "rb") as f:
        loads.append(("mnist/b1/f32", f.read(), 1, "f32", True))
    return loads


def collect(ctx):
    """{configuration key: record} from the loaded library."""
    import torch
    import ore
    from ore import _lib as L
    out = {}
    for label, mb, batch, precision, wino in model_loads():
        m = ore.Model(ctx, mb, max_batch=batch, precision=precision, winograd=wino)
        m.run(torch.zeros((1,) + tuple(m.input_dims), device="cuda"))  # last_n = 1: per-image figures
        torch.cuda.synchronize()
        for fl, flags in fusion_sets():
            m.set_fusion(flags)
            out[f"{label}/{fl}"] = {"steps": m.steps(), "tiles": m.tiles(),
                                    "run_batch": int(L.load().ore_model_run_batch(m.h))}
        m.close()
    return out


def pack(configs):
    """Each distinct record once, configurations mapped to it by index."""
    records, index = [], {}
    for key, rec in configs.items():
        for i, r in enumerate(records):
            if r == rec:
                index[key] = i
                break
        else:
            index[key] = len(records)
            records.append(rec)
    return {"records": records, "configs": index}


def unpack(packed):
    return {key: packed["records"][i] for key, i in packed["configs"].items()}


def main(path):
    import torch  # before the library: one HIP runtime per process, the one torch brings
    if not torch.cuda.is_available():
        sys.exit("no GPU is visible")
    import ore
    ctx = ore.Context(0)
    packed = pack(collect(ctx))
    ctx.close()
    with open(path, "w") as f:
        json.dump(packed, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(packed['configs'])} configurations, {len(packed['records'])} distinct records -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
