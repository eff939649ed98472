#!/usr/bin/env python3
"""Chunk-phase cycles of the LDS Winograd kernel from s_memtime stamps (experiment build only:
PATCHES=tools/patches/wino_stamps_chunk.patch tools/build_exp.sh stamps "-DORE_STAMPS" ore_conv_wino, run with
ORE_LIB=lib/exp/libore_stamps.so).  Wave 0 of each workgroup sums, over its staging chunks after a block's
first, the cycles from the chunk's top to its first MFMA, in its closing vmcnt wait, and in the whole chunk.
Prints the median over workgroups of the per-chunk means.
usage: python tools/stamps_wino_chunks.py [--batch 256] [--layers f6.e3 f8.e3]"""
import argparse
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-rusty-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--layers", nargs="+", default=["f6.e3", "f8.e3"])
    ap.add_argument("--tag", default=os.path.basename(os.environ.get("ORE_LIB", "libore.so")))
    a = ap.parse_args()
    import torch
    import ore
    from bench_ops import CONVS, conv_graph
    lib = ore.load()
    ctx = ore.Context(0)
    tile = ore.Model.TILE_NAMES.index("wino lds")
    for name in a.layers:
        _, cin, h, cout, k, s, pad = [c for c in CONVS if c[0] == name][0]
        ctx.set_conv_tile(tile)
        m = ore.Model(ctx, conv_graph(cin, h, cout, k, s, pad), max_batch=a.batch)
        ctx.set_conv_tile(-1)
        x = torch.randn(a.batch, cin, h, h, device="cuda")
        out = torch.empty((a.batch, m.output_elems), device="cuda")
        for _ in range(3):
            m.run_into(x, out)
        torch.cuda.synchronize()
        assert lib.ore_debug_stamps_wino_chunk_clear() == 0
        m.run_into(x, out)
        torch.cuda.synchronize()
        st = np.zeros(1 << 16, dtype=np.uint32)
        assert lib.ore_debug_stamps_wino_chunk(st.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(st.nbytes)) == 0
        m.close()
        st = st.reshape(-1, 4).astype(np.float64)
        st = st[st[:, 3] > 0]
        per = st[:, :3] / st[:, 3:4]
        med = np.median(per, axis=0)
        print(f"[{a.tag}] {name}: {len(st)} workgroups, cycles per chunk (median of workgroup means): "
              f"top -> first MFMA {med[0]:.0f}, closing vmcnt wait {med[1]:.0f}, chunk {med[2]:.0f}")
    ctx.close()


if __name__ == "__main__":
    main()
