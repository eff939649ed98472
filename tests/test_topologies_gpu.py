"""Every plan of every graph of the topology catalogue (tests/_topologies.py) against a float64
reference: the planner's contract "the result of the graph does not depend on which passes ran", on the
near-misses of each matcher's guards and not only on SqueezeNet's own shapes.

Per entry one model per (precision, Winograd) -- f32 with Winograd, f32 without, f16 -- re-planned with
set_fusion through PLANS.  ints mode (every intermediate a small integer, tests/test_topologies.py):
every plan, precision and Winograd setting returns the float64 reference bit for bit, and under
ORE_KEEP_VALUES so does every value read_value still returns.  real mode: f32 without Winograd and f16
are bit-identical to their unfused plan 0, f32 plan 0 and every Winograd plan are within rtol 1e-5 /
atol 1e-5 of the oracle (the bar of test_pool_expand_fused_bit_identical).  No load or run may fail with
an "internal:" error; the passes an entry declares must show in the FUSE_ALL | FUSE_EAGER plan; results
do not depend on what ran before, on the batch, or on the second stream."""
import numpy as np
import pytest

from ore import FUSE_ALL, FUSE_EAGER as EAGER, KEEP_VALUES as KEEP

import oracle
from _topologies import BATCH, BY_NAME, CATALOGUE, ints_reference

pytestmark = pytest.mark.gpu

E = FUSE_ALL | EAGER
PLANS = [0, 7, FUSE_ALL, E] + [E & ~b for b in (32, 64, 128, 256, 512, 1024, 4096, 8192)] + [E | KEEP]
COMBOS = [("f32", True), ("f32", False), ("f16", True)]
ORE_ERR_HIP = 3


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    import torch
    try:
        torch.cuda.synchronize()
        return t.cpu().numpy()
    except RuntimeError as err:  # a device error: nothing more runs on a GPU that has faulted
        pytest.exit(f"device error, stopping: {err}", returncode=3)


@pytest.fixture(scope="module")
def stream_ctx():
    import torch
    import ore
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    yield ctx, s
    s.synchronize()
    ctx.close()


def _message(err):
    """the library's message of an OreError; a device error ends the session (nothing more runs on a GPU
    that has faulted)"""
    if err.status == ORE_ERR_HIP:
        pytest.exit(f"device error, stopping: {err}", returncode=3)
    return str(err).split(": ", 1)[1]


def _fired(m, b):
    """the matching passes visible in m's current plan (after a run): tile names, the fused steps' names
    (producer+consumer, each a node's first output) and the ops left, read against the graph b built"""
    import ore
    tiles = [ore.Model.TILE_NAMES[t] if t >= 0 else None for t in m.tiles()]
    steps = m.steps()
    kind = lambda v: b.kind.get(v)
    readers = lambda v: [o for o, ins in b.ins.items() if v in ins or v + "r" in ins]
    got = set()
    for tile, st in zip(tiles, steps):
        parts = st["name"].split("+")
        epool = tile is not None and (tile.startswith("epool") or tile == "first conv pool f16")
        if tile == "fire pool f32":
            got.add("fire_pool_f32")
        elif tile == "fire":
            got.add("fire_f32")
        elif tile == "fire f16":
            got.add("fire_f16_concat" if st["name"].endswith("/expand+concat") else "fire_f16")
        elif tile in ("conv1x1 gap f32", "conv1x1 gap f16"):
            got.add("conv_gap")
        elif len(parts) == 2 and kind(parts[0]) == "MaxPool" and kind(parts[1]) == "Conv":
            got.add("pool_squeeze")
        elif len(parts) == 3 and [kind(p) for p in parts] == ["Conv", "MaxPool", "Conv"]:
            got.update(("pool_squeeze", "pool_expand"))
        elif epool:
            if len(parts) == 2 and kind(parts[0]) == "Conv" and kind(parts[1]) == "Conv":
                got.add("first_squeeze")
            nxt = readers(parts[0])
            if any(kind(r) == "MaxPool" for r in nxt):
                got.add("conv_pool")
            if any(kind(r) == "Concat" and any(kind(q) == "MaxPool" for q in readers(r)) for r in nxt):
                got.add("concat_pool")
    wide = [v for v, k in b.kind.items() if k == "Concat" and b.shape[v][1:] != (1, 1)]
    if wide and not got & {"fire_f32", "fire_pool_f32", "fire_f16", "fire_f16_concat", "concat_pool"} and \
            sum(st["op"] == "Concat" for st in steps) == len(b.extras):
        got.add("concat_in_place")
    return got, [f"{st['name']}[{t}]" for t, st in zip(tiles, steps)]


def _run_streams(ctx, s, m, x, streams):
    import torch
    m.set_streams(streams)
    out = torch.empty((x.shape[0], m.output_elems), device="cuda")
    torch.cuda.synchronize()
    m.run_into(x, out)
    s.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", [e.name for e in CATALOGUE])
def test_topology(gpu_ctx, stream_ctx, name):
    import ore
    entry = BY_NAME[name]
    problems = []

    def check(ok, *what):
        if not ok:
            problems.append(" ".join(str(w) for w in what))

    for mode in ("ints", "real"):
        mb, b = entry.model(mode)
        xs = [entry.inputs(mode, k) for k in (0, 1)]
        x, x2 = (_t(v) for v in xs)
        if mode == "ints":
            ref, vals = ints_reference(entry)
        else:
            ref = oracle.Model(mb).run(xs[0], int(np.prod(b.shape[b.out])))
        for prec, wino in COMBOS:
            tag = f"{mode} {prec}{'' if wino or prec == 'f16' else ' direct'}"
            try:
                m = ore.Model(gpu_ctx, mb, max_batch=BATCH, precision=prec, winograd=wino)
            except ore.OreError as err:
                msg = _message(err)
                if prec == "f16" and entry.f16_refused is not None:
                    check(msg == entry.f16_refused and err.status == 2, tag, "load: expected", entry.f16_refused, "got", err)
                else:
                    check(False, tag, "load:", err)
                continue
            try:
                check(not (prec == "f16" and entry.f16_refused), tag, "loads, but the catalogue lists it as refused")
                outs = {}
                for plan in PLANS:
                    try:
                        m.set_fusion(plan)
                        yt = m.run(x)  # kept until the next plan: read_value reads the output where the run put it
                        y = _np(yt)
                    except ore.OreError as err:
                        check(False, tag, f"plan {plan}:", _message(err))
                        continue
                    outs[plan] = y
                    if plan == E:
                        got, names = _fired(m, b)
                        if mode == "ints":
                            print(f"{name} {tag}: {sorted(got)} <- {' '.join(names)}")
                        check(set(entry.must[prec]) <= got, tag, "passes", sorted(set(entry.must[prec]) - got), "did not fire:", names)
                    if mode == "ints":
                        check(np.array_equal(y, ref), tag, f"plan {plan}: output differs from float64,",
                              int((y != ref).sum()), "of", y.size, "max", float(np.abs(y - ref).max()))
                        if plan & KEEP:
                            for vn, v in vals.items():
                                try:
                                    got_v = m.read_value(vn)
                                except ore.OreError as err:  # elided by the plan
                                    check(not _message(err).startswith("internal:"), tag, "read_value", vn, err)
                                    continue
                                check(got_v.shape == v.shape and np.array_equal(got_v, v), tag, f"plan {plan}: value {vn} differs")
                    elif prec == "f32" and wino:
                        check(np.allclose(y, ref, rtol=1e-5, atol=1e-5), tag, f"plan {plan}: off the oracle by",
                              float(np.abs(y - ref).max()))
                    elif plan in outs and 0 in outs:
                        check(np.array_equal(y, outs[0]), tag, f"plan {plan}: differs from plan 0 in",
                              int((y != outs[0]).sum()), "of", y.size)
                if mode == "real" and prec == "f32" and not wino and 0 in outs:
                    check(np.allclose(outs[0], ref, rtol=1e-5, atol=1e-5), tag, "plan 0: off the oracle by",
                          float(np.abs(outs[0] - ref).max()))
                # state and batch, on the fully fused plan: nothing of an earlier run or of a neighbour image leaks
                try:
                    m.set_fusion(E)
                    y1, y2, y1b = _np(m.run(x)), _np(m.run(x2)), _np(m.run(x))
                    check(np.array_equal(y1, y1b) and not np.array_equal(y1, y2), tag, "run(x1), run(x2), run(x1): the first result changed")
                    check(np.array_equal(_np(m.run(x[:2].contiguous())), y1[:2]), tag, "2 images differ from rows 0..1 of the full run")
                    check(np.array_equal(_np(m.run(x[2:].contiguous())), y1[2:]), tag, "image 2 alone differs from row 2 of the full run")
                except ore.OreError as err:
                    check(False, tag, "state / batch runs:", _message(err))
            finally:
                m.close()
            if mode != "ints":
                continue
            # two streams, on a context with a stream of its own
            ctx, s = stream_ctx
            try:
                m = ore.Model(ctx, mb, max_batch=BATCH, precision=prec, winograd=wino)
            except ore.OreError as err:
                _message(err)
                continue  # reported above
            try:
                for plan in (FUSE_ALL, 7):
                    m.set_fusion(plan)
                    one, two = (_run_streams(ctx, s, m, x, n) for n in (1, 2))
                    check(np.array_equal(one, two), tag, f"plan {plan}: two streams differ from one in", int((one != two).sum()))
                    check(np.array_equal(one, ref), tag, f"plan {plan}: own-stream context differs from float64")
            except ore.OreError as err:
                check(False, tag, "two streams:", _message(err))
            finally:
                m.close()
    assert not problems, f"{name}: {len(problems)} problems:\n  " + "\n  ".join(problems[:40])

