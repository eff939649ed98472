"""SqueezeNet-1.0 at input sizes other than 64 and 224, square and not, and partial batches on the 256-image
plan: the two user-facing parameters that drive kernel geometry (the planner's size rules, fire_pool_plan's
bands, the band walker's column pairs, conv + GAP's pixel limit; the LDS Winograd kernel's grouping rule,
bands per image, persistent tiles and the fire kernel's block remap by image count).

Sizes, seed, images and references come from tests/_sizes.py; tests/test_sizes.py holds the caps on the
references alone.  Each size loads with max_batch = n (its 2 or 3 images) and with max_batch = 256, the
production plan whose size rules decide without ORE_FUSE_EAGER.

  a. f32 direct kernels (winograd=False): default fusion at both max_batch values and the eager plan equal
     the unfused run bit for bit; under ORE_KEEP_VALUES every value a fused plan still materialises equals
     the unfused value bit for bit; the unfused run is held node by node to the oracle op applied to the
     GPU's own input (test_squeezenet_node_level_parity's bars).
  b. f32 Winograd: unfused, all eight expand3x3 layers run a Winograd tile and are within 2e-6 * sum|w x|
     of conv_f64 of the GPU's own squeeze output (test_wino_gpu.py's bar); the default plan at both
     max_batch values is within 1e-5 + |oracle - f64| of the oracle per image with float64's argmax
     (test_benched_plan_parity's form).  The margins are printed, vs_f64 is recorded, not asserted.
  c. f16: default plan at both max_batch values and the eager plan equal the unfused f16 run bit for bit;
     in the unfused run all 26 conv + Relu layers pass f16_layer_check on the GPU's own input; rows finite
     and summing to 1 within 1e-5; max |p16 - p_oracle| is printed.
  d. the max_batch = 256 plans of the sweep run the kernels the sweep is there for.
  Partial batches: 227 x 227, one 256-image batch, x[:n] for the counts of _sizes.partial_counts() -- row i of
  every run is row i of the n = 256 run, also on two streams and through capture / replay.

A device error from any load or run ends the session (nothing more runs on a GPU that has faulted); every
model is closed on the way out.  DESIGN.md section "Parity at other input sizes" records the printed figures."""
import contextlib
import json

import numpy as np
import pytest

import oracle

import _sizes
from _convref import F16_AMBIGUOUS_CAP, conv_f64, f16_layer_check
from _knobs import force_tiles

pytestmark = pytest.mark.gpu

SIZES = _sizes.SIZES
IDS = [_sizes.size_id(hw) for hw in SIZES]
ORE_ERR_HIP = 3
PLAN_BATCH = 256  # the production plan
# what autotune picks on large batches and no heuristic does: the LDS-staged Winograd kernel (its workgroup
# grouping follows the image count, ore_wino_geom.h) and a persistent 1x1 tile; forced here, so that the tests
# do not depend on a timing.  Every tile of a family gives the same bits (test_wino_tiles_bit_identical,
# test_forced_tiles_bit_identical)
WINO_LDS, PERSIST = "wino lds", "stream1x1 persist 32x128"


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()  # a copy: the shared images are read-only


def _np(t):
    import torch
    try:
        torch.cuda.synchronize()
        return t.cpu().numpy()
    except RuntimeError as err:  # a device error: nothing more runs on a GPU that has faulted
        pytest.exit(f"device error, stopping: {err}", returncode=3)


@contextlib.contextmanager
def _models(ctx, hw):
    """load(max_batch, **kw) -> a model of the size on ctx; all of them closed on the way out, and an
    ORE_ERR_HIP from any load or run inside the block ends the session."""
    import ore
    opened = []

    def load(max_batch, **kw):
        m = ore.Model(ctx, _sizes.model_bytes(hw), max_batch=max_batch, **kw)
        opened.append(m)
        return m
    try:
        yield load
    except ore.OreError as err:
        if err.status == ORE_ERR_HIP:
            pytest.exit(f"device error, stopping: {err}", returncode=3)
        raise
    finally:
        for m in opened:
            m.close()


def _tile_names(m):
    import ore
    return sorted({ore.Model.TILE_NAMES[t] for t in m.tiles() if t >= 0})


def _force(m, name):
    import ore
    return force_tiles(m, ore.Model.TILE_NAMES.index(name))


def _same(y, y0, what):
    assert y.shape == y0.shape and np.array_equal(y, y0), (
        f"{what}: differs from the unfused run in {int((y != y0).sum())} of {y.size}, max {float(np.abs(y - y0).max())}")


def _plan_runs(load, x, n, **kw):
    """[(what, rows, tile names)] of the unfused run, default fusion at max_batch = n and 256, and the eager plan."""
    import ore
    m = load(n, **kw)
    runs = []
    for what, fusion in (("unfused", 0), ("default", ore.FUSE_ALL), ("eager", ore.FUSE_ALL | ore.FUSE_EAGER)):
        m.set_fusion(fusion)
        runs.append((f"{what}, max_batch {n}", _np(m.run(x)), _tile_names(m)))
    big = load(PLAN_BATCH, **kw)
    runs.append((f"default, max_batch {PLAN_BATCH}", _np(big.run(x)), _tile_names(big)))
    return runs


# ---- a. f32 direct kernels ----

@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_f32_direct_plans_equal_unfused(gpu_ctx, hw):
    x = _t(_sizes.images(hw))
    with _models(gpu_ctx, hw) as load:
        runs = _plan_runs(load, x, x.shape[0], winograd=False)
    y0 = runs[0][1]
    assert y0.shape == (x.shape[0], 1000) and np.isfinite(y0).all()
    print(json.dumps({"size": _sizes.size_id(hw), "f32 direct": {what: tiles for what, _, tiles in runs}}))
    for what, y, tiles in runs[1:]:
        assert not any(t.startswith("wino") for t in tiles), tiles
        _same(y, y0, f"f32 direct {what}")


@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_f32_direct_fused_values_equal_unfused(gpu_ctx, hw):
    """The form of test_fused_padded_layout_values: every value the fused plans still hold, bit for bit."""
    import ore
    nodes, _ = _sizes.graph(hw)
    x = _t(_sizes.images(hw))
    n = x.shape[0]
    with _models(gpu_ctx, hw) as load:
        ref = load(n, winograd=False)
        ref.set_fusion(ore.KEEP_VALUES)
        outs = [ref.run(x)]  # kept alive: read_value of the graph's output reads the buffer the run wrote
        y0 = _np(outs[0])
        for what, fusion in (("default", ore.FUSE_ALL), ("eager", ore.FUSE_ALL | ore.FUSE_EAGER)):
            fused = load(n, winograd=False)
            fused.set_fusion(fusion | ore.KEEP_VALUES)
            outs.append(fused.run(x))
            _same(_np(outs[-1]), y0, f"f32 direct {what} + KEEP_VALUES")
            checked = []
            for node in nodes:
                for name in node.output[:1]:
                    try:
                        v = fused.read_value(name)
                    except ore.OreError as err:
                        assert err.status != ORE_ERR_HIP, err
                        continue  # fused away
                    np.testing.assert_array_equal(v, ref.read_value(name), err_msg=f"{what} plan, value {name}")
                    checked.append(name)
            print(f"sizes {_sizes.size_id(hw)} f32 direct {what}: {len(checked)} of {len(nodes)} values materialised, all equal")
            assert "softmaxout_1" in checked, checked  # the graph's output at the least


@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_f32_unfused_node_level(gpu_ctx, hw):
    """test_squeezenet_node_level_parity's bars on the unfused run: conv 1e-5 * (max|ref| + 1); Relu, MaxPool,
    Concat, Dropout, GlobalAveragePool exact; Softmax 2e-7.  From 224 up on image 0 only."""
    import ore
    nodes, inits = _sizes.graph(hw)
    x = _t(_sizes.images(hw))
    k = x.shape[0] if _sizes.image_count(hw) == 3 else 1
    with _models(gpu_ctx, hw) as load:
        m = load(x.shape[0], winograd=False)
        m.set_fusion(ore.KEEP_VALUES)
        out = m.run(x)  # kept alive: read_value of the graph's output reads this buffer
        _np(out)
        vals = {}

        def val(name):
            if name not in vals:
                vals[name] = m.read_value(name)[:k]
            return vals[name]
        worst = 0.0
        for node in nodes:
            a = node.attrs()
            xi, y = val(node.input[0]), val(node.output[0])
            if node.op_type == "Conv":
                ref = oracle.conv2d(xi, inits[node.input[1]], inits[node.input[2]], pads=a["pads"].ints, strides=a["strides"].ints)
                assert y.shape == ref.shape, node.name
                scale = float(np.abs(ref).max()) + 1.0
                err = float(np.abs(y - ref).max())
                worst = max(worst, err / scale)
                assert err <= 1e-5 * scale, (node.name, err, scale)
            elif node.op_type == "Relu":
                np.testing.assert_array_equal(y, oracle.relu(xi), err_msg=node.name)
            elif node.op_type == "MaxPool":
                ref = oracle.maxpool2d(xi, a["kernel_shape"].ints, a["strides"].ints, auto_pad=a["auto_pad"].s.decode(),
                                       pads=a["pads"].ints)
                np.testing.assert_array_equal(y, ref, err_msg=node.name)
            elif node.op_type == "Concat":
                np.testing.assert_array_equal(y, oracle.concat(xi, val(node.input[1]), 1), err_msg=node.name)
            elif node.op_type == "Dropout":
                np.testing.assert_array_equal(y, xi, err_msg=node.name)
            elif node.op_type == "GlobalAveragePool":
                np.testing.assert_array_equal(y, oracle.gap(xi), err_msg=node.name)
            elif node.op_type == "Softmax":
                assert np.abs(y.reshape(k, -1) - oracle.softmax(xi)).max() <= 2e-7
            else:
                raise AssertionError(node.op_type)
        print(f"sizes {_sizes.size_id(hw)} f32 unfused node level: worst conv error / (max|ref| + 1) = {worst:.3g} (bar 1e-5)")


# ---- b. f32 Winograd ----

@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_wino_unfused_layers_vs_f64(gpu_ctx, hw):
    """On the tile the heuristic picks and on the LDS-staged kernel, which also must agree bit for bit."""
    import ore
    x = _t(_sizes.images(hw))
    layers = [c for c in _sizes.conv_nodes(hw) if "expand3x3" in c[0].name]
    assert len(layers) == 8
    with _models(gpu_ctx, hw) as load:
        m = load(x.shape[0])
        m.set_fusion(ore.KEEP_VALUES)
        refs, first = {}, {}
        for forced in (None, WINO_LDS):
            if forced:
                assert _force(m, forced) == 8
            out = m.run(x)  # kept alive: read_value of the graph's output reads this buffer
            _np(out)
            e3 = [(st["name"], ore.Model.TILE_NAMES[t] if t >= 0 else None) for st, t in zip(m.steps(), m.tiles())
                  if st["op"] == "Conv" and "expand3x3" in st["name"]]
            assert len(e3) == 8 and all(t is not None and t.startswith("wino") for _, t in e3), e3
            assert not forced or all(t == forced for _, t in e3), e3
            worst = 0.0
            for node, w, b, pads, strides in layers:
                assert pads == [1, 1, 1, 1] and strides == [1, 1]
                if node.name not in refs:  # the squeeze in front is a direct conv: the same input under either tile
                    refs[node.name] = conv_f64(m.read_value(node.input[0]), w, b, pads, strides)
                ref, mag = refs[node.name]
                y = m.read_value(node.output[0])
                assert y.shape == ref.shape, node.name
                ratio = float((np.abs(y.astype(np.float64) - ref) / (mag + 1e-30)).max())
                worst = max(worst, ratio)
                assert ratio <= 2e-6, (node.name, forced, ratio)
                if forced:
                    np.testing.assert_array_equal(y, first[node.name], err_msg=f"{node.name}: {forced} vs the default tile")
                first.setdefault(node.name, y)
            print(f"sizes {_sizes.size_id(hw)} wino unfused: tiles {sorted({t for _, t in e3})}, "
                  f"worst |d| / sum|w x| = {worst:.3g} (bar 2e-6)")


@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_wino_default_plan_vs_references(gpu_ctx, hw):
    r64, _ = _sizes.references(hw)
    x = _t(_sizes.images(hw))
    n = x.shape[0]
    rows = []
    with _models(gpu_ctx, hw) as load:
        for mbatch, forced in ((n, False), (PLAN_BATCH, False), (PLAN_BATCH, True)):
            m = load(mbatch)
            if forced:  # the tuned production plan's kernels
                assert _force(m, WINO_LDS) >= 1 and _force(m, PERSIST) >= 1
            y = _np(m.run(x))
            rows.append((mbatch, y, _tile_names(m)))
            assert not forced or {WINO_LDS, PERSIST} <= set(rows[-1][2]), rows[-1][2]
    assert np.array_equal(rows[2][1], rows[1][1]), "forced tiles change the 256-image plan's rows"
    for mbatch, y, tiles in rows:
        marg = _sizes.margins(y, hw)
        print(json.dumps({"size": _sizes.size_id(hw), "precision": "f32", "max_batch": mbatch, "tiles": tiles, "margins": marg}))
        assert y.shape == r64.shape and np.isfinite(y).all()
        for r in marg:
            assert r["vs_oracle"] <= 1e-5 + r["oracle_vs_f64"], (mbatch, r)
        assert np.array_equal(y.argmax(1), r64.argmax(1)), mbatch


# ---- c. f16 ----

@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_f16_plans_equal_unfused(gpu_ctx, hw):
    _, ro = _sizes.references(hw)
    x = _t(_sizes.images(hw))
    with _models(gpu_ctx, hw) as load:
        runs = _plan_runs(load, x, x.shape[0], precision="f16")
    y0 = runs[0][1]
    assert y0.shape == ro.shape and np.isfinite(y0).all()
    assert np.abs(y0.sum(1) - 1.0).max() <= 1e-5
    print(json.dumps({"size": _sizes.size_id(hw), "precision": "f16", "max_dp_vs_oracle": float(np.abs(y0 - ro).max()),
                      "argmax_agrees": bool(np.array_equal(y0.argmax(1), ro.argmax(1))),
                      "tiles": {what: tiles for what, _, tiles in runs}}))
    for what, y, _ in runs[1:]:
        _same(y, y0, f"f16 {what}")


@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_f16_unfused_layers_vs_f64(gpu_ctx, hw):
    """All 26 conv + Relu layers of the unfused f16 run against their contract, each on the GPU's own input
    (the model input for conv1, f16 values behind it).  From 224 up on image 0 only."""
    import ore
    nodes, _ = _sizes.graph(hw)
    relu_of = {nd.input[0]: nd.output[0] for nd in nodes if nd.op_type == "Relu"}
    x = _t(_sizes.images(hw))
    k = x.shape[0] if _sizes.image_count(hw) == 3 else 1
    with _models(gpu_ctx, hw) as load:
        m = load(x.shape[0], precision="f16")
        m.set_fusion(ore.KEEP_VALUES)
        out = m.run(x)  # kept alive: read_value of the graph's output reads this buffer
        _np(out)
        convs = _sizes.conv_nodes(hw)
        assert len(convs) == 26
        worst = {"acc_ratio": (0.0, None), "ambiguous": (0.0, None)}
        for node, w, b, pads, strides in convs:
            xi = m.read_value(node.input[0])[:k]
            got = m.read_value(relu_of[node.output[0]])[:k]
            if node.name != "conv1":  # the GPU's own f16 values: they survive the reference's cast unchanged
                assert np.array_equal(xi.astype(np.float16).astype(np.float32), xi), node.name
            res = f16_layer_check(got, xi, w, b, pads, strides, True)
            for key in worst:
                if res[key] >= worst[key][0]:
                    worst[key] = (res[key], node.name)
            assert res["ambiguous"] <= F16_AMBIGUOUS_CAP, (node.name, res["ambiguous"])
            bad = np.argwhere(~res["ok"])
            assert bad.size == 0, (f"{node.name}: {len(bad)} of {got.size} outputs outside the f16 contract; first "
                                   "(n, m, oh, ow): got / nearest f16 = "
                                   + ", ".join(f"{tuple(j)}: {got[tuple(j)]!r} / {res['ref'][tuple(j)]!r}" for j in bad[:8]))
        print(json.dumps({"size": _sizes.size_id(hw), "precision": "f16", "worst_acc_ratio": worst["acc_ratio"],
                          "worst_ambiguous": worst["ambiguous"]}))


# ---- d. the sweep runs the kernels it claims ----

def test_sweep_runs_the_kernels_it_claims(gpu_ctx):
    """The max_batch = 256 plans (f32 with Winograd, f32 direct, f16) at every size, tile names read after a
    run of the size's images."""
    tiles = {}
    for hw in SIZES:
        x = _t(_sizes.images(hw))
        with _models(gpu_ctx, hw) as load:
            for key, kw in (("f32", {}), ("f32 direct", {"winograd": False}), ("f16", {"precision": "f16"})):
                m = load(PLAN_BATCH, **kw)
                _np(m.run(x))
                tiles[(hw, key)] = _tile_names(m)
    for (hw, key), names in tiles.items():
        print(json.dumps({"size": _sizes.size_id(hw), "plan": key, "tiles": names}))

    def seen(precs, hws=None):
        return {t for (hw, key), names in tiles.items() if key in precs and (hws is None or hw in hws) for t in names}
    others = [hw for hw in SIZES if hw != 224]
    f32 = seen(("f32", "f32 direct"), others)
    for name in ("fire pool f32", "fire", "epool band f32", "epool window f32", "conv1x1 gap f32"):
        assert name in f32, (name, sorted(f32))
    assert any(t.startswith("wino") for t in seen(("f32",), others))
    f16 = seen(("f16",), others)
    # "first conv pool f16": the f16 first conv's patch kernel, "epool band f16": its band kernel
    for name in ("fire f16", "conv1x1 gap f16", "first conv pool f16", "epool band f16"):
        assert name in f16, (name, sorted(f16))
    f32_keys = ("f32", "f32 direct")
    assert "conv1x1 gap f32" not in seen(f32_keys, [288])  # conv10 on 17 x 17 = 289 pixels, past conv + GAP's 256
    assert "fire pool f32" not in seen(f32_keys, [131])    # pool1 plane 31 x 31 = 961 < FIRE_POOL_MIN_HW
    # the band walkers stage input rows 16 bytes at a time into a 224-float window: input widths that are a
    # multiple of 4 and <= 224 only, and the f32 one wants >= 52 column pairs per conv row (width >= 211).  So
    # 226, whose planes are 224's, runs the window / patch kernels (conv_band_pool_f32_geometry: W % 4), and of
    # this sweep only 220 runs the band kernels
    no_band = [hw for hw in SIZES if _sizes.hw_pair(hw)[1] % 4 or _sizes.hw_pair(hw)[1] > 224]
    assert 226 in no_band and set(SIZES) - set(no_band) == {220}
    assert not {"epool band f32", "epool band f16"} & seen(f32_keys + ("f16",), no_band)
    small = [hw for hw in SIZES if max(_sizes.hw_pair(hw)) < 211]
    assert small and "epool band f32" not in seen(f32_keys, small)
    assert "epool band f32" in seen(("f32",), [220]) and "epool band f32" in seen(("f32 direct",), [220])
    assert "epool band f16" in seen(("f16",), [220])


# ---- partial batches on the 256-image plan ----

@pytest.fixture(scope="module")
def stream_ctx():
    import torch
    import ore
    s = torch.cuda.Stream()
    ctx = ore.Context(0, use_torch_stream=False)
    ctx.set_stream(s.cuda_stream)
    yield ctx
    torch.cuda.synchronize()
    ctx.close()


@pytest.fixture(scope="module")
def batch256():
    """One 256-image batch at 227 x 227, uploaded once; images 0 and 1 are the size sweep's."""
    import torch
    from ore import squeezenet
    hw = _sizes.PARTIAL_HW
    x = squeezenet.synthetic_input(_sizes.PARTIAL_MAX, hw, seed=_sizes.SEED + 1)
    two = _sizes.images(hw)
    x[:len(two)] = two
    xt = _t(x)
    yield xt
    del xt
    torch.cuda.empty_cache()


def _run_n(m, x, n):
    import torch
    out = torch.empty((n, m.output_elems), device="cuda")
    torch.cuda.synchronize()
    m.run_into(x[:n], out)
    return _np(out)


@pytest.mark.parametrize("kind", ["f32", "f32 tuned", "f32 direct", "f16"])
def test_partial_batches_on_the_256_plan(stream_ctx, batch256, kind):
    import torch
    import ore
    hw = _sizes.PARTIAL_HW
    kw = {"f32": {}, "f32 tuned": {}, "f32 direct": {"winograd": False}, "f16": {"precision": "f16"}}[kind]
    counts = _sizes.partial_counts()
    r64, _ = _sizes.references(hw)
    with _models(stream_ctx, hw) as load:
        m = load(_sizes.PARTIAL_MAX, **kw)
        if kind == "f32 tuned":
            assert _force(m, WINO_LDS) >= 1 and _force(m, PERSIST) >= 1
        full = _run_n(m, batch256, _sizes.PARTIAL_MAX)
        tiles = _tile_names(m)
        assert kind != "f32 tuned" or {WINO_LDS, PERSIST} <= set(tiles), tiles
        assert full.shape == (_sizes.PARTIAL_MAX, 1000) and np.isfinite(full).all()
        assert np.abs(full.sum(1) - 1.0).max() <= 1e-5
        wino = [st["name"] for st, t in zip(m.steps(), m.tiles()) if t >= 0 and ore.Model.TILE_NAMES[t].startswith("wino")]
        if kind in ("f32", "f32 tuned"):
            # the plan's Winograd layers are among the layers the counts were made for
            layers = dict(zip((f"fire{i}/expand3x3" for i in range(2, 10)), _sizes.expand3x3_layers(hw)))
            assert wino, m.steps()
            lds = [st["name"] for st, t in zip(m.steps(), m.tiles()) if t >= 0 and ore.Model.TILE_NAMES[t] == WINO_LDS]
            assert lds == (wino if kind == "f32 tuned" else []), (lds, wino)
            for name in wino:
                hit = [layer for prefix, layer in layers.items() if prefix in name]
                assert len(hit) == 1, name
                for c in _sizes.mbs_changes(hit[0]):
                    assert {c - 1, c} <= set(counts) | {_sizes.PARTIAL_MAX}, (name, c)
        else:
            assert not wino, wino
        bad = []
        for streams in (1, 2):
            m.set_streams(streams)
            for n in counts + ((_sizes.PARTIAL_MAX,) if streams == 2 else ()):
                y = _run_n(m, batch256, n)
                if not np.array_equal(y, full[:n]):
                    rows = np.flatnonzero((y != full[:n]).any(axis=1))
                    bad.append((streams, n, len(rows), rows[:8].tolist()))
        assert not bad, f"{kind}: (streams, n, rows that differ from the n = 256 run, first rows) {bad}"
        m.set_streams(1)
        n = 65
        out = torch.full((n, m.output_elems), float("nan"), device="cuda")
        torch.cuda.synchronize()
        m.capture(batch256[:n], out)
        m.replay()
        assert np.array_equal(_np(out), full[:n]), "capture / replay at n = 65"
        # the anchors: images 0 and 1 are the size sweep's, run there from their own buffer on a model of their own
        two = _t(_sizes.images(hw))
        own = load(_sizes.PARTIAL_MAX, **kw)  # on the heuristic's tiles, "f32 tuned" too
        y2 = _run_n(own, two, two.shape[0])
        assert np.array_equal(y2, full[:len(y2)]), "rows 0, 1 differ from the size sweep's run of the same images"
        if kind != "f16":
            for r in _sizes.margins(y2, hw):
                assert r["vs_oracle"] <= 1e-5 + r["oracle_vs_f64"], r
            assert np.array_equal(y2.argmax(1), r64.argmax(1))
    print(json.dumps({"partial batches": kind, "counts": list(counts), "wino_layers": wino, "tiles": tiles}))
