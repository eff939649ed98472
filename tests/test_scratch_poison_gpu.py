"""Poisoned scratch memory through every plan (tests/_poison.py): no byte of the memory the library
allocates for itself -- arena pads, tails, lead, the neighbour images' slots, stale values, weight-pack
padding -- may reach a result, whatever bits it holds.

Every model here is loaded on a context with ore_ctx_set_alloc_fill on; ore_model_fill_scratch poisons its
activation memory again after every set_fusion and before every run, and the output tensor starts as the
pattern.  Each case runs under NaN and under the +inf of the model's activation type.  The references never
saw the poisoned code: the float64 executor (catalogue, ints mode, bit for bit), the oracle at the bars of
test_model_gpu / test_wino_gpu / test_f16_gpu (SqueezeNet, MNIST), and as a second check the same model and
plan on a context without fill, bit for bit."""
import os
import warnings
import zlib

import numpy as np
import pytest

from ore import FUSE_ALL, FUSE_EAGER as EAGER, KEEP_VALUES as KEEP

import oracle
from _knobs import conv_tile, force_tiles
from _poison import NAN, count_words, download, filled, make_ctx, patterns, poisoned_run, same_bits
from _topologies import BATCH, BY_NAME, CATALOGUE, ints_reference

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
E = FUSE_ALL | EAGER
PLANS = [0, FUSE_ALL, E, E | KEEP]
COMBOS = [("f32", True), ("f32", False), ("f16", True)]
REAL = ("base-", "f9-", "f10-")  # the entries that also run once with real-valued weights
BARS = {"f32": 1e-5, "f16": 1.5e-2}  # SqueezeNet probabilities against the oracle (test_model_gpu / test_wino_gpu; test_f16_gpu)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@pytest.fixture(scope="module")
def fill_ctx():
    ctx, s = make_ctx()
    yield ctx, s
    s.synchronize()
    ctx.close()


def _load(ctx, pattern, mb, **kw):
    """a model loaded with alloc fill on (pattern None: off, the control)"""
    import ore
    ctx.set_alloc_fill(pattern is not None, pattern or 0)
    try:
        return ore.Model(ctx, mb, **kw)
    finally:
        ctx.set_alloc_fill(False)


def _plain_run(m, x):
    import torch
    y = m.run(x)
    torch.cuda.synchronize()
    return y.cpu().numpy()


class Problems(list):
    def check(self, ok, *what):
        if not ok:
            self.append(" ".join(str(w) for w in what))

    def clean(self, y, pattern, *what):
        """no pattern word and nothing non-finite in a result whose reference is finite"""
        self.check(count_words(y, pattern) == 0 and np.isfinite(y).all(), *what, "poison in the output:",
                   count_words(y, pattern), "pattern words,", int((~np.isfinite(y)).sum()), "non-finite of", y.size)

    def done(self, name):
        assert not self, f"{name}: {len(self)} problems:\n  " + "\n  ".join(self[:40])


# ------------------------------------------------------------------------------------ controls
def test_detector_controls(gpu_ctx, fill_ctx):
    """The detector itself: alloc fill and fill_scratch really put the pattern into every word of every
    activation buffer; a 1-image run on max_batch 3 leaves pattern words in the arena (images 1..2 are never
    written); fill_scratch inside a capture is refused."""
    import torch
    import ore
    ctx, s = fill_ctx
    P2 = 0x7C007C00
    for name, prec in (("f9-first-q16", "f16"), ("f9-first-q16", "f32")):
        entry = BY_NAME[name]
        mb, _ = entry.model("ints")
        x = _t(entry.inputs("ints"))
        m = _load(ctx, NAN, mb, max_batch=BATCH, precision=prec, winograd=False)
        try:
            ctx.set_alloc_fill(True, NAN)  # stage and rows are allocated by these two calls
            m.set_input_norm()
            m.set_topk(1)
            ctx.set_alloc_fill(False)
            bufs = m.scratch_buffers()
            names = [b[0] for b in bufs]
            assert names[0] == "arena" and {"stage", "rows"} <= set(names), names
            assert ("xcvt" in names) == (prec == "f16" and entry.dims[0] <= 4), names
            for bname, ptr, size in bufs:
                assert size > 0 and size % 4 == 0, (bname, size)
                w = download(ctx, ptr, size)
                assert (w == NAN).all(), f"{name} {prec}: {bname} after load holds {int((w != NAN).sum())} other words of {w.size}"
            m.fill_scratch(P2)
            for bname, ptr, size in bufs:
                w = download(ctx, ptr, size)
                assert (w == P2).all(), f"{name} {prec}: {bname} after fill_scratch holds {int((w != P2).sum())} other words"
            for pname, pat in patterns(prec):
                y = poisoned_run(m, s, x[:1].contiguous(), pat)
                assert same_bits(y, ints_reference(entry)[0][:1])
                _, ptr, size = m.scratch_buffers()[0]
                left = count_words(download(ctx, ptr, size), pat)
                print(f"{name} {prec} {pname}: arena words still poisoned after 1 image of {BATCH}: {left} of {size // 4}")
                assert left > 0
            # inside a capture of the caller's
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                g.capture_begin()
                try:
                    with pytest.raises(ore.OreError, match="capture") as refused:
                        m.fill_scratch(NAN)
                finally:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")  # torch remarks that the captured graph is empty: it is meant to be
                        g.capture_end()
            assert refused.value.status == 1  # ORE_ERR_INVALID
        finally:
            m.close()
    m = ore.Model(gpu_ctx, BY_NAME["base-12x12"].model("ints")[0], max_batch=1)
    try:
        assert [b[0] for b in m.scratch_buffers()] == ["arena"]
        assert ore._lib.load().ore_model_scratch_info(m.h, 1, None, None, None) == 1  # past the last one
    finally:
        m.close()


# ------------------------------------------------------------------------------------ the catalogue
def _cases():
    out = [(e.name, "ints") for e in CATALOGUE]
    return out + [(e.name, "real") for e in CATALOGUE if e.name.startswith(REAL)]


@pytest.mark.parametrize("name,mode", _cases())
def test_topology_poisoned(gpu_ctx, fill_ctx, name, mode):
    """Every plan of a catalogue entry, batch 3 and 1 and 2 images on max_batch 3 (the neighbour images' slots
    are then pure poison): ints mode equals the float64 reference bit for bit, KEEP_VALUES values included;
    both modes equal the same model and plan on a context without fill."""
    import ore
    ctx, s = fill_ctx
    entry = BY_NAME[name]
    mb, b = entry.model(mode)
    x = _t(entry.inputs(mode))
    ref, vals = ints_reference(entry) if mode == "ints" else (None, {})
    pb = Problems()
    for prec, wino in COMBOS:
        tag = f"{mode} {prec}{'' if wino or prec == 'f16' else ' direct'}"
        try:
            control = ore.Model(gpu_ctx, mb, max_batch=BATCH, precision=prec, winograd=wino)
        except ore.OreError as err:
            assert err.status != 3, err
            pb.check(prec == "f16" and entry.f16_refused is not None, tag, "load:", err)
            continue
        want = {}
        for plan in PLANS:
            control.set_fusion(plan)
            want[plan] = _plain_run(control, x)
        control.close()
        for pname, pat in patterns(prec):
            m = _load(ctx, pat, mb, max_batch=BATCH, precision=prec, winograd=wino)
            try:
                for plan in PLANS:
                    m.set_fusion(plan)
                    for n in (BATCH, 1, 2):
                        what = (tag, pname, f"plan {plan}", f"{n} images:")
                        y = poisoned_run(m, s, x[:n].contiguous(), pat)
                        pb.clean(y, pat, *what)
                        if ref is not None:
                            pb.check(same_bits(y, ref[:n]), *what, "differs from float64 in", int((y != ref[:n]).sum()), "of", y.size)
                        pb.check(same_bits(y, want[plan][:n]), *what, "differs from the unpoisoned run in",
                                 int((y != want[plan][:n]).sum()), "of", y.size)
                        if plan & KEEP and n == BATCH:
                            for vn, v in vals.items():
                                try:
                                    got = m.read_value(vn)
                                except ore.OreError as err:  # elided by the plan
                                    assert err.status != 3, err
                                    continue
                                pb.check(got.shape == v.shape and np.array_equal(got, v), *what, "value", vn, "differs from float64")
            finally:
                m.close()
    pb.done(name)


# ------------------------------------------------------------------------------------ SqueezeNet, MNIST
def _squeezenet_case(hw):
    """3 images and the oracle's rows for them, from the fixtures the bars were set on (test_squeezenet_mini_vs_oracle;
    test_squeezenet_synth_vs_oracle, whose two images are followed by the first again)"""
    from golden.make_golden import mini_inputs, squeezenet_inputs
    if hw == 64:
        return mini_inputs()[:3], np.load(os.path.join(GOLD, "squeezenet_mini_oracle.npz"))["output"][:3]
    pick = [0, 1, 0]
    return squeezenet_inputs()[pick], np.load(os.path.join(GOLD, "squeezenet_synth_oracle.npz"))["output"][pick]


@pytest.mark.parametrize("prec,wino", COMBOS)
@pytest.mark.parametrize("hw", [64, 224])
def test_squeezenet_poisoned(gpu_ctx, fill_ctx, hw, prec, wino):
    """SqueezeNet at batch 3, default plan and plan 0, against the oracle fixtures and the unpoisoned run."""
    import ore
    from ore import squeezenet
    ctx, s = fill_ctx
    mb = squeezenet.build(hw)
    xs, ref = _squeezenet_case(hw)
    x = _t(xs)
    pb = Problems()
    control = ore.Model(gpu_ctx, mb, max_batch=3, precision=prec, winograd=wino)
    want = {}
    for plan in (FUSE_ALL, 0):
        control.set_fusion(plan)
        want[plan] = _plain_run(control, x)
    control.close()
    for pname, pat in patterns(prec):
        m = _load(ctx, pat, mb, max_batch=3, precision=prec, winograd=wino)
        try:
            for plan in (FUSE_ALL, 0):
                m.set_fusion(plan)
                for n in (3, 2):
                    y = poisoned_run(m, s, x[:n].contiguous(), pat)
                    what = (pname, f"plan {plan}", f"{n} images:")
                    pb.clean(y, pat, *what)
                    err = float(np.abs(y - ref[:n]).max())
                    pb.check(err <= BARS[prec], *what, "off the oracle by", err)
                    pb.check(same_bits(y, want[plan][:n]), *what, "differs from the unpoisoned run in", int((y != want[plan][:n]).sum()))
        finally:
            m.close()
    pb.done(f"squeezenet {hw} {prec} wino={wino}")


@pytest.mark.parametrize("prec,wino", COMBOS)
def test_squeezenet64_forced_tiles_poisoned(gpu_ctx, fill_ctx, prec, wino):
    """Every tile id forced on every step of the 64 model that takes it (ore_model_set_step_tile), fully fused
    plan: against the oracle and the unpoisoned run of the same tiles."""
    import ore
    from ore import squeezenet
    ctx, s = fill_ctx
    mb = squeezenet.build(64)
    xs, ref = _squeezenet_case(64)
    x = _t(xs)
    pb = Problems()
    control = ore.Model(gpu_ctx, mb, max_batch=3, precision=prec, winograd=wino)
    models = {pname: _load(ctx, pat, mb, max_batch=3, precision=prec, winograd=wino) for pname, pat in patterns(prec)}
    ran = []
    try:
        for tile, tname in enumerate(ore.Model.TILE_NAMES):
            if tname is None:
                continue
            control.set_fusion(E)
            if not force_tiles(control, tile):
                continue
            try:
                want = _plain_run(control, x)
            except ore.OreError as err:  # the forced kernel declines this geometry
                assert err.status != 3, err
                continue
            ran.append(tname)
            for pname, pat in patterns(prec):
                m = models[pname]
                m.set_fusion(E)
                force_tiles(m, tile)
                y = poisoned_run(m, s, x, pat)
                pb.clean(y, pat, tname, pname)
                err = float(np.abs(y - ref).max())
                pb.check(err <= BARS[prec], tname, pname, "off the oracle by", err)
                pb.check(same_bits(y, want), tname, pname, "differs from the unpoisoned run in", int((y != want).sum()))
    finally:
        control.close()
        for m in models.values():
            m.close()
    print(f"{prec} wino={wino}: forced {ran}")
    assert ran, "no tile id could be forced on any step"
    pb.done(f"squeezenet 64 forced tiles {prec}")


@pytest.mark.parametrize("fusion", [FUSE_ALL | EAGER, FUSE_ALL, 7, 0])
def test_mnist_poisoned(fill_ctx, fusion):
    from ore import onnx_wire
    ctx, s = fill_ctx
    with open(os.path.join(GOLD, "mnist-8.onnx"), "rb") as f:
        mb = f.read()
    x = onnx_wire.load_tensor(os.path.join(GOLD, "mnist_data_0.pb")).to_numpy()
    g = onnx_wire.load_tensor(os.path.join(GOLD, "mnist_output_0.pb")).to_numpy()
    for pname, pat in patterns("f32"):
        m = _load(ctx, pat, mb, max_batch=4, winograd=False)
        try:
            m.set_fusion(fusion)
            y = poisoned_run(m, s, _t(x), pat)
        finally:
            m.close()
        assert count_words(y, pat) == 0 and np.isfinite(y).all(), pname
        assert np.abs(y - g).max() <= 1e-6 * np.abs(g).max(), pname
        assert y.argmax() == g.argmax() == 2


# ------------------------------------------------------------------------------------ input paths, capture
def _input_path_results(m, stream, pattern, x8, big8, lists):
    """every input path that owns scratch (stage, rows, xcvt), each after a fill_scratch when `pattern` is
    given, into outputs that start as the pattern (or zero): {path: [arrays]}"""
    import torch
    pat = 0 if pattern is None else pattern
    got = {}

    def go(key, entry, x, *outs):
        torch.cuda.synchronize()
        if pattern is not None:
            m.fill_scratch(pattern)
        entry(x, *outs) if x is not None else entry(*outs)
        stream.synchronize()
        got[key] = [o.cpu().numpy() for o in outs]

    E_ = m.output_elems
    m.set_input_norm(scale=[1 / 64.0] * 3, shift=[-2.0] * 3)
    go("run_u8", m.run_u8_into, x8[:2].contiguous(), filled((2, E_), pat))
    for aa in (False, True):
        m.set_input_resize(big8.shape[1:3], antialias=aa)
        go(f"run_u8 resize aa={aa}", m.run_u8_into, big8[:2].contiguous(), filled((2, E_), pat))
    m.set_input_resize(None)
    lst = lists[0]
    go("run_u8_list", lambda out: m.run_u8_list_into(lst, out), None, filled((2, E_), pat))
    m.set_topk(5)
    go("classify top5", m.classify_into, x8[:2].float().permute(0, 3, 1, 2).contiguous(),
       filled((2, 5), pat), filled((2, 5), pat, dtype=torch.int32))
    return got


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_input_paths_poisoned(gpu_ctx, fill_ctx, prec):
    """run_u8, run_u8 behind a resize (plain and antialiased), run_u8_list and classify with top 5 -- 2 images on
    max_batch 3 -- and classify with 2 views on 4 images of max_batch 4: each equals its unpoisoned run bit for
    bit and holds no poison."""
    import torch
    import ore
    ctx, s = fill_ctx
    entry = BY_NAME["f9-first-q16"]
    mb, _ = entry.model("real")
    C, H, W = entry.dims
    rng = np.random.default_rng(77)
    x8 = torch.from_numpy(rng.integers(0, 256, (4, H, W, C), dtype=np.uint8)).cuda()
    big8 = torch.from_numpy(rng.integers(0, 256, (2, 2 * H + 5, 3 * W + 1, C), dtype=np.uint8)).cuda()
    imgs = [torch.from_numpy(rng.integers(0, 256, (hs, ws, C), dtype=np.uint8)).cuda() for hs, ws in ((50, 41), (90, 120))]
    pb = Problems()

    def results(cx, st, pattern):
        out = {}
        m = _load(cx, pattern, mb, max_batch=3, precision=prec, winograd=False)
        lst = ore.ImageList(cx, 3, (H, W), channels=C).set(imgs)
        try:
            out.update(_input_path_results(m, st, pattern, x8, big8, [lst]))
        finally:
            st.synchronize()
            lst.close()
            m.close()
        m = _load(cx, pattern, mb, max_batch=4, precision=prec, winograd=False)
        try:
            cx.set_alloc_fill(pattern is not None, pattern or 0)
            m.set_topk(5)
            m.set_views(2)
            cx.set_alloc_fill(False)
            pat = pattern or 0
            sc, cl = filled((2, 5), pat), filled((2, 5), pat, dtype=torch.int32)
            torch.cuda.synchronize()
            if pattern is not None:
                m.fill_scratch(pattern)
            m.classify_into(x8.float().permute(0, 3, 1, 2).contiguous(), sc, cl)
            st.synchronize()
            out["classify 2 views"] = [sc.cpu().numpy(), cl.cpu().numpy()]
        finally:
            m.close()
        return out

    class _Default:  # the session context runs on torch's current stream
        @staticmethod
        def synchronize():
            torch.cuda.synchronize()

    want = results(gpu_ctx, _Default, None)
    for pname, pat in patterns(prec):
        got = results(ctx, s, pat)
        assert got.keys() == want.keys()
        for key in want:
            for a, b in zip(got[key], want[key]):
                pb.check(count_words(a, pat) == 0, prec, pname, key, "pattern words in the output:", count_words(a, pat))
                pb.check(same_bits(a, b), prec, pname, key, "differs from the unpoisoned run in", int((a != b).sum()), "of", a.size)
            if a.dtype == np.int32:
                pb.check(((a >= 0) & (a < 16)).all(), prec, pname, key, "classes out of range")
    pb.done(f"input paths {prec}")


@pytest.mark.parametrize("prec,wino", COMBOS)
def test_captured_graph_poisoned(fill_ctx, prec, wino):
    """capture, fill_scratch, replay twice: the replays read nothing the capture-time run left behind"""
    import torch
    ctx, s = fill_ctx
    entry = BY_NAME["base-pool-21x20"]
    mb, _ = entry.model("ints")
    x = _t(entry.inputs("ints"))
    ref = ints_reference(entry)[0]
    for pname, pat in patterns(prec):
        m = _load(ctx, pat, mb, max_batch=BATCH, precision=prec, winograd=wino)
        try:
            out = filled((BATCH, m.output_elems), pat)
            torch.cuda.synchronize()
            m.fill_scratch(pat)
            m.capture(x, out)
            for rep in range(2):
                out.copy_(filled((BATCH, m.output_elems), pat))
                torch.cuda.synchronize()
                m.fill_scratch(pat)
                m.replay()
                s.synchronize()
                y = out.cpu().numpy()
                assert count_words(y, pat) == 0 and np.isfinite(y).all(), (pname, rep)
                assert same_bits(y, ref), (pname, rep, int((y != ref).sum()))
        finally:
            m.close()


# ------------------------------------------------------------------------------------ per-op (pack_to_scratch)
PER_OP_CONVS = [
    # family, tile (None: heuristic), winograd, CONV_CASES-style row of test_ops_gpu.py
    ("LDS-staged", None, False, (2, 5, 16, 16, 40, 3, 3, "SAME_UPPER", None, [1, 1], True)),
    ("streaming 1x1", 12, False, (3, 96, 12, 12, 16, 1, 1, "NOTSET", [0, 0, 0, 0], [1, 1], True)),
    ("streaming 3x3", 12, False, (2, 16, 12, 12, 64, 3, 3, "NOTSET", [1, 1, 1, 1], [1, 1], True)),
    ("Winograd", None, True, (2, 16, 9, 9, 64, 3, 3, "NOTSET", [1, 1, 1, 1], [1, 1], True)),
    ("MNIST 5x5", None, False, (1, 8, 14, 14, 16, 5, 5, "SAME_UPPER", None, [1, 1], False)),
]


@pytest.mark.parametrize("pname,pat", patterns("f32"))
def test_per_op_under_alloc_fill(pname, pat):
    """Per-op convs (one per kernel family) and a MatMul on a fresh context with alloc fill on, so the weight
    scratch every one of them packs into starts as the pattern: the bound of test_ops_gpu.py against the oracle.
    The bytes in front of x, which the streaming 3x3 kernel reads masked, are the pattern too."""
    import torch
    import ore
    from test_ops_gpu import _conv_bound
    ctx, s = make_ctx()
    pb = Problems()
    try:
        ctx.set_alloc_fill(True, pat)
        # ascending scratch sizes: every call allocates (and fills) a larger scratch
        order = sorted(PER_OP_CONVS, key=lambda c: c[3][1] * c[3][5] * c[3][6] * max(c[3][4], 128))
        for family, tile, wino, case in order:
            N, C, H, W, M, kh, kw, auto_pad, pads, strides, with_bias = case
            rng = np.random.default_rng(zlib.crc32(repr(case).encode()) ^ 0x77)
            x = rng.standard_normal((N, C, H, W)).astype(np.float32)
            w = rng.standard_normal((M, C, kh, kw)).astype(np.float32)
            b = rng.standard_normal((M,)).astype(np.float32) if with_bias else None
            buf = filled((x.size + 1024 + 64,), pat)  # x 256 B into a 4 KiB page, as test_conv_stream_bit_identical
            xd = buf[1024 + 64:].view(x.shape)
            xd.copy_(_t(x))
            wd, bd = _t(w), (_t(b) if b is not None else None)
            torch.cuda.synchronize()
            ctx.set_conv_algo(ore.CONV_ALGO_WINOGRAD if wino else ore.CONV_ALGO_DIRECT)
            with conv_tile(ctx, -1 if tile is None else tile):
                y = ore.convolution(ctx, xd, wd, bd, auto_pad=auto_pad, pads=pads, strides=strides)
            s.synchronize()
            got = y.cpu().numpy()
            ref = oracle.conv2d(x, w, b, auto_pad=auto_pad, pads=pads, strides=strides)
            eff = "NOTSET" if pads is not None and any(p > 0 for p in pads) else auto_pad
            p, Ho, Wo = oracle.resolve_window(eff, pads, H, W, kh, kw, strides[0], strides[1])
            bound = _conv_bound(x, w, p, strides, Ho, Wo) + (np.abs(b)[None, :, None, None] if b is not None else 0)
            pb.check(np.isfinite(got).all(), family, "non-finite outputs:", int((~np.isfinite(got)).sum()))
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            pb.check(np.all(err <= 2e-6 * bound + 1e-30), family, "max err", float(np.nanmax(err)), "bound", float((2e-6 * bound).max()))
        ctx.set_conv_algo(ore.CONV_ALGO_DIRECT)
        m_, k_, n_ = 37, 256, 10
        rng = np.random.default_rng(m_ * 7 + n_)
        a = rng.standard_normal((m_, k_)).astype(np.float32)
        bb = rng.standard_normal((k_, n_)).astype(np.float32)
        ad, bd = _t(a), _t(bb)
        torch.cuda.synchronize()
        y = ore.mul(ctx, ad, bd)
        s.synchronize()
        got = y.cpu().numpy()
        bound = np.abs(a).astype(np.float64) @ np.abs(bb).astype(np.float64)
        pb.check(np.isfinite(got).all() and np.all(np.abs(got - oracle.matmul(a, bb)) <= 2e-6 * bound + 1e-30), "matmul off the oracle")
    finally:
        s.synchronize()
        ctx.close()
    pb.done(f"per-op {pname}")
