"""CPU: localisation from class activation maps (ore_upsample_maps_f32, ore_cam_boxes_f32, ore_cam_box_host,
ore_model_set_cam_boxes) -- what the GPU tests of tests/test_cam_boxes_gpu.py lean on, and what needs no device.

The references on their own: the pure-Python labelling of _cam_boxes against scipy.ndimage.label on every case; the
library's plain C++ restatement ore_cam_box_host against the numpy reference on every case; the numpy upsample against
F.interpolate in float64; the case table reaches the edges it is there for.  Then box_to_source against the pixels
ore.resize_taps reads, and the argument checks of the three new per-op entries with a NULL context, in the header's
order.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import _cam_boxes as cb
import ore
from ore import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ore.h")
INVALID = 1  # ORE_ERR_INVALID
NAMES = ("ore_upsample_maps_f32", "ore_cam_boxes_f32", "ore_cam_box_host", "ore_model_set_cam_boxes")
P = ctypes.c_void_p(0x1000)  # never dereferenced
# nine roundings of intermediates of at most 2 max|m| (three lerps of three operations), half an ulp each, and three
# tap weights rounded to float32: (9 * 2 + 3) * 2^-24 max|m| < 2^-19 max|m|
UPSAMPLE_TOL = 2.0 ** -19


@pytest.mark.parametrize("case", cb.cases(), ids=cb.case_id)
def test_labelling_equals_scipy(case):
    ndimage = pytest.importorskip("scipy.ndimage")
    name, maps, hw, frac = case
    u, boxes, areas = cb.reference(name)
    for p in range(len(u)):
        mask = cb.mask_of(u[p], frac)
        lab, n = ndimage.label(mask, np.ones((3, 3)))
        comps = cb.components(mask)
        assert n == len(comps)
        if n == 0:
            assert tuple(boxes[p]) == (0, 0, 0, 0) and areas[p] == 0
            continue
        counts = np.bincount(lab.ravel())[1:]  # scipy numbers the components in raster order of their first pixels
        assert [c[0] for c in comps] == counts.tolist()
        best = int(np.argmax(counts))  # the first of equals
        rows, cols = np.nonzero(lab == best + 1)
        assert areas[p] == counts[best]
        assert tuple(boxes[p]) == (rows.min(), cols.min(), rows.max() + 1, cols.max() + 1)


@pytest.mark.parametrize("case", cb.cases(), ids=cb.case_id)
def test_host_entry_equals_the_numpy_reference(case):
    name, maps, hw, frac = case
    u, boxes, areas = cb.reference(name)
    for p in range(len(maps)):
        box, area = ore.cam_box_reference(maps[p], hw, frac)
        assert (box, area) == (tuple(int(v) for v in boxes[p]), int(areas[p])), (name, p)


def _interp64(m, hw):
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.asarray(m, np.float64))[None, None]
    return F.interpolate(t, size=hw, mode="bilinear", align_corners=False)[0, 0].numpy()


def test_numpy_upsample_against_float64_interpolate():
    worst = 0.0
    shapes = [(c[1][p], c[2]) for c in cb.cases() for p in range(len(c[1])) if np.isfinite(c[1]).all()]
    rng = np.random.default_rng(12)
    for _ in range(60):
        hm, wm = (int(v) for v in rng.integers(1, 20, 2))
        hw = (int(rng.integers(hm, 6 * hm + 1)), int(rng.integers(wm, 6 * wm + 1)))
        shapes.append((rng.standard_normal((hm, wm)).astype(np.float32) * np.float32(rng.uniform(0.1, 50.0)), hw))
    for m, hw in shapes:
        err = float(np.abs(cb.upsample(m, hw).astype(np.float64) - _interp64(m, hw)).max()) / float(np.abs(m).max())
        worst = max(worst, err)
        assert err <= UPSAMPLE_TOL, (m.shape, hw, err)
    print(f"numpy upsample against float64 F.interpolate over {len(shapes)} planes: worst error / max|m| = {worst:.3g}")


def test_identity_scale_is_the_plane():
    for name, maps, hw, frac in cb.cases():
        if maps.shape[1:] == hw:
            assert np.array_equal(cb.reference(name)[0].view(np.uint32), maps.view(np.uint32)), name


def test_numpy_taps_are_the_library_s():
    for S, D in ((1, 1), (1, 7), (4, 33), (5, 70), (17, 64), (17, 65), (9, 512), (13, 224), (17, 288)):
        i0, i1, t = ore.resize_taps(S, D, 0, D)
        a0, a1, at = cb.taps(S, D)
        assert np.array_equal(i0, a0) and np.array_equal(i1, a1) and np.array_equal(t.view(np.uint32), at.view(np.uint32))


def test_cases_reach_their_edges():
    cases = {c[0]: c for c in cb.cases()}
    assert len(cases) == len(cb.cases())
    shapes = {(c[1].shape[1:], c[2]) for c in cases.values()}
    for want in (((1, 1), (1, 1)), ((1, 1), (7, 5)), ((3, 2), (3, 2)), ((4, 5), (33, 70)), ((17, 17), (64, 65)),
                 ((2, 9), (40, 512)), ((9, 2), (512, 40)), ((13, 13), (224, 224)), ((17, 17), (288, 288)), ((64, 64), (64, 64)),
                 ((64, 64), (512, 512))):
        assert want in shapes, want
    assert {c[3] for c in cases.values()} >= {0.0, 0.2, 1.0} and {len(c[1]) for c in cases.values()} == {1, 7}
    assert 64 < 70 <= 96 and 65 % 32 == 1 and 512 == ore.CAM_BOX_MAX_SIDE  # W crosses two word boundaries; one bit in the last word; the cap
    ref = {n: cb.reference(n) for n in cases}
    full = lambda n: (0, 0) + cases[n][2]  # noqa: E731
    # the masks: what each is there for
    sp = cb.spiral()
    comps = cb.components(sp > 0)
    assert len(comps) == 1 and comps[0][0] == int(sp.sum()) > 16 * 64 and ref["64x64-spiral"][2][0] == int(sp.sum())
    tie = cb.components(cb.tie_blobs() > 0)
    assert [c[0] for c in tie] == [16, 16] and tie[1][1][1] < tie[0][1][1]  # the later one lies further left
    assert tuple(ref["64x64-tie"][1][0]) == tie[0][1] == (5, 40, 9, 44)
    assert tuple(ref["64x64-diagonal"][1][0]) == (10, 10, 20, 20) and ref["64x64-diagonal"][2][0] == 50 > 30 > 25
    assert len(cb.components(cb.dots() > 0)) == 1024 and tuple(ref["64x64-dots"][1][0]) == (0, 0, 1, 1) and ref["64x64-dots"][2][0] == 1
    assert tuple(ref["64x64-full"][1][0]) == full("64x64-full") and ref["64x64-full"][2][0] == 64 * 64
    fr = cb.components(cb.frame() > 0)
    assert len(fr) == 2 and fr[0][0] > fr[1][0] == 121 and tuple(ref["64x64-frame"][1][0]) == (4, 4, 60, 60)
    # the special values
    assert tuple(ref["constant"][1][0]) == full("constant") and ref["constant"][2][0] == 20 * 16  # thr = lo = hi
    assert np.isnan(cases["nans"][1]).any() and not np.isnan(cases["nans"][1]).all() and (ref["nans"][2] > 0).all()
    assert np.isnan(ref["nans"][0]).any()
    assert np.isnan(cases["all-nan"][1]).all() and tuple(ref["all-nan"][1][0]) == (0, 0, 0, 0) and ref["all-nan"][2][0] == 0
    assert np.isposinf(cases["inf"][1]).sum() == 1 and ref["inf"][2][0] > 0 and ref["inf-frac0"][2][0] == 0
    assert (cases["negative"][1] < 0).all() and 0 < ref["negative"][2][0] < 30 * 29
    assert 64 * 64 == ore.CAM_BOX_MAX_MAP and 1 < ref["64x64-512x512"][2][0] < 512 * 512 // 16
    assert (ref["4x5-33x70-frac0"][2] == 33 * 70).all() and (ref["4x5-33x70-frac1"][2] >= 1).all()
    assert (ref["4x5-33x70-frac1"][2] < ref["4x5-33x70"][2]).all()
    # random upsampled planes under a higher threshold fall into several components: the choice among them is exercised
    for name in ("13x13-224x224-frac06", "4x5-33x70-frac06"):
        assert any(len(cb.components(cb.mask_of(u, 0.6))) > 2 for u in ref[name][0]), name
    for name, (u, boxes, areas) in ref.items():
        H, W = cases[name][2]
        assert (boxes[:, 0] <= boxes[:, 2]).all() and (boxes[:, 2] <= H).all() and (boxes[:, 3] <= W).all()
        assert (areas <= (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).all()


def test_box_to_source_lands_on_the_taps():
    """A window pixel's box, mapped back, is centred on the source coordinate whose neighbours ore.resize_taps names:
    (centre - 1/2) lies between i0 and i1 and its fraction is t."""
    src, resized, origin, out = (375, 500), (256, 341), (16, 58), (224, 224)
    for axis in (0, 1):
        i0, i1, t = ore.resize_taps(src[axis], resized[axis], origin[axis], out[axis])
        for flip in (False, True):
            for o in (0, 1, 57, out[axis] - 1):
                box = [3, 5, 4, 6]
                box[axis], box[axis + 2] = o, o + 1
                got = ore.box_to_source(box, src, resized, origin, out, flip=flip)
                centre = (got[axis] + got[axis + 2]) / 2 - 0.5
                k = out[1] - 1 - o if (flip and axis == 1) else o  # the resized column a flipped descriptor reads
                assert i0[k] <= centre <= i0[k] + 1 and abs(centre - (i0[k] + float(t[k]))) < 1e-4, (axis, flip, o)
                assert got[axis + 2] - got[axis] == pytest.approx(src[axis] / resized[axis])
    # the whole window of an uncropped, unscaled image is the image; flipped or not
    assert ore.box_to_source((0, 0, 8, 9), (8, 9), (8, 9), (0, 0), (8, 9)) == (0.0, 0.0, 8.0, 9.0)
    assert ore.box_to_source((1, 2, 3, 4), (8, 9), (8, 9), (0, 0), (8, 9), flip=True) == (1.0, 5.0, 3.0, 7.0)
    with pytest.raises(ore.OreError, match="box_to_source"):
        ore.box_to_source((0, 0, 1, 1), (8, 9), (8, 9), (1, 0), (8, 9))


# ------------------------------------------------------------------------------------------ the argument checks
def _fails(status):
    assert status == INVALID
    msg = ore.load().ore_last_error(None)
    assert msg
    return msg


def _up(maps=P, planes=3, hm=13, wm=13, h=224, w=224, out=P, ctx=None):
    return ore.load().ore_upsample_maps_f32(ctx, maps, planes, hm, wm, h, w, out)


def _boxes(maps=P, planes=3, hm=13, wm=13, h=224, w=224, frac=0.2, boxes=P, areas=P, ctx=None):
    return ore.load().ore_cam_boxes_f32(ctx, maps, planes, hm, wm, h, w, frac, boxes, areas)


def _host(hm=13, wm=13, h=224, w=224, frac=0.2, map_=None, box=True, area=True):
    m = np.zeros((max(hm, 1), max(wm, 1)), np.float32) if map_ is None else map_
    b, a = (ctypes.c_int32 * 4)(7, 7, 7, 7), ctypes.c_int32(7)
    st = ore.load().ore_cam_box_host(m.ctypes.data_as(ctypes.c_void_p), hm, wm, h, w, frac, b if box else None,
                                     ctypes.byref(a) if area else None)
    return st, tuple(b), a.value


def test_names_and_constants():
    text = open(HEADER).read()
    defs = dict(re.findall(r"#define (ORE_\w+) (-?\d+)", text))
    assert int(defs["ORE_ABI_VERSION"]) == 2 == ore.ABI_VERSION  # additions only
    assert int(defs["ORE_CAM_BOX_MAX_MAP"]) == 4096 == ore.CAM_BOX_MAX_MAP
    assert int(defs["ORE_CAM_BOX_MAX_SIDE"]) == 512 == ore.CAM_BOX_MAX_SIDE
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTED and hasattr(ore.load(), name)
    for fn in ("upsample_maps", "cam_boxes", "cam_box_reference", "box_to_source"):
        assert callable(getattr(ore, fn)), fn
    for attr in ("set_cam_boxes", "classify_boxes", "classify_boxes_u8", "classify_boxes_u8_list"):
        assert hasattr(ore.Model, attr), attr


def test_upsample_argument_checks_in_order():
    assert b"null" in _fails(_up(maps=None, planes=-1))  # the pointers come first
    assert b"null" in _fails(_up(out=None, hm=0))
    assert b"planes" in _fails(_up(planes=-1, hm=0))
    for kw, what in (({"hm": 0}, b"hm = 0"), ({"wm": 16385}, b"wm = 16385"), ({"h": 0, "hm": 1}, b"h = 0"), ({"w": 16385}, b"w = 16385")):
        assert what in _fails(_up(**kw, planes=1 << 40))  # sizes before the product
    assert b"h = 12 below hm = 13" in _fails(_up(h=12, planes=1 << 40))
    assert b"w = 12 below wm = 13" in _fails(_up(w=12))
    assert b"2^31" in _fails(_up(planes=(1 << 31) // (224 * 224) + 1))
    # in range (the largest plane count included, and no Hm Wm or 512 cap here): only the context is missed
    assert b"null" in _fails(_up(planes=((1 << 31) - 1) // (224 * 224)))
    assert b"null" in _fails(_up(hm=100, wm=100, h=16384, w=16384, planes=7))
    assert b"null" in _fails(_up(planes=0))  # planes == 0 still needs a context


def test_boxes_argument_checks_in_order():
    assert b"null" in _fails(_boxes(maps=None, planes=-1))
    assert b"null" in _fails(_boxes(boxes=None, hm=0))
    assert b"planes = -1" in _fails(_boxes(planes=-1, hm=0))
    for hm, wm in ((0, 13), (13, 0), (-1, 5), (64, 65), (4097, 1), (1, 4097)):
        msg = _fails(_boxes(hm=hm, wm=wm, h=1000))  # the map before the sides
        assert b"hm x wm" in msg and b"ORE_CAM_BOX_MAX_MAP" in msg
    for h in (0, 513):
        msg = _fails(_boxes(h=h, w=513))  # h before w
        assert b"h = %d" % h in msg and b"ORE_CAM_BOX_MAX_SIDE" in msg
    for w in (0, 513):
        assert b"w = %d" % w in _fails(_boxes(w=w, h=12))  # the caps before h < hm
    assert b"h = 12 below hm = 13" in _fails(_boxes(h=12, w=12))
    assert b"w = 12 below wm = 13" in _fails(_boxes(w=12, frac=2.0))  # the sizes before frac
    for frac in (-0.001, 1.001, float("nan"), float("inf")):
        assert b"frac" in _fails(_boxes(frac=frac))
    # in range, at the caps, areas NULL: only the context is missed
    assert b"null" in _fails(_boxes(hm=64, wm=64, h=512, w=512, frac=1.0, areas=None))
    assert b"null" in _fails(_boxes(hm=1, wm=512, h=1, w=512, frac=0.0))
    assert b"null" in _fails(_boxes(planes=0))


def test_host_entry_argument_checks_in_order():
    L = ore.load()
    b = (ctypes.c_int32 * 4)()
    assert L.ore_cam_box_host(None, 13, 13, 224, 224, 0.2, b, None) == INVALID and b"null" in L.ore_last_error(None)
    st, box, area = _host(box=False, hm=0)
    assert st == INVALID and b"null" in L.ore_last_error(None)
    for kw, what in (({"hm": 65, "wm": 64, "h": 1000}, b"hm x wm"), ({"h": 513, "w": 513}, b"h = 513"), ({"w": 513, "h": 12}, b"w = 513"),
                     ({"h": 12, "w": 12}, b"h = 12 below"), ({"w": 12, "frac": 2.0}, b"w = 12 below"), ({"frac": -1.0}, b"frac"),
                     ({"frac": float("nan")}, b"frac")):
        st, box, area = _host(**kw)
        assert st == INVALID and what in L.ore_last_error(None), kw
        assert box == (7, 7, 7, 7) and area == 7  # nothing written
    st, box, area = _host(hm=2, wm=2, h=4, w=4, area=False)  # a NULL area is allowed
    assert st == 0 and box == (0, 0, 4, 4)


def test_model_entry_with_a_null_model():
    assert b"null" in _fails(ore.load().ore_model_set_cam_boxes(None, P, P, 10, 0.2))
    assert b"null" in _fails(ore.load().ore_model_set_cam_boxes(None, None, None, 0, 0.0))
