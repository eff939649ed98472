"""The LDS Winograd kernel's workgroup geometry (csrc/ore_wino_geom.h: wm_groups, wm_wg_map) on the host:
every (tile group, m-block) pair is computed by exactly one workgroup, every workgroup's block range is non-empty
(but for the spare ids of a shorter XCD range) and within the layer's blocks, and within the id range an XCD
walks (blockIdx % 8 == x, ascending) the group sizes never increase: large groups first, single blocks last."""
import pytest

from _wino_groups import GROUPED_CASES, WM_CH, WM_TILES, dump, properties

# SqueezeNet-1.0 @224 expand3x3 layers: (H, W, M)
SQUEEZENET = [(54, 54, 64), (54, 54, 128), (27, 27, 192), (27, 27, 256), (13, 13, 256)]
RAGGED = [(2, 5, 7, 40), (3, 1, 1, 32), (2, 2, 3, 24), (1, 9, 1, 16), (5, 6, 6, 33), (4099, 3, 3, 96), (2900, 27, 27, 256)]
SHAPES = ([(n, h, w, m) for n in (256, 128, 1) for h, w, m in SQUEEZENET] + RAGGED +
          [(n, h, w, m) for n, _, h, w, m in GROUPED_CASES])


@pytest.fixture(scope="module", params=[256, 304, 64, 8, 1])
def geos(request):
    return dump(request.param, SHAPES)


def test_every_pair_once_and_ranges(geos):
    for shape, g in zip(SHAPES, geos):
        n, h, w, m = shape
        assert g is not None, shape
        tiles = n * ((h + 1) // 2) * ((w + 1) // 2)
        assert g["ntg"] == -(-tiles // WM_TILES) and g["mtiles"] == -(-m // WM_CH), shape
        assert g["grid"] == len(g["wgs"]) and g["grid"] % 8 == 0
        seen = set()
        spare = 0
        for tg, mb0, mb1 in g["wgs"]:
            if mb1 <= mb0:
                spare += 1
                continue
            assert 0 <= tg < g["ntg"] and 0 <= mb0 < mb1 <= g["mtiles"], (shape, tg, mb0, mb1)
            assert mb1 - mb0 <= g["mbs"], (shape, tg, mb0, mb1)  # the bias slot in LDS holds mbs blocks
            for mb in range(mb0, mb1):
                assert (tg, mb) not in seen, (shape, tg, mb)
                seen.add((tg, mb))
        assert len(seen) == g["ntg"] * g["mtiles"], shape
        assert spare < 8 * max(g["nmg"], g["mtiles"]), (shape, spare)  # spares: only the XCD ranges' difference


def test_sizes_never_increase_within_an_xcd(geos):
    for shape, g in zip(SHAPES, geos):
        for x in range(8):
            sizes = [b - a for _, a, b in g["wgs"][x::8]]
            assert all(s0 >= s1 for s0, s1 in zip(sizes, sizes[1:])), (shape, x)
            tgs = [tg for tg, a, b in g["wgs"][x::8] if b > a]
            assert tgs == sorted(tgs), (shape, x)  # a tile group's workgroups are consecutive


def test_modelled_worst_cu_no_worse_than_single_blocks():
    """The rule's own claim on a 256-CU device: with the dispatcher handing a freed CU the next workgroup id, the
    most loaded CU of an XCD runs no more blocks than with single-block groups throughout."""
    ncu = 256
    for shape, g in zip(SHAPES, dump(ncu, SHAPES)):
        for x in range(8):
            cus = [0] * (ncu // 8)
            for _, a, b in g["wgs"][x::8]:
                cus[cus.index(min(cus))] += b - a
            blocks = sum(cus)
            assert max(cus) <= -(-blocks // len(cus)), (shape, x, max(cus), blocks)


def test_squeezenet_b256_splits():
    """B = 256 on 256 CUs: fire4 keeps 4-block groups, fire2 / 3 / 6 / 7 / 8 two-block groups, each with a
    single-block tail; fire9 stays on single blocks."""
    gs = dump(256, [(256, h, w, m) for h, w, m in SQUEEZENET])
    assert [(g["mbs"], g["nsmall"] > 0) for g in gs] == [(2, True), (4, True), (2, True), (2, True), (1, False)]


def test_grouped_gpu_cases_exercise_what_they_claim():
    """tests/test_wino_groups_gpu.py's shapes have the properties it is there for (256 CUs: an MI355X)."""
    for case, g in zip(GROUPED_CASES, dump(256, [(n, h, w, m) for n, _, h, w, m in GROUPED_CASES])):
        props = properties(case, g)
        assert all(props.values()), (case, props)
