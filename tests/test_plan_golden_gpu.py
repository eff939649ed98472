"""The planner's output against a recorded fixture: for every configuration of tools/dump_plans.py (four
models x precisions x fusion flags) the launched steps (op, name, flops, bytes, mfma_flops), the tile
ids and run_batch must equal tests/golden/plans.json exactly -- strings, ints and doubles alike: the
planner's arithmetic is deterministic.  The fixture was written by tools/dump_plans.py from the library
of commit 55f8c99 (the last one with the planner inside ore_model.cpp) and is never regenerated from the
code under test.  Arena placement, the in-place Concat, padded planes and stream pairing do not show in
these records; the bit-identity tests (test_model_gpu.py, test_f16_gpu.py, test_wino_gpu.py,
test_config4_gpu.py) cover them."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump_plans():
    spec = importlib.util.spec_from_file_location("dump_plans", os.path.join(REPO, "tools", "dump_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def plans(gpu_ctx, golden):
    dp = _dump_plans()
    with open(os.path.join(golden, "plans.json")) as f:
        want = dp.unpack(json.load(f))
    return want, dp.collect(gpu_ctx)


def test_same_configurations(plans):
    want, got = plans
    assert sorted(got) == sorted(want)
    assert len(want) == 130


def test_plans_equal_fixture(plans):
    want, got = plans
    for key in want:
        w, g = want[key], got[key]
        assert g["run_batch"] == w["run_batch"], key
        assert g["tiles"] == w["tiles"], key
        assert len(g["steps"]) == len(w["steps"]), (key, [s["name"] for s in g["steps"]], [s["name"] for s in w["steps"]])
        for i, (gs, ws) in enumerate(zip(g["steps"], w["steps"])):
            assert gs == ws, f"{key}: step {i}"
