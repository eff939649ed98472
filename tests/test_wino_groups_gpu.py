"""Grouped workgroups of the LDS Winograd kernel (tile "wino lds") on the GPU: bit-identity with the register
kernel "wino 32x32 d4" on launches that mix large m-groups and single-block workgroups.
tests/test_wino_gpu.py::test_wino_tiles_bit_identical stays below the 2048 workgroups grouping needs; these
shapes (tiny odd planes, many images, from _wino_groups.GROUPED_CASES) reach it, with a partial last channel
block and tile groups that span images.  The geometry is re-derived for the device's CU count, so the test
cannot pass without exercising what it is there for."""
import numpy as np
import pytest

from _convref import _conv_model
from _knobs import conv_tile
from _wino_groups import GROUPED_CASES, dump, properties

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", GROUPED_CASES)
def test_wino_lds_groups_bit_identical(gpu_ctx, case):
    import torch
    import ore
    N, C, H, W, M = case
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    geo = dump(ncu, [(N, H, W, M)])[0]
    props = properties(case, geo)
    assert all(props.values()), (ncu, props)
    g = torch.Generator(device="cuda")
    g.manual_seed(sum(case))
    x = (torch.rand((N, C, H, W), generator=g, device="cuda") - 0.5) * 100.0
    rng = np.random.default_rng(3)
    w = rng.standard_normal((M, C, 3, 3)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, M).astype(np.float32)
    mb = _conv_model((1, C, H, W), w, b, [1] * 4, [1, 1])
    outs = []
    for name in ("wino 32x32 d4", "wino lds"):
        t = ore.Model.TILE_NAMES.index(name)
        with conv_tile(gpu_ctx, t):
            m = ore.Model(gpu_ctx, mb, max_batch=N)
        y = m.run(x)
        torch.cuda.synchronize()
        assert m.tiles()[0] == t, (m.tiles(), t)
        outs.append(y.cpu().numpy())
        m.close()
        del y
    assert np.abs(outs[0]).max() > 1.0
    np.testing.assert_array_equal(outs[0], outs[1])
