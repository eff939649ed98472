"""CPU: the resize's tap map (ore_resize_taps, csrc/ore_resize_geom.h -- the one the kernels use) against the
numpy statement of include/ore.h, exactly; that statement against torch's CPU bilinear interpolation, to
anchor the convention (half-pixel centres, no antialiasing); and the Python geometry helper."""
import numpy as np
import pytest

import ore
from _resize_ref import images, resize_ref, taps_ref


def _same(S, D, origin, count):
    i0, i1, t = ore.resize_taps(S, D, origin, count)
    r0, r1, rt = taps_ref(S, D, origin, count)
    assert i0.dtype == np.int32 and i1.dtype == np.int32 and t.dtype == np.float32
    np.testing.assert_array_equal(i0, r0, err_msg=f"i0 {S}->{D}")
    np.testing.assert_array_equal(i1, r1, err_msg=f"i1 {S}->{D}")
    np.testing.assert_array_equal(t.view(np.uint32), rt.view(np.uint32), err_msg=f"t {S}->{D}")
    return i0, i1, t


def test_taps_exhaustive_small():
    for S in range(1, 41):
        for D in range(1, 41):
            i0, i1, t = _same(S, D, 0, D)
            assert (i0 <= i1).all() and (i1 <= S - 1).all() and (i0 >= 0).all()
            assert (t >= 0).all() and (t < 1).all()
            if D == S:
                assert (t == 0).all() and (i0 == np.arange(S)).all()


@pytest.mark.parametrize("S,D,origin,count", [(375, 256, 16, 224), (500, 341, 58, 224), (1080, 224, 0, 224),
                                               (1920, 398, 87, 224), (16384, 1, 0, 1), (1, 16384, 5000, 11384),
                                               (16384, 16384, 16000, 384), (16383, 16384, 3, 16381)])
def test_taps_spot(S, D, origin, count):
    i0, i1, t = _same(S, D, origin, count)
    assert (i0 <= i1).all() and (i1 <= S - 1).all() and (t >= 0).all() and (t < 1).all()
    if D == S:
        assert (t == 0).all()


def test_identity_resize_is_the_crop():
    """Rh, Rw = Hs, Ws: every weight is 0 and the result is the cropped bytes."""
    x = images((2, 9, 11, 3))
    got = resize_ref(x, (9, 11), (2, 3), (5, 6))
    np.testing.assert_array_equal(got, x[:, 2:7, 3:9].transpose(0, 3, 1, 2).astype(np.float32))


# source H x W x C -> resized, crop origin, crop size
TORCH_CASES = [((3, 1, 1), (9, 4), (0, 0), (9, 4)), ((7, 5, 3), (16, 12), (0, 0), (16, 12)),
               ((30, 40, 3), (17, 23), (2, 3), (11, 13)), ((97, 131, 3), (8, 8), (0, 0), (8, 8)),
               ((375, 500, 3), (256, 341), (16, 58), (224, 224)), ((61, 83, 4), (40, 52), (1, 4), (36, 44)),
               ((1080, 1920, 1), (224, 398), (0, 87), (224, 224))]


@pytest.mark.parametrize("src,resized,origin,out", TORCH_CASES, ids=lambda v: "x".join(map(str, v)))
def test_restatement_matches_torch_cpu(src, resized, origin, out):
    """Within 255 (4 (Hs + Ws) + 8) 2^-24 grey levels: the slope of a bilinear surface (at most 255 per
    pixel) times a few float32 ulps of a coordinate of magnitude up to Hs + Ws (torch computes the source
    coordinate in float32), plus the lerp's own roundings."""
    import torch
    import torch.nn.functional as F
    hs, ws, c = src
    x = images((1, hs, ws, c), seed=11)
    mine = resize_ref(x, resized, origin, out)
    xf = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).float()
    full = F.interpolate(xf, size=resized, mode="bilinear", align_corners=False, antialias=False).numpy()
    theirs = full[:, :, origin[0]:origin[0] + out[0], origin[1]:origin[1] + out[1]]
    diff = float(np.abs(mine.astype(np.float64) - theirs.astype(np.float64)).max())
    bound = 255.0 * (4 * (hs + ws) + 8) * 2.0 ** -24
    print(f"{src} -> {resized}: max |numpy - torch| = {diff:.3g} grey levels, bound {bound:.3g}")
    assert diff <= bound


def test_center_crop_geometry():
    assert ore.center_crop_geometry((375, 500), 256, (224, 224)) == ((256, 341), (16, 58))
    assert ore.center_crop_geometry((500, 375), 256, (224, 224)) == ((341, 256), (58, 16))
    assert ore.center_crop_geometry((1080, 1920), 224, (224, 224)) == ((224, 398), (0, 87))
    assert ore.center_crop_geometry((64, 64), 64, (64, 64)) == ((64, 64), (0, 0))
    assert ore.center_crop_geometry((100, 100), 33, (32, 31)) == ((33, 33), (0, 1))
    with pytest.raises(ore.OreError):
        ore.center_crop_geometry((375, 500), 200, (224, 224))  # the crop is larger than the resized image
    with pytest.raises(ore.OreError):
        ore.center_crop_geometry((0, 500), 256, (224, 224))
