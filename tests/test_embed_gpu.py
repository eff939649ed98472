"""GPU: the model's embedding (ore_model_set_embed) on the calibrated SqueezeNet at a small input size, f32 and f16,
under ORE_FUSE_ALL and fusion 0: against the float64 plane means of the map conv's input read back from the same
run, equal bit for bit under both fusion settings, without effect on scores and classes, and through ore.nearest."""
import numpy as np
import pytest

from _sizes import SEED, SIZES

pytestmark = pytest.mark.gpu
HW, N, K = SIZES[0], 3, 5
X_NAME = "fire9/concat_2"  # conv10's input


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_embeddings(gpu_ctx, precision):
    """Bound of a raw element: P 2^-24 mean|X| -- an f32 sum of P exact terms in any order, then one division.  The
    normalised one adds C 2^-24 relative: the f32 sum of C squares, its root and the division."""
    import torch
    import ore
    from ore import squeezenet
    x = torch.from_numpy(squeezenet.synthetic_input(N, HW, seed=SEED)).cuda()
    m = ore.Model(gpu_ctx, squeezenet.build_calibrated(HW), max_batch=N, precision=precision)
    try:
        m.set_topk(K)
        C = m.embed_dim
        got = []
        for fusion in (ore.FUSE_ALL, 0):
            m.set_fusion(fusion)
            plain = m.classify(x)
            s1, c1, raw = m.classify_embed(x, normalize=False)
            unit = torch.empty((N, C), dtype=torch.float32, device="cuda")
            m.set_embed_output(unit)  # normalised, into a buffer of the caller's; X stays readable behind the run
            s2, c2 = m.classify(x)
            X = m.read_value(X_NAME).astype(np.float64)
            m.set_embed_output(None)
            torch.cuda.synchronize()
            for s, c in ((s1, c1), (s2, c2)):
                assert torch.equal(c, plain[1]) and np.array_equal(_bits(s), _bits(plain[0])), "classify outputs changed"
            assert X.shape[:2] == (N, C) and tuple(raw.shape) == (N, C)
            P = X.shape[2] * X.shape[3]
            mu, b = X.mean(axis=(2, 3)), P * 2.0 ** -24 * np.abs(X).mean(axis=(2, 3))
            err = np.abs(raw.cpu().numpy() - mu)
            norm = np.linalg.norm(mu, axis=1, keepdims=True)
            ref = mu / norm
            err_n, tol_n = np.abs(unit.cpu().numpy() - ref), b / norm + C * 2.0 ** -24 * np.abs(ref)
            print(f"{precision} fusion {fusion}: raw err / bound {(err[b > 0] / b[b > 0]).max():.3g}, "
                  f"normalised {(err_n[tol_n > 0] / tol_n[tol_n > 0]).max():.3g}")
            assert (err <= b).all() and (err_n <= tol_n).all()
            got.append((_bits(raw), _bits(unit)))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), "the fusion flags show"
        v, i = ore.nearest(gpu_ctx, unit, unit, 1)  # end to end: every image finds itself
        assert i[:, 0].cpu().tolist() == list(range(N)) and (v[:, 0].cpu() - 1).abs().max() <= 1e-5
    finally:
        m.close()
