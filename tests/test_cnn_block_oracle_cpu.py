"""The float64 per-block oracle (oracle/cnn_oracle.py: first_block64, block64, head64) against the float32 forward it
restates: chained block by block it gives forward()'s logits, and its magnitudes bound the values they are the error
scale of.  CPU only; tests/test_cnn_blocks_gpu.py holds the device's blocks to it."""
import numpy as np
import pytest


@pytest.mark.parametrize("shape,dense_sizes,activation", [((2, 40, 40), None, "sigmoid"), ((1, 24, 37), (48, 24), "softmax")])
def test_chained_blocks_reproduce_forward(shape, dense_sizes, activation):
    import cnn_oracle as co
    from cpx.ml_tools import wrresnet as wr

    rng = np.random.default_rng(7)
    x = rng.uniform(0, 255, size=shape + (2,)).astype(np.float32)
    x[:, ::5, :, 1] = 0.0
    w = co.calibrate_bn(wr.random_weights(17, seed=6, dense_sizes=dense_sizes, activation=activation), x)
    want, _ = co.forward(w, x)
    a, mag = co.first_block64(w, x)
    n_blocks = 1
    assert a.shape == shape + (wr.FILTERS[1],)
    assert np.all(mag >= np.abs(a)) and np.all(np.isfinite(mag))
    for si, stage in enumerate((2, 3, 4)):
        for d in range(wr.BLOCKS):
            if (stage, d) == (2, 0):
                continue
            a, mag = co.block64(w, stage, d, a)
            n_blocks += 1
            assert a.dtype == np.float64 and a.shape[-1] == wr.FILTERS[si + 1]
            assert np.all(mag >= np.abs(a)), (stage, d)
            assert float(np.abs(a).max()) > 0.0  # (non-degenerate: a block that kills every activation pins nothing)
    assert n_blocks == 3 * wr.BLOCKS
    logits, hmag = co.head64(w, a)
    assert np.all(hmag >= np.abs(logits))
    assert float(np.abs(want).max()) > 0.05
    assert float(np.abs(logits - want).max()) <= 1e-5, float(np.abs(logits - want).max())


def test_block_magnitude_is_the_error_scale():
    """mag is what float32 rounding is relative to: the same block computed from float32-rounded operands (input,
    weights and every intermediate) stays within the per-block bound the GPU test holds the device's blocks to."""
    import torch

    import cnn_oracle as co
    from cpx.ml_tools import wrresnet as wr

    rng = np.random.default_rng(8)
    x = rng.uniform(0, 255, size=(2, 30, 30, 2)).astype(np.float32)
    w = co.calibrate_bn(wr.random_weights(17, seed=2), x)
    a, _ = co.first_block64(w, x)
    a32 = a.astype(np.float32)
    for stage, d in ((2, 1), (3, 0), (3, 1), (4, 0)):
        want, mag = co.block64(w, stage, d, a32)
        b = "%db%d" % (stage, d)
        s = stage - 1 if d == 0 else 1
        # the block in float32 (torch CPU) from the same float32 input
        with torch.no_grad():
            t = torch.from_numpy(a32).permute(0, 3, 1, 2)
            y = torch.relu(co._bn(t, w, "bn%s_branch2a" % b))
            y = co._conv(y, w, "res%s_branch2a" % b, s, True)
            y = torch.relu(co._bn(y, w, "bn%s_branch2b" % b))
            y = co._conv(y, w, "res%s_branch2b" % b, 1, True)
            sc = co._conv(t, w, "shortcut%d" % stage, s, False) if d == 0 else t
            got = torch.relu(y + sc).permute(0, 2, 3, 1).numpy().astype(np.float64)
        err = float((np.abs(got - want) / mag).max())
        assert err <= 4e-6, (stage, d, err)
        assert err > 0.0
        a32 = got.astype(np.float32)
