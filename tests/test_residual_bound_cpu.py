"""The host side of the fp16 shortcut (include/cpx.h: cpx_cnn_set_residual_bounds): the bound of a stage's first-block
input from the statistics of the BatchNorm that normalises it, and the host's choice of the operand's power-of-two scale
(cpx_cnn_shortcut_scale: pure arithmetic, no device)."""
import ctypes as C
import math

import numpy as np
import pytest


def test_residual_bound_is_mean_plus_sigmas_of_the_first_batchnorm():
    from cpx.ml_tools import wrresnet as wr

    w = wr.random_weights(17, seed=9)
    rng = np.random.default_rng(5)
    for stage, c in ((2, 16), (3, 64), (4, 128)):
        name = "bn%db0_branch2a" % stage
        w[name + "/moving_mean"] = rng.normal(0, 30.0 * stage, size=c).astype(np.float32)
        w[name + "/moving_variance"] = rng.uniform(0.0, 900.0, size=c).astype(np.float32)
    w["bn3b0_branch2a/moving_variance"][7] = 0.0          # a dead channel: eps alone under the root
    w["bn4b0_branch2a/moving_mean"][3] = -5000.0          # the bound is of |x|: a large negative mean counts
    for stage in (2, 3, 4):
        name = "bn%db0_branch2a" % stage
        mean = w[name + "/moving_mean"].astype(np.float64)
        var = w[name + "/moving_variance"].astype(np.float64)
        for sigmas in (64.0, 8.0):
            want = max(abs(m) + sigmas * math.sqrt(v + 1e-3) for m, v in zip(mean, var))
            got = wr.residual_bound(w, stage, sigmas=sigmas)
            assert got == pytest.approx(want, rel=1e-12), (stage, sigmas)
        assert wr.residual_bound(w, stage) == wr.residual_bound(w, stage, sigmas=64.0)
    assert wr.residual_bound(w, 4) >= 5000.0
    # other layers' statistics do not enter
    w["bn3b1_branch2a/moving_mean"][:] = 1e9
    w["bn3b0_branch2b/moving_mean"][:] = 1e9
    assert wr.residual_bound(w, 3) < 1e6


def _scale(bound, wmax):
    from cpx import _lib

    lib = _lib.load()
    sx = C.c_float(-1.0)
    found = lib.cpx_cnn_shortcut_scale(C.c_float(bound), C.c_float(wmax), C.byref(sx))
    return found, float(sx.value)


def _window(bound, wmax):
    """Every exponent e for which 2^e satisfies the conditions of include/cpx.h, by trying them all."""
    return [e for e in range(-80, 81)
            if 2.0 ** 3 <= bound * 2.0 ** e <= 2.0 ** 15 and 2.0 ** -1 <= wmax / 2.0 ** e < 2.0 ** 15]


# (bound of the operand, largest scaled weight): the calibrated test networks' stage 3 and 4 (about 2077 / 1024 and
# 1162 / 1448), the same with the bound 2^-10 of that, bounds and weights at a window's edges, tiny and huge pairs
PAIRS = [(2076.7, 1023.7), (1162.2, 1448.0), (2076.7 / 1024, 1023.7), (1162.2 / 1024, 1448.0), (1.0, 8.0), (4096.0, 0.5),
         (8.0, 2.0 ** 14), (3.0e-3, 6.0e4), (2.5e4, 7.0), (1e-3, 1e-3 * 2.0 ** 25), (300.0, 2.0 ** 20)]


@pytest.mark.parametrize("bound,wmax", PAIRS)
def test_a_scale_is_found_inside_the_window_and_near_two_to_the_twelve(bound, wmax):
    window = _window(bound, wmax)
    assert window, "the case is meant to have a scale"
    found, sx = _scale(bound, wmax)
    assert found == 1
    m, e = math.frexp(sx)
    assert m == 0.5 and (e - 1) in window, (sx, window)   # a power of two that meets every condition
    # ... and of those the one that brings the bound to 2^12 at most (2^11 <= bound sx <= 2^12), or the nearest the window has
    target = 12 - math.frexp(bound)[1]
    assert 2.0 ** 11 <= bound * 2.0 ** target <= 2.0 ** 12
    assert e - 1 == min(max(target, window[0]), window[-1]), (sx, target, window)


@pytest.mark.parametrize("bound,wmax", [
    (2076.7, 1023.7 * 2.0 ** -20),   # shortcut weights 2^20 below the main layer's: their low plane would be lost
    (2076.7, 1023.7 * 2.0 ** 20),    # ... and 2^20 above: the operand would have to sit below its own low plane
    (1e-30, 1e30), (1e30, 1e-30),
])
def test_no_scale_keeps_float32(bound, wmax):
    assert not _window(bound, wmax)
    assert _scale(bound, wmax) == (0, 0.0)


@pytest.mark.parametrize("bound,wmax", [(0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (float("nan"), 1.0), (1.0, float("inf")),
                                        (float("inf"), 1.0)])
def test_no_usable_bound_keeps_float32(bound, wmax):
    assert _scale(bound, wmax) == (0, 0.0)
