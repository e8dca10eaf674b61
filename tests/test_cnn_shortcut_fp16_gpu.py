"""The fused 1x1 projection shortcuts of the first blocks of stages 3 and 4 as fp16x2 products (conv_rw_kernel<.., SC> and
conv_bf3flat_kernel<.., SC>; include/cpx.h: cpx_cnn_set_residual_bounds, CPX_CNN_SHORTCUT_FP16), judged block by block against
the float64 oracle with the criteria and helpers of test_cnn_blocks_gpu.py: err = max |got - want| / mag per block, each
block's oracle fed the device's own output of the block before.
  every block and the head, fp16 route and float32 route alike      err <= 4e-6
  the projection blocks 3b0 and 4b0 on the batch an f32 forward ran   err <= 2 err_f32 + 2^-24"""
import ctypes as C

import numpy as np
import pytest

from test_cnn_blocks_gpu import LAUNCH_TABLES, NAMES, TOL, _assert_f32_accurate, _block_errs, _input, _model, _report, _run

pytestmark = pytest.mark.gpu
K3B0, K4B0 = NAMES.index("3b0"), NAMES.index("4b0")


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3")
    yield eng
    eng.close()


def _engine_under(monkeypatch, value):
    """A fresh engine created under CPX_CNN_SHORTCUT_FP16=value (the switch is read when a handle is created)."""
    from cpx.engine import TrackEngine

    monkeypatch.setenv("CPX_CNN_SHORTCUT_FP16", value)
    eng = TrackEngine(model="lepton3")
    monkeypatch.delenv("CPX_CNN_SHORTCUT_FP16")
    return eng


def _forward(eng, w, x, mode="fp16x2", timing=False, prepare=None):
    """One forward with taps on a fresh network -> (logits, taps, overflow words, conv_timing table or None)."""
    from cpx.ml_tools import wrresnet as wr

    eng.set_cnn_math(mode)
    net = wr.WRResNetDevice(eng, w, 17)
    try:
        if prepare:
            prepare(net)
        if timing:
            eng.conv_timing(True)
        logits, taps, ovf = _run(net, eng, x)
        table = None
        if timing:
            table = {key: (launches, flops) for key, (launches, _, flops) in eng.conv_timing().items()}
            eng.conv_timing(False)
    finally:
        net.close()
        eng.set_cnn_math(eng.DEFAULT_CNN_MATH)
    return logits, taps, ovf, table


_F32_ERRS = {}


def _f32_errs(eng, key, w, x):
    """Per-block errors of an f32 forward of the batch (the projection blocks' yardstick), computed once per case."""
    if key not in _F32_ERRS:
        logits, taps, _, _ = _forward(eng, w, x, mode="f32")
        _F32_ERRS[key] = _block_errs(w, x, logits, taps)[0]
    return _F32_ERRS[key]


def _check_projection_blocks(case, w, x, logits, taps, errs_f32):
    errs, herr = _block_errs(w, x, logits, taps)
    _report(case, "fp16x2", errs, herr)
    _assert_f32_accurate(case, "fp16x2", errs, herr)
    for k in (K3B0, K4B0):
        print("%s %s err %.3e  f32 %.3e" % (case, NAMES[k], errs[k], errs_f32[k]))
        assert errs[k] <= 2.0 * errs_f32[k] + 2.0 ** -24, (case, NAMES[k], errs[k], errs_f32[k])
    return errs


# 2 x 48 x 48: stage 3 at 24 x 24 is one full tile plus a ragged 8, stage 4 at 8 x 8; 2 x 37 x 37: odd maps (19 x 19, 7 x 7), the
# strided operand's last row and column sit where SAME padding's surplus lies; 1 x 20 x 20: a map smaller than a tile;
# 2 x 96 x 160: non-square
SHAPES = [(2, 48, 48), (2, 37, 37), (1, 20, 20), (2, 96, 160)]


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_fp16_shortcut_blocks_are_f32_accurate(engine, n, h, w):
    x = _input(n, h, w, 900 + h + w + n)
    wt = _model(6, x)
    errs_f32 = _f32_errs(engine, (n, h, w), wt, x)
    logits, taps, ovf, _ = _forward(engine, wt, x)
    assert not ovf.any(), ovf
    _check_projection_blocks("sc fp16 %dx%dx%d" % (n, h, w), wt, x, logits, taps, errs_f32)


def test_the_route_is_taken_and_the_switch_restores_the_float32_side_product(engine, monkeypatch):
    """The same batch under CPX_CNN_SHORTCUT_FP16=0 and =1 on fresh engines: float32 products and fp16-plane products are
    different roundings, so 3b0 and 4b0 differ in bits.  Stage 2 is bit-equal.  Both forms meet the accuracy criteria, and
    both show the launch table test_cnn_blocks_gpu.py pins for fp16x2 (the shortcut's FLOPs are not counted there).
    (4b0's input already differs, being 3b2's output: that 4b0's OWN shortcut takes the new route is what the guard test
    below shows, whose overflow word only that route can raise.)"""
    x = _input(2, 48, 48, 1)
    w = _model(2, x)
    errs_f32 = _f32_errs(engine, "switch", w, x)
    got = {}
    for value in ("0", "1"):
        eng = _engine_under(monkeypatch, value)
        try:
            got[value] = _forward(eng, w, x, timing=True)
        finally:
            eng.close()
        logits, taps, ovf, table = got[value]
        assert not ovf.any(), (value, ovf)
        _check_projection_blocks("switch=%s 2x48x48" % value, w, x, logits, taps, errs_f32)
        assert table == LAUNCH_TABLES["fp16x2"], (value, table)
    for k in range(3):
        assert np.array_equal(got["0"][1][k], got["1"][1][k]), NAMES[k]
    assert not np.array_equal(got["0"][1][K3B0], got["1"][1][K3B0])
    assert not np.array_equal(got["0"][1][K4B0], got["1"][1][K4B0])
    # the default handle is the =1 form
    logits, taps, _, _ = _forward(engine, w, x)
    for k in range(9):
        assert np.array_equal(taps[k], got["1"][1][k]), NAMES[k]
    assert np.array_equal(logits, got["1"][0])


def test_the_operand_guard_alone_sends_the_block_to_the_rerun(engine):
    """A calibrated model whose residual bounds are then set to 2^-10 of their computed values: the operand's scale is 2^10
    larger, the calibration batch itself leaves fp16's range in the shortcuts' operands and nowhere else, so exactly 3b0
    and 4b0 raise their overflow words, the rerun computes them, and every block is float32-accurate."""
    x = _input(2, 48, 48, 31)
    w = _model(12, x)

    def shrink(net):
        assert all(b > 0 for b in net.res_bounds)
        bounds = (C.c_float * 3)(*[b * 2.0 ** -10 for b in net.res_bounds])
        assert engine.lib.cpx_cnn_set_residual_bounds(net._cnn, bounds, 3) == 0

    logits, taps, ovf, _ = _forward(engine, w, x, prepare=shrink)
    print("overflow words", ovf.tolist())
    want = np.zeros(9, dtype=bool)
    want[K3B0] = want[K4B0] = True
    assert np.array_equal(ovf != 0, want), ovf
    assert engine.cnn_last_overflow()
    errs, herr = _block_errs(w, x, logits, taps)
    _report("guard 2^-10", "fp16x2", errs, herr, ovf)
    _assert_f32_accurate("guard 2^-10", "fp16x2", errs, herr)
    # ... and with the bounds as computed the same batch raises nothing
    _, _, ovf, _ = _forward(engine, w, x)
    assert not ovf.any(), ovf


def test_no_bound_no_change(engine, monkeypatch):
    """A network that never receives a residual bound (created by cpx_cnn_create through ctypes, with the activation bounds
    alone, as a caller of the C interface before this entry point existed) computes the bits of the
    CPX_CNN_SHORTCUT_FP16=0 form; a bound of 0 set later returns a network to it; and the entry point refuses a wrong count, a negative and a non-finite bound."""
    from cpx.ml_tools import wrresnet as wr

    x = _input(2, 48, 48, 1)
    w = _model(2, x)
    eng0 = _engine_under(monkeypatch, "0")
    try:
        logits0, taps0, _, _ = _forward(eng0, w, x)
    finally:
        eng0.close()
    # a network made by cpx_cnn_create through ctypes, given the activation bounds (the entry point that existed before) and
    # never the residual ones; the WRResNetDevice beside it only holds the uploaded parameters and issues the forward
    engine.set_cnn_math("fp16x2")
    net = wr.WRResNetDevice(engine, w, 17)
    raw = C.c_void_p()
    try:
        prm = net._native_params()
        assert engine.lib.cpx_cnn_create(engine.h, C.byref(prm), C.byref(raw)) == 0
        bounds = (C.c_float * len(net.act_bounds))(*net.act_bounds)
        assert engine.lib.cpx_cnn_set_activation_bounds(raw, bounds, len(net.act_bounds)) == 0
        wrapped, net._cnn = net._cnn, raw
        try:
            logits, taps, ovf = _run(net, engine, x)
        finally:
            net._cnn = wrapped
    finally:
        if raw:
            engine.lib.cpx_cnn_destroy(raw)
        net.close()
        engine.set_cnn_math(engine.DEFAULT_CNN_MATH)
    assert not ovf.any()
    for k in range(9):
        assert np.array_equal(taps[k], taps0[k]), NAMES[k]
    assert np.array_equal(logits, logits0)

    def zero(net):
        assert engine.lib.cpx_cnn_set_residual_bounds(net._cnn, (C.c_float * 3)(0.0, 0.0, 0.0), 3) == 0

    _, taps, _, _ = _forward(engine, w, x, prepare=zero)
    for k in range(9):
        assert np.array_equal(taps[k], taps0[k]), NAMES[k]

    net = wr.WRResNetDevice(engine, w, 17)
    try:
        good = (C.c_float * 4)(100.0, 100.0, 100.0, 100.0)
        for n in (2, 4, 0, 18):
            assert engine.lib.cpx_cnn_set_residual_bounds(net._cnn, good, n) == -1  # CPX_ERR_INVALID
            assert "cpx_cnn_set_residual_bounds" in engine._err()
        for bad in (-1.0, float("nan"), float("inf")):
            assert engine.lib.cpx_cnn_set_residual_bounds(net._cnn, (C.c_float * 3)(100.0, bad, 100.0), 3) == -1
            assert "cpx_cnn_set_residual_bounds" in engine._err()
        assert engine.lib.cpx_cnn_set_residual_bounds(net._cnn, None, 3) == -1
    finally:
        net.close()


def test_a_folded_model_measures_its_residual_bounds(engine, tmp_path):
    """A .tflite model's BatchNorms arrive folded: the residual bounds are measured on the probe batch, with the
    activation bounds' headroom.  On the probe's distribution (uniform 0..255) the forward raises no overflow word and
    every block is float32-accurate."""
    from cpx.ml_tools import wrresnet as wr
    from cpx.ml_tools.tflite_reader import load_tflite
    from test_tflite_import_cpu import tflite_of

    rng = np.random.default_rng(77)
    x = rng.uniform(0, 255, size=(2, 64, 64, 2)).astype(np.float32)
    w0 = _model(8, x)
    p = tmp_path / "m.tflite"
    p.write_bytes(tflite_of(w0, ()))
    w = load_tflite(p)
    seen = {}

    def look(net):
        seen["res"], seen["act"] = list(net.res_bounds), list(net.act_bounds)

    logits, taps, ovf, _ = _forward(engine, w, x, prepare=look)
    assert len(seen["res"]) == 3 and all(b > 0 and np.isfinite(b) for b in seen["res"]), seen
    # measured, not the identity marker's statistics: far above 64 sqrt(1) for stages 3 and 4 of a calibrated network
    assert seen["res"] != [wr.residual_bound(w, s) for s in (2, 3, 4)]
    assert not ovf.any(), ovf
    errs, herr = _block_errs(w, x, logits, taps)
    _report("tflite 2x64x64", "fp16x2", errs, herr, ovf)
    _assert_f32_accurate("tflite", "fp16x2", errs, herr)
