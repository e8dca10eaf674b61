"""Every residual block of the production forward (cpx_cnn_forward_taps: the same launches as cpx_cnn_forward, each
block's final output copied out) against a float64 computation of the same block (oracle/cnn_oracle.py: first_block64,
block64, head64).  Each block's oracle is fed the device's own output of the previous block, so every block is judged
alone and errors do not compound.

The criterion, per block: err = max |got - want| / mag, where mag is the block's sum of |operands| propagated through
both convolutions, the shortcut and the first convolution's error into the second (cnn_oracle.block64).  A float32
computation of the two convolutions is within a few 2^-24 of mag; the bound is the single-layer test's
(test_cnn_gpu.py: test_bf16x3_is_f32_accurate): with mag carrying the first convolution's error scale into the second,
two layers need no more.
  f32, bf16x3, fp16x2 (fp16 blocks and rerun blocks alike)   err <= 4e-6
  fp16x2 on the batch the exact modes ran                    err <= 2 err_bf16x3 + 2^-24 on every block,
                                                             err <= 2 err_f32 + 2^-24 on the projection blocks (d = 0)
  bf16x2                                                     err <= 6 x 2^-16 (two layers at 3 x 2^-16), and other
                                                             bits than bf16x3's on the stage-2 and stage-3 blocks
  head (float32 in every mode), from the last block's tap    |logits - head64| <= 4e-6 x head magnitude
Why not 2 err_f32 on every block, as for one layer: the split-operand kernels put an identity block's residual (its
input, |a| in mag) INTO the accumulators before the first product (conv_bf3_kernel: res_in_acc; the block kernels
likewise), so each of the second convolution's float32 accumulation roundings is relative to a partial sum that holds
|a|; the float32 kernel adds the residual after the last product.  Both are float32-accurate (measured on an MI355X,
3 x 160 x 160: f32 4.4e-8, bf16x3 8.4e-7, fp16x2 8.3e-7 on 2b1), but they are different summation orders, and what
fp16x2's two 11-bit planes must not add to is the exact split's error in the same order.  Blocks with a projection
shortcut accumulate no residual, and there the single-layer criterion against f32 holds as it is.
Why not err_bf16x2 > err_bf16x3 per block, as for one layer: the single-layer test draws log-normal operands, so a few
products dominate each sum and bf16x2's 2^-16 operand errors show undiluted.  A block's calibrated activations and weights
give K >= 288 products of similar size with random-signed errors: about 2^-17 / sqrt(K) of mag, the float32 accumulation's
level (measured, 3 x 160 x 160: 2b2 bf16x2 7.8e-7, bf16x3 8.7e-7; 3b0 1.6e-7, 1.8e-7).  So the block's max error does not
tell the two apart; that the blocks are bf16x2's own arithmetic is checked on their bits.
A block that drops the low fp16 plane is off by up to 2^-11 of an operand: hundreds of times the bound.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = 4e-6
NAMES = ["%db%d" % (stage, d) for stage in (2, 3, 4) for d in range(3)]


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3")
    yield eng
    eng.close()


def _model(seed, x, dense_sizes=None, activation="sigmoid"):
    import cnn_oracle as co
    from cpx.ml_tools import wrresnet as wr

    return co.calibrate_bn(wr.random_weights(17, seed=seed, dense_sizes=dense_sizes, activation=activation), x)


def _input(n, h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 255, size=(n, h, w, 2)).astype(np.float32)
    x[:, ::7, :, 1] = 0.0
    return x


def _block_errs(w, x, logits, taps):
    """-> (per-block err, head err) of one forward's taps (numpy float32) against the float64 oracle."""
    import cnn_oracle as co

    errs = []
    for k, got in enumerate(taps):
        assert np.isfinite(got).all(), NAMES[k]
        if k == 0:
            want, mag = co.first_block64(w, x)
        else:
            want, mag = co.block64(w, int(NAMES[k][0]), int(NAMES[k][2]), taps[k - 1].astype(np.float64))
        assert got.shape == want.shape, (NAMES[k], got.shape, want.shape)
        assert float(np.abs(want).max()) > 0.0, NAMES[k]  # (a block that is all zeros pins nothing)
        errs.append(float((np.abs(got.astype(np.float64) - want) / np.maximum(mag, 1e-30)).max()))
    want, mag = co.head64(w, taps[-1].astype(np.float64))
    herr = float((np.abs(logits.astype(np.float64) - want) / np.maximum(mag, 1e-30)).max())
    return errs, herr


def _report(case, mode, errs, herr, ovf=None):
    line = " ".join("%s %.2e%s" % (n, e, "*" if ovf is not None and ovf[k] else "") for k, (n, e) in enumerate(zip(NAMES, errs)))
    print("blocks %-28s %-7s %s | head %.2e%s" % (case, mode, line, herr, "  (* = rerun)" if ovf is not None and ovf.any() else ""))


def _run(net, engine, x):
    import torch

    logits, _, blocks, ovf = net.forward(torch.from_numpy(x).to(engine.device), taps=True)
    return logits.cpu().numpy(), [b.cpu().numpy() for b in blocks], ovf


def _assert_f32_accurate(case, mode, errs, herr):
    bad = [(n, e) for n, e in zip(NAMES, errs) if not e <= TOL]
    assert not bad, (case, mode, bad)
    assert herr <= TOL, (case, mode, "head", herr)


def test_taps_are_the_forward(engine):
    """The forward with taps computes what cpx_cnn_forward computes (same logits, bit for bit), its last tap is the head's
    input, and n_blocks other than 3 * blocks_per_stage is refused."""
    import torch

    from cpx.ml_tools import wrresnet as wr

    x = _input(2, 48, 48, 1)
    w = _model(2, x)
    net = wr.WRResNetDevice(engine, w, 17)
    xd = torch.from_numpy(x).to(engine.device)
    plain, _ = net.forward(xd)
    logits, _, blocks, ovf = net.forward(xd, taps=True)
    assert torch.equal(plain, logits)
    assert len(blocks) == 9 and ovf.shape == (9,) and not ovf.any()
    assert [tuple(b.shape) for b in blocks] == [(2, 48, 48, 64)] * 3 + [(2, 24, 24, 128)] * 3 + [(2, 8, 8, 256)] * 3
    assert all(bool(torch.isfinite(b).all()) for b in blocks)
    ptrs = (C.c_void_p * 9)(*[b.data_ptr() for b in blocks])
    lg = torch.empty_like(logits)
    for n in (8, 10, 0):
        rc = engine.lib.cpx_cnn_forward_taps(net._cnn, C.c_void_p(xd.data_ptr()), 2, 48, 48, C.c_void_p(lg.data_ptr()),
                                             None, ptrs, n, None)
        assert rc == -1 and "n_blocks" in engine._err(), (n, rc)  # CPX_ERR_INVALID
    net.close()


def test_every_math_mode_is_f32_accurate_per_block(engine):
    """All four math modes on the bench's map (160, stage-2 fs 32), N = 3: each block against float64."""
    from cpx.ml_tools import wrresnet as wr

    x = _input(3, 160, 160, 11)
    w = _model(3, x)
    errs, taps_of = {}, {}
    for mode in ("f32", "bf16x3", "bf16x2", "fp16x2"):
        engine.set_cnn_math(mode)
        net = wr.WRResNetDevice(engine, w, 17)
        logits, taps, ovf = _run(net, engine, x)
        net.close()
        taps_of[mode] = taps
        errs[mode], herr = _block_errs(w, x, logits, taps)
        _report("modes 3x160x160", mode, errs[mode], herr, ovf)
        assert herr <= TOL, (mode, herr)
        if mode == "fp16x2":
            assert not ovf.any(), ovf  # (inside the calibration range: these are the fp16 kernels' blocks)
    engine.set_cnn_math(engine.DEFAULT_CNN_MATH)
    for mode in ("f32", "bf16x3", "fp16x2"):
        _assert_f32_accurate("modes", mode, errs[mode], 0.0)
    for k, n in enumerate(NAMES):
        assert errs["fp16x2"][k] <= 2.0 * errs["bf16x3"][k] + 2.0 ** -24, (n, errs["fp16x2"][k], errs["bf16x3"][k])
        if n.endswith("b0"):  # (no residual in the accumulators: see the module docstring)
            assert errs["fp16x2"][k] <= 2.0 * errs["f32"][k] + 2.0 ** -24, (n, errs["fp16x2"][k], errs["f32"][k])
        assert errs["bf16x2"][k] <= 6 * 2.0 ** -16, (n, errs["bf16x2"][k])
        if n[0] in "23":  # (it IS the other arithmetic: see the module docstring)
            assert not np.array_equal(taps_of["bf16x2"][k], taps_of["bf16x3"][k]), n


@pytest.mark.parametrize("n,h,w", [(1, 320, 320), (2, 150, 150), (2, 37, 37), (2, 20, 20), (2, 96, 160), (1, 160, 160),
                                   (17, 160, 160)])
def test_fp16x2_blocks_over_shapes_and_batches(engine, n, h, w):
    """The default mode on fs 64 (320), ragged tiles (150 = 9 x 16 + 6), 37, a map smaller than a tile at stage 4 (20),
    a non-square map, and N = 1 / 17 at 160 (17 samples: 1700 stage-2 tiles, thirteen rounds of the persistent grid and a
    ragged last one)."""
    from cpx.ml_tools import wrresnet as wr

    x = _input(n, h, w, 100 + h + w + n)
    wt = _model(4, x[:4])
    engine.set_cnn_math("fp16x2")
    net = wr.WRResNetDevice(engine, wt, 17)
    logits, taps, ovf = _run(net, engine, x)
    net.close()
    errs, herr = _block_errs(wt, x, logits, taps)
    _report("shape %dx%dx%d" % (n, h, w), "fp16x2", errs, herr, ovf)
    _assert_f32_accurate((n, h, w), "fp16x2", errs, herr)


@pytest.mark.parametrize("scale", [1e-3, 1.0, 30.0, 60.0, 1000.0, "smooth"])
def test_fp16x2_blocks_over_input_ranges(engine, scale):
    """The calibration range scaled by 1e-3 ... 1000 and a smooth (8x upsampled) input: whichever blocks stay on the fp16
    kernels and whichever are rerun on the guarded bf16x3 launches, every block is float32-accurate.  The per-block
    overflow words say which ran how.  At 30 every block stays on fp16, 3b1's scaled input right at fp16's largest value
    (the float64 activations over the fp16 limit: 0.15 .. 1.0).  At 60 the forward interleaves the two: 2b0, 3b2, 4b0
    and 4b2 stay below the limit (0.3 .. 0.9 of it), 2b1, 2b2, 3b1 and 4b1 exceed it (1.4 .. 2.0), so fp16 blocks
    read a rerun block's output and the other way round.  At 1000 every block reruns (5 .. 33)."""
    from cpx.ml_tools import wrresnet as wr

    x = _input(2, 160, 160, 515)
    w = _model(21, x)
    if scale == "smooth":
        rng = np.random.default_rng(42)
        xs = np.repeat(np.repeat(rng.uniform(0, 255, size=(2, 20, 20, 2)).astype(np.float32), 8, axis=1), 8, axis=2)
    else:
        xs = x * np.float32(scale)
    engine.set_cnn_math("fp16x2")
    net = wr.WRResNetDevice(engine, w, 17)
    logits, taps, ovf = _run(net, engine, np.ascontiguousarray(xs))
    net.close()
    engine.set_cnn_math(engine.DEFAULT_CNN_MATH)
    errs, herr = _block_errs(w, xs, logits, taps)
    _report("range %s" % scale, "fp16x2", errs, herr, ovf)
    print("overflow words", ovf.tolist())
    assert (engine.cnn_last_overflow()) == bool(ovf.any())
    if scale == 60.0:
        assert ovf.any() and not ovf.all(), ovf
        assert not ovf[0] and ovf[1] and ovf[2] and ovf[4] and not ovf[5] and not ovf[6] and ovf[7] and not ovf[8], ovf
    if scale == 1000.0:
        assert ovf.any(), ovf
    _assert_f32_accurate("range %s" % scale, "fp16x2", errs, herr)


# (environment, value, launch counts the form must show: conv_timing keys, 80324 / 320324 = a fused first / later stage-2
# block, 320321 = a stage-2 convolution on its own, 10081 = conv1_1 on its own)
FORMS = [
    ("CPX_CNN_BLOCK_FUSION", "0", {320324: None, 80324: None, 320321: 5}),
    ("CPX_CNN_BLOCK_FUSION", "1", {320324: 2, 80324: None, 320321: 1}),
    ("CPX_CNN_FUSE_SHORTCUT", "0", {80324: None}),
    ("CPX_CNN_FUSE_CONV1", "0", {10081: 1, 80324: 1, 320324: 2}),
]


def _check_launches(launches, want):
    for key, count in want.items():
        if count is None:
            assert key not in launches, (key, launches)
        else:
            assert launches[key][0] == count, (key, launches)


@pytest.mark.parametrize("env,value,want", FORMS)
def test_fp16x2_forms_are_f32_accurate_per_block(monkeypatch, env, value, want):
    """Each fusion form passes the float64 criterion on its own, not only against another form: unfused blocks, only the
    later stage-2 blocks fused, the 1x1 shortcut as a launch of its own, conv1_1 outside the first block.  The switches
    are read when a handle is created.  Ragged tiles (150)."""
    from cpx.engine import TrackEngine
    from cpx.ml_tools import wrresnet as wr

    x = _input(2, 150, 150, 77)
    w = _model(8, x)
    monkeypatch.setenv(env, value)
    eng = TrackEngine(model="lepton3")
    monkeypatch.delenv(env)
    try:
        eng.set_cnn_math("fp16x2")
        net = wr.WRResNetDevice(eng, w, 17)
        eng.conv_timing(True)
        logits, taps, ovf = _run(net, eng, x)
        launches = eng.conv_timing()
        eng.conv_timing(False)
        net.close()
    finally:
        eng.close()
    _check_launches(launches, want)
    assert not ovf.any(), ovf
    errs, herr = _block_errs(w, x, logits, taps)
    _report("form %s=%s" % (env, value), "fp16x2", errs, herr, ovf)
    _assert_f32_accurate((env, value), "fp16x2", errs, herr)


def _launch_table(eng, mode):
    """One forward with taps of the 17-label random model on 2 x 48 x 48 x 2 -> {key: (launches, flops)}, the complete
    conv_timing table of that forward."""
    from cpx.ml_tools import wrresnet as wr

    x = _input(2, 48, 48, 1)
    w = _model(2, x)
    eng.set_cnn_math(mode)
    net = wr.WRResNetDevice(eng, w, 17)
    eng.conv_timing(True)
    _run(net, eng, x)
    table = eng.conv_timing()
    eng.conv_timing(False)
    net.close()
    return {key: (launches, flops) for key, (launches, _, flops) in table.items()}


# The complete conv_timing table of one forward, {key: (launches, FLOPs)}, per (math mode, fusion form); recorded on an
# MI355X from the build BEFORE the forward was split into a plan and an executor, so it pins the dispatch that build
# had.  Keys: (Cin / groups) * 10000 + (Cout / groups) * 10 + stride (+ 5 for a 1x1 layer); "stride 4" = a fused block.
# The FLOP totals are exact doubles the host computes from the shapes (2 N Ho Wo Cout Cin/groups k^2 per launch).
LAUNCH_TABLES = {
    'f32': {10081: (1, 1327104.0), 80321: (1, 42467328.0), 80326: (1, 4718592.0), 320321: (5, 849346560.0),
        320642: (1, 84934656.0), 320647: (1, 9437184.0), 640641: (5, 849346560.0), 641283: (1, 37748736.0),
        641288: (1, 4194304.0), 1281281: (5, 377487360.0)},
    'bf16x3': {10081: (1, 1327104.0), 80321: (1, 42467328.0), 320321: (5, 849346560.0), 320642: (1, 84934656.0),
        640641: (5, 849346560.0), 641283: (1, 37748736.0), 1281281: (5, 377487360.0)},
    'bf16x2': {10081: (1, 1327104.0), 80321: (1, 42467328.0), 320321: (5, 849346560.0), 320642: (1, 84934656.0),
        640641: (5, 849346560.0), 641283: (1, 37748736.0), 1281281: (5, 377487360.0)},
    'fp16x2': {80324: (1, 213663744.0), 320324: (2, 679477248.0), 320642: (1, 84934656.0),
        640641: (5, 849346560.0), 641283: (1, 37748736.0), 1281281: (5, 377487360.0)},
    'fp16x2 CPX_CNN_BLOCK_FUSION=0': {10081: (1, 1327104.0), 80321: (1, 42467328.0), 320321: (5, 849346560.0),
        320642: (1, 84934656.0), 640641: (5, 849346560.0), 641283: (1, 37748736.0), 1281281: (5, 377487360.0)},
    'fp16x2 CPX_CNN_BLOCK_FUSION=1': {10081: (1, 1327104.0), 80321: (1, 42467328.0), 320321: (1, 169869312.0),
        320324: (2, 679477248.0), 320642: (1, 84934656.0), 640641: (5, 849346560.0), 641283: (1, 37748736.0),
        1281281: (5, 377487360.0)},
    'fp16x2 CPX_CNN_FUSE_SHORTCUT=0': {10081: (1, 1327104.0), 80321: (1, 42467328.0), 80326: (1, 4718592.0),
        320321: (1, 169869312.0), 320324: (2, 679477248.0), 320642: (1, 84934656.0), 320647: (1, 9437184.0),
        640641: (5, 849346560.0), 641283: (1, 37748736.0), 641288: (1, 4194304.0), 1281281: (5, 377487360.0)},
    'fp16x2 CPX_CNN_FUSE_CONV1=0': {10081: (1, 1327104.0), 80324: (1, 212336640.0), 320324: (2, 679477248.0),
        320642: (1, 84934656.0), 640641: (5, 849346560.0), 641283: (1, 37748736.0), 1281281: (5, 377487360.0)},
}


@pytest.mark.parametrize("case", ["f32", "bf16x3", "bf16x2", "fp16x2"] + ["fp16x2 %s=%s" % (e, v) for e, v, _ in FORMS])
def test_forward_launch_table(engine, monkeypatch, case):
    """Which launches a forward is made of: every conv_timing key, its launch count and its FLOP total, and no key
    beyond them, for each math mode on a default handle and for fp16x2 under each switch of FORMS (a fresh engine
    created under the switch).  2 x 48 x 48: stage 2 at 48 x 48 takes the fused first block with conv1_1 inside and
    the two later fused blocks, stage 3 runs at 24 x 24, stage 4 at 8 x 8 (the strided layers, the plane hand-off and
    the flattened stage-4 route)."""
    from cpx.engine import TrackEngine

    mode, _, form = case.partition(" ")
    if not form:
        got = _launch_table(engine, mode)
        engine.set_cnn_math(engine.DEFAULT_CNN_MATH)
    else:
        env, value = form.split("=")
        assert (env, value) in [(e, v) for e, v, _ in FORMS]
        monkeypatch.setenv(env, value)
        eng = TrackEngine(model="lepton3")
        monkeypatch.delenv(env)
        try:
            got = _launch_table(eng, mode)
        finally:
            eng.close()
    print("launch table %-36s %r" % (case, got))
    assert got == LAUNCH_TABLES[case], (case, got)


def test_fp16x2_unsplit_block_kernel_is_f32_accurate_per_block():
    """CPX_BLOCK32_SPLIT=0 (conv_block32_kernel instead of the split-role conv_block32s_kernel) is read once per process:
    this form runs in a child."""
    x = _input(2, 150, 150, 77)
    w = _model(8, x)
    logits, taps, ovf, launches = _taps_in_child(w, x, {"CPX_BLOCK32_SPLIT": "0"})
    _check_launches(launches, {80324: 1, 320324: 2, 320321: None})
    assert not ovf.any(), ovf
    errs, herr = _block_errs(w, x, logits, taps)
    _report("form CPX_BLOCK32_SPLIT=0", "fp16x2", errs, herr, ovf)
    _assert_f32_accurate("CPX_BLOCK32_SPLIT=0", "fp16x2", errs, herr)


def _taps_in_child(w, x, env_set):
    """One fp16x2 forward with taps in a fresh process with the environment env_set -> (logits, taps, overflow, launches)."""
    import pickle
    import subprocess
    import sys
    import tempfile

    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "in.pkl"), "wb") as fh:
            pickle.dump((w, x), fh)
        code = (
            "import sys, pickle, torch\n"
            "sys.path.insert(0, %r)\n"
            "from cpx.engine import TrackEngine\n"
            "from cpx.ml_tools import wrresnet as wr\n"
            "w, x = pickle.load(open(%r, 'rb'))\n"
            "eng = TrackEngine(model='lepton3'); eng.set_cnn_math('fp16x2')\n"
            "net = wr.WRResNetDevice(eng, w, 17)\n"
            "eng.conv_timing(True)\n"
            "logits, _, blocks, ovf = net.forward(torch.from_numpy(x).to(eng.device), taps=True)\n"
            "launches = eng.conv_timing()\n"
            "pickle.dump((logits.cpu().numpy(), [b.cpu().numpy() for b in blocks], ovf, launches), open(%r, 'wb'))\n"
            "net.close(); eng.close()\n"
            % (os.path.join(REPO, "classifier-pipeline_amd"), os.path.join(td, "in.pkl"), os.path.join(td, "out.pkl")))
        env = dict(os.environ, **env_set)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        with open(os.path.join(td, "out.pkl"), "rb") as fh:
            return pickle.load(fh)


@pytest.mark.parametrize("model", ["tflite", "hidden_softmax"])
def test_fp16x2_blocks_of_other_models(engine, tmp_path, model):
    """A .tflite model (BatchNorms folded, activation bounds measured on a probe batch rather than taken from BatchNorm
    statistics: WRResNetDevice._measure_activation_bounds), on noise and on a smooth input; and a head with hidden Dense
    layers and softmax."""
    from cpx.ml_tools import wrresnet as wr
    from cpx.ml_tools.tflite_reader import load_tflite
    from test_tflite_import_cpu import tflite_of

    x = _input(3, 160, 160, 41)
    if model == "tflite":
        w0 = _model(8, x)
        p = tmp_path / "m.tflite"
        p.write_bytes(tflite_of(w0, ()))
        w = load_tflite(p)
    else:
        w = _model(5, x[:2], dense_sizes=(48, 24), activation="softmax")
    rng = np.random.default_rng(43)
    smooth = np.repeat(np.repeat(rng.uniform(0, 255, size=(2, 20, 20, 2)).astype(np.float32), 8, axis=1), 8, axis=2)
    engine.set_cnn_math("fp16x2")
    net = wr.WRResNetDevice(engine, w, 17)
    if model == "tflite":
        assert all(b > 0 for b in net.act_bounds)
    for name, xi in (("noise", x), ("smooth", np.ascontiguousarray(smooth))):
        logits, taps, ovf = _run(net, engine, xi)
        errs, herr = _block_errs(w, xi, logits, taps)
        _report("%s %s" % (model, name), "fp16x2", errs, herr, ovf)
        _assert_f32_accurate((model, name), "fp16x2", errs, herr)
    net.close()
    engine.set_cnn_math(engine.DEFAULT_CNN_MATH)
