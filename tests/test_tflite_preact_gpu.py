"""The ResNet / VGG / DenseNet families in the TFLite graph executor on the GPU: the INPUT operator ('caffe' / 'torch' input
modes) against the NumPy statement of keras.applications' preprocess_input, bit for bit; CONV_PRE (the pre-activation folded
into the convolution that reads it) against the AFFINE and CONV launches it replaces, bit for bit, and against float64; a
DenseNet-style and a ResNetV2-style network (tests/tflite_build_preact.py) through LiteInterpreter; ClipClassifier on the
possum fixture with a `resnet`-named model.  The flatbuffers are synthetic and the evaluator reads the Graph only
(tests/tflite_eval.py).  Parity with TensorFlow's own preprocess_input and with the TFLite runtime (ai_edge_litert) on
these families is not pinned here: neither is installed (test_tflite_graph_gpu.py::test_released_model_parity is the route
where the runtime exists)."""
import json
import os
import shutil
from fractions import Fraction

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_preact as tp
import tflite_eval as te
from test_tflite_graph_gpu import CONV_REL, LABELS17, LOGIT_MULTIPLE

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def run(engine, blob, x, output=None, fuse=False, channel_map=None, input_mode=None, out_slice=None, out=None):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    shape = x.shape[1:] if channel_map is None else (x.shape[1], x.shape[2], len(channel_map))
    plan = build_plan(g, input_shape=shape, output=output, channel_map=channel_map, input_mode=input_mode, fuse_preactivation=fuse)
    dev = GraphDevice(engine, plan, out_slice=out_slice)
    got = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device), out=out).cpu().numpy()
    dev.close()
    return g, plan, got


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- 1. INPUT ----
# 128 / 255 = 0.50196...: its quotient lies 1 / 510 of an ulp from the middle between two float32 values.  No float32 divided by
# 255 is an exact tie (255 is odd, the tie's numerator would need 25 significant bits), and 1 / 510 is the nearest any comes
NEAR_TIE = 128.0


def input_sample():
    q = Fraction(NEAR_TIE) / 255 * 2 ** 24   # the quotient in units of its float32 ulp (0.5 <= 128 / 255 < 1)
    assert abs(q - q.numerator // q.denominator - Fraction(1, 2)) == Fraction(1, 510)
    rng = np.random.default_rng(21)
    x = rng.uniform(0, 255, size=(2, 5, 7, 2)).astype(F32)
    special = np.array([0.0, 255.0, -1.0, -254.99, 1e-30, NEAR_TIE, -0.0, 103.939, 123.68, 0.485 * 255, 1.0, 254.0], F32)
    x[0, 0, :6, 0], x[0, 0, :6, 1] = special[:6], special[6:]
    x[1, 4, :6, 1], x[1, 4, :6, 0] = special[:6], special[6:]
    return x


@pytest.mark.parametrize("cmap", [[0, 0, 1], [1, 0, 0], [1, 1, 1]], ids=lambda m: "map%d%d%d" % tuple(m))
@pytest.mark.parametrize("mode", ["caffe", "torch"])
def test_input_operator_equals_the_numpy_statement(engine, mode, cmap):
    """out[c] = ((in0[map[c]] / param) - shift[c]) / scale[c], one correctly rounded float32 operation each: NumPy's.  The
    device's division is checked here -- an approximate reciprocal would miss NEAR_TIE and most of the random values."""
    from cpx import _lib
    from cpx.ml_tools.tflite_graph import INPUT_MODES

    x = input_sample()
    blob = tp.densenet(6)   # any graph of three input channels: the forward is cut off behind the INPUT operator
    from cpx.ml_tools.tflite_reader import Graph

    g, plan, got = run(engine, blob, x, output=Graph(blob).inputs[0], channel_map=cmap, input_mode=mode)
    assert [o.kind for o in plan.ops] == [_lib.GRAPH_INPUT] and got.shape == (2, 5, 7, 3)
    param, shift, scale, _ = INPUT_MODES[mode]
    want = x[..., cmap] / F32(param)
    want = want - shift
    if scale is not None:
        want = want / scale
    assert want.dtype == np.float32
    print("%s %s: %d of %d elements differ" % (mode, cmap, int((bits(got) != bits(want)).sum()), got.size))
    assert np.array_equal(bits(got), bits(want))
    # ... which is the host function of the mode on the mapped sample (caffe_preprocess reverses the channels itself)
    from cpx.ml_tools.interpreter import caffe_preprocess, torch_preprocess

    host = caffe_preprocess(np.ascontiguousarray(x[..., cmap[::-1]])) if mode == "caffe" else torch_preprocess(np.ascontiguousarray(x[..., cmap]))
    assert np.array_equal(bits(host), bits(want))


# ---- 2. CONV_PRE against the two launches and against float64 ----
PRE_CASES = {
    # k, stride, padding, cin, cout, size, N, activation, keyword arguments
    "1x1_40to24": (1, 1, tb.SAME, 40, 24, 9, 2, tb.RELU, {}),                    # Cin no multiple of 16, Cout < 32
    "3x3_same_positive_shift": (3, 1, tb.SAME, 16, 24, 9, 2, tb.RELU, {"shift": "positive"}),
    "3x3_s2_valid": (3, 2, tb.VALID, 32, 48, 11, 2, tb.RELU, {}),
    "cin3_scalar_loads": (3, 1, tb.SAME, 3, 32, 9, 2, tb.RELU, {}),
    "relu6": (3, 1, tb.SAME, 16, 32, 9, 2, tb.RELU6, {}),
    "slice_8to24_of_40": (3, 1, tb.SAME, 16, 24, 9, 2, tb.RELU, {"c_total": 40, "c_from": 8}),
    "three_samples_of_7x7": (1, 1, tb.SAME, 16, 32, 7, 3, tb.RELU, {}),        # 147 pixels: 128 + 19
    "cout96": (1, 1, tb.SAME, 16, 96, 9, 2, tb.RELU, {}),                        # several column blocks
}


def conv64(p, w_ohwi, bias, stride, padding):
    """float64 CONV_2D of the NHWC array p with tests/tflite_eval.py's padding -> (values, sum |p| |w| + |b|)."""
    import torch
    import torch.nn.functional as F

    t = torch.as_tensor(np.asarray(p, np.float64)).permute(0, 3, 1, 2)
    w = torch.as_tensor(np.asarray(w_ohwi, np.float64)).permute(0, 3, 1, 2)
    b = None if bias is None else torch.as_tensor(np.asarray(bias, np.float64))
    pt, pb = te._pads(t.shape[2], w.shape[2], stride, padding)
    pl, pr = te._pads(t.shape[3], w.shape[3], stride, padding)
    t = F.pad(t, (pl, pr, pt, pb))
    y = F.conv2d(t, w, b, stride=stride)
    m = F.conv2d(t.abs(), w.abs(), None if b is None else b.abs(), stride=stride)
    return y.permute(0, 2, 3, 1).numpy(), m.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("name", sorted(PRE_CASES))
def test_conv_pre_equals_the_two_launches_and_float64(engine, name):
    """Bit for bit: the prologue is graph_affine_kernel's two float32 operations and activate(), and the build has
    -ffp-contract=off.  Against float64: CONV_REL of sum |act(x s + h)| |w| (+ |b|), the bound of test_tflite_graph_gpu.py;
    the pre-activation's own two roundings move act(..) by at most 2 x 2^-24 = 1.2e-7 of |x s| + |h|, a thirtieth of that
    bound where nothing cancels in x s + h."""
    import torch

    from cpx import _lib

    k, stride, padding, cin, cout, size, n, act, kw = PRE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    kw = dict(kw)
    if kw.get("shift") == "positive":
        kw["shift"] = rng.uniform(0.5, 1.5, size=cin).astype(F32)
    blob, p_t, y_t = tp.preact_conv(rng, k, stride, padding, cin, cout, size, act=act, **kw)
    cx = kw.get("c_total", cin)
    x = (rng.normal(0, 6.0 if act == tb.RELU6 else 1.0, size=(n, size, size, cx))).astype(F32)
    g, plain, unfused = run(engine, blob, x)
    _, plan, fused = run(engine, blob, x, fuse=True)
    assert len(plan.ops) == len(plain.ops) - 1 and plan.ops[-1].kind == _lib.GRAPH_CONV_PRE and plain.ops[-2].kind == _lib.GRAPH_AFFINE
    assert plain.ops[-1].kind == _lib.GRAPH_CONV and plan.ops[-1].param == float(act)
    n_diff = int((bits(fused) != bits(unfused)).sum())
    print("%s: %d of %d outputs differ between fused and unfused" % (name, n_diff, fused.size))
    assert fused.shape == unfused.shape and n_diff == 0
    assert float(np.abs(fused).max()) > 0.1 and np.all(np.isfinite(fused))

    if "c_total" in kw:
        # the pre-activation reads a slice of what three device convolutions wrote: float64 from the device's own slice
        src = plain.ops[-2].in0
        assert (plain.tensors[src].c_offset, plain.tensors[src].c_stride) == (kw["c_from"], cx) == \
            (plan.tensors[plan.ops[-1].in0].c_offset, plan.tensors[plan.ops[-1].in0].c_stride)
        mul, add, conv = g.ops[-3:]
        s = run(engine, blob, x, output=src)[2].astype(np.float64)
        pre = np.maximum(s * g.const(mul["inputs"][1]).astype(np.float64) + g.const(add["inputs"][1]).astype(np.float64), 0.0)
        want, mag = conv64(pre, g.const(conv["inputs"][1]), g.const(conv["inputs"][2]), stride, padding)
        # ... and the fused convolution writes into a channel slice of the caller's rows without touching the rest
        sentinel = F32(-12345.678)
        oh = fused.shape[1]
        out = torch.full((n, oh, oh, 5 + cout + 3), float(sentinel), dtype=torch.float32, device=engine.device)
        _, _, sliced = run(engine, blob, x, fuse=True, out_slice=(5, 5 + cout + 3), out=out)
        assert np.array_equal(bits(sliced[..., 5:5 + cout]), bits(fused))
        assert np.all(sliced[..., :5] == sentinel) and np.all(sliced[..., 5 + cout:] == sentinel)
    else:
        vals, mags = te.evaluate(g, x, magnitudes=True)
        want, mag = vals[y_t], mags[y_t]
        if act == tb.RELU6:
            assert float((vals[p_t] == 6.0).mean()) > 0.05 and float((vals[p_t] == 0.0).mean()) > 0.05   # both clamps at work
    rel = float((np.abs(fused - want) / mag).max())
    print("%s: max |error| / sum |act(x s + h)| |w| = %.3g (bound %.3g)" % (name, rel, CONV_REL))
    assert rel < CONV_REL

    if kw.get("shift") is not None and "c_total" not in kw:
        # a padded tap must contribute 0, not relu(shift) > 0: the border is where that would show
        border = np.ones(fused.shape[1:3], bool)
        border[1:-1, 1:-1] = False
        assert np.array_equal(bits(fused[:, border]), bits(unfused[:, border]))
        # (what the test would see of a mask applied before the prologue: relu(shift) in the padding, in float64)
        padded = np.broadcast_to(np.maximum(kw["shift"], 0).astype(np.float64), (n, size + 2, size + 2, cin)).copy()
        padded[:, 1:-1, 1:-1] = vals[p_t]
        conv = g.ops[-1]
        wrong = conv64(padded, g.const(conv["inputs"][1]), g.const(conv["inputs"][2]), 1, tb.VALID)[0]
        assert float((np.abs(wrong - want) / mag)[:, border].max()) > 1000 * CONV_REL
        assert float((np.abs(fused - want) / mag)[:, border].max()) < CONV_REL


def test_conv_pre_batch_does_not_matter(engine):
    k, stride, padding, cin, cout, size, _, act, kw = PRE_CASES["three_samples_of_7x7"]
    rng = np.random.default_rng(3)
    blob, _, _ = tp.preact_conv(rng, k, stride, padding, cin, cout, size, act=act)
    x = rng.normal(size=(1, size, size, cin)).astype(F32)
    _, _, one = run(engine, blob, x, fuse=True)
    _, _, five = run(engine, blob, np.repeat(x, 5, axis=0), fuse=True)
    assert all(np.array_equal(bits(five[i]), bits(one[0])) for i in range(5)) and float(np.abs(one).max()) > 0.1


# ---- 3. whole networks through LiteInterpreter ----
def raw_samples(n, size, seed):
    """Seeded 0..255 two-channel samples that differ in structure: what the crop kernel hands these families, unscaled."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
    out = []
    for s in range(n):
        planes = [127.5 + 110 * np.sin(2 * np.pi * ((s + 1) * xx * (c + 1) + (2 * s + 1) * yy + 0.3 * c)) for c in range(2)]
        out.append(np.clip(np.stack(planes, axis=-1) + rng.normal(0, 10, size=(size, size, 2)), 0, 255))
    return np.stack(out).astype(F32)


def write_model(d, name, model_name, blob):
    (d / (name + ".tflite")).write_bytes(blob)
    with open(d / (name + ".json"), "w") as fh:
        json.dump({"labels": LABELS17, "type": "thermal", "version": "test",
                   "hyperparams": {"frame_size": 32, "model_name": model_name, "channels": ["thermal", "thermal", "filtered"]}}, fh)
    return d / (name + ".tflite")


# model_name -> (builder, host preprocess name).  Seed 7 was chosen on the CPU: the float64 logits spread by 6.2 (densenet) and
# 2.7 (resnet) against tolerances of about 1e-5
NETWORKS = {
    "densenet121": (lambda: tp.densenet(17, blocks=(3, 3), growth=8, seed=7), "torch_preprocess"),
    "resnet": (lambda: tp.resnet_v2(17, seed=7, stem_gain=1.0 / 64), "caffe_preprocess"),
}


@pytest.mark.parametrize("model_name", sorted(NETWORKS))
def test_whole_network_through_the_lite_interpreter(engine, tmp_path, monkeypatch, model_name):
    """The method of test_tflite_graph_gpu.py::test_inception_v3_whole_network: the device may
    deviate from the float64 evaluation of the flatbuffer -- on the input NumPy preprocessed -- by LOGIT_MULTIPLE times
    what a float32 evaluation on the CPU does.  Measured on an MI355X: densenet121 1.92e-6 on the CPU, 1.63e-6 on the
    device (ratio 0.85), logits spread 6.2; resnet 1.11e-6 and 1.76e-6 (ratio 1.59), spread 2.7; fused and unfused equal."""
    import torch

    from cpx import _lib
    from cpx.ml_tools import interpreter as ci
    from cpx.ml_tools.tflite_reader import Graph

    builder, host_fn = NETWORKS[model_name]
    blob = builder()
    path = write_model(tmp_path, "m", model_name, blob)
    g = Graph(blob)
    logits_t = g.ops[-1]["inputs"][0]
    x2 = raw_samples(3, 32, seed=11)
    xd = torch.from_numpy(x2).to(engine.device)
    probs, plans = {}, {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT", fuse)
        interp = ci.LiteInterpreter(path, engine=engine)
        probs[fuse] = interp.predict(xd)
        plans[fuse] = interp._plan((32, 32, 2))[1]
        assert plans[fuse].ops[0].kind == _lib.GRAPH_INPUT and not interp.limits_flags() & _lib.LIMITS_TF_SCALING
    n_pre = sum(o.kind == _lib.GRAPH_CONV_PRE for o in plans["1"].ops)
    assert n_pre == (7 if model_name == "densenet121" else 3) and not any(o.kind == _lib.GRAPH_CONV_PRE for o in plans["0"].ops)
    assert len(plans["0"].ops) - len(plans["1"].ops) == (7 if model_name == "densenet121" else 2)
    assert probs["1"].shape == (3, 17) and np.array_equal(bits(probs["1"]), bits(probs["0"]))
    # the logits, by the interpreter's own channel map and mode
    cmap, mode = interp.channel_map(), interp.input_mode
    logits = {f: run(engine, blob, x2, output=logits_t, fuse=f, channel_map=cmap, input_mode=mode)[2] for f in (True, False)}
    assert np.array_equal(bits(logits[True]), bits(logits[False]))
    x3 = np.ascontiguousarray(getattr(ci, host_fn)(np.ascontiguousarray(x2[..., [0, 0, 1]])))
    v64 = te.evaluate(g, x3)
    v32 = te.evaluate(g, x3, dtype=torch.float32)
    yard = float(np.abs(v32[logits_t] - v64[logits_t]).max())
    tol = LOGIT_MULTIPLE * yard
    err = float(np.abs(logits[True] - v64[logits_t]).max())
    spread = min(float(np.ptp(v64[logits_t], axis=1).min()), float(np.ptp(v64[logits_t], axis=0).max()))
    print("%s: float32-CPU vs float64: %.3g; device vs float64: %.3g (ratio %.2f); spread of the logits %.3g; %d launches fused, %d unfused"
          % (model_name, yard, err, err / yard, spread, len(plans["1"].ops), len(plans["0"].ops)))
    assert spread >= 100 * tol, (spread, tol)
    assert err <= tol, (err, yard)
    assert float(np.abs(probs["1"] - v64[g.outputs[0]]).max()) <= 1e-3


# ---- 4. one file end to end ----
def test_clip_classifier_with_a_resnet_named_model(tmp_path, monkeypatch, engine):
    """test_tflite_dw_gpu.py::test_clip_classifier_with_a_mobilenet with a `resnet`-named ('caffe') model: the possum
    fixture tracked, then classified by ClipClassifier's one-file path.  The crop kernel hands the network the unscaled
    sample (the oracle chain's, at the 1e-5 x 127.5 that test holds the scaled one to); what the graph's INPUT operator makes
    of it is caffe_preprocess of the channel-mapped sample, bit for bit; the predictions are the float64 evaluator's on that
    at 1e-3."""
    import classify_oracle as co
    from helpers import GOLDEN
    from cpx import _lib
    from cpx.classify.clipclassifier import ClipClassifier
    from cpx.config import Config
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, caffe_preprocess, get_interpreter
    from cpx.ml_tools.tflite_reader import Graph
    from cpx.track.trackextractor import extract_file

    monkeypatch.delenv("CPX_TFLITE_FUSE_PREACT", raising=False)
    blob = tp.resnet_v2(17, size=160, seed=13, stem_gain=1.0 / 64)
    write_model(tmp_path, "rn", "resnet", blob)
    g = Graph(blob)
    cfg = Config.get_defaults()
    cfg.tracking["thermal"].denoise = False
    cfg.classify.models = [ModelConfig.load({"id": 9, "name": "rn", "model_file": str(tmp_path / "rn.tflite")})]
    src = tmp_path / "possum.cptv"
    shutil.copy(os.path.join(GOLDEN, "possum.cptv"), src)
    clip, _, _ = extract_file(src, cfg, False, save_meta=False)

    interp = get_interpreter(cfg.classify.models[0])
    assert isinstance(interp, LiteInterpreter) and interp.input_mode == "caffe" and interp.channel_map() == [1, 0, 0]
    assert not interp.limits_flags() & _lib.LIMITS_TF_SCALING
    plan = interp._plan((160, 160, 2))[1]
    assert plan.ops[0].kind == _lib.GRAPH_INPUT and sum(o.kind == _lib.GRAPH_CONV_PRE for o in plan.ops) == 3

    fed, answered = [], []
    plain_predict = LiteInterpreter.predict

    def recording_predict(self, x):
        out = plain_predict(self, x)
        fed.extend(x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x))
        answered.extend(np.asarray(out, np.float64))
        return out

    monkeypatch.setattr(LiteInterpreter, "predict", recording_predict)
    meta = ClipClassifier(cfg).process_file(str(src), track=True)
    monkeypatch.setattr(LiteInterpreter, "predict", plain_predict)
    assert meta and os.path.exists(src.with_suffix(".txt")) and meta["models"][0]["id"] == 9
    H, W = clip.res_y, clip.res_x
    assert len(meta["tracks"]) == len(clip.tracks) > 0
    for tm, track in zip(meta["tracks"], clip.tracks):
        assert tm["id"] == track.get_id()
        (pm,) = tm["predictions"]
        assert pm["model_id"] == 9 and set(pm["all_class_confidences"]) == set(LABELS17) and len(pm["predictions"]) > 0
        segs = [np.array(p["frames"]) for p in pm["predictions"]]
        by_frame = {r.frame_number: r for r in track.bounds_history}
        x, _ = co.preprocess_segments(lambda q: clip.frame_buffer.get_frame(q).thermal,
                                      lambda q: clip.frame_buffer.get_frame(q).filtered.astype(np.float64),
                                      by_frame, track.bounds_history, segs, 32, (1, 1, W - 2, H - 2))
        x = np.asarray(x, F32)
        x_fed, fed = np.stack(fed[:len(segs)]), fed[len(segs):]
        probs, answered = np.stack(answered[:len(segs)]), answered[len(segs):]
        dx = float(np.abs(x_fed - x).max())
        print("track %d: the unscaled sample vs the oracle chain's: %.3g (values up to %.4g)" % (tm["id"], dx, float(x_fed.max())))
        assert x_fed.shape == x.shape == (len(segs), 160, 160, 2) and dx <= 1e-5 * 127.5 and float(x_fed.max()) > 50.0
        # what the network itself received: the INPUT operator's output
        want3 = np.ascontiguousarray(caffe_preprocess(np.ascontiguousarray(x_fed[..., [0, 0, 1]])))
        got3 = run(engine, blob, x_fed, output=g.inputs[0], channel_map=interp.channel_map(), input_mode=interp.input_mode)[2]
        assert np.array_equal(bits(got3), bits(want3))
        want_probs = te.evaluate(g, want3)[g.outputs[0]]
        dev = float(np.abs(probs - want_probs).max())
        print("track %d: the one-file path's probabilities vs the evaluator's on its inputs: %.3g" % (tm["id"], dev))
        assert dev <= 1e-3
        score = co.classified_track(probs, prediction_frames=segs, labels=LABELS17)
        got = np.array([pm["all_class_confidences"][l] for l in LABELS17])
        assert np.abs(got - np.round(score, 3)).max() <= 1e-3 + 1e-9
        assert pm["tag"] == LABELS17[int(np.argmax(score))]
    assert not fed and not answered
