"""The 'caffe' / 'torch' input modes and the folded pre-activation through the planner and LiteInterpreter: host work, no
GPU.  The flatbuffers come from tests/tflite_build_preact.py.  keras.applications' own preprocess_input is not installed
here: the yardstick is a literal NumPy transcription of keras.applications.imagenet_utils._preprocess_numpy_input, below."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_dw as td
import tflite_build_preact as tp

from cpx import _lib
from cpx.ml_tools import tflite_graph as tg
from cpx.ml_tools.tflite_graph import build_plan
from cpx.ml_tools.tflite_reader import Graph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CAFFE, TORCH = ("resnet", "resnet152", "vgg16", "vgg19"), ("densenet121",)


def keras_preprocess_numpy_input(x, mode):
    """keras/src/applications/imagenet_utils.py: _preprocess_numpy_input(x, data_format='channels_last', mode), the
    branches for 'caffe' and 'torch' on a float32 array, line by line."""
    assert x.dtype == np.float32
    if mode == "torch":
        x /= 255.0
        mean = [0.485, 0.456, 0.406]
        std = [0.229, 0.224, 0.225]
    else:
        # 'RGB'->'BGR'
        x = x[..., ::-1]
        mean = [103.939, 116.779, 123.68]
        std = None
    x[..., 0] -= mean[0]
    x[..., 1] -= mean[1]
    x[..., 2] -= mean[2]
    if std is not None:
        x[..., 0] /= std[0]
        x[..., 1] /= std[1]
        x[..., 2] /= std[2]
    return x


@pytest.mark.parametrize("mode", ["caffe", "torch"])
def test_host_preprocess_equals_the_keras_transcription(mode):
    from cpx.ml_tools.interpreter import caffe_preprocess, torch_preprocess

    rng = np.random.default_rng(3)
    x = rng.uniform(0, 255, size=(4, 9, 7, 3)).astype(F32)
    x[0, 0, 0] = [0.0, 255.0, 127.5]
    want = keras_preprocess_numpy_input(x.copy(), mode)
    mine = x.copy()
    got = (caffe_preprocess if mode == "caffe" else torch_preprocess)(mine)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.shares_memory(got, mine)   # in place, as Keras does it
    # ... and the same float32 operations written the way the INPUT operator is stated (include/cpx.h)
    param, shift, scale, bgr = tg.INPUT_MODES[mode]
    v = (x[..., ::-1] if bgr else x) / F32(param)
    v = v - shift
    if scale is not None:
        v = v / scale
    assert v.dtype == np.float32 and np.array_equal(v.view(np.uint32), want.view(np.uint32))


# ---- LiteInterpreter on the five names ----
def write_model(d, name, model_name, blob, channels=("thermal", "thermal", "filtered"), labels=6):
    (d / (name + ".tflite")).write_bytes(blob)
    with open(d / (name + ".json"), "w") as fh:
        json.dump({"labels": ["l%d" % i for i in range(labels)], "type": "thermal",
                   "hyperparams": {"frame_size": 32, "model_name": model_name, "channels": list(channels)}}, fh)
    return d / (name + ".tflite")


@pytest.fixture(scope="module")
def small_densenet():
    return tp.densenet(6, blocks=(2, 2), growth=8, seed=1)


@pytest.mark.parametrize("model_name", CAFFE + TORCH)
def test_lite_interpreter_takes_the_channel_mean_families(tmp_path, small_densenet, model_name):
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, caffe_preprocess, get_interpreter, torch_preprocess

    path = write_model(tmp_path, "m", model_name, small_densenet)
    interp = get_interpreter(ModelConfig.load({"id": 1, "name": "m", "model_file": str(path)}))
    assert isinstance(interp, LiteInterpreter)
    caffe = model_name in CAFFE
    assert interp.input_mode == ("caffe" if caffe else "torch")
    assert interp.preprocess_fn is (caffe_preprocess if caffe else torch_preprocess)
    assert not interp.limits_flags() & _lib.LIMITS_TF_SCALING and not interp.limits_flags(single=True) & _lib.LIMITS_TF_SCALING
    # the crop kernel's two-channel sample: the INPUT operator in front, with the mode's constants
    _, plan = interp._plan((32, 32, 2))
    op = plan.ops[0]
    assert op.kind == _lib.GRAPH_INPUT == 18 and op.name == "INPUT" and plan.input_shape == (32, 32, 2)
    assert not any(o.kind in (_lib.GRAPH_INPUT, _lib.GRAPH_CHANNEL_MAP) for o in plan.ops[1:])
    if caffe:
        assert op.channel_map == [1, 0, 0] and op.param == 1.0 and op.scale is None
        assert np.array_equal(op.shift, np.array([103.939, 116.779, 123.68], F32))
    else:
        assert op.channel_map == [0, 0, 1] and op.param == 255.0
        assert np.array_equal(op.shift, np.array([0.485, 0.456, 0.406], F32)) and np.array_equal(op.scale, np.array([0.229, 0.224, 0.225], F32))
    # a sample of the graph's own three channels is the caller's to preprocess: no INPUT operator, as before
    _, own = interp._plan((32, 32, 3))
    assert own.input_shape == (32, 32, 3) and not any(o.kind in (_lib.GRAPH_INPUT, _lib.GRAPH_CHANNEL_MAP) for o in own.ops)


def test_tf_families_keep_their_scaling_flag(tmp_path, small_densenet):
    from cpx.ml_tools.interpreter import LiteInterpreter, inc3_preprocess

    interp = LiteInterpreter(write_model(tmp_path, "m", "resnetv2", small_densenet))
    assert interp.input_mode is None and interp.preprocess_fn is inc3_preprocess and interp.limits_flags() & _lib.LIMITS_TF_SCALING
    _, plan = interp._plan((32, 32, 2))
    assert plan.ops[0].kind == _lib.GRAPH_CHANNEL_MAP and plan.ops[0].channel_map == [0, 0, 1]


def channels_graph(c):
    m = tb.Model()
    x = m.tensor([1, 8, 8, c], name="input")
    m.inputs = [x]
    rng = np.random.default_rng(c)
    y = m.mean(m.conv(x, rng.normal(size=(8, 1, 1, c)).astype(F32), np.zeros(8, F32), 1, tb.SAME, tb.RELU))
    m.outputs = [m.unary("LOGISTIC", m.dense(y, rng.normal(size=(6, 8)).astype(F32), np.zeros(6, F32)))]
    return m.finish()


@pytest.mark.parametrize("model_name,mode", [("vgg16", "caffe"), ("densenet121", "torch")])
@pytest.mark.parametrize("c", [2, 4])
def test_a_graph_of_two_or_four_channels_is_refused_by_mode_name(tmp_path, model_name, mode, c):
    from cpx.ml_tools.interpreter import LiteInterpreter

    channels = ["thermal", "filtered", "thermal", "filtered"][:c]
    path = write_model(tmp_path, "m", model_name, channels_graph(c), channels=channels)
    with pytest.raises(NotImplementedError, match="%r input mode" % mode):
        LiteInterpreter(path)
    # ... and by the planner itself
    with pytest.raises(ValueError, match="input_mode %r" % mode):
        build_plan(Graph(channels_graph(c)), channel_map=[0, 1, 0, 1][:c], input_mode=mode)
    with pytest.raises(ValueError, match="input_mode %r" % mode):
        build_plan(Graph(channels_graph(3)), input_mode=mode)   # no channel map
    with pytest.raises(ValueError, match="input_mode 'tf'"):
        build_plan(Graph(channels_graph(3)), channel_map=[0, 0, 1], input_mode="tf")


@pytest.mark.parametrize("model_name", CAFFE + TORCH)
def test_the_other_interpreters_still_refuse(tmp_path, small_densenet, model_name):
    from cpx.ml_tools.interpreter import Interpreter, WRResNetInterpreter

    path = write_model(tmp_path, "m", model_name, small_densenet)
    with pytest.raises(NotImplementedError, match="caffe"):
        WRResNetInterpreter(path, run_over_network=True)
    with pytest.raises(NotImplementedError, match="caffe"):
        Interpreter(path)


def test_fuse_preact_switch(tmp_path, monkeypatch, small_densenet):
    from cpx.ml_tools.interpreter import LiteInterpreter

    path = write_model(tmp_path, "m", "densenet121", small_densenet)
    monkeypatch.delenv("CPX_TFLITE_FUSE_PREACT", raising=False)
    on = next(iter(LiteInterpreter(path)._plans.values()))
    monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT", "0")
    off = next(iter(LiteInterpreter(path)._plans.values()))
    assert len(on.ops) == len(off.ops) - 5 and "AFFINE>CONV_2D" in on.census() and "AFFINE>CONV_2D" not in off.census()
    monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT", "yes")
    with pytest.raises(ValueError, match="CPX_TFLITE_FUSE_PREACT='yes': one of 0, 1"):
        LiteInterpreter(path)


# ---- folding ----
def signature(plan):
    rows = [(o.kind, o.name, str(o.in0), str(o.in1), str(o.out), o.act, plan.tensors[o.out].arena_offset, plan.tensors[o.out].c_offset)
            for o in plan.ops]
    return zlib.crc32(json.dumps(rows).encode()), plan.arena_floats, len(plan.ops)


def test_densenet_folds_exactly_the_affines_in_front_of_1x1_convolutions():
    g = Graph(tp.densenet(6, blocks=(3, 3), growth=8, seed=2))
    plain, fused = build_plan(g), build_plan(g, fuse_preactivation=True)
    # 2 blocks x 3 layers + 1 transition + the final one in front of MEAN
    assert plain.census() == {"PAD": 2, "CONV_2D": 14, "MAX_POOL_2D": 1, "MUL+ADD": 8, "AVERAGE_POOL_2D": 1, "MEAN": 1,
                              "FULLY_CONNECTED": 1, "LOGISTIC": 1}
    assert fused.census() == {"PAD": 2, "CONV_2D": 7, "AFFINE>CONV_2D": 7, "MAX_POOL_2D": 1, "MUL+ADD": 1, "AVERAGE_POOL_2D": 1,
                              "MEAN": 1, "FULLY_CONNECTED": 1, "LOGISTIC": 1}
    assert len(plain.ops) == 29 and len(fused.ops) == 22 and not plain.copies() and not fused.copies()
    pre = [o for o in fused.ops if o.kind == _lib.GRAPH_CONV_PRE]
    assert len(pre) == 7 and all((o.kh, o.kw) == (1, 1) and o.param == float(tb.RELU) for o in pre)
    # the survivor feeds MEAN
    (last,) = [o for o in fused.ops if o.kind == _lib.GRAPH_AFFINE]
    assert [o.kind for o in fused.ops if o.in0 == last.out] == [_lib.GRAPH_MEAN]
    # every folded convolution reads what its AFFINE read: the growing channel slice of the block's one tensor
    affines = {o.out: o for o in plain.ops if o.kind == _lib.GRAPH_AFFINE}
    convs = {o.out: o for o in plain.ops if o.kind == _lib.GRAPH_CONV}
    for o in pre:
        a = affines[convs[o.out].in0]
        assert o.in0 == a.in0 and np.array_equal(o.pre_scale, a.scale) and np.array_equal(o.pre_shift, a.shift)
        assert a.out not in fused.tensors
    slices = [(fused.tensors[o.in0].C, fused.tensors[o.in0].c_stride) for o in pre]
    assert slices == [(16, 40), (24, 40), (32, 40), (40, 40), (20, 44), (28, 44), (36, 44)]
    assert fused.output_shape == plain.output_shape and fused.arena_floats <= plain.arena_floats


def test_default_is_off_and_changes_no_plan():
    for blob in (tp.densenet(6, seed=2), tp.resnet_v2(6, seed=2), tb.inception_v3(6, (), seed=7, width=0.25)):
        g = Graph(blob)
        assert signature(build_plan(g)) == signature(build_plan(g, fuse_preactivation=False))
        assert not any(o.kind == _lib.GRAPH_CONV_PRE for o in build_plan(g).ops)
    # a family without a pre-activation: nothing to fold
    g = Graph(tb.inception_v3(6, (), seed=7, width=0.25))
    assert signature(build_plan(g, fuse_preactivation=True)) == signature(build_plan(g))


def test_two_readers_fold_into_both_convolutions():
    g = Graph(tp.resnet_v2(6, seed=2))
    plain, fused = build_plan(g), build_plan(g, fuse_preactivation=True)
    assert plain.census()["MUL+ADD"] == 3 and fused.census()["MUL+ADD"] == 1 and fused.census()["AFFINE>CONV_2D"] == 3
    pre = [o for o in fused.ops if o.kind == _lib.GRAPH_CONV_PRE]
    # the first block's projection shortcut and conv1 read the max pool's output; the second block's conv1 the ADD's
    assert pre[0].in0 == pre[1].in0 != pre[2].in0 and pre[0].out != pre[1].out
    assert np.array_equal(pre[0].pre_scale, pre[1].pre_scale) and np.array_equal(pre[0].pre_shift, pre[1].pre_shift)
    assert {plain.ops[k].kind for k, o in enumerate(plain.ops) if o.out == pre[0].in0} == {_lib.GRAPH_MAX_POOL}
    assert len(plain.ops) == len(fused.ops) + 2


def reader_graph(reader):
    """input -> MUL, ADD+RELU -> a 1 x 1 convolution and `reader` beside it -> ADD -> output."""
    rng = np.random.default_rng(5)
    m = tb.Model()
    x = m.tensor([1, 8, 8, 16], name="input")
    m.inputs = [x]
    p = tp.preact(m, rng, x)
    y = m.conv(p, *tp._conv_w(rng, 16, 1, 16), 1, tb.SAME, tb.NONE)
    if reader == "pool":
        z = m.pool("MAX_POOL_2D", p, 3, 1, tb.SAME)
    elif reader == "pad":
        z = m.conv(m.pad(p, [[0, 0], [1, 1], [1, 1], [0, 0]]), *tp._conv_w(rng, 16, 3, 16), 1, tb.VALID, tb.NONE)
    else:
        z = m.conv(p, *tp._conv_w(rng, 16, 3, 16), 1, tb.SAME, tb.NONE)
    m.outputs = [m.binary("ADD", y, z)]
    return m.finish(), p


@pytest.mark.parametrize("reader", ["pool", "pad", "hybrid", "output"])
def test_no_fold_when_a_reader_is_no_float_convolution(reader):
    blob, p = reader_graph("conv" if reader in ("hybrid", "output") else reader)
    g = Graph(blob)
    if reader in ("hybrid", "output"):   # two float32 convolutions read it: both would fold
        assert build_plan(g, fuse_preactivation=True).census()["AFFINE>CONV_2D"] == 2
    if reader == "hybrid":
        g = Graph(td.quantise(blob, min_elements=200))   # both filters (256 and 2304 elements)
        plan = build_plan(g, fuse_preactivation=True, quantised_math="hybrid")
        assert sum(o.kind == _lib.GRAPH_CONV_Q8 for o in plan.ops) == 2
        # multiplied out on the host they are float32 convolutions again
        assert build_plan(g, fuse_preactivation=True, quantised_math="float").census().get("AFFINE>CONV_2D") == 2
    elif reader == "output":
        plan = build_plan(g, fuse_preactivation=True, output=p)
        assert [o.kind for o in plan.ops] == [_lib.GRAPH_AFFINE]
        return
    else:
        plan = build_plan(g, fuse_preactivation=True)
    assert signature(plan) == signature(build_plan(g, quantised_math="hybrid"))
    assert sum(o.kind == _lib.GRAPH_AFFINE for o in plan.ops) == 1 and not any(o.kind == _lib.GRAPH_CONV_PRE for o in plan.ops)


def test_hybrid_twin_quantises_one_of_two_readers():
    """One reader hybrid, one float32: the AFFINE stays for both."""
    blob, _ = reader_graph("conv")
    g = Graph(td.quantise(blob, min_elements=1024))
    plan = build_plan(g, fuse_preactivation=True)
    kinds = [o.kind for o in plan.ops]
    assert kinds.count(_lib.GRAPH_CONV_Q8) == 1 and kinds.count(_lib.GRAPH_CONV) == 1 and kinds.count(_lib.GRAPH_AFFINE) == 1


@pytest.mark.parametrize("act", [tb.RELU, tb.RELU6])
def test_packed_weights_of_a_conv_pre(act):
    rng = np.random.default_rng(9)
    blob, _, _ = tp.preact_conv(rng, 3, 1, tb.SAME, 40, 24, 9, act=act)
    g = Graph(blob)
    plain, fused = build_plan(g), build_plan(g, fuse_preactivation=True)
    (affine, conv), (pre,) = plain.ops, fused.ops
    assert pre.kind == _lib.GRAPH_CONV_PRE == 19 and pre.name == "AFFINE>CONV_2D" and pre.param == float(act) and pre.act == tb.NONE
    assert pre.in0 == fused.input == affine.in0
    image = tg.pack_conv_filter(conv.filter)
    assert image.shape == (9, 48, 32) and pre.weights.dtype == np.float32 and pre.weights.shape == (image.size + 2 * 48,)
    assert np.array_equal(pre.weights[:image.size], image.reshape(-1)) and np.array_equal(conv.weights, image)
    consts = pre.weights[image.size:].reshape(2, 48)
    assert np.array_equal(consts[0, :40], affine.scale) and np.array_equal(consts[1, :40], affine.shift)
    assert not consts[:, 40:].any() and affine.act == act
    assert np.array_equal(pre.shift, conv.shift) and pre.scale is None


def test_describe_prints_the_input_mode(tmp_path, small_densenet):
    path = write_model(tmp_path, "m", "densenet121", small_densenet)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "tflite_to_npz.py"), "--describe", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "input mode: torch (model_name densenet121" in r.stdout and "AFFINE>CONV_2D: 5" in r.stdout
    os.remove(tmp_path / "m.json")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "tflite_to_npz.py"), "--describe", str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "input mode" not in r.stdout
