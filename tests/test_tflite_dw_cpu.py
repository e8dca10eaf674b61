"""DEPTHWISE_CONV_2D (the MobileNetV2 family) through the reader and the planner, float32 and dynamic-range quantised: host
work, no GPU.  The flatbuffers come from tests/tflite_build_dw.py, the evaluation from tests/tflite_eval_dw.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_dw as td
import tflite_eval_dw as ted

from cpx import _lib
from cpx.ml_tools import tflite_graph as tg
from cpx.ml_tools.tflite_reader import Graph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def start(shape):
    m = td.ModelDW()
    x = m.tensor([1] + list(shape), name="input")
    m.inputs = [x]
    return m, x


def test_reader_decodes_every_option():
    rng = np.random.default_rng(0)
    m, x = start((9, 12, 6))
    w = rng.normal(size=(1, 3, 5, 6)).astype(np.float32)
    b = rng.normal(size=6).astype(np.float32)
    m.outputs = [m.depthwise(x, w, b, stride=(2, 1), padding=tb.VALID, act=tb.RELU6)]
    g = Graph(m.finish())
    (op,) = g.ops
    assert op["name"] == "DEPTHWISE_CONV_2D" and op["code"] == 4
    assert (op["padding"], op["stride_h"], op["stride_w"], op["depth_multiplier"], op["act"]) == (tb.VALID, 2, 1, 1, tb.RELU6)
    assert (op["dilation_h"], op["dilation_w"]) == (1, 1)
    assert np.array_equal(g.const(op["inputs"][1]), w) and np.array_equal(g.const(op["inputs"][2]), b)
    g.check_executable()
    # the other value of every field
    m, x = start((9, 12, 6))
    m.outputs = [m.depthwise(x, np.ones((1, 3, 3, 12), np.float32), None, stride=(1, 2), padding=tb.SAME, act=tb.RELU,
                             depth_multiplier=2, dilation=(3, 2))]
    (op,) = Graph(m.finish()).ops
    assert (op["padding"], op["stride_h"], op["stride_w"], op["depth_multiplier"], op["act"]) == (tb.SAME, 1, 2, 2, tb.RELU)
    assert (op["dilation_h"], op["dilation_w"]) == (3, 2)


def test_evaluator_equals_a_triple_loop():
    """5 x 5 x 3 input, 3 x 3, stride 2, SAME: 3 x 3 outputs, one pixel of padding all round (total 2: 1 top, 1 bottom)."""
    rng = np.random.default_rng(1)
    x = rng.normal(size=(2, 5, 5, 3))
    w = rng.normal(size=(1, 3, 3, 3)).astype(np.float32)
    b = rng.normal(size=3).astype(np.float32)
    m, t = start((5, 5, 3))
    m.outputs = [m.depthwise(t, w, b, 2, tb.SAME, tb.RELU)]
    g = Graph(m.finish())
    got, mag = ted.evaluate(g, x, magnitudes=True)
    want = np.zeros((2, 3, 3, 3))
    wmag = np.zeros((2, 3, 3, 3))
    for oy in range(3):
        for ox in range(3):
            acc = np.tile(b.astype(np.float64), (2, 1))
            am = np.tile(np.abs(b.astype(np.float64)), (2, 1))
            for ky in range(3):
                for kx in range(3):
                    iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                    if 0 <= iy < 5 and 0 <= ix < 5:
                        acc += x[:, iy, ix, :] * w[0, ky, kx, :].astype(np.float64)
                        am += np.abs(x[:, iy, ix, :]) * np.abs(w[0, ky, kx, :].astype(np.float64))
            want[:, oy, ox, :] = np.maximum(acc, 0)
            wmag[:, oy, ox, :] = am
    assert got[g.outputs[0]].shape == (2, 3, 3, 3)
    assert float(np.abs(got[g.outputs[0]] - want).max()) < 1e-14 and float(np.abs(mag[g.outputs[0]] - wmag).max()) < 1e-14


def test_plan_shapes_pads_and_weights():
    rng = np.random.default_rng(2)
    m, x = start((16, 10, 8))
    w = rng.normal(size=(1, 3, 3, 8)).astype(np.float32)
    b = rng.normal(size=8).astype(np.float32)
    m.outputs = [m.depthwise(x, w, b, 2, tb.SAME, tb.RELU6)]
    plan = tg.build_plan(Graph(m.finish()))
    (o,) = plan.ops
    assert o.kind == _lib.GRAPH_DWCONV == 15 and o.name == "DEPTHWISE_CONV_2D" and plan.output_shape == (8, 5, 8)
    # an even size at stride 2: one pixel of padding, bottom / right
    assert o.pads == (0, 0, 1, 1) and (o.kh, o.kw, o.stride_h, o.stride_w, o.act) == (3, 3, 2, 2, tb.RELU6)
    assert o.scale is None and np.array_equal(o.shift, b) and o.in1 == -1
    assert o.weights.shape == (9, 8) and np.array_equal(o.weights, w.reshape(9, 8))
    # an odd size: symmetric
    m, x = start((17, 17, 8))
    m.outputs = [m.depthwise(x, w, b, 2, tb.SAME)]
    plan = tg.build_plan(Graph(m.finish()))
    assert plan.ops[0].pads == (1, 1, 1, 1) and plan.output_shape == (9, 9, 8)


def test_mul_add_fold_into_the_depthwise_convolution():
    rng = np.random.default_rng(3)
    m, x = start((9, 9, 12))
    w = rng.normal(size=(1, 3, 3, 12)).astype(np.float32)
    b = rng.normal(size=12).astype(np.float32)
    sc, sf = rng.uniform(0.5, 2, size=12).astype(np.float32), rng.normal(size=12).astype(np.float32)
    y = m.depthwise(x, w, b, 1, tb.SAME, tb.NONE)
    m.outputs = [m.binary("ADD", m.binary("MUL", y, sc), sf, tb.RELU6)]
    plan = tg.build_plan(Graph(m.finish()))
    (o,) = plan.ops
    assert o.name == "DEPTHWISE_CONV_2D+MUL+ADD" and o.kind == _lib.GRAPH_DWCONV and o.act == tb.RELU6
    assert np.array_equal(o.scale, sc) and np.array_equal(o.shift, (b * sc + sf).astype(np.float32))


def test_a_depthwise_convolution_is_placed_in_a_concatenation_slice():
    rng = np.random.default_rng(4)
    m, x = start((9, 9, 10))
    d = m.depthwise(x, rng.normal(size=(1, 3, 3, 10)).astype(np.float32), np.zeros(10, np.float32), 1, tb.SAME, tb.RELU)
    c = m.conv(x, rng.normal(size=(6, 1, 1, 10)).astype(np.float32), np.zeros(6, np.float32), 1, tb.SAME, tb.RELU)
    m.outputs = [m.unary("RELU6", m.concat([c, d]))]
    g = Graph(m.finish())
    plan = tg.build_plan(g)
    assert not plan.copies() and [o.name for o in plan.ops] == ["DEPTHWISE_CONV_2D", "CONV_2D", "RELU6"]
    t = plan.tensors[g.ops[0]["outputs"][0]]
    assert (t.C, t.c_offset, t.c_stride) == (10, 6, 16)


def shared_view_model(rng):
    m, x = start((8, 8, 32))
    y = m.unary("RELU", x)
    qd, sd = td.quantise_filter(rng.normal(size=(1, 3, 3, 32)), 3)
    qc, sc = td.quantise_filter(rng.normal(size=(40, 1, 1, 32)), 0)
    a = m.depthwise(y, m.qfilter(qd, sd, dim=3, name="dw_q8"), rng.normal(size=32).astype(np.float32), 1, tb.SAME, tb.RELU6)
    b = m.conv_q8(y, m.qfilter(qc, sc, name="conv_q8"), rng.normal(size=40).astype(np.float32))
    m.outputs = [m.unary("RELU6", m.concat([a, b]))]
    return m.finish(), qd, sd


def test_one_quant_params_serves_both_quantised_consumers_of_a_view():
    blob, qd, sd = shared_view_model(np.random.default_rng(5))
    g = Graph(blob)
    ten = g.quantised_filter(g.ops[1])
    assert ten is not None and ten["quant"]["dim"] == 3 and np.array_equal(ten["const"], qd)
    plan = tg.build_plan(g)
    assert [o.kind for o in plan.ops] == [_lib.GRAPH_AFFINE, _lib.GRAPH_QUANT_PARAMS, _lib.GRAPH_DWCONV_Q8, _lib.GRAPH_CONV_Q8, _lib.GRAPH_AFFINE]
    qp, dw, cv = plan.ops[1:4]
    assert not plan.copies()
    assert _lib.GRAPH_DWCONV_Q8 == 16 and _lib.GRAPH_DWCONV_Q8 in tg.Q8_KINDS
    assert dw.in1 == cv.in1 == qp.out and qp.in0 == dw.in0 == cv.in0 and qp.param == 0.0
    assert np.array_equal(dw.scale, sd) and dw.weights.dtype == np.uint8
    q, wsum = tg.unpack_dw_filter_q8(dw.weights, qd.shape)
    assert np.array_equal(q, qd) and np.array_equal(wsum, qd.astype(np.int64).sum(axis=(0, 1, 2)))


def test_float_mode_multiplies_the_depthwise_filter_out():
    blob, qd, sd = shared_view_model(np.random.default_rng(5))
    g = Graph(blob)
    plan = tg.build_plan(g, quantised_math="float")
    assert [o.kind for o in plan.ops] == [_lib.GRAPH_AFFINE, _lib.GRAPH_DWCONV, _lib.GRAPH_CONV, _lib.GRAPH_AFFINE]
    want = (qd.astype(np.float32) * sd.reshape(1, 1, 1, -1)).astype(np.float32)
    assert np.array_equal(g.dequantised(g.ops[1]["inputs"][1]), want)
    assert np.array_equal(plan.ops[1].filter, want) and np.array_equal(plan.ops[1].weights, tg.pack_dw_filter(want))
    # one scale for the whole filter
    m, x = start((8, 8, 32))
    m.outputs = [m.depthwise(x, m.qfilter(qd, [0.02], dim=3), None)]
    g = Graph(m.finish())
    assert np.array_equal(g.dequantised(g.ops[0]["inputs"][1]), qd.astype(np.float32) * np.float32(0.02))
    (o,) = [p for p in tg.build_plan(g).ops if p.kind == _lib.GRAPH_DWCONV_Q8]
    assert np.array_equal(o.scale, np.full(32, 0.02, np.float32))


@pytest.mark.parametrize("c", [3, 4, 30, 144])
def test_weight_layouts_round_trip(c):
    rng = np.random.default_rng(c)
    w = rng.normal(size=(1, 3, 5, c)).astype(np.float32)
    p = tg.pack_dw_filter(w)
    cp = -(-c // 4) * 4
    assert p.shape == (15, cp) and p.dtype == np.float32 and not p[:, c:].any()
    assert np.array_equal(p[7, :c], w[0, 1, 2]) and np.array_equal(tg.unpack_dw_filter(p, w.shape), w)
    q = rng.integers(-128, 128, size=(1, 3, 5, c)).astype(np.int8)
    pq = tg.pack_dw_filter_q8(q)
    assert pq.dtype == np.uint8 and pq.size == 15 * cp + 4 * cp
    taps = pq[:15 * cp].view(np.int8).reshape(15, cp)
    assert np.array_equal(taps[7, :c], q[0, 1, 2]) and not taps[:, c:].any()
    wsum = pq[15 * cp:].view(np.int32)
    assert np.array_equal(wsum[:c], q.astype(np.int64).sum(axis=(0, 1, 2))) and not wsum[c:].any()
    back, ws = tg.unpack_dw_filter_q8(pq, q.shape)
    assert np.array_equal(back, q) and np.array_equal(ws, wsum[:c])


def refusal(m):
    g = Graph(m.finish())
    with pytest.raises(NotImplementedError) as e:
        tg.build_plan(g)
    return str(e.value)


def test_refusals_name_the_operator_and_index():
    rng = np.random.default_rng(7)
    q = rng.integers(-127, 128, size=(1, 3, 3, 8)).astype(np.int8)

    def begin():
        m, x = start((8, 8, 8))
        return m, m.unary("RELU", x)

    m, y = begin()
    m.outputs = [m.depthwise(y, np.ones((1, 3, 3, 16), np.float32), None, depth_multiplier=2)]
    msg = refusal(m)
    assert "DEPTHWISE_CONV_2D" in msg and "operator 1" in msg and "depth multiplier 2" in msg
    # a multiplier field that disagrees with the shapes is not repaired
    m, y = begin()
    m.outputs = [m.depthwise(y, np.ones((1, 3, 3, 16), np.float32), None, depth_multiplier=1)]
    msg = refusal(m)
    assert "DEPTHWISE_CONV_2D" in msg and "operator 1" in msg and "depth multiplier" in msg
    m, y = begin()
    m.outputs = [m.depthwise(y, np.ones((1, 3, 3, 8), np.float32), None, dilation=2)]
    msg = refusal(m)
    assert "DEPTHWISE_CONV_2D" in msg and "operator 1" in msg and "dilation" in msg
    m, y = begin()
    m.outputs = [m.depthwise(y, np.ones((2, 3, 3, 8), np.float32), None)]
    msg = refusal(m)
    assert "DEPTHWISE_CONV_2D" in msg and "operator 1" in msg and "[2, 3, 3, 8]" in msg
    # INT8 filters: scales along dimension 0, a non-zero zero point, UINT8
    m, y = begin()
    m.outputs = [m.depthwise(y, m.qfilter(q, np.full(8, 0.01), dim=0), None)]
    msg = refusal(m)
    assert "DEPTHWISE_CONV_2D" in msg and "operator 1" in msg and "dimension 0" in msg
    m, y = begin()
    zp = np.zeros(8, np.int64)
    zp[5] = -2
    m.outputs = [m.depthwise(y, m.qfilter(q, np.full(8, 0.01), zero_point=zp, dim=3), None)]
    msg = refusal(m)
    assert "DEPTHWISE_CONV_2D" in msg and "operator 1" in msg and "zero point" in msg
    m, y = begin()
    m.outputs = [m.depthwise(y, m.qfilter(np.abs(q), np.full(8, 0.01), dim=3, ttype=tb.UINT8), None)]
    msg = refusal(m)
    assert "DEPTHWISE_CONV_2D" in msg and "operator 1" in msg and "UINT8" in msg
    # the same filter with its scales where the converter puts them runs
    m, y = begin()
    m.outputs = [m.depthwise(y, m.qfilter(q, np.full(8, 0.01), dim=3), None)]
    tg.build_plan(Graph(m.finish()))


@pytest.fixture(scope="module")
def mobilenet():
    return td.mobilenet_v2(6, (), seed=1, width=1.0)


def test_mobilenet_v2_census(mobilenet):
    g = Graph(mobilenet)
    census = {}
    for op in g.ops:
        census[op["name"]] = census.get(op["name"], 0) + 1
    assert census == {"DEPTHWISE_CONV_2D": 17, "CONV_2D": 35, "ADD": 10, "PAD": 4, "MEAN": 1, "FULLY_CONNECTED": 1, "LOGISTIC": 1}
    plan = tg.build_plan(g)
    assert plan.census()["DEPTHWISE_CONV_2D"] == 17 and plan.output_shape == (1, 1, 6) and plan.input_shape == (160, 160, 3)
    dws = [o for o in plan.ops if o.kind == _lib.GRAPH_DWCONV]
    assert [plan.tensors[o.out].C for o in dws] == [32, 96, 144, 144, 192, 192, 192, 384, 384, 384, 384, 576, 576, 576, 960, 960, 960]
    assert [o.stride_h for o in dws].count(2) == 4 and all(o.pads == (0, 0, 0, 0) for o in dws if o.stride_h == 2)
    assert plan.tensors[dws[-1].out].H == 5


def test_describe_prints_the_depthwise_census(tmp_path, mobilenet):
    tool = os.path.join(REPO, "tools", "tflite_to_npz.py")
    (tmp_path / "mnv2.tflite").write_bytes(mobilenet)
    r = subprocess.run([sys.executable, tool, "--describe", str(tmp_path / "mnv2.tflite")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "DEPTHWISE_CONV_2D: 17" in r.stdout and "CONV_2D: 35" in r.stdout and "[160, 160, 3]" in r.stdout
    blob = td.quantise(mobilenet)
    g = Graph(blob)
    hybrid = [op for op in g.ops if g.quantised_filter(op) is not None]
    n_dw = sum(op["name"] == "DEPTHWISE_CONV_2D" for op in hybrid)
    # the depthwise filters of 1024 elements or more: 9 x C with C >= 114, i.e. all but the first two (32 and 96 channels)
    assert n_dw == 15 and len(hybrid) > n_dw
    n8 = sum(int(np.prod(g.quantised_filter(op)["shape"])) for op in hybrid)
    (tmp_path / "mnv2q8.tflite").write_bytes(blob)
    r = subprocess.run([sys.executable, tool, "--describe", str(tmp_path / "mnv2q8.tflite")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "DEPTHWISE_CONV_2D: 17" in r.stdout
    assert "hybrid operators (int8 filter, activations quantised per sample): %d; int8 weight bytes: %d" % (len(hybrid), n8) in r.stdout


def test_get_interpreter_routes_a_mobilenet(tmp_path):
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, get_interpreter

    labels = ["l%d" % i for i in range(6)]
    (tmp_path / "mnv2.tflite").write_bytes(td.mobilenet_v2(6, (), seed=1, width=0.25))
    with open(tmp_path / "mnv2.json", "w") as fh:
        json.dump({"labels": labels, "type": "thermal",
                   "hyperparams": {"frame_size": 32, "model_name": "mobilenet", "channels": ["thermal", "thermal", "filtered"]}}, fh)
    interp = get_interpreter(ModelConfig.load({"id": 1, "name": "mnv2", "model_file": str(tmp_path / "mnv2.tflite")}))
    assert isinstance(interp, LiteInterpreter) and interp.labels == labels and interp.shape() == (1, (1, 160, 160, 3))
    assert interp.channel_map() == [0, 0, 1]
    flags = interp.limits_flags()
    assert flags & _lib.LIMITS_TF_SCALING and not flags & _lib.LIMITS_SWAP_CHANNELS
    plan = next(iter(interp._plans.values()))
    assert sum(o.kind == _lib.GRAPH_DWCONV for o in plan.ops) == 17
