"""The EfficientNet family in the TFLite graph planner (cpx/ml_tools/tflite_graph.py), without a GPU: a swish (LOGISTIC +
MUL of two activations) folded into its producer or run as one AFFINE operator, the sigmoid of a squeeze-and-excite gate
folded, the gate's broadcasting MUL, DIV by a constant, the refusals that remain, a generated EfficientNet-B0
(tests/tflite_build_se.py), the plans of the existing families unchanged, and activate() of csrc/cpx_graph_core.h built
for the host against float64."""
import ctypes as C
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_dw as td
import tflite_build_se as ts
from cpx import _lib
from cpx.ml_tools.tflite_graph import ACT_LOGISTIC, ACT_SWISH, build_plan
from cpx.ml_tools.tflite_reader import ACT_NONE, ACT_RELU, Graph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conv_w(rng, co, k, cin):
    return (rng.normal(0, np.sqrt(2.0 / (k * k * cin)), size=(co, k, k, cin)).astype(np.float32),
            rng.normal(0, 0.05, size=co).astype(np.float32))


def dw_w(rng, k, c):
    return (rng.normal(0, np.sqrt(2.0 / (k * k)), size=(1, k, k, c)).astype(np.float32), rng.normal(0, 0.05, size=c).astype(np.float32))


def swish_graph(kind, cin=16, cout=40, k=3, size=9, act=tb.NONE, logistic_first=False, third_reader=False, quantised=False,
                stride=1):
    """input -> CONV_2D | DEPTHWISE_CONV_2D -> swish [-> output; with third_reader: output = ADD(swish, x)]."""
    rng = np.random.default_rng(cin + cout + k)
    m = ts.ModelSE()
    x = m.tensor([1, size, size, cin], name="input")
    m.inputs = [x]
    if kind == "conv":
        y = m.conv(x, *conv_w(rng, cout, k, cin), stride, tb.SAME, act)
    else:
        y = m.depthwise(x, *dw_w(rng, k, cin), stride, tb.SAME, act)
    s = m.swish(y, logistic_first)
    m.outputs = [m.binary("ADD", s, y) if third_reader else s]
    blob = m.finish()
    return (td.quantise(blob, min_elements=0) if quantised else blob), y


def names(plan):
    return [o.name for o in plan.ops]


# ---- the swish ----
@pytest.mark.parametrize("kind,quantised,want_kind", [("conv", False, _lib.GRAPH_CONV), ("dw", False, _lib.GRAPH_DWCONV),
                                                      ("conv", True, _lib.GRAPH_CONV_Q8), ("dw", True, _lib.GRAPH_DWCONV_Q8)],
                         ids=["CONV", "DWCONV", "CONV_Q8", "DWCONV_Q8"])
@pytest.mark.parametrize("logistic_first", [False, True], ids=["x_times_s", "s_times_x"])
def test_swish_folds_into_its_producer(kind, quantised, want_kind, logistic_first):
    blob, _ = swish_graph(kind, quantised=quantised, logistic_first=logistic_first)
    g = Graph(blob)
    plan = build_plan(g)
    op = plan.ops[-1]
    assert len(plan.ops) == (2 if quantised else 1) and op.kind == want_kind and op.act == ACT_SWISH
    assert op.name == g.ops[0]["name"] + "+SWISH" and op.out == g.outputs[0] == plan.output
    assert set(plan.tensors) == {plan.input, plan.output} | ({op.in1} if quantised else set())
    # unfused: the three launches
    plain = build_plan(g, fuse_activations=False)
    assert [o.kind for o in plain.ops][-3:] == [want_kind, _lib.GRAPH_LOGISTIC, _lib.GRAPH_MUL]
    assert all(o.act == ACT_NONE for o in plain.ops) and plain.arena_floats > plan.arena_floats == (4 if quantised else 0)


def test_swish_falls_back_to_one_affine_operator():
    # x has a third reader
    blob, y = swish_graph("conv", third_reader=True)
    plan = build_plan(Graph(blob))
    assert [(o.kind, o.name, o.act) for o in plan.ops] == [(_lib.GRAPH_CONV, "CONV_2D", ACT_NONE), (_lib.GRAPH_AFFINE, "SWISH", ACT_SWISH),
                                                           (_lib.GRAPH_ADD, "ADD", ACT_NONE)]
    assert plan.ops[1].in0 == y and plan.ops[1].scale is None and plan.ops[1].shift is None
    # the producer already carries a fused RELU
    blob, y = swish_graph("dw", act=tb.RELU)
    plan = build_plan(Graph(blob))
    assert [(o.kind, o.act) for o in plan.ops] == [(_lib.GRAPH_DWCONV, ACT_RELU), (_lib.GRAPH_AFFINE, ACT_SWISH)]
    # x is the output asked for: its producer keeps writing x itself, and nothing behind it is needed
    blob, y = swish_graph("conv")
    plan = build_plan(Graph(blob), output=y)
    assert [(o.kind, o.act, o.out) for o in plan.ops] == [(_lib.GRAPH_CONV, ACT_NONE, y)] and plan.output == y
    # x is the graph's input: no producer
    m = ts.ModelSE()
    x = m.tensor([1, 5, 5, 8], name="input")
    m.inputs = [x]
    m.outputs = [m.swish(x)]
    plan = build_plan(Graph(m.finish()))
    assert [(o.kind, o.act) for o in plan.ops] == [(_lib.GRAPH_AFFINE, ACT_SWISH)]
    # a MUL that carries an activation of its own is no swish: LOGISTIC (folded as a sigmoid would be wrong: x has two readers) + MUL
    m = ts.ModelSE()
    x = m.tensor([1, 5, 5, 8], name="input")
    m.inputs = [x]
    y = m.conv(x, *conv_w(np.random.default_rng(1), 8, 1, 8), 1, tb.SAME, tb.NONE)
    m.outputs = [m.mul(y, m.unary("LOGISTIC", y), act=tb.RELU)]
    plan = build_plan(Graph(m.finish()))
    assert [(o.kind, o.act) for o in plan.ops] == [(_lib.GRAPH_CONV, ACT_NONE), (_lib.GRAPH_LOGISTIC, ACT_NONE), (_lib.GRAPH_MUL, ACT_RELU)]


def test_constants_fold_in_front_of_a_swish_and_not_behind_it():
    rng = np.random.default_rng(2)
    m = ts.ModelSE()
    x = m.tensor([1, 7, 7, 8], name="input")
    m.inputs = [x]
    y = m.conv(x, *conv_w(rng, 12, 3, 8), 1, tb.SAME, tb.NONE)
    y = m.binary("ADD", m.binary("MUL", y, rng.uniform(0.5, 2, size=12).astype(np.float32)), rng.normal(size=12).astype(np.float32))
    m.outputs = [m.binary("MUL", m.swish(y), np.full(12, 3.0, np.float32))]
    plan = build_plan(Graph(m.finish()))
    assert [(o.name, o.act) for o in plan.ops] == [("CONV_2D+MUL+ADD+SWISH", ACT_SWISH), ("MUL", ACT_NONE)]
    assert plan.ops[1].kind == _lib.GRAPH_AFFINE and np.all(plan.ops[1].scale == 3.0)


# ---- the sigmoid and the gate ----
def se_graph(gate_first=False, reshape=False, c=24, size=6, spatial_gate=False):
    rng = np.random.default_rng(c)
    m = ts.ModelSE()
    x = m.tensor([1, size, size, c], name="input")
    m.inputs = [x]
    if spatial_gate:
        g = m.conv(x, *conv_w(rng, 1, 1, c), 1, tb.SAME, tb.NONE)   # [H, W, 1]
    else:
        g = m.reshape(m.mean(x), [1, 1, 1, c]) if reshape else m.mean(x, keep_dims=True)
        g = m.swish(m.conv(g, *conv_w(rng, c // 4, 1, c), 1, tb.SAME, tb.NONE))
        g = m.conv(g, *conv_w(rng, c, 1, c // 4), 1, tb.SAME, tb.NONE)
    g = m.unary("LOGISTIC", g)
    m.outputs = [m.mul(g, x) if gate_first else m.mul(x, g)]
    return m.finish()


@pytest.mark.parametrize("gate_first", [False, True])
@pytest.mark.parametrize("reshape", [False, True], ids=["keep_dims", "mean_reshape"])
def test_squeeze_and_excite_block(gate_first, reshape):
    g = Graph(se_graph(gate_first, reshape))
    plan = build_plan(g)
    assert [(o.kind, o.name, o.act) for o in plan.ops] == [
        (_lib.GRAPH_MEAN, "MEAN", ACT_NONE), (_lib.GRAPH_CONV, "CONV_2D+SWISH", ACT_SWISH), (_lib.GRAPH_CONV, "CONV_2D+LOGISTIC", ACT_LOGISTIC),
        (_lib.GRAPH_MUL, "MUL", ACT_NONE)]
    mul = plan.ops[-1]
    t0, t1 = plan.tensors[mul.in0], plan.tensors[mul.in1]
    assert (t0.H, t0.W, t0.C) == (6, 6, 24) and (t1.H, t1.W, t1.C) == (1, 1, 24) and mul.in0 == plan.input   # the gate is in1
    assert plan.output_shape == (6, 6, 24)
    conv_in = plan.tensors[plan.ops[1].in0]
    assert (conv_in.H, conv_in.W, conv_in.C) == (1, 1, 24) and conv_in.alias == reshape   # the convolution reads the RESHAPE's view
    assert conv_in.arena_offset == plan.tensors[plan.ops[0].out].arena_offset
    plain = build_plan(g, fuse_activations=False)
    assert [o.kind for o in plain.ops] == [_lib.GRAPH_MEAN, _lib.GRAPH_CONV, _lib.GRAPH_LOGISTIC, _lib.GRAPH_MUL, _lib.GRAPH_CONV,
                                           _lib.GRAPH_LOGISTIC, _lib.GRAPH_MUL]
    assert all(o.act == ACT_NONE for o in plain.ops)


def test_a_logistic_behind_a_dense_layer_stays_a_launch():
    rng = np.random.default_rng(3)
    m = ts.ModelSE()
    x = m.tensor([1, 4, 4, 8], name="input")
    m.inputs = [x]
    y = m.dense(m.mean(x), rng.normal(size=(5, 8)).astype(np.float32), rng.normal(size=5).astype(np.float32))
    m.outputs = [m.unary("LOGISTIC", y)]
    plan = build_plan(Graph(m.finish()))
    assert [(o.kind, o.act) for o in plan.ops] == [(_lib.GRAPH_MEAN, 0), (_lib.GRAPH_FC, 0), (_lib.GRAPH_LOGISTIC, 0)]


def test_same_shape_mul():
    m = ts.ModelSE()
    x = m.tensor([1, 5, 5, 6], name="input")
    m.inputs = [x]
    m.outputs = [m.mul(m.unary("RELU", x), m.unary("RELU6", x), act=tb.RELU6)]
    plan = build_plan(Graph(m.finish()))
    assert [(o.kind, o.act) for o in plan.ops][-1] == (_lib.GRAPH_MUL, tb.RELU6) and plan.output_shape == (5, 5, 6)


# ---- DIV ----
def test_div_by_a_constant_folds():
    rng = np.random.default_rng(4)
    c = np.array([0.229, 3.0, 7.0, 1e-3, 255.0, 0.1, 9.0, 0.7], np.float32)
    m = ts.ModelSE()
    x = m.tensor([1, 5, 5, 8], name="input")
    m.inputs = [x]
    m.outputs = [m.div(m.conv(x, *conv_w(rng, 8, 1, 8), 1, tb.SAME, tb.NONE), c)]
    plan = build_plan(Graph(m.finish()))
    assert names(plan) == ["CONV_2D+DIV"]
    want = (1.0 / c.astype(np.float64)).astype(np.float32)
    assert np.array_equal(plan.ops[0].scale.view(np.uint32), want.view(np.uint32))
    # on the input (the in-model Normalization) it joins the AFFINE operator in front of it; a scalar divides every channel
    m = ts.ModelSE()
    x = m.tensor([1, 5, 5, 3], name="input")
    m.inputs = [x]
    m.outputs = [m.div(m.binary("SUB", x, np.array([1, 2, 3], np.float32)), np.array([255.0], np.float32))]
    plan = build_plan(Graph(m.finish()))
    assert names(plan) == ["SUB+DIV"] and plan.ops[0].kind == _lib.GRAPH_AFFINE
    r = np.float32(1.0 / 255.0)
    assert np.array_equal(plan.ops[0].scale, np.full(3, r)) and np.array_equal(plan.ops[0].shift, np.array([-1, -2, -3], np.float32) * r)


# ---- refusals: by name and index ----
def refusal(blob, **kw):
    with pytest.raises(NotImplementedError) as e:
        build_plan(Graph(blob), **kw)
    return str(e.value)


def test_refusals_name_the_operator():
    assert "operator 2 (MUL)" in (msg := refusal(se_graph(spatial_gate=True))) and "(6, 6, 1)" in msg
    assert "operator 2 (MUL)" in refusal(se_graph(spatial_gate=True), fuse_activations=False)
    m = ts.ModelSE()
    x = m.tensor([1, 5, 5, 8], name="input")
    m.inputs = [x]
    m.outputs = [m.div(m.unary("RELU", x), m.unary("RELU6", x))]
    assert "operator 2 (DIV) of two activations" in refusal(m.finish())
    m = ts.ModelSE()
    x = m.tensor([1, 5, 5, 8], name="input")
    m.inputs = [x]
    m.outputs = [m.div(m.unary("RELU", x), np.ones(8, np.float32), const_first=True)]
    assert "operator 1 (DIV)" in (msg := refusal(m.finish())) and "c / x" in msg
    m = ts.ModelSE()
    x = m.tensor([1, 5, 5, 8], name="input")
    m.inputs = [x]
    m.outputs = [m.hard_swish(m.unary("RELU", x))]
    assert "operator 1 (HARD_SWISH)" in refusal(m.finish())


# ---- a generated EfficientNet-B0 ----
@pytest.fixture(scope="module")
def b0():
    return ts.efficientnet_b0(17, (), seed=7, width=0.25, size=64, head_gain=4.0)


def test_generated_b0(b0):
    g = Graph(b0)
    census = {}
    for op in g.ops:
        census[op["name"]] = census.get(op["name"], 0) + 1
    # 16 blocks: 15 expansions, 16 depthwise, 2 x 16 SE, 16 projections, stem and top; a swish behind 49 of the convolutions
    assert census == {"MUL": 2 + 49 + 16, "SUB": 1, "PAD": 5, "CONV_2D": 1 + 15 + 32 + 16 + 1, "DEPTHWISE_CONV_2D": 16,
                      "LOGISTIC": 49 + 16 + 1, "MEAN": 17, "ADD": 10, "FULLY_CONNECTED": 1}   # (width 0.25: the first block keeps its 8 channels and adds)
    assert sorted(set(g.const(op["inputs"][1]).shape[1] for op in g.ops if op["name"] == "DEPTHWISE_CONV_2D")) == [3, 5]
    plan = build_plan(g)
    assert plan.census() == {"MUL+SUB+MUL": 1, "PAD": 5, "CONV_2D+SWISH": 33, "DEPTHWISE_CONV_2D+SWISH": 16, "MEAN": 17,
                             "CONV_2D+LOGISTIC": 16, "MUL": 16, "CONV_2D": 16, "ADD": 10, "FULLY_CONNECTED": 1, "LOGISTIC": 1}
    assert plan.output_shape == (1, 1, 17) and plan.input_shape == (64, 64, 3)
    assert sum(o.kind == _lib.GRAPH_MUL for o in plan.ops) == 16 and not plan.copies()
    plain = build_plan(g, fuse_activations=False)
    assert len(plain.ops) == len(plan.ops) + 2 * 49 + 16
    assert plan.arena_floats < plain.arena_floats
    # the converter's other layouts plan to the same launches
    other = build_plan(Graph(ts.efficientnet_b0(17, (), seed=7, width=0.25, size=64, normalisation_div=True, se_reshape=True)))
    assert [o.kind for o in other.ops] == [o.kind for o in plan.ops] and other.ops[0].name == "MUL+SUB+DIV"
    # dynamic-range quantised: the hybrid operators carry the fused activations
    q = build_plan(Graph(td.quantise(b0)))
    acts = {(o.kind, o.act) for o in q.ops}
    assert (_lib.GRAPH_CONV_Q8, ACT_SWISH) in acts and (_lib.GRAPH_DWCONV_Q8, ACT_SWISH) in acts and (_lib.GRAPH_CONV_Q8, ACT_LOGISTIC) in acts
    qf = build_plan(Graph(td.quantise(b0)), quantised_math="float")
    assert [o.name for o in qf.ops] == [o.name for o in plan.ops]


def test_describe_shows_the_fused_operators(b0, tmp_path):
    import sys

    path = tmp_path / "b0.tflite"
    path.write_bytes(b0)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "tflite_to_npz.py"), "--describe", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    launches = [line for line in r.stdout.splitlines() if line.startswith("launches:")]
    assert len(launches) == 1 and "CONV_2D+SWISH: 33" in launches[0] and "DEPTHWISE_CONV_2D+SWISH: 16" in launches[0] \
        and "CONV_2D+LOGISTIC: 16" in launches[0] and "MUL: 16" in launches[0]


# ---- the plans of the existing families: as the parent commit made them ----
def signature(plan):
    rows = [(o.kind, o.name, str(o.in0), str(o.in1), str(o.out), o.act, plan.tensors[o.out].arena_offset, plan.tensors[o.out].c_offset)
            for o in plan.ops]
    return zlib.crc32(json.dumps(rows).encode()), plan.arena_floats, len(plan.ops)


# (crc of kinds, names, tensors, activations and arena offsets; arena floats; launches), computed at the parent commit
PARENT = {
    "inception_v3": ((3586028531, 142344, 110), {"AVERAGE_POOL_2D": 9, "CONV_2D": 94, "FULLY_CONNECTED": 1, "LOGISTIC": 1, "MAX_POOL_2D": 4,
                                                  "MEAN": 1}),
    "mobilenet_v2": ((1720909283, 622144, 70), {"ADD": 11, "CONV_2D": 35, "DEPTHWISE_CONV_2D": 17, "FULLY_CONNECTED": 1, "LOGISTIC": 1,
                                                  "MEAN": 1, "PAD": 4}),
    "mobilenet_v2_q8": ((2631623575, 622144, 111), {"ADD": 10, "CONV_2D": 35, "DEPTHWISE_CONV_2D": 17, "FULLY_CONNECTED": 1, "LOGISTIC": 1,
                                                     "MEAN": 1, "PAD": 4, "QUANT_PARAMS": 42}),
}


@pytest.mark.parametrize("family", sorted(PARENT))
def test_existing_plans_unchanged(family):
    blob = {"inception_v3": lambda: tb.inception_v3(17, (), seed=7, width=0.25),
            "mobilenet_v2": lambda: td.mobilenet_v2(17, (), seed=7, width=0.25),
            "mobilenet_v2_q8": lambda: td.quantise(td.mobilenet_v2(17, (), seed=7, width=0.5))}[family]()
    g = Graph(blob)
    fused, plain = build_plan(g), build_plan(g, fuse_activations=False)
    sig, census = PARENT[family]
    assert signature(fused) == signature(plain) == sig and fused.census() == plain.census() == census
    for a, b in zip(fused.ops, plain.ops):
        assert (a.kind, a.out, a.act, fused.tensors[a.out].arena_offset) == (b.kind, b.out, b.act, plain.tensors[b.out].arena_offset)


# ---- activate() on the host ----
@pytest.fixture(scope="module")
def act_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("graph_act") / "libgraph_act_host.so"
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall",
                           "-I", os.path.join(REPO, "classifier-pipeline_amd", "csrc"), "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "native", "graph_act_host.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.activate_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def host_activate(lib, v, act):
    v = np.ascontiguousarray(v, np.float32)
    out = np.zeros_like(v)
    lib.activate_host(v.ctypes.data_as(C.c_void_p), act, v.size, out.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.parametrize("act", [ACT_SWISH, ACT_LOGISTIC], ids=["swish", "logistic"])
def test_activate_against_float64(act_lib, act):
    edge = np.array([88.0, -88.0, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0], np.float32)
    small = np.logspace(-44, np.log10(88.0), 5000)
    v = np.concatenate([edge, np.linspace(-88, 88, 200001), small, -small]).astype(np.float32)
    got = host_activate(act_lib, v, act)
    x = v.astype(np.float64)
    s = 1.0 / (1.0 + np.exp(-x))
    want = x * s if act == ACT_SWISH else s
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)   # (2^-149 in the denormal range)
    err = np.abs(got.astype(np.float64) - want) / ulp
    print("largest error %.2f ulp at %r" % (err.max(), v[err.argmax()]))
    assert np.all(np.isfinite(got)) and err.max() <= 4.0
    if act == ACT_SWISH:
        assert got[2] == 0.0 and got[3] == 0.0 and np.signbit(got[3]) and not np.signbit(got[2])   # -0.0 * 0.5 = -0.0
        # a fused swish is LOGISTIC then MUL, operation for operation
        sig = host_activate(act_lib, v, ACT_LOGISTIC)
        assert np.array_equal((v * sig).astype(np.float32).view(np.uint32), got.view(np.uint32))
    else:
        assert got[2] == got[3] == 0.5 and got[0] == 1.0 and 0.0 < got[1] < 1e-38
    # beyond the grid nothing turns into a NaN either: expf overflows to inf, the sigmoid is 0, and finite * 0 = -0
    far = host_activate(act_lib, [-89.0, -100.0, -3e38, 89.0, 100.0, 3e38], act)
    assert np.array_equal(far[:3], [0.0] * 3) and np.array_equal(far[3:], np.array([89.0, 100.0, 3e38] if act == ACT_SWISH else [1.0] * 3, np.float32))
    assert act_lib.mean_wide_pixels_host() == _lib.GRAPH_MEAN_WIDE_PIXELS == 256 and act_lib.mean_stripes_host() == 64
