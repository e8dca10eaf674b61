"""The host side of the full-integer EfficientNet path (no GPU): the planner's 256-entry tables against the NumPy restatement
of the arithmetic (tests/tflite_eval_i8.evaluate, which reads the Graph only), the rules by which a table folds into the
convolution in front of it, what the two build_plan options integer_gate_mul / integer_lut leave alone when they are off,
the plan of a small EfficientNet-B0, and LiteInterpreter's CPX_TFLITE_I8_LUT."""
import json

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_i8_se as tis
import tflite_eval_i8 as te8
from cpx import _lib
from cpx.ml_tools import tflite_graph as tg
from cpx.ml_tools import tflite_graph_i8 as tg8
from cpx.ml_tools.tflite_reader import Graph

NAMES = {getattr(_lib, "GRAPH_" + k): k for k in ("QUANTIZE", "DEQUANTIZE", "CONV_I8", "CONV_I8_GROUPED", "DWCONV_I8", "FC_I8", "ADD_I8",
                                                  "MUL_I8", "MEAN_I8", "SLICE", "LUT_I8", "LOGISTIC", "SOFTMAX")}
X_QP, SWISH_QP = (np.float32(0.05), 7), (np.float32(0.026), -117)
HDR = 4 * _lib.GRAPH_I8_HDR_WORDS
Q = np.arange(-128, 128)


def plan_of(blob, **options):
    options = dict(dict(integer_gate_mul=True, integer_lut=True), **options)
    return tg.build_plan(Graph(blob), integer_activations=True, grouped_convolutions=True, **options)


def kinds(plan):
    return [NAMES.get(o.kind, o.name) + ("+LUT" if o.act == _lib.GRAPH_ACT_LUT else "") for o in plan.ops]


def every_byte(qp):
    """[1, 1, 1, 256] float32 that QUANTIZE with `qp` turns into q = -128 .. 127."""
    return (np.float32(qp[0]) * (Q - qp[1]).astype(np.float32)).astype(np.float32).reshape(1, 1, 1, 256)


def conv(m, x, cout, k=1, groups=1, qp=X_QP, rng=None):
    rng = rng or np.random.default_rng(cout)
    cin = m.shape(x)[3]
    w, ws, bias = tis.random_filter(rng, (cout, k, k, cin // groups), k * k * cin // groups, m.qp(x), qp[0])
    return m.conv_i8(x, w, ws, bias, qp)


# ---- the tables ----
TABLE_SWEEP = [
    # (s_in, z_in), (s_out, z_out)
    ((0.05, 7), tis.LOGISTIC_QP),
    ((0.05, -128), tis.LOGISTIC_QP),            # the zero point's two edges
    ((0.05, 127), tis.LOGISTIC_QP),
    ((0.5, 3), tis.LOGISTIC_QP),                # +-64: the table saturates at both ends, 127 by the clamp (256 - 128)
    ((0.0235, -20), (1.0 / 200.0, -100)),       # a calibrated output range
    ((0.11, 40), (1.0 / 255.0, -128)),
    ((0.003, 0), (1.0 / 256.0, -128)),          # +-0.4: the middle of the sigmoid only
    ((0.05, 7), (1.0 / 1000.0, -128)),          # an output scale that clamps most of the table at 127
]


@pytest.mark.parametrize("in_qp,out_qp", TABLE_SWEEP)
def test_logistic_table_equals_the_restatement(in_qp, out_qp):
    in_qp, out_qp = (np.float32(in_qp[0]), in_qp[1]), (np.float32(out_qp[0]), out_qp[1])
    m, q = tis.start([1, 1, 1, 256], in_qp)
    y = m.logistic_i8(q, out_qp)
    g = Graph(tis.finish(m, m.quantize(y, out_qp)))
    vals = te8.evaluate(g, every_byte(in_qp))
    assert np.array_equal(vals[q].reshape(-1), Q)
    want = vals[y].reshape(-1)
    got = tg8.logistic_table(in_qp[0], in_qp[1], out_qp[0], out_qp[1])
    assert got.dtype == np.int8 and got.shape == (256,) and np.array_equal(got, want)
    assert np.all(np.diff(want) >= 0)
    if in_qp[0] == np.float32(0.5):
        assert want[0] == -128 and want[-1] == 127
    # the planner puts exactly these bytes behind the header of the LUT_I8 launch
    plan = plan_of(tis.finish(m, m.quantize(y, out_qp)))
    assert kinds(plan) == ["QUANTIZE", "LUT_I8", "QUANTIZE", "DEQUANTIZE"]
    shift = plan.ops[1].shift
    assert shift.dtype == np.uint8 and shift.size == _lib.GRAPH_I8_LUT_BYTES == 320 and np.array_equal(tg8.table_of(shift), want)


@pytest.mark.parametrize("act", [tb.NONE, tb.RELU6, tb.RELU])
@pytest.mark.parametrize("in_qp,l_qp,out_qp", [(X_QP, tis.LOGISTIC_QP, SWISH_QP), ((0.047, -128), (1.0 / 250.0, -120), (0.03, -100)),
                                               ((0.2, 127), tis.LOGISTIC_QP, (0.01, -128)), ((0.5, -3), (1.0 / 256.0, -128), (0.3, 5))])
def test_swish_table_equals_logistic_then_mul(in_qp, l_qp, out_qp, act):
    """S[q + 128] = MUL_I8(q, L[q + 128]) with the MUL's own constants, its fused RELU / RELU6 included."""
    in_qp, l_qp, out_qp = [(np.float32(s), z) for s, z in (in_qp, l_qp, out_qp)]
    for logistic_first in (False, True):
        m, q = tis.start([1, 1, 1, 256], in_qp)
        y = m.swish_i8(q, out_qp, l_qp, act, logistic_first)
        g = Graph(tis.finish(m, y))
        want = te8.evaluate(g, every_byte(in_qp))[y].reshape(-1)
        got = tg8.swish_table(in_qp, l_qp, out_qp, act)
        assert got.dtype == np.int8 and np.array_equal(got, want)
        lo, hi = te8.clamp_bounds(act, *out_qp)
        assert want.min() >= lo and want.max() <= hi
        plan = plan_of(tis.finish(m, y))
        if act == tb.NONE:   # the pair the planner takes whole
            assert kinds(plan) == ["QUANTIZE", "LUT_I8", "DEQUANTIZE"] and np.array_equal(tg8.table_of(plan.ops[1].shift), want)
        else:                # a MUL with a fused activation is no swish to the planner: the LOGISTIC's table, then MUL_I8
            assert kinds(plan) == ["QUANTIZE", "LUT_I8", "MUL_I8", "DEQUANTIZE"]


def test_mbqm_on_python_integers():
    rng = np.random.default_rng(4)
    for _ in range(400):
        m, e = tg8.quantize_multiplier(float(rng.uniform(1e-4, 0.9)) * 2.0 ** int(rng.integers(-6, 3)))
        x = int(rng.integers(-(2 ** 16), 2 ** 16))
        assert tg8._mbqm(x, m, e) == int(te8.mbqm(x, m, e))
    assert tg8._mbqm(-3, 2 ** 30, -1) == int(te8.mbqm(-3, 2 ** 30, -1)) and tg8._mbqm(5, 2 ** 30, -1) == int(te8.mbqm(5, 2 ** 30, -1))


# ---- the fold rules ----
def test_tables_fold_into_the_three_filter_kinds():
    """CONV_I8, DWCONV_I8 and CONV_I8_GROUPED take the table of the swish behind them: the activation LUT, 320 bytes in
    `shift` whose first 64 are the header the convolution had (that of the tensor it wrote before the fold), the same M /
    shift / bias, and x is gone."""
    for what, kind in (("conv", "CONV_I8"), ("dw", "DWCONV_I8"), ("grouped", "CONV_I8_GROUPED")):
        m, q = tis.start([1, 5, 6, 16], tis.IN_QPS[1])
        if what == "dw":
            w, ws, bias = tis.random_filter(np.random.default_rng(1), (1, 3, 3, 16), 9, tis.IN_QPS[1], X_QP[0], per_channel_axis=3)
            x = m.depthwise_i8(q, w, ws, bias, X_QP)
        else:
            x = conv(m, q, 24, 3, groups=2 if what == "grouped" else 1)
        y = m.swish_i8(x, SWISH_QP)
        blob = tis.finish(m, y)
        plan, plain = plan_of(blob), plan_of(blob, integer_lut=False)
        assert kinds(plan) == ["QUANTIZE", kind + "+LUT", "DEQUANTIZE"], kinds(plan)
        assert kinds(plain) == ["QUANTIZE", kind, "DEQUANTIZE", "LOGISTIC", "QUANTIZE", "MUL_I8", "DEQUANTIZE"], kinds(plain)
        o, p = plan.ops[1], plain.ops[1]
        assert o.out == y and x not in plan.tensors and o.shift.size == 320 and p.shift.size == HDR
        assert np.array_equal(o.shift[:HDR], p.shift) and np.array_equal(o.scale, p.scale) and np.array_equal(o.weights, p.weights)
        assert np.array_equal(tg8.table_of(o.shift), tg8.swish_table(X_QP, tis.LOGISTIC_QP, SWISH_QP, tb.NONE))
        assert plan.tensors[y].dtype == "int8" and (plan.tensors[y].scale, plan.tensors[y].zero_point) == SWISH_QP


def test_a_lone_logistic_folds_and_a_second_table_does_not():
    """conv -> LOGISTIC folds (the gate's sigmoid); a LOGISTIC behind that one finds a producer that already carries a table
    and is a launch."""
    m, q = tis.start([1, 1, 1, 16], tis.IN_QPS[0])
    a = m.logistic_i8(conv(m, q, 8))
    b = m.logistic_i8(a, (np.float32(1.0 / 128.0), -128))
    plan = plan_of(tis.finish(m, m.quantize(b, (np.float32(0.01), -100))))
    assert kinds(plan) == ["QUANTIZE", "CONV_I8+LUT", "LUT_I8", "QUANTIZE", "DEQUANTIZE"]
    assert np.array_equal(tg8.table_of(plan.ops[1].shift), tg8.logistic_table(*X_QP, *tis.LOGISTIC_QP))


def test_a_third_reader_of_x_makes_the_swish_one_launch():
    m, q = tis.start([1, 4, 4, 16], tis.IN_QPS[0])
    x = conv(m, q, 16)
    y = m.swish_i8(x, SWISH_QP)
    out = m.binary_i8("ADD", x, y, (np.float32(0.06), -20))
    plan = plan_of(tis.finish(m, out))
    assert kinds(plan) == ["QUANTIZE", "CONV_I8", "LUT_I8", "ADD_I8", "DEQUANTIZE"]
    assert (plan.ops[2].in0, plan.ops[2].out, plan.ops[2].name) == (x, y, "SWISH") and plan.ops[2].shift.size == 320


def test_nothing_folds_into_fc_i8():
    rng = np.random.default_rng(2)
    m, q = tis.start([1, 1, 1, 40], tis.IN_QPS[0])
    w, ws, bias = tis.random_filter(rng, (12, 40), 40, tis.IN_QPS[0], X_QP[0])
    x = m.dense_i8(q, w, ws[:1], bias, X_QP)
    plan = plan_of(tis.finish(m, m.swish_i8(x, SWISH_QP)))
    assert kinds(plan) == ["QUANTIZE", "FC_I8", "LUT_I8", "DEQUANTIZE"]


def test_the_head_keeps_its_three_launches():
    """An INT8 LOGISTIC that a DEQUANTIZE reads is the head: DEQUANTIZE -> LOGISTIC -> QUANTIZE under either setting."""
    m, q = tis.start([1, 1, 1, 16], tis.IN_QPS[0])
    blob = tis.finish(m, m.logistic_i8(conv(m, q, 8)))
    for lut in (False, True):
        assert kinds(plan_of(blob, integer_lut=lut)) == ["QUANTIZE", "CONV_I8", "DEQUANTIZE", "LOGISTIC", "QUANTIZE", "DEQUANTIZE"]


def test_a_producer_inside_a_concatenation_folds_and_keeps_its_slice():
    m, q = tis.start([1, 4, 4, 16], tis.IN_QPS[0])
    a = m.swish_i8(conv(m, q, 16), SWISH_QP)
    b = m.swish_i8(conv(m, q, 24, 3), SWISH_QP)
    plan = plan_of(tis.finish(m, m.concat_i8([a, b])))
    assert kinds(plan) == ["QUANTIZE", "CONV_I8+LUT", "CONV_I8+LUT", "DEQUANTIZE"]
    assert [(plan.tensors[t].c_offset, plan.tensors[t].c_stride) for t in (a, b)] == [(0, 40), (16, 40)]
    assert [o.out for o in plan.ops[1:3]] == [a, b]


# ---- the defaults ----
def test_both_options_default_to_off():
    """The gate MUL is refused with the text it always had (now naming the option), an interior LOGISTIC is three launches,
    and the small EfficientNet is refused at its first gate."""
    m, q = tis.start([1, 4, 4, 8], X_QP)
    gate = m.mean_i8(q, X_QP, keep_dims=True)
    blob = tis.finish(m, m.gate_mul_i8(q, gate, X_QP))
    with pytest.raises(NotImplementedError) as e:
        tg.build_plan(Graph(blob), integer_activations=True)
    assert "operator 2 (MUL) of two INT8 tensors of shapes (4, 4, 8), (1, 1, 8): only one shape is run (a [1, 1, C] gate is not)" in str(e.value)
    assert "integer_gate_mul=True" in str(e.value)
    for gate_first in (False, True):
        m, q = tis.start([1, 4, 4, 8], X_QP)
        gate = m.mean_i8(q, SWISH_QP, keep_dims=True)
        y = m.gate_mul_i8(q, gate, X_QP, gate_first=gate_first)
        plan = tg.build_plan(Graph(tis.finish(m, y)), integer_activations=True, integer_gate_mul=True)
        assert kinds(plan) == ["QUANTIZE", "MEAN_I8", "MUL_I8", "DEQUANTIZE"] and (plan.ops[2].in0, plan.ops[2].in1) == (q, gate)
        hdr = tg8.unpack_header(plan.ops[2].shift)
        assert (hdr[_lib.GRAPH_I8_HDR_Z_IN], hdr[_lib.GRAPH_I8_HDR_Z_IN1]) == (X_QP[1], SWISH_QP[1])
    # every other broadcast stays refused with the option on
    m, q = tis.start([1, 4, 4, 8], X_QP)
    row = m.pool_i8("AVERAGE_POOL_2D", q, (4, 1), (4, 1), tb.VALID)
    with pytest.raises(NotImplementedError, match=r"operator 2 \(MUL\).*\[H, W, C\] by \[1, 1, C\]"):
        plan_of(tis.finish(m, m.binary_i8("MUL", q, row, X_QP)))
    m, q = tis.start([1, 4, 4, 8], X_QP)
    gate = m.mean_i8(q, X_QP, keep_dims=True)
    with pytest.raises(NotImplementedError, match=r"operator 2 \(ADD\)"):
        plan_of(tis.finish(m, m.binary_i8("ADD", q, gate, X_QP)))
    m, q = tis.start([1, 4, 4, 16], tis.IN_QPS[0])
    blob = tis.finish(m, m.swish_i8(conv(m, q, 16), SWISH_QP))
    assert kinds(tg.build_plan(Graph(blob), integer_activations=True)) == \
        ["QUANTIZE", "CONV_I8", "DEQUANTIZE", "LOGISTIC", "QUANTIZE", "MUL_I8", "DEQUANTIZE"]
    small = Graph(tis.small_efficientnet())
    with pytest.raises(NotImplementedError, match=r"operator 17 \(MUL\) of two INT8 tensors of shapes \(16, 16, 32\), \(1, 1, 32\)"):
        tg.build_plan(small, integer_activations=True)
    with pytest.raises(NotImplementedError, match=r"operator 17 \(MUL\)"):
        tg.build_plan(small, integer_activations=True, integer_lut=True)
    assert "MUL_I8" in kinds(tg.build_plan(small, integer_activations=True, integer_gate_mul=True))


# ---- the small EfficientNet ----
def test_small_efficientnet_plan():
    """Every swish and every gate sigmoid the flatbuffer holds (13 and 4) is a table folded into its convolution: no LUT_I8
    launch, no DEQUANTIZE / LOGISTIC / QUANTIZE inside, int8 tensors from the QUANTIZE to the DEQUANTIZE, and a smaller
    arena than the plan that keeps the float32 LOGISTICs."""
    g = Graph(tis.small_efficientnet())
    swishes, lone = tis.swishes_and_gates(g)
    assert (len(swishes), len(lone)) == (13, 4)
    plan = plan_of(tis.small_efficientnet(), fold_windows=True)
    plain = plan_of(tis.small_efficientnet(), fold_windows=True, integer_lut=False)
    ks = kinds(plan)
    assert sum(o.name.endswith("+SWISH") and o.act == _lib.GRAPH_ACT_LUT for o in plan.ops) == 13
    assert sum(o.name.endswith("+LOGISTIC") and o.act == _lib.GRAPH_ACT_LUT for o in plan.ops) == 4
    assert "LUT_I8" not in ks and ks.count("MUL_I8") == 4 + 2   # (the four gates; the Rescaling and the Normalization)
    assert ks[0] == "QUANTIZE" and ks[-2:] == ["DEQUANTIZE", "LOGISTIC"]
    assert not set(ks[1:-2]) & {"QUANTIZE", "DEQUANTIZE", "LOGISTIC"}
    for o in plan.ops[1:-2]:
        assert all(plan.tensors[t].dtype == "int8" for t in (o.in0, o.in1, o.out) if t != -1), o.name
    assert sorted(k for k, t in plan.tensors.items() if t.dtype == "float32") == sorted([plan.input, plan.ops[-1].in0, plan.output])
    assert kinds(plain).count("LOGISTIC") == 18 and len(plain.ops) == len(plan.ops) + 17 * 3 + 13
    print("arena bytes per sample: tables %d, integer_lut=False %d; launches %d against %d"
          % (plan.arena_bytes_per_sample, plain.arena_bytes_per_sample, len(plan.ops), len(plain.ops)))
    assert plan.arena_bytes_per_sample < plain.arena_bytes_per_sample


# ---- LiteInterpreter ----
def test_lite_interpreter_reads_cpx_tflite_i8_lut(tmp_path, monkeypatch):
    from cpx.ml_tools.interpreter import LiteInterpreter

    (tmp_path / "eff_i8.tflite").write_bytes(tis.small_efficientnet())
    with open(tmp_path / "eff_i8.json", "w") as fh:
        json.dump({"labels": ["a", "b", "c", "d", "e"], "type": "thermal", "version": "test",
                   "hyperparams": {"frame_size": 32, "model_name": "efficientnetb0", "channels": ["thermal", "thermal", "filtered"]}}, fh)
    monkeypatch.delenv("CPX_TFLITE_I8_LUT", raising=False)
    interp = LiteInterpreter(tmp_path / "eff_i8.tflite")
    assert interp._plan_options["integer_lut"] is True and interp._plan_options["integer_gate_mul"] is True
    assert "LUT_I8" not in kinds(next(iter(interp._plans.values())))
    monkeypatch.setenv("CPX_TFLITE_I8_LUT", "0")
    interp = LiteInterpreter(tmp_path / "eff_i8.tflite")
    assert interp._plan_options["integer_lut"] is False and interp._plan_options["integer_gate_mul"] is True
    assert kinds(next(iter(interp._plans.values()))).count("LOGISTIC") == 18
    monkeypatch.setenv("CPX_TFLITE_I8_LUT", "yes")
    with pytest.raises(ValueError, match="CPX_TFLITE_I8_LUT"):
        LiteInterpreter(tmp_path / "eff_i8.tflite")
