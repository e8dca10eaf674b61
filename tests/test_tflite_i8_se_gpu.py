"""The EfficientNet family's full-integer operators on the GPU: LUT_I8, the activation LUT of CONV_I8 / CONV_I8_GROUPED /
DWCONV_I8 and MUL_I8 by a [1, 1, C] gate (csrc/cpx_graph_i8.hip), a whole squeeze-and-excite block and a small
EfficientNet-B0, against the NumPy restatement of the arithmetic (tests/tflite_eval_i8.py, which reads the Graph only: the
planner's tables take no part in it).  Every comparison is np.array_equal on the dequantised output: no tolerance.  The
flatbuffers are synthetic (tests/tflite_build_i8_se.py); parity with a TFLite runtime is not pinned."""
import json

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_i8_se as tis
import tflite_eval_i8 as te8
from tflite_build_i8_se import IN_QPS, levels, random_filter as scaled_filter

pytestmark = pytest.mark.gpu

LABELS5 = ["bird", "cat", "false-positive", "hedgehog", "possum"]
X_QP = (np.float32(0.05), 7)              # a swish's x: +-6.4 around a non-zero zero point
SWISH_QP = (np.float32(0.026), -117)      # its output: [-0.28, 6.4] widened to hold 0


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def run(engine, blob, x, output=None, **options):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    options = dict(dict(integer_gate_mul=True, integer_lut=True), **options)
    plan = build_plan(g, input_shape=x.shape[1:], output=output, integer_activations=True, grouped_convolutions=True, **options)
    dev = GraphDevice(engine, plan)
    out = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device)).cpu().numpy()
    dev.close()
    return g, plan, out


def kinds(plan):
    from cpx import _lib

    names = {getattr(_lib, "GRAPH_" + k): k for k in ("QUANTIZE", "DEQUANTIZE", "CONV_I8", "CONV_I8_GROUPED", "DWCONV_I8", "FC_I8",
                                                      "ADD_I8", "MUL_I8", "MAX_POOL_I8", "AVG_POOL_I8", "MEAN_I8", "SLICE", "LUT_I8")}
    return [names.get(o.kind, o.name) + ("+LUT" if o.act == _lib.GRAPH_ACT_LUT else "") for o in plan.ops]


def check(engine, blob, x, what, expect_kinds=None, **options):
    """The forward's output equals the restatement's, bit for bit."""
    g, plan, got = run(engine, blob, x, **options)
    want = te8.evaluate(g, x)[g.outputs[0]]
    if expect_kinds is not None:
        assert kinds(plan) == expect_kinds, kinds(plan)
    differ = int((got.reshape(want.shape) != want).sum())
    print("%s: %d of %d elements differ, %d distinct values" % (what, differ, want.size, len(np.unique(want))))
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want), what
    return g, plan, got


# ---- LUT_I8 alone ----
@pytest.mark.parametrize("c", [16, 5])
def test_lut_i8(engine, c):
    """N = 3, 3 x 5 pixels; C = 16 moves sixteen bytes per lane, C = 5 goes byte by byte.  A swish and a lone LOGISTIC behind
    a QUANTIZE (nothing to fold into) are LUT_I8 launches; then the same inside a concatenation: the table's output at
    channel offset C of a row of 3 C, and a second table that READS that slice."""
    rng = np.random.default_rng([3, c])
    x = levels(rng, (3, 3, 5, c), X_QP, every=True)   # all 256 values at C = 16; 225 elements at C = 5: -128 .. 95 and 127
    m, q = tis.start([1, 3, 5, c], X_QP)
    g, _, _ = check(engine, tis.finish(m, m.swish_i8(q, SWISH_QP)), x, "swish C %d" % c, ["QUANTIZE", "LUT_I8", "DEQUANTIZE"])
    assert len(np.unique(te8.evaluate(g, x)[q])) == min(256, x.size)
    m, q = tis.start([1, 3, 5, c], X_QP)
    y = m.quantize(m.logistic_i8(q), (np.float32(1.0 / 200.0), -100))
    check(engine, tis.finish(m, y), x, "LOGISTIC C %d" % c, ["QUANTIZE", "LUT_I8", "QUANTIZE", "DEQUANTIZE"])
    m, q = tis.start([1, 3, 5, c], X_QP)
    a = m.quantize(q, SWISH_QP)
    b = m.swish_i8(q, SWISH_QP, logistic_first=True)
    d = m.swish_i8(b, SWISH_QP, l_qp=(np.float32(1.0 / 250.0), -120))
    g, plan, _ = check(engine, tis.finish(m, m.concat_i8([a, b, d])), x, "LUT_I8 in a concatenation, C %d" % c,
                       ["QUANTIZE", "QUANTIZE", "LUT_I8", "LUT_I8", "DEQUANTIZE"])
    assert (plan.tensors[b].c_offset, plan.tensors[b].c_stride) == (c, 3 * c) and plan.tensors[d].c_offset == 2 * c


# ---- CONV_I8 + table ----
CONV_LUT_CASES = [
    # k, stride, cin, cout, groups
    (1, 1, 24, 40, 1),
    (3, 1, 24, 40, 1),
    (3, 2, 24, 40, 1),
    (1, 2, 32, 40, 1),      # sixteen bytes at a time
    (3, 1, 16, 48, 2),      # CONV_I8_GROUPED
    (1, 1, 24, 160, 1),     # four tiles per workgroup, gridDim.y = 2
    (1, 1, 32, 160, 1),     # ... sixteen bytes at a time
    (3, 1, 32, 48, 2),      # CONV_I8_GROUPED, sixteen bytes at a time
    (3, 1, 16, 80, 2),      # ... two tiles per group, byte by byte
    (1, 1, 32, 80, 2),      # ... and sixteen bytes at a time
    (3, 1, 16, 144, 2),     # ... three tiles per group (above 64 channels): four per workgroup, byte by byte
    (1, 1, 32, 144, 2),     # ... and sixteen bytes at a time
]


@pytest.mark.parametrize("case", CONV_LUT_CASES, ids=lambda c: "k%d_s%d_%d_%d_g%d" % c)
def test_conv_i8_with_table(engine, case):
    """CONV_2D + swish on N = 3 samples of 7 x 9: 189 pixels at stride 1 (two workgroups, the last partial), 40 output
    channels = two tiles with the second partial.  z_in != 0; the MUL's operands in either order."""
    k, stride, cin, cout, groups = case
    for n, in_qp in enumerate(IN_QPS):
        rng = np.random.default_rng([k, stride, cin, cout, n])
        m, q = tis.start([1, 7, 9, cin], in_qp)
        w, ws, bias = scaled_filter(rng, (cout, k, k, cin // groups), k * k * cin // groups, in_qp, X_QP[0])
        y = m.swish_i8(m.conv_i8(q, w, ws, bias, X_QP, stride, tb.SAME), SWISH_QP, logistic_first=bool(n))
        _, plan, got = check(engine, tis.finish(m, y), levels(rng, (3, 7, 9, cin), in_qp), "conv + swish %s z_in %d" % (case, in_qp[1]),
                             ["QUANTIZE", ("CONV_I8_GROUPED" if groups > 1 else "CONV_I8") + "+LUT", "DEQUANTIZE"])
        assert len(np.unique(got)) > 40   # (the table's output is not saturated)


def test_conv_i8_with_table_into_a_concatenation(engine):
    """Two convolutions with a swish behind each write the channel slices (offsets 0 and 24 of 64) of a concatenated tensor;
    a gate's LOGISTIC folds into a third."""
    rng = np.random.default_rng(77)
    in_qp = IN_QPS[1]
    m, q = tis.start([1, 7, 9, 24], in_qp)

    def conv(x, cout, k, qp_in):
        w, ws, bias = scaled_filter(rng, (cout, k, k, m.shape(x)[3]), k * k * m.shape(x)[3], qp_in, X_QP[0])
        return m.conv_i8(x, w, ws, bias, X_QP, 1, tb.SAME)

    a = m.swish_i8(conv(q, 24, 1, in_qp), SWISH_QP)
    b = m.swish_i8(conv(q, 40, 3, in_qp), SWISH_QP)
    cat = m.concat_i8([a, b])
    y = m.quantize(m.logistic_i8(conv(cat, 20, 1, SWISH_QP)), (np.float32(1.0 / 200.0), -100))
    g, plan, _ = check(engine, tis.finish(m, y), levels(rng, (3, 7, 9, 24), in_qp), "conv + swish into a concatenation",
                       ["QUANTIZE", "CONV_I8+LUT", "CONV_I8+LUT", "CONV_I8+LUT", "QUANTIZE", "DEQUANTIZE"])
    assert (plan.tensors[b].c_offset, plan.tensors[b].c_stride) == (24, 64)


# ---- DWCONV_I8 + table ----
@pytest.mark.parametrize("c", [24, 32])
def test_dwconv_i8_with_table(engine, c):
    """3 x 3 stride 1 SAME, and 5 x 5 stride 2 VALID behind a PAD that fold_windows folds into it."""
    for k, stride in ((3, 1), (5, 2)):
        for in_qp in IN_QPS:
            rng = np.random.default_rng([k, c, in_qp[1]])
            m, q = tis.start([1, 7, 9, c], in_qp)
            w, ws, bias = scaled_filter(rng, (1, k, k, c), k * k, in_qp, X_QP[0], per_channel_axis=3)
            if stride == 2:
                t = m.depthwise_i8(m.pad_i8(q, [[0, 0], [2, 2], [1, 2], [0, 0]]), w, ws, bias, X_QP, 2, tb.VALID)
            else:
                t = m.depthwise_i8(q, w, ws, bias, X_QP, 1, tb.SAME)
            check(engine, tis.finish(m, m.swish_i8(t, SWISH_QP)), levels(rng, (3, 7, 9, c), in_qp),
                  "depthwise %d x %d + swish, C %d z_in %d" % (k, k, c, in_qp[1]), ["QUANTIZE", "DWCONV_I8+LUT", "DEQUANTIZE"],
                  fold_windows=True)


# ---- MUL_I8 by the gate ----
@pytest.mark.parametrize("gate_first", [False, True])
@pytest.mark.parametrize("c", [24, 32])
def test_gate_mul_i8(engine, c, gate_first):
    """N = 3 samples whose means differ by far more than a step: a gate taken from the wrong sample shows everywhere.  Three
    different non-zero zero points and a fused RELU."""
    rng = np.random.default_rng([c, gate_first])
    qp, gate_qp, out_qp = (np.float32(0.04), -9), (np.float32(0.025), 21), (np.float32(0.05), -40)
    x = levels(rng, (3, 4, 6, c), qp)
    x[0], x[2] = np.float32(0.5) * x[0] + np.float32(2.0), np.float32(0.5) * x[2] - np.float32(2.0)
    m, q = tis.start([1, 4, 6, c], qp)
    gate = m.mean_i8(q, gate_qp, keep_dims=True)
    y = m.gate_mul_i8(q, gate, out_qp, tb.RELU, gate_first=gate_first)
    g, plan, got = check(engine, tis.finish(m, y), x, "gate MUL C %d" % c, ["QUANTIZE", "MEAN_I8", "MUL_I8", "DEQUANTIZE"])
    gates = te8.evaluate(g, x)[gate]
    assert np.abs(gates[0] - gates[1]).mean() > 20 and np.abs(gates[2] - gates[1]).mean() > 20
    mul = next(o for o in plan.ops if o.name == "MUL")
    assert (mul.in0, mul.in1) == (q, gate)


def test_graph_create_refuses_a_table_or_a_gate_elsewhere(engine):
    """cpx_graph_create: the activation LUT on any kind but the three filter kinds, and a 1 x 1 x C second operand of ADD_I8."""
    from cpx import _lib
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    m, q = tis.start([1, 4, 6, 16], X_QP)
    gate = m.mean_i8(q, X_QP, keep_dims=True)
    blob = tis.finish(m, m.gate_mul_i8(q, gate, SWISH_QP))
    for change, why in ((dict(act=_lib.GRAPH_ACT_LUT), "activation LUT"), (dict(kind=_lib.GRAPH_ADD_I8, param=1.0), "different shapes")):
        plan = build_plan(Graph(blob), integer_activations=True, integer_gate_mul=True)
        mul = next(o for o in plan.ops if o.kind == _lib.GRAPH_MUL_I8)
        vars(mul).update(change)
        with pytest.raises(_lib.CpxError, match=why):
            GraphDevice(engine, plan)
    GraphDevice(engine, build_plan(Graph(blob), integer_activations=True, integer_gate_mul=True)).close()


# ---- a whole squeeze-and-excite block ----
@pytest.mark.parametrize("reshape", [False, True])
def test_squeeze_and_excite_block_i8(engine, reshape):
    """depthwise + swish -> MEAN (keep_dims, or MEAN + RESHAPE) -> 1 x 1 + swish -> 1 x 1 + LOGISTIC -> MUL by the gate ->
    the projection.  Everything folds: no LUT_I8 launch."""
    rng = np.random.default_rng(50 + reshape)
    in_qp, c = IN_QPS[0], 32
    m, q = tis.start([1, 6, 5, c], in_qp)
    w, ws, bias = scaled_filter(rng, (1, 3, 3, c), 9, in_qp, X_QP[0], per_channel_axis=3)
    y = m.swish_i8(m.depthwise_i8(q, w, ws, bias, X_QP, 1, tb.SAME), SWISH_QP)
    sq_qp = (np.float32(0.012), -100)
    sq = m.reshape_i8(m.mean_i8(y, sq_qp), [1, 1, 1, c]) if reshape else m.mean_i8(y, sq_qp, keep_dims=True)
    w, ws, bias = scaled_filter(rng, (8, 1, 1, c), c, sq_qp, X_QP[0])
    r = m.swish_i8(m.conv_i8(sq, w, ws, bias, X_QP), SWISH_QP)
    w, ws, bias = scaled_filter(rng, (c, 1, 1, 8), 8, SWISH_QP, X_QP[0])
    gate = m.logistic_i8(m.conv_i8(r, w, ws, bias, X_QP))
    gated = m.gate_mul_i8(y, gate, (np.float32(0.02), -120))
    w, ws, bias = scaled_filter(rng, (16, 1, 1, c), c, (np.float32(0.02), -120), np.float32(0.03))
    out = m.conv_i8(gated, w, ws, bias, (np.float32(0.03), 4))
    g, plan, got = check(engine, tis.finish(m, out), levels(rng, (3, 6, 5, c), in_qp), "squeeze-and-excite, reshape %s" % reshape,
                         ["QUANTIZE", "DWCONV_I8+LUT", "MEAN_I8", "CONV_I8+LUT", "CONV_I8+LUT", "MUL_I8", "CONV_I8", "DEQUANTIZE"])
    assert not np.array_equal(got[0], got[1]) and len(np.unique(got)) > 40


# ---- the small EfficientNet ----
@pytest.fixture(scope="module")
def network():
    from cpx.ml_tools.tflite_reader import Graph

    blob = tis.small_efficientnet()
    g = Graph(blob)
    x = np.random.default_rng(21).uniform(0, 255, size=(3, 32, 32, 3)).astype(np.float32)
    logits_t = next(op["outputs"][0] for op in g.ops if op["name"] == "DEQUANTIZE")
    return blob, g, x, logits_t, te8.evaluate(g, x)


def test_small_efficientnet_logits_bit_equal(engine, network):
    """The DEQUANTIZE's result at N = 3, bit for bit, every table folded.  The reference alone shows that this is no vacuous
    pass: the samples' logits differ and no swish output with more than one pixel is saturated (at most 25 % of its values
    at -128 or 127).  The same file with integer_lut=False (the float32 kernel between a DEQUANTIZE and a QUANTIZE) may
    differ where an element of an interior LOGISTIC sits within 1e-3 of a tie: those are counted and printed, and the two
    plans must agree outright only where there is none."""
    blob, g, x, logits_t, want = network
    swishes, lone = tis.swishes_and_gates(g)
    worst = 0.0
    for _, mul, _ in swishes:
        v = want[g.ops[mul]["outputs"][0]]
        if v.shape[1] * v.shape[2] > 1:
            worst = max(worst, float(((v == -128) | (v == 127)).mean()))
    print("largest saturated share of a swish output: %.1f %%" % (100 * worst))
    assert worst <= 0.25
    assert not np.array_equal(want[logits_t][0], want[logits_t][1]) and not np.array_equal(want[logits_t][1], want[logits_t][2])
    _, plan, got = run(engine, blob, x, output=logits_t, fold_windows=True)
    assert "LUT_I8" not in kinds(plan) and sum(k.endswith("+LUT") for k in kinds(plan)) == len(swishes) + len(lone)
    print("tabled plan: %d of %d logits differ, launches %s" % (int((got != want[logits_t]).sum()), got.size, plan.census()))
    assert np.array_equal(got, want[logits_t])
    _, plain, other = run(engine, blob, x, output=logits_t, fold_windows=True, integer_lut=False)
    near = total = 0
    for i, op in enumerate(g.ops):
        if op["name"] == "LOGISTIC" and i < len(g.ops) - 1 and g.tensors[op["outputs"][0]]["type"] == te8.INT8:
            xf = te8.dequantize(want[op["inputs"][0]], *te8._qp(g, op["inputs"][0])).astype(np.float64)
            t = (1.0 / (1.0 + np.exp(-xf))) / float(te8._qp(g, op["outputs"][0])[0])
            near += int((np.abs(t - np.floor(t) - 0.5) <= 1e-3).sum())
            total += t.size
    print("integer_lut=False: %d launches against %d; %d of %d LOGISTIC elements within 1e-3 of a tie; %d of %d logits differ "
          "from the tabled plan" % (len(plain.ops), len(plan.ops), near, total, int((other != got).sum()), got.size))
    assert len(plain.ops) >= len(plan.ops) + 3 * (len(swishes) + len(lone))
    assert near > 0 or np.array_equal(other, got)


def test_get_interpreter_with_a_full_integer_efficientnet(network, tmp_path):
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, get_interpreter

    blob, g, x, logits_t, _ = network
    (tmp_path / "eff_i8.tflite").write_bytes(blob)
    with open(tmp_path / "eff_i8.json", "w") as fh:
        json.dump({"labels": LABELS5, "type": "thermal", "version": "test",
                   "hyperparams": {"frame_size": 32, "model_name": "efficientnetb0", "channels": ["thermal", "thermal", "filtered"]}}, fh)
    interp = get_interpreter(ModelConfig.load({"id": 5, "name": "eff_i8", "model_file": str(tmp_path / "eff_i8.tflite")}))
    assert isinstance(interp, LiteInterpreter) and interp._plan_options["integer_lut"] and interp._plan_options["integer_gate_mul"]
    x2 = np.ascontiguousarray(x[..., :2])
    got = interp.predict(x2)
    want = te8.evaluate(g, np.ascontiguousarray(x2[..., [0, 0, 1]]))[logits_t]
    # (behind the DEQUANTIZE the head is the float32 LOGISTIC kernel: one float32 expf and division per element)
    probs = 1.0 / (1.0 + np.exp(-want.astype(np.float64)))
    assert got.shape == (3, 5) and float(np.abs(got - probs).max()) <= 1e-6
