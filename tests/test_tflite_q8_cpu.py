"""Dynamic-range quantised TFLite files (INT8 filters, float32 activations) through the reader and the planner: host work,
no GPU.  The flatbuffers come from tests/tflite_build_q8.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_q8 as tq

from cpx import _lib
from cpx.ml_tools import tflite_graph as tg
from cpx.ml_tools.tflite_reader import Graph, convert


def test_quantisation_table_reads_back_exactly():
    rng = np.random.default_rng(0)
    m = tq.ModelQ8()
    x = m.tensor([1, 8, 8, 32], name="input")
    m.inputs = [x]
    q = rng.integers(-127, 128, size=(40, 3, 3, 32)).astype(np.int8)
    scale = rng.uniform(1e-3, 1e-2, size=40).astype(np.float32)
    y = m.conv_q8(x, m.qfilter(q, scale, name="conv_filter"), rng.normal(size=40).astype(np.float32), act=tb.RELU)
    y = m.mean(y)
    qd = rng.integers(-127, 128, size=(30, 40)).astype(np.int8)
    m.outputs = [m.dense_q8(y, m.qfilter(qd, [0.0125], name="dense_filter"), np.zeros(30, np.float32), asymmetric=True)]
    g = Graph(m.finish())
    conv, fc = g.ops[0], g.ops[2]
    t = g.tensors[conv["inputs"][1]]
    assert t["type"] == 9 and t["const"].dtype == np.int8 and np.array_equal(t["const"], q) and t["name"] == "conv_filter"
    assert np.array_equal(t["quant"]["scale"], scale) and t["quant"]["scale"].dtype == np.float32
    assert np.array_equal(t["quant"]["zero_point"], np.zeros(40, np.int64)) and t["quant"]["dim"] == 0
    t = g.tensors[fc["inputs"][1]]
    assert np.array_equal(t["const"], qd) and np.array_equal(t["quant"]["scale"], np.array([0.0125], np.float32))
    assert fc["asymmetric_quantize_inputs"] is True and g.tensors[x]["quant"] is None
    g.check_executable()
    m2 = tq.ModelQ8()
    x = m2.tensor([1, 1, 1, 40], name="input")
    m2.inputs = [x]
    m2.outputs = [m2.dense_q8(m2.reshape(x, [1, 40]), m2.qfilter(qd, [0.5]), np.zeros(30, np.float32), asymmetric=False)]
    assert Graph(m2.finish()).ops[-1]["asymmetric_quantize_inputs"] is False


def small_block(rng, cin=64):
    """A two-branch block: a placed concatenation of two quantised 1 x 1 convolutions' outputs that three quantised
    convolutions read."""
    m = tb.Model()
    x = m.tensor([1, 9, 9, cin], name="input")
    m.inputs = [x]

    def conv(t, co, k=1):
        ci = m.shape(t)[3]
        return m.conv(t, rng.normal(0, 0.1, size=(co, k, k, ci)).astype(np.float32), rng.normal(0, 0.05, size=co).astype(np.float32),
                      1, tb.SAME, tb.RELU)

    cat = m.concat([conv(x, 32), conv(x, 48)])
    m.outputs = [m.unary("RELU6", m.concat([conv(cat, 24), conv(cat, 16, 3), conv(cat, 40)]))]
    return m.finish()


def test_float_mode_multiplies_the_filters_out():
    rng = np.random.default_rng(1)
    blob = tq.quantise(small_block(rng))
    g = Graph(blob)
    assert sum(g.quantised_filter(op) is not None for op in g.ops) == 5
    plan = tg.build_plan(g, quantised_math="float")
    assert not any(o.kind in tg.Q8_KINDS + (_lib.GRAPH_QUANT_PARAMS,) for o in plan.ops)
    convs = [o for o in plan.ops if o.kind == _lib.GRAPH_CONV]
    assert len(convs) == 5
    for o in convs:
        ten = g.tensors[g.ops[o.source]["inputs"][1]]
        want = ten["const"].astype(np.float32) * ten["quant"]["scale"].reshape(-1, 1, 1, 1)
        assert o.filter.dtype == np.float32 and np.array_equal(o.filter, want)
        assert np.array_equal(o.weights, tg.pack_conv_filter(want))
    with pytest.raises(ValueError, match="quantised_math"):
        tg.build_plan(g, quantised_math="int4")


def test_quantise_keeps_small_filters_float():
    rng = np.random.default_rng(2)
    m = tb.Model()
    x = m.tensor([1, 8, 8, 3], name="input")
    m.inputs = [x]
    y = m.conv(x, rng.normal(size=(32, 3, 3, 3)).astype(np.float32), np.zeros(32, np.float32))    # 864 elements
    m.outputs = [m.conv(y, rng.normal(size=(32, 1, 1, 32)).astype(np.float32), np.zeros(32, np.float32))]   # 1024
    g = Graph(tq.quantise(m.finish()))
    assert [g.quantised_filter(op) is not None for op in g.ops] == [False, True]
    w = Graph(m.finish()).const(g.ops[1]["inputs"][1])
    ten = g.tensors[g.ops[1]["inputs"][1]]
    assert np.array_equal(ten["quant"]["scale"], (np.abs(w).reshape(32, -1).max(axis=1) / np.float32(127)).astype(np.float32))
    assert int(np.abs(ten["const"]).max()) == 127
    plan = tg.build_plan(g)
    assert [o.kind for o in plan.ops] == [_lib.GRAPH_CONV, _lib.GRAPH_QUANT_PARAMS, _lib.GRAPH_CONV_Q8]


def test_one_quant_params_per_input_view_and_its_lifetime():
    rng = np.random.default_rng(3)
    g = Graph(tq.quantise(small_block(rng)))
    plan = tg.build_plan(g)
    kinds = [o.kind for o in plan.ops]
    assert kinds.count(_lib.GRAPH_CONV_Q8) == 5 and kinds.count(_lib.GRAPH_QUANT_PARAMS) == 2 and not plan.copies()
    cat = g.ops[2]["outputs"][0]
    qp = [k for k, o in enumerate(plan.ops) if o.kind == _lib.GRAPH_QUANT_PARAMS and o.in0 == cat]
    assert len(qp) == 1
    qp = qp[0]
    producers = [k for k, o in enumerate(plan.ops) if plan.tensors[o.out].storage == cat and o.kind == _lib.GRAPH_CONV_Q8]
    consumers = [k for k, o in enumerate(plan.ops) if o.kind == _lib.GRAPH_CONV_Q8 and o.in0 == cat]
    assert len(producers) == 2 and len(consumers) == 3
    assert max(producers) < qp < min(consumers)
    ptid = plan.ops[qp].out
    assert all(plan.ops[k].in1 == ptid for k in consumers)
    p = plan.tensors[ptid]
    assert (p.H, p.W, p.C, p.c_offset, p.c_stride) == (1, 1, 4, 0, 4)
    assert plan.lifetimes[ptid] == (qp, max(consumers))
    # the arena: no two tensors that are live at the same operator overlap
    spans = []
    for s, (a, b) in plan.lifetimes.items():
        t = plan.tensors[s]
        if not t.external:
            spans.append((t.arena_offset, t.arena_offset + t.H * t.W * t.C, a, b, s))
    assert any(s == ptid for *_, s in spans)
    for i, (o0, e0, a0, b0, s0) in enumerate(spans):
        for o1, e1, a1, b1, s1 in spans[i + 1:]:
            if not (b0 < a1 or b1 < a0):
                assert e0 <= o1 or e1 <= o0, (s0, s1)


def test_symmetric_and_asymmetric_dense_get_their_own_parameters():
    rng = np.random.default_rng(4)
    m = tq.ModelQ8()
    x = m.tensor([1, 1, 1, 64], name="input")
    m.inputs = [x]
    flat = m.reshape(m.unary("RELU", x), [1, 64])
    q = rng.integers(-127, 128, size=(20, 64)).astype(np.int8)
    a = m.dense_q8(flat, m.qfilter(q, [0.01]), np.zeros(20, np.float32), asymmetric=True)
    b = m.dense_q8(flat, m.qfilter(q, [0.02]), np.ones(20, np.float32), asymmetric=False)
    m.outputs = [m.binary("ADD", a, b)]
    plan = tg.build_plan(Graph(m.finish()))
    qps = [o for o in plan.ops if o.kind == _lib.GRAPH_QUANT_PARAMS]
    assert sorted(o.param for o in qps) == [0.0, 1.0]
    fcs = [o for o in plan.ops if o.kind == _lib.GRAPH_FC_Q8]
    assert [next(q.param for q in qps if q.out == o.in1) for o in fcs] == [0.0, 1.0]
    assert np.array_equal(fcs[1].scale, np.full(20, 0.02, np.float32)) and np.array_equal(fcs[1].shift, np.ones(20, np.float32))


def test_mul_add_fold_into_a_q8_convolution():
    rng = np.random.default_rng(5)
    m = tq.ModelQ8()
    x = m.tensor([1, 9, 9, 32], name="input")
    m.inputs = [x]
    q = rng.integers(-127, 128, size=(48, 3, 3, 32)).astype(np.int8)
    fs = rng.uniform(1e-3, 1e-2, size=48).astype(np.float32)
    bias = rng.normal(0, 0.05, size=48).astype(np.float32)
    mul = rng.uniform(0.5, 2.0, size=48).astype(np.float32)
    add = rng.normal(0, 1.0, size=48).astype(np.float32)
    y = m.conv_q8(x, m.qfilter(q, fs), bias)
    m.outputs = [m.binary("ADD", m.binary("MUL", y, mul), add, tb.RELU)]
    plan = tg.build_plan(Graph(m.finish()))
    assert [o.name for o in plan.ops] == ["QUANT_PARAMS", "CONV_2D+MUL+ADD"]
    o = plan.ops[1]
    assert o.kind == _lib.GRAPH_CONV_Q8 and o.act == tb.RELU
    assert o.scale.dtype == np.float32 and np.array_equal(o.scale, (fs * mul).astype(np.float32))
    assert np.array_equal(o.shift, (bias * mul + add).astype(np.float32))


@pytest.mark.parametrize("shape", [(40, 1, 1, 64), (48, 3, 3, 36), (5, 1, 7, 130), (33, 2, 5, 3)])
def test_filter_layout_round_trips_and_wsum_is_the_integer_sum(shape):
    rng = np.random.default_rng(sum(shape))
    w = rng.integers(-128, 128, size=shape).astype(np.int8)
    packed = tg.pack_conv_filter_q8(w)
    co, kh, kw, ci = shape
    nch, nt = -(-ci // _lib.GRAPH_CONV_Q8_KC), -(-co // _lib.GRAPH_CONV_CO)
    assert packed.dtype == np.uint8 and packed.size == kh * kw * nch * nt * 1024 + 4 * nt * 32
    back, wsum = tg.unpack_conv_filter_q8(packed, shape)
    assert np.array_equal(back, w)
    assert np.array_equal(wsum, w.reshape(co, -1).astype(np.int64).sum(axis=1))
    # the fragment order, restated: lane l of tile t at step (tap, chunk) holds channel 32 t + (l & 31), k = 16 (l >> 5) + j
    frag = packed[:packed.size - 4 * nt * 32].view(np.int8).reshape(kh * kw, nch, nt, 64, 16)
    for tap, chunk, t, lane, j in [(0, 0, 0, 0, 0), (kh * kw - 1, nch - 1, nt - 1, 37, 5), (0, nch - 1, 0, 63, 15)]:
        c, k = 32 * t + (lane & 31), 32 * chunk + 16 * (lane >> 5) + j
        want = w.reshape(co, kh * kw, ci)[c, tap, k] if c < co and k < ci else 0
        assert frag[tap, chunk, t, lane, j] == want
    fc = rng.integers(-128, 128, size=(7, 50)).astype(np.int8)
    p = tg.pack_fc_filter_q8(fc)
    assert p.size == 7 * 52 + 4 * 7
    assert np.array_equal(p[:7 * 52].view(np.int8).reshape(7, 52)[:, :50], fc) and not p[:7 * 52].reshape(7, 52)[:, 50:].any()
    assert np.array_equal(p[7 * 52:].view(np.int32), fc.astype(np.int64).sum(axis=1))


def test_describe_prints_the_hybrid_census(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(6)
    blob = tq.quantise(small_block(rng))
    (tmp_path / "q8.tflite").write_bytes(blob)
    g = Graph(blob)
    n8 = sum(int(np.prod(g.quantised_filter(op)["shape"])) for op in g.ops if g.quantised_filter(op) is not None)
    r = subprocess.run([sys.executable, os.path.join(repo, "tools", "tflite_to_npz.py"), "--describe", str(tmp_path / "q8.tflite")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "QUANT_PARAMS: 2" in r.stdout
    assert "hybrid operators (int8 filter, activations quantised per sample): 5; int8 weight bytes: %d, float32 weight bytes: 0" % n8 \
        in r.stdout


def refusal(m):
    g = Graph(m.finish())
    with pytest.raises(NotImplementedError) as e:
        tg.build_plan(g)
    return str(e.value)


def test_refusals_name_the_operator_and_index():
    rng = np.random.default_rng(7)
    q = rng.integers(-127, 128, size=(40, 1, 1, 32)).astype(np.int8)

    def start():
        m = tq.ModelQ8()
        x = m.tensor([1, 8, 8, 32], name="input")
        m.inputs = [x]
        return m, m.unary("RELU", x)

    # a quantised activation: INT8 and UINT8
    for ttype, tname in ((tq.INT8, "INT8"), (tb.UINT8, "UINT8")):
        m, y = start()
        z = m.tensor([1, 8, 8, 32], ttype=ttype, name="quantised")
        m.op("ADD", [y, y], [z], {0: ("b", 0)})
        m.outputs = [z]
        msg = refusal(m)
        assert "ADD" in msg and "operator 1" in msg and tname in msg
    # a UINT8 and an INT16 filter
    for ttype, tname in ((tb.UINT8, "UINT8"), (tq.INT16, "INT16")):
        m, y = start()
        m.outputs = [m.conv_q8(y, m.qfilter(np.abs(q), np.full(40, 0.01), ttype=ttype), np.zeros(40, np.float32))]
        msg = refusal(m)
        assert "CONV_2D" in msg and "operator 1" in msg and tname in msg
    # a non-zero filter zero point
    m, y = start()
    zp = np.zeros(40, np.int64)
    zp[17] = 3
    m.outputs = [m.conv_q8(y, m.qfilter(q, np.full(40, 0.01), zero_point=zp), np.zeros(40, np.float32))]
    msg = refusal(m)
    assert "CONV_2D" in msg and "operator 1" in msg and "zero point" in msg
    # scales along another dimension; a number of scales that is neither 1 nor Cout
    m, y = start()
    m.outputs = [m.conv_q8(y, m.qfilter(q, np.full(32, 0.01), dim=3), np.zeros(40, np.float32))]
    msg = refusal(m)
    assert "CONV_2D" in msg and "operator 1" in msg and "dimension 3" in msg
    m, y = start()
    m.outputs = [m.conv_q8(y, m.qfilter(q, np.full(5, 0.01)), np.zeros(40, np.float32))]
    msg = refusal(m)
    assert "CONV_2D" in msg and "operator 1" in msg and "5 scales" in msg
    # an INT8 bias
    m, y = start()
    b = m.tensor([40], np.zeros(40, np.int8), "bias_q8", tq.INT8, quant=([0.01], [0], 0))
    m.outputs = [m.conv_q8(y, m.qfilter(q, np.full(40, 0.01)), b)]
    msg = refusal(m)
    assert "CONV_2D" in msg and "operator 1" in msg and "INT8" in msg and "bias_q8" in msg
    # an INT8 filter of a dense layer whose bias is fine, but on an operator that takes no INT8 constant
    m, y = start()
    z = m.tensor([1, 8, 8, 32])
    m.op("MUL", [y, m.tensor([32], np.ones(32, np.int8), "mul_q8", tq.INT8, quant=([0.01], [0], 0))], [z], {0: ("b", 0)})
    m.outputs = [z]
    msg = refusal(m)
    assert "MUL" in msg and "operator 1" in msg and "INT8" in msg
    # DEQUANTIZE / QUANTIZE
    for code, name in ((6, "DEQUANTIZE"), (114, "QUANTIZE")):
        m, y = start()
        z = m.tensor([1, 8, 8, 32])
        m.op("ADD", [y], [z], None, code=code)
        m.outputs = [z]
        msg = refusal(m)
        assert name in msg and "operator 1" in msg


def test_a_sum_that_could_overflow_int32_is_refused():
    # 7 * 7 * 1354 * 127 * 255 >= 2^31 > 7 * 7 * 1353 * 127 * 255
    for cin, refused in ((1353, False), (1354, True)):
        m = tq.ModelQ8()
        x = m.tensor([1, 8, 8, cin], name="input")
        m.inputs = [x]
        y = m.unary("RELU", x)
        m.outputs = [m.conv_q8(y, m.qfilter(np.ones((4, 7, 7, cin), np.int8), np.full(4, 0.01)), np.zeros(4, np.float32))]
        assert (7 * 7 * cin * 127 * 255 >= 2 ** 31) == refused
        if refused:
            msg = refusal(m)
            assert "CONV_2D" in msg and "operator 1" in msg and "int32" in msg
        else:
            tg.build_plan(Graph(m.finish()))


def test_wrresnet_walk_refuses_a_quantised_filter_by_name():
    rng = np.random.default_rng(8)
    m = tq.ModelQ8()
    x = m.tensor([1, 8, 8, 32], name="input")
    m.inputs = [x]
    q = rng.integers(-127, 128, size=(40, 1, 1, 32)).astype(np.int8)
    m.outputs = [m.conv_q8(x, m.qfilter(q, np.full(40, 0.01), name="conv1_q8"), np.zeros(40, np.float32))]
    with pytest.raises(NotImplementedError, match="conv1_q8"):
        convert(Graph(m.finish()))


def test_a_float32_plan_is_unchanged():
    """The float32 path through the new planner: the operators and the arena it planned before there was a quantised
    mode (their count, the checksum of their names and the arena size are recorded from that planner), and the same
    through both modes."""
    import zlib

    blob = tb.inception_v3(6, (16,), seed=1, width=0.25)
    g = Graph(blob)
    assert all(t["quant"] is None for t in g.tensors) and not any(g.quantised_filter(op) for op in g.ops)
    plans = [tg.build_plan(g), tg.build_plan(g, quantised_math="float")]
    for plan in plans:
        assert not any(o.kind in tg.Q8_KINDS + (_lib.GRAPH_QUANT_PARAMS,) for o in plan.ops)
        census = plan.census()
        assert census["CONV_2D"] == 94 and census["FULLY_CONNECTED"] == 2 and "QUANT_PARAMS" not in census
    assert (len(plans[0].ops), plans[0].arena_floats) == (111, 142344)
    assert zlib.crc32(" ".join(o.name for o in plans[0].ops).encode()) == 2279996077
    assert [o.name for o in plans[0].ops] == [o.name for o in plans[1].ops]
    assert plans[0].arena_floats == plans[1].arena_floats
    for a, b in zip(plans[0].ops, plans[1].ops):
        assert (a.kind, a.in0, a.in1, a.out) == (b.kind, b.in0, b.in1, b.out)
        if a.weights is not None:
            assert a.weights.dtype == np.float32 and np.array_equal(a.weights, b.weights)
    # the quantised twin of the same file keeps the float plan's shapes and adds only parameter tensors
    gq = Graph(tq.quantise(blob))
    pq = tg.build_plan(gq)
    assert pq.output_shape == plans[0].output_shape and pq.input_shape == plans[0].input_shape
    assert [o.name for o in pq.ops if o.kind != _lib.GRAPH_QUANT_PARAMS] == [o.name for o in plans[0].ops]
