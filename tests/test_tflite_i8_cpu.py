"""The planner's side of full-integer TFLite graphs (cpx/ml_tools/tflite_graph_i8.py, tflite_reader.check_executable(integer=
True)): the kinds and the census of whole networks, the arena in bytes, the window folds, the SOFTMAX lowering, every
refusal by operator name and index, and the float16-weight fold.  No GPU."""
import numpy as np
import pytest

import tflite_build as tb
import tflite_build_i8 as ti
import tflite_build_q8 as tq
import tflite_eval_i8 as te8
import tflite_plan_digest as tpd
from cpx import _lib
from cpx.ml_tools import tflite_graph as tg
from cpx.ml_tools import tflite_graph_i8 as tgi
from cpx.ml_tools.tflite_reader import Graph

NAMES = {getattr(_lib, "GRAPH_" + k): k for k in ("QUANTIZE", "DEQUANTIZE", "CONV_I8", "CONV_I8_GROUPED", "DWCONV_I8", "FC_I8", "ADD_I8",
                                                  "MUL_I8", "MAX_POOL_I8", "AVG_POOL_I8", "MEAN_I8", "SLICE", "SOFTMAX", "LOGISTIC")}
QP = (np.float32(0.05), 3)


def plan_of(blob, **options):
    return tg.build_plan(Graph(blob), integer_activations=True, grouped_convolutions=True, **options)


def kinds(plan):
    return [NAMES.get(o.kind, "float:" + o.name) for o in plan.ops]


def count(plan):
    out = {}
    for k in kinds(plan):
        out[k] = out.get(k, 0) + 1
    return out


def refusal(blob, **options):
    with pytest.raises(NotImplementedError) as e:
        plan_of(blob, **options)
    return str(e.value)


def wrresnet_blobs():
    from cpx.ml_tools import wrresnet as wr

    blob = tb.wrresnet(wr.random_weights(17, seed=5), size=32)
    return blob, ti.quantise_full(blob, np.random.default_rng(5).normal(0, 1, size=(4, 32, 32, 2)))


def inception_block():
    """1 x 1 | 1 x 1 -> 3 x 3 | AVERAGE_POOL -> 1 x 1 | MAX_POOL, concatenated, and a 1 x 1 convolution behind: three
    producers write into the concatenation, the max pool's output too."""
    rng = np.random.default_rng(3)
    m = tb.Model()

    def cbn(x, co, k):
        cin = m.shape(x)[3]
        return m.conv(x, rng.normal(0, np.sqrt(2.0 / (k * k * cin)), size=(co, k, k, cin)).astype(np.float32),
                      rng.normal(0, 0.05, size=co).astype(np.float32), 1, tb.SAME, tb.RELU)

    x = m.tensor([1, 9, 9, 16], name="input")
    m.inputs = [x]
    stem = cbn(x, 16, 1)
    cat = m.concat([cbn(stem, 8, 1), cbn(cbn(stem, 8, 1), 12, 3), cbn(m.pool("AVERAGE_POOL_2D", stem, 3, 1, tb.SAME), 8, 1),
                    m.pool("MAX_POOL_2D", stem, 3, 1, tb.SAME)])
    m.outputs = [cbn(cat, 10, 1)]
    return m.finish()


# ---- kinds, census, arena ----
def test_wrresnet_plan_and_arena():
    blob, q = wrresnet_blobs()
    plan = plan_of(q)
    assert count(plan) == {"QUANTIZE": 1, "CONV_I8_GROUPED": 22, "MUL_I8": 10, "ADD_I8": 19, "MEAN_I8": 1, "FC_I8": 1, "DEQUANTIZE": 1,
                           "LOGISTIC": 1}
    assert kinds(plan)[:4] == ["QUANTIZE", "CONV_I8_GROUPED", "MUL_I8", "ADD_I8"] and kinds(plan)[-3:] == ["FC_I8", "DEQUANTIZE", "LOGISTIC"]
    f32 = tg.build_plan(Graph(blob), grouped_convolutions=True)
    print("arena bytes per sample: int8 %d, float32 %d" % (plan.arena_bytes_per_sample, f32.arena_bytes_per_sample))
    assert plan.arena_bytes_per_sample * 3 < f32.arena_bytes_per_sample
    types = {t.dtype for t in plan.tensors.values()}
    assert types == {"int8", "float32"}
    assert all(t.scale is not None and -128 <= t.zero_point <= 127 for t in plan.tensors.values() if t.dtype == "int8")
    # a BatchNorm behind a residual ADD: MUL and ADD by INT8 constants, the constant as bytes in `weights`
    mul = next(o for o in plan.ops if o.kind == _lib.GRAPH_MUL_I8)
    assert mul.in1 == -1 and mul.weights.dtype == np.uint8 and mul.weights.size == plan.tensors[mul.in0].C


def test_mobilenet_block_plan_and_pad_fold():
    blob = ti.mobilenet_v2_blocks(5, size=48)
    q = ti.quantise_full(blob, np.random.default_rng(6).normal(0, 1, size=(4, 48, 48, 3)))
    plain, folded = plan_of(q), plan_of(q, fold_windows=True)
    assert count(plain) == {"QUANTIZE": 1, "CONV_I8": 7, "DWCONV_I8": 3, "ADD_I8": 2, "SLICE": 1, "MEAN_I8": 1, "FC_I8": 1, "DEQUANTIZE": 1,
                            "SOFTMAX": 1}
    assert count(folded) == {k: v for k, v in count(plain).items() if k != "SLICE"} and len(folded.ops) == len(plain.ops) - 1
    pad = next(o for o in plain.ops if o.kind == _lib.GRAPH_SLICE)
    dw = next(o for o in folded.ops if o.name == "PAD>DEPTHWISE_CONV_2D")
    assert pad.name == "PAD" and pad.pads[:2] == (0, 0) and dw.pads == (0, 0, 1, 1) and dw.kind == _lib.GRAPH_DWCONV_I8
    # the zero point the SLICE fills with is its tensor's
    assert tgi.unpack_header(pad.shift)[_lib.GRAPH_I8_HDR_Z_IN] == plain.tensors[pad.out].zero_point
    f32 = tg.build_plan(Graph(blob))
    assert plain.arena_bytes_per_sample * 3 < f32.arena_bytes_per_sample


def test_inception_block_concatenation():
    blob = inception_block()
    q = ti.quantise_full(blob, np.random.default_rng(7).normal(0, 1, size=(4, 9, 9, 16)))
    plan = plan_of(q)
    assert count(plan) == {"QUANTIZE": 1, "CONV_I8": 6, "AVG_POOL_I8": 1, "MAX_POOL_I8": 1, "DEQUANTIZE": 1}
    assert not plan.copies()   # every part is written in place
    g = Graph(q)
    cat = next(op for op in g.ops if op["name"] == "CONCATENATION")
    offs = [plan.tensors[t].c_offset for t in cat["inputs"]]
    assert offs == [0, 8, 20, 28] and all(plan.tensors[t].c_stride == 44 and plan.tensors[t].dtype == "int8" for t in cat["inputs"])
    # the graph's restatement runs on it (the pools' and the concatenation's parameters are equal)
    x = np.random.default_rng(8).normal(0, 1, size=(2, 9, 9, 16)).astype(np.float32)
    assert te8.evaluate(g, x)[g.outputs[0]].shape == (2, 9, 9, 10)


def test_softmax_lowers_to_three_launches():
    blob = ti.mobilenet_v2_blocks(5, size=48)
    q = ti.quantise_full(blob, np.random.default_rng(6).normal(0, 1, size=(4, 48, 48, 3)), float_tail=False)
    plan = plan_of(q)
    assert kinds(plan)[-5:] == ["FC_I8", "DEQUANTIZE", "SOFTMAX", "QUANTIZE", "DEQUANTIZE"]
    quant = plan.ops[-2]
    assert quant.param == float(np.float32(1.0 / 256.0)) and tgi.unpack_header(quant.shift)[_lib.GRAPH_I8_HDR_Z_OUT] == -128


def test_the_default_plan_still_refuses_with_todays_text():
    _, q = wrresnet_blobs()
    with pytest.raises(NotImplementedError) as e:
        tg.build_plan(Graph(q), grouped_convolutions=True)
    assert str(e.value).startswith("operator 0 (QUANTIZE) is not in the set the graph executor runs: ADD, AVERAGE_POOL_2D, ")
    assert "QUANTIZE" not in str(e.value).split(":", 1)[1]
    # without its QUANTIZE the first INT8 activation stops it, as ever
    m = tq.ModelQ8()
    x = m.tensor([1, 8, 8, 32], name="input")
    m.inputs = [x]
    z = m.tensor([1, 8, 8, 32], ttype=tq.INT8, name="quantised", quant=([0.1], [0], 0))
    m.op("RELU", [x], [z], None)
    m.outputs = [z]
    with pytest.raises(NotImplementedError) as e:
        tg.build_plan(Graph(m.finish()))
    assert str(e.value) == "operator 0 (RELU): tensor 'quantised' has type INT8, only float32 graphs are run"


def test_headers_carry_the_issues_integers():
    """One ADD by hand: s1 = 0.5, s2 = 0.25, s_out = 1: twice = 1, m1 = QM(0.5), m2 = QM(0.25), mo = QM(2^-20)."""
    m, q = ti.start([1, 4, 4, 8], (np.float32(0.5), 1))
    b = m.quantize(q, (np.float32(0.25), -2))
    y = m.binary_i8("ADD", q, b, (np.float32(1.0), 7), tb.RELU6)
    plan = plan_of(ti.finish(m, y))
    h = tgi.unpack_header(plan.ops[2].shift)
    H = {k: int(h[getattr(_lib, "GRAPH_I8_HDR_" + k)]) for k in ("Z_IN", "Z_IN1", "Z_OUT", "LO", "HI", "M0", "S0", "M1", "S1", "MO", "SO", "LEFT")}
    assert H == dict(Z_IN=1, Z_IN1=-2, Z_OUT=7, LO=7, HI=13, M0=2 ** 30, S0=0, M1=2 ** 30, S1=-1, MO=2 ** 30, SO=-19, LEFT=20)
    rq = tgi.unpack_header(plan.ops[1].shift)
    assert (rq[_lib.GRAPH_I8_HDR_M0], rq[_lib.GRAPH_I8_HDR_S0]) == (2 ** 30, 2)   # 0.5 / 0.25


# ---- refusals, by operator name and index ----
def test_refusals():
    rng = np.random.default_rng(9)
    w = rng.integers(-127, 128, size=(8, 1, 1, 8)).astype(np.int8)
    ws = np.full(8, 0.01, np.float32)

    def conv(m, x, **kw):
        return m.conv_i8(x, w, ws, np.zeros(8, np.int32), (np.float32(0.1), 0), **kw)

    # UINT8 and INT16 activations
    for ttype, tname in ((tb.UINT8, "UINT8"), (tq.INT16, "INT16")):
        m, q = ti.start([1, 4, 4, 8], QP)
        y = conv(m, q)
        shape, _, bi, name = m.tensors[y]
        m.tensors[y] = (shape, ttype, bi, name)
        msg = refusal(ti.finish(m, y))
        assert "operator 1 (CONV_2D)" in msg and tname in msg
    # a per-channel quantised activation
    m, q = ti.start([1, 4, 4, 8], QP)
    y = conv(m, q)
    m.quant[y] = ([0.1] * 8, [0] * 8, 3)
    msg = refusal(ti.finish(m, y))
    assert "operator 1 (CONV_2D)" in msg and "per-channel" in msg
    # an INT8 graph input; an INT8 graph output
    m = ti.ModelI8()
    x = m.qact([1, 4, 4, 8], QP, "input")
    m.inputs = [x]
    msg = refusal(ti.finish(m, conv(m, x)))
    assert "operator 0 (CONV_2D)" in msg and "input" in msg and "INT8" in msg
    m, q = ti.start([1, 4, 4, 8], QP)
    m.outputs = [conv(m, q)]
    msg = refusal(m.finish())
    assert "operator 1 (CONV_2D)" in msg and "output" in msg and "INT8" in msg
    # an asymmetric filter
    m, q = ti.start([1, 4, 4, 8], QP)
    wt = m.qfilter(w, ws, zero_point=np.array([0, 0, 0, 2, 0, 0, 0, 0]))
    y = m.qact([1, 0, 0, 8], (np.float32(0.1), 0))
    m.op("CONV_2D", [q, wt], [y], {0: ("b", 0), 1: ("i", 1), 2: ("i", 1), 3: ("b", 0), 4: ("i", 1), 5: ("i", 1)})
    msg = refusal(ti.finish(m, y))
    assert "operator 1 (CONV_2D)" in msg and "zero point" in msg
    # a float32 bias on an INT8 convolution
    m, q = ti.start([1, 4, 4, 8], QP)
    y = m.qact([1, 0, 0, 8], (np.float32(0.1), 0))
    m.op("CONV_2D", [q, m.qfilter(w, ws), m.tensor([8], np.zeros(8, np.float32))], [y],
         {0: ("b", 0), 1: ("i", 1), 2: ("i", 1), 3: ("b", 0), 4: ("i", 1), 5: ("i", 1)})
    msg = refusal(ti.finish(m, y))
    assert "operator 1 (CONV_2D)" in msg and "INT32" in msg
    # a [1, 1, C] gate MUL on INT8
    m, q = ti.start([1, 4, 4, 8], QP)
    gate = m.mean_i8(q, QP, keep_dims=True)
    msg = refusal(ti.finish(m, m.binary_i8("MUL", q, gate, QP)))
    assert "operator 2 (MUL)" in msg and "[1, 1, C]" in msg
    # an INT8 DIV
    m, q = ti.start([1, 4, 4, 8], QP)
    tb.CODES.setdefault("DIV", 42)
    msg = refusal(ti.finish(m, m.binary_i8("DIV", q, q, QP)))
    assert "operator 1 (DIV)" in msg and "division" in msg
    # HARD_SWISH
    m, q = ti.start([1, 4, 4, 8], QP)
    y = m.qact([1, 4, 4, 8], QP)
    m.op("RELU", [q], [y], None, code=117)
    msg = refusal(ti.finish(m, y))
    assert "operator 1 (HARD_SWISH)" in msg
    # a constant minus an activation
    m, q = ti.start([1, 4, 4, 8], QP)
    msg = refusal(ti.finish(m, m.binary_i8("SUB", q, m.qconst(np.ones(8, np.int8), QP), QP, const_first=True)))
    assert "operator 1 (SUB)" in msg and "c - x" in msg
    # pools, PAD and CONCATENATION whose parameters differ
    other = (np.float32(0.06), 3)
    for kind in ("MAX_POOL_2D", "AVERAGE_POOL_2D"):
        m, q = ti.start([1, 4, 4, 8], QP)
        msg = refusal(ti.finish(m, m.pool_i8(kind, q, 2, 2, tb.VALID, qp=other)))
        assert "operator 1 (%s)" % kind in msg and "different quantisation parameters" in msg
    m, q = ti.start([1, 4, 4, 8], QP)
    msg = refusal(ti.finish(m, m.pad_i8(q, [[0, 0], [1, 1], [1, 1], [0, 0]], qp=(QP[0], 4))))
    assert "operator 1 (PAD)" in msg and "different quantisation parameters" in msg
    m, q = ti.start([1, 4, 4, 8], QP)
    msg = refusal(ti.finish(m, m.concat_i8([q, m.quantize(q, other)])))
    assert "operator 2 (CONCATENATION)" in msg and "different quantisation parameters" in msg
    # a mixed operator: only QUANTIZE and DEQUANTIZE change the type
    m, q = ti.start([1, 4, 4, 8], QP)
    y = m.unary("RELU", q)
    m.outputs = [y]
    msg = refusal(m.finish())
    assert "operator 1 (RELU)" in msg and "mixes" in msg


def test_multiplier_refusals():
    w = np.ones((8, 1, 1, 8), np.int8)
    # a scale that is not above 0
    m, q = ti.start([1, 4, 4, 8], QP)
    y = m.conv_i8(q, w, np.full(8, 0.01, np.float32), None, (np.float32(0.0), 0))
    msg = refusal(ti.finish(m, y))
    assert "operator 1 (CONV_2D)" in msg and "not above 0" in msg
    # a multiplier that needs a left shift above 30
    m, q = ti.start([1, 4, 4, 8], QP)
    msg = refusal(ti.finish(m, m.quantize(q, (np.float32(1e-11), 0))))
    assert "operator 1 (QUANTIZE)" in msg and "above 30" in msg
    # |x| * 2^left reaches 2^31: a requantisation by 2^24 of up to 255
    m, q = ti.start([1, 4, 4, 8], (np.float32(2.0 ** 24), 0))
    msg = refusal(ti.finish(m, m.quantize(q, (np.float32(1.0), 0))))
    assert "operator 1 (QUANTIZE)" in msg and "overflow int32" in msg
    # ADD's output multiplier must be below 1: twice / (2^20 s_out) with a tiny output scale
    m, q = ti.start([1, 4, 4, 8], QP)
    msg = refusal(ti.finish(m, m.binary_i8("ADD", q, q, (np.float32(1e-8), 0))))
    assert "operator 1 (ADD)" in msg and "below 1" in msg
    # K * 255 * 127 + max |bias| below 2^31
    for bias, refused in ((2 ** 31 - 8 * 255 * 127, True), (2 ** 31 - 1 - 8 * 255 * 127, False)):
        m, q = ti.start([1, 4, 4, 8], QP)
        y = m.conv_i8(q, w, np.full(8, 1e-9, np.float32), np.full(8, bias, np.int32), (np.float32(1.0), 0))
        if refused:
            msg = refusal(ti.finish(m, y))
            assert "operator 1 (CONV_2D)" in msg and "int32" in msg
        else:
            plan_of(ti.finish(m, y))


# ---- float16-weight files ----
def _float16_file(blob):
    """The converter's float16 mode of a float32 flatbuffer: every float32 constant becomes a FLOAT16 tensor (appended, so
    that no tensor id moves) behind a DEQUANTIZE in front of the graph's operators."""
    g = Graph(blob)
    m = tq.ModelQ8()
    halves = {}
    for k, t in enumerate(g.tensors):
        if t["const"] is not None and t["type"] == 0:
            m.tensor(t["shape"], None, t["name"] or "t")
            halves[k] = np.asarray(t["const"], np.float16)
        else:
            m.tensor(t["shape"], t["const"], t["name"] or "t", t["type"])
    for k, h in halves.items():
        m.buffers.append(h.astype("<f2").tobytes())
        m.tensors.append((list(h.shape), 1, len(m.buffers) - 1, "half_%d" % k))
        m.op("DEQUANTIZE", [len(m.tensors) - 1], [k], None, code=ti.DEQUANTIZE)
    from tflite_build_dw import _options

    for op in g.ops:
        m.op(op["name"], op["inputs"], op["outputs"], _options(op))
    m.inputs, m.outputs = list(g.inputs), list(g.outputs)
    return m.finish(), halves


def _rounded_file(blob, halves):
    g = Graph(blob)
    m = tq.ModelQ8()
    for k, t in enumerate(g.tensors):
        m.tensor(t["shape"], halves[k].astype(np.float32) if k in halves else t["const"], t["name"] or "t", t["type"])
    from tflite_build_dw import _options

    for op in g.ops:
        m.op(op["name"], op["inputs"], op["outputs"], _options(op))
    m.inputs, m.outputs = list(g.inputs), list(g.outputs)
    return m.finish()


def test_float16_weight_file_plans_as_the_rounded_float32_file():
    blob = ti.mobilenet_v2_blocks(5, size=48)
    f16, halves = _float16_file(blob)
    assert len(halves) > 20
    g16, g32 = Graph(f16), Graph(_rounded_file(blob, halves))
    assert [op["name"] for op in g16.ops] == [op["name"] for op in g32.ops]   # the DEQUANTIZEs are folded on load
    for options in ({}, dict(fold_windows=True, fuse_preactivation=True)):
        assert tpd.digest(tg.build_plan(g16, **options)) == tpd.digest(tg.build_plan(g32, **options))
    # and it is the fp16-rounded weights, not the originals
    assert tpd.digest(tg.build_plan(g16)) != tpd.digest(tg.build_plan(Graph(blob)))
