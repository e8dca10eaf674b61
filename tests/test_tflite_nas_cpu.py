"""STRIDED_SLICE / SLICE through the reader, the window folds and the depthwise pre-activation through the planner, the
NASNet stand-in and an inceptionresnetv2 block: host work, no GPU.  The flatbuffers come from tests/tflite_build_nas.py
(a structural stand-in for the converter's layout of a NASNet, see there)."""
import json

import numpy as np
import pytest
import torch

import tflite_build as tb
import tflite_build_dw as td
import tflite_build_nas as tn
import tflite_build_preact as tp
import tflite_build_se as ts
import tflite_eval_nas as ten

from cpx import _lib
from cpx.ml_tools.tflite_graph import build_plan
from cpx.ml_tools.tflite_reader import Graph

F32 = np.float32
FOLDS = dict(fold_windows=True, fuse_preactivation_dw=True)


def model(shape=(1, 7, 6, 5)):
    m = tn.ModelNAS()
    x = m.tensor(list(shape), name="input")
    m.inputs = [x]
    return m, x


def finish(m, y):
    m.outputs = [y]
    return Graph(m.finish())


# ---- 1. the reader against NumPy ----
X = np.arange(1 * 7 * 6 * 5, dtype=F32).reshape(1, 7, 6, 5)
SPECS = {
    "masks": (lambda m, x: m.strided_slice(x, [0, 1, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1], begin_mask=0b1001, end_mask=0b1111),
              X[:, 1:, 1:, :]),
    "explicit_ends": (lambda m, x: m.strided_slice(x, [0, 1, 1, 0], [1, 7, 6, 5], [1, 1, 1, 1]), X[:, 1:7, 1:6, :]),
    "negative": (lambda m, x: m.strided_slice(x, [0, -5, -4, 0], [1, -1, -2, 5], [1, 1, 1, 1]), X[:, -5:-1, -4:-2, :]),
    "stride2": (lambda m, x: m.strided_slice(x, [0, 0, 0, 0], [0, 0, 0, 0], [1, 2, 2, 1], begin_mask=15, end_mask=15), X[:, ::2, ::2, :]),
    "stride3_from_1": (lambda m, x: m.strided_slice(x, [0, 1, 2, 0], [1, 7, 6, 5], [1, 3, 2, 1]), X[:, 1:7:3, 2:6:2, :]),
    "clamped_end": (lambda m, x: m.strided_slice(x, [0, 2, -100, 0], [1, 100, 4, 5], [1, 1, 1, 1]), X[:, 2:100, -100:4, :]),
    "slice_to_the_end": (lambda m, x: m.slice(x, [0, 1, 1, 0], [-1, -1, -1, -1]), X[:, 1:, 1:, :]),
    "slice_sizes": (lambda m, x: m.slice(x, [0, 2, 0, 0], [1, 3, 4, 5]), X[:, 2:5, 0:4, :]),
}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_resolved_slice_reproduces_numpy(name):
    build, want = SPECS[name]
    m, x = model()
    g = finish(m, build(m, x))
    g.check_executable()
    op = g.ops[0]
    assert op["name"] in ("STRIDED_SLICE", "SLICE") and op["code"] in (45, 65)
    form = op["slice"]
    assert len(form) == 4 and form[0] == (0, 1, 1) and form[3] == (0, 1, 5)
    got = X[np.ix_(*[b + s * np.arange(n) for b, s, n in form])]
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(ten.evaluate(g, X, dtype=torch.float32)[g.outputs[0]], want)
    # ... and the planner's operator: the start as a negative pad, the bottom / right pads what the size implies
    plan = build_plan(g)
    (o,) = plan.ops
    assert o.kind == _lib.GRAPH_SLICE == 20 and plan.output_shape == want.shape[1:]
    assert (o.pads[0], o.pads[1], o.stride_h, o.stride_w) == (-form[1][0], -form[2][0], form[1][1], form[2][1])
    assert max(o.pads) <= 0 and (o.kh, o.kw, o.act) == (1, 1, 0)
    assert want.shape[1] == (7 + o.pads[0] + o.pads[2] - 1) // o.stride_h + 1 and want.shape[2] == (6 + o.pads[1] + o.pads[3] - 1) // o.stride_w + 1


def test_strided_slice_options_are_read():
    m, x = model()
    g = finish(m, m.strided_slice(x, [0, 1, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1], begin_mask=9, end_mask=15, ellipsis_mask=2,
                                  new_axis_mask=4, shrink_axis_mask=1, offset=True))
    op = g.ops[0]
    assert [op[k] for k in ("begin_mask", "end_mask", "ellipsis_mask", "new_axis_mask", "shrink_axis_mask", "offset")] == [9, 15, 2, 4, 1, True]
    assert (op["begin"], op["end"], op["strides"]) == ([0, 1, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]) and op["slice"] is None


# ---- 2. refusals ----
def _runtime_index(m):
    return m.tensor([4], None, "runtime_index", tb.INT32)


REFUSALS = {
    "begin_not_constant": (lambda m, x: m.strided_slice(x, _runtime_index(m), [0] * 4, [1] * 4, end_mask=15),
                           r"operator 0 \(STRIDED_SLICE\): begin is not a constant"),
    "end_not_constant": (lambda m, x: m.strided_slice(x, [0] * 4, _runtime_index(m), [1] * 4), r"operator 0 \(STRIDED_SLICE\): end is not a constant"),
    "strides_not_constant": (lambda m, x: m.strided_slice(x, [0] * 4, [0] * 4, _runtime_index(m), end_mask=15),
                             r"operator 0 \(STRIDED_SLICE\): strides is not a constant"),
    "slice_size_not_constant": (lambda m, x: m.slice(x, [0] * 4, _runtime_index(m)), r"operator 0 \(SLICE\): size is not a constant"),
    "ellipsis": (lambda m, x: m.strided_slice(x, [0] * 4, [0] * 4, [1] * 4, end_mask=15, ellipsis_mask=1), r"operator 0 \(STRIDED_SLICE\): ellipsis_mask 1"),
    "new_axis": (lambda m, x: m.strided_slice(x, [0] * 4, [0] * 4, [1] * 4, end_mask=15, new_axis_mask=2), r"operator 0 \(STRIDED_SLICE\): new_axis_mask 2"),
    "shrink_axis": (lambda m, x: m.strided_slice(x, [0] * 4, [0] * 4, [1] * 4, end_mask=15, shrink_axis_mask=4), r"operator 0 \(STRIDED_SLICE\): shrink_axis_mask 4"),
    "offset": (lambda m, x: m.strided_slice(x, [0] * 4, [1, 3, 3, 5], [1] * 4, offset=True), r"operator 0 \(STRIDED_SLICE\): offset"),
    "negative_stride": (lambda m, x: m.strided_slice(x, [0, 6, 0, 0], [1, 0, 6, 5], [1, -1, 1, 1]), r"operator 0 \(STRIDED_SLICE\): strides \[1, -1, 1, 1\]"),
    "zero_stride": (lambda m, x: m.strided_slice(x, [0] * 4, [1, 7, 6, 5], [1, 1, 0, 1]), r"operator 0 \(STRIDED_SLICE\): strides \[1, 1, 0, 1\]"),
    "empty": (lambda m, x: m.strided_slice(x, [0, 4, 0, 0], [1, 4, 6, 5], [1] * 4), r"operator 0 \(STRIDED_SLICE\): the result is empty along axis 1"),
    "batch": (lambda m, x: m.strided_slice(x, [1, 0, 0, 0], [2, 7, 6, 5], [1] * 4), r"operator 0 \(STRIDED_SLICE\): (the result is empty along axis 0|only the full range is run on the batch axis)"),
    "channels": (lambda m, x: m.strided_slice(x, [0, 0, 0, 1], [1, 7, 6, 4], [1] * 4), r"operator 0 \(STRIDED_SLICE\): only the full range is run on the channel axis"),
    "channel_stride": (lambda m, x: m.strided_slice(x, [0] * 4, [0] * 4, [1, 1, 1, 2], end_mask=15), r"only the full range is run on the channel axis"),
    "slice_channels": (lambda m, x: m.slice(x, [0, 0, 0, 2], [1, 7, 6, 3]), r"operator 0 \(SLICE\): only the full range is run on the channel axis"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_operator(name):
    build, message = REFUSALS[name]
    m, x = model()
    g = finish(m, build(m, x))
    with pytest.raises(NotImplementedError, match=message):
        g.check_executable()
    with pytest.raises(NotImplementedError, match=message):
        build_plan(g)


def test_a_slice_is_refused_against_the_planned_shape():
    """The flatbuffer does not state H and W: the planner resolves against the shape it plans for."""
    m, x = model((1, 0, 0, 5))
    g = finish(m, m.strided_slice(x, [0, 4, 0, 0], [1, 6, 6, 5], [1] * 4))
    assert build_plan(g, input_shape=(7, 6, 5)).output_shape == (2, 6, 5)
    with pytest.raises(NotImplementedError, match=r"operator 0 \(STRIDED_SLICE\): the result is empty along axis 1"):
        build_plan(g, input_shape=(4, 6, 5))


# ---- 3. the planner's folds ----
def conv_w(rng, co, k, ci):
    return rng.normal(0, 0.3, size=(co, k, k, ci)).astype(F32)


def kinds(plan):
    return [o.kind for o in plan.ops]


def test_one_by_one_pools_become_slices():
    rng = np.random.default_rng(0)
    m, x = model((1, 9, 9, 8))
    a = m.pool("AVERAGE_POOL_2D", x, 1, 2, tb.VALID)
    b = m.pool("MAX_POOL_2D", x, 1, (3, 1), tb.SAME)
    c = m.pool("AVERAGE_POOL_2D", x, 1, 2, tb.VALID, act=tb.RELU)      # a fused activation: stays a pool
    d = m.pool("AVERAGE_POOL_2D", x, (1, 2), 2, tb.VALID)              # wider than 1: a mean of two
    outs = [m.conv(t, conv_w(rng, 8, 1, 8), None) for t in (a, b, c, d)]
    g = finish(m, m.concat([outs[0], outs[2]]))
    for out_t, want_kind, strides in ((outs[0], _lib.GRAPH_SLICE, (2, 2)), (outs[1], _lib.GRAPH_SLICE, (3, 1)),
                                      (outs[2], _lib.GRAPH_AVG_POOL, (2, 2)), (outs[3], _lib.GRAPH_AVG_POOL, (2, 2))):
        plain, fold = build_plan(g, output=out_t), build_plan(g, output=out_t, fold_windows=True)
        assert plain.ops[0].kind in (_lib.GRAPH_AVG_POOL, _lib.GRAPH_MAX_POOL) and fold.ops[0].kind == want_kind
        assert (fold.ops[0].stride_h, fold.ops[0].stride_w) == strides and plain.output_shape == fold.output_shape
        assert fold.ops[0].name == plain.ops[0].name
        # the pool kernel's mean is 0 + e: the SLICE of an AVERAGE pool makes +0.0 of a -0.0 as well (param 1)
        assert fold.ops[0].param == (1.0 if want_kind == _lib.GRAPH_SLICE and fold.ops[0].name[0] == "A" else 0.0)
    assert build_plan(g, output=outs[0], fold_windows=True).ops[0].pads == (0, 0, 0, 0)     # 9 -> 5: (5 - 1) * 2 + 1 = 9
    assert build_plan(g, output=outs[1], fold_windows=True).ops[0].pads == (0, 0, -2, 0)    # 9 -> 3 rows: 7 of 9 read


def test_chains_compose_into_one_slice():
    rng = np.random.default_rng(1)
    m, x = model((1, 31, 31, 8))
    r = m.unary("RELU", x)
    t = m.crop_top_left(m.pad(r, [[0, 0], [0, 1], [0, 1], [0, 0]]))
    y = m.conv(m.pool("AVERAGE_POOL_2D", t, 1, 2, tb.VALID), conv_w(rng, 8, 1, 8), None)
    g = finish(m, y)
    plain, fold = build_plan(g), build_plan(g, fold_windows=True)
    assert plain.census() == {"RELU": 1, "PAD": 1, "STRIDED_SLICE": 1, "AVERAGE_POOL_2D": 1, "CONV_2D": 1}
    assert fold.census() == {"RELU": 1, "PAD>STRIDED_SLICE>AVERAGE_POOL_2D": 1, "CONV_2D": 1}
    o = fold.ops[1]
    # rows 1, 3, .. 29 and the zero row 31: pad_top -1, stride 2, one row of zeros at the bottom
    assert o.kind == _lib.GRAPH_SLICE and o.pads == (-1, -1, 1, 1) and (o.stride_h, o.stride_w) == (2, 2) and o.in0 == plain.ops[0].out
    assert o.param == 1.0   # the AVERAGE pool's + 0.0f stays with the chain
    assert fold.arena_floats < plain.arena_floats
    both = build_plan(g, **FOLDS)
    assert both.census() == {"RELU>PAD>STRIDED_SLICE>AVERAGE_POOL_2D": 1, "CONV_2D": 1} and both.ops[0].act == tb.RELU
    assert both.ops[0].in0 == both.input


def test_a_slice_then_a_pad_is_not_composed():
    """The PAD's zeros lie inside the original tensor: a SLICE reads the original there."""
    rng = np.random.default_rng(2)
    m, x = model((1, 9, 9, 8))
    t = m.pad(m.crop_top_left(m.unary("RELU", x)), [[0, 0], [0, 1], [0, 1], [0, 0]])
    g = finish(m, m.conv(m.pool("MAX_POOL_2D", t, 3, 2, tb.VALID), conv_w(rng, 8, 1, 8), None))
    fold = build_plan(g, fold_windows=True)
    assert fold.census() == build_plan(g).census() == {"RELU": 1, "STRIDED_SLICE": 1, "PAD": 1, "MAX_POOL_2D": 1, "CONV_2D": 1}
    # ... while a PAD then a slice that reaches the PAD's own zeros composes, and the next slice composes onto that no more
    m, x = model((1, 9, 9, 8))
    t = m.slice(m.pad(m.unary("RELU", x), [[0, 0], [2, 1], [0, 3], [0, 0]]), [0, 1, 0, 0], [-1, -1, -1, -1])
    g = finish(m, m.conv(m.crop_top_left(t), conv_w(rng, 8, 1, 8), None))
    fold = build_plan(g, fold_windows=True)
    assert fold.census() == {"RELU": 1, "PAD>SLICE>STRIDED_SLICE": 1, "CONV_2D": 1} and fold.ops[1].pads == (0, -1, 1, 3)
    assert fold.ops[1].param == 0.0


pad_then = tn.pad_then


@pytest.mark.parametrize("reader,kind,k,stride,pads", [
    ("conv", _lib.GRAPH_CONV, 3, 1, ((1, 1), (1, 1))), ("conv", _lib.GRAPH_CONV, 7, 2, ((3, 3), (2, 3))),
    ("dw", _lib.GRAPH_DWCONV, 5, 2, ((1, 2), (1, 2))), ("dw", _lib.GRAPH_DWCONV, 7, 2, ((2, 3), (2, 3)))])
def test_a_pad_folds_into_its_valid_convolution(reader, kind, k, stride, pads):
    g = Graph(pad_then(reader, pads, k, stride, size=11))
    plain, fold = build_plan(g), build_plan(g, fold_windows=True)
    name = "CONV_2D" if reader == "conv" else "DEPTHWISE_CONV_2D"
    assert plain.census() == {"RELU": 1, "PAD": 1, name: 1} and fold.census() == {"RELU": 1, "PAD>" + name: 1}
    o = fold.ops[-1]
    assert o.kind == kind and o.pads == (pads[0][0], pads[1][0], pads[0][1], pads[1][1]) and o.in0 == plain.ops[0].out
    assert (o.stride_h, o.kh) == (stride, k) and fold.output_shape == plain.output_shape and fold.arena_floats < plain.arena_floats
    assert np.array_equal(o.weights, plain.ops[-1].weights)


@pytest.mark.parametrize("reader", ["conv", "dw"])
def test_a_pad_folds_into_a_hybrid_operator_and_moves_its_quant_params(reader):
    g = Graph(pad_then(reader, ((1, 2), (1, 2)), 5, 2, hybrid=True, size=11, c=8 if reader == "conv" else 48))
    plain, fold = build_plan(g), build_plan(g, fold_windows=True)
    q8 = _lib.GRAPH_CONV_Q8 if reader == "conv" else _lib.GRAPH_DWCONV_Q8
    assert kinds(plain) == [_lib.GRAPH_AFFINE, _lib.GRAPH_PAD, _lib.GRAPH_QUANT_PARAMS, q8]
    assert kinds(fold) == [_lib.GRAPH_AFFINE, _lib.GRAPH_QUANT_PARAMS, q8]
    relu_out = plain.ops[0].out
    assert fold.ops[1].in0 == relu_out == fold.ops[2].in0 and fold.ops[2].in1 == fold.ops[1].out and fold.ops[2].pads == (1, 1, 2, 2)
    # multiplied out on the host it is the float32 fold
    assert build_plan(g, fold_windows=True, quantised_math="float").census() == \
        {"RELU": 1, "PAD>" + ("CONV_2D" if reader == "conv" else "DEPTHWISE_CONV_2D"): 1}


@pytest.mark.parametrize("case", ["two_readers", "max_pool", "average_pool_3x3", "pad_as_wide_as_the_kernel", "padded_tensor_is_the_output",
                                  "same_padding"])
def test_a_pad_that_does_not_fold(case):
    if case == "two_readers":
        blob = pad_then("conv", extra_reader=True)
    elif case == "max_pool":
        blob = pad_then("MAX_POOL_2D")
    elif case == "average_pool_3x3":
        blob = pad_then("AVERAGE_POOL_2D")
    elif case == "pad_as_wide_as_the_kernel":
        blob = pad_then("dw", ((1, 3), (1, 1)), 3)
    elif case == "padded_tensor_is_the_output":
        blob = pad_then("conv", as_output=True)
    else:
        rng = np.random.default_rng(4)
        m, x = model((1, 9, 9, 8))
        p = m.pad(m.unary("RELU", x), [[0, 0], [1, 1], [1, 1], [0, 0]])
        m.outputs = [m.conv(p, conv_w(rng, 8, 3, 8), None, 1, tb.SAME)]   # SAME brings pads of its own
        blob = m.finish()
    g = Graph(blob)
    plain, fold = build_plan(g), build_plan(g, **FOLDS)
    assert fold.census() == plain.census() and fold.census()["PAD"] == 1 and kinds(fold) == kinds(plain)
    assert [o.pads for o in fold.ops] == [o.pads for o in plain.ops] and fold.arena_floats == plain.arena_floats


def test_a_pad_inside_a_concatenation_does_not_fold():
    rng = np.random.default_rng(5)
    m, x = model((1, 9, 9, 8))
    r = m.unary("RELU", x)
    p = m.pad(r, [[0, 0], [1, 1], [1, 1], [0, 0]])
    y = m.conv(p, conv_w(rng, 8, 3, 8), None, 1, tb.VALID)
    q = m.pad(y, [[0, 0], [1, 1], [1, 1], [0, 0]])
    g = finish(m, m.conv(m.concat([p, q]), conv_w(rng, 8, 1, 16), None))
    fold = build_plan(g, fold_windows=True)
    assert fold.census() == build_plan(g).census() and fold.census()["PAD"] == 2


# ---- 4. with the keywords off nothing moves; MobileNetV2 loses its PADs ----
TODAY = {
    "mobilenet_v2": (lambda: td.mobilenet_v2(6, size=64, width=0.35),
                     {"CONV_2D": 35, "DEPTHWISE_CONV_2D": 17, "PAD": 4, "ADD": 10, "MEAN": 1, "FULLY_CONNECTED": 1, "LOGISTIC": 1}),
    "efficientnet_b0": (lambda: ts.efficientnet_b0(6, size=64, width=0.5), None),
    "resnet_v2": (lambda: tp.resnet_v2(6, seed=1), None),
}


@pytest.mark.parametrize("name", sorted(TODAY))
def test_plans_with_the_keywords_off_are_todays(name):
    """The census each family has at the parent commit (recorded there for MobileNetV2; for all three: the keywords left
    out, set to False, and -- no STRIDED_SLICE, 1 x 1 pool or bare RELU in front of a depthwise convolution in them --
    whatever fuse_preactivation_dw alone changes: nothing)."""
    builder, census = TODAY[name]
    g = Graph(builder())
    plain = build_plan(g, fuse_preactivation=True)
    off = build_plan(g, fuse_preactivation=True, fold_windows=False, fuse_preactivation_dw=False)
    dw = build_plan(g, fuse_preactivation=True, fuse_preactivation_dw=True)
    if census is not None:
        assert build_plan(g).census() == census
    for other in (off, dw):
        assert [(o.kind, o.name, o.in0, o.in1, o.out, o.pads, o.act, o.param) for o in other.ops] == \
            [(o.kind, o.name, o.in0, o.in1, o.out, o.pads, o.act, o.param) for o in plain.ops]
        assert other.arena_floats == plain.arena_floats
        assert {k: (t.arena_offset, t.c_offset, t.c_stride) for k, t in other.tensors.items()} == \
            {k: (t.arena_offset, t.c_offset, t.c_stride) for k, t in plain.tensors.items()}
    assert not any(o.kind in (_lib.GRAPH_SLICE, _lib.GRAPH_DWCONV_PRE) for o in plain.ops)


@pytest.mark.parametrize("quantised", [False, True])
def test_mobilenet_v2_loses_exactly_its_four_pads(quantised):
    blob = td.mobilenet_v2(6, size=64, width=0.35)
    g = Graph(td.quantise(blob) if quantised else blob)
    plain, fold = build_plan(g), build_plan(g, **FOLDS)
    pads = [o for o in plain.ops if o.kind == _lib.GRAPH_PAD]
    assert len(pads) == 4 and not any(o.kind == _lib.GRAPH_PAD for o in fold.ops) and len(fold.ops) == len(plain.ops) - 4
    assert fold.arena_floats <= plain.arena_floats
    rest = [o for o in plain.ops if o.kind != _lib.GRAPH_PAD]
    padded = {p.out: p for p in pads}
    n_folded = 0
    for a, b in zip(rest, fold.ops):
        assert (a.kind, a.out, a.in1, a.act, a.kh, a.stride_h) == (b.kind, b.out, b.in1, b.act, b.kh, b.stride_h)
        if a.in0 in padded:
            p = padded[a.in0]
            assert b.in0 == p.in0 and (b.pads == p.pads == (0, 0, 1, 1) or b.kind == _lib.GRAPH_QUANT_PARAMS)
            assert b.name == ("PAD>" + a.name if b.kind != _lib.GRAPH_QUANT_PARAMS else a.name)
            n_folded += b.kind != _lib.GRAPH_QUANT_PARAMS
        else:
            assert (a.in0, a.pads, a.name) == (b.in0, b.pads, b.name)
        assert a.weights is b.weights or np.array_equal(a.weights, b.weights)
    assert n_folded == 4


# ---- 5. the pre-activation in front of depthwise convolutions and slices ----
def preact_readers(readers, hybrid=False):
    """RELU6 on the input with the given readers; their outputs (all 5 x 5) are added up."""
    rng = np.random.default_rng(6)
    m = tn.ModelNAS()
    c = 48 if hybrid else 8
    x = m.tensor([1, 9, 9, c], name="input")
    m.inputs = [x]
    r = m.unary("RELU6", x)
    outs = []
    for kind in readers:
        if kind == "conv":
            outs.append(m.conv(r, conv_w(rng, c, 3, c), np.zeros(c, F32), 2, tb.SAME))
        elif kind == "dw":
            outs.append(m.depthwise(r, rng.normal(0, 0.3, size=(1, 5, 5, c)).astype(F32), np.zeros(c, F32), 2, tb.SAME))
        elif kind == "slice":
            outs.append(m.strided_slice(r, [0] * 4, [0] * 4, [1, 2, 2, 1], begin_mask=15, end_mask=15))
        elif kind == "max_pool":
            outs.append(m.pool("MAX_POOL_2D", r, 3, 2, tb.SAME))
    y = outs[0]
    for o in outs[1:]:
        y = m.binary("ADD", y, o)
    m.outputs = [m.binary("ADD", y, y) if len(outs) == 1 else y]
    blob = m.finish()
    if hybrid:
        blob = td.quantise(blob, min_elements=5 * 5 * 48)   # the depthwise filter alone (the 3 x 3 CONV_2D is larger: float mode below)
    return blob


def test_a_bare_relu_with_mixed_readers_is_dropped_under_the_flag():
    g = Graph(preact_readers(["conv", "dw", "slice"]))
    plain = build_plan(g, fuse_preactivation=True)
    assert plain.census() == {"RELU6": 1, "CONV_2D": 1, "DEPTHWISE_CONV_2D": 1, "STRIDED_SLICE": 1, "ADD": 2}   # today's rule: kept
    assert build_plan(g, fuse_preactivation=True, fold_windows=True).census() == plain.census()
    for kw in (dict(fuse_preactivation_dw=True), dict(fuse_preactivation=True, fuse_preactivation_dw=True)):
        plan = build_plan(g, **kw)
        assert plan.census() == {"AFFINE>CONV_2D": 1, "RELU6>DEPTHWISE_CONV_2D": 1, "RELU6>STRIDED_SLICE": 1, "ADD": 2}
        conv, dw, sl = plan.ops[:3]
        assert (conv.kind, dw.kind, sl.kind) == (_lib.GRAPH_CONV_PRE, _lib.GRAPH_DWCONV_PRE, _lib.GRAPH_SLICE) and _lib.GRAPH_DWCONV_PRE == 21
        assert conv.in0 == dw.in0 == sl.in0 == plan.input and conv.param == dw.param == float(tb.RELU6) and sl.act == tb.RELU6
        assert np.array_equal(conv.pre_scale, np.ones(8, F32)) and np.array_equal(conv.pre_shift, np.zeros(8, F32))
        assert dw.weights.shape == (25, 8) and np.array_equal(dw.weights, plain.ops[2].weights)


def test_a_relu_that_keeps_its_launch():
    # a MAX_POOL reader
    g = Graph(preact_readers(["dw", "max_pool"]))
    assert build_plan(g, fuse_preactivation=True, **FOLDS).census() == {"RELU6": 1, "DEPTHWISE_CONV_2D": 1, "MAX_POOL_2D": 1, "ADD": 1}
    # a DWCONV_Q8 reader: it quantises with the parameters of the stored, activated tensor
    g = Graph(preact_readers(["dw"], hybrid=True))
    plan = build_plan(g, fuse_preactivation=True, **FOLDS)
    assert kinds(plan) == [_lib.GRAPH_AFFINE, _lib.GRAPH_QUANT_PARAMS, _lib.GRAPH_DWCONV_Q8, _lib.GRAPH_ADD]
    assert build_plan(g, fuse_preactivation=True, quantised_math="float", **FOLDS).census() == {"RELU6>DEPTHWISE_CONV_2D": 1, "ADD": 1}
    # the flag off
    g = Graph(preact_readers(["dw", "slice"]))
    assert build_plan(g, fuse_preactivation=True, fold_windows=True).census() == {"RELU6": 1, "DEPTHWISE_CONV_2D": 1, "STRIDED_SLICE": 1, "ADD": 1}
    assert build_plan(g, **FOLDS).census() == {"RELU6>DEPTHWISE_CONV_2D": 1, "RELU6>STRIDED_SLICE": 1, "ADD": 1}
    # a pre-activation with constants in front of a depthwise convolution stays a launch
    rng = np.random.default_rng(7)
    m, x = model((1, 9, 9, 8))
    y = m.conv(x, conv_w(rng, 8, 1, 8), None)
    a = m.binary("ADD", m.binary("MUL", y, rng.uniform(0.5, 1.5, size=8).astype(F32)), rng.normal(size=8).astype(F32), tb.RELU)
    d = m.depthwise(a, rng.normal(0, 0.3, size=(1, 3, 3, 8)).astype(F32), np.zeros(8, F32))
    g = finish(m, m.conv(m.concat([y, d]), conv_w(rng, 8, 1, 16), None))
    plan = build_plan(g, fuse_preactivation=True, **FOLDS)
    assert plan.census() == {"CONV_2D": 2, "MUL+ADD": 1, "DEPTHWISE_CONV_2D": 1}


# ---- 6. the NASNet stand-in ----
@pytest.fixture(scope="module")
def nasnets():
    return {merge: Graph(tn.nasnet(17, merge_relus=merge)) for merge in (False, True)}


@pytest.mark.parametrize("merge_relus", [False, True])
def test_nasnet_plans_under_both_settings(nasnets, merge_relus):
    g = nasnets[merge_relus]
    assert sum(o["name"] == "STRIDED_SLICE" for o in g.ops) == 4
    plain = build_plan(g)
    fold = build_plan(g, fuse_preactivation=True, **FOLDS)
    assert plain.output_shape == fold.output_shape == (1, 1, 17)
    sizes = sorted(set(t.H for t in plain.tensors.values()) - {1, 64}, reverse=True)
    assert [s for s in sizes if s in (31, 16, 8, 4, 2)] == [31, 16, 8, 4, 2]
    assert sum(o.kind == _lib.GRAPH_SLICE for o in plain.ops) == 4 and plain.census()["PAD"] == 24
    print("NASNet stand-in (merge_relus %s): %d launches, %d with the folds; arena %d -> %d floats per sample"
          % (merge_relus, len(plain.ops), len(fold.ops), plain.arena_floats, fold.arena_floats))
    print(fold.census())
    assert len(fold.ops) < len(plain.ops) and fold.arena_floats <= plain.arena_floats
    # no bare RELU but the head's in front of MEAN
    bare = [o for o in fold.ops if o.kind == _lib.GRAPH_AFFINE and o.scale is None and o.shift is None and not o.copy]
    assert len(bare) == 1 and [r.kind for r in fold.ops if r.in0 == bare[0].out] == [_lib.GRAPH_MEAN]
    # no PAD but the one in front of each reduction cell's three 3 x 3 pools, which the fold rules leave alone ("padding
    # never wins", "divided by the in-bounds count")
    left = [o for o in fold.ops if o.kind == _lib.GRAPH_PAD]
    assert len(left) == 4
    for p in left:
        readers = [r for r in fold.ops if r.in0 == p.out]
        assert sorted(r.kind for r in readers) == [_lib.GRAPH_MAX_POOL, _lib.GRAPH_MAX_POOL, _lib.GRAPH_AVG_POOL] and all(r.kh == 3 for r in readers)
    # each adjust block's two paths: two SLICE launches on the block's un-activated input, RELU taken along
    slices = [o for o in fold.ops if o.kind == _lib.GRAPH_SLICE]
    assert [o.name for o in slices] == ["RELU>AVERAGE_POOL_2D", "RELU>PAD>STRIDED_SLICE>AVERAGE_POOL_2D"] * 4
    for a, b in zip(slices[0::2], slices[1::2]):
        assert a.in0 == b.in0 and a.act == b.act == tb.RELU and (a.stride_h, a.stride_w) == (b.stride_h, b.stride_w) == (2, 2)
        odd = fold.tensors[a.in0].H % 2
        assert a.pads == (0, 0, odd - 1, odd - 1) and b.pads == (-1, -1, odd, odd)
    assert fold.tensors[slices[0].in0].H == 31
    assert sum(o.kind == _lib.GRAPH_DWCONV_PRE for o in fold.ops) == 35 and sum(o.kind == _lib.GRAPH_DWCONV for o in fold.ops) == 35
    assert sum(o.name.startswith("RELU>PAD>DEPTHWISE") for o in fold.ops) == 16


def test_nasnet_with_cropping_as_slice(nasnets):
    g = Graph(tn.nasnet(17, as_slice=True))
    fold = build_plan(g, fuse_preactivation=True, **FOLDS)
    assert fold.census()["RELU>PAD>SLICE>AVERAGE_POOL_2D"] == 4
    ref = build_plan(nasnets[False], fuse_preactivation=True, **FOLDS)
    assert [(o.kind, o.pads, o.stride_h) for o in fold.ops] == [(o.kind, o.pads, o.stride_h) for o in ref.ops]


def test_get_interpreter_on_a_nasnet_named_sidecar(tmp_path, monkeypatch):
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, get_interpreter, inc3_preprocess

    (tmp_path / "n.tflite").write_bytes(tn.nasnet(6))
    with open(tmp_path / "n.json", "w") as fh:
        json.dump({"labels": ["l%d" % i for i in range(6)], "type": "thermal",
                   "hyperparams": {"frame_size": 32, "model_name": "nasnet", "channels": ["thermal", "thermal", "filtered"]}}, fh)
    monkeypatch.delenv("CPX_TFLITE_FOLD_WINDOWS", raising=False)
    monkeypatch.delenv("CPX_TFLITE_FUSE_PREACT", raising=False)
    monkeypatch.delenv("CPX_TFLITE_FUSE_PREACT_DW", raising=False)
    # the defaults: the window folds on, the RELU into depthwise convolutions and slices off (it measured slower at N = 1)
    _, default = LiteInterpreter(tmp_path / "n.tflite")._plan((64, 64, 2))
    assert sum(o.kind == _lib.GRAPH_PAD for o in default.ops) == 4 and sum(o.kind == _lib.GRAPH_SLICE for o in default.ops) == 8
    assert not any(o.kind == _lib.GRAPH_DWCONV_PRE or (o.kind == _lib.GRAPH_SLICE and o.act) for o in default.ops)
    assert sum(o.kind == _lib.GRAPH_CONV_PRE for o in default.ops) > 0
    monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT_DW", "1")
    interp = get_interpreter(ModelConfig.load({"id": 1, "name": "n", "model_file": str(tmp_path / "n.tflite")}))
    assert isinstance(interp, LiteInterpreter) and interp.preprocess_fn is inc3_preprocess and interp.input_mode is None
    assert interp.limits_flags() & _lib.LIMITS_TF_SCALING
    _, plan = interp._plan((64, 64, 2))
    assert plan.ops[0].kind == _lib.GRAPH_CHANNEL_MAP and sum(o.kind == _lib.GRAPH_PAD for o in plan.ops) == 4
    assert sum(o.kind == _lib.GRAPH_SLICE for o in plan.ops) == 8 and sum(o.kind == _lib.GRAPH_DWCONV_PRE for o in plan.ops) == 35
    monkeypatch.setenv("CPX_TFLITE_FOLD_WINDOWS", "0")
    monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT", "0")
    _, plain = LiteInterpreter(tmp_path / "n.tflite")._plan((64, 64, 2))
    assert sum(o.kind == _lib.GRAPH_PAD for o in plain.ops) == 24 and sum(o.kind == _lib.GRAPH_SLICE for o in plain.ops) == 4
    assert not any(o.kind in (_lib.GRAPH_DWCONV_PRE, _lib.GRAPH_CONV_PRE) for o in plain.ops)
    monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT", "1")
    monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT_DW", "2")
    with pytest.raises(ValueError, match="CPX_TFLITE_FUSE_PREACT_DW='2': one of 0, 1"):
        LiteInterpreter(tmp_path / "n.tflite")
    monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT_DW", "1")
    monkeypatch.setenv("CPX_TFLITE_FOLD_WINDOWS", "yes")
    with pytest.raises(ValueError, match="CPX_TFLITE_FOLD_WINDOWS='yes': one of 0, 1"):
        LiteInterpreter(tmp_path / "n.tflite")


# ---- 7. inceptionresnetv2 ----
def test_an_inception_resnet_block_plans_and_evaluates(tmp_path):
    """The residual scaling (MUL by 0.17) folds into the 1 x 1 convolution, the ADD carries the RELU.  float32 against
    float64 on the CPU at CONV_REL (tests/test_tflite_graph_gpu.py) of the magnitude that reaches the output: |x| + the
    convolution's sum |x| |w| + |b|, scaled."""
    from test_tflite_graph_gpu import CONV_REL
    from cpx.ml_tools.interpreter import LiteInterpreter

    blob = tn.inception_resnet_block()
    g = Graph(blob)
    plan = build_plan(g, fuse_preactivation=True, **FOLDS)
    assert plan.census() == {"CONV_2D": 6, "CONV_2D+MUL": 1, "ADD": 1} and plan.ops[-1].act == tb.RELU
    up = plan.ops[-2]
    assert np.array_equal(up.scale, np.full(32, 0.17, F32)) and plan.output_shape == (9, 9, 32)
    x = np.random.default_rng(8).normal(size=(2, 9, 9, 32)).astype(F32)
    v64, mag = ten.evaluate(g, x, magnitudes=True)
    v32 = ten.evaluate(g, x, dtype=torch.float32)
    out, conv_t = g.outputs[0], g.ops[-3]["outputs"][0]
    bound = CONV_REL * (np.abs(x) + 0.17 * mag[conv_t])
    err = np.abs(v32[out] - v64[out])
    print("inceptionresnetv2 block: float32 vs float64 %.3g, bound %.3g at the worst element" % (float(err.max()), float(bound[err == err.max()].max())))
    assert np.all(err <= bound) and float(np.abs(v64[out]).max()) > 0.5 and float((v64[out] == 0).mean()) > 0.05
    (tmp_path / "m.tflite").write_bytes(blob)
    with open(tmp_path / "m.json", "w") as fh:
        json.dump({"labels": ["a"], "type": "thermal", "hyperparams": {"frame_size": 9, "model_name": "inceptionresnetv2",
                                                                       "channels": ["thermal", "filtered"]}}, fh)
    interp = LiteInterpreter(tmp_path / "m.tflite", load_model=False)
    assert interp.limits_flags() & _lib.LIMITS_TF_SCALING
