"""The NASNet family in the TFLite graph executor on the GPU: SLICE (STRIDED_SLICE / SLICE, 1 x 1 pools, chains with a PAD)
against NumPy indexing, bit for bit; DWCONV_PRE against the RELU and DWCONV launches it replaces, bit for bit, and against
float64; a PAD folded into its VALID convolution (float32 and hybrid) against the two launches; the adjust block; the
NASNet stand-in of tests/tflite_build_nas.py through LiteInterpreter and ClipClassifier.  The flatbuffers are synthetic and
the evaluator reads the Graph only (tests/tflite_eval_nas.py).  Parity with the TFLite runtime (ai_edge_litert) and the
converter's exact layout of a NASNet are not pinned here: neither is installed."""
import json
import os
import shutil

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_dw as td
import tflite_build_nas as tn
import tflite_eval_nas as ten
from test_tflite_graph_gpu import CONV_REL, LABELS17, LOGIT_MULTIPLE
from test_tflite_preact_gpu import raw_samples, write_model

pytestmark = pytest.mark.gpu
F32 = np.float32
FOLDS = dict(fold_windows=True, fuse_preactivation_dw=True, fuse_preactivation=True)
SENTINEL = F32(-12345.678)


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def run(engine, blob, x, output=None, out_slice=None, out=None, channel_map=None, quantised_math="hybrid", **plan_kw):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    shape = x.shape[1:] if channel_map is None else (x.shape[1], x.shape[2], len(channel_map))
    plan = build_plan(g, input_shape=shape, output=output, channel_map=channel_map, quantised_math=quantised_math, **plan_kw)
    dev = GraphDevice(engine, plan, out_slice=out_slice)
    got = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device), out=out).cpu().numpy()
    dev.close()
    return g, plan, got


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def signed_sample(rng, shape, scale=1.0):
    """Normal values with negatives, and a -0.0, a +0.0 and a tiny negative in every sample: an activation applied by
    mistake, or left out, shows in the bits."""
    x = rng.normal(0, scale, size=shape).astype(F32)
    kind = rng.random(size=shape)
    x[kind < 0.04] = -0.0
    x[(kind >= 0.04) & (kind < 0.06)] = 0.0
    x[(kind >= 0.06) & (kind < 0.08)] = -1e-30
    assert np.signbit(x).any() and (bits(x) == 0x80000000).any()
    return x


# ---- 1. SLICE against NumPy ----
def crop(m, t):
    return m.crop_top_left(t)


def from_row_1_stride_2(m, t):
    return m.strided_slice(t, [0, 1, 1, 0], [0, 0, 0, 0], [1, 2, 2, 1], begin_mask=0b1001, end_mask=0b1111)


def every_other(m, t):
    return m.strided_slice(t, [0, 0, 0, 0], [0, 0, 0, 0], [1, 2, 2, 1], begin_mask=15, end_mask=15)


def pool_1x1_s2(m, t):
    return m.pool("AVERAGE_POOL_2D", t, 1, 2, tb.VALID)


def max_pool_1x1_s2(m, t):
    return m.pool("MAX_POOL_2D", t, 1, 2, tb.VALID)


def adjust_path(m, t):
    return pool_1x1_s2(m, crop(m, m.pad(t, [[0, 0], [0, 1], [0, 1], [0, 0]])))


def pure_pad(m, t):
    p = m.pad(t, [[0, 0], [2, 3], [2, 3], [0, 0]])
    return m.slice(p, [0, 0, 0, 0], [-1, -1, -1, -1])   # the full range: PAD > SLICE is one SLICE launch of positive pads


def padded(x, pads):
    return np.pad(x, ((0, 0), pads[0], pads[1], (0, 0)))


# name -> (chain, NumPy's answer, N, H, W, C, keyword arguments)
SLICE_CASES = {
    "7x6x3_scalar_path": (crop, lambda x: x[:, 1:, 1:], 3, 7, 6, 3, {}),
    "7x6x8_quad_path": (every_other, lambda x: x[:, ::2, ::2], 3, 7, 6, 8, {}),
    "9x9x12_cropped": (crop, lambda x: x[:, 1:, 1:], 3, 9, 9, 12, {}),
    "31_from_row_1_stride_2": (from_row_1_stride_2, lambda x: x[:, 1::2, 1::2], 2, 31, 31, 8, {}),
    "31_to_16_average_pool_1x1": (pool_1x1_s2, lambda x: x[:, ::2, ::2], 2, 31, 31, 8, {"mean": True}),
    "31_to_16_max_pool_1x1": (max_pool_1x1_s2, lambda x: x[:, ::2, ::2], 2, 31, 31, 8, {}),
    "adjust_path_one_launch": (adjust_path, lambda x: padded(x, ((0, 1), (0, 1)))[:, 1::2, 1::2], 2, 31, 31, 8, {"zero_edge": True, "mean": True}),
    "pure_pad_2_3": (pure_pad, lambda x: padded(x, ((2, 3), (2, 3))), 3, 7, 6, 8, {}),
    "relu": (adjust_path, lambda x: padded(np.maximum(x, 0), ((0, 1), (0, 1)))[:, 1::2, 1::2], 3, 9, 9, 8, {"act": "RELU", "mean": True}),
    "relu6": (crop, lambda x: np.minimum(np.maximum(x, 0), 6)[:, 1:, 1:], 3, 7, 6, 8, {"act": "RELU6", "scale": 6.0}),
    "relu_scalar_path": (crop, lambda x: np.maximum(x, 0)[:, 1:, 1:], 3, 7, 6, 3, {"act": "RELU"}),
    "input_slice_8_to_24_of_40": (adjust_path, lambda x: padded(x, ((0, 1), (0, 1)))[:, 1::2, 1::2], 3, 9, 9, 16, {"c_total": 40, "c_from": 8, "mean": True}),
    "input_slice_off_the_quad_grid": (crop, lambda x: x[:, 1:, 1:], 3, 7, 6, 16, {"c_total": 40, "c_from": 6}),
    "output_into_wider_rows": (adjust_path, lambda x: padded(x, ((0, 1), (0, 1)))[:, 1::2, 1::2], 3, 9, 9, 8, {"out_slice": (4, 20), "mean": True}),
    "output_off_the_quad_grid": (crop, lambda x: x[:, 1:, 1:], 3, 7, 6, 8, {"out_slice": (5, 16)}),
}


def slice_graph(chain, H, W, C, act=None, c_total=None, c_from=0, seed=0):
    """input (-> RELU / RELU6) -> chain -> output.  c_total: the chain (or its activation) reads the channels
    [c_from, c_from + C) of a c_total-channel concatenation instead: a 1 x 1 convolution of the input, the input through a
    1 x 1 MAX_POOL_2D of stride 1 (the one producer that hands a -0.0 on: an AFFINE or a convolution adds its shift, be it
    0), another convolution.  -> (blob, the tensor that is read)."""
    rng = np.random.default_rng(seed)
    m = tn.ModelNAS()
    x = m.tensor([1, H, W, C], name="input")
    m.inputs = [x]
    src = x
    if c_total is not None:
        def conv(c):
            return m.conv(x, rng.normal(0, 0.3, size=(c, 1, 1, C)).astype(F32), rng.normal(size=c).astype(F32), 1, tb.SAME, tb.NONE)

        src = m.pool("MAX_POOL_2D", x, 1, 1, tb.VALID)
        m.concat([conv(c_from), src, conv(c_total - c_from - C)])
    m.outputs = [chain(m, src if act is None else m.unary(act, src))]
    return m.finish(), src


@pytest.mark.parametrize("name", sorted(SLICE_CASES))
def test_slice_equals_numpy_bit_for_bit(engine, name):
    """One SLICE launch for the whole chain, and it is a copy: the bits of NumPy's indexing of the very input.  A chain
    through a 1 x 1 AVERAGE_POOL_2D ("mean") is NumPy's + 0.0, as the pool launch's sum from 0 is: its -0.0 is a +0.0.  With an
    activation the values are NumPy's and the bits those of the RELU launch + the chain's launches it replaces; the zero it
    makes of a negative or of -0.0 is compared with its sign set aside, which IEEE 754's maxNum leaves open and NumPy's
    maximum and the device's v_max_f32 need not agree on."""
    import torch

    from cpx import _lib

    chain, want_fn, n, H, W, C, kw = SLICE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    blob, src = slice_graph(chain, H, W, C, act=kw.get("act"), c_total=kw.get("c_total"), c_from=kw.get("c_from", 0))
    x = signed_sample(rng, (n, H, W, C), kw.get("scale", 1.0))
    g, plan, got = run(engine, blob, x, **FOLDS)
    _, plain, unfolded = run(engine, blob, x)
    # (the producer of a concatenation's slice is a launch of its own: its tensor is not one the chain may drop)
    assert plan.ops[-1].kind == _lib.GRAPH_SLICE and sum(o.kind == _lib.GRAPH_SLICE for o in plan.ops) == (2 if "c_total" in kw else 1)
    assert not any(o.kind in (_lib.GRAPH_PAD, _lib.GRAPH_AVG_POOL, _lib.GRAPH_MAX_POOL, _lib.GRAPH_AFFINE) for o in plan.ops)
    assert len(plan.ops) < len(plain.ops) or len(plain.ops) == 1 or "c_total" in kw
    x_in = x
    if "c_total" in kw:
        t = plan.tensors[plan.ops[-1].in0]
        assert (t.c_offset, t.c_stride) == (kw["c_from"], kw["c_total"])
        x_in = run(engine, blob, x, output=src)[2]
        assert np.array_equal(bits(x_in), bits(x))
    want = np.ascontiguousarray(want_fn(x_in), F32)
    if kw.get("mean"):
        want = want + F32(0)
    assert plan.ops[-1].param == (1.0 if kw.get("mean") else 0.0)
    assert got.shape == want.shape == unfolded.shape
    assert np.signbit(x_in).any() and (bits(x_in) == 0x80000000).any()
    if "act" in kw:
        assert np.array_equal(bits(got + F32(0)), bits(want + F32(0))) and np.array_equal(bits(got), bits(unfolded))
        assert float(got.max()) > 0.5 and (kw["act"] != "RELU6" or (float((got == 6).mean()) > 0.02))
        assert float((got == 0).mean()) > 0.3
    else:
        n_diff = int((bits(got) != bits(want)).sum())
        print("%s: %d of %d elements differ from NumPy's; launches %d -> %d" % (name, n_diff, got.size, len(plain.ops), len(plan.ops)))
        assert n_diff == 0 and np.array_equal(bits(unfolded), bits(want))
        assert (bits(got) == 0x80000000).any() != bool(kw.get("mean"))    # the -0.0 came through as it is, or as the pool's +0.0
    if kw.get("zero_edge"):
        assert np.all(bits(got[:, -1]) == 0) and np.all(bits(got[:, :, -1]) == 0) and float(np.abs(got[:, :-1, :-1]).min()) >= 0
        assert plan.ops[-1].pads == (-1, -1, 1, 1) and (plan.ops[-1].stride_h, plan.ops[-1].stride_w) == (2, 2)
    if "out_slice" in kw:
        off, stride = kw["out_slice"]
        out = torch.full(got.shape[:3] + (stride,), float(SENTINEL), dtype=torch.float32, device=engine.device)
        _, _, sliced = run(engine, blob, x, out_slice=(off, stride), out=out, **FOLDS)
        assert np.array_equal(bits(sliced[..., off:off + C]), bits(want))
        assert np.all(sliced[..., :off] == SENTINEL) and np.all(sliced[..., off + C:] == SENTINEL)


def test_slice_batch_does_not_matter(engine):
    rng = np.random.default_rng(5)
    blob, _ = slice_graph(adjust_path, 31, 31, 8)
    x = signed_sample(rng, (1, 31, 31, 8))
    _, _, one = run(engine, blob, x, **FOLDS)
    _, _, five = run(engine, blob, np.repeat(x, 5, axis=0), **FOLDS)
    assert one.shape == (1, 16, 16, 8) and all(np.array_equal(bits(five[i]), bits(one[0])) for i in range(5))
    assert np.array_equal(bits(one), bits(padded(x, ((0, 1), (0, 1)))[:, 1::2, 1::2] + F32(0)))


# ---- 2. DWCONV_PRE against the two launches and against float64 ----
DW_PRE_CASES = {
    # k, stride, C, H, W, N, activation, keyword arguments
    "k3_s1": (3, 1, 24, 9, 9, 2, "RELU", {}),
    "k3_s2": (3, 2, 24, 9, 9, 2, "RELU", {}),
    "k5_s1": (5, 1, 24, 9, 9, 2, "RELU", {}),
    "k5_s2": (5, 2, 24, 9, 9, 2, "RELU", {}),
    "k7_s1": (7, 1, 24, 9, 9, 2, "RELU", {}),
    "k7_s2": (7, 2, 24, 11, 11, 2, "RELU", {}),
    "c3_scalar_k3": (3, 1, 3, 9, 9, 2, "RELU", {}),
    "c3_scalar_k5_s2": (5, 2, 3, 9, 9, 2, "RELU", {}),
    "relu6_both_clamps": (3, 1, 24, 9, 9, 2, "RELU6", {"scale": 6.0}),
    "slice_8_to_24_of_40": (3, 1, 16, 9, 9, 2, "RELU", {"c_total": 40, "c_from": 8}),
    "w5_ragged_run": (3, 1, 24, 6, 5, 3, "RELU", {}),     # 5 output columns: a run of 4 and a run of 1
    "w5_ragged_run_k5_s2": (5, 2, 24, 7, 9, 3, "RELU", {}),
}


def dw_pre_graph(k, stride, C, H, W, act, c_total=None, c_from=0, seed=0):
    rng = np.random.default_rng(seed)

    def chain(m, t):
        w = rng.normal(0, np.sqrt(2.0 / (k * k)), size=(1, k, k, C)).astype(F32)
        return m.depthwise(t, w, rng.normal(0, 0.05, size=C).astype(F32), stride, tb.SAME, tb.NONE)

    return slice_graph(chain, H, W, C, act=act, c_total=c_total, c_from=c_from, seed=seed + 1)


@pytest.mark.parametrize("name", sorted(DW_PRE_CASES))
def test_dwconv_pre_equals_the_two_launches_and_float64(engine, name):
    """Bit for bit: activate() on the loaded quad is what graph_affine_kernel stored.  Against float64: CONV_REL of
    sum |act(x)| |w| + |b| (the magnitude tests/tflite_eval_dw.py hands out), the bound of the float32 operators; the
    activation itself is exact."""
    from cpx import _lib

    k, stride, C, H, W, n, act, kw = DW_PRE_CASES[name]
    seed = sum(map(ord, name))
    blob, src = dw_pre_graph(k, stride, C, H, W, act, kw.get("c_total"), kw.get("c_from", 0), seed)
    x = signed_sample(np.random.default_rng(seed + 2), (n, H, W, C), kw.get("scale", 1.0))
    g, plan, fused = run(engine, blob, x, **FOLDS)
    _, plain, unfused = run(engine, blob, x)
    assert plan.ops[-1].kind == _lib.GRAPH_DWCONV_PRE and len(plan.ops) == len(plain.ops) - 1
    assert (plain.ops[-2].kind, plain.ops[-1].kind) == (_lib.GRAPH_AFFINE, _lib.GRAPH_DWCONV)
    assert plan.ops[-1].param == float(tb.RELU if act == "RELU" else tb.RELU6) and plan.ops[-1].name == act + ">DEPTHWISE_CONV_2D"
    n_diff = int((bits(fused) != bits(unfused)).sum())
    print("%s: %d of %d outputs differ between fused and unfused" % (name, n_diff, fused.size))
    assert fused.shape == unfused.shape and n_diff == 0 and np.all(np.isfinite(fused)) and float(np.abs(fused).max()) > 0.1
    if name.startswith("w5"):
        assert fused.shape[2] == 5
    dw = g.ops[-1]
    if "c_total" in kw:
        t = plan.tensors[plan.ops[-1].in0]
        assert (t.c_offset, t.c_stride) == (kw["c_from"], kw["c_total"])
        x_in = run(engine, blob, x, output=src)[2]
    else:
        x_in = x
    hi = 6.0 if act == "RELU6" else np.inf
    pre = np.minimum(np.maximum(x_in.astype(np.float64), 0.0), hi)
    if act == "RELU6":
        assert float((pre == 6.0).mean()) > 0.05 and float((pre == 0.0).mean()) > 0.05
    import tflite_eval_dw as ted
    import torch

    want, mag = ted.depthwise(dw, pre, g.const(dw["inputs"][1]), g.const(dw["inputs"][2]), torch.float64, magnitude=True)
    rel = float((np.abs(fused - want) / mag).max())
    print("%s: max |error| / (sum |act(x)| |w| + |b|) = %.3g (bound %.3g)" % (name, rel, CONV_REL))
    assert rel < CONV_REL


# ---- 3. a PAD folded into its VALID operator against the two launches ----
PAD_CASES = {
    # reader, k, stride, pads, hybrid
    "conv_3x3": ("conv", 3, 1, ((1, 1), (1, 1)), False),
    "conv_7x7_s2": ("conv", 7, 2, ((3, 3), (3, 3)), False),
    "dw_5x5_s2": ("dw", 5, 2, ((1, 2), (1, 2)), False),
    "dw_7x7_s2": ("dw", 7, 2, ((2, 3), (2, 3)), False),
    "conv_q8_3x3": ("conv", 3, 1, ((1, 1), (1, 1)), True),
    "conv_q8_7x7_s2": ("conv", 7, 2, ((3, 3), (3, 3)), True),
    "dw_q8_5x5_s2": ("dw", 5, 2, ((1, 2), (1, 2)), True),
    "dw_q8_7x7_s2": ("dw", 7, 2, ((2, 3), (2, 3)), True),
}


@pytest.mark.parametrize("name", sorted(PAD_CASES))
def test_a_folded_pad_equals_the_pad_launch_and_the_valid_operator(engine, name):
    """The same bits (cpx/ml_tools/tflite_graph.py gives the argument) from a strictly smaller arena.  Sample 2 is all
    positive: 0 is its minimum only through QUANT_PARAMS' rmin = min(0, min x), which the padded zeros therefore do not move."""
    from cpx import _lib

    reader, k, stride, pads, hybrid = PAD_CASES[name]
    c = 48 if hybrid and reader == "dw" else 16
    blob = tn.pad_then(reader, pads, k, stride, hybrid=hybrid, size=13, c=c, relu=False, seed=sum(map(ord, name)))
    rng = np.random.default_rng(9)
    x = signed_sample(rng, (3, 13, 13, c))
    x[2] = rng.uniform(0.5, 2.0, size=x[2].shape).astype(F32)
    g, fold, got = run(engine, blob, x, **FOLDS)
    _, plain, want = run(engine, blob, x)
    kind = {("conv", False): _lib.GRAPH_CONV, ("conv", True): _lib.GRAPH_CONV_Q8, ("dw", False): _lib.GRAPH_DWCONV,
            ("dw", True): _lib.GRAPH_DWCONV_Q8}[(reader, hybrid)]
    assert [o.kind for o in plain.ops] == [_lib.GRAPH_PAD] + ([_lib.GRAPH_QUANT_PARAMS] if hybrid else []) + [kind]
    assert [o.kind for o in fold.ops] == ([_lib.GRAPH_QUANT_PARAMS] if hybrid else []) + [kind]
    assert fold.ops[-1].pads == (pads[0][0], pads[1][0], pads[0][1], pads[1][1]) and fold.ops[-1].in0 == fold.input
    assert fold.arena_floats < plain.arena_floats
    n_diff = int((bits(got) != bits(want)).sum())
    print("%s: %d of %d outputs differ; arena %d -> %d floats per sample" % (name, n_diff, got.size, plain.arena_floats, fold.arena_floats))
    assert got.shape == want.shape and n_diff == 0 and float(np.abs(got).max()) > 0.1 and np.all(np.isfinite(got))
    assert float(x[2].min()) > 0 and float(np.abs(got[2]).max()) > 0.1
    # ... and against the evaluator of the flatbuffer, PAD and all: float64 at CONV_REL of the magnitude (float32), or
    # the hybrid restatement, which the existing tests hold the unfolded operators to bit for bit
    out = g.outputs[0]
    if hybrid:
        import tflite_eval_dw as ted

        assert np.array_equal(bits(got), bits(ted.evaluate_hybrid(g, x)[0][out]))
    else:
        v, mag = ten.evaluate(g, x, magnitudes=True)
        assert float((np.abs(got - v[out]) / mag[out]).max()) < CONV_REL


# ---- 4. the adjust block ----
def test_the_adjust_block_folded_equals_unfolded_and_float64(engine):
    """RELU -> (1 x 1 pool stride 2 | PAD -> [:, 1:, 1:, :] -> 1 x 1 pool stride 2) -> 1 x 1 CONV_2D each -> CONCATENATION
    -> MUL + ADD, 31 x 31 x 16, N = 2.  The RELU, the PAD and the STRIDED_SLICE launches go: 8 launches become 5 (the two
    pools stay launches, now SLICEs; the count by the fold rules is 3 fewer)."""
    from cpx import _lib

    blob = tn.adjust_block(31, 16, 16, seed=4)
    x = signed_sample(np.random.default_rng(10), (2, 31, 31, 16))
    g, fold, got = run(engine, blob, x, **FOLDS)
    _, plain, want = run(engine, blob, x)
    assert [o.name for o in plain.ops] == ["RELU", "AVERAGE_POOL_2D", "CONV_2D", "PAD", "STRIDED_SLICE", "AVERAGE_POOL_2D", "CONV_2D", "MUL+ADD"]
    assert [o.name for o in fold.ops] == ["RELU>AVERAGE_POOL_2D", "CONV_2D", "RELU>PAD>STRIDED_SLICE>AVERAGE_POOL_2D", "CONV_2D", "MUL+ADD"]
    assert [o.kind for o in fold.ops] == [_lib.GRAPH_SLICE, _lib.GRAPH_CONV, _lib.GRAPH_SLICE, _lib.GRAPH_CONV, _lib.GRAPH_AFFINE]
    assert got.shape == (2, 16, 16, 16) and np.array_equal(bits(got), bits(want)) and fold.arena_floats < plain.arena_floats
    v, mag = ten.evaluate(g, x, magnitudes=True)
    mul, add = g.ops[-2], g.ops[-1]
    s, h = (np.abs(g.const(op["inputs"][1]).astype(np.float64)) for op in (mul, add))
    convs = [op["outputs"][0] for op in g.ops if op["name"] == "CONV_2D"]
    bound = np.concatenate([mag[t] for t in convs], axis=-1) * s + h
    rel = float((np.abs(got - v[g.outputs[0]]) / bound).max())
    print("adjust block: max |error| / magnitude = %.3g (bound %.3g); %d -> %d launches" % (rel, CONV_REL, len(plain.ops), len(fold.ops)))
    assert rel < CONV_REL
    # the shifted path is not the plain one: on the odd 31 they read different pixels
    a, b = (run(engine, blob, x, output=t, **FOLDS)[2] for t in convs)
    assert a.shape == b.shape and float(np.abs(a).max()) > 0.1 and float(np.abs(b[:, -1]).max()) <= float(np.abs(g.const(g.ops[6]["inputs"][2])).max())


# ---- 5. the NASNet stand-in through LiteInterpreter ----
NASNET_SEED = 2


def test_nasnet_through_the_lite_interpreter(engine, tmp_path, monkeypatch):
    """The method of test_tflite_preact_gpu.py::test_whole_network_through_the_lite_interpreter: the device may deviate
    from the float64 evaluation of the flatbuffer by LOGIT_MULTIPLE times what a float32 evaluation on the CPU does.  Seed 2
    was chosen on the CPU with the two evaluators (of seeds 0 to 3): the float64 logits spread by 0.41 against a float32
    deviation of 2.3e-7, 450 tolerances.  Measured on an MI355X: 1.97e-7 on the CPU, 2.23e-7 on the device (ratio 1.13),
    spread 0.412; 239 launches folded, 311 unfolded, the probabilities and logits equal bit for bit."""
    import torch

    from cpx import _lib
    from cpx.ml_tools import interpreter as ci
    from cpx.ml_tools.tflite_reader import Graph

    blob = tn.nasnet(17, size=64, seed=NASNET_SEED)
    path = write_model(tmp_path, "n", "nasnet", blob)
    g = Graph(blob)
    logits_t = g.ops[-1]["inputs"][0]
    x2 = (raw_samples(3, 64, seed=11) / F32(127.5) - F32(1.0)).astype(F32)
    xd = torch.from_numpy(x2).to(engine.device)
    probs, plans = {}, {}
    for flag in ("1", "0"):
        monkeypatch.setenv("CPX_TFLITE_FOLD_WINDOWS", flag)
        monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT", flag)
        monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT_DW", flag)   # (off by default: slower at N = 1)
        interp = ci.LiteInterpreter(path, engine=engine)
        assert interp.limits_flags() & _lib.LIMITS_TF_SCALING
        probs[flag] = interp.predict(xd)
        plans[flag] = interp._plan((64, 64, 2))[1]
        assert plans[flag].ops[0].kind == _lib.GRAPH_CHANNEL_MAP
    print("NASNet stand-in: %d launches folded, %d unfolded; arena %d and %d floats per sample"
          % (len(plans["1"].ops), len(plans["0"].ops), plans["1"].arena_floats, plans["0"].arena_floats))
    print("folded: %s" % plans["1"].census())
    assert len(plans["1"].ops) < len(plans["0"].ops)
    assert sum(o.kind == _lib.GRAPH_DWCONV_PRE for o in plans["1"].ops) == 35 and sum(o.kind == _lib.GRAPH_SLICE for o in plans["1"].ops) == 8
    assert not any(o.kind in (_lib.GRAPH_DWCONV_PRE, _lib.GRAPH_CONV_PRE) for o in plans["0"].ops)
    assert probs["1"].shape == (3, 17) and np.array_equal(bits(probs["1"]), bits(probs["0"]))
    cmap = interp.channel_map()
    off = dict(fold_windows=False, fuse_preactivation_dw=False, fuse_preactivation=False)
    logits = {f: run(engine, blob, x2, output=logits_t, channel_map=cmap, **(FOLDS if f else off))[2] for f in (True, False)}
    assert np.array_equal(bits(logits[True]), bits(logits[False]))
    x3 = np.ascontiguousarray(x2[..., [0, 0, 1]])
    v64 = ten.evaluate(g, x3)
    v32 = ten.evaluate(g, x3, dtype=torch.float32)
    yard = float(np.abs(v32[logits_t] - v64[logits_t]).max())
    tol = LOGIT_MULTIPLE * yard
    err = float(np.abs(logits[True] - v64[logits_t]).max())
    spread = min(float(np.ptp(v64[logits_t], axis=1).min()), float(np.ptp(v64[logits_t], axis=0).max()))
    print("nasnet: float32-CPU vs float64: %.3g; device vs float64: %.3g (ratio %.2f); spread of the logits %.3g"
          % (yard, err, err / yard, spread))
    assert spread >= 100 * tol, (spread, tol)
    assert err <= tol, (err, yard)
    assert float(np.abs(probs["1"] - v64[g.outputs[0]]).max()) <= 1e-3


# ---- 6. one file end to end ----
def test_clip_classifier_with_a_nasnet_named_model(tmp_path, monkeypatch, engine):
    """test_tflite_preact_gpu.py::test_clip_classifier_with_a_resnet_named_model with a `nasnet`-named ('tf') model of size
    160: the possum fixture tracked, then classified by ClipClassifier's one-file path.  The crop kernel scales the sample
    x / 127.5 - 1 (the oracle chain's at 1e-5, the bound test_tflite_dw_gpu.py holds the scaled sample to); the predictions
    are the float64 evaluator's on the inputs the network was fed, at 1e-3."""
    import classify_oracle as co
    from helpers import GOLDEN
    from cpx import _lib
    from cpx.classify.clipclassifier import ClipClassifier
    from cpx.config import Config
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, get_interpreter
    from cpx.ml_tools.tflite_reader import Graph
    from cpx.track.trackextractor import extract_file

    monkeypatch.delenv("CPX_TFLITE_FUSE_PREACT", raising=False)
    monkeypatch.delenv("CPX_TFLITE_FOLD_WINDOWS", raising=False)
    monkeypatch.setenv("CPX_TFLITE_FUSE_PREACT_DW", "1")   # (off by default; here every new operator runs)
    blob = tn.nasnet(17, size=160, seed=13, head_gain=4.0)
    write_model(tmp_path, "nn", "nasnet", blob)
    g = Graph(blob)
    cfg = Config.get_defaults()
    cfg.tracking["thermal"].denoise = False
    cfg.classify.models = [ModelConfig.load({"id": 9, "name": "nn", "model_file": str(tmp_path / "nn.tflite")})]
    src = tmp_path / "possum.cptv"
    shutil.copy(os.path.join(GOLDEN, "possum.cptv"), src)
    clip, _, _ = extract_file(src, cfg, False, save_meta=False)

    interp = get_interpreter(cfg.classify.models[0])
    assert isinstance(interp, LiteInterpreter) and interp.input_mode is None and interp.channel_map() == [0, 0, 1]
    assert interp.limits_flags() & _lib.LIMITS_TF_SCALING
    plan = interp._plan((160, 160, 2))[1]
    assert plan.ops[0].kind == _lib.GRAPH_CHANNEL_MAP and sum(o.kind == _lib.GRAPH_SLICE for o in plan.ops) == 8
    assert sum(o.kind == _lib.GRAPH_DWCONV_PRE for o in plan.ops) == 35 and sum(o.kind == _lib.GRAPH_PAD for o in plan.ops) == 4

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
        x = (np.asarray(x, F32) / F32(127.5) - F32(1.0)).astype(F32)
        x_fed, fed = np.stack(fed[:len(segs)]), fed[len(segs):]
        probs, answered = np.stack(answered[:len(segs)]), answered[len(segs):]
        assert x_fed.shape == x.shape == (len(segs), 160, 160, 2) and float(np.abs(x_fed - x).max()) <= 1e-5
        want_probs = ten.evaluate(g, np.ascontiguousarray(x_fed[..., [0, 0, 1]]))[g.outputs[0]]
        dev = float(np.abs(probs - want_probs).max())
        print("track %d: the one-file path's probabilities vs the evaluator's on its inputs: %.3g; they spread by %.3g"
              % (tm["id"], dev, float(np.ptp(want_probs, axis=1).min())))
        assert dev <= 1e-3
        score = co.classified_track(probs, prediction_frames=segs, labels=LABELS17)
        got = np.array([pm["all_class_confidences"][l] for l in LABELS17])
        assert np.abs(got - np.round(score, 3)).max() <= 1e-3 + 1e-9
        assert pm["tag"] == LABELS17[int(np.argmax(score))]
    assert not fed and not answered
