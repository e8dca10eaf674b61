"""The EfficientNet family in the TFLite graph executor on the GPU: the fused swish and sigmoid (CPX_GRAPH_ACT_SWISH /
ACT_LOGISTIC) against the unfused launches, bit for bit, and against float64; CPX_GRAPH_MUL (same shape and the [1, 1, C] gate
of a squeeze-and-excite block); MEAN's two summation orders; a whole squeeze-and-excite block and a whole EfficientNet-B0
(tests/tflite_build_se.py), float32 and dynamic-range quantised; get_interpreter with `efficientnetv2b3`.  The flatbuffers are
synthetic and the evaluators read the Graph only (tests/tflite_eval_se.py); parity with the TFLite runtime (ai_edge_litert)
on this family is not pinned here -- the standing the other families have (test_tflite_graph_gpu.py::
test_released_model_parity is the route where the runtime exists)."""
import json
import os
import shutil

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_dw as td
import tflite_build_se as ts
import tflite_eval_se as tes
from test_tflite_graph_gpu import CONV_REL, LABELS17, LOGIT_MULTIPLE, samples

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def run(engine, blob, x, output=None, quantised_math="hybrid", fuse=True, out_slice=None, out=None):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    plan = build_plan(g, input_shape=x.shape[1:], output=output, quantised_math=quantised_math, fuse_activations=fuse)
    dev = GraphDevice(engine, plan, out_slice=out_slice)
    got = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device), out=out).cpu().numpy()
    dev.close()
    return g, plan, got


def kinds(plan):
    from cpx import _lib

    names = {_lib.GRAPH_CONV: "CONV", _lib.GRAPH_CONV_Q8: "CONV_Q8", _lib.GRAPH_DWCONV: "DWCONV", _lib.GRAPH_DWCONV_Q8: "DWCONV_Q8",
             _lib.GRAPH_FC: "FC", _lib.GRAPH_FC_Q8: "FC_Q8", _lib.GRAPH_QUANT_PARAMS: "QUANT_PARAMS", _lib.GRAPH_MUL: "MUL",
             _lib.GRAPH_MEAN: "MEAN", _lib.GRAPH_LOGISTIC: "LOGISTIC", _lib.GRAPH_AFFINE: "AFFINE", _lib.GRAPH_ADD: "ADD",
             _lib.GRAPH_PAD: "PAD", _lib.GRAPH_MAX_POOL: "MAX_POOL", _lib.GRAPH_AVG_POOL: "AVG_POOL", _lib.GRAPH_SOFTMAX: "SOFTMAX",
             _lib.GRAPH_CHANNEL_MAP: "CHANNEL_MAP"}
    return [names[o.kind] for o in plan.ops]


def conv_w(rng, co, k, cin):
    return (rng.normal(0, np.sqrt(2.0 / (k * k * cin)), size=(co, k, k, cin)).astype(F32), rng.normal(0, 0.05, size=co).astype(F32))


def dw_w(rng, k, c):
    return rng.normal(0, np.sqrt(2.0 / (k * k)), size=(1, k, k, c)).astype(F32), rng.normal(0, 0.05, size=c).astype(F32)


# ---- 1. fused equals unfused, bit for bit; fused against float64 ----
ACT_CASES = [
    # kind, k, stride, cin, cout, size, quantised
    ("conv", 3, 1, 16, 40, 9, False),
    ("dw", 5, 2, 36, 36, 8, False),
    ("dw", 3, 1, 6, 6, 9, False),      # channel by channel
    ("conv", 1, 1, 64, 32, 5, True),
    ("dw", 3, 1, 144, 144, 9, True),
]


def act_graph(case, tail):
    """input -> CONV_2D | DEPTHWISE_CONV_2D -> swish | LOGISTIC -> output; -> (blob, the convolution's output tensor)."""
    kind, k, stride, cin, cout, size, quantised = case
    rng = np.random.default_rng(k * 100 + stride + cin + cout + size)
    m = ts.ModelSE()
    x = m.tensor([1, size, size, cin], name="input")
    m.inputs = [x]
    y = m.conv(x, *conv_w(rng, cout, k, cin), stride, tb.SAME, tb.NONE) if kind == "conv" else \
        m.depthwise(x, *dw_w(rng, k, cin), stride, tb.SAME, tb.NONE)
    m.outputs = [m.swish(y) if tail == "swish" else m.unary("LOGISTIC", y)]
    blob = m.finish()
    return (td.quantise(blob, min_elements=0) if quantised else blob), y, rng


def act_id(c):
    return "%s%d_s%d_%dto%d_at%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "_q8" if c[6] else "")


@pytest.mark.parametrize("tail", ["swish", "logistic"])
@pytest.mark.parametrize("case", ACT_CASES, ids=act_id)
def test_fused_activation_equals_the_launches_and_float64(engine, case, tail):
    """Bit for bit because logistic() of csrc/cpx_graph_core.h is one inline function, called by activate() and by
    graph_logistic_kernel, and the build has -ffp-contract=off.  Against float64 (the float32 cases): a swish has slope
    <= 1.1, so the convolution's error CONV_REL x mag passes with that factor, plus about 4 ulp of the sigmoid chain on a
    value below |v| <= mag: 1.25 x CONV_REL x mag in all.  A sigmoid has slope <= 1 / 4 and its own chain rounds a value
    below 1 four times."""
    from cpx.ml_tools.tflite_graph import ACT_LOGISTIC, ACT_SWISH

    blob, y, rng = act_graph(case, tail)
    x = rng.uniform(-3, 3, size=(3, case[5], case[5], case[3])).astype(F32)
    g, plan, fused = run(engine, blob, x)
    _, plain, unfused = run(engine, blob, x, fuse=False)
    assert plan.ops[-1].act == (ACT_SWISH if tail == "swish" else ACT_LOGISTIC) and len(plain.ops) == len(plan.ops) + (2 if tail == "swish" else 1)
    assert kinds(plain)[-1] == ("MUL" if tail == "swish" else "LOGISTIC") and all(o.act == 0 for o in plain.ops)
    print("%s %s: %d of %d elements differ between fused and unfused" % (act_id(case), tail, int((fused != unfused).sum()), fused.size))
    assert np.array_equal(fused.view(np.uint32), unfused.view(np.uint32))
    assert float(np.abs(fused).max()) > 0.1 and np.all(np.isfinite(fused))
    if case[6]:
        return
    vals, mag = tes.evaluate(g, x, magnitudes=True)
    err = np.abs(fused - vals[g.outputs[0]])
    if tail == "swish":
        rel = float((err / mag[y]).max())
        print("max |error| / mag = %.3g (bound %.3g)" % (rel, 1.25 * CONV_REL))
        assert rel < 1.25 * CONV_REL
    else:
        over = float((err - (0.25 * CONV_REL * mag[y] + 4 * 2.0 ** -24)).max())
        print("max |error| = %.3g; largest excess over the bound %.3g" % (float(err.max()), over))
        assert over <= 0.0


# ---- 2. MUL ----
def mul_graph(c, size=5, gate=None, slices=False):
    """a = RELU6(input), b = the [1, 1, C] MAX_POOL_2D of the input over the whole map (gate: 'second' | 'first') or
    RELU(input) (gate None): both are exact on the device, so the product is known to the bit.  slices: a lives at channel
    3 of a concatenation."""
    rng = np.random.default_rng(c + size)
    m = ts.ModelSE()
    x = m.tensor([1, size, size, c], name="input")
    m.inputs = [x]
    a = m.unary("RELU6", x)
    if slices:
        m.concat([m.conv(x, *conv_w(rng, 3, 1, c), 1, tb.SAME, tb.NONE), a])
    b = m.unary("RELU", x) if gate is None else m.pool("MAX_POOL_2D", x, size, 1, tb.VALID)
    m.outputs = [m.mul(b, a) if gate == "first" else m.mul(a, b)]
    return m.finish(), a


def mul_want(x, gate):
    a = np.clip(x, 0, 6).astype(np.float64)
    b = np.maximum(x, 0).astype(np.float64) if gate is None else x.max(axis=(1, 2), keepdims=True).astype(np.float64)
    return a * b   # exact in float64


def check_mul(got, x, gate, what):
    want = mul_want(x, gate)
    ulp = np.spacing(np.abs(want).astype(F32)).astype(np.float64)
    err = float((np.abs(got.astype(np.float64) - want) / ulp).max())
    print("%s: largest error %.2f ulp, %d of %d elements are not the correctly rounded product"
          % (what, err, int((got != want.astype(F32)).sum()), got.size))
    assert got.shape == want.shape and err <= 1.0 and float(np.abs(got).max()) > 1.0


@pytest.mark.parametrize("gate", [None, "second", "first"], ids=["same_shape", "gate_second", "gate_first"])
@pytest.mark.parametrize("c", [32, 30, 3])
def test_mul_against_float64(engine, c, gate):
    from cpx import _lib

    blob, _ = mul_graph(c, gate=gate)
    x = np.random.default_rng(c).uniform(-4, 8, size=(3, 5, 5, c)).astype(F32)
    _, plan, got = run(engine, blob, x)
    mul = plan.ops[-1]
    assert kinds(plan)[-1] == "MUL" and mul.kind == _lib.GRAPH_MUL
    assert (plan.tensors[mul.in1].H == 1) == (gate is not None) and plan.tensors[mul.in0].H == 5
    check_mul(got, x, gate, "C = %d, %s" % (c, gate))


@pytest.mark.parametrize("off,extra,slices", [(8, 4, False), (5, 38, True)], ids=["quads", "element_by_element"])
@pytest.mark.parametrize("gate", [None, "second"], ids=["same_shape", "gate"])
def test_mul_in_concatenation_slices_leaves_the_neighbours_alone(engine, gate, off, extra, slices):
    """in0 at channel 3 of a concatenation and the output at channel 5 of rows of 5 + C + 38 channels of a buffer filled
    with a sentinel (element by element); dense in0 and a slice at channel 8 of rows of 8 + C + 4 keep the 16-byte path."""
    import torch

    c = 24
    blob, a = mul_graph(c, gate=gate, slices=slices)
    x = np.random.default_rng(off).uniform(-4, 8, size=(3, 5, 5, c)).astype(F32)
    sentinel = F32(-12345.678)
    out = torch.full((3, 5, 5, off + c + extra), float(sentinel), dtype=torch.float32, device=engine.device)
    _, plan, got = run(engine, blob, x, out_slice=(off, off + c + extra), out=out)
    assert (plan.tensors[a].c_offset, plan.tensors[a].c_stride) == ((3, 3 + c) if slices else (0, c)) and not plan.copies()
    check_mul(got[..., off:off + c], x, gate, "slice at %d" % off)
    assert np.all(got[..., :off] == sentinel) and np.all(got[..., off + c:] == sentinel)


@pytest.mark.parametrize("c", [32, 30])
def test_mul_batch_does_not_matter(engine, c):
    blob, _ = mul_graph(c, size=7, gate="second")   # 49 pixels: workgroups cross samples
    x = np.random.default_rng(c + 1).uniform(-4, 8, size=(1, 7, 7, c)).astype(F32)
    _, _, one = run(engine, blob, x)
    _, _, five = run(engine, blob, np.repeat(x, 5, axis=0))
    assert all(np.array_equal(five[k], one[0]) for k in range(5)) and float(np.abs(one).max()) > 1.0


# ---- 3. MEAN: the serial order below 256 pixels, the striped one from there on ----
def mean_graph(c, h, w, sliced=False):
    m = ts.ModelSE()
    x = m.tensor([1, h, w, c], name="input")
    m.inputs = [x]
    a = x
    if sliced:   # RELU(input) at channel 3 of a concatenation
        a = m.unary("RELU", x)
        m.concat([m.conv(x, *conv_w(np.random.default_rng(1), 3, 1, c), 1, tb.SAME, tb.NONE), a])
    m.outputs = [m.mean(a)]
    return m.finish(), a


def serial_mean(x):
    """include/cpx.h, CPX_GRAPH_MEAN below 256 pixels: one float32 chain over the pixels in raster order."""
    flat = x.reshape(x.shape[0], -1, x.shape[3]).astype(F32)
    s = np.zeros((x.shape[0], x.shape[3]), F32)
    for i in range(flat.shape[1]):
        s = (s + flat[:, i]).astype(F32)
    return (s / F32(flat.shape[1])).astype(F32)


def striped_mean(x):
    """... from 256 pixels on: stripe i of 64 sums the pixels i, i + 64, ... in that order; the tree s[i] += s[i + d], d = 32 .. 1."""
    flat = x.reshape(x.shape[0], -1, x.shape[3]).astype(F32)
    hw = flat.shape[1]
    s = np.zeros((64, x.shape[0], x.shape[3]), F32)
    for i in range(hw):
        s[i % 64] = (s[i % 64] + flat[:, i]).astype(F32)
    d = 32
    while d >= 1:
        s[:d] = (s[:d] + s[d:2 * d]).astype(F32)
        d //= 2
    return (s[0] / F32(hw)).astype(F32)


MEAN_MAPS = [(15, 17), (16, 16), (17, 17), (23, 13)]   # 255 (the serial kernel), 256, 289 and 299 pixels


@pytest.mark.parametrize("c,sliced", [(32, False), (30, False), (3, False), (32, True)], ids=["c32", "c30", "c3", "c32_in_a_slice"])
@pytest.mark.parametrize("h,w", MEAN_MAPS, ids=["255px", "256px", "289px", "23x13"])
def test_mean_both_orders(engine, h, w, c, sliced):
    """Against float64: within CONV_REL x mean |x| per channel (a chain of n float32 additions of values around 1 errs by a
    few 2^-24 on the mean); against the order include/cpx.h states, restated in NumPy float32: bit for bit, the serial
    order at 255 pixels, the striped one from 256 on; N = 1 against N = 5: identical bits."""
    blob, a = mean_graph(c, h, w, sliced)
    x = np.random.default_rng(h * w + c).uniform(-1, 3, size=(5, h, w, c)).astype(F32)
    x[1:] = x[:1]
    x[4] = np.random.default_rng(c).uniform(-2, 2, size=(h, w, c))
    _, plan, got = run(engine, blob, x)
    assert kinds(plan)[-1] == "MEAN" and got.shape == (5, c)
    if sliced:
        assert (plan.tensors[a].c_offset, plan.tensors[a].c_stride) == (3, 3 + c)
    seen = np.maximum(x, 0) if sliced else x
    want = seen.astype(np.float64).mean(axis=(1, 2))
    scale = np.abs(seen).astype(np.float64).mean(axis=(1, 2))
    rel = float((np.abs(got - want) / scale).max())
    print("%d x %d x %d: max |error| / mean |x| = %.3g" % (h, w, c, rel))
    assert rel <= CONV_REL
    restated = serial_mean(seen) if h * w < 256 else striped_mean(seen)
    assert np.array_equal(got.view(np.uint32), restated.view(np.uint32)), int((got != restated).sum())
    _, _, one = run(engine, blob, x[:1])
    assert all(np.array_equal(got[k], one[0]) for k in range(4)) and not np.array_equal(got[4], one[0])


# ---- 4. a whole squeeze-and-excite block ----
def se_block(c, size, reshape, gate_first):
    rng = np.random.default_rng(c + size)
    m = ts.ModelSE()
    x = m.tensor([1, size, size, c], name="input")
    m.inputs = [x]
    y = m.swish(m.depthwise(x, *dw_w(rng, 3, c), 1, tb.SAME, tb.NONE))
    g = m.reshape(m.mean(y), [1, 1, 1, c]) if reshape else m.mean(y, keep_dims=True)
    g = m.swish(m.conv(g, *conv_w(rng, c // 4, 1, c), 1, tb.SAME, tb.NONE))
    g = m.unary("LOGISTIC", m.conv(g, *conv_w(rng, c, 1, c // 4), 1, tb.SAME, tb.NONE))
    m.outputs = [m.conv(m.mul(g, y) if gate_first else m.mul(y, g), *conv_w(rng, 16, 1, c), 1, tb.SAME, tb.NONE)]
    return m.finish()


@pytest.mark.parametrize("c,size,reshape,gate_first", [(96, 17, False, False), (40, 9, True, True)], ids=["wide_mean", "reshape_gate_first"])
def test_squeeze_and_excite_block(engine, c, size, reshape, gate_first):
    """depthwise + swish -> MEAN -> 1 x 1 (swish) -> 1 x 1 -> LOGISTIC -> MUL by the gate -> projection, held to float64 by
    the whole-network criterion: LOGIT_MULTIPLE times what a float32 evaluation of the same graph on the CPU deviates."""
    import torch

    blob = se_block(c, size, reshape, gate_first)
    x = np.random.default_rng(size).uniform(-2, 2, size=(3, size, size, c)).astype(F32)
    g, plan, got = run(engine, blob, x)
    assert kinds(plan) == ["DWCONV", "MEAN", "CONV", "CONV", "MUL", "CONV"]
    _, _, unfused = run(engine, blob, x, fuse=False)
    assert np.array_equal(got, unfused)
    v64, v32 = tes.evaluate(g, x), tes.evaluate(g, x, dtype=torch.float32)
    t = g.outputs[0]
    yard, err = float(np.abs(v32[t] - v64[t]).max()), float(np.abs(got - v64[t]).max())
    print("float32-CPU vs float64: %.3g; device vs float64: %.3g (ratio %.2f); values up to %.3g" % (yard, err, err / yard, np.abs(v64[t]).max()))
    assert err <= LOGIT_MULTIPLE * yard and float(np.abs(v64[t]).max()) > 1.0


# ---- 5. a whole EfficientNet-B0 ----
# Width 0.25 at 64 x 64, N = 3, 17 labels; seed and head_gain are chosen so that the float64 logits alone meet
# spread >= 100 x tolerance (checked on the CPU: float32 deviates from float64 by 6.9e-7, the logits spread by 0.32).
# Measured on an MI355X: the device deviates from float64 by 3.87e-7 -- ratio 0.57; the quantised twin: hybrid against float
# math on the device 0.0214, the restatement against float64 of the dequantised graph 0.0214, the device 5.96e-8 from the
# restatement; float math 4.11e-7 from float64 where float32 on the CPU is 3.66e-7.
B0_SEED, B0_HEAD_GAIN = 7, 4.0


def b0_inputs():
    return ((samples(3, 64, seed=11) + 1.0) * 127.5).astype(F32)   # 0 .. 255: the model rescales and normalises itself


def test_efficientnet_b0_whole_network(engine):
    """The method of test_tflite_graph_gpu.py::test_inception_v3_whole_network."""
    import torch

    from cpx.ml_tools.tflite_reader import Graph

    blob = ts.efficientnet_b0(17, (), seed=B0_SEED, width=0.25, size=64, head_gain=B0_HEAD_GAIN)
    x = b0_inputs()
    g = Graph(blob)
    logits_t = g.ops[-1]["inputs"][0]
    v64, v32 = tes.evaluate(g, x), tes.evaluate(g, x, dtype=torch.float32)
    yard = float(np.abs(v32[logits_t] - v64[logits_t]).max())
    tol = LOGIT_MULTIPLE * yard
    _, plan, logits = run(engine, blob, x, output=logits_t)
    assert kinds(plan).count("MUL") == 16 and kinds(plan).count("LOGISTIC") == 0 and kinds(plan).count("DWCONV") == 16
    _, plain, unfused = run(engine, blob, x, output=logits_t, fuse=False)
    assert kinds(plain).count("LOGISTIC") == 65 and np.array_equal(logits, unfused)   # fused against unfused: bit-equal
    _, _, probs = run(engine, blob, x)
    err = float(np.abs(logits - v64[logits_t]).max())
    spread = min(float(np.ptp(v64[logits_t], axis=1).min()), float(np.ptp(v64[logits_t], axis=0).max()))
    print("float32-CPU vs float64: %.3g; device vs float64: %.3g (ratio %.2f); spread of the logits %.3g" % (yard, err, err / yard, spread))
    assert spread >= 100 * tol, (spread, tol)
    assert err <= tol, (err, yard)
    assert float(np.abs(probs - v64[g.outputs[0]]).max()) <= 1e-3
    # the converter's other layout (DIV, MEAN + RESHAPE) runs to the same values: 1 / sd as a DIV is the same float32 scale
    other = ts.efficientnet_b0(17, (), seed=B0_SEED, width=0.25, size=64, head_gain=B0_HEAD_GAIN, normalisation_div=True, se_reshape=True)
    _, _, logits_o = run(engine, other, x, output=Graph(other).ops[-1]["inputs"][0])
    assert float(np.abs(logits_o - v64[logits_t]).max()) <= tol


def test_quantised_efficientnet_b0_whole_network(engine):
    """Dynamic-range quantised (td.quantise: filters of 1024 elements or more INT8).  The criterion of
    test_tflite_q8_gpu.py::test_inception_v3_whole_network for the two arithmetics: the hybrid run may differ from the
    quantised_math="float" run by twice what the hybrid restatement differs from float64 of the dequantised graph (the
    quantisation noise itself); the float run is held to float64 as the float32 network is.  Fused against unfused: bit-equal."""
    import torch

    from cpx.ml_tools.tflite_reader import Graph

    blob = td.quantise(ts.efficientnet_b0(17, (), seed=B0_SEED, width=0.25, size=64, head_gain=B0_HEAD_GAIN))
    x = b0_inputs()
    g = Graph(blob)
    logits_t = g.ops[-1]["inputs"][0]
    hyb, _ = tes.evaluate_hybrid(g, x)
    deq64, deq32 = tes.evaluate_dequantised(g, x), tes.evaluate_dequantised(g, x, dtype=torch.float32)
    yard = float(np.abs(hyb[logits_t] - deq64[logits_t]).max())
    _, plan, logits = run(engine, blob, x, output=logits_t)
    n_q8 = sum(g.quantised_filter(op) is not None for op in g.ops)
    assert kinds(plan).count("CONV_Q8") + kinds(plan).count("DWCONV_Q8") + kinds(plan).count("FC_Q8") == n_q8 > 20
    _, _, unfused = run(engine, blob, x, output=logits_t, fuse=False)
    assert np.array_equal(logits, unfused)
    _, fplan, flogits = run(engine, blob, x, output=logits_t, quantised_math="float")
    assert not {"CONV_Q8", "DWCONV_Q8", "FC_Q8", "QUANT_PARAMS"} & set(kinds(fplan))
    other = float(np.abs(flogits - logits).max())
    fyard, ferr = float(np.abs(deq32[logits_t] - deq64[logits_t]).max()), float(np.abs(flogits - deq64[logits_t]).max())
    print("hybrid restatement vs float64 of the dequantised graph: %.4g; hybrid vs float math on the device: %.4g; device vs the "
          "restatement: %.4g; float math: float32-CPU vs float64 %.3g, device vs float64 %.3g"
          % (yard, other, float(np.abs(logits - hyb[logits_t]).max()), fyard, ferr))
    assert other <= 2 * yard, (other, yard)
    assert ferr <= LOGIT_MULTIPLE * fyard, (ferr, fyard)


# ---- 6. through the public interface ----
@pytest.fixture(scope="module")
def effnet_model(tmp_path_factory):
    """A width-0.25 EfficientNet-B0-shaped file + sidecar under the reference's `efficientnetv2b3` name: no input scaling,
    three input channels fed from the two-channel sample by the channel map."""
    from helpers import GOLDEN

    d = tmp_path_factory.mktemp("effnet")
    with open(os.path.join(GOLDEN, "classify_variants_golden.json")) as fh:
        golden = json.load(fh)
    assert golden["labels"] == LABELS17
    hp = {"frame_size": 32, "model_name": "efficientnetv2b3", "channels": ["thermal", "thermal", "filtered"]}
    blob = ts.efficientnet_b0(len(LABELS17), (), seed=13, width=0.25, size=160, head_gain=4.0)
    (d / "effnet.tflite").write_bytes(blob)
    with open(d / "effnet.json", "w") as fh:
        json.dump({"labels": LABELS17, "hyperparams": hp, "type": "thermal", "version": "test"}, fh)
    with open(d / "wr.json", "w") as fh:
        json.dump({"labels": LABELS17, "hyperparams": {"frame_size": 32}, "type": "thermal", "version": "test"}, fh)
    return d, blob, golden["variants"]["inceptionv3_scaling"]


def test_get_interpreter_with_an_efficientnet(tmp_path, effnet_model):
    """The possum fixture tracked and classified through get_interpreter: a LiteInterpreter, its inputs the unscaled samples a
    wr-resnet interpreter gets for the same segments, its predictions the float64 evaluator's on those inputs at 1e-3; the
    batched many-file path gives the same predictions."""
    from cpx import _lib
    from cpx.classify.clipclassifier import ClipClassifier
    from cpx.config import Config
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, WRResNetInterpreter, get_interpreter
    from cpx.ml_tools.tflite_reader import Graph
    from cpx.track.trackextractor import extract_file
    from helpers import GOLDEN

    d, blob, gold = effnet_model
    g = Graph(blob)
    cfg = Config.get_defaults()
    cfg.tracking["thermal"].denoise = False
    cfg.classify.models = [ModelConfig.load({"id": 9, "name": "effnet", "model_file": str(d / "effnet.tflite")})]
    src = tmp_path / "possum.cptv"
    shutil.copy(os.path.join(GOLDEN, "possum.cptv"), src)
    clip, _, _ = extract_file(src, cfg, False, save_meta=False)

    interp = get_interpreter(cfg.classify.models[0])
    assert isinstance(interp, LiteInterpreter) and interp.preprocess_fn is None and not interp.limits_flags() & _lib.LIMITS_TF_SCALING
    plan = next(iter(interp._plans.values()))
    assert sum(o.kind == _lib.GRAPH_MUL for o in plan.ops) == 16 and sum(o.act == _lib.GRAPH_ACT_SWISH for o in plan.ops) == 49
    plain = WRResNetInterpreter(d / "wr.npz", load_model=False)
    seen = {}

    def capture(key, answer):
        def predict(x):
            seen[key] = x.cpu().numpy()
            return answer(x)
        return predict

    interp.predict = capture("lite", interp.predict)
    plain.predict = capture("wr", lambda x: np.full((int(x.shape[0]), len(LABELS17)), 0.5, np.float32))
    assert len(clip.tracks) == len(gold["possum"]) > 0
    by_track = {}
    for track, want in zip(clip.tracks, gold["possum"]):
        segs = [np.array(s) for s in want["segments"]]
        pred = interp.classify_track(clip, track, segment_frames=segs)
        plain.classify_track(clip, track, segment_frames=segs)
        x = seen["lite"]
        assert list(x.shape) == want["shape"] and np.array_equal(x, seen["wr"]) and float(x.max()) > 100.0   # unscaled
        probs = tes.evaluate(g, np.ascontiguousarray(x[..., [0, 0, 1]]))[g.outputs[0]]
        got = np.array([p.prediction for p in pred.predictions], dtype=np.float64)
        print("track %d: predictions vs the float64 evaluator's: %.3g" % (track.get_id(), float(np.abs(got - probs).max())))
        assert got.shape == probs.shape and float(np.abs(got - probs).max()) <= 1e-3
        assert float(np.ptp(probs, axis=1).min()) > 0.1     # the labels are told apart by far more than the tolerance
        by_track[track.get_id()] = track
    # ---- the batched many-file path ----
    dd = tmp_path / "batched"
    dd.mkdir()
    shutil.copy(os.path.join(GOLDEN, "possum.cptv"), dd / "possum.cptv")
    cc = ClipClassifier(cfg)
    cc.process(str(dd), track=True)
    assert cc.last_run is not None and cc.last_run["files"] == 1
    with open(dd / "possum.txt") as fh:
        meta = json.load(fh)
    assert len(meta["tracks"]) == len(clip.tracks)
    for tm in meta["tracks"]:
        (pm,) = tm["predictions"]
        segs = [np.array(p["frames"]) for p in pm["predictions"]]
        pred = interp.classify_track(clip, by_track[tm["id"]], segment_frames=segs)
        got = np.array([pm["all_class_confidences"][l] for l in LABELS17])
        assert np.abs(got - np.round(np.array(pred.class_best_score, np.float64), 3)).max() <= 1e-3 + 1e-9
        assert pm["tag"] == LABELS17[int(np.argmax(pred.class_best_score))]
