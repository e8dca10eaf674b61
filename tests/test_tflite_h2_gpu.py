"""The fp16x2 convolution math of the TFLite graph executor on the GPU (build_plan(conv_math="fp16x2"): RANGE and
CONV_F16X2, csrc/cpx_graph_h2.hip): against the NumPy restatement of include/cpx.h's arithmetic (tests/tflite_eval_h2.py),
bit for bit where every partial sum is exact, and against the float64 evaluation of the same flatbuffer
(tests/tflite_eval.py) beside the exact-float32 kernel (conv_math="f32") on the same case."""
import json
import os

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_se as ts
import tflite_eval as te
import tflite_eval_h2 as th

pytestmark = pytest.mark.gpu

F32 = np.float32
# float32 accumulation against the accumulated magnitude sum |x| |w|: the project's bound for float32-accurate
# convolutions (tests/test_tflite_graph_gpu.py, tests/test_cnn_gpu.py)
CONV_REL = 4e-6
# the whole-network yardstick of tests/test_tflite_graph_gpu.py: the device may deviate from float64 by this multiple of
# what a float32 evaluation of the same graph on the CPU does
LOGIT_MULTIPLE = 4.0


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def run(engine, blob, x, output=None, conv_math="fp16x2", **kw):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    plan = build_plan(g, input_shape=x.shape[1:], output=output, conv_math=conv_math, **kw)
    dev = GraphDevice(engine, plan)
    out = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device)).cpu().numpy()
    dev.close()
    return g, plan, out


def conv_graph(w, bias, stride, padding, size, act=tb.NONE):
    m = tb.Model()
    x = m.tensor([1, size, size, w.shape[3]], name="input")
    m.inputs = [x]
    m.outputs = [m.conv(x, w, bias, stride, padding, act)]
    return m.finish()


def he_normal(rng, cout, kh, kw, cin):
    return rng.normal(0, np.sqrt(2.0 / (kh * kw * cin)), size=(cout, kh, kw, cin)).astype(F32)


def pads_of(size, kh, kw, stride, padding):
    (pt, pb), (pl, pr) = te._pads(size, kh, stride, padding), te._pads(size, kw, stride, padding)
    return pt, pl, pb, pr


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- operand map, exact ----
@pytest.mark.parametrize("cout", [32, 80])
@pytest.mark.parametrize("kh,kw,cin", [(3, 3, 32), (1, 1, 288), (1, 7, 40)])
def test_operand_map_exact(engine, kh, kw, cin, cout):
    """Operands from small integers, K = taps * Cin <= 288.  Activations x = a + b * 2^-12 with |a| in {1, 2, 3} and b of
    a's sign, |b| <= 3 (<= 1 beside |a| = 1): a sample's range is 2^13, so xs = a * 2^13 + 2 b splits into xh = a * 2^13
    and xl = 2 b with no tie.  Weights 2^-6 * (4 a' + b' * 2^-10) with |a'| in {2, 3} and b' of a's sign, |b'| <= 3: the
    scaled weight lies in [8, 16), wh = 4 a' and wl = b' * 2^-10.  Every product is a multiple of 8 and every partial sum
    stays below 288 * (36 * 2^13 + 144) < 2^27: 24 bits, exact in float32 in any order.  The device must equal the
    restatement BIT FOR BIT -- a wrong fragment order, a swapped plane, a wrong k half or a dropped low plane moves the sum."""
    assert kh * kw * cin <= 288
    rng = np.random.default_rng(kh * 1000 + kw * 100 + cin + cout)
    size, n = 6, 2
    shape = (n, size, size, cin)
    mag_a = rng.integers(1, 4, size=shape)
    mag_a[:, 0, 0, 0] = 3   # every sample's largest magnitude is in [2, 4): up = 2^13
    sign = rng.choice(np.array([-1, 1]), size=shape)
    mag_b = rng.integers(0, 4, size=shape) % np.where(mag_a == 1, 2, 4)
    x = (sign * (mag_a + mag_b * 2.0 ** -12)).astype(F32)
    shape = (cout, kh, kw, cin)
    a = rng.integers(2, 4, size=shape) * rng.choice(np.array([-1, 1]), size=shape)
    b = rng.integers(0, 4, size=shape) * np.sign(a)
    w = ((4.0 * a + b * 2.0 ** -10) * 2.0 ** -6).astype(F32)
    bias = (rng.integers(-16, 17, size=cout) / 8.0).astype(F32)
    pads = pads_of(size, kh, kw, 1, tb.SAME)
    want, parts = th.conv(x, w, (1, 1), pads, shift=bias, parts=True)
    assert np.all(parts["up"] == 2.0 ** 13) and np.all(parts["kw"] == 6)
    f64 = np.float64
    # the two planes hold the operand without loss, and the low one is in use
    assert np.array_equal(parts["xh"].astype(f64), sign * mag_a * 2.0 ** 13) and np.array_equal(parts["xl"].astype(f64), sign * mag_b * 2.0)
    assert np.array_equal(parts["wh"].astype(f64), 4.0 * a) and np.array_equal(parts["wl"].astype(f64), b * 2.0 ** -10)
    assert np.any(parts["xl"] != 0) and np.any(parts["wl"] != 0)
    assert np.array_equal(parts["acc"], parts["acc"].astype(F32).astype(np.float64)) and np.abs(parts["acc"]).max() < 2.0 ** 27
    high_only = th._conv64(parts["xh"], parts["wh"], (1, 1), pads)
    assert np.any(high_only != parts["acc"])   # the low planes carry part of every sum
    _, plan, got = run(engine, conv_graph(w, bias, 1, tb.SAME, size), x)
    assert [o.name for o in plan.ops] == ["RANGE", "CONV_2D"]
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))


# ---- against float64, beside the exact-float32 kernel ----
CONV_CASES = [
    # kh, kw, stride, padding, cin, cout, size
    (1, 1, 1, tb.SAME, 192, 80, 8),
    (1, 1, 2, tb.VALID, 48, 80, 17),
    (3, 3, 2, tb.VALID, 3, 32, 19),
    (3, 3, 1, tb.SAME, 32, 48, 17),
    (5, 5, 2, tb.SAME, 3, 48, 17),
    (1, 7, 1, tb.SAME, 80, 96, 17),
    (7, 1, 2, tb.SAME, 32, 3, 8),
    (3, 1, 1, tb.SAME, 288, 64, 3),
]
SAME_3X3 = CONV_CASES[3]
CASES = [(c, "uniform") for c in CONV_CASES] + [(SAME_3X3, f) for f in th.FAMILIES if f != "uniform"]


def both_maths(engine, case, x, seed):
    """-> (rel(fp16x2), rel(f32), the fp16x2 output): max |error| / sum |x||w| of the two maths on one case."""
    kh, kw, stride, padding, cin, cout, size = case
    rng = np.random.default_rng(seed)
    w = he_normal(rng, cout, kh, kw, cin)
    blob = conv_graph(w, None, stride, padding, size)   # no bias: the scale below is sum |x||w| and nothing else
    g, _, got = run(engine, blob, x)
    _, plan32, got32 = run(engine, blob, x, conv_math="f32")
    assert [o.name for o in plan32.ops] == ["CONV_2D"]
    vals, mag = te.evaluate(g, x, magnitudes=True)
    want, scale = vals[g.outputs[0]], mag[g.outputs[0]]
    assert got.shape == want.shape and np.all(np.isfinite(got))
    return float((np.abs(got - want) / scale).max()), float((np.abs(got32 - want) / scale).max()), got


@pytest.mark.parametrize("case,family", CASES, ids=lambda v: v if isinstance(v, str) else "%dx%d_s%d_%s_%dto%d_at%d" % (
    v[0], v[1], v[2], "SV"[v[3]], v[4], v[5], v[6]))
def test_convolution_against_float64(engine, case, family):
    kh, kw, stride, padding, cin, cout, size = case
    rng = np.random.default_rng(kh * 100 + kw * 10 + stride + cin + cout + size)
    x = th.families(rng, (2, size, size, cin))[family].astype(F32)
    rel, rel32, _ = both_maths(engine, case, x, seed=cin + cout)
    print("%s %s: max |error| / sum |x||w|: fp16x2 %.3g, f32 %.3g" % (case, family, rel, rel32))
    assert rel < CONV_REL, rel
    assert rel <= 2 * rel32 + 2.0 ** -24, (rel, rel32)


def test_range_keeps_a_scaled_sample_finite(engine):
    """A sample scaled by 1e6 beside an ordinary one: fp16 alone holds neither the products nor the sample."""
    rng = np.random.default_rng(77)
    kh, kw, stride, padding, cin, cout, size = SAME_3X3
    x = rng.uniform(-1, 1, size=(2, size, size, cin)).astype(F32)
    x[1] *= F32(1e6)
    rel, rel32, got = both_maths(engine, SAME_3X3, x, seed=5)
    print("scaled: max |error| / sum |x||w|: fp16x2 %.3g, f32 %.3g; largest |output| %.3g" % (rel, rel32, float(np.abs(got).max())))
    assert np.all(np.isfinite(got)) and rel < CONV_REL, rel


def test_range_keeps_a_spike_finite(engine):
    """One sample carries a single 3e38 among values of +-1.  RANGE scales a sample by ONE power of two, so that sample's
    other elements, 2^-128 of its largest, fall out of both planes (include/cpx.h; elements below 2^-18 of the largest
    lose their low plane): an output whose window misses the spike comes out as its bias.  Element by element that
    sample's max |error| / sum |x||w| is therefore about 0.4 by construction (0.43 in the NumPy restatement), and the
    bound that the arithmetic can be held to is CONV_REL of the SAMPLE's largest sum |x||w|.  Held element by element:
    the outputs whose window holds the spike, and the whole of the ordinary sample beside it (nothing leaks across
    samples).  Everything is finite."""
    rng = np.random.default_rng(77)
    kh, kw, stride, padding, cin, cout, size = SAME_3X3
    x = rng.uniform(-1, 1, size=(2, size, size, cin)).astype(F32)
    x[1, 5, 7, 3] = F32(3e38)
    w = he_normal(rng, cout, kh, kw, cin)
    bias = rng.normal(0, 0.05, size=cout).astype(F32)
    blob = conv_graph(w, bias, stride, padding, size)
    g, _, got = run(engine, blob, x)
    _, _, got32 = run(engine, blob, x, conv_math="f32")
    vals, mag = te.evaluate(g, x, magnitudes=True)
    want, scale = vals[g.outputs[0]], mag[g.outputs[0]]
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(got32))
    each = np.abs(got - want) / scale
    each32 = np.abs(got32 - want) / scale
    whole = float(np.abs(got[1] - want[1]).max() / scale[1].max())
    print("spike: max |error| / sum |x||w| element by element: ordinary sample fp16x2 %.3g (f32 %.3g), spike's window %.3g "
          "(f32 %.3g), spike's sample %.3g (f32 %.3g); against the sample's largest sum: %.3g"
          % (each[0].max(), each32[0].max(), each[1, 4:7, 6:9].max(), each32[1, 4:7, 6:9].max(), each[1].max(), each32[1].max(), whole))
    assert float(each[0].max()) < CONV_REL and float(each[1, 4:7, 6:9].max()) < CONV_REL
    assert whole < CONV_REL


def test_a_tile_that_crosses_samples_takes_each_samples_range(engine):
    """Three samples of ranges 1, 1e3 and 1e-3 on an 8 x 8 map: 192 pixels in tiles of 128, so the second tile starts in
    the middle of sample 1 and a wave's 32 rows hold two samples.  Every sample's output is, bit for bit, its output at N = 1."""
    rng = np.random.default_rng(41)
    w = he_normal(rng, 48, 3, 3, 32)
    blob = conv_graph(w, rng.normal(0, 0.05, size=48).astype(F32), 1, tb.SAME, 8)
    x = rng.uniform(-1, 1, size=(3, 8, 8, 32)).astype(F32)
    x[1] *= F32(1e3)
    x[2] *= F32(1e-3)
    _, _, all3 = run(engine, blob, x)
    ups = [float(th.range_params(s)[0]) for s in x]
    assert len(set(ups)) == 3
    for k in range(3):
        _, _, one = run(engine, blob, x[k:k + 1])
        assert np.array_equal(bits(all3[k]), bits(one[0])), k
    want, mag = th.conv_float64(x, w, pads=(1, 1, 1, 1))
    assert float((np.abs(all3 - np.asarray(blob_bias(blob)) - want) / mag).max()) < CONV_REL


def blob_bias(blob):
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    return g.const(g.ops[0]["inputs"][2]).astype(np.float64)


def samples(n, size, seed):
    """Seeded 0..255 samples that differ in structure, scaled x / 127.5 - 1 (tests/test_tflite_graph_gpu.py's)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
    out = []
    for s in range(n):
        planes = [127.5 + 110 * np.sin(2 * np.pi * ((s + 1) * xx * (c + 1) + (2 * s + 1) * yy + 0.3 * c)) for c in range(3)]
        img = np.stack(planes, axis=-1) + rng.normal(0, 10, size=(size, size, 3))
        out.append(np.clip(img, 0, 255))
    return (np.stack(out) / 127.5 - 1.0).astype(F32)


def test_batch_does_not_matter(engine):
    import torch

    from cpx import _lib
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(tb.inception_v3(9, (32,), seed=3, width=0.25))
    plan = build_plan(g, conv_math="fp16x2")
    assert not any(o.kind == _lib.GRAPH_CONV for o in plan.ops)
    dev = GraphDevice(engine, plan)
    x = samples(1, 160, seed=5)
    one = dev.forward(torch.from_numpy(x).to(engine.device)).cpu().numpy()
    five = dev.forward(torch.from_numpy(np.repeat(x, 5, axis=0)).to(engine.device)).cpu().numpy()
    again = dev.forward(torch.from_numpy(np.repeat(x, 5, axis=0)).to(engine.device)).cpu().numpy()
    dev.close()
    assert all(np.array_equal(bits(five[k]), bits(one[0])) for k in range(5))
    assert np.array_equal(bits(five), bits(again))


@pytest.mark.parametrize("cin,cout,size", [(20, 48, 17), (3, 5, 19)])
def test_sliced_store_leaves_a_sentinel_buffer_untouched(engine, cin, cout, size):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(31)
    w = he_normal(rng, cout, 3, 3, cin)
    g = Graph(conv_graph(w, rng.normal(0, 0.05, size=cout).astype(F32), 1, tb.SAME, size, act=tb.RELU))
    xs = rng.uniform(-2, 2, size=(3, size, size, cin)).astype(F32)
    vals, mag = te.evaluate(g, xs, magnitudes=True)
    want, scale = vals[g.outputs[0]], mag[g.outputs[0]]
    off, stride = 7, cout + 7 + 38   # the slice neither starts nor ends on a 32-channel tile
    dev = GraphDevice(engine, build_plan(g, conv_math="fp16x2"), out_slice=(off, stride))
    sentinel = F32(-12345.678)
    out = torch.full((3, size, size, stride), float(sentinel), dtype=torch.float32, device=engine.device)
    dev.forward(torch.from_numpy(xs).to(engine.device), out=out)
    got = out.cpu().numpy()
    dev.close()
    assert float((np.abs(got[..., off:off + cout] - want) / scale).max()) < CONV_REL
    assert np.all(got[..., :off] == sentinel) and np.all(got[..., off + cout:] == sentinel)


def test_a_sliced_input_is_ranged_by_its_own_channels(engine):
    """b = the input's first 12 channels and a = 2^100 times its first 20, both by 1 x 1 selections (exact in either math),
    live side by side in one concatenated tensor; the 3 x 3 convolution reads b's slice.  Were its RANGE to see the
    neighbour's 1e30, b's values would scale to nothing."""
    from cpx import _lib

    rng = np.random.default_rng(17)
    m = tb.Model()
    x = m.tensor([1, 9, 9, 24], name="input")
    m.inputs = [x]
    sel_a = np.zeros((20, 1, 1, 24), F32)
    sel_a[np.arange(20), 0, 0, np.arange(20)] = 2.0 ** 100
    sel_b = np.zeros((12, 1, 1, 24), F32)
    sel_b[np.arange(12), 0, 0, np.arange(12)] = 1.0
    a = m.conv(x, sel_a, None, 1, tb.SAME, tb.NONE)
    b = m.conv(x, sel_b, None, 1, tb.SAME, tb.NONE)
    m.concat([a, b])
    w = he_normal(rng, 40, 3, 3, 12)
    y = m.conv(b, w, None, 1, tb.SAME, tb.NONE)
    m.outputs = [y]
    xs = rng.uniform(-1, 1, size=(2, 9, 9, 24)).astype(F32)
    g, plan, got = run(engine, m.finish(), xs, output=y)
    last = plan.ops[-1]
    view = plan.tensors[last.in0]
    assert last.kind == _lib.GRAPH_CONV_F16X2 and (view.C, view.c_offset, view.c_stride) == (12, 20, 32)
    assert plan.ops[-2].kind == _lib.GRAPH_RANGE and plan.ops[-2].in0 == last.in0
    want, mag = th.conv_float64(xs[..., :12], w, pads=(1, 1, 1, 1))
    assert float(np.abs(want).max()) > 0.5
    assert float((np.abs(got - want) / mag).max()) < CONV_REL


@pytest.mark.parametrize("tail", ["RELU", "RELU6", "SWISH", "MUL_ADD"])
def test_fused_activation_and_folded_affine(engine, tail):
    """The epilogue is CONV's: a fused RELU / RELU6, a folded swish and MUL + ADD by constants behind the convolution give
    the restatement's epilogue on the restatement's accumulator, and the float64 value within CONV_REL of the accumulated
    magnitudes."""
    from cpx import _lib

    rng = np.random.default_rng(len(tail))
    cin, cout, size = 32, 48, 9
    w = he_normal(rng, cout, 3, 3, cin)
    bias = rng.normal(0, 0.5, size=cout).astype(F32)
    m = ts.ModelSE()
    x = m.tensor([1, size, size, cin], name="input")
    m.inputs = [x]
    scale, shift, act = None, bias, 0
    if tail in ("RELU", "RELU6"):
        act = tb.RELU if tail == "RELU" else tb.RELU6
        y = m.conv(x, w, bias, 1, tb.SAME, act)
    elif tail == "SWISH":
        y, act = m.swish(m.conv(x, w, bias, 1, tb.SAME, tb.NONE)), _lib.GRAPH_ACT_SWISH
    else:
        mul, add = rng.uniform(0.5, 2.0, size=cout).astype(F32), rng.normal(0, 1.0, size=cout).astype(F32)
        y = m.binary("ADD", m.binary("MUL", m.conv(x, w, bias, 1, tb.SAME, tb.NONE), mul), add, tb.RELU)
        scale, shift, act = mul, (bias * mul + add).astype(F32), tb.RELU   # the planner's fold: (v + b) * s + a = v * s + (b * s + a)
    m.outputs = [y]
    xs = rng.uniform(-4, 4, size=(2, size, size, cin)).astype(F32)
    g, plan, got = run(engine, m.finish(), xs)
    assert [o.kind for o in plan.ops] == [_lib.GRAPH_RANGE, _lib.GRAPH_CONV_F16X2] and plan.ops[1].act == act
    _, mag = th.conv_float64(xs, w, pads=(1, 1, 1, 1))
    gain = np.ones(cout) if scale is None else np.abs(scale.astype(np.float64))
    # the float32 accumulation order is the device's own: CONV_REL of the magnitudes, times the scale, through an
    # activation of slope <= 1.1 (swish), plus the epilogue's own float32 roundings
    tol = 1.1 * CONV_REL * mag * gain
    want = th.conv(xs, w, (1, 1), (1, 1, 1, 1), scale=scale, shift=shift, act=act)
    assert np.all(np.abs(got.astype(np.float64) - want) <= tol + 16 * np.finfo(F32).eps * np.abs(want))
    want64 = te.evaluate(g, xs)[g.outputs[0]]
    assert np.all(np.abs(got - want64) <= tol + 8 * np.finfo(F32).eps * (np.abs(want64) + mag * gain))
    if tail == "RELU6":
        assert float(got.max()) == 6.0 and float(got.min()) == 0.0


def test_inception_v3_whole_network(engine):
    """Measured on an MI355X: see the figures printed below and DESIGN.md section 6."""
    import torch

    from cpx.ml_tools.tflite_reader import Graph

    blob = tb.inception_v3(17, (), seed=7, width=0.5, head_gain=4.0)
    x = samples(3, 160, seed=11)
    g = Graph(blob)
    logits_t = g.ops[-1]["inputs"][0]
    v64 = te.evaluate(g, x)
    v32 = te.evaluate(g, x, dtype=torch.float32)
    yard = float(np.abs(v32[logits_t] - v64[logits_t]).max())
    tol = LOGIT_MULTIPLE * yard
    _, _, logits = run(engine, blob, x, output=logits_t)
    _, _, logits32 = run(engine, blob, x, output=logits_t, conv_math="f32")
    err = float(np.abs(logits - v64[logits_t]).max())
    err32 = float(np.abs(logits32 - v64[logits_t]).max())
    spread = min(float(np.ptp(v64[logits_t], axis=1).min()), float(np.ptp(v64[logits_t], axis=0).max()))
    print("float32-CPU vs float64: %.3g; fp16x2 device vs float64: %.3g (ratio %.2f); f32 device vs float64: %.3g (ratio %.2f); "
          "spread of the logits %.3g" % (yard, err, err / yard, err32, err32 / yard, spread))
    assert spread >= 100 * tol, (spread, tol)
    assert err <= tol, (err, yard)


LABELS17 = ["bird", "cat", "deer", "dog", "false-positive", "hedgehog", "human", "kiwi", "leporidae", "mustelid", "penguin",
            "possum", "rodent", "sheep", "vehicle", "wallaby", "land-bird"]


def test_lite_interpreter_honours_the_environment(tmp_path, monkeypatch):
    """A float32 .tflite behind LiteInterpreter with CPX_TFLITE_CONV_MATH=fp16x2: the possum fixture's tracks get the
    default's tags, confidences within 1e-3, from a plan that holds CONV_F16X2; a bad value is refused."""
    import shutil

    from helpers import GOLDEN
    from cpx import _lib
    from cpx.config import Config
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, get_interpreter
    from cpx.track.trackextractor import extract_file

    hp = {"frame_size": 32, "model_name": "inceptionv3", "channels": ["thermal", "thermal", "filtered"]}
    (tmp_path / "inc3.tflite").write_bytes(tb.inception_v3(len(LABELS17), (), seed=13, width=0.25, head_gain=4.0))
    with open(tmp_path / "inc3.json", "w") as fh:
        json.dump({"labels": LABELS17, "hyperparams": hp, "type": "thermal", "version": "test"}, fh)
    cfg = Config.get_defaults()
    cfg.tracking["thermal"].denoise = False
    cfg.classify.models = [ModelConfig.load({"id": 9, "name": "inc3", "model_file": str(tmp_path / "inc3.tflite")})]
    src = tmp_path / "possum.cptv"
    shutil.copy(os.path.join(GOLDEN, "possum.cptv"), src)
    clip, _, _ = extract_file(src, cfg, False, save_meta=False)
    with open(os.path.join(GOLDEN, "classify_variants_golden.json")) as fh:
        gold = json.load(fh)["variants"]["inceptionv3_scaling"]["possum"]   # the reference's segments of every track
    assert len(clip.tracks) == len(gold) > 0

    def classify(math):
        if math is None:
            monkeypatch.delenv("CPX_TFLITE_CONV_MATH", raising=False)
        else:
            monkeypatch.setenv("CPX_TFLITE_CONV_MATH", math)
        interp = get_interpreter(cfg.classify.models[0])
        assert isinstance(interp, LiteInterpreter)
        preds = [interp.classify_track(clip, track, segment_frames=[np.array(s) for s in want["segments"]])
                 for track, want in zip(clip.tracks, gold)]
        assert all(p is not None for p in preds)
        kinds = set(o.kind for plan in interp._plans.values() for o in plan.ops)
        return preds, kinds

    base, kinds32 = classify(None)
    got, kinds16 = classify("fp16x2")
    assert _lib.GRAPH_CONV in kinds32 and _lib.GRAPH_CONV_F16X2 not in kinds32 and _lib.GRAPH_RANGE not in kinds32
    assert _lib.GRAPH_CONV_F16X2 in kinds16 and _lib.GRAPH_RANGE in kinds16 and _lib.GRAPH_CONV not in kinds16
    for a, b in zip(base, got):
        assert a.predicted_tag() == b.predicted_tag() and a.predicted_tag() in LABELS17
        assert float(np.abs(np.asarray(a.class_best_score) - np.asarray(b.class_best_score)).max()) <= 1e-3
        pa = np.array([p.prediction for p in a.predictions])
        pb = np.array([p.prediction for p in b.predictions])
        assert pa.shape == pb.shape and float(np.abs(pa - pb).max()) <= 1e-3
    monkeypatch.setenv("CPX_TFLITE_CONV_MATH", "half")
    with pytest.raises(ValueError, match="CPX_TFLITE_CONV_MATH"):
        get_interpreter(cfg.classify.models[0])
