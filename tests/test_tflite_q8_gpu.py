"""The hybrid operators of the TFLite graph executor (CPX_GRAPH_QUANT_PARAMS / CONV_Q8 / FC_Q8, csrc/cpx_graph_q8.hip) on
the GPU against the NumPy restatement of their arithmetic (tests/tflite_eval_q8.py, which reads the Graph only).  The
flatbuffers are synthetic (tests/tflite_build_q8.py); parity with the TFLite runtime on a quantised file is not pinned
here, as for float files (test_tflite_graph_gpu.py::test_released_model_parity is the route where the runtime exists)."""
import json
import os
import shutil

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_q8 as tq
import tflite_eval_q8 as tq8
from test_tflite_graph_gpu import LABELS17, samples

pytestmark = pytest.mark.gpu

# A hybrid output against the restatement: q is bit-reproducible and the integer sum exact, so only the four float32
# roundings of the epilogue (int -> float, sx * scale, the product, + shift) may differ: 4 x 2^-24 = 2.4e-7 of the
# magnitude |acc - zp wsum| sx scale + |shift|; four times that.
Q8_REL = 1e-6


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def run(engine, blob, x, output=None, quantised_math="hybrid"):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    plan = build_plan(g, input_shape=x.shape[1:], output=output, quantised_math=quantised_math)
    dev = GraphDevice(engine, plan)
    out = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device)).cpu().numpy()
    dev.close()
    return g, plan, out


def kinds(plan):
    from cpx import _lib

    names = {_lib.GRAPH_CONV_Q8: "CONV_Q8", _lib.GRAPH_FC_Q8: "FC_Q8", _lib.GRAPH_QUANT_PARAMS: "QUANT_PARAMS"}
    return [names.get(o.kind, o.name) for o in plan.ops]


def check_against_helper(g, got, x, what):
    vals, mag = tq8.evaluate_hybrid(g, x)
    t = g.outputs[0]
    want = vals[t]
    assert got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = Q8_REL * mag[t]
    rel = float((err / np.maximum(mag[t], 1e-30)).max())
    print("%s: max |error| / magnitude = %.3g, %d of %d elements differ" % (what, rel, int((err > 0).sum()), err.size))
    assert np.all(err <= bound), (what, rel)
    return want


# ---- (a) the operand map, with exact integers ----
@pytest.mark.parametrize("cout", [64, 40])
def test_operand_map_exact(engine, cout):
    """Integers in, integers out: inputs in [-128, 127] with both ends give sx = 1, zp = 0, q = x; the asymmetric filter
    w[co][ci] = ((7 co + 13 ci) mod 255) - 127 with scales 1 and no bias makes the output the integer product, every
    value below 2^24.  A wrong A / B / C lane map or a swapped row / column shows here."""
    rng = np.random.default_rng(40 + cout)
    x = rng.integers(-128, 128, size=(1, 8, 8, 64)).astype(np.float32)
    x[0, 0, 0, 0], x[0, 7, 7, 63] = -128.0, 127.0
    co, ci = np.mgrid[0:cout, 0:64]
    w = (((7 * co + 13 * ci) % 255) - 127).astype(np.int8)
    m = tq.ModelQ8()
    xin = m.tensor([1, 8, 8, 64], name="input")
    m.inputs = [xin]
    m.outputs = [m.conv_q8(xin, m.qfilter(w.reshape(cout, 1, 1, 64), np.ones(cout, np.float32)), np.zeros(cout, np.float32))]
    g, plan, got = run(engine, m.finish(), x)
    assert kinds(plan) == ["QUANT_PARAMS", "CONV_Q8"]
    want = x.reshape(64, 64).astype(np.int64) @ w.astype(np.int64).T
    assert int(np.abs(want).max()) < 2 ** 24 and not np.array_equal(w[:40, :40], w[:40, :40].T)
    assert np.array_equal(got.reshape(64, cout).astype(np.int64), want) and np.array_equal(got, np.round(got))


# ---- (b) convolutions against the restatement ----
def three_samples(rng, size, cin):
    """One sample all positive (zp = -128: a padded tap staged as 0 instead of zp shows at every border), one mostly
    negative, one all zeros."""
    return np.stack([rng.uniform(1, 5, size=(size, size, cin)), rng.uniform(-3, 0.5, size=(size, size, cin)),
                     np.zeros((size, size, cin))]).astype(np.float32)


def one_conv_q8(rng, kh, kw, stride, padding, cin, cout, size, act=tb.NONE):
    m = tb.Model()
    x = m.tensor([1, size, size, cin], name="input")
    m.inputs = [x]
    w = rng.normal(0, np.sqrt(2.0 / (kh * kw * cin)), size=(cout, kh, kw, cin)).astype(np.float32)
    m.outputs = [m.conv(x, w, rng.normal(0, 0.05, size=cout).astype(np.float32), stride, padding, act)]
    return tq.quantise(m.finish(), min_elements=0)


CONV_CASES = [
    # kh, kw, stride, padding, cin, cout, size
    (1, 1, 1, tb.SAME, 192, 320, 8),
    (1, 1, 2, tb.VALID, 48, 80, 17),
    (3, 3, 1, tb.SAME, 32, 48, 17),
    (3, 3, 2, tb.SAME, 80, 192, 17),
    (3, 3, 2, tb.VALID, 36, 40, 9),
    (5, 5, 1, tb.SAME, 48, 64, 9),
    (1, 7, 1, tb.SAME, 136, 160, 17),
    (7, 1, 2, tb.SAME, 40, 24, 8),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "%dx%d_s%d_%s_%dto%d_at%d" % (c[0], c[1], c[2], "SV"[c[3]], c[4], c[5], c[6]))
def test_convolution_against_the_restatement(engine, case):
    kh, kw, stride, padding, cin, cout, size = case
    rng = np.random.default_rng(kh * 100 + kw * 10 + stride + cin + cout + size)
    blob = one_conv_q8(rng, kh, kw, stride, padding, cin, cout, size)
    x = three_samples(rng, size, cin)
    g, plan, got = run(engine, blob, x)
    assert kinds(plan) == ["QUANT_PARAMS", "CONV_Q8"]
    sx, inv, zp = tq8.quant_params(x)
    assert list(zp) == [-128, zp[1], 0] and -128 < zp[1] < 127 and sx[2] == 1.0
    want = check_against_helper(g, got, x, str(case))
    assert float(np.abs(want[0]).max()) > 0.1


# ---- (c) a tile that crosses samples, (h) batch independence ----
def crossing_graph():
    rng = np.random.default_rng(77)
    blob = one_conv_q8(rng, 3, 3, 1, tb.SAME, 32, 32, 5, act=tb.RELU)
    x = rng.uniform(-1, 1, size=(7, 5, 5, 32)).astype(np.float32)
    x *= np.array([1, 100, 1, 100, 0.01, 1, 100], np.float32).reshape(7, 1, 1, 1)   # neighbours' ranges 100 x apart
    return blob, x


def test_a_tile_crossing_samples_takes_each_pixels_own_parameters(engine):
    """7 x 25 = 175 pixels over 128-pixel tiles: every sample shares its tile with neighbours whose range is 100 times
    its own or a hundredth of it, and sample 5 lies across the two tiles."""
    blob, x = crossing_graph()
    g, plan, got = run(engine, blob, x)
    sx, _, _ = tq8.quant_params(x)
    assert float(sx.max() / sx.min()) > 100
    check_against_helper(g, got, x, "crossing")


def test_batch_does_not_matter(engine):
    blob, x = crossing_graph()
    _, _, five = run(engine, blob, np.ascontiguousarray(x[:5]))
    for k in (0, 4):
        _, _, one = run(engine, blob, np.ascontiguousarray(x[k:k + 1]))
        assert np.array_equal(one[0], five[k])


# ---- (d) the parameters of a channel slice ----
def test_min_max_see_the_views_own_channels_only(engine):
    """A RELU output placed inside a concatenation whose other part is 50 times larger also feeds a quantised 1 x 1
    convolution: its quantisation parameters come from its own 32 of the 64 channels."""
    rng = np.random.default_rng(12)
    m = tq.ModelQ8()
    x = m.tensor([1, 8, 8, 32], name="input")
    m.inputs = [x]
    a = m.unary("RELU", x)
    b = m.unary("RELU", m.binary("MUL", x, np.full(32, 50.0, np.float32)))
    cat = m.concat([a, b])
    q = rng.integers(-127, 128, size=(64, 1, 1, 32)).astype(np.int8)
    y = m.conv_q8(a, m.qfilter(q, rng.uniform(1e-3, 1e-2, size=64).astype(np.float32)), rng.normal(0, 0.05, size=64).astype(np.float32))
    m.outputs = [m.binary("ADD", y, cat)]
    xs = rng.uniform(-1, 2, size=(2, 8, 8, 32)).astype(np.float32)
    g, plan, got = run(engine, m.finish(), xs)
    assert not plan.copies()
    ta = plan.tensors[g.ops[0]["outputs"][0]]
    assert (ta.C, ta.c_offset, ta.c_stride) == (32, 0, 64)
    vals, mag = tq8.evaluate_hybrid(g, xs)
    t = g.ops[-2]["outputs"][0]   # the convolution's output; the ADD adds one more float32 rounding of the sum
    want = vals[g.outputs[0]]
    bound = Q8_REL * mag[t] + 2.0 ** -23 * np.abs(want)
    assert np.all(np.abs(got.astype(np.float64) - want) <= bound)
    # parameters taken over all 64 channels would be far coarser
    cat_t, a_t = g.ops[-1]["inputs"][1], g.ops[0]["outputs"][0]
    assert np.all(tq8.quant_params(vals[cat_t])[0] > 10 * tq8.quant_params(vals[a_t])[0])


# ---- (e) the sliced store ----
def test_sliced_store_leaves_a_sentinel_buffer_untouched(engine):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(31)
    cin, cout, size = 20, 48, 17
    g = Graph(one_conv_q8(rng, 3, 3, 1, tb.SAME, cin, cout, size, act=tb.RELU))
    xs = rng.uniform(-2, 2, size=(3, size, size, cin)).astype(np.float32)
    vals, mag = tq8.evaluate_hybrid(g, xs)
    want = vals[g.outputs[0]]
    off, stride = 7, cout + 7 + 38   # the middle slice; it neither starts nor ends on a 32-channel tile
    dev = GraphDevice(engine, build_plan(g), out_slice=(off, stride))
    sentinel = np.float32(-12345.678)
    out = torch.full((3, size, size, stride), float(sentinel), dtype=torch.float32, device=engine.device)
    dev.forward(torch.from_numpy(xs).to(engine.device), out=out)
    got = out.cpu().numpy()
    dev.close()
    assert np.all(np.abs(got[..., off:off + cout].astype(np.float64) - want) <= Q8_REL * mag[g.outputs[0]])
    assert np.all(got[..., :off] == sentinel) and np.all(got[..., off + cout:] == sentinel)


# ---- (f) FULLY_CONNECTED ----
@pytest.mark.parametrize("asymmetric", [True, False])
@pytest.mark.parametrize("cin,cout", [(2048, 17), (50, 7), (1030, 33)])
def test_fully_connected_against_the_restatement(engine, cin, cout, asymmetric):
    rng = np.random.default_rng(cin + cout + int(asymmetric))
    m = tq.ModelQ8()
    x = m.tensor([1, 1, 1, cin], name="input")
    m.inputs = [x]
    q, scale = tq.quantise_filter(rng.normal(0, np.sqrt(2.0 / cin), size=(cout, cin)), per_channel=False)
    m.outputs = [m.dense_q8(x, m.qfilter(q, scale), rng.normal(0, 0.05, size=cout).astype(np.float32), asymmetric=asymmetric)]
    xs = rng.uniform(-1, 3, size=(5, 1, 1, cin)).astype(np.float32)
    xs[1] = 0.0
    xs[3] = rng.uniform(0.5, 2, size=(1, 1, cin))
    g, plan, got = run(engine, m.finish(), xs)
    assert kinds(plan) == ["QUANT_PARAMS", "FC_Q8"] and plan.ops[0].param == (0.0 if asymmetric else 1.0)
    _, _, zp = tq8.quant_params(xs.reshape(5, -1), symmetric=not asymmetric)
    assert (zp[3] == -128) == asymmetric and zp[1] == 0
    check_against_helper(g, got.reshape(5, cout), xs, "fc %d -> %d %s" % (cin, cout, asymmetric))


# ---- (g) the whole network ----
# Measured on an MI355X (width 0.5, 160 x 160 x 3, N = 3, 17 logits): see DESIGN.md section 6.
#   dev  = max |device logits - hybrid restatement|                       = WHOLE_NET_DEV below
#   yard = max |hybrid restatement - float64 of the dequantised graph|    = the quantisation noise itself
# An activation off by one float32 ulp may flip a later q by one step, so dev has no derived bound; the device may
# deviate by four times what was measured (box-to-box scatter of a maximum over 51 logits, as LOGIT_MULTIPLE).
#   measured: dev = 0 (the 51 logits equal the restatement's bit for bit), yard = 0.04843, float math on the device vs
#   hybrid 0.04843, spread of the logits 1.267.  Four times a measured 0 is 0: the assertion below is equality, and
#   tolerance <= yard / 4 and spread >= 100 x tolerance hold with it.
WHOLE_NET_DEV = 0.0
WHOLE_NET_MULTIPLE = 4.0
# predict hands out LOGISTIC of the logits: the (g) tolerance through a slope of at most 1/4, and the float32 evaluation
# of 1 / (1 + exp(-v)) on the device against the restatement's, a few roundings of a value below 1 (measured: 1.5e-8)
SIGMOID_ROUNDING = 4 * 2.0 ** -24


@pytest.fixture(scope="module")
def whole_network():
    from cpx.ml_tools.tflite_reader import Graph

    blob = tq.quantise(tb.inception_v3(17, (), seed=7, width=0.5, head_gain=4.0))
    x = samples(3, 160, seed=11)
    g = Graph(blob)
    logits_t = g.ops[-1]["inputs"][0]
    hyb, _ = tq8.evaluate_hybrid(g, x)
    deq = tq8.evaluate_dequantised(g, x)
    return blob, x, g, logits_t, hyb, deq


def test_inception_v3_whole_network(engine, whole_network):
    blob, x, g, logits_t, hyb, deq = whole_network
    _, plan, logits = run(engine, blob, x, output=logits_t)
    assert kinds(plan).count("CONV_Q8") + kinds(plan).count("FC_Q8") == sum(g.quantised_filter(op) is not None for op in g.ops) > 80
    _, fplan, flogits = run(engine, blob, x, output=logits_t, quantised_math="float")
    assert "CONV_Q8" not in kinds(fplan) and "QUANT_PARAMS" not in kinds(fplan)
    dev = float(np.abs(logits - hyb[logits_t]).max())
    yard = float(np.abs(hyb[logits_t] - deq[logits_t]).max())
    other = float(np.abs(flogits - logits).max())
    spread = min(float(np.ptp(deq[logits_t], axis=1).min()), float(np.ptp(deq[logits_t], axis=0).max()))
    print("device vs hybrid restatement: %.4g; hybrid restatement vs float64 of the dequantised graph: %.4g; float math on the "
          "device vs hybrid: %.4g; spread of the logits %.4g" % (dev, yard, other, spread))
    tol = WHOLE_NET_MULTIPLE * WHOLE_NET_DEV
    assert dev <= tol, (dev, tol)
    assert tol <= yard / 4, (tol, yard)     # or the test is vacuous: a wrong zero point, scale or wsum lands at or above yard
    assert spread >= 100 * tol, (spread, tol)
    assert other <= 2 * yard, (other, yard)  # the same model with the other arithmetic


# ---- (i) through the public interface ----
@pytest.fixture(scope="module")
def quantised_model(tmp_path_factory):
    """A dynamic-range quantised width-0.25 Inception-v3 file + sidecar, as test_tflite_graph_gpu.inception_model."""
    from helpers import GOLDEN

    d = tmp_path_factory.mktemp("inc3q8")
    with open(os.path.join(GOLDEN, "classify_variants_golden.json")) as fh:
        golden = json.load(fh)
    hp = dict(golden["variants"]["inceptionv3_scaling"]["hyperparams"])
    hp["channels"] = ["thermal", "thermal", "filtered"]
    blob = tq.quantise(tb.inception_v3(len(LABELS17), (), seed=13, width=0.25, head_gain=4.0))
    (d / "inc3q8.tflite").write_bytes(blob)
    with open(d / "inc3q8.json", "w") as fh:
        json.dump({"labels": LABELS17, "hyperparams": hp, "type": "thermal", "version": "test"}, fh)
    return d, blob


def _config(d):
    from cpx.config import Config
    from cpx.config.config import ModelConfig

    cfg = Config.get_defaults()
    cfg.tracking["thermal"].denoise = False
    cfg.classify.models = [ModelConfig.load({"id": 9, "name": "inc3q8", "model_file": str(d / "inc3q8.tflite")})]
    return cfg


def _tags(directory):
    out = {}
    for name in ("possum", "hedgehog"):
        with open(os.path.join(str(directory), name + ".txt")) as fh:
            meta = json.load(fh)
        assert len(meta["tracks"]) > 0
        out[name] = [(t["id"], t["predictions"][0]["tag"]) for t in meta["tracks"]]
    return out


def test_quantised_file_through_the_public_interface(tmp_path, monkeypatch, quantised_model):
    from cpx import _lib
    from cpx.classify.clipclassifier import ClipClassifier
    from cpx.ml_tools.interpreter import LiteInterpreter, get_interpreter
    from cpx.ml_tools.tflite_reader import Graph
    from helpers import GOLDEN

    d, blob = quantised_model
    cfg = _config(d)
    monkeypatch.delenv("CPX_TFLITE_QUANT_MATH", raising=False)
    interp = get_interpreter(cfg.classify.models[0])
    assert isinstance(interp, LiteInterpreter)
    plan = next(iter(interp._plans.values()))
    assert sum(o.kind == _lib.GRAPH_CONV_Q8 for o in plan.ops) > 80
    g = Graph(blob)
    x = samples(2, 160, seed=3)
    got = interp.predict(x)
    want = tq8.evaluate_hybrid(g, x)[0][g.outputs[0]]
    err = float(np.abs(got - want).max())
    print("predict vs the hybrid restatement (probabilities): %.4g" % err)
    assert got.shape == want.shape == (2, 17) and err <= WHOLE_NET_MULTIPLE * WHOLE_NET_DEV + SIGMOID_ROUNDING
    # the batched many-file path, with either arithmetic
    tags = {}
    for mode in ("hybrid", "float"):
        dd = tmp_path / mode
        dd.mkdir()
        for name in ("possum", "hedgehog"):
            shutil.copy(os.path.join(GOLDEN, name + ".cptv"), dd / (name + ".cptv"))
        monkeypatch.setenv("CPX_TFLITE_QUANT_MATH", mode)
        cc = ClipClassifier(cfg)
        cc.process(str(dd), track=True)
        assert cc.last_run is not None and cc.last_run["files"] == 2
        tags[mode] = _tags(dd)
    assert tags["hybrid"] == tags["float"]
    fplan = next(iter(get_interpreter(cfg.classify.models[0])._plans.values()))   # CPX_TFLITE_QUANT_MATH=float is still set
    assert not any(o.kind in (_lib.GRAPH_CONV_Q8, _lib.GRAPH_FC_Q8, _lib.GRAPH_QUANT_PARAMS) for o in fplan.ops)
    assert [o.name for o in fplan.ops] == [o.name for o in plan.ops if o.kind != _lib.GRAPH_QUANT_PARAMS]
