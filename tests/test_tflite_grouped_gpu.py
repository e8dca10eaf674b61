"""Grouped CONV_2D on the device (CPX_GRAPH_CONV_GROUPED / CONV_Q8_GROUPED: csrc/cpx_graph.hip, csrc/cpx_graph_q8.hip):
each float32 case against float64 and, bit for bit, against the existing ungrouped CONV run group by group; the hybrid
operator against its NumPy restatement (tests/tflite_eval_grouped.py); views; the WR-ResNet-22-4's own flatbuffer, float32
and dynamic-range quantised, as a whole network and through the public interface.  Parity with the TFLite runtime is not
pinned, as for every hybrid operator here."""
import json
import os
import shutil

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_q8 as tq
import tflite_eval as te
import tflite_eval_grouped as tgr
import tflite_eval_q8 as tq8

pytestmark = pytest.mark.gpu

# float32 accumulation against the accumulated magnitude sum |x| |w|: the CONV_REL of tests/test_tflite_graph_gpu.py
CONV_REL = 4e-6
# a hybrid output against the restatement: the Q8_REL of tests/test_tflite_q8_gpu.py (four float32 roundings of the
# epilogue, 4 x 2^-24 of the magnitude; four times that)
Q8_REL = 1e-6
LABELS17 = ["l%d" % i for i in range(17)]


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def run(engine, blob, x, output=None, grouped=True, **kw):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    plan = build_plan(g, input_shape=x.shape[1:], output=output, grouped_convolutions=grouped, **kw)
    dev = GraphDevice(engine, plan)
    out = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device)).cpu().numpy()
    dev.close()
    return g, plan, out


def kinds(plan):
    from cpx import _lib

    names = {_lib.GRAPH_CONV: "CONV", _lib.GRAPH_CONV_GROUPED: "CONV_GROUPED", _lib.GRAPH_CONV_Q8_GROUPED: "CONV_Q8_GROUPED",
             _lib.GRAPH_CONV_Q8: "CONV_Q8", _lib.GRAPH_FC_Q8: "FC_Q8", _lib.GRAPH_QUANT_PARAMS: "QUANT_PARAMS", _lib.GRAPH_PAD: "PAD"}
    return [names.get(o.kind, o.name) for o in plan.ops]


def pair(v):
    return (v, v) if np.isscalar(v) else tuple(v)


def conv_graph(w, bias, stride, padding, hw, G=1, act=tb.NONE, pads=None):
    """One CONV_2D of G groups on a G * (filter depth)-channel input; pads: an explicit PAD in front."""
    m = tb.Model()
    x = m.tensor([1, hw[0], hw[1], G * w.shape[3]], name="input")
    m.inputs = [x]
    y = x if pads is None else m.pad(x, [[0, 0], [pads[0], pads[1]], [pads[2], pads[3]], [0, 0]])
    m.outputs = [m.conv(y, w, bias, stride, padding, act)]
    return m.finish()


# kh, kw, stride, padding, Cin, G, Cout, (H, W), N
F32_CASES = [
    (3, 3, 1, tb.SAME, 2, 2, 16, (9, 9), 3),        # conv1_1: Cg = 1, Cog = 8
    (3, 3, 1, tb.SAME, 16, 2, 64, (9, 9), 3),
    (1, 1, 1, tb.VALID, 16, 2, 64, (9, 9), 3),
    (3, 3, 2, tb.SAME, 64, 2, 128, (11, 11), 2),
    (1, 1, 2, tb.VALID, 64, 2, 128, (11, 11), 2),
    (3, 3, 3, tb.SAME, 128, 2, 256, (11, 11), 2),
    (1, 1, 3, tb.VALID, 128, 2, 256, (11, 11), 2),
    (3, 3, 1, tb.SAME, 12, 2, 80, (7, 13), 3),      # Cg = 6: group 1 starts off a 16-byte boundary; Cog = 40: a tile tail
    (3, 3, (2, 3), tb.SAME, 24, 3, 30, (13, 7), 2),
    (3, 3, (3, 2), tb.SAME, 24, 3, 30, (7, 13), 2),  # ... and its H / W twin
    (1, 1, 1, tb.SAME, 8, 2, 192, (5, 5), 2),       # three tiles per group
    (1, 1, 1, tb.SAME, 8, 2, 256, (5, 5), 2),       # two-tile waves
]


def case_id(c):
    s = pair(c[2])
    return "%dx%d_s%d%d_%s_%dto%d_g%d_at%dx%d" % (c[0], c[1], s[0], s[1], "SV"[c[3]], c[4], c[6], c[5], c[7][0], c[7][1])


def ungrouped_reference(engine, w, bias, stride, padding, x, G):
    """The existing ungrouped CONV on the host-sliced input channels and filter rows of each group, concatenated.  CONV
    stops at stride 2: an axis of stride 3 runs at stride 1 behind an explicit PAD of the SAME arithmetic and is
    subsampled on the host -- output o of stride 3 is output 3 o of stride 1 with the same window, hence the same chain."""
    from cpx.ml_tools.tflite_graph import same_pads

    cog, cg = w.shape[0] // G, w.shape[3]
    sh, sw = pair(stride)
    H, W = x.shape[1:3]
    parts = []
    for k in range(G):
        xs = np.ascontiguousarray(x[..., k * cg:(k + 1) * cg])
        ws, bs = w[k * cog:(k + 1) * cog], bias[k * cog:(k + 1) * cog]
        if 3 in (sh, sw):
            rh, rw = (1 if sh == 3 else sh), (1 if sw == 3 else sw)
            pads = None
            ho, wo = (H - w.shape[1]) // sh + 1, (W - w.shape[2]) // sw + 1
            if padding == tb.SAME:
                ho, pt, pb = same_pads(H, w.shape[1], sh)
                wo, pl, pr = same_pads(W, w.shape[2], sw)
                pads = (pt, pb, pl, pr)
            _, plan, full = run(engine, conv_graph(ws, bs, (rh, rw), tb.VALID, (H, W), pads=pads), xs, grouped=False)
            assert "CONV" in kinds(plan) and "CONV_GROUPED" not in kinds(plan)
            got = full[:, ::(3 if sh == 3 else 1), ::(3 if sw == 3 else 1)][:, :ho, :wo]
            assert got.shape[1:3] == (ho, wo)
        else:
            _, plan, got = run(engine, conv_graph(ws, bs, stride, padding, (H, W)), xs, grouped=False)
            assert kinds(plan) == ["CONV"]
        parts.append(got)
    return np.concatenate(parts, axis=3)


@pytest.mark.parametrize("case", F32_CASES, ids=case_id)
def test_float32_grouped_convolution(engine, case):
    kh, kw, stride, padding, cin, G, cout, hw, N = case
    rng = np.random.default_rng(kh * 100 + kw * 10 + sum(pair(stride)) + cin + cout + hw[0])
    cg = cin // G
    w = rng.normal(0, np.sqrt(2.0 / (kh * kw * cg)), size=(cout, kh, kw, cg)).astype(np.float32)
    bias = rng.normal(0, 0.05, size=cout).astype(np.float32)
    x = rng.uniform(-1, 1, size=(N,) + hw + (cin,)).astype(np.float32)
    g, plan, got = run(engine, conv_graph(w, bias, stride, padding, hw, G), x)
    assert kinds(plan) == ["CONV_GROUPED"] and plan.ops[0].groups == G
    vals, mag = te.evaluate(g, x, magnitudes=True)
    want = vals[g.outputs[0]]
    assert got.shape == want.shape
    rel = float((np.abs(got - want) / mag[g.outputs[0]]).max())
    print("%s: max |error| / sum |x||w| = %.3g" % (case_id(case), rel))
    assert rel < CONV_REL, rel
    ref = ungrouped_reference(engine, w, bias, stride, padding, x, G)
    assert ref.shape == got.shape and ref.tobytes() == got.tobytes()


def test_batch_and_activation_do_not_move_a_float32_bit(engine):
    """Sample 0 of N = 1 and of N = 5 (its tile then holds other samples' pixels): the same bits; RELU is max(v, 0) of them."""
    rng = np.random.default_rng(70)
    w = rng.normal(0, 0.1, size=(80, 3, 3, 6)).astype(np.float32)
    bias = rng.normal(0, 0.05, size=80).astype(np.float32)
    x = rng.uniform(-1, 1, size=(5, 7, 5, 12)).astype(np.float32)
    blob = conv_graph(w, bias, 1, tb.SAME, (7, 5), 2)
    _, _, five = run(engine, blob, x)
    _, _, one = run(engine, blob, np.ascontiguousarray(x[:1]))
    assert one[0].tobytes() == five[0].tobytes()
    _, _, relu = run(engine, conv_graph(w, bias, 1, tb.SAME, (7, 5), 2, act=tb.RELU), x)
    assert np.array_equal(relu, np.maximum(five, 0)) and (five < 0).any()


# ---- the hybrid operator ----
@pytest.mark.parametrize("cog", [32, 40])
def test_operand_map_exact(engine, cog):
    """Integers in, integers out (after test_tflite_q8_gpu.py::test_operand_map_exact): inputs in [-128, 127] with both
    ends give sx = 1, zp = 0, q = x over the WHOLE tensor; w[co][ci] = ((7 co + 13 ci) mod 255) - 127 with the absolute
    output channel co, so the two groups' filters differ and a group mix-up -- the wrong image, the wrong input
    channels, the wrong wsum -- shows; scales 1, no bias: the output is the integer product, every value below 2^24."""
    G, cg = 2, 64
    rng = np.random.default_rng(40 + cog)
    x = rng.integers(-128, 128, size=(1, 8, 8, G * cg)).astype(np.float32)
    x[0, 0, 0, 0], x[0, 7, 7, G * cg - 1] = -128.0, 127.0
    co, ci = np.mgrid[0:G * cog, 0:cg]
    w = (((7 * co + 13 * ci) % 255) - 127).astype(np.int8)
    m = tq.ModelQ8()
    xin = m.tensor([1, 8, 8, G * cg], name="input")
    m.inputs = [xin]
    m.outputs = [m.conv_q8(xin, m.qfilter(w.reshape(G * cog, 1, 1, cg), np.ones(G * cog, np.float32)), np.zeros(G * cog, np.float32))]
    g, plan, got = run(engine, m.finish(), x)
    assert kinds(plan) == ["QUANT_PARAMS", "CONV_Q8_GROUPED"]
    xi = x.reshape(64, G, cg).astype(np.int64)
    want = np.concatenate([xi[:, k] @ w[k * cog:(k + 1) * cog].astype(np.int64).T for k in range(G)], axis=1)
    assert int(np.abs(want).max()) < 2 ** 24 and not np.array_equal(w[:cog], w[cog:])
    assert np.array_equal(got.reshape(64, G * cog).astype(np.int64), want) and np.array_equal(got, np.round(got))


def two_range_input(rng, N, hw, cin):
    """Group 0 in [-1, 1], group 1 in [0, 50]: parameters of the whole tensor are fifty times coarser than group 0's own."""
    half = cin // 2
    return np.concatenate([rng.uniform(-1, 1, size=(N,) + hw + (half,)), rng.uniform(0, 50, size=(N,) + hw + (cin - half,))],
                          axis=3).astype(np.float32)


def quantised_conv(rng, kh, kw, stride, padding, cin, G, cout, hw, act=tb.NONE):
    cg = cin // G
    w = rng.normal(0, np.sqrt(2.0 / (kh * kw * cg)), size=(cout, kh, kw, cg)).astype(np.float32)
    return tq.quantise(conv_graph(w, rng.normal(0, 0.05, size=cout).astype(np.float32), stride, padding, hw, G, act), min_elements=0)


def check_against_helper(g, got, x, what, t=None):
    vals, mag = tgr.evaluate_hybrid(g, x)
    t = g.outputs[0] if t is None else t
    want = vals[t]
    assert got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = float((err / np.maximum(mag[t], 1e-30)).max())
    print("%s: max |error| / magnitude = %.3g, %d of %d elements differ" % (what, rel, int((err > 0).sum()), err.size))
    assert np.all(err <= Q8_REL * mag[t]), (what, rel)
    return vals, mag


Q8_CASES = [F32_CASES[i] for i in (1, 2, 3, 4, 5, 6, 7)]   # the geometries above with Cg in (8, 32, 64, 6)


@pytest.mark.parametrize("case", Q8_CASES, ids=case_id)
def test_hybrid_grouped_convolution_against_the_restatement(engine, case):
    kh, kw, stride, padding, cin, G, cout, hw, N = case
    assert cin // G in (8, 32, 64, 6)
    rng = np.random.default_rng(kh * 100 + kw * 10 + sum(pair(stride)) + cin + cout + hw[0] + 1)
    blob = quantised_conv(rng, kh, kw, stride, padding, cin, G, cout, hw)
    x = two_range_input(rng, N, hw, cin)
    g, plan, got = run(engine, blob, x)
    assert kinds(plan) == ["QUANT_PARAMS", "CONV_Q8_GROUPED"]
    vals, mag = check_against_helper(g, got, x, case_id(case))
    # parameters per group would land outside the bound: the case tells the two arithmetics apart
    per, _ = tgr.evaluate_hybrid(g, x, per_group=True)
    t = g.outputs[0]
    outside = np.abs(per[t].astype(np.float64) - vals[t]) > Q8_REL * mag[t]
    assert outside[..., :cout // 2].mean() > 0.5, float(outside.mean())
    sx_whole, sx_own = tq8.quant_params(x)[0], tq8.quant_params(x[..., :cin // 2])[0]
    assert np.all(sx_whole > 20 * sx_own)


def crossing_graph():
    rng = np.random.default_rng(77)
    blob = quantised_conv(rng, 3, 3, 1, tb.SAME, 16, 2, 64, (9, 9), act=tb.RELU)
    x = two_range_input(rng, 5, (9, 9), 16)
    x *= np.array([1, 100, 0.01, 100, 1], np.float32).reshape(5, 1, 1, 1)   # neighbours' ranges 100 x apart
    return blob, x


def test_a_tile_crossing_samples_takes_each_pixels_own_parameters(engine):
    """3 x 81 = 243 pixels over 128-pixel tiles: sample 1 lies across the two tiles, between neighbours whose range is a
    hundredth and a ten-thousandth of its own."""
    blob, x = crossing_graph()
    x = np.ascontiguousarray(x[:3])
    g, plan, got = run(engine, blob, x)
    sx, _, _ = tq8.quant_params(x)
    assert float(sx.max() / sx.min()) > 1000
    check_against_helper(g, got, x, "crossing")


def test_batch_does_not_matter(engine):
    blob, x = crossing_graph()
    _, _, five = run(engine, blob, x)
    _, _, one = run(engine, blob, np.ascontiguousarray(x[:1]))
    assert one[0].tobytes() == five[0].tobytes()


# ---- views ----
def view_graph(rng, quantised):
    """b (16 channels) lives at channel 8 of the 24 of a concatenation whose first part is 50 times larger, and feeds a
    grouped 3 x 3 convolution (G = 2, Cg = 8) whose output is added to the concatenation."""
    m = tb.Model()
    x = m.tensor([1, 9, 9, 16], name="input")
    m.inputs = [x]
    a = m.unary("RELU", m.binary("MUL", x, np.full(16, 50.0, np.float32)))
    a8 = m.conv(a, rng.normal(0, 0.3, size=(8, 1, 1, 16)).astype(np.float32), np.full(8, 20.0, np.float32), 1, tb.SAME, tb.RELU)
    b = m.unary("RELU6", m.binary("ADD", x, np.full(16, 1.0, np.float32)))
    cat = m.concat([a8, b])
    y = m.conv(b, rng.normal(0, 0.1, size=(24, 3, 3, 8)).astype(np.float32), rng.normal(0, 0.05, size=24).astype(np.float32), 1, tb.SAME)
    m.outputs = [m.binary("ADD", y, cat)]
    blob = m.finish()
    return blob, (tq.quantise(blob, min_elements=200) if quantised else blob)   # (the 1 x 1 filter, 128 elements, stays float32)


@pytest.mark.parametrize("quantised", [False, True], ids=["float32", "hybrid"])
def test_a_grouped_convolution_reads_a_tensor_inside_a_concatenation(engine, quantised):
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(12)
    fblob, blob = view_graph(rng, quantised)
    xs = rng.uniform(-1, 2, size=(2, 9, 9, 16)).astype(np.float32)
    g, plan, got = run(engine, blob, xs)
    assert not plan.copies() and ("CONV_Q8_GROUPED" if quantised else "CONV_GROUPED") in kinds(plan)
    conv = next(o for o in plan.ops if getattr(o, "groups", 1) == 2)
    b_t = conv.in0
    assert (plan.tensors[b_t].C, plan.tensors[b_t].c_offset, plan.tensors[b_t].c_stride) == (16, 8, 24)
    y_t, cat_t = g.ops[-1]["inputs"]
    a8_t = next(op["outputs"][0] for op in g.ops if op["name"] == "CONV_2D" and g.const(op["inputs"][1]).shape[1] == 1)
    # float64 of the float32 file (the quantised one keeps its tensor ids): the magnitudes of the two float32 sums
    v64, m64 = te.evaluate(Graph(fblob), xs, magnitudes=True)
    cat_mag = np.concatenate([m64[a8_t], np.abs(v64[b_t])], axis=3)
    if quantised:
        vals, mag = tgr.evaluate_hybrid(g, xs)
        want = vals[g.outputs[0]].astype(np.float64)
        # the hybrid sum at Q8_REL; the float32 1 x 1 convolution in the concatenation, on the device and in the float32
        # restatement each within CONV_REL of float64; the final ADD rounds once more
        bound = Q8_REL * mag[y_t] + 2 * CONV_REL * cat_mag + 2.0 ** -23 * np.abs(want)
        # QUANT_PARAMS see the tensor's own 16 channels: over all 24 of the concatenation they would be far coarser
        q = next(o for o in plan.ops if o.out == conv.in1)
        assert q.in0 == b_t
        assert np.all(tq8.quant_params(vals[cat_t])[0] > 10 * tq8.quant_params(vals[b_t])[0])
    else:
        want = v64[g.outputs[0]]
        bound = CONV_REL * (m64[y_t] + cat_mag) + 2.0 ** -23 * np.abs(want)
    assert got.shape == want.shape and np.all(np.abs(got.astype(np.float64) - want) <= bound)


@pytest.mark.parametrize("quantised", [False, True], ids=["float32", "hybrid"])
def test_sliced_store_leaves_a_sentinel_buffer_untouched(engine, quantised):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(31)
    cin, cout, hw = 12, 80, (7, 13)   # Cog = 40: each group's tile tail must stay inside the group AND inside the slice
    w = rng.normal(0, 0.2, size=(cout, 3, 3, cin // 2)).astype(np.float32)
    blob = conv_graph(w, rng.normal(0, 0.05, size=cout).astype(np.float32), 1, tb.SAME, hw, 2, act=tb.RELU)
    g = Graph(tq.quantise(blob, min_elements=0) if quantised else blob)
    xs = rng.uniform(-2, 2, size=(3,) + hw + (cin,)).astype(np.float32)
    if quantised:
        vals, mag = tgr.evaluate_hybrid(g, xs)
        want, bound = vals[g.outputs[0]], Q8_REL * mag[g.outputs[0]]
    else:
        vals, mag = te.evaluate(g, xs, magnitudes=True)
        want, bound = vals[g.outputs[0]], CONV_REL * mag[g.outputs[0]]
    off, stride = 7, cout + 7 + 38   # the middle slice; it neither starts nor ends on a 32-channel tile
    dev = GraphDevice(engine, build_plan(g, grouped_convolutions=True), out_slice=(off, stride))
    sentinel = np.float32(-12345.678)
    out = torch.full((3,) + hw + (stride,), float(sentinel), dtype=torch.float32, device=engine.device)
    dev.forward(torch.from_numpy(xs).to(engine.device), out=out)
    got = out.cpu().numpy()
    dev.close()
    assert np.all(np.abs(got[..., off:off + cout].astype(np.float64) - want) <= bound)
    assert np.all(got[..., :off] == sentinel) and np.all(got[..., off + cout:] == sentinel)


def test_create_names_what_is_wrong(engine):
    """cpx_graph_create checks the groups and keeps the existing kinds' limits."""
    from cpx import _lib
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(3)
    w = rng.normal(0, 0.1, size=(12, 3, 3, 4)).astype(np.float32)
    g = Graph(conv_graph(w, np.zeros(12, np.float32), 1, tb.SAME, (9, 9), 2))

    def refused(change):
        plan = build_plan(g, input_shape=(9, 9, 8), grouped_convolutions=True)
        change(plan.ops[0])
        with pytest.raises(_lib.CpxError) as e:
            GraphDevice(engine, plan)
        return str(e.value)

    assert "number of groups" in refused(lambda o: setattr(o, "groups", 1))
    assert "input channels" in refused(lambda o: setattr(o, "groups", 3))
    assert "output channels" in refused(lambda o: setattr(o, "groups", 8))   # 8 divides the 8 inputs, not the 12 outputs
    assert "strides are 1 to 3" in refused(lambda o: setattr(o, "stride_h", 4))
    # an ungrouped CONV keeps its limit of 2
    w1 = rng.normal(0, 0.1, size=(16, 3, 3, 8)).astype(np.float32)
    g1 = Graph(conv_graph(w1, np.zeros(16, np.float32), 2, tb.SAME, (9, 9)))
    plan = build_plan(g1, input_shape=(9, 9, 8))
    plan.ops[0].stride_h = plan.ops[0].stride_w = 3
    plan.tensors[plan.output].H = plan.tensors[plan.output].W = 3
    with pytest.raises(_lib.CpxError, match="bad stride"):
        GraphDevice(engine, plan)


# ---- the whole network ----
# Measured on an MI355X (WR-ResNet-22-4, 160 x 160 x 2, N = 2, 17 logits): see DESIGN.md section 6.
#   dev  = max |device logits - hybrid restatement|
#   yard = max |hybrid restatement - float64 of the dequantised graph|: the quantisation noise itself
# An activation off by one float32 ulp may flip a later q by one step, so dev has no derived bound; the device may
# deviate by four times what was measured (the box-to-box allowance of test_tflite_q8_gpu.py for a maximum over the logits).
#   measured: dev = 5.96e-8 (one float32 ulp of one logit), yard = 0.01082, float math on the fused kernels vs hybrid
#   0.01082, spread of the logits 0.2356: tolerance 2.4e-7 <= yard / 4 = 2.7e-3 and spread >= 100 x tolerance hold.
WHOLE_NET_DEV = 5.96e-8
WHOLE_NET_MULTIPLE = 4.0
SIGMOID_ROUNDING = 4 * 2.0 ** -24   # predict hands out LOGISTIC of the logits (test_tflite_q8_gpu.py)
WR_TOL = 2e-4   # what tests/test_cnn_gpu.py and test_evaluator_matches_the_network_oracle hold the network to


@pytest.fixture(scope="module")
def network():
    import cnn_oracle as co
    from cpx.ml_tools import wrresnet as wr
    from cpx.ml_tools.tflite_reader import Graph

    x = np.random.default_rng(2).uniform(0, 255, size=(2, 160, 160, 2)).astype(np.float32)
    w = co.calibrate_bn(wr.random_weights(17, seed=3), x)
    blob = tb.wrresnet(w)
    return w, x, blob, Graph(blob)


def test_wrresnet_float32_file_on_the_graph_executor(engine, network):
    import torch

    from cpx.ml_tools import wrresnet as wr

    w, x, blob, g = network
    logits_t = g.ops[-1]["inputs"][0]
    _, plan, logits = run(engine, blob, x, output=logits_t)
    assert kinds(plan).count("CONV_GROUPED") == 22 and "CONV" not in kinds(plan)
    want = te.evaluate(g, x)[logits_t]
    net = wr.WRResNetDevice(engine, w, 17)
    fused = net.forward(torch.from_numpy(x).to(engine.device))[0].cpu().numpy()
    net.close()
    e64, ef = float(np.abs(logits - want).max()), float(np.abs(logits - fused).max())
    print("graph executor vs float64: %.4g; vs the fused network: %.4g; launches: %d" % (e64, ef, len(plan.ops)))
    assert logits.shape == want.shape == (2, 17) and e64 <= WR_TOL
    assert ef <= 2 * WR_TOL   # each is within WR_TOL of the same yardstick
    assert float(np.ptp(want, axis=1).min()) > 100 * WR_TOL


def test_wrresnet_quantised_file_on_the_graph_executor(engine, network):
    import torch

    from cpx.ml_tools import wrresnet as wr
    from cpx.ml_tools.tflite_reader import Graph, convert

    w, x, blob, _ = network
    qblob = tq.quantise(blob)
    g = Graph(qblob)
    logits_t = g.ops[-1]["inputs"][0]
    hyb, _ = tgr.evaluate_hybrid(g, x)
    deq = tq8.evaluate_dequantised(g, x)
    _, plan, logits = run(engine, qblob, x, output=logits_t)
    assert kinds(plan).count("CONV_Q8_GROUPED") == 20 and kinds(plan).count("CONV_GROUPED") == 2 and kinds(plan).count("FC_Q8") == 1
    # float math on the fused path: the filters multiplied out, the fused kernels in their default math
    net = wr.WRResNetDevice(engine, convert(g, quantised_math="float"), 17)
    flogits = net.forward(torch.from_numpy(x).to(engine.device))[0].cpu().numpy()
    net.close()
    dev = float(np.abs(logits - hyb[logits_t]).max())
    yard = float(np.abs(hyb[logits_t] - deq[logits_t]).max())
    other = float(np.abs(flogits - logits).max())
    spread = min(float(np.ptp(deq[logits_t], axis=1).min()), float(np.ptp(deq[logits_t], axis=0).max()))
    print("device vs hybrid restatement: %.4g; hybrid restatement vs float64 of the dequantised graph: %.4g; float math on the "
          "fused kernels vs hybrid: %.4g; spread of the logits %.4g" % (dev, yard, other, spread))
    tol = WHOLE_NET_MULTIPLE * WHOLE_NET_DEV
    assert dev <= tol, (dev, tol)
    assert tol <= yard / 4, (tol, yard)      # or the test is vacuous
    assert spread >= 100 * tol, (spread, tol)
    assert other <= 2 * yard, (other, yard)


# ---- through the public interface ----
@pytest.fixture(scope="module")
def quantised_model(tmp_path_factory):
    """A dynamic-range quantised WR-ResNet-22-4 file + sidecar, as the reference's converter writes its own network
    (BatchNorm-calibrated on a recorded classify input, as test_classifier_gpu.py's model)."""
    import cnn_oracle as co
    from cpx.ml_tools import wrresnet as wr
    from helpers import GOLDEN

    d = tmp_path_factory.mktemp("wrq8")
    z = np.load(os.path.join(GOLDEN, "hedgehog_classify_fs32.npz"))
    w = co.calibrate_bn(wr.random_weights(len(LABELS17), seed=11), z["t0_input"])
    blob = tq.quantise(tb.wrresnet(w))
    (d / "wrq8.tflite").write_bytes(blob)
    with open(d / "wrq8.json", "w") as fh:
        json.dump({"labels": LABELS17, "hyperparams": {"frame_size": 32}, "type": "thermal", "version": "test"}, fh)
    return d, blob, z["t0_input"]


def _config(d):
    from cpx.config import Config
    from cpx.config.config import ModelConfig

    cfg = Config.get_defaults()
    cfg.tracking["thermal"].denoise = False
    cfg.classify.models = [ModelConfig.load({"id": 9, "name": "wrq8", "model_file": str(d / "wrq8.tflite")})]
    return cfg


def _tags(directory):
    out = {}
    for name in ("possum", "hedgehog"):
        with open(os.path.join(str(directory), name + ".txt")) as fh:
            meta = json.load(fh)
        assert len(meta["tracks"]) > 0
        out[name] = [(t["id"], t["predictions"][0]["tag"]) for t in meta["tracks"]]
    return out


def test_quantised_wrresnet_through_the_public_interface(tmp_path, monkeypatch, quantised_model):
    from cpx import _lib
    from cpx.classify.clipclassifier import ClipClassifier
    from cpx.ml_tools.interpreter import LiteInterpreter, WRResNetInterpreter, get_interpreter
    from cpx.ml_tools.tflite_reader import Graph
    from helpers import GOLDEN

    d, blob, recorded = quantised_model
    cfg = _config(d)
    monkeypatch.delenv("CPX_TFLITE_QUANT_MATH", raising=False)
    interp = get_interpreter(cfg.classify.models[0])
    assert isinstance(interp, LiteInterpreter)
    plan = next(iter(interp._plans.values()))
    assert sum(o.kind == _lib.GRAPH_CONV_Q8_GROUPED for o in plan.ops) == 20
    g = Graph(blob)
    x = np.ascontiguousarray(recorded[:2], np.float32)
    got = interp.predict(x)
    want = tgr.evaluate_hybrid(g, x)[0][g.outputs[0]]
    err = float(np.abs(got - want).max())
    print("predict vs the hybrid restatement (probabilities): %.4g" % err)
    assert got.shape == want.shape == (2, 17) and err <= WHOLE_NET_MULTIPLE * WHOLE_NET_DEV + SIGMOID_ROUNDING
    # the batched many-file path, with either arithmetic; the one-file path
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
        one = tmp_path / (mode + "_one")
        one.mkdir()
        shutil.copy(os.path.join(GOLDEN, "possum.cptv"), one / "possum.cptv")
        meta = ClipClassifier(cfg).process_file(str(one / "possum.cptv"), track=True)
        # (the one-file path draws its own segments: its tags are not the batched path's)
        assert meta and meta["models"][0]["id"] == 9 and os.path.exists(one / "possum.txt")
        assert [t["id"] for t in meta["tracks"]] == [i for i, _ in tags[mode]["possum"]]
        assert all(t["predictions"][0]["tag"] in LABELS17 for t in meta["tracks"])
    assert tags["hybrid"] == tags["float"]
    finterp = get_interpreter(cfg.classify.models[0])   # CPX_TFLITE_QUANT_MATH=float is still set
    assert isinstance(finterp, WRResNetInterpreter) and finterp._weights["res2b0_branch2a/kernel"].dtype == np.float32
