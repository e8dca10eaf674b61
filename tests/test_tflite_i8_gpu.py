"""The full-integer operators of the TFLite graph executor (CPX_GRAPH_QUANTIZE .. CPX_GRAPH_MEAN_I8 and SLICE on bytes,
csrc/cpx_graph_i8.hip) on the GPU against the NumPy restatement of their arithmetic (tests/tflite_eval_i8.py, which reads
the Graph only).  Every step is integer, or one exact float32 operation at the two ends, so the comparison is
np.array_equal on the dequantised output: no tolerance.  The flatbuffers are synthetic (tests/tflite_build_i8.py); parity
with a TFLite runtime is not pinned, as for every other file kind."""
import json

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_i8 as ti
import tflite_eval_i8 as te8

pytestmark = pytest.mark.gpu

LABELS17 = ["bird", "cat", "deer", "dog", "false-positive", "hedgehog", "human", "kiwi", "leporidae", "mustelid", "penguin",
            "possum", "rodent", "sheep", "vehicle", "wallaby", "land-bird"]


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
    plan = build_plan(g, input_shape=x.shape[1:], output=output, integer_activations=True, grouped_convolutions=True, **options)
    dev = GraphDevice(engine, plan)
    out = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device)).cpu().numpy()
    dev.close()
    return g, plan, out


def kinds(plan):
    from cpx import _lib

    names = {getattr(_lib, "GRAPH_" + k): k for k in ("QUANTIZE", "DEQUANTIZE", "CONV_I8", "CONV_I8_GROUPED", "DWCONV_I8", "FC_I8",
                                                      "ADD_I8", "MUL_I8", "MAX_POOL_I8", "AVG_POOL_I8", "MEAN_I8", "SLICE")}
    return [names.get(o.kind, o.name) for o in plan.ops]


def check(engine, blob, x, what, expect_kinds=None, **options):
    """The forward's output equals the restatement's, bit for bit."""
    g, plan, got = run(engine, blob, x, **options)
    want = te8.evaluate(g, x)[g.outputs[0]]
    if expect_kinds is not None:
        assert kinds(plan) == expect_kinds, kinds(plan)
    differ = int((got.reshape(want.shape) != want).sum())
    print("%s: %d of %d elements differ" % (what, differ, want.size))
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want), what
    return g, plan, got


def levels(rng, shape, qp):
    """float32 samples that sit exactly on the levels of (scale, zero point), every level of [-128, 127] equally likely,
    both ends present."""
    q = rng.integers(-128, 128, size=shape)
    q.reshape(-1)[:2] = (-128, 127)
    return (np.float32(qp[0]) * (q - qp[1]).astype(np.float32)).astype(np.float32)


# the three input tensors of every convolution case: zero point -128 (an all-positive tensor), one inside, one POSITIVE -- a
# padded tap staged as 0 instead of z_in shows at every border of the last two
IN_QPS = ((np.float32(0.02), -128), (np.float32(0.03), 3), (np.float32(0.017), 90))


def random_filter(rng, shape, k_products, s_in, per_channel_axis=0):
    """-> (int8 filter, per-channel scales, int32 bias, an output scale that puts the accumulators' spread at ~60 steps)."""
    w = rng.integers(-127, 128, size=shape).astype(np.int8)
    co = shape[per_channel_axis]
    ws = (rng.uniform(0.5, 1.5, size=co) * 0.01).astype(np.float32)
    spread = np.sqrt(k_products) * 74.0 * 73.0
    bias = rng.integers(-int(spread / 2), int(spread / 2) + 1, size=co).astype(np.int32)
    return w, ws, bias, np.float32(float(s_in) * 0.01 * spread / 60.0)


def conv_graph(rng, kh, kw, stride, padding, cin, cout, hw, in_qp, act=tb.NONE, groups=1, z_out=-11):
    m, q = ti.start([1, hw[0], hw[1], cin], in_qp)
    w, ws, bias, s_out = random_filter(rng, (cout, kh, kw, cin // groups), kh * kw * cin // groups, in_qp[0])
    return ti.finish(m, m.conv_i8(q, w, ws, bias, (s_out, z_out), stride, padding, act))


def shapes_of(size):
    """A square map and a non-square one with its H / W twin."""
    return ((size, size), (size, size + 4), (size + 4, size))


# ---- (a) the operand map, with exact integers ----
@pytest.mark.parametrize("cout", [64, 40])
def test_operand_map_exact(engine, cout):
    """Integers in, integers out: scales 1 and zero points 0 at the input and the filter, the asymmetric filter
    w[co][ci] = ((7 co + 13 ci) mod 255) - 127, an output scale of 2^10 so that MBQM is an exact rounding shift.  A wrong
    A / B / C lane map or a swapped row / column shows here."""
    rng = np.random.default_rng(40 + cout)
    x = rng.integers(-128, 128, size=(1, 8, 8, 64)).astype(np.float32)
    x[0, 0, 0, 0], x[0, 7, 7, 63] = -128.0, 127.0
    co, ci = np.mgrid[0:cout, 0:64]
    w = (((7 * co + 13 * ci) % 255) - 127).astype(np.int8)
    m, q = ti.start([1, 8, 8, 64], (np.float32(1.0), 0))
    y = m.conv_i8(q, w.reshape(cout, 1, 1, 64), np.ones(cout, np.float32), None, (np.float32(1024.0), 0))
    g, plan, got = run(engine, ti.finish(m, y), x)
    assert kinds(plan) == ["QUANTIZE", "CONV_I8", "DEQUANTIZE"]
    acc = x.reshape(64, 64).astype(np.int64) @ w.astype(np.int64).T
    assert not np.array_equal(w[:40, :40], w[:40, :40].T)
    # acc / 2^10 rounded half away from zero for acc >= 0, half towards zero below (SRDHM by 2^30, shift -9: by hand)
    want = np.clip(te8.mbqm(acc, 2 ** 30, -9), -128, 127)
    assert len(np.unique(want)) > 100
    assert np.array_equal(got.reshape(64, cout).astype(np.int64) // 1024, want) and np.array_equal(got % 1024, np.zeros_like(got))


# ---- (b) MBQM's ties, through the kernel ----
def test_mbqm_ties_through_conv(engine):
    """A 1 x 1 CONV_I8 with the diagonal filter w[c][c] = 1 and a crafted INT32 bias: channel c's accumulator is q[c] +
    bias[c].  Multipliers of exactly 1/2 (channels 0..15) and 1/4 (16..31); accumulators +-1, +-3, +-5 and the saturating
    ends; outputs clamped at -128, at 127 and at a RELU6 bound."""
    w = np.zeros((32, 1, 1, 32), np.int8)
    w[np.arange(32), 0, 0, np.arange(32)] = 1
    accs = np.array([1, -1, 3, -3, 5, -5, 0, 2, -2, 600, -600, 253, 255, -255, 257, -257], np.int64)
    q = np.tile(np.array([1, -1, 3, -3, 5, -5, 0, 2, -2, 100, -100, 127, 127, -128, 127, -128], np.int64), 2)
    bias = (np.tile(accs, 2) - q).astype(np.int32)
    ws = np.concatenate([np.full(16, 0.5), np.full(16, 0.25)]).astype(np.float32)
    for act, out_qp in ((tb.NONE, (np.float32(1.0), 0)), (tb.RELU6, (np.float32(1.0), -2)), (tb.RELU, (np.float32(1.0), 1))):
        m, t = ti.start([1, 1, 2, 32], (np.float32(1.0), 0))
        y = m.conv_i8(t, w, ws, bias, out_qp, 1, tb.SAME, act)
        x = np.stack([q, q[::-1]]).reshape(1, 1, 2, 32).astype(np.float32)
        g, plan, got = check(engine, ti.finish(m, y), x, "ties act %d" % act)
        if act == tb.NONE:
            # by hand: x / 2 -> 1, 0, 2, -1, 3, -2 (a positive tie up, a negative one towards zero); the ends saturate
            assert list(got[0, 0, 0, :6]) == [1, 0, 2, -1, 3, -2] and got[0, 0, 0, 9] == 127 and got[0, 0, 0, 10] == -128
            # x / 4 rounds twice: 5 -> SRDHM 3 -> RDivPOT(3, 1) = 2; -5 -> -2 -> -1
            assert list(got[0, 0, 0, 16:22]) == [1, 0, 1, -1, 2, -1]
        if act == tb.RELU6:
            assert got.max() == 6.0 and got.min() == 0.0   # q in [-2, 4] at zero point -2


# ---- (c) convolutions at the smallest shapes that can go wrong ----
CONV_CASES = [
    # kh, kw, stride, padding, cin, cout, size
    (1, 1, 1, tb.SAME, 192, 320, 8),
    (3, 3, 2, tb.SAME, 80, 192, 17),      # one-sided pads
    (3, 3, 2, tb.VALID, 36, 40, 9),       # the byte path, a partial chunk and a partial tile
    (3, 3, 1, tb.SAME, 3, 32, 9),         # the layer behind QUANTIZE
    (1, 7, 1, tb.SAME, 136, 160, 17),
    (7, 1, 2, tb.SAME, 40, 24, 8),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "%dx%d_s%d_p%d_%d_%d_%d" % c)
def test_conv_i8(engine, case):
    kh, kw, stride, padding, cin, cout, size = case
    for k, in_qp in enumerate(IN_QPS):
        for hw in (shapes_of(size) if k == 2 else (shapes_of(size)[0],)):
            rng = np.random.default_rng([kh, kw, cin, cout, k, hw[0], hw[1]])
            blob = conv_graph(rng, kh, kw, stride, padding, cin, cout, hw, in_qp, act=(tb.NONE, tb.RELU, tb.RELU6)[k])
            check(engine, blob, levels(rng, (2, hw[0], hw[1], cin), in_qp), "conv %s z_in %d %s" % (case, in_qp[1], hw),
                  ["QUANTIZE", "CONV_I8", "DEQUANTIZE"])


@pytest.mark.parametrize("cg", [8, 32])
def test_conv_i8_grouped(engine, cg):
    """3 x 3, stride 3, G = 2: Cg = 8 stages byte by byte, Cg = 32 sixteen bytes at a time."""
    for k, in_qp in enumerate(IN_QPS):
        for hw in (shapes_of(10) if k == 2 else ((10, 10),)):
            rng = np.random.default_rng([33, cg, k, hw[0], hw[1]])
            blob = conv_graph(rng, 3, 3, 3, tb.SAME, 2 * cg, 48, hw, in_qp, groups=2)
            check(engine, blob, levels(rng, (3, hw[0], hw[1], 2 * cg), in_qp), "grouped Cg %d z_in %d %s" % (cg, in_qp[1], hw),
                  ["QUANTIZE", "CONV_I8_GROUPED", "DEQUANTIZE"])


@pytest.mark.parametrize("cg", [8, 32])
@pytest.mark.parametrize("cog", [40, 72])
def test_conv_i8_grouped_over_several_tiles(engine, cog, cg):
    """The grouped kernel with two tiles per wave (Cog = 40: the second one partial) and with four (Cog = 72: three tiles,
    above 64 channels per group), byte by byte and sixteen bytes at a time; N = 3 samples of 10 x 10 at stride 3."""
    rng = np.random.default_rng([34, cg, cog])
    blob = conv_graph(rng, 3, 3, 3, tb.SAME, 2 * cg, 2 * cog, (10, 10), IN_QPS[2], groups=2)
    check(engine, blob, levels(rng, (3, 10, 10, 2 * cg), IN_QPS[2]), "grouped Cg %d Cog %d" % (cg, cog),
          ["QUANTIZE", "CONV_I8_GROUPED", "DEQUANTIZE"])


@pytest.mark.parametrize("c_first", [16, 5])
def test_conv_i8_inside_a_concatenation(engine, c_first):
    """Two convolutions write into the channel slices of a concatenated tensor (the second at channel offset 16 or 5 of a
    wider tensor); a third reads the second's slice where it lies (c_offset = 16: sixteen bytes at a time; 5: bytes), a
    fourth the whole concatenation."""
    rng = np.random.default_rng(70 + c_first)
    in_qp, mid_qp = IN_QPS[2], (np.float32(0.05), 40)
    m, q = ti.start([1, 9, 9, 24], in_qp)

    def conv(x, cin, cout, k, out_qp, qp_in):
        w, ws, bias, s_out = random_filter(rng, (cout, k, k, cin), k * k * cin, qp_in[0])
        # (the two parts of a concatenation carry ITS parameters: the output scale is given, the filter scales follow)
        ws = (ws * (float(out_qp[0]) / float(s_out))).astype(np.float32) if out_qp[0] is not None else ws
        return m.conv_i8(x, w, ws, bias, (s_out if out_qp[0] is None else out_qp[0], out_qp[1]), 1, tb.SAME)

    a = conv(q, 24, c_first, 1, mid_qp, in_qp)
    b = conv(q, 24, 32, 3, mid_qp, in_qp)
    cat = m.concat_i8([a, b])
    y1 = conv(b, 32, 20, 3, (None, -5), mid_qp)
    y2 = conv(cat, c_first + 32, 20, 1, (None, 9), mid_qp)
    out = m.binary_i8("ADD", y1, y2, (np.float32(2.0 * max(m.qp(y1)[0], m.qp(y2)[0])), 2))
    g, plan, got = check(engine, ti.finish(m, out), levels(rng, (2, 9, 9, 24), in_qp), "concatenation, first part %d" % c_first)
    assert kinds(plan) == ["QUANTIZE", "CONV_I8", "CONV_I8", "CONV_I8", "CONV_I8", "ADD_I8", "DEQUANTIZE"]
    assert plan.tensors[b].c_offset == c_first and plan.tensors[b].c_stride == c_first + 32


def test_tile_across_samples_and_batch_independence(engine):
    """A 5 x 5 map at N = 7: 175 pixels, so the first 128-pixel tile ends inside sample 5.  Each sample alone gives the
    same rows."""
    rng = np.random.default_rng(80)
    in_qp = IN_QPS[1]
    blob = conv_graph(rng, 3, 3, 1, tb.SAME, 48, 40, (5, 5), in_qp)
    x = levels(rng, (7, 5, 5, 48), in_qp)
    _, _, got = check(engine, blob, x, "N = 7")
    for n in range(7):
        assert np.array_equal(run(engine, blob, x[n:n + 1])[2][0], got[n])


# ---- (d) depthwise ----
DW_CASES = [(3, 1, tb.SAME, 32, 9), (3, 2, tb.SAME, 32, 9), (3, 1, tb.SAME, 20, 9), (3, 2, tb.SAME, 20, 10), (5, 1, tb.SAME, 16, 9),
            (3, 2, tb.VALID, 24, 11)]


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "k%d_s%d_p%d_c%d_%d" % c)
def test_dwconv_i8(engine, case):
    """Positive zero points: a padded tap that contributed z_in * w instead of nothing shows at every border.  C = 32 and
    16 move sixteen bytes per lane, C = 20 and 24 go channel by channel; stride 2 on an even map pads one side only."""
    k, stride, padding, c, size = case
    for in_qp in IN_QPS[1:]:
        for hw in shapes_of(size):
            rng = np.random.default_rng([k, stride, c, in_qp[1], hw[0], hw[1]])
            m, q = ti.start([1, hw[0], hw[1], c], in_qp)
            w, ws, bias, s_out = random_filter(rng, (1, k, k, c), k * k, in_qp[0], per_channel_axis=3)
            y = m.depthwise_i8(q, w, ws, bias, (s_out, 17), stride, padding, tb.RELU6 if c == 32 else tb.NONE)
            check(engine, ti.finish(m, y), levels(rng, (2, hw[0], hw[1], c), in_qp), "depthwise %s z_in %d %s" % (case, in_qp[1], hw),
                  ["QUANTIZE", "DWCONV_I8", "DEQUANTIZE"])


def test_fc_i8(engine):
    rng = np.random.default_rng(90)
    for in_qp in IN_QPS:
        m, q = ti.start([1, 1, 1, 130], in_qp)
        w, ws, bias, s_out = random_filter(rng, (17, 130), 130, in_qp[0])
        y = m.dense_i8(q, w, ws[:1], bias, (s_out, -3), tb.RELU if in_qp[1] > 0 else tb.NONE)
        check(engine, ti.finish(m, y), levels(rng, (5, 1, 1, 130), in_qp), "FC z_in %d" % in_qp[1], ["QUANTIZE", "FC_I8", "DEQUANTIZE"])


# ---- (e) element and window operators ----
@pytest.mark.parametrize("name", ["ADD", "SUB", "MUL"])
@pytest.mark.parametrize("c", [32, 20])
def test_binary_i8(engine, name, c):
    """Two activations with scales a factor 37 apart, and an activation by a per-channel constant."""
    rng = np.random.default_rng([ord(name[0]), c])
    qa, qb = (np.float32(0.01), -20), (np.float32(0.37), 35)
    out = (np.float32(0.2), -6) if name != "MUL" else (np.float32(0.37 * 0.01 * 60), 10)
    m, q = ti.start([1, 6, 7, c], qa)
    b = m.quantize(q, qb)                  # the same values, requantised onto the coarse scale
    y = m.binary_i8(name, q, b, out, tb.RELU if name == "ADD" else tb.NONE)
    x = levels(rng, (3, 6, 7, c), qa)
    check(engine, ti.finish(m, y), x, "%s of two activations" % name,
          ["QUANTIZE", "QUANTIZE", "ADD_I8" if name != "MUL" else "MUL_I8", "DEQUANTIZE"])
    m, q = ti.start([1, 6, 7, c], qa)
    konst = m.qconst(rng.integers(-128, 128, size=c).astype(np.int8), qb)
    y = m.binary_i8(name, q, konst, out, tb.NONE, const_first=name != "SUB")
    check(engine, ti.finish(m, y), x, "%s by a constant" % name, ["QUANTIZE", "ADD_I8" if name != "MUL" else "MUL_I8", "DEQUANTIZE"])


@pytest.mark.parametrize("c", [16, 12])
def test_pools_i8(engine, c):
    """AVERAGE_POOL with negative sums and odd counts (4, 6 and 9 elements at the border of a SAME 3 x 3 window), MAX_POOL;
    a square map and a non-square one with its twin."""
    qp = (np.float32(0.1), 100)   # most levels lie below the zero point: negative sums of q
    for kind, k, stride, padding, act in (("AVERAGE_POOL_2D", 3, 1, tb.SAME, tb.NONE), ("AVERAGE_POOL_2D", 2, 2, tb.VALID, tb.RELU),
                                          ("MAX_POOL_2D", 3, 2, tb.SAME, tb.NONE), ("MAX_POOL_2D", 3, 2, tb.VALID, tb.RELU6)):
        for hw in shapes_of(7):
            rng = np.random.default_rng([k, stride, c, hw[0], hw[1]])
            m, q = ti.start([1, hw[0], hw[1], c], qp)
            y = m.pool_i8(kind, q, k, stride, padding, act)
            check(engine, ti.finish(m, y), levels(rng, (2, hw[0], hw[1], c), qp), "%s %d %s" % (kind, k, hw),
                  ["QUANTIZE", "MAX_POOL_I8" if kind[0] == "M" else "AVG_POOL_I8", "DEQUANTIZE"])


@pytest.mark.parametrize("hw", [(7, 7), (20, 20), (4, 9), (9, 4)])
@pytest.mark.parametrize("c", [32, 10])
def test_mean_i8(engine, hw, c):
    rng = np.random.default_rng([hw[0], hw[1], c])
    qp = (np.float32(0.05), -30)
    m, q = ti.start([1, hw[0], hw[1], c], qp)
    y = m.mean_i8(q, (np.float32(0.021), 12))
    x = levels(rng, (3, hw[0], hw[1], c), qp)
    x[1] = x[1, :1, :1]   # a constant sample: the mean is its level
    check(engine, ti.finish(m, y), x, "MEAN %s x %d" % (hw, c), ["QUANTIZE", "MEAN_I8", "DEQUANTIZE"])


def test_quantize_ties_ends_and_requantisation(engine):
    """QUANTIZE of values on ties and beyond both ends (NaN and the infinities among them), then int8 -> int8."""
    for c in (16, 3):
        for qp in ((np.float32(0.5), -7), (np.float32(0.013), 120)):
            ties = (np.arange(-200, 200) + 0.5).astype(np.float32) * qp[0]
            x = np.concatenate([ties, np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 3e-39], np.float32)])
            x = np.resize(x, (2, 3, 17 * 4, c)).astype(np.float32)
            m, q = ti.start([1, 3, 17 * 4, c], qp)
            y = m.quantize(q, (np.float32(0.031), 5))
            g, plan, got = check(engine, ti.finish(m, y), x, "QUANTIZE %s x %d" % (qp, c), ["QUANTIZE", "QUANTIZE", "DEQUANTIZE"])
            first = te8.evaluate(g, x)[q]
            assert first.min() == -128 and first.max() == 127 and first.reshape(-1)[400] == qp[1]   # (the NaN)


@pytest.mark.parametrize("c", [16, 6])
def test_pad_and_strided_slice_i8(engine, c):
    """PAD and a strided SLICE with a non-zero zero point: the zero region is the zero point, a real 0 behind DEQUANTIZE."""
    qp = (np.float32(0.25), 77)
    for hw in shapes_of(7):
        rng = np.random.default_rng([c, hw[0], hw[1]])
        x = levels(rng, (2, hw[0], hw[1], c), qp)
        m, q = ti.start([1, hw[0], hw[1], c], qp)
        y = m.pad_i8(q, [[0, 0], [1, 2], [0, 3], [0, 0]])
        _, _, got = check(engine, ti.finish(m, y), x, "PAD %s" % (hw,), ["QUANTIZE", "SLICE", "DEQUANTIZE"])
        assert np.all(got[:, 0] == 0.0) and np.all(got[:, :, -3:] == 0.0)
        m, q = ti.start([1, hw[0], hw[1], c], qp)
        y = m.strided_slice_i8(q, [0, 1, 2, 0], [0, 0, 0, 0], [1, 2, 3, 1], begin_mask=0b1001, end_mask=0b1111)
        check(engine, ti.finish(m, y), x, "STRIDED_SLICE %s" % (hw,), ["QUANTIZE", "SLICE", "DEQUANTIZE"])
        # a PAD in front of a VALID depthwise convolution: folded with fold_windows, a SLICE without; the same bits
        m, q = ti.start([1, hw[0], hw[1], c], qp)
        w, ws, bias, s_out = random_filter(rng, (1, 3, 3, c), 9, qp[0], per_channel_axis=3)
        y = m.depthwise_i8(m.pad_i8(q, [[0, 0], [0, 1], [0, 1], [0, 0]]), w, ws, bias, (s_out, 3), 2, tb.VALID)
        blob = ti.finish(m, y)
        _, _, a = check(engine, blob, x, "PAD > DW", ["QUANTIZE", "SLICE", "DWCONV_I8", "DEQUANTIZE"])
        _, _, b = check(engine, blob, x, "PAD > DW folded", ["QUANTIZE", "DWCONV_I8", "DEQUANTIZE"], fold_windows=True)
        assert np.array_equal(a, b)


# ---- (f) whole networks ----
def _wrresnet_i8(float_tail=True):
    from cpx.ml_tools import wrresnet as wr

    rng = np.random.default_rng(5)
    blob = tb.wrresnet(wr.random_weights(17, seed=5), size=32)
    return ti.quantise_full(blob, rng.normal(0, 1, size=(4, 32, 32, 2)), float_tail=float_tail)


def _mobilenet_i8(float_tail=True):
    rng = np.random.default_rng(6)
    return ti.quantise_full(ti.mobilenet_v2_blocks(5, size=48), rng.normal(0, 1, size=(4, 48, 48, 3)), float_tail=float_tail)


@pytest.fixture(scope="module")
def networks():
    from cpx.ml_tools.tflite_reader import Graph

    out = {}
    for name, blob, shape in (("wrresnet", _wrresnet_i8(), (5, 32, 32, 2)), ("mobilenet_v2", _mobilenet_i8(), (5, 48, 48, 3))):
        g = Graph(blob)
        x = np.random.default_rng(len(name)).normal(0, 1, size=shape).astype(np.float32)
        logits_t = next(op["outputs"][0] for op in g.ops if op["name"] == "DEQUANTIZE")
        out[name] = (blob, x, logits_t, te8.evaluate(g, x))
    return out


@pytest.mark.parametrize("name", ["wrresnet", "mobilenet_v2"])
def test_whole_network_logits_bit_equal(engine, networks, name):
    """The logits -- the DEQUANTIZE behind the last FULLY_CONNECTED -- of the WR-ResNet stand-in at 32 x 32 (grouped
    convolutions, MUL and ADD by INT8 constants) and of a three-block MobileNetV2 at 48 x 48, at N = 1 and N = 5, with the
    window folds on and off."""
    blob, x, logits_t, want = networks[name]
    outs = []
    for fold in (False, True):
        for n in (1, 5):
            g, plan, got = run(engine, blob, x[:n], output=logits_t, fold_windows=fold)
            differ = int((got != want[logits_t][:n]).sum())
            print("%s fold_windows %s N %d: %d of %d logits differ, launches %s" % (name, fold, n, differ, got.size, plan.census()))
            assert np.array_equal(got, want[logits_t][:n])
            outs.append(got)
    assert len(np.unique(want[logits_t])) > 5   # (the logits are not saturated)


def test_lite_interpreter_runs_a_full_integer_file(engine, networks, tmp_path):
    from cpx.ml_tools.interpreter import LiteInterpreter

    blob, x, logits_t, want = networks["wrresnet"]
    (tmp_path / "wr_i8.tflite").write_bytes(blob)
    with open(tmp_path / "wr_i8.json", "w") as fh:
        json.dump({"labels": LABELS17, "hyperparams": {"frame_size": 32, "model_name": "wr-resnet"}, "type": "thermal", "version": "test"}, fh)
    interp = LiteInterpreter(tmp_path / "wr_i8.tflite", engine=engine)
    got = interp.predict(x[:3])
    # (behind the DEQUANTIZE the head is the float32 LOGISTIC kernel: one float32 expf and division per element)
    probs = 1.0 / (1.0 + np.exp(-want[logits_t][:3].astype(np.float64)))
    assert got.shape == (3, 17) and float(np.abs(got - probs).max()) <= 1e-6


def test_softmax_head_i8(engine):
    """An INT8 SOFTMAX is DEQUANTIZE -> the float32 kernel -> QUANTIZE.  Its int8 output equals round(p64 / s_out) + z_out of
    a float64 softmax of the restatement's logits, except where p64 / s_out lies within 1e-3 of a half-integer: there
    either neighbour is accepted, for at most 1 % of the elements."""
    from cpx.ml_tools.tflite_reader import Graph

    blob = _mobilenet_i8(float_tail=False)
    g = Graph(blob)
    x = np.random.default_rng(12).normal(0, 1, size=(40, 48, 48, 3)).astype(np.float32)
    _, plan, got = run(engine, blob, x)
    assert kinds(plan)[-4:] == ["DEQUANTIZE", "SOFTMAX", "QUANTIZE", "DEQUANTIZE"]
    vals = te8.evaluate(g, x)
    sm = next(op for op in g.ops if op["name"] == "SOFTMAX")
    s_out, z_out = te8._qp(g, sm["outputs"][0])
    logits = te8.dequantize(vals[sm["inputs"][0]], *te8._qp(g, sm["inputs"][0])).astype(np.float64)
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    t = (e / e.sum(axis=-1, keepdims=True)) / float(s_out)
    want = np.clip(te8.round_half_away(t) + z_out, -128, 127)
    near_tie = np.abs(t - np.floor(t) - 0.5) <= 1e-3
    q = np.round(got.astype(np.float64) / float(s_out)).astype(np.int64) + z_out
    print("SOFTMAX: %d of %d elements near a tie, %d differ" % (int(near_tie.sum()), t.size, int((q != want).sum())))
    assert near_tie.mean() <= 0.01
    assert np.all((q == want) | (near_tie & (np.abs(q - want) <= 1)))
