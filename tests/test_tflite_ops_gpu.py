"""The float32 operators of the graph executor's first commit, one by one, on the GPU: FULLY_CONNECTED (a second and a
33rd trip of graph_fc_kernel's lane loop, a ragged last trip, one input), SOFTMAX (logits that overflow expf without the
subtraction of the maximum, more than one pixel), ADD / SUB of two activations, AFFINE (every constant operator, as a launch
and folded into the convolution in front), LOGISTIC as a launch and the copies a CONCATENATION cannot avoid.  One-operator
graphs (plus a producer where a view is needed) of tests/tflite_build*.py, N = 3, against the float64 evaluation of the same
flatbuffer (tests/tflite_eval*.py) or, where the operator is one or two correctly rounded float32 operations, NumPy's bits."""
import numpy as np
import pytest

import tflite_build as tb
import tflite_build_se as ts
import tflite_eval as te
import tflite_eval_se as tes
from test_tflite_graph_gpu import CONV_REL, LOGIT_MULTIPLE
from tflite_aniso_cases import kinds

pytestmark = pytest.mark.gpu
F32 = np.float32
N = 3
H, W = 5, 3
# one correctly rounded float32 operation is within 2^-24 of its exact result
AFFINE_REL = 2.0 ** -22     # x * sc + sf against float64: the reciprocal's rounding plus the product's, each 2^-24, doubled
FLOOR = 2.0 ** -23          # of a measured float32-against-float64 yardstick


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def run(engine, blob, x, output=None, out_slice=None, out=None, **plan_kw):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    plan = build_plan(g, input_shape=x.shape[1:], output=output, **plan_kw)
    dev = GraphDevice(engine, plan, out_slice=out_slice)
    got = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device), out=out).cpu().numpy()
    dev.close()
    return g, plan, got


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_bits(what, got, want):
    n_diff = int((bits(got) != bits(want)).sum()) if got.shape == want.shape else -1
    print("%s: %d of %d elements differ from NumPy's" % (what, n_diff, got.size))
    assert got.shape == want.shape and want.dtype == F32 and n_diff == 0, (what, got.shape, want.shape, n_diff)


def start(c, h=H, w=W):
    m = ts.ModelSE()
    x = m.tensor([1, h, w, c], name="input")
    m.inputs = [x]
    return m, x


def through(m, t):
    """A 1 x 1 MAX_POOL_2D of stride 1: a launch that hands every value on as it is, so that its reader reads an
    activation of the arena and no fold removes that reader's launch."""
    return m.pool("MAX_POOL_2D", t, 1, 1, tb.VALID)


def yardstick(g, x, t):
    """What a float32 evaluation of the graph on the CPU deviates from the float64 one on tensor t; the device may deviate
    by LOGIT_MULTIPLE times that (tests/test_tflite_graph_gpu.py), with a floor of one float32 ulp of 1."""
    import torch

    v64 = tes.evaluate(g, x)[t]
    yard = float(np.abs(tes.evaluate(g, x, dtype=torch.float32)[t] - v64).max())
    return v64, yard, max(LOGIT_MULTIPLE * yard, FLOOR)


# ---- 1. FULLY_CONNECTED ----
def dense(m, x, w, b, act=tb.NONE):
    y = m.tensor([1, w.shape[0]])
    return m.op("FULLY_CONNECTED", [x, m.tensor(w.shape, w)] + ([] if b is None else [m.tensor(b.shape, b)]), [y], {0: ("b", act)})


def fc_weights(rng, cin, cout, bias):
    return (rng.normal(0, np.sqrt(2.0 / cin), size=(cout, cin)).astype(F32), rng.normal(0, 0.3, size=cout).astype(F32) if bias else None)


FC_CASES = [
    # Cin, Cout, bias, activation: graph_fc_kernel's lanes take k = lane, lane + 64, ...
    (1, 1, True, tb.NONE), (1, 17, False, tb.NONE),           # one lane has work
    (63, 1, False, tb.NONE), (63, 17, True, tb.NONE),         # one trip, the last lane idle
    (64, 1, True, tb.NONE), (64, 17, False, tb.NONE),         # exactly one trip
    (65, 1, False, tb.NONE), (65, 17, True, tb.RELU),         # a second trip for lane 0 alone
    (200, 1, True, tb.NONE), (200, 17, False, tb.NONE),       # four trips, the last ragged
    (2048, 1, False, tb.NONE), (2048, 17, True, tb.NONE),     # 32 trips
]


@pytest.mark.parametrize("case", FC_CASES, ids=lambda c: "%dto%d_%s%s" % (c[0], c[1], "bias" if c[2] else "nobias", "_relu" if c[3] else ""))
def test_fully_connected_against_float64(engine, case):
    cin, cout, bias, act = case
    rng = np.random.default_rng(cin * 100 + cout)
    m, x = start(cin, 1, 1)
    w, b = fc_weights(rng, cin, cout, bias)
    m.outputs = [dense(m, x, w, b, act)]
    xs = rng.uniform(-1, 1, size=(N, 1, 1, cin)).astype(F32)
    g, plan, got = run(engine, m.finish(), xs)
    assert kinds(plan) == ["FC"] and (plan.ops[0].shift is None) == (not bias)
    vals, mag = te.evaluate(g, xs, magnitudes=True)
    t = g.outputs[0]
    assert got.shape == vals[t].shape == (N, cout)
    rel = float((np.abs(got - vals[t]) / mag[t]).max())
    print("%s: max |error| / (sum |x| |w| + |b|) = %.3g (bound %.3g)" % (case, rel, CONV_REL))
    assert rel < CONV_REL
    if act == tb.RELU:
        assert (got == 0).any() and (got > 0).any() and float(got.min()) == 0


def test_fully_connected_reads_a_reshaped_mean(engine):
    """MEAN (keep_dims) -> RESHAPE -> FULLY_CONNECTED: the dense layer reads the MEAN's storage through the RESHAPE's view.
    Held to float64 on the means the device itself wrote."""
    rng = np.random.default_rng(77)
    c, cout = 65, 17
    m, x = start(c)
    mean = m.mean(x, keep_dims=True)
    w, b = fc_weights(rng, c, cout, True)
    m.outputs = [dense(m, m.reshape(mean, [1, c]), w, b)]
    xs = rng.uniform(-1, 1, size=(N, H, W, c)).astype(F32)
    blob = m.finish()
    g, plan, got = run(engine, blob, xs)
    assert kinds(plan) == ["MEAN", "FC"] and plan.tensors[plan.ops[1].in0].alias and plan.tensors[plan.ops[1].in0].storage == mean
    m2, x2 = start(c)      # (a tensor with a view cannot be handed out: the same MEAN as a graph of its own)
    m2.outputs = [m2.mean(x2, keep_dims=True)]
    means = run(engine, m2.finish(), xs)[2].astype(np.float64)
    assert means.shape == (N, c) and float(np.abs(means - xs.astype(np.float64).mean(axis=(1, 2))).max()) < 1e-6
    want = means @ w.astype(np.float64).T + b.astype(np.float64)
    mag = np.abs(means) @ np.abs(w.astype(np.float64)).T + np.abs(b.astype(np.float64))
    rel = float((np.abs(got - want) / mag).max())
    print("reshaped mean: max |error| / (sum |x| |w| + |b|) = %.3g (bound %.3g)" % (rel, CONV_REL))
    assert got.shape == want.shape and rel < CONV_REL


def test_fully_connected_batch_does_not_matter(engine):
    rng = np.random.default_rng(78)
    m, x = start(200, 1, 1)
    m.outputs = [dense(m, x, *fc_weights(rng, 200, 17, True))]
    blob = m.finish()
    xs = rng.uniform(-1, 1, size=(1, 1, 1, 200)).astype(F32)
    _, _, one = run(engine, blob, xs)
    _, _, five = run(engine, blob, np.repeat(xs, 5, axis=0))
    assert one.shape == (1, 17) and all(np.array_equal(bits(five[i]), bits(one[0])) for i in range(5)) and float(np.abs(one).max()) > 0.1


# ---- 2. SOFTMAX ----
def softmax_logits(kind, c, h, w):
    rng = np.random.default_rng(c * 10 + h)
    x = rng.uniform(-4, 4, size=(N, h, w, c)).astype(F32)
    if kind == "large":     # expf(80) fits, expf(1.5 * 80) and expf(1e4) do not: without the maximum's subtraction inf / inf
        x[0, ..., 0] = 80.0
        x[0, ..., c - 1] = -80.0
        x[1, ..., c // 2] = 1e4
        x[1, ..., 0] = -1e4
        x[2, ..., c - 1] = 80.0 if c == 1 else 1e4
        x[2, ..., 0] = -80.0 if c > 1 else x[2, ..., 0]
    return x


SOFTMAX_CASES = [
    # C, beta, logits, H, W
    (17, 1.0, "uniform", 1, 1), (17, 1.5, "uniform", 1, 1), (17, 1.0, "large", 1, 1), (17, 1.5, "large", 1, 1),
    (1, 1.0, "uniform", 1, 1), (1, 1.5, "large", 1, 1), (17, 1.5, "uniform", 3, 5), (17, 1.0, "large", 3, 5),
]


@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=lambda c: "c%d_beta%g_%s_%dx%d" % c)
def test_softmax_against_float64(engine, case):
    """The tolerance is measured, not fixed in advance: what float32 on the CPU deviates from float64 on the same graph,
    times LOGIT_MULTIPLE, with a floor of 2^-23 (expf's own error is the library's).  Measured on an MI355X: see DESIGN.md."""
    c, beta, kind, h, w = case
    m, x = start(c, h, w)
    m.outputs = [m.softmax(x, beta)]
    xs = softmax_logits(kind, c, h, w)
    g, plan, got = run(engine, m.finish(), xs)
    assert kinds(plan) == ["SOFTMAX"] and plan.ops[0].param == F32(beta)
    v64, yard, tol = yardstick(g, xs, g.outputs[0])
    v64 = v64.reshape(got.shape)
    err = float(np.abs(got - v64).max())
    rows = got.astype(np.float64).sum(axis=-1)
    top = np.take_along_axis(got, v64.argmax(axis=-1)[..., None], axis=-1) - v64.max(axis=-1, keepdims=True)
    print("%s: float32-CPU vs float64 %.3g, device vs float64 %.3g (tolerance %.3g); rows sum to 1 within %.3g"
          % (case, yard, err, tol, float(np.abs(rows - 1).max())))
    assert got.shape == ((N, c) if (h, w) == (1, 1) else (N, h, w, c))
    assert np.all(np.isfinite(got)) and float(np.abs(rows - 1).max()) < 1e-6
    assert float(np.abs(top).max()) <= tol and err <= tol
    if kind == "large" and c > 1:
        assert float(got.max(axis=-1).min()) > 0.4 and float(got.min()) == 0.0    # the entries at -80 and -1e4 underflow to 0
    if c == 1:
        assert np.all(got == 1.0)


# ---- 3. ADD / SUB of two activations ----
def add_graph(rng, name, order, act, c, into_slice=False):
    """a = the input, b = the input times a per-channel constant, each through a launch of its own; y = a (+|-) b in the
    given operand order.  into_slice: y is the channels [5, 5 + c) of a concatenation behind a 5-channel convolution."""
    m, x = start(c)
    a = through(m, x)
    b = through(m, m.binary("MUL", x, rng.uniform(0.5, 2.0, size=c).astype(F32)))
    y = m.binary(name, *((a, b) if order == "ab" else (b, a)), act)
    out, conv = y, None
    if into_slice:
        conv = m.conv(x, rng.normal(0, 0.3, size=(5, 1, 1, c)).astype(F32), rng.normal(size=5).astype(F32), 1, tb.SAME, tb.NONE)
        out = through(m, m.concat([conv, y]))     # (the concatenated tensor itself cannot be the graph's output)
    m.outputs = [out]
    return m.finish(), a, b, conv


def activated(v, act):
    return v if act == tb.NONE else np.maximum(v, F32(0)) if act == tb.RELU else np.clip(v, F32(0), F32(6))


@pytest.mark.parametrize("c", [8, 6])
@pytest.mark.parametrize("act", [tb.NONE, tb.RELU, tb.RELU6], ids=["none", "relu", "relu6"])
@pytest.mark.parametrize("name,order", [("ADD", "ab"), ("SUB", "ab"), ("SUB", "ba")])
def test_add_sub_of_two_activations_is_one_float32_operation(engine, name, order, act, c):
    """Exact: one float32 addition of the two float32 operands the device itself holds, then the clamp."""
    rng = np.random.default_rng(c + act + len(order + name))
    blob, a_t, b_t, _ = add_graph(rng, name, order, act, c)
    xs = rng.uniform(-4, 4, size=(N, H, W, c)).astype(F32)
    g, plan, got = run(engine, blob, xs)
    assert kinds(plan) == ["MAX_POOL", "AFFINE", "MAX_POOL", "ADD"] and plan.ops[-1].param == (1.0 if name == "ADD" else -1.0)
    a, b = (run(engine, blob, xs, output=t)[2] for t in (a_t, b_t))
    assert np.array_equal(bits(a), bits(xs)) and not np.array_equal(a, b)
    first, second = (a, b) if order == "ab" else (b, a)
    want = activated(first + second if name == "ADD" else first - second, act)
    check_bits("%s %s act %d c%d" % (name, order, act, c), got, want)
    assert not np.array_equal(got, activated(second - first, act))     # the operand order shows
    if act != tb.NONE:
        assert (got == 0).any() and (name != "ADD" or act != tb.RELU6 or (got == 6).any())


def test_add_into_a_concatenation_slice(engine):
    rng = np.random.default_rng(5)
    c = 6
    blob, a_t, b_t, conv_t = add_graph(rng, "SUB", "ba", tb.RELU, c, into_slice=True)
    xs = rng.uniform(-4, 4, size=(N, H, W, c)).astype(F32)
    g, plan, got = run(engine, blob, xs)
    assert sorted(kinds(plan)) == sorted(["MAX_POOL", "AFFINE", "MAX_POOL", "ADD", "CONV", "MAX_POOL"]) and not plan.copies()
    add = next(o for o in plan.ops if o.name == "SUB")
    assert (plan.tensors[add.out].c_offset, plan.tensors[add.out].c_stride) == (5, 5 + c)
    a, b = (run(engine, blob, xs, output=t)[2] for t in (a_t, b_t))
    check_bits("SUB into the slice at channel 5", got[..., 5:], activated(b - a, tb.RELU))
    vals, mag = te.evaluate(g, xs, magnitudes=True)
    assert float((np.abs(got[..., :5] - vals[conv_t]) / mag[conv_t]).max()) < CONV_REL    # the neighbour is still the convolution's


# ---- 4. AFFINE: an operator by a constant ----
AFFINE_OPS = ["MUL", "ADD", "SUB", "C_MINUS_X", "DIV"]


def constant_op(m, t, op, const):
    if op == "DIV":
        return m.div(t, const)
    return m.binary("SUB" if op == "C_MINUS_X" else op, t, const, const_first=op == "C_MINUS_X")


def affine_constant(rng, per_channel, c):
    v = rng.uniform(0.6, 3.0, size=c if per_channel else 1) * rng.choice([-1.0, 1.0], size=c if per_channel else 1)
    return v.astype(F32)


@pytest.mark.parametrize("per_channel", [True, False], ids=["per_channel", "one_element"])
@pytest.mark.parametrize("op", AFFINE_OPS)
def test_affine_launch_is_two_float32_operations(engine, op, per_channel):
    """The input has a second reader, so the operator is a launch of its own: the bits of NumPy's float32 x * sc + sf with
    the planner's constants, and within 2^-22 (relative) of the float64 evaluation of the flatbuffer, which knows nothing of
    sc and sf."""
    c = 6
    rng = np.random.default_rng(AFFINE_OPS.index(op) * 2 + per_channel)
    m, x = start(c)
    p = through(m, x)
    const = affine_constant(rng, per_channel, c)
    y = constant_op(m, p, op, const)
    m.unary("RELU", p)      # the second reader
    m.outputs = [y]
    xs = rng.uniform(-2, 2, size=(N, H, W, c)).astype(F32)
    g, plan, got = run(engine, m.finish(), xs)
    assert kinds(plan) == ["MAX_POOL", "AFFINE"] and plan.ops[1].name == ("SUB" if op == "C_MINUS_X" else op)
    sc, sf = plan.ops[1].scale, plan.ops[1].shift
    assert sc.dtype == sf.dtype == F32 and sc.shape == sf.shape == (c,)
    want = (xs * sc).astype(F32) + sf
    check_bits("%s %s" % (op, "per channel" if per_channel else "one element"), got, want)
    v64 = tes.evaluate(g, xs)[y]
    rel = float((np.abs(got - v64) / np.abs(v64)).max())
    print("%s: max relative error against float64 = %.3g (bound %.3g)" % (op, rel, AFFINE_REL))
    assert float(np.abs(v64).min()) > 0 and rel <= AFFINE_REL


@pytest.mark.parametrize("per_channel", [True, False], ids=["per_channel", "one_element"])
@pytest.mark.parametrize("op", AFFINE_OPS)
def test_affine_folded_into_the_convolution(engine, op, per_channel):
    """CONV_2D -> the operator, nothing else reading the convolution: one launch, held to float64 within CONV_REL of the
    magnitude the operator makes of the convolution's (sum |x| |w| + |b|) |scale| + |shift|."""
    c, cout = 6, 24
    rng = np.random.default_rng(20 + AFFINE_OPS.index(op) * 2 + per_channel)
    m, x = start(c)
    w = rng.normal(0, np.sqrt(2.0 / (9 * c)), size=(cout, 3, 3, c)).astype(F32)
    conv = m.conv(x, w, rng.normal(0, 0.05, size=cout).astype(F32), 1, tb.SAME, tb.NONE)
    const = affine_constant(rng, per_channel, cout)
    y = constant_op(m, conv, op, const)
    m.outputs = [y]
    xs = rng.uniform(-1, 1, size=(N, H, W, c)).astype(F32)
    g, plan, got = run(engine, m.finish(), xs)
    assert kinds(plan) == ["CONV"] and plan.ops[0].name == "CONV_2D+" + ("SUB" if op == "C_MINUS_X" else op)
    v64 = tes.evaluate(g, xs)[y]
    mag = te.evaluate(FirstOperatorOnly(g), xs, magnitudes=True)[1][conv]
    k = np.abs(const.astype(np.float64))
    bound = mag * k if op == "MUL" else mag / k if op == "DIV" else mag + k
    rel = float((np.abs(got - v64) / bound).max())
    print("%s folded: max |error| / magnitude = %.3g (bound %.3g)" % (op, rel, CONV_REL))
    assert got.shape == v64.shape and rel < CONV_REL


class FirstOperatorOnly:
    """The graph cut off behind its first operator, for tflite_eval.evaluate (which does not know DIV)."""

    def __init__(self, g):
        self.g, self.inputs, self.ops, self.tensors = g, g.inputs, g.ops[:1], g.tensors

    def const(self, t):
        return self.g.const(t)


# ---- 5. LOGISTIC as a launch ----
SPECIAL = np.array([88.0, -88.0, 104.0, -104.0, 0.0, -0.0, 1e-40, -1e-40], F32)


def test_logistic_launch(engine):
    """Behind a launch with two readers nothing folds.  expf(104) overflows float32: the answer there is exactly 0 or 1."""
    rng = np.random.default_rng(31)
    c = 8
    m, x = start(c)
    p = through(m, x)
    s = m.unary("LOGISTIC", p)
    m.unary("RELU", p)      # the second reader
    m.outputs = [s]
    xs = rng.uniform(-12, 12, size=(N, H, W, c)).astype(F32)
    xs[0, 0, 0], xs[2, H - 1, W - 1] = SPECIAL, SPECIAL[::-1]
    g, plan, got = run(engine, m.finish(), xs)
    assert kinds(plan) == ["MAX_POOL", "LOGISTIC"]
    v64, yard, tol = yardstick(g, xs, s)
    err = float(np.abs(got - v64).max())
    print("logistic: float32-CPU vs float64 %.3g, device vs float64 %.3g (tolerance %.3g)" % (yard, err, tol))
    assert np.all(np.isfinite(got)) and err <= tol
    assert np.all(got[xs == 104] == 1.0) and np.all(got[xs == -104] == 0.0) and np.all(got[xs == 88] == 1.0)
    assert float(got[xs == -88].max()) < 1e-38 and np.all(got[xs == 0] == 0.5) and np.all(got[np.abs(xs) == F32(1e-40)] == 0.5)
    assert float(got.min()) >= 0 and float(got.max()) <= 1


def test_logistic_behind_a_convolution_with_two_readers(engine):
    """A LOGISTIC folds into the CONV_2D in front of it only where nothing else reads that convolution; here a RELU does.
    Against float64 on the convolution's values as the device wrote them."""
    rng = np.random.default_rng(32)
    c, cout = 6, 24
    m, x = start(c)
    conv = m.conv(x, rng.normal(0, 2.0, size=(cout, 1, 1, c)).astype(F32), rng.normal(size=cout).astype(F32), 1, tb.SAME, tb.NONE)
    s = m.unary("LOGISTIC", conv)
    m.unary("RELU", conv)
    m.outputs = [s]
    blob = m.finish()
    xs = rng.uniform(-2, 2, size=(N, H, W, c)).astype(F32)
    g, plan, got = run(engine, blob, xs)
    assert kinds(plan) == ["CONV", "LOGISTIC"]
    z = run(engine, blob, xs, output=conv)[2]
    import torch

    want = torch.sigmoid(torch.from_numpy(z.astype(np.float64))).numpy()
    yard = float(np.abs(torch.sigmoid(torch.from_numpy(z)).numpy() - want).max())
    tol = max(LOGIT_MULTIPLE * yard, FLOOR)
    err = float(np.abs(got - want).max())
    print("logistic behind a convolution: float32-CPU vs float64 %.3g, device vs float64 %.3g (tolerance %.3g)" % (yard, err, tol))
    assert err <= tol and float(np.ptp(got)) > 0.9


# ---- 6. the copies of a CONCATENATION ----
def concat_graph(what):
    """-> (model, the names of the plan's launches, NumPy's answer on x).  The concatenated tensor cannot be the graph's
    output (its parts would be views of it): a 1 x 1 MAX_POOL_2D hands it on, bit for bit."""
    relu = lambda v: np.maximum(v, F32(0))
    if what == "same_tensor_twice":
        m, x = start(6)
        p = through(m, x)
        m.outputs = [through(m, m.concat([p, p]))]
        return m, ["MAX_POOL_2D", "COPY", "MAX_POOL_2D"], lambda v: np.concatenate([v, v], axis=-1)
    if what == "graph_input_as_a_part":
        m, x = start(6)
        m.outputs = [through(m, m.concat([x, m.unary("RELU", x)]))]
        return m, ["RELU", "COPY", "MAX_POOL_2D"], lambda v: np.concatenate([v, relu(v)], axis=-1)
    if what == "reshape_alias_as_a_part":
        m, x = start(8)
        v = m.reshape(through(m, x), [1, H, W, 8])
        m.outputs = [through(m, m.concat([m.unary("RELU", x), v]))]
        return m, ["MAX_POOL_2D", "RELU", "COPY", "MAX_POOL_2D"], lambda v: np.concatenate([relu(v), v], axis=-1)
    assert what == "fused_relu6"
    m, x = start(6)
    two = np.full(6, 2.0, F32)
    m.outputs = [through(m, m.concat([through(m, x), m.binary("MUL", x, two)], act=tb.RELU6))]
    return m, ["MAX_POOL_2D", "MUL", "CONCATENATION_ACT", "MAX_POOL_2D"], lambda v: np.clip(np.concatenate([v, v * two], axis=-1), F32(0), F32(6))


@pytest.mark.parametrize("what", ["same_tensor_twice", "graph_input_as_a_part", "reshape_alias_as_a_part", "fused_relu6"])
def test_concatenation_copies(engine, what):
    """The parts a producer cannot write in place are copied by an AFFINE launch without constants, and a fused activation
    is one more pass over the whole tensor: the bits of np.concatenate (then the clamp)."""
    m, names, want_fn = concat_graph(what)
    c = m.shape(m.inputs[0])[3]
    xs = np.random.default_rng(len(what)).uniform(-3, 5, size=(N, H, W, c)).astype(F32)
    g, plan, got = run(engine, m.finish(), xs)
    assert [o.name for o in plan.ops] == names, [o.name for o in plan.ops]
    assert len(plan.copies()) == names.count("COPY")
    want = want_fn(xs)
    check_bits(what, got, want)
    if what == "fused_relu6":
        assert (got == 0).any() and (got == 6).any()
