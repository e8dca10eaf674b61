"""Grouped CONV_2D in the TFLite graph executor, host side (no GPU): the plan of the WR-ResNet-22-4's own flatbuffer, float32
and dynamic-range quantised (what the reference's converter writes, src/tfliteconverter.py:54-62), the grouped packers,
the NumPy restatement of CONV_Q8_GROUPED (tests/tflite_eval_grouped.py) against the references the suite trusts, the
conversion with the filters multiplied out, the routing of get_interpreter, the refusals and the tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tflite_build as tb
import tflite_build_q8 as tq
import tflite_eval as te
import tflite_eval_grouped as tgr
import tflite_eval_q8 as tq8

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS17 = ["l%d" % i for i in range(17)]


@pytest.fixture(scope="module")
def wr_weights():
    from cpx.ml_tools import wrresnet as wr

    return wr.random_weights(17, seed=5)


@pytest.fixture(scope="module")
def wr_blob(wr_weights):
    return tb.wrresnet(wr_weights)


@pytest.fixture(scope="module")
def wr_blob_q8(wr_blob):
    return tq.quantise(wr_blob)


def convs(plan):
    return [o for o in plan.ops if o.name.startswith("CONV_2D")]


# ---- the WR-ResNet plans ----
def test_wrresnet_float32_plan(wr_blob):
    from cpx import _lib
    from cpx.ml_tools.tflite_graph import build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(wr_blob)
    plan = build_plan(g, grouped_convolutions=True)
    cs = convs(plan)
    assert len(cs) == 22 and all(o.kind == _lib.GRAPH_CONV_GROUPED and o.groups == 2 for o in cs)
    assert {o.stride_h for o in cs} == {1, 2, 3} and all(o.stride_h == o.stride_w for o in cs)
    assert plan.input_shape == (160, 160, 2) and plan.output_shape == (1, 1, 17)
    # the pre-activations stay AFFINE launches, also where LiteInterpreter asks for the fold (there is no grouped CONV_PRE)
    folded = build_plan(g, grouped_convolutions=True, fuse_preactivation=True, fold_windows=True)
    assert [o.name for o in folded.ops] == [o.name for o in plan.ops]
    assert sum(o.kind == _lib.GRAPH_AFFINE for o in plan.ops) == 10 and not any(o.kind == _lib.GRAPH_CONV_PRE for o in folded.ops)
    # fp16x2 leaves grouped convolutions on the float32 kernel
    h2 = build_plan(g, grouped_convolutions=True, conv_math="fp16x2")
    assert [o.kind for o in h2.ops] == [o.kind for o in plan.ops]
    # the weights are G images of the ungrouped packer
    o = cs[3]
    assert o.weights.dtype == np.float32 and o.weights.size == 2 * o.kh * o.kw * 16 * 32 * (-(-o.filter.shape[3] // 16)) * (-(-o.filter.shape[0] // 2 // 32))
    for call in (lambda: build_plan(g), lambda: g.check_executable()):
        with pytest.raises(NotImplementedError, match="grouped"):
            call()


def test_wrresnet_quantised_plan(wr_blob_q8):
    from cpx import _lib
    from cpx.ml_tools.tflite_graph import Q8_KINDS, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(wr_blob_q8)
    plan = build_plan(g, grouped_convolutions=True)
    kinds = [o.kind for o in plan.ops]
    assert kinds.count(_lib.GRAPH_CONV_Q8_GROUPED) == 20 and kinds.count(_lib.GRAPH_CONV_GROUPED) == 2
    assert kinds.count(_lib.GRAPH_FC_Q8) == 1 and _lib.GRAPH_CONV_Q8_GROUPED in Q8_KINDS
    f32 = sorted(int(o.filter.size) for o in plan.ops if o.kind == _lib.GRAPH_CONV_GROUPED)
    assert f32 == [144, 512]   # conv1_1 and shortcut2, under the converter's 1024-element threshold
    # one QUANT_PARAMS per input view, shared by its readers: the stage's first block feeds shortcut and conv a from
    # different tensors, every hybrid operator's in1 is the parameter tensor of its own in0
    for o in plan.ops:
        if o.kind in Q8_KINDS:
            q = next(p for p in plan.ops if p.out == o.in1)
            assert q.kind == _lib.GRAPH_QUANT_PARAMS and q.in0 == o.in0 and plan.ops.index(q) < plan.ops.index(o)
    params = [o for o in plan.ops if o.kind == _lib.GRAPH_QUANT_PARAMS]
    assert len(params) == len(set((o.in0, o.param) for o in params))
    assert all(o.scale is not None and o.shift is not None and o.scale.shape == o.shift.shape == (o.filter.shape[0],)
               for o in plan.ops if o.kind == _lib.GRAPH_CONV_Q8_GROUPED)
    fplan = build_plan(g, grouped_convolutions=True, quantised_math="float")
    fk = [o.kind for o in fplan.ops]
    assert fk.count(_lib.GRAPH_CONV_GROUPED) == 22 and not any(k in Q8_KINDS + (_lib.GRAPH_QUANT_PARAMS,) for k in fk)
    assert [o.name for o in fplan.ops] == [o.name for o in plan.ops if o.kind != _lib.GRAPH_QUANT_PARAMS]
    with pytest.raises(NotImplementedError, match="grouped"):
        build_plan(g)


def test_constants_fold_into_a_grouped_convolution():
    """CONV's epilogue: MUL / ADD by constants and a swish behind a grouped convolution fold into it, float32 and hybrid."""
    from cpx import _lib
    from cpx.ml_tools.tflite_graph import ACT_SWISH, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(2)
    m = tb.Model()
    x = m.tensor([1, 9, 9, 64], name="input")
    m.inputs = [x]
    y = m.conv(x, rng.normal(0, 0.1, size=(32, 3, 3, 32)).astype(np.float32), np.zeros(32, np.float32), 1, tb.SAME, tb.NONE)
    sc, sh = rng.uniform(0.5, 2, size=32).astype(np.float32), rng.normal(0, 1, size=32).astype(np.float32)
    y = m.binary("ADD", m.binary("MUL", y, sc), sh)
    m.outputs = [m.binary("MUL", y, m.unary("LOGISTIC", y))]
    for blob, kind in ((m.finish(), _lib.GRAPH_CONV_GROUPED), (tq.quantise(m.finish()), _lib.GRAPH_CONV_Q8_GROUPED)):
        plan = build_plan(Graph(blob), grouped_convolutions=True)
        o = plan.ops[-1]
        assert [p.kind for p in plan.ops if p.kind != _lib.GRAPH_QUANT_PARAMS] == [kind]
        assert o.name == "CONV_2D+MUL+ADD+SWISH" and o.act == ACT_SWISH and o.groups == 2
        fs = 1.0 if o.filter_scale is None else o.filter_scale
        assert np.array_equal(o.scale, (fs * sc).astype(np.float32)) and np.array_equal(o.shift, sh)


# ---- the packers ----
@pytest.mark.parametrize("G,cg,cog", [(2, 1, 8), (2, 6, 40), (3, 8, 10), (2, 64, 128)])
def test_grouped_packers_round_trip(G, cg, cog):
    from cpx.ml_tools import tflite_graph as tg

    rng = np.random.default_rng(G * 1000 + cg * 10 + cog)
    shape = (G * cog, 3, 2, cg)
    w = rng.normal(size=shape).astype(np.float32)
    packed = tg.pack_conv_filter_grouped(w, G)
    assert packed.dtype == np.float32 and packed.ndim == 1
    one = packed.size // G
    for k in range(G):
        assert packed[k * one:(k + 1) * one].tobytes() == tg.pack_conv_filter(w[k * cog:(k + 1) * cog]).tobytes()
    assert np.array_equal(tg.unpack_conv_filter_grouped(packed, shape, G), w)

    q = rng.integers(-127, 128, size=shape).astype(np.int8)
    pq = tg.pack_conv_filter_q8_grouped(q, G)
    nws = 4 * (-(-cog // 32) * 32)
    img = (pq.size - G * nws) // G
    for k in range(G):
        ref = tg.pack_conv_filter_q8(q[k * cog:(k + 1) * cog])
        assert pq[k * img:(k + 1) * img].tobytes() == ref[:-nws].tobytes()
        assert pq[G * img + k * nws:G * img + (k + 1) * nws].tobytes() == ref[-nws:].tobytes()
    back, wsum = tg.unpack_conv_filter_q8_grouped(pq, shape, G)
    assert np.array_equal(back, q)
    # wsum sums each group's OWN rows only (the rows hold one group's input channels: there is nothing else to sum)
    assert np.array_equal(wsum, q.reshape(G * cog, -1).astype(np.int64).sum(axis=1))
    assert img % 16 == 0 and one % 4 == 0   # every image starts on a 16-byte boundary
    with pytest.raises(ValueError):
        tg.pack_conv_filter_grouped(w, G + 5)


# ---- the helper against the references the suite trusts ----
def one_grouped_conv(rng, kh, kw, stride, padding, cin, G, cout, hw, act=tb.NONE, quantised=False):
    m = tb.Model()
    x = m.tensor([1, hw[0], hw[1], cin], name="input")
    m.inputs = [x]
    w = rng.normal(0, np.sqrt(2.0 / (kh * kw * (cin // G))), size=(cout, kh, kw, cin // G)).astype(np.float32)
    m.outputs = [m.conv(x, w, rng.normal(0, 0.05, size=cout).astype(np.float32), stride, padding, act)]
    return tq.quantise(m.finish(), min_elements=0) if quantised else m.finish()


def test_the_helper_with_one_group_is_the_q8_helper():
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(4)
    g = Graph(one_grouped_conv(rng, 3, 3, 2, tb.SAME, 24, 1, 40, (9, 7), act=tb.RELU, quantised=True))
    x = rng.uniform(-2, 3, size=(3, 9, 7, 24)).astype(np.float32)
    op = g.ops[0]
    ten, bias = g.quantised_filter(op), g.const(op["inputs"][2])
    v0, m0 = tq8.hybrid_conv(op, x, ten, bias)
    v1, m1 = tgr.hybrid_conv_grouped(op, x, ten, bias)
    assert v0.tobytes() == v1.tobytes() and m0.tobytes() == m1.tobytes()
    a, b = tq8.evaluate_hybrid(g, x), tgr.evaluate_hybrid(g, x)
    assert a[0][g.outputs[0]].tobytes() == b[0][g.outputs[0]].tobytes()


def test_the_helpers_float_path_is_the_float_evaluator(wr_blob):
    """evaluate_hybrid on a graph without INT8 filters runs tflite_eval operator by operator in float32."""
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(6)
    g = Graph(one_grouped_conv(rng, 3, 3, (2, 3), tb.SAME, 24, 3, 30, (13, 7)))
    x = rng.uniform(-1, 1, size=(2, 13, 7, 24)).astype(np.float32)
    got = tgr.evaluate_hybrid(g, x)[0][g.outputs[0]]
    want = te.evaluate(g, x, dtype=torch.float32)[g.outputs[0]]
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    want64, mag = te.evaluate(g, x, magnitudes=True)
    assert float((np.abs(got - want64[g.outputs[0]]) / mag[g.outputs[0]]).max()) < 4e-6


def test_the_helper_quantises_the_whole_tensor_once():
    """Groups of very different ranges: parameters per group give another result, the whole-tensor ones are coarser for
    the small group."""
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(9)
    g = Graph(one_grouped_conv(rng, 3, 3, 1, tb.SAME, 16, 2, 64, (9, 9), quantised=True))
    x = np.concatenate([rng.uniform(-1, 1, size=(2, 9, 9, 8)), rng.uniform(0, 50, size=(2, 9, 9, 8))], axis=3).astype(np.float32)
    whole, mag = tgr.evaluate_hybrid(g, x)
    per, _ = tgr.evaluate_hybrid(g, x, per_group=True)
    t = g.outputs[0]
    assert float((np.abs(whole[t].astype(np.float64) - per[t]) / mag[t]).max()) > 1e-3
    deq = tq8.evaluate_dequantised(g, x)[t]
    # the quantisation noise of group 0's outputs is what the coarse parameters make it
    assert np.abs(whole[t][..., :32] - deq[..., :32]).max() > 5 * np.abs(per[t][..., :32] - deq[..., :32]).max()


# ---- conversion ----
def test_convert_multiplies_the_filters_out(wr_weights, wr_blob, wr_blob_q8):
    from cpx.ml_tools.tflite_reader import Graph, convert

    g, gq = Graph(wr_blob), Graph(wr_blob_q8)
    with pytest.raises(NotImplementedError, match="INT8 filter") as e:
        convert(gq)
    first = next(gq.quantised_filter(op) for op in gq.ops if gq.quantised_filter(op) is not None)
    assert repr(first["name"]) in str(e.value) and "quantised_math" in str(e.value) and "LiteInterpreter" in str(e.value)
    with pytest.raises(ValueError):
        convert(gq, quantised_math="hybrid")
    w, wq = convert(g), convert(gq, quantised_math="float")
    assert sorted(w) == sorted(wq)
    # the converter's layout (the shortcut reads the block's raw input, the ReLU behind the residual ADD fused into it)
    # walks back to the weights it was written from
    for k in ("conv1_1/kernel", "res2b0_branch2b/kernel", "shortcut4/kernel", "res4b2_branch2b/bias", "prediction/kernel"):
        assert np.array_equal(w[k], wr_weights[k]), k
    n_q = 0
    for op in gq.ops:
        ten = gq.quantised_filter(op)
        if ten is None or op["name"] != "CONV_2D":
            continue
        want = ten["const"].astype(np.float32) * np.asarray(ten["quant"]["scale"], np.float32).reshape(-1, 1, 1, 1)   # OHWI
        hits = [k for k, v in wq.items() if k.endswith("/kernel") and v.ndim == 4 and v.shape == want.transpose(1, 2, 3, 0).shape
                and np.array_equal(v, want.transpose(1, 2, 3, 0))]
        assert len(hits) == 1, ten["name"]
        n_q += 1
    assert n_q == 20
    for k in w:
        if isinstance(w[k], np.ndarray):
            if k in ("conv1_1/kernel", "shortcut2/kernel") or not k.endswith("/kernel"):
                assert np.array_equal(w[k], wq[k]), k
            else:
                assert not np.array_equal(w[k], wq[k]) and np.abs(w[k] - wq[k]).max() <= np.abs(w[k]).max() / 127 * 0.51, k
    fc = gq.quantised_filter(gq.ops[-2])
    assert np.array_equal(wq["prediction/kernel"], (fc["const"].astype(np.float32) * np.float32(fc["quant"]["scale"][0])).T)


# ---- routing ----
def write_wr(d, name, blob):
    (d / (name + ".tflite")).write_bytes(blob)
    with open(d / (name + ".json"), "w") as fh:
        json.dump({"labels": LABELS17, "type": "thermal", "hyperparams": {"frame_size": 32, "model_name": "wr-resnet"}}, fh)


def test_get_interpreter_routes_the_wrresnet_files(tmp_path, monkeypatch, wr_blob, wr_blob_q8):
    from cpx import _lib
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, WRResNetInterpreter, get_interpreter

    write_wr(tmp_path, "wrf", wr_blob)
    write_wr(tmp_path, "wrq", wr_blob_q8)
    cf = ModelConfig.load({"id": 1, "name": "wrf", "model_file": str(tmp_path / "wrf.tflite")})
    cq = ModelConfig.load({"id": 2, "name": "wrq", "model_file": str(tmp_path / "wrq.tflite")})
    monkeypatch.delenv("CPX_TFLITE_QUANT_MATH", raising=False)
    a = get_interpreter(cf)
    assert isinstance(a, WRResNetInterpreter) and a._weights["conv1_1/kernel"].shape == (3, 3, 1, 16)
    b = get_interpreter(cq)
    assert isinstance(b, LiteInterpreter) and b.labels == LABELS17
    plan = next(iter(b._plans.values()))
    assert sum(o.kind == _lib.GRAPH_CONV_Q8_GROUPED for o in plan.ops) == 20
    assert b.channel_map() == [0, 1] and not b.limits_flags() & _lib.LIMITS_TF_SCALING
    # the crop kernel's two-channel sample is the graph's own input: no channel map in front
    key, p2 = b._plan((160, 160, 2))
    assert p2 is plan and key[1] is None
    monkeypatch.setenv("CPX_TFLITE_QUANT_MATH", "float")
    c = get_interpreter(cq)
    assert isinstance(c, WRResNetInterpreter)
    q = a._weights["res2b0_branch2a/kernel"], c._weights["res2b0_branch2a/kernel"]
    assert q[0].shape == q[1].shape and not np.array_equal(*q) and np.abs(q[0] - q[1]).max() < np.abs(q[0]).max() / 127
    assert isinstance(get_interpreter(cf), WRResNetInterpreter)
    monkeypatch.setenv("CPX_TFLITE_QUANT_MATH", "nonsense")
    with pytest.raises(ValueError, match="CPX_TFLITE_QUANT_MATH"):
        get_interpreter(cq)
    monkeypatch.delenv("CPX_TFLITE_QUANT_MATH")
    # a LiteInterpreter constructed on the float32 file plans it: the independent float32 device implementation
    d = LiteInterpreter(tmp_path / "wrf.tflite")
    fplan = next(iter(d._plans.values()))
    assert sum(o.kind == _lib.GRAPH_CONV_GROUPED for o in fplan.ops) == 22
    # not loading stays not loading
    assert isinstance(get_interpreter(cq, load_model=False), LiteInterpreter)


# ---- refusals ----
def refusal(model, **kw):
    from cpx.ml_tools.tflite_graph import build_plan
    from cpx.ml_tools.tflite_reader import Graph

    with pytest.raises(NotImplementedError) as e:
        build_plan(Graph(model.finish()), grouped_convolutions=True, **kw)
    return str(e.value)


def test_what_is_still_refused_names_the_operator():
    def start(c=8):
        m = tb.Model()
        x = m.tensor([1, 12, 12, c], name="input")
        m.inputs = [x]
        return m, m.conv(x, np.ones((c, 3, 3, c), np.float32), np.zeros(c, np.float32), 1, tb.SAME, tb.RELU)

    m, y = start()
    m.outputs = [m.conv(y, np.ones((4, 3, 3, 3), np.float32), np.zeros(4, np.float32), 1, tb.SAME)]   # 3 does not divide 8
    msg = refusal(m)
    assert "CONV_2D" in msg and "operator 1" in msg and "does not divide the input depth" in msg
    m, y = start()
    m.outputs = [m.conv(y, np.ones((6, 3, 3, 2), np.float32), np.zeros(6, np.float32), 1, tb.SAME)]   # G = 4, Cout = 6
    msg = refusal(m)
    assert "CONV_2D" in msg and "operator 1" in msg and "4 groups" in msg and "output channels" in msg
    m, y = start()
    m.outputs = [m.conv(y, np.ones((4, 3, 3, 4), np.float32), np.zeros(4, np.float32), 1, tb.SAME, dilation=2)]
    msg = refusal(m)
    assert "CONV_2D" in msg and "operator 1" in msg and "dilation" in msg
    m, y = start()
    m.outputs = [m.conv(y, np.ones((1, 3, 3, 16), np.float32), np.zeros(16, np.float32), 1, tb.SAME, name="DEPTHWISE_CONV_2D")]
    msg = refusal(m)
    assert "DEPTHWISE_CONV_2D" in msg and "operator 1" in msg and "depth multiplier" in msg
    for stride in (4, (1, 4)):
        m, y = start()
        m.outputs = [m.conv(y, np.ones((4, 3, 3, 4), np.float32), np.zeros(4, np.float32), stride, tb.SAME)]
        msg = refusal(m)
        assert "CONV_2D" in msg and "operator 1" in msg and "strides" in msg
    # an ungrouped convolution keeps its own limit of 2 whatever the flag says
    m, y = start()
    m.outputs = [m.conv(y, np.ones((4, 3, 3, 8), np.float32), np.zeros(4, np.float32), 3, tb.SAME)]
    msg = refusal(m)
    assert "operator 1" in msg and "strides 3, 3" in msg


def test_the_overflow_check_counts_one_groups_channels():
    """7 x 7 x 1353 products fit the int32 accumulator, 7 x 7 x 1354 do not (test_tflite_q8_cpu.py): a grouped filter is
    refused by the channels of ONE group, not by the tensor's."""
    from cpx.ml_tools.tflite_graph import build_plan
    from cpx.ml_tools.tflite_reader import Graph

    for cg, refused in ((1353, False), (1354, True)):
        m = tq.ModelQ8()
        x = m.tensor([1, 7, 7, 2 * cg], name="input")
        m.inputs = [x]
        q = np.ones((2, 7, 7, cg), np.int8)
        m.outputs = [m.conv_q8(x, m.qfilter(q, np.ones(2, np.float32)), np.zeros(2, np.float32))]
        g = Graph(m.finish())
        assert (7 * 7 * cg * 127 * 255 >= 2 ** 31) == refused and 7 * 7 * 2 * cg * 127 * 255 >= 2 ** 31
        if refused:
            with pytest.raises(NotImplementedError, match="overflow"):
                build_plan(g, grouped_convolutions=True)
        else:
            build_plan(g, grouped_convolutions=True)


# ---- the tool ----
def test_describe_names_the_groups_and_dequantise_converts(tmp_path, wr_blob_q8):
    tool = os.path.join(REPO, "tools", "tflite_to_npz.py")
    write_wr(tmp_path, "wrq", wr_blob_q8)
    r = subprocess.run([sys.executable, tool, "--describe", str(tmp_path / "wrq.tflite")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "grouped convolutions: 22 (20 hybrid)" in r.stdout and "operator 0: G = 2," in r.stdout
    assert r.stdout.count("G = 2 (hybrid)") == 20 and "hybrid operators (int8 filter, activations quantised per sample): 21" in r.stdout
    r = subprocess.run([sys.executable, tool, str(tmp_path / "wrq.tflite"), str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode != 0 and "INT8 filter" in r.stderr
    r = subprocess.run([sys.executable, tool, "--dequantise", str(tmp_path / "wrq.tflite"), str(tmp_path / "out")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    z = np.load(tmp_path / "out.npz")
    assert z["res4b2_branch2b/kernel"].shape == (3, 3, 128, 256) and (tmp_path / "out.json").exists()
