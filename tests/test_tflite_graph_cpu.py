"""The host side of the TFLite graph executor: the reader's options, the planner (cpx/ml_tools/tflite_graph.py: shapes,
concatenation by placement, arena lifetimes, refusals) and get_interpreter's routing, on synthetic flatbuffers
(tests/tflite_build.py) against a float64 evaluation of the same Graph (tests/tflite_eval.py).  No GPU."""
import json

import numpy as np
import pytest

import tflite_build as tb
import tflite_eval as te


def test_evaluator_matches_the_network_oracle():
    """The float64 evaluator against the checker the rest of the suite trusts: the WR-ResNet flatbuffer (grouped filters)
    evaluated operator by operator gives oracle/cnn_oracle.forward's logits, at that oracle's 2e-4."""
    import cnn_oracle as co
    from cpx.ml_tools import wrresnet as wr
    from cpx.ml_tools.tflite_reader import Graph

    w = wr.random_weights(17, seed=5)
    x = np.random.default_rng(3).uniform(0, 255, size=(2, 160, 160, 2)).astype(np.float32)
    w = co.calibrate_bn(w, x)
    g = Graph(tb.wrresnet(w))
    assert g.const(g.ops[4]["inputs"][1]).shape[3] * 2 == 16   # grouped: the filter's depth is half the tensor's
    vals = te.evaluate(g, x)
    want, want_p = co.forward(w, x)
    logits = vals[g.ops[-1]["inputs"][0]]
    assert float(np.abs(logits - want).max()) <= 2e-4
    assert float(np.abs(vals[g.outputs[0]] - want_p).max()) <= 1e-4


def test_reader_decodes_the_options():
    from cpx.ml_tools.tflite_reader import Graph

    m = tb.Model()
    x = m.tensor([1, 12, 12, 8], name="input")
    m.inputs = [x]
    w = np.ones((4, 3, 5, 8), np.float32)
    c = m.conv(x, w, np.zeros(4, np.float32), (2, 1), tb.VALID, tb.RELU6)
    a = m.pool("AVERAGE_POOL_2D", x, (3, 2), (2, 1), tb.SAME, tb.RELU)
    p = m.pool("MAX_POOL_2D", x, (2, 3), (1, 2), tb.VALID)
    cc = m.concat([x, x], axis=-1, act=tb.RELU)
    r6 = m.unary("RELU6", cc)
    s = m.binary("SUB", r6, np.ones(16, np.float32), tb.RELU, const_first=True)
    mk = m.mean(s, (1, 2), keep_dims=True)
    mn = m.mean(s, (2, 1), keep_dims=False)
    sm = m.softmax(mn, 0.25)
    rs = m.reshape(mk, [1, 16])
    pd = m.pad(x, [[0, 0], [1, 2], [3, 0], [0, 0]])
    m.outputs = [sm]
    g = Graph(m.finish())
    by = {o["outputs"][0]: o for o in g.ops}
    o = by[c]
    assert (o["name"], o["padding"], o["stride_h"], o["stride_w"], o["act"], o["dilation_h"], o["dilation_w"]) == \
        ("CONV_2D", 1, 2, 1, 3, 1, 1)
    o = by[a]
    assert (o["name"], o["padding"], o["stride_h"], o["stride_w"], o["filter_height"], o["filter_width"], o["act"]) == \
        ("AVERAGE_POOL_2D", 0, 2, 1, 3, 2, 1)
    o = by[p]
    assert (o["name"], o["padding"], o["stride_h"], o["stride_w"], o["filter_height"], o["filter_width"], o["act"]) == \
        ("MAX_POOL_2D", 1, 1, 2, 2, 3, 0)
    assert (by[cc]["name"], by[cc]["axis"], by[cc]["act"]) == ("CONCATENATION", -1, 1)
    assert by[r6]["name"] == "RELU6" and (by[s]["name"], by[s]["act"]) == ("SUB", 1)
    assert (by[mk]["name"], by[mk]["axes"], by[mk]["keep_dims"]) == ("MEAN", [1, 2], True)
    assert (by[mn]["axes"], by[mn]["keep_dims"]) == ([2, 1], False)
    assert by[sm]["name"] == "SOFTMAX" and by[sm]["beta"] == 0.25
    assert by[rs]["name"] == "RESHAPE" and by[rs]["new_shape"] == [1, 16]
    assert by[pd]["name"] == "PAD" and by[pd]["paddings"] == [[0, 0], [1, 2], [3, 0], [0, 0]]


@pytest.mark.parametrize("size", [160, 75])
def test_plan_shapes_placement_and_arena(size):
    from cpx.ml_tools.tflite_graph import build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(tb.inception_v3(11, (24,), seed=2, width=0.25, size=160))
    plan = build_plan(g, input_shape=(size, size, 3))
    x = np.random.default_rng(1).uniform(-1, 1, size=(1, size, size, 3)).astype(np.float32)
    vals = te.evaluate(g, x)
    # shape inference: every tensor of the plan has the shape the evaluation actually produced
    checked = 0
    for tid, t in plan.tensors.items():
        v = vals[tid]
        assert (t.H, t.W, t.C) == (tuple(v.shape[1:]) if v.ndim == 4 else (1, 1, v.shape[1])), tid
        checked += 1
    assert checked == 94 + 13 + 15 + 1 + 2 + 1 + 1   # convolutions, pools, concatenations, mean, dense, logistic, input
    # concatenation by placement: no copy operator, and no launch for a CONCATENATION at all
    census = plan.census()
    assert not plan.copies() and census == {"CONV_2D": 94, "MAX_POOL_2D": 4, "AVERAGE_POOL_2D": 9, "MEAN": 1,
                                            "FULLY_CONNECTED": 2, "LOGISTIC": 1}
    # ... the slices of one storage tile its channels exactly
    by_storage = {}
    for tid, t in plan.tensors.items():
        by_storage.setdefault(t.storage, []).append(t)
    for sid, ts in by_storage.items():
        root = plan.tensors[sid]
        leaves = sorted((t.c_offset, t.C) for t in ts if not any(u is not t and u.c_offset >= t.c_offset and
                                                                   u.c_offset + u.C <= t.c_offset + t.C and u.C < t.C for u in ts))
        assert all(t.c_stride == root.C and t.c_offset + t.C <= root.C for t in ts)
        pos = 0
        for off, c in leaves:
            assert off == pos, (sid, leaves)
            pos += c
        assert pos == root.C
    # arena lifetimes: two storages alive at the same operator never overlap
    external = {plan.input, plan.out_storage}
    spans = []
    for sid, (a, b) in plan.lifetimes.items():
        if sid in external:
            continue
        root = plan.tensors[sid]
        off = root.arena_offset
        assert off >= 0 and off + root.H * root.W * root.C <= plan.arena_floats
        spans.append((off, off + root.H * root.W * root.C, a, b))
    assert len(spans) > 50
    for i, (o0, e0, a0, b0) in enumerate(spans):
        for o1, e1, a1, b1 in spans[i + 1:]:
            if not (b0 < a1 or b1 < a0):
                assert e0 <= o1 or e1 <= o0
    # the arena is reused: far below the sum of all tensors
    assert plan.arena_floats < sum(e - o for o, e, _, _ in spans) / 4
    # every operator reads what an earlier one wrote
    written = {plan.input}
    for o in plan.ops:
        assert plan.tensors[o.in0].storage in written
        written.add(plan.tensors[o.out].storage)


def test_a_tensor_in_two_concatenations_is_copied_once():
    from cpx.ml_tools.tflite_graph import build_plan
    from cpx.ml_tools.tflite_reader import Graph

    m = tb.Model()
    x = m.tensor([1, 8, 8, 4], name="input")
    m.inputs = [x]
    a = m.unary("RELU", x)
    b = m.unary("RELU6", x)
    c1 = m.concat([a, b])
    c2 = m.concat([b, a])
    m.outputs = [m.binary("ADD", c1, c2)]
    plan = build_plan(Graph(m.finish()))
    assert len(plan.copies()) == 2


def refused(model_or_bytes):
    from cpx.ml_tools.tflite_graph import build_plan
    from cpx.ml_tools.tflite_reader import Graph

    with pytest.raises(NotImplementedError) as e:
        build_plan(Graph(model_or_bytes if isinstance(model_or_bytes, bytes) else model_or_bytes.finish()))
    return str(e.value)


def test_refusals_name_the_operator():
    w = np.ones((4, 3, 3, 8), np.float32)

    def start():
        m = tb.Model()
        x = m.tensor([1, 12, 12, 8], name="input")
        m.inputs = [x]
        return m, m.conv(x, w, np.zeros(4, np.float32), 1, tb.SAME, tb.RELU)

    m, y = start()
    m.outputs = [m.conv(y, np.ones((1, 3, 3, 4), np.float32), np.zeros(4, np.float32), 1, tb.SAME, name="DEPTHWISE_CONV_2D")]
    msg = refused(m)
    assert "DEPTHWISE_CONV_2D" in msg and "operator 1" in msg
    m, y = start()
    q = m.tensor([1, 12, 12, 4], ttype=tb.UINT8, name="quantised")
    m.op("ADD", [y, y], [q], {0: ("b", 0)})
    m.outputs = [q]
    msg = refused(m)
    assert "ADD" in msg and "operator 1" in msg and "UINT8" in msg
    m, y = start()
    m.outputs = [m.conv(y, np.ones((4, 3, 3, 4), np.float32), np.zeros(4, np.float32), 1, tb.SAME, dilation=2)]
    msg = refused(m)
    assert "CONV_2D" in msg and "operator 1" in msg and "dilation" in msg
    m, y = start()
    m.outputs = [m.unary("TANH", y)]
    msg = refused(m)
    assert "TANH" in msg and "operator 1" in msg
    m, y = start()
    z = m.tensor([1, 12, 12, 4])
    m.op("ADD", [y], [z], None, code=150)   # an operator code the reader has no name for
    m.outputs = [z]
    msg = refused(m)
    assert "OP_150" in msg and "operator 1" in msg
    m, y = start()
    m.outputs = [m.conv(y, np.ones((4, 3, 3, 2), np.float32), np.zeros(4, np.float32), 1, tb.SAME)]   # grouped
    msg = refused(m)
    assert "CONV_2D" in msg and "operator 1" in msg and "grouped" in msg


def write_model(tmp_path, channels, name="inc3", n_labels=6, model_name="inceptionv3"):
    blob = tb.inception_v3(n_labels, (16,), seed=1, width=0.25, size=160)
    (tmp_path / (name + ".tflite")).write_bytes(blob)
    labels = ["l%d" % i for i in range(n_labels)]
    with open(tmp_path / (name + ".json"), "w") as fh:
        json.dump({"labels": labels, "type": "thermal",
                   "hyperparams": {"frame_size": 32, "model_name": model_name, "channels": channels, "dense_sizes": [16]}}, fh)
    return labels


def test_get_interpreter_routes_a_tflite_graph(tmp_path):
    from cpx.config.config import ModelConfig
    from cpx.ml_tools.interpreter import LiteInterpreter, WRResNetInterpreter, get_interpreter
    from cpx import _lib

    labels = write_model(tmp_path, ["thermal", "thermal", "filtered"])
    cfg = ModelConfig.load({"id": 1, "name": "inc3", "model_file": str(tmp_path / "inc3.tflite")})
    interp = get_interpreter(cfg)
    assert isinstance(interp, LiteInterpreter) and interp.TYPE == "TFLite"
    assert interp.labels == labels and interp.shape() == (1, (1, 160, 160, 3))
    assert interp.channel_map() == [0, 0, 1]
    flags = interp.limits_flags()
    assert flags & _lib.LIMITS_TF_SCALING and not flags & _lib.LIMITS_SWAP_CHANNELS
    write_model(tmp_path, ["flow"], name="flow")
    bad = get_interpreter(ModelConfig.load({"id": 2, "name": "flow", "model_file": str(tmp_path / "flow.tflite")}))
    with pytest.raises(NotImplementedError, match="flow"):
        bad.limits_flags()
    # the other routes stay as they were
    for name in ("model.keras", "model.h5", "forest.sav"):
        with pytest.raises(NotImplementedError, match="keras_to_npz"):
            get_interpreter(ModelConfig.load({"id": 3, "name": "k", "model_file": str(tmp_path / name)}))
    with pytest.raises(NotImplementedError, match="only the wr-resnet network"):
        WRResNetInterpreter(tmp_path / "inc3.tflite")
    served = get_interpreter(cfg, run_over_network=True)
    assert isinstance(served, WRResNetInterpreter) and served.run_over_network
    # a label count that does not match the graph's output is an error at load
    write_model(tmp_path, ["thermal", "thermal", "filtered"], name="short")
    with open(tmp_path / "short.json") as fh:
        meta = json.load(fh)
    meta["labels"] = meta["labels"][:-1]
    with open(tmp_path / "short.json", "w") as fh:
        json.dump(meta, fh)
    with pytest.raises(ValueError, match="labels"):
        get_interpreter(ModelConfig.load({"id": 4, "name": "short", "model_file": str(tmp_path / "short.tflite")}))


def test_describe_prints_census_and_refusal(tmp_path):
    import os
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    write_model(tmp_path, ["thermal", "thermal", "filtered"])
    tool = os.path.join(repo, "tools", "tflite_to_npz.py")
    r = subprocess.run([sys.executable, tool, "--describe", str(tmp_path / "inc3.tflite")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "CONV_2D: 94" in r.stdout and "arena bytes per sample" in r.stdout and "[160, 160, 3]" in r.stdout
    m = tb.Model()
    x = m.tensor([1, 8, 8, 4], name="input")
    m.inputs = [x]
    m.outputs = [m.unary("TANH", x)]
    (tmp_path / "bad.tflite").write_bytes(m.finish())
    r = subprocess.run([sys.executable, tool, "--describe", str(tmp_path / "bad.tflite")], capture_output=True, text=True)
    assert r.returncode != 0 and "TANH" in (r.stdout + r.stderr)
