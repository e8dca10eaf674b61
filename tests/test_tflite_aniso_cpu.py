"""The anisotropic cases of tests/tflite_aniso_cases.py without a device: (1) the planner's shapes and pads on every case
against the evaluator's shapes and tflite_eval._pads; (2) the table's own conditions; (3) the references can tell H from W:
the same operator with its H and W parameters exchanged gives another shape, or values that differ by more than 1000
tolerances -- shown on the references alone, no wrong plan is ever run; (4) the divisions the planner refuses."""
import numpy as np
import pytest

import tflite_aniso_cases as ac
import tflite_build_se as ts
import tflite_eval as te

CONV_REL = 4e-6      # tests/test_tflite_graph_gpu.py's bound for the float32 window operators
AVG_ABS = 2e-6       # ... and for AVERAGE_POOL_2D
WINDOW_KINDS = ("CONV", "CONV_PRE", "CONV_Q8", "DWCONV", "DWCONV_PRE", "DWCONV_Q8", "MAX_POOL", "AVG_POOL")


def graph_of(blob):
    from cpx.ml_tools.tflite_reader import Graph

    return Graph(blob)


def emulate_slice(o, x, ho, wo):
    """include/cpx.h, CPX_GRAPH_SLICE, from the planned numbers: out[y, x] = in[y * stride_h - pad_top, x * stride_w - pad_left],
    0 outside the input."""
    out = np.zeros((x.shape[0], ho, wo, x.shape[3]), x.dtype)
    for y in range(ho):
        for xx in range(wo):
            iy, ix = y * o.stride_h - o.pads[0], xx * o.stride_w - o.pads[1]
            if 0 <= iy < x.shape[1] and 0 <= ix < x.shape[2]:
                out[:, y, xx] = x[:, iy, ix]
    return out


# ---- 1. planner geometry ----
@pytest.mark.parametrize("folded", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("name", ac.NAMES)
def test_planner_geometry(name, folded):
    c = ac.BY_NAME[name]
    blob, info = ac.build(c)
    x = ac.inputs(c)
    assert x.shape == (ac.N, c["H"], c["W"], c["c"])
    g, plan = ac.plan_of(c, blob, folded)
    vals, _ = ac.reference(c, g, x)
    got = ac.kinds(plan)
    if folded:
        assert got == ac.plan_kinds(c), got
    elif c["op"] in ac.UNFOLDED_KINDS:
        assert got == ac.UNFOLDED_KINDS[c["op"]], got
    # shapes: every tensor of the plan that the flatbuffer knows, and the output
    for tid, t in plan.tensors.items():
        if isinstance(tid, (int, np.integer)) and tid in vals:
            assert (t.H, t.W, t.C) == vals[tid].shape[1:], (tid, (t.H, t.W, t.C), vals[tid].shape)
    assert plan.output_shape == vals[g.outputs[0]].shape[1:]
    by_output = {op["outputs"][0]: op for op in g.ops}
    for o, kind in zip(plan.ops, got):
        if kind in WINDOW_KINDS:
            op = g.ops[o.source]
            src = op["inputs"][0]
            if "pool" in op["name"].lower():
                kh, kw = op["filter_height"], op["filter_width"]
            else:
                kh, kw = g.tensors[op["inputs"][1]]["shape"][1:3]
            assert (o.kh, o.kw, o.stride_h, o.stride_w) == (kh, kw, op["stride_h"], op["stride_w"])
            H, W = vals[src].shape[1:3]
            pt, pb = te._pads(H, kh, op["stride_h"], op["padding"])
            pl, pr = te._pads(W, kw, op["stride_w"], op["padding"])
            if o.name.startswith("PAD>"):     # the launch took the PAD in front of it: VALID, and the PAD's four
                pd = by_output[src]["paddings"]
                assert (pt, pl, pb, pr) == (0, 0, 0, 0) and by_output[src]["name"] == "PAD"
                pt, pl, pb, pr = pd[1][0], pd[2][0], pd[1][1], pd[2][1]
                assert o.in0 == by_output[src]["inputs"][0]
            assert o.pads == (pt, pl, pb, pr), (o.name, o.pads, (pt, pl, pb, pr))
        elif kind == "PAD":
            pd = g.ops[o.source]["paddings"]
            assert o.pads == (pd[1][0], pd[2][0], pd[1][1], pd[2][1])
        elif kind == "SLICE":
            y = plan.tensors[o.out]
            assert np.array_equal(emulate_slice(o, vals[o.in0], y.H, y.W), vals[o.out]), (o.name, o.pads, o.stride_h, o.stride_w)
    # the case's own operator carries the case's numbers
    if c["op"] != "slice":
        main = plan.ops[0] if c["op"] == "pad" else plan.ops[-1]
        if folded or c["pad"] is None or c["op"] == "pad":
            assert main.pads == ac.pads_of(c), (main.pads, ac.pads_of(c))
        if c["op"] != "pad":
            assert (main.stride_h, main.stride_w) == c["s"] and (main.kh, main.kw) == c["k"]
            assert plan.output_shape[:2] == ac.window_shape(c)
    elif folded and not c["kw"].get("c_total"):
        assert len(plan.ops) == 1      # the whole chain is ONE launch


def test_the_stated_planner_examples():
    assert ac.pads_of(ac.BY_NAME["conv_3x3_s21_same_10x7"]) == (0, 1, 1, 1)
    assert ac.pads_of(ac.BY_NAME["conv_5x3_s22_same_10x7"]) == (1, 1, 2, 1)
    for name in ("pad_conv_3x5_valid_7x9", "pad_dw_3x5_s12_valid_7x9", "pad_dw_q8_3x5_s12_valid_7x9"):
        c = ac.BY_NAME[name]
        _, plan = ac.plan_of(c, ac.build(c)[0])
        assert plan.ops[-1].pads == ac.FOLDED_PADS == ac.pads_of(c) and len(plan.ops) == len(ac.plan_kinds(c))
    c = ac.BY_NAME["slice_pad_crop_pool_one_launch"]
    _, plan = ac.plan_of(c, ac.build(c)[0])
    assert [o.name for o in plan.ops] == ["PAD>STRIDED_SLICE>AVERAGE_POOL_2D"] and plan.ops[0].param == 1.0
    assert plan.ops[0].pads[:2] == (-1, 2) and (plan.ops[0].stride_h, plan.ops[0].stride_w) == (2, 1)


# ---- 2. the table ----
def test_the_table_meets_its_own_conditions():
    base = [c for c in ac.CASES if c["twin_of"] is None]
    twins = {c["twin_of"]: c for c in ac.CASES if c["twin_of"] is not None}
    assert len(base) == len(twins) == len(ac.CASES) // 2
    for c in ac.CASES:
        assert c["H"] != c["W"] and max(c["H"], c["W"]) <= ac.MAX_MAP and max(c["c"], c["cout"], c["kw"].get("c_total", 0)) <= ac.MAX_CHANNELS
        assert ac.inputs(c).shape[0] == ac.N == 3
        assert ac.asymmetries(c), c["name"]
        assert c["row"] in ac.ROWS and c["op"] in ac.PLAN_KINDS
    for c in base:
        t = twins[c["name"]]
        assert (t["H"], t["W"], t["k"], t["s"]) == (c["W"], c["H"], c["k"][::-1], c["s"][::-1]) and t["op"] == c["op"] and t["row"] == c["row"]
        if c["op"] != "slice":
            p, q = ac.pads_of(c), ac.pads_of(t)
            assert q == (p[1], p[0], p[3], p[2]), (c["name"], p, q)    # SAME's own arithmetic transposes with the map
            assert ac.window_shape(t) == ac.window_shape(c)[::-1]
    # every row and every plan kind, in both orientations
    for row in ac.ROWS:
        assert any(c["row"] == row for c in base) and any(c["row"] == row for c in twins.values()), row
    for op in ac.PLAN_KINDS:
        assert any(c["op"] == op for c in base) and any(c["op"] == op for c in twins.values()), op
    # CONV_2D: the four windows, both load widths and both column-tile counts
    conv = [c for c in base if c["op"] == "conv"]
    assert {(c["k"], c["s"], c["padding"], c["H"], c["W"]) for c in conv} == {
        ((3, 3), (2, 1), ac.SAME, 10, 7), ((5, 3), (2, 2), ac.SAME, 10, 7), ((3, 2), (1, 2), ac.VALID, 6, 9), ((1, 1), (2, 1), ac.VALID, 9, 6)}
    assert {c["c"] for c in conv} == {5, 8} and {c["cout"] for c in conv} == {24, 40}
    assert {(c["s"], c["padding"]) for c in base if c["op"] == "conv_q8"} == {((2, 1), ac.SAME), ((1, 2), ac.VALID)}
    # DEPTHWISE: all eight instantiations, every case with stride_h != stride_w, and each case's twin launches the
    # instantiation of the other stride_w
    dw = [c for c in ac.CASES if c["op"] == "dw"]
    assert {ac.dw_instantiation(c) for c in dw} == {(v, s, k) for v in (True, False) for s in (1, 2) for k in (True, False)}
    assert all(c["s"] in ((2, 1), (1, 2)) and c["k"] in ((3, 3), (3, 5), (5, 3)) and c["c"] in (8, 6) and c["padding"] == ac.SAME for c in dw)
    assert {(c["H"], c["W"]) for c in dw if c["twin_of"] is None} == {(10, 7), (9, 6)}
    for op in ("dw_q8", "dw_pre"):
        assert {c["s"][1] for c in base if c["op"] == op} == {1, 2} and len([c for c in base if c["op"] == op]) == 2
    # pools, PAD, folded PAD, SLICE
    for op in ("max_pool", "avg_pool"):
        assert {(c["k"], c["s"], c["H"], c["W"]) for c in base if c["op"] == op} == {((3, 3), (2, 1), 10, 7), ((2, 3), (1, 2), 7, 10)}
    assert {c["c"] for c in base if c["op"] == "pad"} == {8, 6}
    assert all(c["pad"] == ac.PADS and ac.pads_of(c) == ac.FOLDED_PADS for c in base if c["row"] in ("PAD", "PAD_FOLDED"))
    assert {c["op"] for c in base if c["row"] == "PAD_FOLDED"} == {"pad_conv", "pad_dw", "pad_dw_q8"}
    sl = [c for c in base if c["op"] == "slice"]
    assert len(sl) == 5 and sum(bool(c["kw"].get("c_total")) for c in sl) == 1 and sum("out_slice" in c["kw"] for c in sl) == 1
    assert any(c["kw"].get("c_from", 0) % 4 for c in sl) and any(c["kw"].get("out_slice", (0, 0))[0] % 4 for c in sl)


# ---- 3. sensitivity, on the references alone ----
def window_answer(c, x, s, pads):
    """The case's operator with explicit strides and pads on x -> (values, magnitudes or None)."""
    if c["op"] in ac.POOLS:
        return ac.pool_reference(x, ac.POOLS[c["op"]], c["k"], s, pads), None
    blob, info = ac.build(c, explicit=(s, pads))
    vals, mag = ac.reference(c, graph_of(blob), x)
    t = info["pad"] if c["op"] == "pad" else info["out"]
    return vals[t], mag.get(t)


def differs(c, own, other, mag):
    """By more than 1000 tolerances; a bit-exact case: somewhere in every sample.  Where the shapes differ the case is
    sensitive by shape already; a kernel that exchanged the parameters would still fill the planned shape, so the values
    are compared on the rows and columns both shapes have."""
    h, w = min(own.shape[1], other.shape[1]), min(own.shape[2], other.shape[2])
    own, other, mag = own[:, :h, :w], other[:, :h, :w], None if mag is None else mag[:, :h, :w]
    if c["op"] in ac.BIT_EXACT:
        return all(bool((own[n] != other[n]).any()) for n in range(own.shape[0]))
    if c["op"] == "avg_pool":
        return float(np.abs(own - other).max()) > 1000 * AVG_ABS
    return float((np.abs(own - other) / mag).max()) > 1000 * CONV_REL


@pytest.mark.parametrize("name", ac.NAMES)
def test_the_reference_tells_h_from_w(name):
    c = ac.BY_NAME[name]
    x = ac.inputs(c)
    blob, info = ac.build(c)
    g = graph_of(blob)
    vals, mags = ac.reference(c, g, x)
    if c["op"] == "slice":
        own = vals[info["out"]]
        x_in = vals[info["src"]]
        assert np.array_equal(own, ac.numpy_steps(x_in, c["steps"]))      # the evaluator and the NumPy statement of the chain agree
        swapped = ac.swapped_steps(c["steps"])
        assert swapped != c["steps"]
        other = ac.numpy_steps(x_in, swapped)
        assert np.array_equal(other, ac.reference(c, graph_of(ac.build(c, steps=swapped)[0]), x)[0][g.outputs[0]])
        if other.shape != own.shape:
            print("%s: sensitive by shape, %s against %s" % (name, own.shape[1:3], other.shape[1:3]))
        assert differs(c, own, other, None)
        return
    t = info["pad"] if c["op"] == "pad" else info["out"]
    own, mag = vals[t], mags.get(t)
    assert own.shape[1:3] == ac.window_shape(c)
    # the explicit form used below is the operator: with the case's own numbers it gives the case's own answer
    same, _ = window_answer(c, x, c["s"], ac.pads_of(c))
    assert np.array_equal(same, own) if c["op"] in ac.BIT_EXACT else float(np.abs(same - own).max()) < 1e-12
    ex = ac.exchanges(c)
    assert ex
    kept = [(label, s, p) for label, s, p in ex if ac.window_shape(c, s, p) == own.shape[1:3]]
    if not kept:
        print("%s: sensitive by shape, %s against %s" % (name, own.shape[1:3], [ac.window_shape(c, s, p) for _, s, p in ex]))
        assert all(ac.window_shape(c, s, p) != own.shape[1:3] for _, s, p in ex)
    for label, s, p in kept or ex:
        other, _ = window_answer(c, x, s, p)
        h, w = min(own.shape[1], other.shape[1]), min(own.shape[2], other.shape[2])
        gap = float(np.abs(own[:, :h, :w].astype(np.float64) - other[:, :h, :w]).max())
        print("%s: with the %s exchanged the answer moves by up to %.3g" % (name, label, gap))
        # (where only the shape tells -- pad_bottom against pad_right, which no kernel reads: they size the output -- the
        # shared rows and columns may agree)
        assert differs(c, own, other, mag) or not kept, (name, label)


# ---- 4. divisions the planner refuses, by the operator's name ----
@pytest.mark.parametrize("what", ["by_zero", "constant_by_activation"])
def test_refused_divisions(what):
    from cpx.ml_tools.tflite_graph import build_plan

    m = ts.ModelSE()
    x = m.tensor([1, 5, 3, 6], name="input")
    m.inputs = [x]
    c = np.array([1.0, 2.0, 0.0, 4.0, 5.0, 6.0], np.float32) if what == "by_zero" else np.full(6, 2.0, np.float32)
    m.outputs = [m.div(x, c, const_first=what != "by_zero")]
    with pytest.raises(NotImplementedError, match=r"DIV.*(constant 0|c / x)"):
        build_plan(graph_of(m.finish()))
