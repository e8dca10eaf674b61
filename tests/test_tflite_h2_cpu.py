"""The fp16x2 convolution math of the TFLite graph executor (build_plan(conv_math="fp16x2"): CPX_GRAPH_RANGE /
CPX_GRAPH_CONV_F16X2, include/cpx.h) on the host: the arithmetic alone against float64 (tests/tflite_eval_h2.py, the NumPy
restatement), RANGE's edge cases -- the restatement and the C++ function the kernel calls, compiled for the host --, the
filter packing and the planner.  Needs no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tflite_build as tb
import tflite_build_preact as tp
import tflite_build_q8 as tq
import tflite_eval_h2 as th

from cpx import _lib
from cpx.ml_tools import tflite_graph as tg
from cpx.ml_tools.tflite_reader import Graph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

# |restatement - float64| <= H2_REL * sum |x| |w|, derived, not measured: the two split remainders |x - xh - xl| <= 2^-22 |x|
# and |w - wh - wl| <= 2^-22 |w| (11 + 11 significand bits, each plane rounded to nearest), the dropped product
# |wl xl| <= 2^-22 |w| |x|, and one float32 rounding of the result (2^-24 of at most the sum): 3 * 2^-22 + 2^-24 < 2^-20
H2_REL = 2.0 ** -20


@pytest.mark.parametrize("family", th.FAMILIES)
def test_the_arithmetic_alone_is_float32_grade(family):
    """K = 3 * 3 * 288, He-normal weights.  Measured (max |error| / sum |x||w|): uniform 9.7e-9, wide 2.7e-8, relu 1.3e-8,
    spike 2.3e-7, tiny 9.1e-9 against the bound 9.5e-7."""
    rng = np.random.default_rng(12)
    x = th.families(rng, (2, 5, 5, 288))[family].astype(F32)
    w = rng.normal(0, np.sqrt(2.0 / (9 * 288)), size=(24, 3, 3, 288)).astype(F32)
    got, parts = th.conv(x, w, pads=(1, 1, 1, 1), parts=True)
    want, mag = th.conv_float64(x, w, pads=(1, 1, 1, 1))
    assert np.all(np.isfinite(got))
    rel = float((np.abs(got.astype(np.float64) - want) / mag).max())
    print("%s: max |error| / sum |x||w| = %.3g (bound %.3g); largest staged |xh| = %.6g" % (family, rel, H2_REL, parts["max_xh"]))
    # m * up < 2^15 in float32; rounding to fp16 may reach 2^15 itself (a finite fp16: the largest is 65504), never more
    assert all(float(np.abs(s).max()) * float(u) < 2.0 ** 15 for s, u in zip(x, parts["up"]))
    assert parts["max_xh"] <= 2.0 ** 15
    assert rel <= H2_REL, rel


@pytest.fixture(scope="module")
def range_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("graph_range") / "libgraph_range_host.so"
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall",
                           "-I", os.path.join(REPO, "classifier-pipeline_amd", "csrc"), "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "native", "graph_range_host.cpp"), "-o", str(out)])
    return C.CDLL(str(out))


def host_range(lib, m):
    m = np.ascontiguousarray(m, F32)
    up, down = np.empty_like(m), np.empty_like(m)
    lib.range_params_host(m.ctypes.data_as(C.c_void_p), int(m.size), up.ctypes.data_as(C.c_void_p), down.ctypes.data_as(C.c_void_p))
    return up, down


def is_normal(v):
    return np.isfinite(v) and abs(float(v)) >= float(np.finfo(F32).tiny)


def test_range_edge_cases(range_lib):
    # an all-zero sample, an infinite and a NaN maximum: no scaling
    for m in (0.0, np.inf, np.nan):
        assert th.range_params(np.full((2, 2, 3), m, F32)) == (1.0, 1.0)
    assert th.range_params(np.array([0.0, -np.inf, 1.0], F32)) == (1.0, 1.0)
    # m = 2^j exactly: f = 0.5, e = j + 1, so m * up = 2^14 until the clamp holds
    for j in (-140, -20, 0, 14, 15, 16, 127):
        m = F32(np.ldexp(1.0, j))
        up, down = th.range_params(np.array([m, -m / 2, 0], F32))
        k = min(15 - (j + 1), 100)
        assert (up, down) == (F32(np.ldexp(1.0, k)), F32(np.ldexp(1.0, -k))), j
        assert is_normal(up) and is_normal(down) and float(up) * float(down) == 1.0
        assert float(m) * float(up) == (2.0 ** 14 if j >= -86 else 2.0 ** (j + 100)) < 2.0 ** 15
    # just below a power of two: still below 2^15
    m = np.nextafter(F32(2.0 ** 20), F32(0))
    assert float(m) * float(th.range_params(np.array([m]))[0]) < 2.0 ** 15
    # a float32 subnormal maximum: the clamp holds, up and down are normal float32
    sub = F32(1e-41)
    assert 0 < sub < np.finfo(F32).tiny
    up, down = th.range_params(np.array([sub, 0], F32))
    assert (up, down) == (F32(2.0 ** 100), F32(2.0 ** -100)) and is_normal(up) and is_normal(down)
    # the C++ function the kernel calls agrees with the restatement, bit for bit
    rng = np.random.default_rng(3)
    ms = np.concatenate([np.ldexp(1.0, np.arange(-149, 128)), np.ldexp(rng.uniform(0.5, 1, 2000), rng.integers(-149, 129, 2000)),
                         [0.0, -0.0, np.inf, -1.0, np.nan, 3e38, 65504.0, 1e-41, float(np.finfo(F32).max)]]).astype(F32)
    up, down = host_range(range_lib, ms)
    want = [th.range_params(np.array([m], F32)) if not m < 0 else (F32(1), F32(1)) for m in ms]
    assert np.array_equal(up.view(np.uint32), np.array([w[0] for w in want], F32).view(np.uint32))
    assert np.array_equal(down.view(np.uint32), np.array([w[1] for w in want], F32).view(np.uint32))


@pytest.mark.parametrize("shape", [(3, 1, 1, 3), (80, 1, 7, 48), (2048, 1, 1, 288), (3, 5, 5, 288), (80, 5, 5, 3), (48, 1, 1, 48)],
                         ids=lambda s: "x".join(map(str, s)))
def test_filter_packing_round_trips(shape):
    rng = np.random.default_rng(sum(shape))
    co, kh, kw, ci = shape
    w = (rng.normal(0, 1, size=shape) * 2.0 ** rng.integers(-12, 6, size=(co, 1, 1, 1))).astype(F32)
    if co > 2:
        w[1] = 0   # an all-zero filter: kw = 0
    wh, wl, kwc = th.split_filter(w)
    live = np.abs(w).reshape(co, -1).max(axis=1) > 0
    assert np.all(kwc[~live] == 0)
    top = np.abs(wh.astype(np.float64).reshape(co, -1)).max(axis=1)
    assert np.all((top[live] >= 8) & (top[live] <= 16))   # [8, 16) before the rounding to fp16, which may reach 16
    packed = tg.pack_conv_filter_f16x2(w)
    KC, CO = _lib.GRAPH_CONV_H2_KC, _lib.GRAPH_CONV_CO
    assert KC == 32 and CO == 32
    nch, nt = -(-ci // KC), -(-co // CO)
    assert packed.dtype == np.uint8 and packed.size == 2 * kh * kw * nch * nt * 4 * 64 * 8 + 4 * nt * CO
    gh, gl, gk = tg.unpack_conv_filter_f16x2(packed, shape)
    assert gh.dtype == np.float16 and np.array_equal(gh.view(np.uint16), wh.view(np.uint16))
    assert np.array_equal(gl.view(np.uint16), wl.view(np.uint16)) and np.array_equal(gk, kwc)
    # the fragment order, element by element: [tap][chunk][tile][plane][m][lane][8], lane = 32 * half + channel of the tile
    frag = packed[:packed.size - 4 * nt * CO].view(np.float16).reshape(kh * kw, nch, nt, 2, 2, 64, 8)
    wdown = packed[packed.size - 4 * nt * CO:].view(F32)
    assert np.array_equal(wdown[:co], np.ldexp(F32(1), -kwc).astype(F32)) and np.all(wdown[co:] == 1)
    planes = np.zeros((2, nt * CO, kh * kw, nch * KC), np.float16)   # zeros beyond Cin / Cout
    planes[0, :co, :, :ci], planes[1, :co, :, :ci] = wh.reshape(co, kh * kw, ci), wl.reshape(co, kh * kw, ci)
    tap, chunk, tile, plane, m, lane, j = np.indices(frag.shape, sparse=True)
    want = planes[plane, tile * CO + (lane & 31), tap, chunk * KC + 16 * m + 8 * (lane >> 5) + j]
    assert np.array_equal(frag.view(np.uint16), want.view(np.uint16)) and np.count_nonzero(want) > 0


def kinds(plan):
    return [o.kind for o in plan.ops]


def ops_equal(a, b):
    """Two plans, operator for operator: kinds, names, tensors, windows, constants and the packed weights."""
    assert len(a.ops) == len(b.ops)
    for p, q in zip(a.ops, b.ops):
        assert (p.kind, p.name, p.in0, p.in1, p.out, p.kh, p.kw, p.stride_h, p.stride_w, p.pads, p.act, p.param) == \
            (q.kind, q.name, q.in0, q.in1, q.out, q.kh, q.kw, q.stride_h, q.stride_w, q.pads, q.act, q.param)
        for f in ("weights", "scale", "shift"):
            u, v = getattr(p, f), getattr(q, f)
            assert (u is None) == (v is None) and (u is None or (u.dtype == v.dtype and np.array_equal(u, v)))
    assert a.arena_floats == b.arena_floats and set(a.tensors) == set(b.tensors)
    return True


def check_ranges(plan):
    """One RANGE per distinct input view of the fp16x2 convolutions, each in front of its first consumer and behind every
    producer of its view; -> the number of RANGE operators."""
    convs = [o for o in plan.ops if o.kind == _lib.GRAPH_CONV_F16X2]
    ranges = [o for o in plan.ops if o.kind == _lib.GRAPH_RANGE]
    assert len(set(o.in0 for o in ranges)) == len(ranges) == len(set(o.in0 for o in convs))
    by_view = {o.in0: o for o in ranges}
    for r in ranges:
        t = plan.tensors[r.out]
        assert (t.H, t.W, t.C) == (1, 1, 4)
        at = plan.ops.index(r)
        readers = [plan.ops.index(o) for o in convs if o.in0 == r.in0]
        assert readers and min(readers) > at and all(plan.ops[k].in1 == r.out for k in readers)
        storage = plan.tensors[r.in0].storage
        writers = [k for k, o in enumerate(plan.ops) if plan.tensors[o.out].storage == storage]
        assert all(k < at for k in writers)
        # in front of the FIRST consumer: nothing between the RANGE and it reads the range tensor, and the operator right
        # behind the RANGE is that consumer
        assert min(readers) == at + 1
    for o in convs:
        assert o.in1 == by_view[o.in0].out and o.weights.dtype == np.uint8
    return len(ranges)


def test_inception_v3_plans_with_one_range_per_view():
    g = Graph(tb.inception_v3(9, (32,), seed=3, width=0.25))
    base = tg.build_plan(g)
    assert ops_equal(tg.build_plan(g, conv_math="f32"), base)
    plan = tg.build_plan(g, conv_math="fp16x2")
    n_conv = kinds(base).count(_lib.GRAPH_CONV)
    assert n_conv == 94 and _lib.GRAPH_CONV not in kinds(plan) and kinds(plan).count(_lib.GRAPH_CONV_F16X2) == 94
    n_ranges = check_ranges(plan)
    assert len(plan.ops) == len(base.ops) + n_ranges and n_ranges < 94   # the branches of a block share their input's
    # everything else is planned as before, in the same order
    rest = [o for o in plan.ops if o.kind != _lib.GRAPH_RANGE]
    for o, b in zip(rest, base.ops):
        assert (o.name, o.in0, o.out, o.pads, o.act) == (b.name, b.in0, b.out, b.pads, b.act)
        assert o.kind == (_lib.GRAPH_CONV_F16X2 if b.kind == _lib.GRAPH_CONV else b.kind)
        if o.kind == _lib.GRAPH_CONV_F16X2:
            assert np.array_equal(o.weights, tg.pack_conv_filter_f16x2(o.filter)) and np.array_equal(o.shift, b.shift)
    with pytest.raises(ValueError, match="conv_math"):
        tg.build_plan(g, conv_math="bf16")
    assert tg.CONV_MATHS == ("f32", "fp16x2")
    assert (_lib.GRAPH_RANGE, _lib.GRAPH_CONV_F16X2) == (22, 23)


def test_a_folded_pad_moves_the_range_to_its_input():
    rng = np.random.default_rng(4)
    m = tb.Model()
    x = m.tensor([1, 9, 9, 8], name="input")
    m.inputs = [x]
    a = m.conv(x, rng.normal(0, 0.2, size=(16, 1, 1, 8)).astype(F32), np.zeros(16, F32), 1, tb.SAME, tb.RELU)
    p = m.pad(a, [[0, 0], [1, 1], [1, 1], [0, 0]])
    y = m.conv(p, rng.normal(0, 0.1, size=(8, 3, 3, 16)).astype(F32), np.zeros(8, F32), 2, tb.VALID, tb.NONE)
    z = m.conv(a, rng.normal(0, 0.1, size=(8, 1, 1, 16)).astype(F32), np.zeros(8, F32), 2, tb.SAME, tb.NONE)   # a second reader of `a`
    m.outputs = [m.binary("ADD", y, z)]
    g = Graph(m.finish())
    kept = tg.build_plan(g, conv_math="fp16x2")
    assert [o.name for o in kept.ops] == ["RANGE", "CONV_2D", "PAD", "RANGE", "CONV_2D", "RANGE", "CONV_2D", "ADD"]
    plan = tg.build_plan(g, conv_math="fp16x2", fold_windows=True)
    assert [o.name for o in plan.ops] == ["RANGE", "CONV_2D", "RANGE", "PAD>CONV_2D", "CONV_2D", "ADD"]
    check_ranges(plan)
    folded = plan.ops[3]
    assert folded.kind == _lib.GRAPH_CONV_F16X2 and folded.in0 == a and folded.pads == (1, 1, 1, 1)
    assert plan.ops[2].in0 == a and folded.in1 == plan.ops[2].out == plan.ops[4].in1   # ONE range of `a`, shared
    assert p not in plan.tensors


def test_a_densenet_block_keeps_its_affine_launch():
    g = Graph(tp.densenet(5, blocks=(2, 2), growth=8, stem=16, size=32, seed=2))
    fused = tg.build_plan(g, fuse_preactivation=True, fold_windows=True)
    assert _lib.GRAPH_CONV_PRE in kinds(fused)
    plan = tg.build_plan(g, fuse_preactivation=True, fold_windows=True, conv_math="fp16x2")
    ks = kinds(plan)
    assert _lib.GRAPH_CONV_PRE not in ks and _lib.GRAPH_CONV not in ks
    unfused = tg.build_plan(g, fold_windows=True)
    assert ks.count(_lib.GRAPH_AFFINE) == kinds(unfused).count(_lib.GRAPH_AFFINE) > kinds(fused).count(_lib.GRAPH_AFFINE)
    assert ks.count(_lib.GRAPH_CONV_F16X2) == kinds(unfused).count(_lib.GRAPH_CONV)
    check_ranges(plan)
    # a convolution reads the AFFINE's output, and so does its RANGE: the pre-activated values are what is measured
    affine_outs = {o.out for o in plan.ops if o.kind == _lib.GRAPH_AFFINE}
    assert any(o.kind == _lib.GRAPH_RANGE and o.in0 in affine_outs for o in plan.ops)


def test_a_quantised_graph_plans_hybrid_as_before_and_float_as_fp16x2():
    rng = np.random.default_rng(1)
    m = tb.Model()
    x = m.tensor([1, 9, 9, 64], name="input")
    m.inputs = [x]
    c = m.conv(x, rng.normal(0, 0.1, size=(48, 3, 3, 64)).astype(F32), rng.normal(0, 0.05, size=48).astype(F32), 1, tb.SAME, tb.RELU)
    m.outputs = [m.conv(c, rng.normal(0, 0.1, size=(40, 3, 3, 48)).astype(F32), rng.normal(0, 0.05, size=40).astype(F32), 1, tb.SAME, tb.RELU)]
    g = Graph(tq.quantise(m.finish()))
    assert all(g.quantised_filter(op) is not None for op in g.ops)
    hybrid = tg.build_plan(g, quantised_math="hybrid")
    assert _lib.GRAPH_CONV_Q8 in kinds(hybrid)
    assert ops_equal(tg.build_plan(g, quantised_math="hybrid", conv_math="fp16x2"), hybrid)
    assert ops_equal(tg.build_plan(g, quantised_math="hybrid", conv_math="f32"), hybrid)
    both = tg.build_plan(g, quantised_math="float", conv_math="fp16x2")
    assert kinds(both) == [_lib.GRAPH_RANGE, _lib.GRAPH_CONV_F16X2, _lib.GRAPH_RANGE, _lib.GRAPH_CONV_F16X2]
    for o in both.ops[1::2]:
        ten = g.tensors[g.ops[o.source]["inputs"][1]]
        want = ten["const"].astype(F32) * ten["quant"]["scale"].reshape(-1, 1, 1, 1)
        assert np.array_equal(o.weights, tg.pack_conv_filter_f16x2(want))


def test_interpreter_reads_the_environment(monkeypatch):
    from cpx.ml_tools.interpreter import LiteInterpreter

    monkeypatch.delenv("CPX_TFLITE_CONV_MATH", raising=False)
    assert LiteInterpreter.conv_math() == "f32"
    monkeypatch.setenv("CPX_TFLITE_CONV_MATH", "fp16x2")
    assert LiteInterpreter.conv_math() == "fp16x2"
    monkeypatch.setenv("CPX_TFLITE_CONV_MATH", "fp16")
    with pytest.raises(ValueError, match="CPX_TFLITE_CONV_MATH"):
        LiteInterpreter.conv_math()


def test_describe_counts_the_fp16x2_convolutions_and_range_launches(capsys):
    import importlib.util

    spec = importlib.util.spec_from_file_location("tflite_to_npz", os.path.join(REPO, "tools", "tflite_to_npz.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g = Graph(tp.densenet(5, blocks=(2, 2), growth=8, stem=16, size=32, seed=2))
    assert tool.describe(g) == 0
    assert "conv_math" not in capsys.readouterr().out
    assert tool.describe(g, conv_math="fp16x2") == 0
    out = capsys.readouterr().out
    plan = tg.build_plan(g, fuse_preactivation=True, fold_windows=True, conv_math="fp16x2")
    n_conv, n_range = kinds(plan).count(_lib.GRAPH_CONV_F16X2), kinds(plan).count(_lib.GRAPH_RANGE)
    assert "conv_math fp16x2: %d convolutions go fp16x2 behind %d RANGE launches; 5 pre-activations stay AFFINE launches" % (n_conv, n_range) in out
