"""The windowed operators of the TFLite graph executor on non-square maps with unequal strides and one-sided pads
(tests/tflite_aniso_cases.py: every case and its twin with H / W and all per-axis parameters exchanged, N = 3) against
their references: float64 for the float32 operators, the NumPy restatement for the hybrid ones, NumPy's own indexing and
np.pad for the copies.  A stride_h / stride_w, pad_top / pad_left or H / W exchanged anywhere between the planner, the
GraphOpArgs marshalling and a kernel's index arithmetic fails here; tests/test_tflite_aniso_cpu.py shows on the references
alone that these inputs tell the two apart.  Every case also pins the kinds of its plan's launches, so that it cannot run
another kernel than the one it names."""
import numpy as np
import pytest

import tflite_aniso_cases as ac
from test_tflite_graph_gpu import CONV_REL

pytestmark = pytest.mark.gpu
F32 = np.float32
AVG_ABS = 2e-6                      # AVERAGE_POOL_2D: tests/test_tflite_graph_gpu.py::test_pools' bound
SENTINEL = F32(-12345.678)


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


def check_bits(name, got, want, what):
    n_diff = int((bits(got) != bits(want)).sum()) if got.shape == want.shape else -1
    print("%s: %d of %d elements differ from %s" % (name, n_diff, got.size, what))
    assert got.shape == want.shape and n_diff == 0, (name, what, got.shape, want.shape, n_diff)


@pytest.mark.parametrize("name", ac.NAMES)
def test_anisotropic_window(engine, name):
    c = ac.BY_NAME[name]
    op = c["op"]
    blob, info = ac.build(c)
    x = ac.inputs(c)
    folds = ac.FOLDS.get(op, {})
    g, plan, got = run(engine, blob, x, **folds)
    assert ac.kinds(plan) == ac.plan_kinds(c), ac.kinds(plan)
    assert np.all(np.isfinite(got)) and float(np.abs(got).max()) > 0.1
    vals, mags = ac.reference(c, g, x)
    out = g.outputs[0]
    if op != "slice":
        main = plan.ops[0] if op == "pad" else plan.ops[-1]
        assert main.pads == ac.pads_of(c)
    if op != "slice" and op != "pad":
        assert (main.stride_h, main.stride_w) == c["s"] and (main.kh, main.kw) == c["k"] and got.shape[1:3] == ac.window_shape(c)

    # ---- against the reference ----
    if op in ac.HYBRID:
        check_bits(name, got, vals[out], "the restatement")
        assert float(np.abs(vals[out][0]).max()) > 0.1
    elif op in ("max_pool", "pad"):
        # (values, not bits: which of a -0.0 and a +0.0 is the maximum IEEE 754 leaves open)
        n_diff = int((got != vals[out]).sum()) if got.shape == vals[out].shape else -1
        print("%s: %d of %d maxima differ from float64's" % (name, n_diff, got.size))
        assert n_diff == 0
    elif op == "avg_pool":
        err = float(np.abs(got - vals[out]).max())
        print("%s: max |error| = %.3g (bound %.3g)" % (name, err, AVG_ABS))
        assert got.shape == vals[out].shape and err < AVG_ABS
    elif op == "slice":
        x_in = x
        if c["kw"].get("c_total"):
            t = plan.tensors[plan.ops[-1].in0]
            assert (t.c_offset, t.c_stride) == (c["kw"]["c_from"], c["kw"]["c_total"]) and t.c_offset % 4 != 0
            x_in = run(engine, blob, x, output=info["src"])[2]
            assert np.array_equal(bits(x_in), bits(x))
        else:
            assert len(plan.ops) == 1
        assert (bits(x_in) == 0x80000000).any()
        want = ac.numpy_steps(x_in, c["steps"])
        check_bits(name, got, want, "NumPy's indexing")
        mean = any(st[0] == "pool" and st[1][0] == "A" for st in c["steps"])
        assert plan.ops[-1].param == (1.0 if mean else 0.0) and (bits(got) == 0x80000000).any() != mean
        assert np.array_equal(want.astype(np.float64), vals[out])
        if "out_slice" in c["kw"]:
            import torch

            off, stride = c["kw"]["out_slice"]
            buf = torch.full(got.shape[:3] + (stride,), float(SENTINEL), dtype=torch.float32, device=engine.device)
            _, _, sliced = run(engine, blob, x, out_slice=(off, stride), out=buf, **folds)
            assert np.array_equal(bits(sliced[..., off:off + c["c"]]), bits(want)) and off % 4 != 0
            assert np.all(sliced[..., :off] == SENTINEL) and np.all(sliced[..., off + c["c"]:] == SENTINEL)
    else:
        rel = float((np.abs(got - vals[out]) / mags[out]).max())
        print("%s: max |error| / (sum |x| |w| + |b|) = %.3g (bound %.3g)" % (name, rel, CONV_REL))
        assert got.shape == vals[out].shape and rel < CONV_REL

    # ---- PAD as a launch: the padded tensor itself is np.pad's bits ----
    if op == "pad":
        _, pplan, padded = run(engine, blob, x, output=info["pad"], **folds)
        assert ac.kinds(pplan) == ["PAD"] and pplan.ops[0].pads == ac.pads_of(c)
        check_bits(name, padded, np.pad(x, ((0, 0), c["pad"][0], c["pad"][1], (0, 0))), "np.pad")
        assert (bits(padded) == 0x80000000).any()

    # ---- a folded launch is bit-equal to the launches it replaces ----
    if op in ac.UNFOLDED_KINDS:
        _, plain, unfolded = run(engine, blob, x)
        assert ac.kinds(plain) == ac.UNFOLDED_KINDS[op] and len(plan.ops) == len(plain.ops) - 1
        check_bits(name, got, unfolded, "the unfolded plan")
        if c["pad"] is not None:
            assert plan.ops[-1].in0 == plan.input and plan.arena_floats < plain.arena_floats
            if c["twin_of"] is None:
                assert plan.ops[-1].pads == ac.FOLDED_PADS
            if op in ("pad_conv", "pad_dw"):
                assert float(x[2].min()) > 0    # an all-positive sample: its minimum is 0 only through the padding
