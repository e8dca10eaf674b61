"""Helper (not a test): the anisotropic cases of the TFLite graph executor's windowed operators -- every map H != W, N = 3,
and at least one of stride_h != stride_w, pad_top != pad_left, pad_bottom != pad_right or a slice whose begin / stride
differ per axis -- and the builders of their one-operator graphs.  Shared by tests/test_tflite_aniso_cpu.py (planner
geometry, the table's self-check, sensitivity of the references) and tests/test_tflite_aniso_gpu.py (the kernels), so that
both see the same cases.  Every base case has its twin: H / W and every per-axis parameter exchanged.

Everything here is plain arithmetic on the case list and the flatbuffer writers of tests/tflite_build*.py; nothing depends
on what a kernel or the planner gives."""
import numpy as np

import tflite_build as tb
import tflite_build_dw as td
import tflite_build_nas as tn
import tflite_build_preact as tp
import tflite_eval as te

F32 = np.float32
N = 3
SAME, VALID = tb.SAME, tb.VALID
PADS = ((1, 2), (3, 0))            # PAD [[0,0],[1,2],[3,0],[0,0]]: all four differ
FOLDED_PADS = (1, 3, 2, 0)         # ... as the launch that took it carries them: top, left, bottom, right
MAX_MAP, MAX_CHANNELS = 14, 96

# operator of a case -> the kinds of the plan's launches (names of the CPX_GRAPH_* enum), with the case's folds on
PLAN_KINDS = {
    "conv": ["CONV"], "conv_pre": ["CONV_PRE"], "conv_q8": ["QUANT_PARAMS", "CONV_Q8"],
    "dw": ["DWCONV"], "dw_q8": ["QUANT_PARAMS", "DWCONV_Q8"], "dw_pre": ["DWCONV_PRE"],
    "max_pool": ["MAX_POOL"], "avg_pool": ["AVG_POOL"], "pad": ["PAD", "MAX_POOL"],
    "pad_conv": ["CONV"], "pad_dw": ["DWCONV"], "pad_dw_q8": ["QUANT_PARAMS", "DWCONV_Q8"], "slice": ["SLICE"],
}
# ... and without them (the launches the folded ones are held bit-equal to)
UNFOLDED_KINDS = {
    "conv_pre": ["AFFINE", "CONV"], "dw_pre": ["AFFINE", "DWCONV"], "pad_conv": ["PAD", "CONV"], "pad_dw": ["PAD", "DWCONV"],
    "pad_dw_q8": ["PAD", "QUANT_PARAMS", "DWCONV_Q8"],
}
FOLDS = {
    "conv_pre": dict(fuse_preactivation=True), "dw_pre": dict(fuse_preactivation_dw=True),
    "pad": dict(fold_windows=True), "pad_conv": dict(fold_windows=True), "pad_dw": dict(fold_windows=True),
    "pad_dw_q8": dict(fold_windows=True), "slice": dict(fold_windows=True),
}
HYBRID = ("conv_q8", "dw_q8", "pad_dw_q8")
DEPTHWISE = ("dw", "dw_q8", "dw_pre", "pad_dw", "pad_dw_q8")
CONVOLUTION = ("conv", "conv_pre", "conv_q8", "pad_conv")
POOLS = {"max_pool": "MAX_POOL_2D", "avg_pool": "AVERAGE_POOL_2D"}
BIT_EXACT = HYBRID + ("max_pool", "pad", "slice")     # the rest: a relative bound on the magnitude


def case(row, name, op, H, W, c, cout=0, k=(1, 1), s=(1, 1), padding=VALID, pad=None, steps=None, **kw):
    return dict(row=row, name=name, op=op, H=H, W=W, c=c, cout=cout, k=tuple(k), s=tuple(s), padding=padding, pad=pad,
                steps=steps, kw=kw, twin_of=None)


def _swap(v):
    return (v[1], v[0])


def swapped_steps(steps):
    """A SLICE chain with the H and W parameters of every step exchanged."""
    return [(st[0],) + tuple(_swap(st[1:])) if st[0] != "pool" else ("pool", st[1], _swap(st[2])) for st in steps]


def twin(c):
    """The case with H / W and every per-axis parameter exchanged."""
    t = dict(c, name=c["name"] + "_T", H=c["W"], W=c["H"], k=_swap(c["k"]), s=_swap(c["s"]), twin_of=c["name"])
    if c["pad"] is not None:
        t["pad"] = _swap(c["pad"])
    if c["steps"] is not None:
        t["steps"] = swapped_steps(c["steps"])
    return t


BASE = [
    # ---- CONV_2D float32: Cin 5 (scalar loads) and 8 (16-byte loads), Cout 24 (NTN = 1) and 40 (NTN = 2) ----
    case("CONV", "conv_3x3_s21_same_10x7", "conv", 10, 7, 5, 24, (3, 3), (2, 1), SAME),
    case("CONV", "conv_5x3_s22_same_10x7", "conv", 10, 7, 8, 40, (5, 3), (2, 2), SAME),
    case("CONV", "conv_3x2_s12_valid_6x9", "conv", 6, 9, 8, 24, (3, 2), (1, 2), VALID),
    case("CONV", "conv_1x1_s21_valid_9x6", "conv", 9, 6, 5, 40, (1, 1), (2, 1), VALID),
    case("CONV_PRE", "conv_pre_3x3_s21_same_10x7", "conv_pre", 10, 7, 8, 24, (3, 3), (2, 1), SAME),
    case("CONV_Q8", "conv_q8_3x3_s21_same_10x7", "conv_q8", 10, 7, 8, 40, (3, 3), (2, 1), SAME),
    case("CONV_Q8", "conv_q8_3x3_s12_valid_9x6", "conv_q8", 9, 6, 5, 24, (3, 3), (1, 2), VALID),
    # ---- DEPTHWISE float32: [16-byte or scalar][stride_w 1 or 2][kw <= 3 or kw > 3], base cases and twins together ----
    case("DWCONV", "dw_3x3_s21_c8_10x7", "dw", 10, 7, 8, 8, (3, 3), (2, 1), SAME),
    case("DWCONV", "dw_3x5_s21_c8_9x6", "dw", 9, 6, 8, 8, (3, 5), (2, 1), SAME),
    case("DWCONV", "dw_5x3_s21_c8_10x7", "dw", 10, 7, 8, 8, (5, 3), (2, 1), SAME),
    case("DWCONV", "dw_3x3_s21_c6_9x6", "dw", 9, 6, 6, 6, (3, 3), (2, 1), SAME),
    case("DWCONV", "dw_3x5_s21_c6_10x7", "dw", 10, 7, 6, 6, (3, 5), (2, 1), SAME),
    case("DWCONV", "dw_5x3_s21_c6_9x6", "dw", 9, 6, 6, 6, (5, 3), (2, 1), SAME),
    case("DWCONV_Q8", "dw_q8_3x5_s21_c8_10x7", "dw_q8", 10, 7, 8, 8, (3, 5), (2, 1), SAME),
    case("DWCONV_Q8", "dw_q8_3x3_s12_c6_9x6", "dw_q8", 9, 6, 6, 6, (3, 3), (1, 2), SAME),
    case("DWCONV_PRE", "dw_pre_5x3_s21_c8_10x7", "dw_pre", 10, 7, 8, 8, (5, 3), (2, 1), SAME),
    case("DWCONV_PRE", "dw_pre_3x3_s12_c6_9x6", "dw_pre", 9, 6, 6, 6, (3, 3), (1, 2), SAME),
    # ---- pools ----
    case("MAX_POOL", "max_pool_3x3_s21_same_10x7", "max_pool", 10, 7, 20, 20, (3, 3), (2, 1), SAME),
    case("MAX_POOL", "max_pool_2x3_s12_same_7x10", "max_pool", 7, 10, 20, 20, (2, 3), (1, 2), SAME),
    case("AVG_POOL", "avg_pool_3x3_s21_same_10x7", "avg_pool", 10, 7, 20, 20, (3, 3), (2, 1), SAME),
    case("AVG_POOL", "avg_pool_2x3_s12_same_7x10", "avg_pool", 7, 10, 20, 20, (2, 3), (1, 2), SAME),
    # ---- PAD as a launch (in front of a 3 x 3 MAX_POOL_2D, into which no PAD folds) ----
    case("PAD", "pad_1230_c8_7x9", "pad", 7, 9, 8, 8, pad=PADS),
    case("PAD", "pad_1230_c6_7x9", "pad", 7, 9, 6, 6, pad=PADS),
    # ---- PAD folded into the VALID operator behind it ----
    case("PAD_FOLDED", "pad_conv_3x5_valid_7x9", "pad_conv", 7, 9, 8, 24, (3, 5), (1, 1), VALID, pad=PADS),
    case("PAD_FOLDED", "pad_dw_3x5_s12_valid_7x9", "pad_dw", 7, 9, 8, 8, (3, 5), (1, 2), VALID, pad=PADS),
    case("PAD_FOLDED", "pad_dw_q8_3x5_s12_valid_7x9", "pad_dw_q8", 7, 9, 8, 8, (3, 5), (1, 2), VALID, pad=PADS),
    # ---- SLICE: steps of (kind, H parameters, W parameters) ----
    case("SLICE", "slice_from_1_by_2_and_from_2", "slice", 7, 6, 8, 8, steps=[("ss", (1, 2), (2, 1))]),          # x[:, 1::2, 2:]
    case("SLICE", "slice_crop_10_02_scalar", "slice", 7, 6, 3, 3, steps=[("crop", (1, 0), (0, 2))], as_slice=True),
    case("SLICE", "slice_pad_crop_pool_one_launch", "slice", 9, 6, 8, 8,
         steps=[("pad", (0, 1), (2, 0)), ("crop", (1, 0), (0, 1)), ("pool", "AVERAGE_POOL_2D", (2, 1))]),
    case("SLICE", "slice_reads_off_the_quad_grid", "slice", 7, 6, 16, 16, steps=[("ss", (1, 2), (2, 1))], c_total=40, c_from=6),
    case("SLICE", "slice_writes_off_the_quad_grid", "slice", 7, 6, 8, 8, steps=[("crop", (1, 0), (0, 2))], out_slice=(5, 16)),
]
CASES = BASE + [twin(c) for c in BASE]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c["name"] for c in CASES]
ROWS = ["CONV", "CONV_PRE", "CONV_Q8", "DWCONV", "DWCONV_Q8", "DWCONV_PRE", "MAX_POOL", "AVG_POOL", "PAD", "PAD_FOLDED", "SLICE"]


KIND_NAMES = ("CONV", "MAX_POOL", "AVG_POOL", "ADD", "AFFINE", "MEAN", "FC", "LOGISTIC", "SOFTMAX", "PAD", "CHANNEL_MAP", "CONV_Q8",
              "FC_Q8", "QUANT_PARAMS", "DWCONV", "DWCONV_Q8", "MUL", "INPUT", "CONV_PRE", "SLICE", "DWCONV_PRE")


def seed_of(c):
    return sum(map(ord, c["name"]))


def kinds(plan):
    """The plan's launches by the names of the CPX_GRAPH_* enum."""
    from cpx import _lib

    names = {getattr(_lib, "GRAPH_" + n): n for n in KIND_NAMES}
    return [names[o.kind] for o in plan.ops]


def plan_of(c, blob, folded=True):
    """(Graph, plan) of a case's flatbuffer on the case's map, with the case's folds or without any."""
    from cpx.ml_tools.tflite_graph import build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    return g, build_plan(g, input_shape=(c["H"], c["W"], c["c"]), **(FOLDS.get(c["op"], {}) if folded else {}))


def plan_kinds(c):
    """The launches of the case's plan, by kind."""
    if c["kw"].get("c_total"):   # the 1 x 1 MAX_POOL_2D that feeds the concatenation's slice is a SLICE too, then the two convolutions
        return ["SLICE", "CONV", "CONV", "SLICE"]
    return PLAN_KINDS[c["op"]]


# ---- geometry, from tflite_eval._pads alone ----
def pads_of(c):
    """(pad_top, pad_left, pad_bottom, pad_right) of the case's windowed operator: the PAD's four where there is one (the
    operator behind it is VALID), TensorFlow's SAME / VALID arithmetic per axis otherwise."""
    if c["pad"] is not None:
        (pt, pb), (pl, pr) = c["pad"]
        return (pt, pl, pb, pr)
    pt, pb = te._pads(c["H"], c["k"][0], c["s"][0], c["padding"])
    pl, pr = te._pads(c["W"], c["k"][1], c["s"][1], c["padding"])
    return (pt, pl, pb, pr)


def window_shape(c, s=None, pads=None):
    """Output pixels of the window with explicit strides and pads (default: the case's own)."""
    (sh, sw), (pt, pl, pb, pr) = s or c["s"], pads or pads_of(c)
    return ((c["H"] + pt + pb - c["k"][0]) // sh + 1, (c["W"] + pl + pr - c["k"][1]) // sw + 1)


def dw_instantiation(c):
    """[16-byte or scalar][stride_w][kw <= 3 or above] of graph_dw_kernel that a depthwise case launches."""
    return (c["c"] % 4 == 0, c["s"][1], c["k"][1] > 3)


def asymmetries(c):
    """Which of the asymmetry conditions the case meets."""
    out = []
    if c["steps"] is not None:
        if any(st[0] == "pool" and st[2][0] != st[2][1] or st[0] != "pool" and st[1] != st[2] for st in c["steps"]):
            out.append("slice")
        return out
    pt, pl, pb, pr = pads_of(c)
    if c["s"][0] != c["s"][1]:
        out.append("stride")
    if pt != pl:
        out.append("pad_top_left")
    if pb != pr:
        out.append("pad_bottom_right")
    return out


def exchanges(c):
    """[(label, strides, pads)]: the H and W parameters of the window exchanged -- the strides, the pads, both -- leaving
    out what is the case itself."""
    s, p = c["s"], pads_of(c)
    ps = (p[1], p[0], p[3], p[2])
    out = []
    for label, s2, p2 in (("strides", _swap(s), p), ("pads", s, ps), ("strides and pads", _swap(s), ps)):
        if (s2, p2) != (s, p) and not any((s2, p2) == (a, b) for _, a, b in out):
            out.append((label, s2, p2))
    return out


# ---- inputs ----
def signed_sample(rng, shape, scale=1.0):
    """Normal values with a -0.0, a +0.0 and a tiny negative sprinkled in: a copy that is not one shows in the bits."""
    x = rng.normal(0, scale, size=shape).astype(F32)
    kind = rng.random(size=shape)
    x[kind < 0.04] = -0.0
    x[(kind >= 0.04) & (kind < 0.06)] = 0.0
    x[(kind >= 0.06) & (kind < 0.08)] = -1e-30
    return x


def three_samples(rng, H, W, c):
    """One sample all positive (zp = -128: a padded tap staged as 0 instead of zp shows at every border), one all negative
    (zp = 127), one mixed."""
    return np.stack([rng.uniform(1, 5, size=(H, W, c)), rng.uniform(-4, -0.5, size=(H, W, c)),
                     rng.uniform(-2, 3, size=(H, W, c))]).astype(F32)


def inputs(c):
    rng = np.random.default_rng(seed_of(c) + 1)
    shape = (N, c["H"], c["W"], c["c"])
    if c["op"] in HYBRID:
        return three_samples(rng, *shape[1:])
    if c["op"] in POOLS:
        return rng.uniform(-5, -1, size=shape).astype(F32)   # negative: a padded zero must never win a maximum
    if c["op"] in ("pad", "slice", "dw_pre"):
        return signed_sample(rng, shape)
    if c["op"] == "pad_conv" or c["op"] == "pad_dw":
        x = signed_sample(rng, shape)
        x[2] = rng.uniform(0.5, 2.0, size=shape[1:]).astype(F32)
        return x
    return rng.uniform(-1, 1, size=shape).astype(F32)


# ---- graphs ----
def emit_steps(m, t, steps, H, W, as_slice=False):
    """The chain of a SLICE case behind tensor t of H x W pixels -> its last tensor."""
    for st in steps:
        if st[0] == "pad":
            (t0, t1), (l0, l1) = st[1], st[2]
            t = m.pad(t, [[0, 0], [t0, t1], [l0, l1], [0, 0]])
            H, W = H + t0 + t1, W + l0 + l1
        elif st[0] == "ss":      # x[:, bh::sh, bw::sw]
            (bh, sh), (bw, sw) = st[1], st[2]
            t = m.strided_slice(t, [0, bh, bw, 0], [0, 0, 0, 0], [1, sh, sw, 1], begin_mask=0b1001, end_mask=0b1111)
            H, W = -(-(H - bh) // sh), -(-(W - bw) // sw)
        elif st[0] == "crop":    # Cropping2D((t0, t1), (l0, l1)): as a SLICE with sizes, or a STRIDED_SLICE with ends from the back
            (t0, t1), (l0, l1) = st[1], st[2]
            if as_slice:
                t = m.slice(t, [0, t0, l0, 0], [-1, H - t0 - t1, W - l0 - l1, -1])
            else:
                t = m.strided_slice(t, [0, t0, l0, 0], [0, -t1, -l1, 0], [1, 1, 1, 1], begin_mask=0b1001,
                                    end_mask=0b1001 | (2 if t1 == 0 else 0) | (4 if l1 == 0 else 0))
            H, W = H - t0 - t1, W - l0 - l1
        else:
            t = m.pool(st[1], t, 1, st[2], VALID)
            H, W = -(-H // st[2][0]), -(-W // st[2][1])
    return t


def numpy_steps(x, steps):
    """What the chain is in NumPy's indexing (a 1 x 1 AVERAGE_POOL_2D is the element + 0.0: its -0.0 is a +0.0)."""
    for st in steps:
        if st[0] == "pad":
            x = np.pad(x, ((0, 0), st[1], st[2], (0, 0)))
        elif st[0] == "ss":
            x = x[:, st[1][0]::st[1][1], st[2][0]::st[2][1]]
        elif st[0] == "crop":
            x = x[:, st[1][0]:x.shape[1] - st[1][1], st[2][0]:x.shape[2] - st[2][1]]
        else:
            x = x[:, ::st[2][0], ::st[2][1]]
            if st[1][0] == "A":
                x = x + x.dtype.type(0)
    return np.ascontiguousarray(x)


def build(c, explicit=None, steps=None):
    """-> (flatbuffer bytes, {"out": the operator's output tensor, "pad": the PAD's output, "src": what a SLICE chain reads}).
    explicit = (strides, (pt, pl, pb, pr)): the window as PAD + the VALID operator with these instead of the case's own
    (the filters are the case's: drawn first, from the case's seed); steps: another chain for a SLICE case."""
    rng = np.random.default_rng(seed_of(c))
    op, H, W, cin, (kh, kw) = c["op"], c["H"], c["W"], c["c"], c["k"]
    m = tn.ModelNAS()
    x = m.tensor([1, H, W, cin], name="input")
    m.inputs = [x]
    info = {}
    if op == "slice":
        src = x
        if c["kw"].get("c_total"):
            c_total, c_from = c["kw"]["c_total"], c["kw"]["c_from"]

            def conv(co):
                return m.conv(x, rng.normal(0, 0.3, size=(co, 1, 1, cin)).astype(F32), rng.normal(size=co).astype(F32), 1, SAME, tb.NONE)

            src = m.pool("MAX_POOL_2D", x, 1, 1, VALID)    # the one producer that hands a -0.0 on
            m.concat([conv(c_from), src, conv(c_total - c_from - cin)])
        info["src"] = src
        info["out"] = emit_steps(m, src, c["steps"] if steps is None else steps, H, W, c["kw"].get("as_slice", False))
        m.outputs = [info["out"]]
        return m.finish(), info
    if op in CONVOLUTION:
        w = rng.normal(0, np.sqrt(2.0 / (kh * kw * cin)), size=(c["cout"], kh, kw, cin)).astype(F32)
        b = rng.normal(0, 0.05, size=c["cout"]).astype(F32)
    elif op in DEPTHWISE:
        w = rng.normal(0, np.sqrt(2.0 / (kh * kw)), size=(1, kh, kw, cin)).astype(F32)
        b = rng.normal(0, 0.05, size=cin).astype(F32)
    t = x
    if op == "conv_pre":
        t = info["pre"] = tp.preact(m, rng, x)        # MUL, ADD + RELU by per-channel constants
    elif op == "dw_pre":
        t = info["pre"] = m.unary("RELU", x)
    s, padding, pads = c["s"], c["padding"], c["pad"]
    if explicit is not None:
        s, (pt, pl, pb, pr) = explicit
        padding, pads = VALID, ((pt, pb), (pl, pr)) if max(pt, pl, pb, pr) > 0 or op == "pad" else None
    if pads is not None:
        t = info["pad"] = m.pad(t, [[0, 0], list(pads[0]), list(pads[1]), [0, 0]])
    if op in CONVOLUTION:
        y = m.conv(t, w, b, s, padding, tb.NONE)
    elif op in DEPTHWISE:
        y = m.depthwise(t, w, b, s, padding, tb.NONE)
    elif op in POOLS:
        y = m.pool(POOLS[op], t, c["k"], s, padding)
    else:
        assert op == "pad", op
        y = m.pool("MAX_POOL_2D", t, 3, 1, VALID)
    info["out"] = y
    m.outputs = [y]
    blob = m.finish()
    return (td.quantise(blob, min_elements=0) if op in HYBRID else blob), info


def reference(c, g, x):
    """-> ({tensor id: array}, {tensor id: magnitude}): the restatement of the hybrid arithmetic (float32, tests/tflite_eval_dw.py)
    for a hybrid case, else the float64 evaluation operator by operator (tests/tflite_eval_nas.py, which hands CONV_2D and
    the pools to tflite_eval, DEPTHWISE_CONV_2D to tflite_eval_dw and slices to NumPy)."""
    import tflite_eval_dw as ted
    import tflite_eval_nas as ten

    if c["op"] in HYBRID:
        return ted.evaluate_hybrid(g, x)
    return ten.evaluate(g, x, magnitudes=True)


def pool_reference(x, kind, k, s, pads):
    """float64 MAX_POOL_2D / AVERAGE_POOL_2D with explicit strides and pads: padding never wins a maximum and is left out
    of an average's divisor."""
    (kh, kw), (sh, sw), (pt, pl, pb, pr) = k, s, pads
    fill = -np.inf if kind[0] == "M" else 0.0
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (pt, pb), (pl, pr), (0, 0)), constant_values=fill)
    inside = np.pad(np.ones(x.shape[1:3]), ((pt, pb), (pl, pr)))
    ho, wo = (xp.shape[1] - kh) // sh + 1, (xp.shape[2] - kw) // sw + 1
    out = np.empty((x.shape[0], ho, wo, x.shape[3]))
    for oy in range(ho):
        for ox in range(wo):
            win = xp[:, oy * sh:oy * sh + kh, ox * sw:ox * sw + kw]
            if kind[0] == "M":
                out[:, oy, ox] = win.max(axis=(1, 2))
            else:
                out[:, oy, ox] = win.sum(axis=(1, 2)) / inside[oy * sh:oy * sh + kh, ox * sw:ox * sw + kw].sum()
    return out
