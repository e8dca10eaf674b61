"""The full-integer half of the graph planner (cpx/ml_tools/tflite_graph.py: build_plan(..., integer_activations=True)): the
operators of a file converted with a representative dataset -- INT8 activations with one scale and one zero point, INT32
biases, per-channel INT8 filters, QUANTIZE / DEQUANTIZE at the two ends -- lowered to the executor's int8 kinds
(include/cpx.h: CPX_GRAPH_QUANTIZE .. CPX_GRAPH_LUT_I8, and SLICE on bytes).  The arithmetic is the TFLite reference
integer kernels' as published, fixed in include/cpx.h; parity with a TFLite runtime is not pinned.  Everything an operator
needs beyond its filter is worked out HERE, in float64 from the float32 scales widened to double, and rides as integers:
the int32 header (`shift`: zero points, clamp, multipliers and shifts) and, for the filter kinds, int32 M[c], shift[c],
bias[c] per output channel (`scale`).  With integer_lut an interior LOGISTIC or swish is a 256-entry table made here too
(logistic_table, swish_table), which rides behind the header.  What cannot be run is refused by the operator's name and
index."""
import math

import numpy as np

from .. import _lib
from .tflite_reader import ACT_NONE, ACT_RELU, ACT_RELU6, SLICE_OPS, resolve_slice

INT8 = 9
ADD_LEFT = 20   # ADD_I8 / SUB: the operands are shifted up by this many bits before they are rescaled


def round_half_away(v):
    return int(math.floor(abs(v) + 0.5)) * (-1 if v < 0 else 1)


def quantize_multiplier(real):
    """real (a float64) -> (M, shift) with real ~ M * 2^(shift - 31): (f, shift) = frexp(real), M = round-half-away(f * 2^31);
    M == 2^31: M /= 2, shift += 1; shift < -31: (0, 0)."""
    f, shift = math.frexp(float(real))
    m = round_half_away(f * 2.0 ** 31)
    if m == 2 ** 31:
        m //= 2
        shift += 1
    if shift < -31:
        m, shift = 0, 0
    return m, shift


def qparams(g, tid):
    """-> (float32 scale, int zero point) of an INT8 tensor of the flatbuffer."""
    q = g.tensors[tid]["quant"]
    return np.float32(q["scale"][0]), int(q["zero_point"][0])


def is_int8(g, tid):
    return g.tensors[tid]["type"] == INT8


def _multiplier(what, real, worst, below_one=False):
    """QM(real) for an operator whose input magnitude is at most `worst`; the refusals of the issue's arithmetic."""
    if not (real > 0.0) or not math.isfinite(real):
        raise NotImplementedError("%s: a scale that is not above 0 (multiplier %r)" % (what, real))
    m, shift = quantize_multiplier(real)
    if shift > 30:
        raise NotImplementedError("%s: the multiplier %r needs a left shift of %d bits, above 30" % (what, real, shift))
    if below_one and shift > 0:
        raise NotImplementedError("%s: the multiplier %r must be below 1" % (what, real))
    if worst * 2 ** max(shift, 0) >= 2 ** 31:
        raise NotImplementedError("%s: a value of up to %d shifted left by %d bits could overflow int32" % (what, worst, max(shift, 0)))
    return m, shift


def clamp_of(act, s_out, z_out, what):
    """The clamp [lo, hi] that carries a fused activation."""
    if act == ACT_NONE:
        return -128, 127
    if act == ACT_RELU:
        return max(-128, z_out), 127
    if act == ACT_RELU6:
        return max(-128, z_out), min(127, z_out + round_half_away(float(np.float32(6.0) / np.float32(s_out))))
    raise NotImplementedError("%s: fused activation %d" % (what, act))


def header(**fields):
    """The int32 header of a full-integer operator (include/cpx.h: CPX_GRAPH_I8_HDR_*), as the bytes that are uploaded."""
    h = np.zeros(_lib.GRAPH_I8_HDR_WORDS, np.int32)
    for k, v in fields.items():
        h[getattr(_lib, "GRAPH_I8_HDR_" + k.upper())] = v
    return h.view(np.uint8)


def unpack_header(b):
    return np.asarray(b, np.uint8).view(np.int32)


def _mbqm(x, m, shift):
    """MBQM on Python integers (include/cpx.h): SRDHM by m, then the rounding division by 2^max(-shift, 0)."""
    x <<= max(shift, 0)
    if x == m == -2 ** 31:
        v = 2 ** 31 - 1
    else:
        ab = x * m
        ab += 2 ** 30 if ab >= 0 else 1 - 2 ** 30
        v = abs(ab) // 2 ** 31 * (-1 if ab < 0 else 1)   # C's division: it truncates
    e = max(-shift, 0)
    mask = (1 << e) - 1
    return (v >> e) + (1 if (v & mask) > (mask >> 1) + (1 if v < 0 else 0) else 0)


def logistic_table(s_in, z_in, s_out, z_out):
    """The 256 bytes of an INT8 LOGISTIC (include/cpx.h, "Tables"), entry q + 128 for q = -128 .. 127: the float64 logistic
    of the dequantised input float32(s_in) * float32(q - z_in), divided by float64(s_out), rounded half away, + z_out,
    clamped."""
    q = np.arange(-128, 128)
    x = (np.float32(s_in) * (q - int(z_in)).astype(np.float32)).astype(np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        t = (1.0 / (1.0 + np.exp(-x))) / float(np.float32(s_out))
    r = (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int64)
    return np.clip(r + int(z_out), -128, 127).astype(np.int8)


def swish_table(x_qp, l_qp, out_qp, act, what="MUL"):
    """The 256 bytes of y = MUL(x, LOGISTIC(x)): S[q + 128] = MUL_I8(q, L[q + 128]) with the MUL's own constants -- the zero
    points of x and of the LOGISTIC's output, QM(s_x * s_l / s_out), and the clamp of its fused activation `act`."""
    (s_x, z_x), (s_l, z_l), (s_out, z_out) = x_qp, l_qp, out_qp
    if not (float(s_x) > 0.0 and float(s_l) > 0.0 and float(s_out) > 0.0):
        raise NotImplementedError("%s: a scale that is not above 0" % what)
    L = logistic_table(s_x, z_x, s_l, z_l)
    m, e = _multiplier(what, float(s_x) * float(s_l) / float(s_out), 255 * 255)
    lo, hi = clamp_of(act, s_out, z_out, what)
    return np.array([min(max(z_out + _mbqm((q - z_x) * (int(L[q + 128]) - z_l), m, e), lo), hi) for q in range(-128, 128)], np.int8)


def with_table(hdr, table):
    """The header with the 256-entry table behind it: what `shift` points at for LUT_I8 and for an operator with the
    activation LUT (include/cpx.h: CPX_GRAPH_I8_LUT_BYTES)."""
    out = np.concatenate([np.asarray(hdr, np.uint8)[:4 * _lib.GRAPH_I8_HDR_WORDS], np.asarray(table, np.int8).view(np.uint8)])
    assert out.size == _lib.GRAPH_I8_LUT_BYTES, out.size
    return out


def table_of(shift):
    """-> the int8 table behind a header made by with_table."""
    return np.asarray(shift, np.uint8)[4 * _lib.GRAPH_I8_HDR_WORDS:].view(np.int8)


def _emit_table(s, i, x, y, table, name, readers):
    """y = T[x]: folded into x's producer as the activation LUT where _fold_into_producer allows it (a kind of KINDS' table
    column that carries no table yet; x an own tensor with exactly `readers` readers, not the output), else ONE LUT_I8
    launch x -> y."""
    from .tflite_graph import LUT_INTO, PlanOp, _fold_into_producer

    if _fold_into_producer(s, x, y, LUT_INTO, name, _lib.GRAPH_ACT_LUT, readers=readers):
        p = s.producer[y]
        p.shift = with_table(p.shift, table)
    else:
        s.emit(PlanOp(_lib.GRAPH_LUT_I8, name, x.id, y, shift=with_table(header(), table)), i)


def lower_integer_swish(s, i, mul, logistic, x, y, what):
    """integer_lut: the swish y = MUL(x, LOGISTIC(x)) (tflite_graph._find_swishes) on INT8 tensors as one table of x."""
    from .tflite_graph import PlanTensor

    g = s.g
    if not all(is_int8(g, t) for t in (x.id, y, logistic["outputs"][0])):
        raise NotImplementedError("%s mixes INT8 and float32 activations: only QUANTIZE and DEQUANTIZE change the type" % what)
    table = swish_table(qparams(g, x.id), qparams(g, logistic["outputs"][0]), qparams(g, y), mul.get("act", 0), what)
    s.T[y] = PlanTensor(y, x.H, x.W, x.C)
    _emit_table(s, i, x, y, table, "SWISH", 2)


def per_channel(m, shift, bias):
    """int32 [3][C]: M[c], shift[c], bias[c] of a filter kind, as bytes."""
    return np.ascontiguousarray(np.stack([np.asarray(m, np.int64), np.asarray(shift, np.int64), np.asarray(bias, np.int64)])
                                .astype(np.int32)).reshape(-1).view(np.uint8)


def _filter(s, what, op, ins, cout_dim):
    """-> (int8 filter, float32 scales per output channel) of a full-integer filter operator."""
    ten = s.g.quantised_filter(op)
    if ten is None:
        raise NotImplementedError("%s: a filter that is not an INT8 constant on INT8 activations" % what)
    sc = np.asarray(ten["quant"]["scale"], np.float32).reshape(-1)
    channels = ten["shape"][cout_dim]
    return ten["const"], (np.full(channels, sc[0], np.float32) if sc.size == 1 else sc)


def _filter_constants(s, what, ins, x_id, y, fscale, k_products, act):
    """The header and the per-channel integers of CONV_I8 / DWCONV_I8 / FC_I8: (M, shift)[c] = QM(s_in * s_w[c] / s_out) in
    float64, the bias the file's INT32 tensor as it is (or 0); K * 255 * 127 + max |bias| stays below 2^31."""
    g = s.g
    s_in, z_in = qparams(g, x_id)
    s_out, z_out = qparams(g, y)
    co = fscale.size
    bias = g.const(ins[2]) if len(ins) > 2 else None
    if bias is not None and (g.tensors[ins[2]]["type"] != 2 or bias.size != co):
        raise NotImplementedError("%s: the bias of a full-integer operator is an INT32 tensor of %d values" % (what, co))
    bias = np.zeros(co, np.int64) if bias is None else np.asarray(bias, np.int64).reshape(-1)
    worst = k_products * 255 * 127 + int(np.abs(bias).max(initial=0))
    if worst >= 2 ** 31:
        raise NotImplementedError("%s: %d products of an 8-bit activation and an INT8 weight and the bias could overflow the "
                                  "int32 accumulator" % (what, k_products))
    if not float(s_out) > 0.0:
        raise NotImplementedError("%s: a scale that is not above 0" % what)
    ms = [_multiplier(what, float(s_in) * float(fscale[c]) / float(s_out), worst) for c in range(co)]
    lo, hi = clamp_of(act, s_out, z_out, what)
    return header(z_in=z_in, z_out=z_out, lo=lo, hi=hi), per_channel([m for m, _ in ms], [e for _, e in ms], bias)


def _same_params(s, what, a, b, why):
    if qparams(s.g, a) != qparams(s.g, b):
        raise NotImplementedError("%s: %s carry different quantisation parameters (%s against %s)"
                                  % (what, why, qparams(s.g, a), qparams(s.g, b)))


def _requantize(s, i, name, x, y, act, what, PlanOp):
    s_in, z_in = qparams(s.g, x.id)
    s_out, z_out = qparams(s.g, y)
    if not float(s_out) > 0.0:
        raise NotImplementedError("%s: a scale that is not above 0" % what)
    m, e = _multiplier(what, float(s_in) / float(s_out), 255)
    lo, hi = clamp_of(act, s_out, z_out, what)
    s.emit(PlanOp(_lib.GRAPH_QUANTIZE, name, x.id, y, shift=header(z_in=z_in, z_out=z_out, m0=m, s0=e, lo=lo, hi=hi)), i)


def lower_integer_op(s, i, op, what, x, y, ins, act_ins, grouped_convolutions, integer_gate_mul=False, integer_lut=False):
    """One operator of the flatbuffer that reads or writes INT8 activations -> its PlanOps (tflite_graph.lower_ops calls this
    for such an operator).  -> False for the operators whose float32 lowering serves unchanged (RESHAPE: a view;
    CONCATENATION: a placement, once the parameters are checked).  integer_gate_mul: a MUL by the [1, 1, C] gate of a
    squeeze-and-excite block is MUL_I8 with the gate as in1; integer_lut: an interior LOGISTIC is a table (_emit_table)."""
    from .tflite_graph import PlanOp, PlanTensor, slice_pads, window

    g, T, name = s.g, s.T, op["name"]
    act = op.get("act", 0)
    if name == "QUANTIZE":
        T[y] = PlanTensor(y, x.H, x.W, x.C)
        if not is_int8(g, y):
            raise NotImplementedError("%s: the output is not INT8" % what)
        s_out, z_out = qparams(g, y)
        if is_int8(g, x.id):
            _requantize(s, i, name, x, y, ACT_NONE, what, PlanOp)
        else:
            if not float(s_out) > 0.0:
                raise NotImplementedError("%s: a scale that is not above 0" % what)
            s.emit(PlanOp(_lib.GRAPH_QUANTIZE, name, x.id, y, param=float(s_out), shift=header(z_out=z_out)), i)
        return True
    if name == "DEQUANTIZE":
        if not is_int8(g, x.id) or g.tensors[y]["type"] != 0:
            raise NotImplementedError("%s: only INT8 to float32 is run" % what)
        s_in, z_in = qparams(g, x.id)
        if not float(s_in) > 0.0:
            raise NotImplementedError("%s: a scale that is not above 0" % what)
        T[y] = PlanTensor(y, x.H, x.W, x.C)
        s.emit(PlanOp(_lib.GRAPH_DEQUANTIZE, name, x.id, y, param=float(s_in), shift=header(z_in=z_in)), i)
        return True
    if any(not is_int8(g, t) for t in act_ins) or not is_int8(g, y):
        raise NotImplementedError("%s mixes INT8 and float32 activations: only QUANTIZE and DEQUANTIZE change the type" % what)
    if name == "RESHAPE":
        _same_params(s, what, x.id, y, "input and output")
        return False
    if name == "CONCATENATION":
        for t in act_ins:
            _same_params(s, what, t, y, "an input and the output")
        if act != ACT_NONE:
            raise NotImplementedError("%s with a fused activation on INT8 tensors" % what)
        return False
    if name in ("RELU", "RELU6"):
        T[y] = PlanTensor(y, x.H, x.W, x.C)
        _requantize(s, i, name, x, y, ACT_RELU if name == "RELU" else ACT_RELU6, what, PlanOp)
        return True
    if name in ("CONV_2D", "DEPTHWISE_CONV_2D"):
        dw = name == "DEPTHWISE_CONV_2D"
        w, fscale = _filter(s, what, op, ins, 3 if dw else 0)
        kh, kw, depth = w.shape[1:]
        co = depth if dw else w.shape[0]
        groups = 1
        if depth != x.C:
            if dw or not grouped_convolutions:
                raise NotImplementedError(("%s: depth multiplier (filter depth %d, input depth %d), only 1 is run" if dw else
                                           "%s: grouped convolution (filter depth %d, input depth %d)") % (what, depth, x.C))
            if depth < 1 or x.C % depth != 0 or co % (x.C // depth) != 0:
                raise NotImplementedError("%s: grouped convolution whose filter depth %d and %d output channels do not divide "
                                          "by the groups of the input depth %d" % (what, depth, co, x.C))
            groups = x.C // depth
        sh, sw = op.get("stride_h", 1), op.get("stride_w", 1)
        strides = (1, 2, 3) if groups > 1 else (1, 2)
        if not (1 <= kh <= 7 and 1 <= kw <= 7 and sh in strides and sw in strides):
            raise NotImplementedError("%s: %d x %d kernel with strides %d, %d" % (what, kh, kw, sh, sw))
        ho, pt, pb = window(x.H, kh, sh, op.get("padding", 0))
        wo, pl, pr = window(x.W, kw, sw, op.get("padding", 0))
        if ho < 1 or wo < 1:
            raise NotImplementedError("%s: the %d x %d input is smaller than the kernel" % (what, x.H, x.W))
        T[y] = PlanTensor(y, ho, wo, co)
        hdr, prm = _filter_constants(s, what, ins, x.id, y, fscale, kh * kw * (1 if dw else depth), act)
        kind = _lib.GRAPH_DWCONV_I8 if dw else _lib.GRAPH_CONV_I8_GROUPED if groups > 1 else _lib.GRAPH_CONV_I8
        s.emit(PlanOp(kind, name, x.id, y, kh=kh, kw=kw, stride_h=sh, stride_w=sw, pads=(pt, pl, pb, pr), groups=groups,
                      filter=w, filter_scale=fscale, scale=prm, shift=hdr), i)
        return True
    if name == "FULLY_CONNECTED":
        w, fscale = _filter(s, what, op, ins, 0)
        if x.H != 1 or x.W != 1 or w.ndim != 2 or w.shape[1] != x.C:
            raise NotImplementedError("%s: weights %s on a %d x %d x %d input" % (what, list(w.shape), x.H, x.W, x.C))
        T[y] = PlanTensor(y, 1, 1, w.shape[0])
        hdr, prm = _filter_constants(s, what, ins, x.id, y, fscale, w.shape[1], act)
        s.emit(PlanOp(_lib.GRAPH_FC_I8, name, x.id, y, filter=w, filter_scale=fscale, scale=prm, shift=hdr), i)
        return True
    if name in ("ADD", "SUB", "MUL"):
        s1, z1 = qparams(g, x.id)
        s_out, z_out = qparams(g, y)
        konst = None
        if len(act_ins) == 2:
            b = T[act_ins[1]]
            if (x.H, x.W, x.C) != (b.H, b.W, b.C):
                if not integer_gate_mul:
                    raise NotImplementedError("%s of two INT8 tensors of shapes %s, %s: only one shape is run (a [1, 1, C] gate "
                                              "is not); build_plan(integer_gate_mul=True) plans a MUL by such a gate as MUL_I8"
                                              % (what, (x.H, x.W, x.C), (b.H, b.W, b.C)))
                # [H, W, C] by the [1, 1, C] gate of its sample, in either order: the gate is in1
                if name == "MUL" and (x.H, x.W, x.C) == (1, 1, b.C):
                    x, b = b, x
                if name != "MUL" or (b.H, b.W, b.C) != (1, 1, x.C):
                    raise NotImplementedError("%s of two INT8 tensors of shapes %s, %s: only one shape, or for a MUL [H, W, C] "
                                              "by [1, 1, C]" % (what, (T[act_ins[0]].H, T[act_ins[0]].W, T[act_ins[0]].C),
                                                                (T[act_ins[1]].H, T[act_ins[1]].W, T[act_ins[1]].C)))
                s1, z1 = qparams(g, x.id)
            s2, z2 = qparams(g, b.id)
            in1 = b.id
        else:
            cid = next(t for t in ins if g.const(t) is not None)
            if not is_int8(g, cid):
                raise NotImplementedError("%s: the constant operand of an INT8 operator is not INT8" % what)
            if ins[0] == cid and name == "SUB":
                raise NotImplementedError("%s: a constant minus an INT8 activation (c - x) is not run" % what)
            c = np.asarray(g.const(cid))
            konst = np.full(x.C, c.reshape(-1)[0], np.int8) if c.size == 1 else c.reshape(-1).astype(np.int8)
            if konst.size != x.C or (c.ndim > 1 and c.shape[-1] != c.size):
                raise NotImplementedError("%s: a constant of shape %s against %d channels" % (what, list(c.shape), x.C))
            s2, z2 = qparams(g, cid)
            in1 = -1
        if not (float(s1) > 0.0 and float(s2) > 0.0 and float(s_out) > 0.0):
            raise NotImplementedError("%s: a scale that is not above 0" % what)
        lo, hi = clamp_of(act, s_out, z_out, what)
        T[y] = PlanTensor(y, x.H, x.W, x.C)
        if name == "MUL":
            m, e = _multiplier(what, float(s1) * float(s2) / float(s_out), 255 * 255)
            hdr = header(z_in=z1, z_in1=z2, z_out=z_out, lo=lo, hi=hi, m0=m, s0=e)
            kind, param = _lib.GRAPH_MUL_I8, 0.0
        else:
            twice = 2.0 * max(float(s1), float(s2))
            m1, e1 = _multiplier(what, float(s1) / twice, 255 << ADD_LEFT, below_one=True)
            m2, e2 = _multiplier(what, float(s2) / twice, 255 << ADD_LEFT, below_one=True)
            mo, eo = _multiplier(what, twice / (2.0 ** ADD_LEFT * float(s_out)), 2 * (255 << ADD_LEFT), below_one=True)
            hdr = header(z_in=z1, z_in1=z2, z_out=z_out, lo=lo, hi=hi, m0=m1, s0=e1, m1=m2, s1=e2, mo=mo, so=eo, left=ADD_LEFT)
            kind, param = _lib.GRAPH_ADD_I8, (1.0 if name == "ADD" else -1.0)
        s.emit(PlanOp(kind, name, x.id, y, in1=in1, param=param, shift=hdr,
                      weights=None if konst is None else np.ascontiguousarray(konst).view(np.uint8)), i)
        return True
    if name in ("MAX_POOL_2D", "AVERAGE_POOL_2D"):
        _same_params(s, what, x.id, y, "input and output")
        kh, kw = op["filter_height"], op["filter_width"]
        sh, sw = op["stride_h"], op["stride_w"]
        if not (1 <= kh <= 7 and 1 <= kw <= 7 and 1 <= sh <= 7 and 1 <= sw <= 7):
            raise NotImplementedError("%s: %d x %d window with strides %d, %d" % (what, kh, kw, sh, sw))
        ho, pt, pb = window(x.H, kh, sh, op["padding"])
        wo, pl, pr = window(x.W, kw, sw, op["padding"])
        if ho < 1 or wo < 1:
            raise NotImplementedError("%s: the %d x %d input is smaller than the window" % (what, x.H, x.W))
        s_out, z_out = qparams(g, y)
        lo, hi = clamp_of(act, s_out, z_out, what)
        T[y] = PlanTensor(y, ho, wo, x.C)
        s.emit(PlanOp(_lib.GRAPH_MAX_POOL_I8 if name[0] == "M" else _lib.GRAPH_AVG_POOL_I8, name, x.id, y, kh=kh, kw=kw,
                      stride_h=sh, stride_w=sw, pads=(pt, pl, pb, pr), shift=header(z_in=z_out, z_out=z_out, lo=lo, hi=hi)), i)
        return True
    if name == "MEAN":
        axes = sorted(a % 4 for a in op["axes"])
        if axes != [1, 2]:
            raise NotImplementedError("%s over axes %s: only H and W (global average pooling)" % (what, op["axes"]))
        s_in, z_in = qparams(g, x.id)
        s_out, z_out = qparams(g, y)
        if not (float(s_in) > 0.0 and float(s_out) > 0.0):
            raise NotImplementedError("%s: a scale that is not above 0" % what)
        m, e = _multiplier(what, float(s_in) / float(s_out), 128 * x.H * x.W)
        bias = z_out - int(np.float32(np.float32(np.float32(z_in) * s_in) / s_out))
        T[y] = PlanTensor(y, 1, 1, x.C)
        s.emit(PlanOp(_lib.GRAPH_MEAN_I8, name, x.id, y, shift=header(z_in=z_in, z_out=z_out, m0=m, s0=e, left=bias, lo=-128, hi=127)), i)
        return True
    if name == "PAD" or name in SLICE_OPS:
        _same_params(s, what, x.id, y, "input and output")
        _, z = qparams(g, y)
        if name == "PAD":
            pd = op["paddings"]
            if len(pd) != 4 or pd[0] != [0, 0] or pd[3] != [0, 0] or min(min(p) for p in pd) < 0:
                raise NotImplementedError("%s with paddings %s: only H and W are padded" % (what, pd))
            T[y] = PlanTensor(y, x.H + pd[1][0] + pd[1][1], x.W + pd[2][0] + pd[2][1], x.C)
            # (a PAD until the window folds have run: one that is left is made a SLICE by finish_pads)
            s.emit(PlanOp(_lib.GRAPH_PAD, name, x.id, y, pads=(pd[1][0], pd[2][0], pd[1][1], pd[2][1]), shift=header(z_in=z)), i)
        else:
            (_, (y0, sh, ho), (x0, sw, wo), _) = resolve_slice(op, (1, x.H, x.W, x.C), what)
            if sh > 7 or sw > 7:
                raise NotImplementedError("%s: strides %d, %d, only 1 to 7 are run" % (what, sh, sw))
            T[y] = PlanTensor(y, ho, wo, x.C)
            s.emit(PlanOp(_lib.GRAPH_SLICE, name, x.id, y, stride_h=sh, stride_w=sw,
                          pads=slice_pads(x.H, x.W, ho, wo, sh, sw, -y0, -x0), shift=header(z_in=z)), i)
        return True
    if name in ("SOFTMAX", "LOGISTIC"):
        s_in, z_in = qparams(g, x.id)
        s_out, z_out = qparams(g, y)
        if not (float(s_in) > 0.0 and float(s_out) > 0.0):
            raise NotImplementedError("%s: a scale that is not above 0" % what)
        # integer_lut: an interior LOGISTIC (the gate's sigmoid; a swish's that could not be taken whole) is its table.  The
        # head -- a DEQUANTIZE among the readers -- stays as below
        if integer_lut and name == "LOGISTIC" and not any(g.ops[r]["name"] == "DEQUANTIZE" for r in s.consumers.get(y, [])):
            T[y] = PlanTensor(y, x.H, x.W, x.C)
            _emit_table(s, i, x, y, logistic_table(s_in, z_in, s_out, z_out), "LOGISTIC", 1)
            return True
        # DEQUANTIZE -> the float32 kernel -> QUANTIZE: three launches on a [N, labels] tensor.  The TFLite runtime's
        # fixed-point tables may differ from it by a step
        t0, t1 = ("float", y, 0), ("float", y, 1)
        T[t0], T[t1], T[y] = PlanTensor(t0, x.H, x.W, x.C), PlanTensor(t1, x.H, x.W, x.C), PlanTensor(y, x.H, x.W, x.C)
        s.emit(PlanOp(_lib.GRAPH_DEQUANTIZE, "DEQUANTIZE", x.id, t0, param=float(s_in), shift=header(z_in=z_in)), i)
        s.emit(PlanOp(_lib.GRAPH_LOGISTIC if name == "LOGISTIC" else _lib.GRAPH_SOFTMAX, name, t0, t1,
                      param=float(op.get("beta", 1.0))), i)
        s.emit(PlanOp(_lib.GRAPH_QUANTIZE, "QUANTIZE", t1, y, param=float(s_out), shift=header(z_out=z_out)), i)
        return True
    raise NotImplementedError("%s is not run on INT8 activations" % what)


def annotate_types(s):
    """Every tensor of the plan that is an INT8 tensor of the flatbuffer (or a slice of one: a concatenation's copy) gets
    its dtype, scale and zero point."""
    g = s.g
    for key, t in s.T.items():
        tid = key if isinstance(key, (int, np.integer)) else key[0] if isinstance(key, tuple) and isinstance(key[0], (int, np.integer)) else None
        if tid is not None and is_int8(g, tid):
            t.dtype = "int8"
            t.scale, t.zero_point = qparams(g, tid)


def finish_pads(s):
    """Behind the window folds: a PAD of an int8 tensor that is still a launch is a SLICE on bytes with the zero point as
    its fill (include/cpx.h: CPX_GRAPH_SLICE)."""
    from .tflite_graph import slice_pads

    for o in s.ops:
        if o.kind == _lib.GRAPH_PAD and s.T[o.in0].dtype == "int8":
            a, y = s.T[o.in0], s.T[o.out]
            o.kind, o.pads = _lib.GRAPH_SLICE, slice_pads(a.H, a.W, y.H, y.W, 1, 1, o.pads[0], o.pads[1])
