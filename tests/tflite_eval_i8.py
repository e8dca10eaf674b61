"""Helper (not a test): the NumPy restatement of the full-integer arithmetic of the graph executor (include/cpx.h: "The
full-integer arithmetic"; the TFLite reference integer kernels' as published).  It reads the tflite_reader.Graph only --
nothing of the planner, nothing of the C++ -- and is written from the arithmetic's text: QuantizeMultiplier, SRDHM, RDivPOT,
MBQM, the clamp, and one function per operator.  Integers are int64 arrays that are asserted to stay inside int32 where the
device holds them in int32."""
import math

import numpy as np
import torch
import torch.nn.functional as F

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
INT8 = 9


def round_half_away(v):
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def quantize_multiplier(real):
    f, shift = math.frexp(float(real))
    m = int(round_half_away(f * 2.0 ** 31))
    if m == 2 ** 31:
        m, shift = m // 2, shift + 1
    if shift < -31:
        m, shift = 0, 0
    return m, shift


def _trunc_div(a, b):
    return np.sign(a) * (np.abs(a) // b)


def srdhm(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    ab = a * b
    nudge = np.where(ab >= 0, 2 ** 30, 1 - 2 ** 30)
    out = _trunc_div(ab + nudge, 2 ** 31)
    return np.where((a == I32_MIN) & (b == I32_MIN), I32_MAX, out)


def rdivpot(x, e):
    x, e = np.asarray(x, np.int64), np.asarray(e, np.int64)
    mask = (np.int64(1) << e) - 1
    rem = x & mask
    thr = (mask >> 1) + (x < 0)
    return (x >> e) + (rem > thr)


def mbqm(x, m, shift):
    x, shift = np.asarray(x, np.int64), np.asarray(shift, np.int64)
    left, right = np.maximum(shift, 0), np.maximum(-shift, 0)
    up = x * (np.int64(1) << left)
    assert np.all((up >= I32_MIN) & (up <= I32_MAX)), "x * 2^left leaves int32"
    return rdivpot(srdhm(up, m), right)


def clamp_bounds(act, s_out, z_out):
    if act == 0:
        return -128, 127
    if act == 1:
        return max(-128, z_out), 127
    assert act == 3, act
    return max(-128, z_out), min(127, z_out + int(round_half_away(np.float32(6.0) / np.float32(s_out))))


def quantize_f32(x, s, z):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (x / np.float32(s)).astype(np.float32)
        # roundf, half away from zero: in float64, where |t| + 0.5 is exact for every float32 t below 2^52
        t64 = t.astype(np.float64)
        t = (np.sign(t64) * np.floor(np.abs(t64) + 0.5)).astype(np.float32)
        nan = np.isnan(t)
        t = np.clip(np.where(nan, 0, t), np.float32(-128 - z), np.float32(127 - z))
    return np.where(nan, z, t.astype(np.int64) + z)


def dequantize(q, s, z):
    return (np.float32(s) * (np.asarray(q, np.int64) - z).astype(np.float32)).astype(np.float32)


def requantize(q, s_in, z_in, s_out, z_out, lo=-128, hi=127):
    m, e = quantize_multiplier(float(np.float32(s_in)) / float(np.float32(s_out)))
    return np.clip(z_out + mbqm(np.asarray(q, np.int64) - z_in, m, e), lo, hi)


def add_i8(q1, q2, sign, p1, p2, po, lo, hi):
    (s1, z1), (s2, z2), (so, zo) = [(float(np.float32(s)), z) for s, z in (p1, p2, po)]
    twice = 2.0 * max(s1, s2)
    m1, m2, mo = quantize_multiplier(s1 / twice), quantize_multiplier(s2 / twice), quantize_multiplier(twice / (2.0 ** 20 * so))
    a = mbqm((np.asarray(q1, np.int64) - z1) << 20, *m1)
    b = mbqm((np.asarray(q2, np.int64) - z2) << 20, *m2)
    return np.clip(zo + mbqm(a + sign * b, *mo), lo, hi)


def mul_i8(q1, q2, p1, p2, po, lo, hi):
    (s1, z1), (s2, z2), (so, zo) = [(float(np.float32(s)), z) for s, z in (p1, p2, po)]
    m = quantize_multiplier(s1 * s2 / so)
    return np.clip(zo + mbqm((np.asarray(q1, np.int64) - z1) * (np.asarray(q2, np.int64) - z2), *m), lo, hi)


def round_div(acc, n):
    acc, n = np.asarray(acc, np.int64), np.asarray(n, np.int64)
    return np.where(acc > 0, _trunc_div(acc + n // 2, n), _trunc_div(acc - n // 2, n))


def _pads(size, k, s, padding):
    if padding == 1:
        return 0, 0
    out = (size + s - 1) // s
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def _qp(g, t):
    q = g.tensors[t]["quant"]
    return np.float32(q["scale"][0]), int(q["zero_point"][0])


def _filter_out(g, op, acc, co_axis_scales, x_t, y_t):
    """acc [..., Cout] (int64, bias added) -> the int8 output."""
    s_in, _ = _qp(g, x_t)
    s_out, z_out = _qp(g, y_t)
    sc = np.asarray(co_axis_scales, np.float32).reshape(-1)
    if sc.size == 1:
        sc = np.full(acc.shape[-1], sc[0], np.float32)
    ms = [quantize_multiplier(float(s_in) * float(w) / float(s_out)) for w in sc]
    assert np.all(np.abs(acc) < 2 ** 31)
    lo, hi = clamp_bounds(op.get("act", 0), s_out, z_out)
    return np.clip(z_out + mbqm(acc, np.array([m for m, _ in ms], np.int64), np.array([e for _, e in ms], np.int64)), lo, hi)


def evaluate(g, x_nhwc):
    """-> {tensor id: array}: int64 for an INT8 tensor (its quantised values), float32 for a float32 one."""
    val = {g.inputs[0]: np.asarray(x_nhwc, np.float32)}

    def i8(t):
        return g.tensors[t]["type"] == INT8

    for op in g.ops:
        name, ins = op["name"], [t for t in op["inputs"] if t >= 0]
        y = op["outputs"][0]
        a = val.get(ins[0])
        if name == "QUANTIZE":
            s, z = _qp(g, y)
            r = requantize(a, *_qp(g, ins[0]), s, z) if i8(ins[0]) else quantize_f32(a, s, z)
        elif name == "DEQUANTIZE":
            r = dequantize(a, *_qp(g, ins[0]))
        elif not i8(y):
            if name == "SOFTMAX":
                e = np.exp(op.get("beta", 1.0) * (a.astype(np.float64) - a.astype(np.float64).max(axis=-1, keepdims=True)))
                r = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
            elif name == "LOGISTIC":
                r = (1.0 / (1.0 + np.exp(-a.astype(np.float64)))).astype(np.float32)
            else:
                raise NotImplementedError("float32 %s" % name)
        elif name in ("CONV_2D", "DEPTHWISE_CONV_2D"):
            dw = name == "DEPTHWISE_CONV_2D"
            wt = g.tensors[ins[1]]
            w = np.asarray(wt["const"], np.int64)
            _, z_in = _qp(g, ins[0])
            kh, kw = w.shape[1], w.shape[2]
            sh, sw = op.get("stride_h", 1), op.get("stride_w", 1)
            pt, pb = _pads(a.shape[1], kh, sh, op.get("padding", 0))
            pl, pr = _pads(a.shape[2], kw, sw, op.get("padding", 0))
            # (q - z_in) with zeros around it: a padded tap contributes nothing.  float64 holds every sum exactly (< 2^31)
            xin = F.pad(torch.from_numpy((a - z_in).astype(np.float64)).permute(0, 3, 1, 2), (pl, pr, pt, pb))
            if dw:
                wk = torch.from_numpy(w.astype(np.float64)).permute(3, 0, 1, 2)   # [C, 1, kh, kw]
                acc = F.conv2d(xin, wk, stride=(sh, sw), groups=a.shape[3])
            else:
                wk = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)
                acc = F.conv2d(xin, wk, stride=(sh, sw), groups=a.shape[3] // w.shape[3])
            acc = acc.permute(0, 2, 3, 1).numpy().astype(np.int64)
            if len(ins) > 2:
                acc = acc + np.asarray(g.const(ins[2]), np.int64)
            r = _filter_out(g, op, acc, wt["quant"]["scale"], ins[0], y)
        elif name == "FULLY_CONNECTED":
            wt = g.tensors[ins[1]]
            _, z_in = _qp(g, ins[0])
            acc = (a.reshape(a.shape[0], -1) - z_in) @ np.asarray(wt["const"], np.int64).T
            if len(ins) > 2:
                acc = acc + np.asarray(g.const(ins[2]), np.int64)
            r = _filter_out(g, op, acc, wt["quant"]["scale"], ins[0], y)
        elif name in ("ADD", "SUB", "MUL"):
            first_const = g.const(ins[0]) is not None
            assert not (first_const and name == "SUB")
            ta, tb_ = (ins[1], ins[0]) if first_const else (ins[0], ins[1])
            qa = val[ta]
            qb = val[tb_] if tb_ in val else np.asarray(g.const(tb_), np.int64)
            s_out, z_out = _qp(g, y)
            lo, hi = clamp_bounds(op.get("act", 0), s_out, z_out)
            if name == "MUL":
                r = mul_i8(qa, qb, _qp(g, ta), _qp(g, tb_), (s_out, z_out), lo, hi)
            else:
                r = add_i8(qa, qb, 1 if name == "ADD" else -1, _qp(g, ta), _qp(g, tb_), (s_out, z_out), lo, hi)
        elif name in ("RELU", "RELU6"):
            s_out, z_out = _qp(g, y)
            lo, hi = clamp_bounds(1 if name == "RELU" else 3, s_out, z_out)
            r = requantize(a, *_qp(g, ins[0]), s_out, z_out, lo, hi)
        elif name in ("MAX_POOL_2D", "AVERAGE_POOL_2D"):
            assert _qp(g, ins[0]) == _qp(g, y)
            kh, kw, sh, sw = op["filter_height"], op["filter_width"], op["stride_h"], op["stride_w"]
            pt, _ = _pads(a.shape[1], kh, sh, op["padding"])
            pl, _ = _pads(a.shape[2], kw, sw, op["padding"])
            ho = -(-a.shape[1] // sh) if op["padding"] == 0 else (a.shape[1] - kh) // sh + 1
            wo = -(-a.shape[2] // sw) if op["padding"] == 0 else (a.shape[2] - kw) // sw + 1
            lo, hi = clamp_bounds(op.get("act", 0), *_qp(g, y))
            r = np.zeros((a.shape[0], ho, wo, a.shape[3]), np.int64)
            for oy in range(ho):
                for ox in range(wo):
                    y0, y1 = max(oy * sh - pt, 0), min(oy * sh - pt + kh, a.shape[1])
                    x0, x1 = max(ox * sw - pl, 0), min(ox * sw - pl + kw, a.shape[2])
                    win = a[:, y0:y1, x0:x1, :].reshape(a.shape[0], -1, a.shape[3])
                    r[:, oy, ox, :] = win.max(axis=1) if name[0] == "M" else round_div(win.sum(axis=1), win.shape[1])
            r = np.clip(r, lo, hi)
        elif name == "MEAN":
            assert sorted(v % 4 for v in op["axes"]) == [1, 2]
            s_in, z_in = _qp(g, ins[0])
            s_out, z_out = _qp(g, y)
            n = a.shape[1] * a.shape[2]
            acc = mbqm(a.sum(axis=(1, 2)), *quantize_multiplier(float(s_in) / float(s_out)))
            bias = z_out - int(np.float32(np.float32(np.float32(z_in) * s_in) / s_out))
            r = np.clip(round_div(acc, n) + bias, -128, 127)
            if op["keep_dims"]:
                r = r[:, None, None, :]
        elif name == "CONCATENATION":
            assert all(_qp(g, t) == _qp(g, y) for t in ins)
            r = np.concatenate([val[t] for t in ins], axis=op.get("axis", 0))
        elif name == "RESHAPE":
            assert _qp(g, ins[0]) == _qp(g, y)
            shp = [int(v) for v in (g.const(ins[1]) if len(ins) > 1 else op["new_shape"])]
            r = a.reshape([a.shape[0]] + shp[1:])
        elif name == "PAD":
            assert _qp(g, ins[0]) == _qp(g, y)
            (_, _), (t0, t1), (l0, l1), (_, _) = op["paddings"]
            r = np.pad(a, ((0, 0), (t0, t1), (l0, l1), (0, 0)), constant_values=_qp(g, y)[1])
        elif name in ("STRIDED_SLICE", "SLICE"):
            assert _qp(g, ins[0]) == _qp(g, y)
            (_, (y0, sh, ho), (x0, sw, wo), _) = op["slice"]
            r = a[:, y0:y0 + sh * ho:sh, x0:x0 + sw * wo:sw, :]
        elif name in ("SOFTMAX", "LOGISTIC"):
            # the issue's statement of the int8 head: a float64 function of the dequantised input, rounded half away
            xf = dequantize(a, *_qp(g, ins[0])).astype(np.float64)
            if name == "SOFTMAX":
                e = np.exp(op.get("beta", 1.0) * (xf - xf.max(axis=-1, keepdims=True)))
                p = e / e.sum(axis=-1, keepdims=True)
            else:
                p = 1.0 / (1.0 + np.exp(-xf))
            s_out, z_out = _qp(g, y)
            r = np.clip(round_half_away(p / float(s_out)) + z_out, -128, 127)
        else:
            raise NotImplementedError(name)
        val[y] = np.ascontiguousarray(r)
    return val
