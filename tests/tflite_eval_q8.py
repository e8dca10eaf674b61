"""Helper (not a test): the hybrid arithmetic of a dynamic-range quantised graph (include/cpx.h, CPX_GRAPH_QUANT_PARAMS /
CONV_Q8 / FC_Q8) restated operator by operator in NumPy / PyTorch-CPU.  It reads the tflite_reader.Graph only -- nothing
of cpx/ml_tools/tflite_graph.py.  Integer sums are float64 convolutions (every term is an integer far below 2^53: exact);
round-half-away is done in float64 on the float32 product.  The other operators are tflite_eval's, in float32, one
operator at a time.  `evaluate_dequantised` evaluates the same graph with the filters multiplied out (int8 x scale), in
float64 by default: the model the quantised file stands for."""
import numpy as np
import torch
import torch.nn.functional as F

import tflite_eval as te


def round_half_away(v):
    v = np.asarray(v, np.float64)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def quant_params(x, symmetric=False):
    """x: float32 [N, ...] -> (sx float32 [N], inv float32 [N], zp int64 [N]), per sample."""
    x = np.asarray(x, np.float32)
    flat = x.reshape(x.shape[0], -1)
    rmin = np.minimum(np.float32(0), flat.min(axis=1))
    rmax = np.maximum(np.float32(0), flat.max(axis=1))
    sx, inv, zp = np.ones(len(flat), np.float32), np.ones(len(flat), np.float32), np.zeros(len(flat), np.int64)
    for n in range(len(flat)):
        lo, hi = np.float64(rmin[n]), np.float64(rmax[n])
        if symmetric:
            m = max(-lo, hi)
            if m != 0:
                sx[n], inv[n] = np.float32(m / 127.0), np.float32(127.0 / m)
        elif lo != hi:
            s = (hi - lo) / 255.0
            a, b = -128.0 - lo / s, 127.0 - hi / s
            z = a if 128.0 + abs(lo / s) < 127.0 + abs(hi / s) else b
            zp[n] = int(min(max(round_half_away(z), -128.0), 127.0))
            sx[n], inv[n] = np.float32(s), np.float32(1.0 / s)
    return sx, inv, zp


def quantise_input(x, inv, zp):
    """q = clamp(round-half-away(float32(x * inv)) + zp, -128, 127), float64 [N, ...] of integers."""
    x = np.asarray(x, np.float32)
    shape = (-1,) + (1,) * (x.ndim - 1)
    prod = (x * inv.reshape(shape)).astype(np.float32)   # ONE float32 multiply
    return np.clip(round_half_away(prod) + zp.reshape(shape).astype(np.float64), -128.0, 127.0)


def _finish(acc_z, sx, scale, shift, act):
    """acc_z: float64 integers acc - zp * wsum, channels last -> (float32 value, float64 magnitude)."""
    shape = (-1,) + (1,) * (acc_z.ndim - 1)
    m = (sx.reshape(shape) * scale.astype(np.float32)).astype(np.float32)
    v = (acc_z.astype(np.float32) * m).astype(np.float32)
    v = (v + shift.astype(np.float32)).astype(np.float32)
    mag = np.abs(acc_z) * m.astype(np.float64) + np.abs(shift.astype(np.float64))
    if act == 1:
        v = np.maximum(v, np.float32(0))
    elif act == 3:
        v = np.clip(v, np.float32(0), np.float32(6))
    else:
        assert act == 0, act
    return v, mag


def _scales(ten):
    sc = np.asarray(ten["quant"]["scale"], np.float32).reshape(-1)
    return np.full(ten["shape"][0], sc[0], np.float32) if sc.size == 1 else sc


def hybrid_conv(op, x, ten, bias):
    w = ten["const"]                       # int8 OHWI
    sx, inv, zp = quant_params(x)
    # (q - zp) with zero padding: a padded tap is q = zp, and sum (q - zp) w = acc - zp * wsum as integers
    qz = quantise_input(x, inv, zp) - zp.reshape(-1, 1, 1, 1).astype(np.float64)
    kh, kw = w.shape[1], w.shape[2]
    sh, sw = op.get("stride_h", 1), op.get("stride_w", 1)
    pt, pb = te._pads(x.shape[1], kh, sh, op.get("padding", 0))
    pl, pr = te._pads(x.shape[2], kw, sw, op.get("padding", 0))
    xin = F.pad(torch.from_numpy(qz).permute(0, 3, 1, 2), (pl, pr, pt, pb))
    acc_z = F.conv2d(xin, torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2), stride=(sh, sw)).permute(0, 2, 3, 1).numpy()
    shift = np.zeros(w.shape[0], np.float32) if bias is None else np.asarray(bias, np.float32).reshape(-1)
    return _finish(acc_z, sx, _scales(ten), shift, op.get("act", 0))


def hybrid_fc(op, x, ten, bias):
    w = ten["const"]                       # int8 [out, in]
    flat = np.asarray(x, np.float32).reshape(x.shape[0], -1)
    sx, inv, zp = quant_params(flat, symmetric=not op.get("asymmetric_quantize_inputs", False))
    qz = quantise_input(flat, inv, zp) - zp.reshape(-1, 1).astype(np.float64)
    acc_z = qz @ w.astype(np.float64).T
    shift = np.zeros(w.shape[0], np.float32) if bias is None else np.asarray(bias, np.float32).reshape(-1)
    return _finish(acc_z, sx, _scales(ten), shift, op.get("act", 0))


class _OneOp:
    """One operator as a graph of its own for tflite_eval.evaluate: the activations it reads pose as constants."""

    def __init__(self, g, op, val):
        self.g, self.val, self.ops = g, val, [op]
        self.inputs = [next(t for t in op["inputs"] if t in val)]
        self.tensors = [dict(t, type=0) if k in val else t for k, t in enumerate(g.tensors)]

    def const(self, t):
        return self.val[t] if t in self.val else self.g.const(t)


def evaluate_hybrid(g, x_nhwc):
    """-> ({tensor id: float32 array}, {tensor id of a hybrid output: float64 magnitude |acc - zp wsum| sx scale + |shift|})."""
    val = {g.inputs[0]: np.asarray(x_nhwc, np.float32)}
    mag = {}
    for op in g.ops:
        ins = [t for t in op["inputs"] if t >= 0]
        ten = g.quantised_filter(op)
        y = op["outputs"][0]
        if ten is not None:
            bias = g.const(ins[2]) if len(ins) > 2 else None
            val[y], mag[y] = (hybrid_conv if op["name"] == "CONV_2D" else hybrid_fc)(op, val[ins[0]], ten, bias)
        else:
            shim = _OneOp(g, op, val)
            val[y] = te.evaluate(shim, val[shim.inputs[0]], dtype=torch.float32)[y]
    return val, mag


class _Dequantised:
    def __init__(self, g):
        self.inputs, self.outputs, self.ops = g.inputs, g.outputs, g.ops
        self.tensors = [dict(t, type=0, const=g.dequantised(k)) if t["type"] == 9 else t for k, t in enumerate(g.tensors)]

    def const(self, t):
        return self.tensors[t]["const"]


def evaluate_dequantised(g, x_nhwc, dtype=torch.float64):
    return te.evaluate(_Dequantised(g), x_nhwc, dtype=dtype)
