"""Helper (not a test): tflite_eval / tflite_eval_q8 for graphs with DEPTHWISE_CONV_2D.  It reads the tflite_reader.Graph
only -- nothing of cpx/ml_tools/tflite_graph.py -- and evaluates one operator at a time, the way tflite_eval_q8._OneOp
does: DEPTHWISE_CONV_2D here (a grouped convolution on PyTorch-CPU, float64 by default, with the magnitude
sum |x| |w| + |b|; its hybrid form as the integer restatement of include/cpx.h, CPX_GRAPH_DWCONV_Q8), the CONV_2D /
FULLY_CONNECTED hybrids with tflite_eval_q8's functions, everything else with tflite_eval.evaluate."""
import numpy as np
import torch
import torch.nn.functional as F

import tflite_eval as te
import tflite_eval_q8 as tq8


def _geometry(op, x_shape, w_shape):
    sh, sw = op.get("stride_h", 1), op.get("stride_w", 1)
    pt, pb = te._pads(x_shape[1], w_shape[1], sh, op.get("padding", 0))
    pl, pr = te._pads(x_shape[2], w_shape[2], sw, op.get("padding", 0))
    return (sh, sw), (pl, pr, pt, pb)


def depthwise(op, x, w, bias, dtype=torch.float64, magnitude=False):
    """x: [N, H, W, C], w: [1, kh, kw, C] -> NHWC numpy (and sum |x| |w| + |b|)."""
    a = torch.as_tensor(np.asarray(x), dtype=dtype)
    wt = torch.as_tensor(np.array(w), dtype=dtype).permute(3, 0, 1, 2)   # [C, 1, kh, kw]
    b = None if bias is None else torch.as_tensor(np.array(bias), dtype=dtype).reshape(-1)
    c = a.shape[3]
    assert wt.shape[0] == c, "depth multiplier 1 only"
    stride, pads = _geometry(op, a.shape, w.shape)
    xin = F.pad(a.permute(0, 3, 1, 2), pads)
    y = te._act(F.conv2d(xin, wt, b, stride=stride, groups=c), op.get("act", 0)).permute(0, 2, 3, 1).contiguous().numpy()
    if not magnitude:
        return y
    mag = F.conv2d(xin.abs(), wt.abs(), None if b is None else b.abs(), stride=stride, groups=c)
    return y, mag.permute(0, 2, 3, 1).contiguous().numpy()


def hybrid_depthwise(op, x, ten, bias):
    """The integer restatement: q per sample, a padded tap q = zp, acc - zp wsum = sum (q - zp) w exactly, then the
    float32 epilogue of tflite_eval_q8._finish with the scales along dimension 3."""
    w = ten["const"]                       # int8 [1, kh, kw, C]
    x = np.asarray(x, np.float32)
    sx, inv, zp = tq8.quant_params(x)
    qz = tq8.quantise_input(x, inv, zp) - zp.reshape(-1, 1, 1, 1).astype(np.float64)
    stride, pads = _geometry(op, x.shape, w.shape)
    c = x.shape[3]
    xin = F.pad(torch.from_numpy(qz).permute(0, 3, 1, 2), pads)
    acc_z = F.conv2d(xin, torch.from_numpy(w.astype(np.float64)).permute(3, 0, 1, 2), stride=stride, groups=c)
    acc_z = acc_z.permute(0, 2, 3, 1).contiguous().numpy()
    sc = np.asarray(ten["quant"]["scale"], np.float32).reshape(-1)
    sc = np.full(c, sc[0], np.float32) if sc.size == 1 else sc
    shift = np.zeros(c, np.float32) if bias is None else np.asarray(bias, np.float32).reshape(-1)
    return tq8._finish(acc_z, sx, sc, shift, op.get("act", 0))


def _bias(g, ins):
    return g.const(ins[2]) if len(ins) > 2 else None


def evaluate(g, x_nhwc, dtype=torch.float64, magnitudes=False):
    """tflite_eval.evaluate for a float32 graph that may hold DEPTHWISE_CONV_2D."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    val = {g.inputs[0]: np.asarray(x_nhwc, np_dtype)}
    mag = {}
    for op in g.ops:
        ins = [t for t in op["inputs"] if t >= 0]
        y = op["outputs"][0]
        if op["name"] == "DEPTHWISE_CONV_2D":
            val[y], mag[y] = depthwise(op, val[ins[0]], g.const(ins[1]), _bias(g, ins), dtype, magnitude=True)
        else:
            shim = tq8._OneOp(g, op, val)
            out = te.evaluate(shim, val[shim.inputs[0]], dtype=dtype, magnitudes=magnitudes)
            if magnitudes:
                out, m = out
                mag.update(m)
            val[y] = out[y]
    return (val, mag) if magnitudes else val


def evaluate_hybrid(g, x_nhwc):
    """tflite_eval_q8.evaluate_hybrid with the depthwise operator, hybrid where its filter is INT8, float32 otherwise."""
    val = {g.inputs[0]: np.asarray(x_nhwc, np.float32)}
    mag = {}
    for op in g.ops:
        ins = [t for t in op["inputs"] if t >= 0]
        ten = g.quantised_filter(op)
        y = op["outputs"][0]
        if ten is not None:
            fn = {"CONV_2D": tq8.hybrid_conv, "FULLY_CONNECTED": tq8.hybrid_fc, "DEPTHWISE_CONV_2D": hybrid_depthwise}[op["name"]]
            val[y], mag[y] = fn(op, val[ins[0]], ten, _bias(g, ins))
        elif op["name"] == "DEPTHWISE_CONV_2D":
            val[y] = depthwise(op, val[ins[0]], g.const(ins[1]), _bias(g, ins), torch.float32)
        else:
            shim = tq8._OneOp(g, op, val)
            val[y] = te.evaluate(shim, val[shim.inputs[0]], dtype=torch.float32)[y]
    return val, mag


def evaluate_dequantised(g, x_nhwc, dtype=torch.float64):
    """The graph with its INT8 filters multiplied out (int8 x scale, along each filter's own quantised dimension)."""
    return evaluate(tq8._Dequantised(g), x_nhwc, dtype=dtype)
