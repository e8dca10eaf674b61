"""Helper (not a test): tflite_eval_dw for graphs of the EfficientNet family.  The broadcasting MUL, MEAN with keep_dims and
RESHAPE are tflite_eval's already; this adds DIV (an activation by a constant, or two activations) and walks the graph
one operator at a time the way tflite_eval_dw does.  It reads the tflite_reader.Graph only -- nothing of
cpx/ml_tools/tflite_graph.py."""
import numpy as np
import torch

import tflite_eval as te
import tflite_eval_dw as ted
import tflite_eval_q8 as tq8


def _div(g, op, val, np_dtype):
    a, b = (val[t] if t in val else np.asarray(g.const(t)) for t in op["inputs"][:2])
    r = te._act(torch.as_tensor(np.asarray(a, np_dtype) / np.asarray(b, np_dtype)), op.get("act", 0)).numpy()
    return np.ascontiguousarray(r)


def evaluate(g, x_nhwc, dtype=torch.float64, magnitudes=False):
    """tflite_eval_dw.evaluate with DIV."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    val = {g.inputs[0]: np.asarray(x_nhwc, np_dtype)}
    mag = {}
    for op in g.ops:
        ins = [t for t in op["inputs"] if t >= 0]
        y = op["outputs"][0]
        if op["name"] == "DIV":
            val[y] = _div(g, op, val, np_dtype)
        elif op["name"] == "DEPTHWISE_CONV_2D":
            val[y], mag[y] = ted.depthwise(op, val[ins[0]], g.const(ins[1]), ted._bias(g, ins), dtype, magnitude=True)
        else:
            shim = tq8._OneOp(g, op, val)
            out = te.evaluate(shim, val[shim.inputs[0]], dtype=dtype, magnitudes=magnitudes)
            if magnitudes:
                out, m = out
                mag.update(m)
            val[y] = out[y]
    return (val, mag) if magnitudes else val


def evaluate_hybrid(g, x_nhwc):
    """tflite_eval_dw.evaluate_hybrid with DIV."""
    val = {g.inputs[0]: np.asarray(x_nhwc, np.float32)}
    mag = {}
    for op in g.ops:
        ins = [t for t in op["inputs"] if t >= 0]
        ten = g.quantised_filter(op)
        y = op["outputs"][0]
        if ten is not None:
            fn = {"CONV_2D": tq8.hybrid_conv, "FULLY_CONNECTED": tq8.hybrid_fc, "DEPTHWISE_CONV_2D": ted.hybrid_depthwise}[op["name"]]
            val[y], mag[y] = fn(op, val[ins[0]], ten, ted._bias(g, ins))
        elif op["name"] == "DIV":
            val[y] = _div(g, op, val, np.float32)
        elif op["name"] == "DEPTHWISE_CONV_2D":
            val[y] = ted.depthwise(op, val[ins[0]], g.const(ins[1]), ted._bias(g, ins), torch.float32)
        else:
            shim = tq8._OneOp(g, op, val)
            val[y] = te.evaluate(shim, val[shim.inputs[0]], dtype=torch.float32)[y]
    return val, mag


def evaluate_dequantised(g, x_nhwc, dtype=torch.float64):
    return evaluate(tq8._Dequantised(g), x_nhwc, dtype=dtype)
