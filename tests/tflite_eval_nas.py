"""Helper (not a test): tflite_eval_se for graphs with STRIDED_SLICE / SLICE (a NASNet's Cropping2D).  A slice is NumPy
indexing by the form the reader resolved it into -- (start, stride, count) per axis, tflite_reader.resolve_slice on the
shape of the array at hand, since a flatbuffer need not state the shapes of its activations; every other operator is handed
to tflite_eval_se one at a time.  It reads the tflite_reader.Graph only -- nothing of cpx/ml_tools/tflite_graph.py."""
import numpy as np
import torch

import tflite_eval_q8 as tq8
import tflite_eval_se as tes

SLICE_OPS = ("STRIDED_SLICE", "SLICE")


def resolved(op, shape):
    from cpx.ml_tools.tflite_reader import resolve_slice

    return op.get("slice") or resolve_slice(op, list(shape), op["name"])


def slice_array(op, x):
    index = tuple(slice(b, b + s * (n - 1) + 1, s) for b, s, n in resolved(op, x.shape)[1:])
    return np.ascontiguousarray(x[(slice(None),) + index])


class _OneOpGraph(tq8._OneOp):
    """... that tflite_eval_se.evaluate can walk: it reads g.ops, g.inputs, g.const and g.quantised_filter."""

    def quantised_filter(self, op):
        return self.g.quantised_filter(op)


def evaluate(g, x_nhwc, dtype=torch.float64, magnitudes=False):
    """tflite_eval_se.evaluate with STRIDED_SLICE / SLICE -> {tensor id: array} (and the magnitudes of the filter
    operators' outputs)."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    val = {g.inputs[0]: np.asarray(x_nhwc, np_dtype)}
    mag = {}
    for op in g.ops:
        y = op["outputs"][0]
        if op["name"] in SLICE_OPS:
            val[y] = slice_array(op, val[op["inputs"][0]])
            continue
        shim = _OneOpGraph(g, op, val)
        out = tes.evaluate(shim, val[shim.inputs[0]], dtype=dtype, magnitudes=magnitudes)
        if magnitudes:
            out, m = out
            mag.update(m)
        val[y] = out[y]
    return (val, mag) if magnitudes else val
