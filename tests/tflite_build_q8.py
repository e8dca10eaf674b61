"""Helper (not a test): dynamic-range quantised TFLite flatbuffers, as the converter writes them with
`optimizations = [Optimize.DEFAULT]` and no representative dataset: the filter of a CONV_2D / FULLY_CONNECTED with at
least 1024 elements is INT8 with symmetric scales (one per output channel for a convolution, one for a dense layer),
everything else stays float32.  `ModelQ8` is tflite_build.Model with INT8 tensors that carry a quantisation table and
FULLY_CONNECTED's asymmetric_quantize_inputs; `quantise` re-emits a float flatbuffer that way."""
import struct

import numpy as np

import tflite_build as tb

INT16, INT8 = 7, 9
_DTYPES = {tb.FLOAT32: "<f4", tb.INT32: "<i4", tb.UINT8: "u1", INT16: "<i2", INT8: "i1"}


class ModelQ8(tb.Model):
    def __init__(self):
        super().__init__()
        self.quant = {}   # tensor index -> (scales, zero points, quantized_dimension)

    def tensor(self, shape, data=None, name="t", ttype=None, quant=None):
        if data is not None and ttype in (tb.UINT8, INT16, INT8):
            self.buffers.append(np.ascontiguousarray(data, _DTYPES[ttype]).tobytes())
            self.tensors.append((list(shape), ttype, len(self.buffers) - 1, name))
            idx = len(self.tensors) - 1
        else:
            idx = super().tensor(shape, data, name, ttype)
        if quant is not None:
            scale, zero_point, dim = quant
            self.quant[idx] = ([float(v) for v in np.asarray(scale, np.float32).reshape(-1)],
                               [int(v) for v in np.asarray(zero_point).reshape(-1)], int(dim))
        return idx

    def qfilter(self, q, scale, zero_point=None, dim=0, ttype=INT8, name="filter_q8"):
        """An integer constant with its quantisation table; zero_point defaults to zeros, one per scale."""
        scale = np.asarray(scale, np.float32).reshape(-1)
        zp = np.zeros(scale.size, np.int64) if zero_point is None else zero_point
        return self.tensor(np.shape(q), q, name, ttype, quant=(scale, zp, dim))

    def conv_q8(self, x, w_tensor, bias, stride=1, padding=tb.SAME, act=tb.NONE):
        """CONV_2D whose filter is the tensor `w_tensor` (see qfilter); bias: a float array, a tensor id or None."""
        y = self.tensor([1, 0, 0, self.shape(w_tensor)[0]])
        ins = [x, w_tensor]
        if bias is not None:
            ins.append(bias if isinstance(bias, (int, np.integer)) else self.tensor(np.shape(bias), np.asarray(bias, np.float32)))
        sh, sw = (stride, stride) if np.isscalar(stride) else stride
        return self.op("CONV_2D", ins, [y], {0: ("b", padding), 1: ("i", sw), 2: ("i", sh), 3: ("b", act), 4: ("i", 1), 5: ("i", 1)})

    def dense_q8(self, x, w_tensor, bias, act=tb.NONE, asymmetric=True):
        y = self.tensor([1, self.shape(w_tensor)[0]])
        ins = [x, w_tensor] + ([] if bias is None else [self.tensor(np.shape(bias), np.asarray(bias, np.float32))])
        return self.op("FULLY_CONNECTED", ins, [y], {0: ("b", act), 3: ("b", 1 if asymmetric else 0)})

    def finish(self):
        """tflite_build.Model.finish with the tensors' quantisation tables (Tensor field 4: scale = field 2, zero_point =
        field 3, an int64 vector, quantized_dimension = field 6)."""
        w = tb._Writer()
        code_list = sorted(set(o[0] for o in self.ops))

        def int64s(values):
            w.pad()
            pos = len(w.b)
            w.b += struct.pack("<I%dq" % len(values), len(values), *values)
            return pos

        def quant_w(q):
            scale, zp, dim = q
            return lambda: w.table({2: ("ref", lambda: w.scalars("f", scale)), 3: ("ref", lambda: int64s(zp)), 6: ("i", dim)})

        def tensor_w(k, t):
            shape, ttype, bi, name = t
            f = {0: ("ref", lambda: w.scalars("i", shape)), 1: ("b", ttype), 2: ("I", bi),
                 3: ("ref", lambda: w.raw(name.encode(), b"\0"))}
            if k in self.quant:
                f[4] = ("ref", quant_w(self.quant[k]))
            return lambda: w.table(f)

        def options_w(opts):
            f = {}
            for k, (kind, val) in opts.items():
                f[k] = ("ref", (lambda v=val: w.scalars("i", v))) if kind == "ints" else (kind, val)
            return lambda: w.table(f)

        def op_w(o):
            code, ins, outs, ot, opts = o
            f = {0: ("I", code_list.index(code)), 1: ("ref", lambda: w.scalars("i", ins)), 2: ("ref", lambda: w.scalars("i", outs))}
            if opts is not None:
                f[3] = ("B", ot)
                f[4] = ("ref", options_w(opts))
            return lambda: w.table(f)

        def sub_w():
            return w.table({0: ("ref", lambda: w.tables([tensor_w(k, t) for k, t in enumerate(self.tensors)])),
                            1: ("ref", lambda: w.scalars("i", self.inputs)), 2: ("ref", lambda: w.scalars("i", self.outputs)),
                            3: ("ref", lambda: w.tables([op_w(o) for o in self.ops]))})

        def code_w(c):
            return lambda: w.table({0: ("b", min(c, 127)), 3: ("i", c)})

        def buffer_w(d):
            return lambda: w.table({0: ("ref", lambda: w.raw(d))} if d else {})

        root = w.table({0: ("I", 3), 1: ("ref", lambda: w.tables([code_w(c) for c in code_list])),
                        2: ("ref", lambda: w.tables([sub_w])),
                        4: ("ref", lambda: w.tables([buffer_w(d) for d in self.buffers]))})
        struct.pack_into("<I", w.b, 0, root)
        return bytes(w.b)


def quantise_filter(w, per_channel):
    """The converter's symmetric quantisation: scale = max |w| / 127 (per first-dimension slice or per tensor), round, clip
    to +-127.  -> (int8 array, float32 scales)."""
    w = np.asarray(w, np.float32)
    flat = np.abs(w.reshape(w.shape[0], -1))
    m = flat.max(axis=1) if per_channel else np.array([flat.max()])
    scale = np.where(m > 0, m / np.float32(127), np.float32(1)).astype(np.float32)
    q = np.clip(np.round(w / scale.reshape((-1,) + (1,) * (w.ndim - 1))), -127, 127).astype(np.int8)
    return q, scale


def _options(op):
    n = op["name"]
    if n == "CONV_2D":
        return {0: ("b", op["padding"]), 1: ("i", op["stride_w"]), 2: ("i", op["stride_h"]), 3: ("b", op["act"]),
                4: ("i", op["dilation_w"]), 5: ("i", op["dilation_h"])}
    if n in ("AVERAGE_POOL_2D", "MAX_POOL_2D"):
        return {0: ("b", op["padding"]), 1: ("i", op["stride_w"]), 2: ("i", op["stride_h"]), 3: ("i", op["filter_width"]),
                4: ("i", op["filter_height"]), 5: ("b", op["act"])}
    if n == "CONCATENATION":
        return {0: ("i", op["axis"]), 1: ("b", op["act"])}
    if n in ("ADD", "MUL", "SUB"):
        return {0: ("b", op["act"])}
    if n == "FULLY_CONNECTED":
        return {0: ("b", op["act"]), 3: ("b", 1 if op.get("asymmetric_quantize_inputs") else 0)}
    if n == "SOFTMAX":
        return {0: ("f", op["beta"])}
    if n == "MEAN":
        return {0: ("b", 1 if op["keep_dims"] else 0)}
    if n == "RESHAPE":
        return {0: ("ints", list(op["new_shape"]))}
    if n == "PAD":
        return {}
    return None


def quantise(blob, min_elements=1024, asymmetric_fc=True):
    """A float flatbuffer (of the operators tflite_build writes) -> the dynamic-range quantised one: same tensors, same
    operators, every CONV_2D / FULLY_CONNECTED filter of at least min_elements elements INT8."""
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    filters = {}
    for op in g.ops:
        if op["name"] in ("CONV_2D", "FULLY_CONNECTED"):
            t = op["inputs"][1]
            w = g.const(t)
            if w is not None and w.dtype == np.float32 and w.size >= min_elements:
                filters[t] = op["name"] == "CONV_2D"
    m = ModelQ8()
    for k, t in enumerate(g.tensors):
        if k in filters:
            q, scale = quantise_filter(t["const"], filters[k])
            m.qfilter(q, scale, name=t["name"] or "t")
        else:
            m.tensor(t["shape"], t["const"], t["name"] or "t", t["type"])
    for op in g.ops:
        if op["name"] == "FULLY_CONNECTED" and op["inputs"][1] in filters:
            op = dict(op, asymmetric_quantize_inputs=asymmetric_fc)
        m.op(op["name"], op["inputs"], op["outputs"], _options(op))
    m.inputs, m.outputs = list(g.inputs), list(g.outputs)
    return m.finish()
