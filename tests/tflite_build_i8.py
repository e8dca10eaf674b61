"""Helper (not a test): full-integer TFLite flatbuffers, as the converter writes them when it is given a representative
dataset: INT8 activations (asymmetric, one scale and one zero point), per-channel symmetric INT8 filters, INT32 biases at
s_in * s_w[c], INT8 constants for MUL / ADD operands, QUANTIZE in front and DEQUANTIZE behind.  `quantise_full` re-emits a
float32 flatbuffer of tflite_build.Model that way from a calibration batch; `ModelI8` builds single operators with
hand-chosen scales and zero points."""
import numpy as np

import tflite_build as tb
import tflite_build_dw as td
import tflite_build_nas  # noqa: F401  (registers STRIDED_SLICE / SLICE with tflite_build)
import tflite_build_q8 as tq
import tflite_eval_dw as ted

INT8 = tq.INT8
QUANTIZE, DEQUANTIZE = 114, 6
SAME_PARAMS = ("MAX_POOL_2D", "AVERAGE_POOL_2D", "PAD", "RESHAPE", "CONCATENATION", "STRIDED_SLICE", "SLICE")


def asymmetric(lo, hi):
    """The range widened to hold 0 -> (float32 scale, zero point) of an INT8 tensor."""
    lo, hi = min(float(lo), 0.0), max(float(hi), 0.0)
    if hi == lo:
        return np.float32(1.0 / 255.0), 0
    scale = np.float32((hi - lo) / 255.0)
    return scale, int(np.clip(np.round(-128.0 - lo / float(scale)), -128, 127))


def to_int8(x, scale, zp):
    return np.clip(np.round(np.asarray(x, np.float64) / float(scale)) + zp, -128, 127).astype(np.int8)


class ModelI8(td.ModelDW):
    """Direct builders: every activation tensor is made with its (scale, zero point)."""

    def qact(self, shape, qp, name="q"):
        return self.tensor(list(shape), None, name, INT8, quant=([qp[0]], [qp[1]], 0))

    def qconst(self, q, qp, name="const_q8"):
        return self.tensor(np.shape(q), np.asarray(q, np.int8), name, INT8, quant=([qp[0]], [qp[1]], 0))

    def qp(self, t):
        s, z, _ = self.quant[t]
        return np.float32(s[0]), int(z[0])

    def quantize(self, x, qp):
        return self.op("QUANTIZE", [x], [self.qact(self.shape(x), qp)], None, code=QUANTIZE)

    def dequantize(self, x):
        return self.op("DEQUANTIZE", [x], [self.tensor(list(self.shape(x)))], None, code=DEQUANTIZE)

    def _bias(self, bias, x, w_scales):
        if bias is None:
            return []
        s = np.float32(self.qp(x)[0]) * np.asarray(w_scales, np.float32).reshape(-1)
        return [self.tensor(np.shape(bias), np.asarray(bias, np.int32), "bias_i32", tb.INT32, quant=(s, np.zeros(s.size, np.int64), 0))]

    def conv_i8(self, x, w_q, w_scales, bias_i32, out_qp, stride=1, padding=tb.SAME, act=tb.NONE):
        """w_q: int8 OHWI; w_scales: one or one per output channel; bias_i32: int32 [Cout] or None."""
        wt = self.qfilter(np.asarray(w_q, np.int8), w_scales)
        y = self.qact([1, 0, 0, np.shape(w_q)[0]], out_qp)
        sh, sw = (stride, stride) if np.isscalar(stride) else stride
        return self.op("CONV_2D", [x, wt] + self._bias(bias_i32, x, w_scales), [y],
                       {0: ("b", padding), 1: ("i", sw), 2: ("i", sh), 3: ("b", act), 4: ("i", 1), 5: ("i", 1)})

    def depthwise_i8(self, x, w_q, w_scales, bias_i32, out_qp, stride=1, padding=tb.SAME, act=tb.NONE):
        wt = self.qfilter(np.asarray(w_q, np.int8), w_scales, dim=3)
        y = self.qact([1, 0, 0, np.shape(w_q)[3]], out_qp)
        sh, sw = (stride, stride) if np.isscalar(stride) else stride
        return self.op("DEPTHWISE_CONV_2D", [x, wt] + self._bias(bias_i32, x, w_scales), [y],
                       {0: ("b", padding), 1: ("i", sw), 2: ("i", sh), 3: ("i", 1), 4: ("b", act), 5: ("i", 1), 6: ("i", 1)})

    def dense_i8(self, x, w_q, w_scale, bias_i32, out_qp, act=tb.NONE):
        wt = self.qfilter(np.asarray(w_q, np.int8), w_scale)
        y = self.qact([1, np.shape(w_q)[0]], out_qp)
        return self.op("FULLY_CONNECTED", [x, wt] + self._bias(bias_i32, x, w_scale), [y], {0: ("b", act)})

    def binary_i8(self, name, a, b, out_qp, act=tb.NONE, const_first=False):
        """b: the id of an INT8 tensor (an activation, or a constant made with qconst)."""
        y = self.qact(self.shape(a), out_qp)
        return self.op(name, [b, a] if const_first else [a, b], [y], {0: ("b", act)})

    def pool_i8(self, kind, x, k, stride, padding, act=tb.NONE, qp=None):
        """The operators that keep the parameters (pool, pad, concat, slices) are built as ever and their output then made
        INT8 with the input's parameters -- or `qp`'s, for a file the planner has to refuse."""
        return self._retype(self.pool(kind, x, k, stride, padding, act), self.qp(x) if qp is None else qp)

    def _retype(self, y, qp):
        shape, _, bi, name = self.tensors[y]
        self.tensors[y] = (shape, INT8, bi, name)
        self.quant[y] = ([float(qp[0])], [int(qp[1])], 0)
        return y

    def mean_i8(self, x, out_qp, keep_dims=False):
        return self._retype(self.mean(x, keep_dims=keep_dims), out_qp)

    def pad_i8(self, x, paddings, qp=None):
        return self._retype(self.pad(x, paddings), self.qp(x) if qp is None else qp)

    def concat_i8(self, xs, qp=None):
        return self._retype(self.concat(xs), self.qp(xs[0]) if qp is None else qp)

    def strided_slice_i8(self, x, begin, end, strides, **masks):
        y = self.tensor([1, 0, 0, self.shape(x)[3]])
        idx = [self.tensor([4], np.array(v, np.int32)) for v in (begin, end, strides)]
        self.op("STRIDED_SLICE", [x] + idx, [y], {0: ("i", masks.get("begin_mask", 0)), 1: ("i", masks.get("end_mask", 0)),
                                                 2: ("i", 0), 3: ("i", 0), 4: ("i", 0), 5: ("b", 0)})
        return self._retype(y, self.qp(x))


def start(shape, qp):
    """-> (model, the INT8 tensor behind the QUANTIZE of a float32 input of `shape`)."""
    m = ModelI8()
    x = m.tensor(list(shape), name="input")
    m.inputs = [x]
    return m, m.quantize(x, qp)


def finish(m, y):
    m.outputs = [m.dequantize(y)]
    return m.finish()


def _options(op):
    n = op["name"]
    if n == "STRIDED_SLICE":
        return {0: ("i", op["begin_mask"]), 1: ("i", op["end_mask"]), 2: ("i", op["ellipsis_mask"]), 3: ("i", op["new_axis_mask"]),
                4: ("i", op["shrink_axis_mask"]), 5: ("b", 1 if op["offset"] else 0)}
    if n == "SLICE":
        return {}
    return td._options(op)


def quantise_full(blob, calibration, float_tail=True):
    """A float32 flatbuffer -> the full-integer one.  Every activation's range is what a float64 evaluation
    (tflite_eval) of the calibration samples gives, widened to hold 0; the operators that move values (pools, PAD, RESHAPE,
    CONCATENATION, slices) are forced to one set of parameters for their inputs and output.  float_tail: a last LOGISTIC /
    SOFTMAX stays float32 behind the DEQUANTIZE (the logits are then the DEQUANTIZE's output); False quantises it too
    (its output at scale 1 / 256, zero point -128, as the converter fixes them)."""
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    vals = ted.evaluate(g, np.asarray(calibration, np.float64))
    gin, gout = g.inputs[0], g.outputs[0]
    ops = list(g.ops)
    tail = ops.pop() if float_tail and ops[-1]["name"] in ("LOGISTIC", "SOFTMAX") else None
    last = ops[-1]["outputs"][0]
    acts = [gin] + [op["outputs"][0] for op in ops]
    # one set of parameters where values only move
    parent = {t: t for t in acts}

    def find(t):
        while parent[t] != t:
            t = parent[t]
        return t

    for op in ops:
        if op["name"] in SAME_PARAMS:
            for t in [t for t in op["inputs"] if t in parent]:
                parent[find(t)] = find(op["outputs"][0])
    lo, hi = {}, {}
    for t in acts:
        r = find(t)
        lo[r], hi[r] = min(lo.get(r, 0.0), float(vals[t].min())), max(hi.get(r, 0.0), float(vals[t].max()))
    qp = {t: asymmetric(lo[find(t)], hi[find(t)]) for t in acts}
    if not float_tail and ops[-1]["name"] in ("LOGISTIC", "SOFTMAX"):
        qp[last] = (np.float32(1.0 / 256.0), -128)

    m = ModelI8()
    filters, biases, consts = {}, {}, {}
    for op in ops:
        ins = [t for t in op["inputs"] if t >= 0]
        if op["name"] in td.FILTER_DIM:
            filters[ins[1]] = (op["name"], ins[0])
            if len(ins) > 2:
                biases[ins[2]] = ins[1]
        elif op["name"] in ("ADD", "SUB", "MUL"):
            for t in ins:
                if g.const(t) is not None:
                    consts[t] = True
    wscale = {}
    for k, t in enumerate(g.tensors):
        name = t["name"] or "t"
        if k in filters:
            opname, _ = filters[k]
            dim = td.FILTER_DIM[opname]
            q, scale = td.quantise_filter(t["const"], dim, per_channel=opname != "FULLY_CONNECTED")
            wscale[k] = scale
            m.qfilter(q, scale, dim=dim, name=name)
        elif k in biases:
            m.tensor(t["shape"], None, name)   # (placeholder: written below, once the filter's scales are known)
        elif k in consts:
            c = np.asarray(t["const"], np.float64)
            p = asymmetric(c.min(), c.max())
            m.qconst(to_int8(c, *p), p, name=name)
        elif k in qp and t["const"] is None and k != gin:
            m.qact(t["shape"], qp[k], name)
        else:
            m.tensor(t["shape"], t["const"], name, t["type"])
    for k, wk in biases.items():
        s = np.float32(qp[filters[wk][1]][0]) * wscale[wk]
        s = np.full(g.tensors[k]["const"].size, s[0], np.float32) if s.size == 1 else s
        b = np.round(np.asarray(g.tensors[k]["const"], np.float64) / s.astype(np.float64)).astype(np.int64)
        m.buffers.append(np.ascontiguousarray(b, "<i4").tobytes())
        m.tensors[k] = (list(g.tensors[k]["shape"]), tb.INT32, len(m.buffers) - 1, g.tensors[k]["name"] or "bias")
        m.quant[k] = ([float(v) for v in s], [0] * s.size, 0)
    q_in = m.qact(g.tensors[gin]["shape"], qp[gin], "input_q")
    m.op("QUANTIZE", [gin], [q_in], None, code=QUANTIZE)
    for op in ops:
        m.op(op["name"], [q_in if t == gin else t for t in op["inputs"]], op["outputs"], _options(op))
    out_f = m.tensor(g.tensors[last]["shape"], None, "dequantised")
    m.op("DEQUANTIZE", [last], [out_f], None, code=DEQUANTIZE)
    if tail is not None:
        m.op(tail["name"], [out_f], tail["outputs"], _options(tail))
        m.outputs = list(tail["outputs"])
    else:
        m.outputs = [out_f]
    m.inputs = [gin]
    return m.finish()


def mobilenet_v2_blocks(n_labels, size=48, seed=0, activation="softmax"):
    """Three MobileNetV2 blocks behind the stem (expansion 1 at stride 1, expansion 6 at stride 2 with its PAD, expansion 6
    at stride 1 with the residual ADD), the 1 x 1 head convolution, MEAN, Dense."""
    rng = np.random.default_rng(seed)
    m = td.ModelDW()

    def conv(x, co, k, stride, act):
        cin = m.shape(x)[3]
        w = rng.normal(0.0, np.sqrt(2.0 / (k * k * cin)), size=(co, k, k, cin)).astype(np.float32)
        return m.conv(x, w, rng.normal(0.0, 0.05, size=co).astype(np.float32), stride, tb.SAME, act)

    def depthwise(x, stride):
        c = m.shape(x)[3]
        w = rng.normal(0.0, np.sqrt(2.0 / 9), size=(1, 3, 3, c)).astype(np.float32)
        b = rng.normal(0.0, 0.05, size=c).astype(np.float32)
        if stride == 2:
            return m.depthwise(m.pad(x, [[0, 0], [0, 1], [0, 1], [0, 0]]), w, b, 2, tb.VALID, tb.RELU6)
        return m.depthwise(x, w, b, 1, tb.SAME, tb.RELU6)

    x = m.tensor([1, size, size, 3], name="input")
    m.inputs = [x]
    x = conv(x, 16, 3, 2, tb.RELU6)
    for t, c, s in ((1, 16, 1), (6, 24, 2), (6, 24, 1)):
        cin = m.shape(x)[3]
        y = x if t == 1 else conv(x, t * cin, 1, 1, tb.RELU6)
        y = conv(depthwise(y, s), c, 1, 1, tb.NONE)
        x = m.binary("ADD", x, y) if s == 1 and cin == c else y
    x = m.mean(conv(x, 64, 1, 1, tb.RELU6))
    logits = m.dense(x, rng.normal(0.0, np.sqrt(2.0 / 64), size=(n_labels, 64)).astype(np.float32),
                     rng.normal(0.0, 0.05, size=n_labels).astype(np.float32))
    m.outputs = [m.softmax(logits) if activation == "softmax" else m.unary("LOGISTIC", logits)]
    return m.finish()
