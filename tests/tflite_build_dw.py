"""Helper (not a test): TFLite flatbuffers with DEPTHWISE_CONV_2D, float32 and dynamic-range quantised, as the converter
writes them.  `ModelDW` is tflite_build_q8.ModelQ8 (so that one model can hold float32 and INT8 filters) with the
operator and its real DepthwiseConv2DOptions; `quantise` is tflite_build_q8.quantise with the converter's rule for
depthwise filters (1024 elements or more: INT8, symmetric scales along dimension 3); `mobilenet_v2` emits the converter's
layout of tf.keras.applications.MobileNetV2(include_top=False) -> GlobalAveragePooling2D -> Dense... (the reference's
`mobilenet` family, ml_tools/kerasmodel.py:144-151): BatchNorms folded, RELU6 fused, a stride-2 depthwise convolution as
PAD ((0, 1), (0, 1)) + VALID, which is what Keras' correct_pad makes of an even-sized input."""
import numpy as np

import tflite_build as tb
import tflite_build_q8 as tq

FILTER_DIM = {"CONV_2D": 0, "FULLY_CONNECTED": 0, "DEPTHWISE_CONV_2D": 3}   # where the per-channel scales go


class ModelDW(tq.ModelQ8):
    def depthwise(self, x, w_1hwc, bias, stride=1, padding=tb.SAME, act=tb.NONE, depth_multiplier=1, dilation=1):
        """w_1hwc: a float32 array [1, kh, kw, C * depth_multiplier], or the id of a tensor (see qfilter); bias: an array or None."""
        if isinstance(w_1hwc, (int, np.integer)):
            wt = int(w_1hwc)
        else:
            w_1hwc = np.asarray(w_1hwc, np.float32)
            wt = self.tensor(w_1hwc.shape, w_1hwc)
        y = self.tensor([1, 0, 0, self.shape(wt)[3]])
        ins = [x, wt] + ([] if bias is None else [self.tensor(np.shape(bias), np.asarray(bias, np.float32))])
        sh, sw = (stride, stride) if np.isscalar(stride) else stride
        dh, dw = (dilation, dilation) if np.isscalar(dilation) else dilation
        return self.op("DEPTHWISE_CONV_2D", ins, [y], {0: ("b", padding), 1: ("i", sw), 2: ("i", sh), 3: ("i", depth_multiplier),
                                                        4: ("b", act), 5: ("i", dw), 6: ("i", dh)})


def quantise_filter(w, dim, per_channel=True):
    """tflite_build_q8.quantise_filter with the scales along dimension `dim` -> (int8 array, float32 scales)."""
    q, scale = tq.quantise_filter(np.moveaxis(np.asarray(w, np.float32), dim, 0), per_channel)
    return np.ascontiguousarray(np.moveaxis(q, 0, dim)), scale


def _options(op):
    if op["name"] == "DEPTHWISE_CONV_2D":
        return {0: ("b", op["padding"]), 1: ("i", op["stride_w"]), 2: ("i", op["stride_h"]), 3: ("i", op["depth_multiplier"]),
                4: ("b", op["act"]), 5: ("i", op["dilation_w"]), 6: ("i", op["dilation_h"])}
    return tq._options(op)


def quantise(blob, min_elements=1024, asymmetric_fc=True, dw_per_channel=True):
    """A float flatbuffer -> the dynamic-range quantised one: every CONV_2D / DEPTHWISE_CONV_2D / FULLY_CONNECTED filter of
    at least min_elements elements INT8 (a convolution's scales per output channel -- dimension 0, a depthwise one's
    dimension 3 -- a dense layer's one)."""
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    filters = {}
    for op in g.ops:
        if op["name"] in FILTER_DIM:
            t = op["inputs"][1]
            w = g.const(t)
            if w is not None and w.dtype == np.float32 and w.size >= min_elements:
                filters[t] = op["name"]
    m = ModelDW()
    for k, t in enumerate(g.tensors):
        if k in filters:
            name = filters[k]
            per_channel = name == "CONV_2D" or (name == "DEPTHWISE_CONV_2D" and dw_per_channel)
            q, scale = quantise_filter(t["const"], FILTER_DIM[name], per_channel)
            m.qfilter(q, scale, dim=FILTER_DIM[name], name=t["name"] or "t")
        else:
            m.tensor(t["shape"], t["const"], t["name"] or "t", t["type"])
    for op in g.ops:
        if op["name"] == "FULLY_CONNECTED" and op["inputs"][1] in filters:
            op = dict(op, asymmetric_quantize_inputs=asymmetric_fc)
        m.op(op["name"], op["inputs"], op["outputs"], _options(op))
    m.inputs, m.outputs = list(g.inputs), list(g.outputs)
    return m.finish()


BLOCKS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))   # t, c, n, s


def mobilenet_v2(n_labels, dense_sizes=(), seed=0, width=1.0, size=160, activation="sigmoid", head_gain=1.0):
    """-> flatbuffer bytes.  Weights as tflite_build.inception_v3 draws them: normal with variance 2 / fan-in (a depthwise
    filter's fan-in is its kh * kw taps), biases normal 0.05.  `width` is Keras' alpha (channel counts to multiples of 8);
    head_gain scales the last Dense's weights."""
    rng = np.random.default_rng(seed)
    m = ModelDW()

    def ch(c):
        v = max(8, int(c * width + 4) // 8 * 8)
        return v + 8 if v < 0.9 * c * width else v

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
    x = conv(x, ch(32), 3, 2, tb.RELU6)
    for t, c, n, s in BLOCKS:
        for i in range(n):
            cin, stride = m.shape(x)[3], s if i == 0 else 1
            y = x if t == 1 else conv(x, t * cin, 1, 1, tb.RELU6)
            y = conv(depthwise(y, stride), ch(c), 1, 1, tb.NONE)
            x = m.binary("ADD", x, y) if stride == 1 and cin == ch(c) else y
    x = conv(x, ch(1280) if width > 1.0 else 1280, 1, 1, tb.RELU6)
    x = m.mean(x)
    for d in dense_sizes:
        cin = m.shape(x)[1]
        x = m.dense(x, rng.normal(0.0, np.sqrt(2.0 / cin), size=(d, cin)).astype(np.float32),
                    rng.normal(0.0, 0.05, size=d).astype(np.float32), tb.RELU)
    cin = m.shape(x)[1]
    logits = m.dense(x, (head_gain * rng.normal(0.0, np.sqrt(2.0 / cin), size=(n_labels, cin))).astype(np.float32),
                     rng.normal(0.0, 0.05, size=n_labels).astype(np.float32))
    out = m.softmax(logits) if activation == "softmax" else m.unary("LOGISTIC", logits)
    m.outputs = [out]
    return m.finish()
