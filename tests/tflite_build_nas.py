"""Helper (not a test): TFLite flatbuffers with STRIDED_SLICE and SLICE, and a NASNet-layout network.  `ModelNAS` is
tflite_build_se.ModelSE with the two operators and their real options (StridedSliceOptions: begin_mask, end_mask,
ellipsis_mask, new_axis_mask, shrink_axis_mask, offset; SliceOptions is empty).

`nasnet` follows keras.applications.nasnet (NASNet-A: the reference's `nasnet` family is NASNetLarge,
ml_tools/kerasmodel.py:103-224) as restated from memory -- neither Keras nor the converter is installed, so this is a
STRUCTURAL STAND-IN, not the converter's exact layout of a NASNet: whether the converter merges identical RELUs of one
tensor (merge_relus) and whether Cropping2D arrives as STRIDED_SLICE or SLICE is unpinned.  What it has of a NASNet:
`_adjust_block`'s two half-size paths (AveragePooling2D(1, strides=2), and ZeroPadding2D(((0,1),(0,1))) ->
Cropping2D(((1,0),(1,0))) -> the same pool), a bare Activation('relu') in front of every separable convolution on a
tensor that has other readers, ZeroPadding2D(correct_pad) + VALID in front of every stride-2 separable convolution and
pool, the five branches of the normal and the reduction cell, (x, ip) handed from cell to cell with skip_reduction."""
import numpy as np

import tflite_build as tb
import tflite_build_dw as td
import tflite_build_se as ts

tb.CODES.setdefault("STRIDED_SLICE", 45)
tb.CODES.setdefault("SLICE", 65)
tb.OPTION_TYPES.setdefault("STRIDED_SLICE", 32)
tb.OPTION_TYPES.setdefault("SLICE", 44)


class ModelNAS(ts.ModelSE):
    def _index(self, v):
        """A constant int32 vector, or the id of a tensor that is to stand there."""
        return int(v) if isinstance(v, (int, np.integer)) else self.tensor([len(v)], np.array(v, np.int32))

    def strided_slice(self, x, begin, end, strides, begin_mask=0, end_mask=0, ellipsis_mask=0, new_axis_mask=0,
                      shrink_axis_mask=0, offset=False):
        y = self.tensor([1, 0, 0, self.shape(x)[3]])
        return self.op("STRIDED_SLICE", [x, self._index(begin), self._index(end), self._index(strides)], [y],
                       {0: ("i", begin_mask), 1: ("i", end_mask), 2: ("i", ellipsis_mask), 3: ("i", new_axis_mask),
                        4: ("i", shrink_axis_mask), 5: ("b", 1 if offset else 0)})

    def slice(self, x, begin, size):
        y = self.tensor([1, 0, 0, self.shape(x)[3]])
        return self.op("SLICE", [x, self._index(begin), self._index(size)], [y], {})

    def crop_top_left(self, x, as_slice=False):
        """Cropping2D(((1, 0), (1, 0))): [:, 1:, 1:, :], as the STRIDED_SLICE with masks or as a SLICE with sizes -1."""
        if as_slice:
            return self.slice(x, [0, 1, 1, 0], [-1, -1, -1, -1])
        return self.strided_slice(x, [0, 1, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1], begin_mask=0b1001, end_mask=0b1111)


def _conv1x1(m, rng, x, co, act=tb.NONE, gain=1.0):
    cin = m.shape(x)[3]
    w = (gain * rng.normal(0.0, np.sqrt(2.0 / cin), size=(co, 1, 1, cin))).astype(np.float32)
    return m.conv(x, w, rng.normal(0.0, 0.05, size=co).astype(np.float32), 1, tb.SAME, act)


def adjust_paths(m, rng, r, filters, as_slice=False):
    """The half-size paths of _adjust_block on the activated tensor r, concatenated, with the BatchNorm that cannot fold."""
    p1 = _conv1x1(m, rng, m.pool("AVERAGE_POOL_2D", r, 1, 2, tb.VALID), filters // 2)
    p2 = m.crop_top_left(m.pad(r, [[0, 0], [0, 1], [0, 1], [0, 0]]), as_slice)
    p2 = _conv1x1(m, rng, m.pool("AVERAGE_POOL_2D", p2, 1, 2, tb.VALID), filters - filters // 2)
    y = m.concat([p1, p2])
    y = m.binary("MUL", y, rng.uniform(0.7, 1.3, size=filters).astype(np.float32))
    return m.binary("ADD", y, rng.normal(0.0, 0.1, size=filters).astype(np.float32))


def adjust_block(size=31, cin=16, filters=16, seed=0, as_slice=False):
    """-> flatbuffer bytes: RELU -> the two paths -> CONCATENATION -> MUL + ADD on a size x size x cin input."""
    rng = np.random.default_rng(seed)
    m = ModelNAS()
    x = m.tensor([1, size, size, cin], name="input")
    m.inputs = [x]
    m.outputs = [adjust_paths(m, rng, m.unary("RELU", x), filters, as_slice)]
    return m.finish()


def nasnet(n_labels, size=64, penultimate=96, num_blocks=1, stem_filters=8, seed=0, skip_reduction=True, merge_relus=False,
           as_slice=False, filter_multiplier=2, dense_sizes=(), activation="sigmoid", head_gain=1.0, gain=0.7):
    """-> flatbuffer bytes.  Weights: normal with variance 2 / fan-in times gain^2 (every branch ends in an ADD of two of
    them), biases normal 0.05; BatchNorms folded into the 1 x 1 convolutions, the depthwise filters carry a zero bias.
    size 64 gives maps of 31, 16, 8, 4 and 2 pixels a side: the odd 31 makes the shifted adjust path differ from the plain one."""
    rng = np.random.default_rng(seed)
    m = ModelNAS()
    hw = {}        # tensor id -> pixels a side
    relus = {}

    def relu(x):
        if merge_relus and x in relus:
            return relus[x]
        y = m.unary("RELU", x)
        hw[y] = hw[x]
        relus[x] = y
        return y

    def conv1x1(x, co, act=tb.NONE):
        y = _conv1x1(m, rng, x, co, act, gain)
        hw[y] = hw[x]
        return y

    def depthwise(x, k, stride):
        c = m.shape(x)[3]
        w = rng.normal(0.0, np.sqrt(2.0 / (k * k)), size=(1, k, k, c)).astype(np.float32)
        if stride == 2:
            pd = ts.correct_pad(hw[x], k)
            y = m.depthwise(m.pad(x, [[0, 0], pd, pd, [0, 0]]), w, np.zeros(c, np.float32), 2, tb.VALID, tb.NONE)
            hw[y] = (hw[x] + sum(pd) - k) // 2 + 1
        else:
            y = m.depthwise(x, w, np.zeros(c, np.float32), 1, tb.SAME, tb.NONE)
            hw[y] = hw[x]
        return y

    def sep(x, filters, k, s=1):
        y = conv1x1(depthwise(relu(x), k, s), filters, tb.RELU)
        return conv1x1(depthwise(y, k, 1), filters)

    def pool(kind, x, k, s, padded=None):
        if s == 2:      # on the zero-padded tensor, VALID
            y = m.pool(kind, padded, k, 2, tb.VALID)
            hw[y] = (hw[padded] - k) // 2 + 1
        else:
            y = m.pool(kind, x, k, 1, tb.SAME)
            hw[y] = hw[x]
        return y

    def add(a, b):
        y = m.binary("ADD", a, b)
        hw[y] = hw[a]
        return y

    def adjust(p, ip, filters):
        if p is None:
            p = ip
        if hw[p] != hw[ip]:
            y = adjust_paths(m, rng, relu(p), filters, as_slice)
            hw[y] = (hw[p] - 1) // 2 + 1
            return y
        if m.shape(p)[3] != filters:
            return conv1x1(relu(p), filters)
        return p

    def concat(xs):
        y = m.concat(xs)
        hw[y] = hw[xs[0]]
        return y

    def normal(ip, p, filters):
        p = adjust(p, ip, filters)
        h = conv1x1(relu(ip), filters)
        x1 = add(sep(h, filters, 5), sep(p, filters, 3))
        x2 = add(sep(p, filters, 5), sep(p, filters, 3))
        x3 = add(pool("AVERAGE_POOL_2D", h, 3, 1), p)
        x4 = add(pool("AVERAGE_POOL_2D", p, 3, 1), pool("AVERAGE_POOL_2D", p, 3, 1))
        x5 = add(sep(h, filters, 3), h)
        return concat([p, x1, x2, x3, x4, x5]), ip

    def reduction(ip, p, filters):
        p = adjust(p, ip, filters)
        h = conv1x1(relu(ip), filters)
        pd = ts.correct_pad(hw[h], 3)
        h3 = m.pad(h, [[0, 0], pd, pd, [0, 0]])
        hw[h3] = hw[h] + sum(pd)
        x1 = add(sep(h, filters, 5, 2), sep(p, filters, 7, 2))
        x2 = add(pool("MAX_POOL_2D", h, 3, 2, h3), sep(p, filters, 7, 2))
        x3 = add(pool("AVERAGE_POOL_2D", h, 3, 2, h3), sep(p, filters, 5, 2))
        x4 = add(pool("AVERAGE_POOL_2D", x1, 3, 1), x2)
        x5 = add(sep(x1, filters, 3), pool("MAX_POOL_2D", h, 3, 2, h3))
        return concat([x2, x3, x4, x5]), ip

    filters, f = penultimate // 24, filter_multiplier
    x = m.tensor([1, size, size, 3], name="input")
    m.inputs = [x]
    w = (gain * rng.normal(0.0, np.sqrt(2.0 / 27), size=(stem_filters, 3, 3, 3))).astype(np.float32)
    x = m.conv(x, w, rng.normal(0.0, 0.05, size=stem_filters).astype(np.float32), 2, tb.VALID, tb.NONE)
    hw[x] = (size - 3) // 2 + 1
    p = None
    x, p = reduction(x, p, max(filters // f ** 2, 1))
    x, p = reduction(x, p, max(filters // f, 1))
    for stage in range(3):
        if stage:
            x, p0 = reduction(x, p, filters * f ** stage)
            p = p if skip_reduction else p0
        for _ in range(num_blocks):
            x, p = normal(x, p, filters * f ** stage)
    x = m.mean(m.unary("RELU", x))
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


def inception_resnet_block(size=9, cin=32, seed=0, scale=0.17):
    """-> flatbuffer bytes: one block of the reference's `inceptionresnetv2` family: three branches concatenated, a 1 x 1
    CONV_2D without an activation, the residual scaling as a MUL by the constant `scale`, ADD to the input with a fused RELU."""
    rng = np.random.default_rng(seed)
    m = ts.ModelSE()

    def cbn(x, co, k):
        c = m.shape(x)[3]
        w = rng.normal(0.0, np.sqrt(2.0 / (k * k * c)), size=(co, k, k, c)).astype(np.float32)
        return m.conv(x, w, rng.normal(0.0, 0.05, size=co).astype(np.float32), 1, tb.SAME, tb.RELU)

    x = m.tensor([1, size, size, cin], name="input")
    m.inputs = [x]
    b0 = cbn(x, 8, 1)
    b1 = cbn(cbn(x, 8, 1), 8, 3)
    b2 = cbn(cbn(cbn(x, 8, 1), 12, 3), 16, 3)
    mixed = m.concat([b0, b1, b2])
    w = rng.normal(0.0, np.sqrt(2.0 / 32), size=(cin, 1, 1, 32)).astype(np.float32)
    up = m.conv(mixed, w, rng.normal(0.0, 0.05, size=cin).astype(np.float32), 1, tb.SAME, tb.NONE)
    up = m.binary("MUL", up, np.array([scale], np.float32))
    m.outputs = [m.binary("ADD", x, up, tb.RELU)]
    return m.finish()


def pad_then(reader, pads=((1, 1), (1, 1)), k=3, stride=1, extra_reader=False, as_output=False, hybrid=False, size=9, c=8,
             relu=True, seed=3):
    """-> flatbuffer bytes: (RELU ->) PAD -> reader, VALID: "conv" (CONV_2D), "dw" (DEPTHWISE_CONV_2D) or a pool's name.
    extra_reader: a MAX_POOL_2D reads the padded tensor too; as_output: the padded tensor is the graph's output; hybrid:
    the filter INT8 (tflite_build_dw.quantise)."""
    rng = np.random.default_rng(seed)
    m = td.ModelDW()
    x = m.tensor([1, size, size, c], name="input")
    m.inputs = [x]
    p = m.pad(m.unary("RELU", x) if relu else x, [[0, 0], list(pads[0]), list(pads[1]), [0, 0]])
    if reader == "conv":
        y = m.conv(p, rng.normal(0, 0.3, size=(40 if hybrid else 8, k, k, c)).astype(np.float32), np.zeros(40 if hybrid else 8, np.float32), stride, tb.VALID)
    elif reader == "dw":
        y = m.depthwise(p, rng.normal(0, 0.3, size=(1, k, k, c)).astype(np.float32), np.zeros(c, np.float32), stride, tb.VALID)
    else:
        y = m.pool(reader, p, k, stride, tb.VALID)
    if extra_reader:
        y = m.binary("ADD", y, m.pool("MAX_POOL_2D", p, k, stride, tb.VALID))
    m.outputs = [p if as_output else y]
    blob = m.finish()
    return td.quantise(blob, min_elements=64) if hybrid else blob
