"""Helper (not a test): TFLite flatbuffers of the pre-activation families, as the converter writes them, with the writer
of tests/tflite_build.py.  A pre-activation is a BatchNorm + ReLU IN FRONT of a convolution, on a tensor that has other
readers (the next concatenation, the shortcut): MUL by a constant, then ADD of a constant with a fused RELU.
`densenet` emits the layout of tf.keras.applications.DenseNet121(include_top=False) -> GlobalAveragePooling2D -> Dense
(the reference's `densenet121` family, ml_tools/kerasmodel.py:103-222) with any block sizes and growth rate, `densenet121`
the full layout; `resnet_v2` a stem and bottleneck blocks of ResNet50V2, the first with the projection shortcut that
reads the pre-activation beside conv1; `preact_conv` one pre-activation in front of one convolution."""
import numpy as np

import tflite_build as tb

F32 = np.float32


def _conv_w(rng, co, k, cin, gain=1.0, bias=True):
    w = (gain * rng.normal(0.0, np.sqrt(2.0 / (k * k * cin)), size=(co, k, k, cin))).astype(F32)
    return w, (rng.normal(0.0, 0.05, size=co).astype(F32) if bias else None)


def preact(m, rng, x, act=tb.RELU, shift=None):
    """BatchNorm + activation in front of a convolution: MUL + ADD by per-channel constants, the activation fused."""
    c = m.shape(x)[3]
    scale = rng.uniform(0.6, 1.4, size=c).astype(F32)
    shift = rng.normal(0.0, 0.3, size=c).astype(F32) if shift is None else np.asarray(shift, F32)
    return m.binary("ADD", m.binary("MUL", x, scale), shift, act)


def head(m, rng, x, n_labels, head_gain, activation="sigmoid"):
    x = m.mean(preact(m, rng, x))
    cin = m.shape(x)[1]
    logits = m.dense(x, (head_gain * rng.normal(0.0, np.sqrt(2.0 / cin), size=(n_labels, cin))).astype(F32),
                     rng.normal(0.0, 0.05, size=n_labels).astype(F32))
    return m.softmax(logits) if activation == "softmax" else m.unary("LOGISTIC", logits)


def densenet(n_labels, blocks=(2, 2), growth=8, stem=16, size=32, seed=0, head_gain=1.0, stem_gain=1.0, activation="sigmoid"):
    """-> flatbuffer bytes.  Stem: PAD 3 + CONV 7 x 7 stride 2 VALID (BatchNorm folded, RELU fused) + PAD 1 + MAX_POOL 3 x 3
    stride 2 VALID.  Dense layer: [MUL, ADD+RELU, CONV 1 x 1 to 4 x growth (the BatchNorm behind it folded, RELU fused),
    CONV 3 x 3 SAME to growth, CONCATENATION of the layer's input and that].  Transition: [MUL, ADD+RELU, CONV 1 x 1 to half
    the channels, AVERAGE_POOL 2 x 2].  Then MUL / ADD+RELU, MEAN, FULLY_CONNECTED, LOGISTIC."""
    rng = np.random.default_rng(seed)
    m = tb.Model()
    x = m.tensor([1, size, size, 3], name="input")
    m.inputs = [x]
    x = m.pad(x, [[0, 0], [3, 3], [3, 3], [0, 0]])
    x = m.conv(x, *_conv_w(rng, stem, 7, 3, gain=stem_gain), 2, tb.VALID, tb.RELU)
    x = m.pool("MAX_POOL_2D", m.pad(x, [[0, 0], [1, 1], [1, 1], [0, 0]]), 3, 2, tb.VALID)
    for b, layers in enumerate(blocks):
        for _ in range(layers):
            c = m.shape(x)[3]
            y = m.conv(preact(m, rng, x), *_conv_w(rng, 4 * growth, 1, c), 1, tb.SAME, tb.RELU)
            y = m.conv(y, *_conv_w(rng, growth, 3, 4 * growth, bias=False), 1, tb.SAME, tb.NONE)
            x = m.concat([x, y])
        if b + 1 < len(blocks):
            c = m.shape(x)[3]
            y = m.conv(preact(m, rng, x), *_conv_w(rng, c // 2, 1, c, bias=False), 1, tb.SAME, tb.NONE)
            x = m.pool("AVERAGE_POOL_2D", y, 2, 2, tb.VALID)
    m.outputs = [head(m, rng, x, n_labels, head_gain, activation)]
    return m.finish()


def densenet121(n_labels, size=160, seed=0, head_gain=1.0):
    """The full layout: blocks of 6, 12, 24 and 16 layers, growth 32, a stem of 64 channels: 120 convolutions and 62
    pre-activations (58 dense layers, 3 transitions, the final one in front of MEAN)."""
    return densenet(n_labels, blocks=(6, 12, 24, 16), growth=32, stem=64, size=size, seed=seed, head_gain=head_gain)


def resnet_v2(n_labels, size=32, filters=8, seed=0, head_gain=1.0, stem_gain=1.0):
    """-> flatbuffer bytes.  Stem: CONV 3 x 3 stride 2 (ResNetV2's stem has no BatchNorm), PAD 1 + MAX_POOL 3 x 3
    stride 2, then two bottleneck blocks of
    ResNet50V2 (keras.applications.resnet_v2: block2): preact = RELU(BN(x)); the first block's shortcut is CONV 1 x 1 of
    preact -- so the pre-activation feeds TWO convolutions --, the second's is x itself; CONV 1 x 1 (BN folded, RELU),
    PAD 1 + CONV 3 x 3 VALID (BN folded, RELU), CONV 1 x 1; ADD.  Then post-BN + RELU, MEAN, FULLY_CONNECTED, LOGISTIC."""
    rng = np.random.default_rng(seed)
    m = tb.Model()
    x = m.tensor([1, size, size, 3], name="input")
    m.inputs = [x]
    x = m.conv(x, *_conv_w(rng, 4 * filters, 3, 3, gain=stem_gain), 2, tb.SAME, tb.NONE)
    x = m.pool("MAX_POOL_2D", m.pad(x, [[0, 0], [1, 1], [1, 1], [0, 0]]), 3, 2, tb.VALID)
    for project in (True, False):
        c = m.shape(x)[3]
        p = preact(m, rng, x)
        short = m.conv(p, *_conv_w(rng, 4 * filters, 1, c), 1, tb.SAME, tb.NONE) if project else x
        y = m.conv(p, *_conv_w(rng, filters, 1, c, bias=False), 1, tb.SAME, tb.RELU)
        y = m.conv(m.pad(y, [[0, 0], [1, 1], [1, 1], [0, 0]]), *_conv_w(rng, filters, 3, filters, bias=False), 1, tb.VALID, tb.RELU)
        y = m.conv(y, *_conv_w(rng, 4 * filters, 1, filters), 1, tb.SAME, tb.NONE)
        x = m.binary("ADD", short, y)
    m.outputs = [head(m, rng, x, n_labels, head_gain)]
    return m.finish()


def preact_conv(rng, k, stride, padding, cin, cout, size, act=tb.RELU, shift=None, c_total=None, c_from=0):
    """input -> MUL, ADD+act -> CONV_2D k x k -> output; -> (blob, the pre-activation's tensor, the convolution's output
    tensor).  c_total: the graph's input has c_total channels and the pre-activation reads the channels
    [c_from, c_from + cin) of a c_total-channel concatenation of three 1 x 1 convolutions of it."""
    m = tb.Model()
    cx = cin if c_total is None else c_total
    x = m.tensor([1, size, size, cx], name="input")
    m.inputs = [x]
    src = x
    if c_total is not None:
        parts = [m.conv(x, *_conv_w(rng, c, 1, cx), 1, tb.SAME, tb.NONE) for c in (c_from, cin, c_total - c_from - cin)]
        m.concat(parts)
        src = parts[1]
    p = preact(m, rng, src, act=act, shift=shift)
    y = m.conv(p, *_conv_w(rng, cout, k, cin), stride, padding, tb.NONE)
    m.outputs = [y]
    return m.finish(), p, y
