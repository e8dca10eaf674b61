"""Helper (not a test): TFLite flatbuffers of the EfficientNet family, as the converter writes them.  `ModelSE` is
tflite_build_dw.ModelDW with a MUL of two tensors (either may be the [1, 1, 1, C] gate), DIV, MEAN with keep_dims and
HARD_SWISH (which the executor refuses by name); `efficientnet_b0` emits the converter's layout of
tf.keras.applications.EfficientNetB0(include_top=False) -> GlobalAveragePooling2D -> Dense... (the reference's
`efficientnetb0` family, ml_tools/kerasmodel.py:181-216): the in-model Rescaling and Normalization as MUL / SUB / MUL (or DIV)
by constants, BatchNorms folded, a stride-2 convolution as PAD (Keras' correct_pad) + VALID, 3 x 3 and 5 x 5 depthwise
filters, squeeze-and-excite with ratio 0.25, swish as LOGISTIC + MUL, the residual ADD."""
import numpy as np

import tflite_build as tb
import tflite_build_dw as td

tb.CODES.setdefault("DIV", 42)
tb.CODES.setdefault("HARD_SWISH", 117)
tb.OPTION_TYPES.setdefault("DIV", 29)


class ModelSE(td.ModelDW):
    def mul(self, a, b, act=tb.NONE):
        """MUL of two activations, inputs in this order; the output takes the larger shape."""
        sa, sb = self.shape(a), self.shape(b)
        gate_first = len(sa) == 4 and sa[1:3] == [1, 1] and sb[1:3] != [1, 1]
        y = self.tensor(list(sb if gate_first else sa))
        return self.op("MUL", [a, b], [y], {0: ("b", act)})

    def div(self, a, b, act=tb.NONE, const_first=False):
        """DIV: b a tensor id or a constant array; const_first: b / a."""
        if not isinstance(b, (int, np.integer)):
            b = self.tensor(np.shape(b), np.asarray(b, np.float32))
        y = self.tensor(list(self.shape(a)))
        return self.op("DIV", [b, a] if const_first else [a, b], [y], {0: ("b", act)})

    def swish(self, x, logistic_first=False):
        s = self.unary("LOGISTIC", x)
        return self.mul(s, x) if logistic_first else self.mul(x, s)

    def hard_swish(self, x):
        return self.unary("HARD_SWISH", x)


# kernel, repeats, filters in, filters out, expand ratio, stride (tf.keras.applications.efficientnet.DEFAULT_BLOCKS_ARGS)
B0_BLOCKS = ((3, 1, 32, 16, 1, 1), (3, 2, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2), (3, 3, 40, 80, 6, 2), (5, 3, 80, 112, 6, 1),
             (5, 4, 112, 192, 6, 2), (3, 1, 192, 320, 6, 1))


def correct_pad(size, k):
    """Keras' correct_pad for one axis: what ZeroPadding2D puts in front of a stride-2 VALID convolution."""
    return [k // 2 - (1 - size % 2), k // 2]


def efficientnet_b0(n_labels, dense_sizes=(), seed=0, width=1.0, size=224, activation="sigmoid", head_gain=1.0,
                    normalisation_div=False, se_reshape=False, blocks=B0_BLOCKS):
    """-> flatbuffer bytes.  Weights as tflite_build.inception_v3 draws them (normal with variance 2 / fan-in, biases normal
    0.05; the projection behind a gate 1.4 times that deviation, so that activations keep their scale).  `width` is the width coefficient (channel counts to multiples of 8).  normalisation_div: the Normalization's
    1 / sqrt(variance) as a DIV by sqrt(variance); se_reshape: the squeeze as MEAN without keep_dims + RESHAPE to
    [1, 1, 1, C] (older Keras versions)."""
    rng = np.random.default_rng(seed)
    m = ModelSE()

    def ch(c):
        v = max(8, int(c * width + 4) // 8 * 8)
        return v + 8 if v < 0.9 * c * width else v

    def conv(x, co, k, stride=1, swish=True, logistic=False, padding=tb.SAME, gain=1.0):
        cin = m.shape(x)[3]
        w = (gain * rng.normal(0.0, np.sqrt(2.0 / (k * k * cin)), size=(co, k, k, cin))).astype(np.float32)
        y = m.conv(x, w, rng.normal(0.0, 0.05, size=co).astype(np.float32), stride, padding, tb.NONE)
        if logistic:
            return m.unary("LOGISTIC", y)
        return m.swish(y) if swish else y

    def depthwise(x, k, stride, hw):
        c = m.shape(x)[3]
        w = rng.normal(0.0, np.sqrt(2.0 / (k * k)), size=(1, k, k, c)).astype(np.float32)
        b = rng.normal(0.0, 0.05, size=c).astype(np.float32)
        if stride == 2:
            x = m.pad(x, [[0, 0], correct_pad(hw, k), correct_pad(hw, k), [0, 0]])
            return m.swish(m.depthwise(x, w, b, 2, tb.VALID, tb.NONE))
        return m.swish(m.depthwise(x, w, b, 1, tb.SAME, tb.NONE))

    x = m.tensor([1, size, size, 3], name="input")
    m.inputs = [x]
    # Rescaling(1 / 255) and Normalization (the ImageNet statistics), per channel
    x = m.binary("MUL", x, np.array([1.0 / 255.0], np.float32))
    x = m.binary("SUB", x, np.array([0.485, 0.456, 0.406], np.float32))
    sd = np.sqrt(np.array([0.229, 0.224, 0.225], np.float64) ** 2)
    x = m.div(x, sd.astype(np.float32)) if normalisation_div else m.binary("MUL", x, (1.0 / sd).astype(np.float32))
    hw = size
    x = conv(m.pad(x, [[0, 0], correct_pad(hw, 3), correct_pad(hw, 3), [0, 0]]), ch(32), 3, 2, padding=tb.VALID)
    hw = (hw + 1) // 2
    for k, repeats, fin, fout, expand, stride in blocks:
        for r in range(repeats):
            cin, s = m.shape(x)[3], stride if r == 0 else 1
            y = x if expand == 1 else conv(x, cin * expand, 1)
            y = depthwise(y, k, s, hw)
            hw = (hw + 1) // 2 if s == 2 else hw
            c = m.shape(y)[3]
            if se_reshape:
                g = m.reshape(m.mean(y), [1, 1, 1, c])
            else:
                g = m.mean(y, keep_dims=True)
            g = conv(conv(g, max(1, int(cin * 0.25)), 1), c, 1, logistic=True)
            y = conv(m.mul(y, g), ch(fout), 1, swish=False, gain=1.4)   # (the gate is about 1 / 2)
            x = m.binary("ADD", y, x) if s == 1 and cin == ch(fout) else y
    x = conv(x, ch(1280), 1)
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
