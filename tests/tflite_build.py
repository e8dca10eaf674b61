"""Helper (not a test): writes float32 TFLite flatbuffers for the operator set cpx/ml_tools/tflite_reader.py reads, laid
out as the TFLite converter writes them -- TensorFlow is not needed.  `Model` collects tensors and operators and
serialises them; `inception_v3` emits the converter's layout of the reference's inceptionv3 family
(ml_tools/kerasmodel.py:171-180,259-350: tf.keras.applications.InceptionV3(include_top=False) -> GlobalAveragePooling2D
-> Dense(relu)... -> Dense(n_labels, sigmoid | softmax)): every convolution with its BatchNorm folded into filter and
bias and ReLU fused; `wrresnet` writes the WR-ResNet-22-4 of cpx/ml_tools/wrresnet.py, grouped filters included."""
import struct

import numpy as np

CODES = {"ADD": 0, "AVERAGE_POOL_2D": 1, "CONCATENATION": 2, "CONV_2D": 3, "DEPTHWISE_CONV_2D": 4, "FULLY_CONNECTED": 9,
         "LOGISTIC": 14, "MAX_POOL_2D": 17, "MUL": 18, "RELU": 19, "RELU6": 21, "RESHAPE": 22, "SOFTMAX": 25, "PAD": 34,
         "MEAN": 40, "SUB": 41, "TANH": 28}
# BuiltinOptions union members (schema.fbs)
OPTION_TYPES = {"CONV_2D": 1, "DEPTHWISE_CONV_2D": 2, "AVERAGE_POOL_2D": 5, "MAX_POOL_2D": 5, "FULLY_CONNECTED": 8,
                "SOFTMAX": 9, "CONCATENATION": 10, "ADD": 11, "RESHAPE": 17, "MUL": 21, "PAD": 22, "MEAN": 27, "SUB": 28}
FLOAT32, INT32, UINT8 = 0, 2, 3
SAME, VALID = 0, 1
NONE, RELU, RELU6 = 0, 1, 3


class _Writer:
    """Forward-only flatbuffer serialiser: a table is written with zeroed offset slots, each child right after it, and the
    slot is patched with the distance."""

    def __init__(self):
        self.b = bytearray(b"\0\0\0\0TFL3")

    def pad(self, n=4):
        self.b += b"\0" * (-len(self.b) % n)

    def scalars(self, fmt, values):
        self.pad()
        pos = len(self.b)
        self.b += struct.pack("<I%d%s" % (len(values), fmt), len(values), *values)
        return pos

    def raw(self, data, terminator=b""):
        self.pad()
        pos = len(self.b)
        self.b += struct.pack("<I", len(data)) + bytes(data) + terminator
        return pos

    def tables(self, writers):
        self.pad()
        pos = len(self.b)
        self.b += struct.pack("<I", len(writers)) + b"\0\0\0\0" * len(writers)
        for k, w in enumerate(writers):
            slot = pos + 4 + 4 * k
            struct.pack_into("<I", self.b, slot, w() - slot)
        return pos

    def table(self, fields):
        """fields: {field id: (struct code, value) | ("ref", callable that writes the child and returns its position)}."""
        self.pad()
        n = max(fields) + 1 if fields else 0
        sizes = {"I": 4, "i": 4, "f": 4, "b": 1, "B": 1, "ref": 4}
        body, offs, refs, cur = bytearray(), [0] * n, [], 4
        for fid in sorted(fields, key=lambda f: -sizes[fields[f][0]]):   # widest first: no padding inside
            kind, val = fields[fid]
            offs[fid] = cur
            if kind == "ref":
                refs.append((cur, val))
                body += b"\0\0\0\0"
            else:
                body += struct.pack("<" + kind, val)
            cur += sizes[kind]
        vt_pos = len(self.b)
        self.b += struct.pack("<HH%dH" % n, 4 + 2 * n, 4 + len(body), *offs)
        self.pad()
        pos = len(self.b)
        self.b += struct.pack("<i", pos - vt_pos) + body
        for rel, w in refs:
            struct.pack_into("<I", self.b, pos + rel, w() - (pos + rel))
        return pos


class Model:
    def __init__(self):
        self.tensors, self.buffers, self.ops = [], [b""], []
        self.inputs, self.outputs = [], []

    def tensor(self, shape, data=None, name="t", ttype=None):
        bi = 0
        if data is not None:
            data = np.asarray(data)
            if ttype is None:
                ttype = FLOAT32 if data.dtype.kind == "f" else INT32
            self.buffers.append(np.ascontiguousarray(data, "<f4" if ttype == FLOAT32 else "<i4").tobytes())
            bi = len(self.buffers) - 1
        self.tensors.append((list(shape), FLOAT32 if ttype is None else ttype, bi, name))
        return len(self.tensors) - 1

    def op(self, name, inputs, outputs, options=None, code=None):
        """options: {field id: (struct code, value) | ("ints", [..])} of the operator's options table."""
        self.ops.append((CODES[name] if code is None else code, list(inputs), list(outputs), OPTION_TYPES.get(name, 0), options))
        return outputs[0]

    def shape(self, t):
        return self.tensors[t][0]

    # ---- the operators, with the converter's option layout ----
    def conv(self, x, w_ohwi, bias, stride=1, padding=SAME, act=NONE, dilation=1, name="CONV_2D"):
        w_ohwi = np.asarray(w_ohwi, np.float32)
        y = self.tensor([1, 0, 0, w_ohwi.shape[0]])
        ins = [x, self.tensor(w_ohwi.shape, w_ohwi)] + ([] if bias is None else [self.tensor(bias.shape, bias)])
        sh, sw = (stride, stride) if np.isscalar(stride) else stride
        opts = {0: ("b", padding), 1: ("i", sw), 2: ("i", sh), 3: ("b", act)}
        if name == "CONV_2D":
            opts.update({4: ("i", dilation), 5: ("i", dilation)})
        return self.op(name, ins, [y], opts)

    def pool(self, kind, x, k, stride, padding, act=NONE):
        kh, kw = (k, k) if np.isscalar(k) else k
        sh, sw = (stride, stride) if np.isscalar(stride) else stride
        y = self.tensor([1, 0, 0, self.shape(x)[3]])
        return self.op(kind, [x], [y], {0: ("b", padding), 1: ("i", sw), 2: ("i", sh), 3: ("i", kw), 4: ("i", kh), 5: ("b", act)})

    def concat(self, xs, axis=3, act=NONE):
        y = self.tensor([1, 0, 0, sum(self.shape(x)[3] for x in xs)])
        return self.op("CONCATENATION", xs, [y], {0: ("i", axis), 1: ("b", act)})

    def binary(self, name, a, b, act=NONE, const_first=False):
        """b: a tensor id or a constant array."""
        if not isinstance(b, (int, np.integer)):
            b = self.tensor(np.shape(b), np.asarray(b, np.float32))
        y = self.tensor(list(self.shape(a)))
        return self.op(name, [b, a] if const_first else [a, b], [y], {0: ("b", act)})

    def unary(self, name, x, options=None):
        y = self.tensor(list(self.shape(x)))
        return self.op(name, [x], [y], options)

    def softmax(self, x, beta=1.0):
        return self.unary("SOFTMAX", x, {0: ("f", beta)})

    def mean(self, x, axes=(1, 2), keep_dims=False):
        c = self.shape(x)[3]
        y = self.tensor([1, 1, 1, c] if keep_dims else [1, c])
        return self.op("MEAN", [x, self.tensor([len(axes)], np.array(axes, np.int32))], [y], {0: ("b", 1 if keep_dims else 0)})

    def dense(self, x, w_out_in, bias, act=NONE):
        y = self.tensor([1, w_out_in.shape[0]])
        return self.op("FULLY_CONNECTED", [x, self.tensor(w_out_in.shape, w_out_in), self.tensor(bias.shape, bias)], [y],
                       {0: ("b", act)})

    def reshape(self, x, shape):
        y = self.tensor(list(shape))
        return self.op("RESHAPE", [x, self.tensor([len(shape)], np.array(shape, np.int32))], [y], {0: ("ints", list(shape))})

    def pad(self, x, paddings):
        s = self.shape(x)
        y = self.tensor([1, 0, 0, s[3]])
        return self.op("PAD", [x, self.tensor([4, 2], np.array(paddings, np.int32))], [y], {})

    # ---- serialise ----
    def finish(self):
        w = _Writer()
        code_list = sorted(set(o[0] for o in self.ops))

        def tensor_w(t):
            shape, ttype, bi, name = t
            return lambda: w.table({0: ("ref", lambda: w.scalars("i", shape)), 1: ("b", ttype), 2: ("I", bi),
                                    3: ("ref", lambda: w.raw(name.encode(), b"\0"))})

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
            return w.table({0: ("ref", lambda: w.tables([tensor_w(t) for t in self.tensors])),
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


def inception_v3(n_labels, dense_sizes=(), seed=0, width=1.0, size=160, activation="sigmoid", head_gain=1.0):
    """-> flatbuffer bytes.  Weights: normal with variance 2 / fan-in, biases normal 0.05 -- activations keep their scale
    through the 94 convolutions.  `width` scales every channel count (to multiples of 4); head_gain scales the last Dense's
    weights (the spread of the logits)."""
    rng = np.random.default_rng(seed)
    m = Model()

    def ch(c):
        return max(4, int(round(c * width / 4.0)) * 4)

    def cbn(x, filters, kh, kw, stride=1, padding=SAME):
        cin = m.shape(x)[3]
        co = ch(filters)
        w = rng.normal(0.0, np.sqrt(2.0 / (kh * kw * cin)), size=(co, kh, kw, cin)).astype(np.float32)
        b = rng.normal(0.0, 0.05, size=co).astype(np.float32)
        return m.conv(x, w, b, stride, padding, RELU)

    x = m.tensor([1, size, size, 3], name="input")
    m.inputs = [x]
    x = cbn(x, 32, 3, 3, 2, VALID)
    x = cbn(x, 32, 3, 3, 1, VALID)
    x = cbn(x, 64, 3, 3)
    x = m.pool("MAX_POOL_2D", x, 3, 2, VALID)
    x = cbn(x, 80, 1, 1, 1, VALID)
    x = cbn(x, 192, 3, 3, 1, VALID)
    x = m.pool("MAX_POOL_2D", x, 3, 2, VALID)
    for pool_ch in (32, 64, 64):    # mixed 0, 1, 2
        b1 = cbn(x, 64, 1, 1)
        b5 = cbn(cbn(x, 48, 1, 1), 64, 5, 5)
        b3 = cbn(cbn(cbn(x, 64, 1, 1), 96, 3, 3), 96, 3, 3)
        bp = cbn(m.pool("AVERAGE_POOL_2D", x, 3, 1, SAME), pool_ch, 1, 1)
        x = m.concat([b1, b5, b3, bp])
    b3 = cbn(x, 384, 3, 3, 2, VALID)   # mixed 3
    bd = cbn(cbn(cbn(x, 64, 1, 1), 96, 3, 3), 96, 3, 3, 2, VALID)
    x = m.concat([b3, bd, m.pool("MAX_POOL_2D", x, 3, 2, VALID)])
    for c7 in (128, 160, 160, 192):    # mixed 4 .. 7
        b1 = cbn(x, 192, 1, 1)
        b7 = cbn(cbn(cbn(x, c7, 1, 1), c7, 1, 7), 192, 7, 1)
        bd = cbn(cbn(cbn(cbn(cbn(x, c7, 1, 1), c7, 7, 1), c7, 1, 7), c7, 7, 1), 192, 1, 7)
        bp = cbn(m.pool("AVERAGE_POOL_2D", x, 3, 1, SAME), 192, 1, 1)
        x = m.concat([b1, b7, bd, bp])
    b3 = cbn(cbn(x, 192, 1, 1), 320, 3, 3, 2, VALID)   # mixed 8
    b7 = cbn(cbn(cbn(cbn(x, 192, 1, 1), 192, 1, 7), 192, 7, 1), 192, 3, 3, 2, VALID)
    x = m.concat([b3, b7, m.pool("MAX_POOL_2D", x, 3, 2, VALID)])
    for _ in range(2):                 # mixed 9, 10: the nested concatenations
        b1 = cbn(x, 320, 1, 1)
        t = cbn(x, 384, 1, 1)
        b3 = m.concat([cbn(t, 384, 1, 3), cbn(t, 384, 3, 1)])
        t = cbn(cbn(x, 448, 1, 1), 384, 3, 3)
        bd = m.concat([cbn(t, 384, 1, 3), cbn(t, 384, 3, 1)])
        bp = cbn(m.pool("AVERAGE_POOL_2D", x, 3, 1, SAME), 192, 1, 1)
        x = m.concat([b1, b3, bd, bp])
    x = m.mean(x)
    for d in dense_sizes:
        cin = m.shape(x)[1]
        x = m.dense(x, rng.normal(0.0, np.sqrt(2.0 / cin), size=(d, cin)).astype(np.float32),
                    rng.normal(0.0, 0.05, size=d).astype(np.float32), RELU)
    cin = m.shape(x)[1]
    logits = m.dense(x, (head_gain * rng.normal(0.0, np.sqrt(2.0 / cin), size=(n_labels, cin))).astype(np.float32),
                     rng.normal(0.0, 0.05, size=n_labels).astype(np.float32))
    out = m.softmax(logits) if activation == "softmax" else m.unary("LOGISTIC", logits)
    m.outputs = [out]
    return m.finish()


def wrresnet(w, hidden=(), size=160):
    """The converter's layout of the WR-ResNet-22-4 with cpx weights `w` (Keras layout, cpx.ml_tools.wrresnet): BatchNorms
    in front of a block as MUL + ADD(relu), the BatchNorm between a block's convolutions folded into the first, grouped
    filters (OHWI with I = Cin / 2) -- the inverse of tools/tflite_to_npz.py's weight mapping, with the dataflow of
    oracle/cnn_oracle.forward: the shortcut reads the block's raw input and ReLU follows the residual ADD."""
    from cpx.ml_tools.wrresnet import bn_affine

    m = Model()

    def conv(x, kernel_hwio, bias, stride, same, relu):
        return m.conv(x, np.transpose(kernel_hwio, (3, 0, 1, 2)), np.asarray(bias, np.float32), stride, SAME if same else VALID,
                      RELU if relu else NONE)

    def affine(x, scale, shift):
        return m.binary("ADD", m.binary("MUL", x, scale), shift, RELU)

    x = m.tensor([1, size, size, 2], name="input")
    m.inputs = [x]
    cur = conv(x, w["conv1_1/kernel"], w["conv1_1/bias"], 1, True, False)
    for stage in (2, 3, 4):
        for d in range(3):
            b = "%db%d" % (stage, d)
            s = (stage - 1) if d == 0 else 1
            act = affine(cur, *bn_affine(w, "bn%s_branch2a" % b))
            sc2, sh2 = bn_affine(w, "bn%s_branch2b" % b)
            ka = (w["res%s_branch2a/kernel" % b] * sc2[None, None, None, :]).astype(np.float32)
            ba = (w["res%s_branch2a/bias" % b] * sc2 + sh2).astype(np.float32)
            short = cur
            if d == 0:
                short = conv(cur, w["shortcut%d/kernel" % stage], w["shortcut%d/bias" % stage], s, False, False)
            mid = conv(act, ka, ba, s, True, True)
            out = conv(mid, w["res%s_branch2b/kernel" % b], w["res%s_branch2b/bias" % b], 1, True, False)
            cur = m.binary("ADD", out, short, RELU)
    cur = affine(cur, *bn_affine(w, "final_bn"))
    cur = m.mean(cur)
    for i in range(len(hidden)):
        cur = m.dense(cur, np.ascontiguousarray(w["dense_%d/kernel" % i].T), w["dense_%d/bias" % i], RELU)
    logits = m.dense(cur, np.ascontiguousarray(w["prediction/kernel"].T), w["prediction/bias"])
    out = m.softmax(logits) if w.get("prediction/activation") == "softmax" else m.unary("LOGISTIC", logits)
    m.outputs = [out]
    return m.finish()
