"""Helper (not a test): full-integer flatbuffers with the EfficientNet family's operators -- an INT8 LOGISTIC, the swish
(LOGISTIC + MUL of one x) and the MUL by a squeeze-and-excite gate -- built operator by operator with hand-chosen scales
and zero points (ModelI8SE on tflite_build_i8.ModelI8), and the small EfficientNet-B0 the whole-network tests share."""
import numpy as np

import tflite_build as tb
import tflite_build_i8 as ti
import tflite_build_se as ts

LOGISTIC_QP = (np.float32(1.0 / 256.0), -128)   # what the converter fixes for a LOGISTIC's output
SMALL_BLOCKS = ((3, 1, 32, 16, 1, 1), (3, 1, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2))


class ModelI8SE(ti.ModelI8):
    def logistic_i8(self, x, out_qp=LOGISTIC_QP):
        return self._retype(self.unary("LOGISTIC", x), out_qp)

    def swish_i8(self, x, out_qp, l_qp=LOGISTIC_QP, act=tb.NONE, logistic_first=False):
        """y = MUL(x, LOGISTIC(x)), the operands in either order."""
        return self.binary_i8("MUL", x, self.logistic_i8(x, l_qp), out_qp, act, const_first=logistic_first)

    def gate_mul_i8(self, x, gate, out_qp, act=tb.NONE, gate_first=False):
        """[H, W, C] by the [1, 1, C] gate; the output has x's shape."""
        return self.binary_i8("MUL", x, gate, out_qp, act, const_first=gate_first)

    def reshape_i8(self, x, shape):
        return self._retype(self.reshape(x, shape), self.qp(x))


# the input tensors of the convolution cases: a zero point inside the range and a POSITIVE one -- a padded tap staged as 0
# instead of z_in shows at every border
IN_QPS = ((np.float32(0.03), 3), (np.float32(0.017), 90))


def levels(rng, shape, qp, every=False):
    """float32 samples that sit exactly on the levels of (scale, zero point), every level of [-128, 127] equally likely,
    both ends present.  every: the values -128, -127, ... in order as far as the tensor holds them (all 256 from 256
    elements on), 127 last."""
    q = rng.integers(-128, 128, size=shape)
    q.reshape(-1)[:2] = (-128, 127)
    if every:
        n = min(256, q.size)
        q.reshape(-1)[:n] = np.arange(-128, 128)[:n]
        q.reshape(-1)[-1] = 127
    return (np.float32(qp[0]) * (q - qp[1]).astype(np.float32)).astype(np.float32)


def random_filter(rng, shape, k_products, in_qp, s_out, per_channel_axis=0):
    """-> (int8 filter, per-channel scales, int32 bias): the filter scales are chosen so that the accumulators' spread is
    about 60 steps of the GIVEN output scale."""
    w = rng.integers(-127, 128, size=shape).astype(np.int8)
    co = shape[per_channel_axis]
    spread = np.sqrt(k_products) * 74.0 * 73.0
    ws = (rng.uniform(0.5, 1.5, size=co) * 60.0 * float(s_out) / (float(in_qp[0]) * spread)).astype(np.float32)
    bias = rng.integers(-int(spread / 2), int(spread / 2) + 1, size=co).astype(np.int32)
    return w, ws, bias


def start(shape, qp):
    """-> (model, the INT8 tensor behind the QUANTIZE of a float32 input of `shape`)."""
    m = ModelI8SE()
    x = m.tensor(list(shape), name="input")
    m.inputs = [x]
    return m, m.quantize(x, qp)


finish = ti.finish


def small_efficientnet(float_tail=True):
    """The stem, four MBConv blocks with squeeze-and-excite (3 x 3 and 5 x 5 depthwise, two of them behind a PAD at stride
    2, one residual ADD) and the head of an EfficientNet-B0 at 32 x 32, through quantise_full with four calibration samples
    of 0 .. 255."""
    blob = ts.efficientnet_b0(5, seed=1, size=32, blocks=SMALL_BLOCKS)
    return ti.quantise_full(blob, np.random.default_rng(0).uniform(0, 255, size=(4, 32, 32, 3)), float_tail=float_tail)


def swishes_and_gates(g):
    """-> ([(LOGISTIC index, MUL index, x)] of the graph's swishes, [LOGISTIC index] of the other interior INT8 LOGISTICs),
    read off the flatbuffer alone."""
    readers = {}
    for i, op in enumerate(g.ops):
        for t in op["inputs"]:
            readers.setdefault(t, []).append(i)
    swishes, lone = [], []
    for i, op in enumerate(g.ops):
        if op["name"] != "LOGISTIC" or g.tensors[op["outputs"][0]]["type"] != ti.INT8:
            continue
        x, s = op["inputs"][0], op["outputs"][0]
        r = readers.get(s, [])
        if len(r) == 1 and g.ops[r[0]]["name"] == "MUL" and sorted(g.ops[r[0]]["inputs"]) == sorted((x, s)):
            swishes.append((i, r[0], x))
        elif not any(g.ops[k]["name"] == "DEQUANTIZE" for k in r):
            lone.append(i)
    return swishes, lone
