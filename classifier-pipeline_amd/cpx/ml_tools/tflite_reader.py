"""Pure-Python reader of float32 and dynamic-range quantised TFLite models (.tflite).  The flatbuffer is parsed here -- TensorFlow is not needed,
only NumPy.  Two users:

* `Graph` decodes subgraph 0 of any float32 model made of the operators in OPS below, with their options: CONV_2D
  (dilation 1 only), DEPTHWISE_CONV_2D (filter [1, kh, kw, C]; depth multiplier 1 and dilation 1 only), AVERAGE_POOL_2D, MAX_POOL_2D, CONCATENATION, ADD, SUB, MUL, DIV, RELU, RELU6, MEAN, FULLY_CONNECTED,
  LOGISTIC, SOFTMAX, RESHAPE, PAD, STRIDED_SLICE, SLICE (over H and W, resolved on the host by resolve_slice into start,
  stride and count per axis; a NASNet's Cropping2D).  That is the set the converter writes for the reference's `inceptionv3` family
  (ml_tools/kerasmodel.py:171-180,259-350; the artefact the reference's CI classifies with, .github/workflows/
  release.yml:46 `inc3-tflite-15122023.tar`, is one), for its `mobilenet` family (MobileNetV2, kerasmodel.py:144-151) and
  for its `efficientnetb0` / `b1` / `b5` / `efficientnetv2b3` families (kerasmodel.py:181-216: swish as LOGISTIC + MUL of two
  activations, the squeeze-and-excite gate as a broadcasting MUL, the in-model Rescaling / Normalization as MUL / SUB /
  ADD / DIV by constants; HARD_SWISH is refused by name).  cpx/ml_tools/tflite_graph.py plans such a graph for the device
  executor (cpx_graph_*), the LiteInterpreter of cpx/ml_tools/interpreter.py runs it -- what the reference's
  LiteInterpreter does with any `.tflite` (src/ml_tools/interpreter.py:520-560,597-628).  A dynamic-range quantised file
  (what the reference's converter writes, src/tfliteconverter.py:54-62: the filters of CONV_2D / DEPTHWISE_CONV_2D / FULLY_CONNECTED
  with 1024 or more elements INT8 with symmetric scales -- along dimension 0, a depthwise filter's along dimension 3 --
  everything else float32) is read too: an INT8 constant comes with its quantisation table (`quant`: scale, zero_point,
  dim), FULLY_CONNECTED with asymmetric_quantize_inputs.
  check_executable() refuses everything else by operator name and index: a depth multiplier, quantised activations,
  UINT8 / INT16 or asymmetric filters, an INT8 constant anywhere but as such a filter, DEQUANTIZE / QUANTIZE
  (check_executable(integer=True) lets a full-integer graph through -- what the converter writes when it is given a
  representative dataset: INT8 activations with one scale and one zero point, INT32 biases, INT8 constants as operands of
  ADD / SUB / MUL, QUANTIZE / DEQUANTIZE at the two ends; cpx/ml_tools/tflite_graph_i8.py plans it.  A DEQUANTIZE of a FLOAT16
  constant, the converter's float16 mode, is folded on load into a float32 constant either way), grouped
  CONV_2D (check_executable(grouped=True) lets one through where the filter depth divides the input depth and the groups
  divide the output channels: the graph executor's CONV_GROUPED / CONV_Q8_GROUPED), a dynamic shape, an operator outside
  the set.
* `convert` / `load_tflite` walk ONE topology, a WR-ResNet-22-4, into the Keras-layout weights of
  cpx/ml_tools/wrresnet.py (the fused MFMA network); get_interpreter on such a path converts on load,
  tools/tflite_to_npz.py writes the same arrays to an .npz.  A dynamic-range quantised file is refused by the name of its
  first INT8 tensor unless quantised_math="float" is given, which multiplies the filters out, float32(int8) * scale
  (get_interpreter does under CPX_TFLITE_QUANT_MATH=float; by default it hands such a file to the graph executor).

What is read: the float32 graph of WR-ResNet-22-4 (src/ml_tools/resnet/wr_resnet.py:5-98) as the TFLite converter
writes it -- CONV_2D (filter OHWI, bias, fused ReLU: a convolution with the BatchNorm that follows it folded in), MUL +
ADD by per-channel constants (a BatchNorm that follows a residual ADD cannot be folded: scale and shift), RELU, ADD of
two activations (the residual, with or without the ReLU behind it fused; the 1 x 1 shortcut in front of the block's
BatchNorm, behind it or behind the main branch), MEAN (global average pooling), FULLY_CONNECTED, LOGISTIC / SOFTMAX.  The walk follows
the operators in order and fills the Keras-layout names; a folded or affine-only BatchNorm becomes gamma = scale,
beta = shift, moving_mean = 0, moving_variance = 1 - eps (so that the loader's gamma / sqrt(var + eps) gives the scale
back exactly).  Anything else (quantised tensors, another topology) is refused with the operator that stopped the walk."""
import struct

import numpy as np

BN_EPS = np.float32(1e-3)
OPS = {0: "ADD", 1: "AVERAGE_POOL_2D", 2: "CONCATENATION", 3: "CONV_2D", 4: "DEPTHWISE_CONV_2D", 9: "FULLY_CONNECTED", 14: "LOGISTIC",
       17: "MAX_POOL_2D", 18: "MUL", 19: "RELU", 21: "RELU6", 25: "SOFTMAX", 40: "MEAN", 41: "SUB", 22: "RESHAPE", 34: "PAD",
       42: "DIV", 45: "STRIDED_SLICE", 65: "SLICE", 6: "DEQUANTIZE", 114: "QUANTIZE"}
SLICE_OPS = ("STRIDED_SLICE", "SLICE")
# the two ends of a full-integer graph: run with check_executable(integer=True) only, refused by name without
INTEGER_OPS = ("DEQUANTIZE", "QUANTIZE")
# operators that are recognised only to be refused by name (check_executable)
REFUSED_OPS = {67: "TRANSPOSE_CONV", 23: "RESIZE_BILINEAR", 28: "TANH", 39: "TRANSPOSE", 32: "CUSTOM", 117: "HARD_SWISH"}
TENSOR_TYPES = {0: "FLOAT32", 1: "FLOAT16", 2: "INT32", 3: "UINT8", 4: "INT64", 6: "BOOL", 7: "INT16", 9: "INT8"}
PADDING_SAME, PADDING_VALID = 0, 1
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 3
# operators whose second input may be an INT8 filter -> the dimension its per-channel scales run along (the output channels)
FILTER_OPS = {"CONV_2D": 0, "FULLY_CONNECTED": 0, "DEPTHWISE_CONV_2D": 3}


# ---- flatbuffer access ---------------------------------------------------------------------------------------
class Table:
    def __init__(self, buf, pos):
        self.buf, self.pos = buf, pos
        self.vt = pos - struct.unpack_from("<i", buf, pos)[0]
        self.vt_size = struct.unpack_from("<H", buf, self.vt)[0]

    def _off(self, field):
        o = 4 + 2 * field
        if o >= self.vt_size:
            return 0
        return struct.unpack_from("<H", self.buf, self.vt + o)[0]

    def scalar(self, field, fmt, default=0):
        o = self._off(field)
        return struct.unpack_from("<" + fmt, self.buf, self.pos + o)[0] if o else default

    def _indirect(self, field):
        o = self._off(field)
        if not o:
            return None
        loc = self.pos + o
        return loc + struct.unpack_from("<I", self.buf, loc)[0]

    def table(self, field):
        p = self._indirect(field)
        return None if p is None else Table(self.buf, p)

    def string(self, field):
        p = self._indirect(field)
        if p is None:
            return None
        n = struct.unpack_from("<I", self.buf, p)[0]
        return bytes(self.buf[p + 4:p + 4 + n]).decode("utf-8", "replace")

    def vector(self, field, fmt=None):
        """fmt: struct code of scalar elements, or None for a vector of tables."""
        p = self._indirect(field)
        if p is None:
            return []
        n = struct.unpack_from("<I", self.buf, p)[0]
        if fmt is not None:
            return list(struct.unpack_from("<%d%s" % (n, fmt), self.buf, p + 4))
        out = []
        for i in range(n):
            loc = p + 4 + 4 * i
            out.append(Table(self.buf, loc + struct.unpack_from("<I", self.buf, loc)[0]))
        return out

    def bytes_vector(self, field):
        p = self._indirect(field)
        if p is None:
            return b""
        n = struct.unpack_from("<I", self.buf, p)[0]
        return bytes(self.buf[p + 4:p + 4 + n])


class Graph:
    """Tensors (shape, constant data), operators (name, inputs, outputs, options) of subgraph 0."""

    def __init__(self, data):
        buf = memoryview(data)
        if len(data) < 8 or bytes(buf[4:8]) != b"TFL3":
            raise ValueError("not a TFLite flatbuffer (file identifier TFL3 missing)")
        model = Table(buf, struct.unpack_from("<I", buf, 0)[0])
        codes = []
        for oc in model.vector(1):
            code = oc.scalar(3, "i", 0)
            if code == 0:
                code = oc.scalar(0, "b", 0)   # files written before builtin_code was widened
            codes.append(code)
        buffers = [b.bytes_vector(0) for b in model.vector(4)]
        sub = model.vector(2)[0]
        self.tensors = []
        for t in sub.vector(0):
            shape = t.vector(0, "i")
            ttype = t.scalar(1, "b", 0)
            raw = buffers[t.scalar(2, "I", 0)] if t.scalar(2, "I", 0) < len(buffers) else b""
            const = None
            if raw:
                if ttype == 0:
                    const = np.frombuffer(raw, "<f4").reshape(shape)
                elif ttype == 1:
                    # FLOAT16: the weights of the converter's float16 mode, each behind a DEQUANTIZE that is folded below
                    const = np.frombuffer(raw, "<f2").reshape(shape)
                elif ttype == 2:
                    const = np.frombuffer(raw, "<i4").reshape(shape)
                elif ttype in (9, 3, 7):
                    # INT8: a dynamic-range quantised filter; UINT8 / INT16 are decoded so that check_executable can refuse
                    # them by the operator that reads them
                    const = np.frombuffer(raw, {9: "i1", 3: "u1", 7: "<i2"}[ttype]).reshape(shape)
                else:
                    raise NotImplementedError("tensor %r has type %s: only float32 models and INT8 filters are read"
                                              % (t.string(3), TENSOR_TYPES.get(ttype, ttype)))
            quant = None
            q = t.table(4)
            if q is not None and q.vector(2, "f"):
                quant = dict(scale=np.array(q.vector(2, "f"), np.float32), zero_point=np.array(q.vector(3, "q"), np.int64),
                             dim=q.scalar(6, "i", 0))
            self.tensors.append(dict(shape=shape, type=ttype, const=const, name=t.string(3), quant=quant))
        self.inputs = sub.vector(1, "i")
        self.outputs = sub.vector(2, "i")
        self.ops = []
        for op in sub.vector(3):
            code = codes[op.scalar(0, "I", 0)]
            opts = op.table(4)
            o = dict(name=OPS.get(code, "OP_%d" % code), inputs=op.vector(1, "i"), outputs=op.vector(2, "i"), act=0)
            if opts is not None:
                if o["name"] == "CONV_2D":
                    o.update(padding=opts.scalar(0, "b", 0), stride_w=opts.scalar(1, "i", 1), stride_h=opts.scalar(2, "i", 1),
                             act=opts.scalar(3, "b", 0), dilation_w=opts.scalar(4, "i", 1), dilation_h=opts.scalar(5, "i", 1))
                    if o["dilation_w"] != 1 or o["dilation_h"] != 1:
                        raise NotImplementedError("operator %d (CONV_2D): dilation %d x %d, only 1 x 1 is read"
                                                  % (len(self.ops), o["dilation_h"], o["dilation_w"]))
                elif o["name"] == "DEPTHWISE_CONV_2D":
                    # (what does not run -- a depth multiplier, a dilation -- is refused by check_executable)
                    o.update(padding=opts.scalar(0, "b", 0), stride_w=opts.scalar(1, "i", 1), stride_h=opts.scalar(2, "i", 1),
                             depth_multiplier=opts.scalar(3, "i", 0), act=opts.scalar(4, "b", 0),
                             dilation_w=opts.scalar(5, "i", 1), dilation_h=opts.scalar(6, "i", 1))
                elif o["name"] in ("AVERAGE_POOL_2D", "MAX_POOL_2D"):
                    o.update(padding=opts.scalar(0, "b", 0), stride_w=opts.scalar(1, "i", 1), stride_h=opts.scalar(2, "i", 1),
                             filter_width=opts.scalar(3, "i", 1), filter_height=opts.scalar(4, "i", 1),
                             act=opts.scalar(5, "b", 0))
                elif o["name"] == "CONCATENATION":
                    o.update(axis=opts.scalar(0, "i", 0), act=opts.scalar(1, "b", 0))
                elif o["name"] in ("ADD", "MUL", "SUB", "DIV", "FULLY_CONNECTED"):
                    o["act"] = opts.scalar(0, "b", 0)
                    if o["name"] == "FULLY_CONNECTED":
                        o["asymmetric_quantize_inputs"] = bool(opts.scalar(3, "b", 0))
                elif o["name"] == "SOFTMAX":
                    o["beta"] = opts.scalar(0, "f", 0.0)
                elif o["name"] == "MEAN":
                    o["keep_dims"] = bool(opts.scalar(0, "b", 0))
                elif o["name"] == "RESHAPE":
                    o["new_shape"] = opts.vector(0, "i")
                elif o["name"] == "STRIDED_SLICE":
                    o.update(begin_mask=opts.scalar(0, "i", 0), end_mask=opts.scalar(1, "i", 0), ellipsis_mask=opts.scalar(2, "i", 0),
                             new_axis_mask=opts.scalar(3, "i", 0), shrink_axis_mask=opts.scalar(4, "i", 0),
                             offset=bool(opts.scalar(5, "b", 0)))
            if o["name"] in SLICE_OPS:
                for k, key in enumerate(("begin", "end", "strides") if o["name"] == "STRIDED_SLICE" else ("begin", "size"), 1):
                    v = self.tensors[o["inputs"][k]]["const"] if len(o["inputs"]) > k and o["inputs"][k] >= 0 else None
                    o[key] = None if v is None else [int(e) for e in np.asarray(v).reshape(-1)]
                for key in ("begin_mask", "end_mask", "ellipsis_mask", "new_axis_mask", "shrink_axis_mask"):
                    o.setdefault(key, 0)
                o.setdefault("offset", False)
                # (start, stride, count) per axis on the flatbuffer's own shape; None where that shape is dynamic or the
                # operator is one check_executable refuses
                o["slice"] = None
                shape = self.tensors[o["inputs"][0]]["shape"]
                if len(shape) == 4 and min(shape[1:]) > 0:
                    try:
                        o["slice"] = resolve_slice(o, shape, "operator %d (%s)" % (len(self.ops), o["name"]))
                    except NotImplementedError:
                        pass
            if o["name"] == "FULLY_CONNECTED":
                o.setdefault("asymmetric_quantize_inputs", False)
            if o["name"] == "MEAN":
                o.setdefault("keep_dims", False)
                ax = self.tensors[o["inputs"][1]]["const"] if len(o["inputs"]) > 1 else None
                o["axes"] = None if ax is None else [int(v) for v in np.asarray(ax).reshape(-1)]
            elif o["name"] == "PAD":
                pd = self.tensors[o["inputs"][1]]["const"] if len(o["inputs"]) > 1 else None
                o["paddings"] = None if pd is None else [[int(a), int(b)] for a, b in np.asarray(pd).reshape(-1, 2)]
            elif o["name"] == "SOFTMAX":
                o.setdefault("beta", 1.0)
            o["code"] = code
            self.ops.append(o)
        self._fold_float16_constants()

    def _fold_float16_constants(self):
        """The converter's float16 mode stores every weight as a FLOAT16 constant behind a DEQUANTIZE: such an operator is
        folded here, on load -- its output becomes the float32 constant (the conversion is exact) and the operator is gone,
        so the graph plans as the float32 graph of the fp16-rounded weights."""
        kept = []
        for o in self.ops:
            src = self.tensors[o["inputs"][0]] if o["name"] == "DEQUANTIZE" and len(o["inputs"]) == 1 and o["inputs"][0] >= 0 else None
            if src is not None and src["type"] == 1 and src["const"] is not None and len(o["outputs"]) == 1:
                out = self.tensors[o["outputs"][0]]
                out["const"], out["type"] = src["const"].astype(np.float32), 0
            else:
                kept.append(o)
        self.ops = kept

    def const(self, idx):
        return self.tensors[idx]["const"]

    def quantised_filter(self, op):
        """The filter tensor of a CONV_2D / DEPTHWISE_CONV_2D / FULLY_CONNECTED if it is an INT8 constant (dynamic-range
        quantisation), else None."""
        if op["name"] in FILTER_OPS and len(op["inputs"]) > 1 and op["inputs"][1] >= 0:
            ten = self.tensors[op["inputs"][1]]
            if ten["type"] == 9 and ten["const"] is not None:
                return ten
        return None

    def dequantised(self, idx):
        """A constant as float32: an INT8 filter multiplied out by its scales (one, or one per slice of its quantised
        dimension)."""
        ten = self.tensors[idx]
        if ten["type"] != 9:
            return ten["const"]
        sc = ten["quant"]["scale"].astype(np.float32)
        w = ten["const"].astype(np.float32)
        dim = ten["quant"]["dim"] if sc.size > 1 else 0
        return (w * sc.reshape((1,) * dim + (-1,) + (1,) * (w.ndim - 1 - dim))).astype(np.float32)

    def _check_integer_tensor(self, i, name, k, t, ten, integer):
        """check_executable(integer=True): -> True where tensor `t`, input or output k of operator i, is one a full-integer
        graph may hold: an INT8 activation with exactly one scale and one zero point (not the graph's input or output: the
        reference feeds and reads float32), the INT32 bias of a filter operator, an INT8 constant with one scale and one
        zero point as an operand of ADD / SUB / MUL.  What is refused here is refused by the operator's name and index."""
        if not integer:
            return False
        what, tname = "operator %d (%s)" % (i, name), TENSOR_TYPES.get(ten["type"], ten["type"])
        if ten["const"] is None and ten["type"] in (3, 7):
            raise NotImplementedError("%s: tensor %r is a %s activation, only INT8 activations are run" % (what, ten["name"], tname))
        if ten["type"] == 2 and ten["const"] is not None and k == 2 and name in FILTER_OPS:
            return True
        if ten["type"] != 9 or (ten["const"] is not None and name not in ("ADD", "SUB", "MUL")):
            if ten["type"] == 9 and name == "DIV":
                raise NotImplementedError("%s: a division on INT8 tensors is not run" % what)
            return False
        q = ten["quant"]
        if q is None or q["scale"].size != 1 or q["zero_point"].size != 1:
            raise NotImplementedError("%s: tensor %r is INT8 with %d scales and %d zero points (per-channel quantised "
                                      "activations are not run: exactly one of each)"
                                      % (what, ten["name"], 0 if q is None else q["scale"].size, 0 if q is None else q["zero_point"].size))
        if not -128 <= int(q["zero_point"][0]) <= 127:
            raise NotImplementedError("%s: tensor %r has the zero point %d, outside INT8" % (what, ten["name"], q["zero_point"][0]))
        if t in self.inputs or t in self.outputs:
            raise NotImplementedError("%s: tensor %r, the graph's %s, is INT8: only float32 inputs and outputs are run "
                                      "(QUANTIZE in front, DEQUANTIZE behind)" % (what, ten["name"], "input" if t in self.inputs else "output"))
        if name == "DIV":
            raise NotImplementedError("%s: a division on INT8 tensors is not run" % what)
        return True

    def check_executable(self, grouped=False, integer=False):
        """Raises NotImplementedError, naming the operator and its index, for whatever the graph executor
        (cpx/ml_tools/tflite_graph.py) does not run: an operator outside OPS, a STRIDED_SLICE / SLICE that resolve_slice
        refuses, a tensor that is not float32 (int32 constants of MEAN / RESHAPE / PAD / STRIDED_SLICE / SLICE excepted; an INT8 constant as the filter of CONV_2D / FULLY_CONNECTED with
        symmetric scales along dimension 0, or of DEPTHWISE_CONV_2D along dimension 3, excepted), grouped CONV_2D, a
        DEPTHWISE_CONV_2D with a depth multiplier or a dilation other than 1, a dynamic shape.  grouped=True lets a grouped
        CONV_2D through where the filter depth divides the input depth and the groups divide the output channels.
        integer=True lets a full-integer graph through (what a converter given a representative dataset writes): QUANTIZE /
        DEQUANTIZE, INT8 activations with one scale and one zero point, INT32 biases, INT8 constants as operands of ADD /
        SUB / MUL (_check_integer_tensor); without it every one of those is refused as ever, with the same texts."""
        for i, op in enumerate(self.ops):
            name = op["name"]
            if op["code"] not in OPS or (name in INTEGER_OPS and not integer):
                raise NotImplementedError("operator %d (%s) is not in the set the graph executor runs: %s"
                                          % (i, REFUSED_OPS.get(op["code"], name),
                                             ", ".join(sorted(v for v in OPS.values() if v not in INTEGER_OPS))))
            if name in SLICE_OPS:
                shape = self.tensors[op["inputs"][0]]["shape"]
                # (a dynamic H or W: the planner resolves against the shape it plans for, and refuses there)
                resolve_slice(op, shape if len(shape) == 4 and min(shape[1:]) > 0 else None, "operator %d (%s)" % (i, name))
            for k, t in enumerate(list(op["inputs"]) + list(op["outputs"])):
                if t < 0:
                    continue
                ten = self.tensors[t]
                int_const = ten["type"] == 2 and ten["const"] is not None and k >= 1 and \
                    name in ("MEAN", "RESHAPE", "PAD") + SLICE_OPS
                if ten["type"] == 9 and ten["const"] is not None and k == 1 and name in FILTER_OPS:
                    q = ten["quant"]
                    if q is None:
                        raise NotImplementedError("operator %d (%s): the INT8 filter %r has no quantisation scales" % (i, name, ten["name"]))
                    if np.any(q["zero_point"] != 0):
                        raise NotImplementedError("operator %d (%s): the INT8 filter %r has a non-zero zero point, only symmetric "
                                                  "filters are run" % (i, name, ten["name"]))
                    qdim = FILTER_OPS[name]
                    per_channel = q["dim"] == qdim and len(ten["shape"]) > qdim and q["scale"].size == ten["shape"][qdim]
                    # (one scale: CONV_2D / FULLY_CONNECTED state dimension 0 with it; a depthwise filter may state either)
                    if not (per_channel or (q["scale"].size == 1 and q["dim"] in (0, qdim))):
                        raise NotImplementedError("operator %d (%s): the INT8 filter %r has %d scales along dimension %d, "
                                                  "only one or one per output channel (dimension %d) are run"
                                                  % (i, name, ten["name"], q["scale"].size, q["dim"], qdim))
                    continue
                if self._check_integer_tensor(i, name, k, t, ten, integer):
                    continue
                if ten["type"] != 0 and not int_const:
                    raise NotImplementedError("operator %d (%s): tensor %r has type %s, only float32 graphs are run"
                                              % (i, name, ten["name"], TENSOR_TYPES.get(ten["type"], ten["type"])))
                if ten["const"] is None and any(d < 0 for d in ten["shape"][1:]):
                    raise NotImplementedError("operator %d (%s): tensor %r has a dynamic shape %s"
                                              % (i, name, ten["name"], ten["shape"]))
            if name == "CONV_2D":
                w = self.const(op["inputs"][1])
                if w is None:
                    raise NotImplementedError("operator %d (CONV_2D): the filter is not a constant" % i)
                cin = self.tensors[op["inputs"][0]]["shape"]
                if len(cin) == 4 and cin[3] > 0 and w.shape[3] != cin[3]:
                    if not grouped:
                        raise NotImplementedError("operator %d (CONV_2D): grouped convolution (filter depth %d, input depth %d)"
                                                  % (i, w.shape[3], cin[3]))
                    if w.shape[3] < 1 or cin[3] % w.shape[3] != 0:
                        raise NotImplementedError("operator %d (CONV_2D): grouped convolution whose filter depth %d does not "
                                                  "divide the input depth %d" % (i, w.shape[3], cin[3]))
                    if w.shape[0] % (cin[3] // w.shape[3]) != 0:
                        raise NotImplementedError("operator %d (CONV_2D): grouped convolution of %d groups (filter depth %d, input "
                                                  "depth %d) that do not divide its %d output channels"
                                                  % (i, cin[3] // w.shape[3], w.shape[3], cin[3], w.shape[0]))
            if name == "DEPTHWISE_CONV_2D":
                w = self.const(op["inputs"][1]) if len(op["inputs"]) > 1 and op["inputs"][1] >= 0 else None
                if w is None:
                    raise NotImplementedError("operator %d (DEPTHWISE_CONV_2D): the filter is not a constant" % i)
                if op.get("dilation_w", 1) != 1 or op.get("dilation_h", 1) != 1:
                    raise NotImplementedError("operator %d (DEPTHWISE_CONV_2D): dilation %d x %d, only 1 x 1 is run"
                                              % (i, op.get("dilation_h", 1), op.get("dilation_w", 1)))
                if w.ndim != 4 or w.shape[0] != 1:
                    raise NotImplementedError("operator %d (DEPTHWISE_CONV_2D): a filter of shape %s, [1, kh, kw, channels] is run"
                                              % (i, list(w.shape)))
                cin = self.tensors[op["inputs"][0]]["shape"]
                mult = op.get("depth_multiplier", 0)
                # (TFLite's prepare step checks the field against the shapes too; a field that disagrees is not repaired)
                if mult != 1:
                    raise NotImplementedError("operator %d (DEPTHWISE_CONV_2D): depth multiplier %d, only 1 is run" % (i, mult))
                if len(cin) == 4 and cin[3] > 0 and w.shape[3] != cin[3]:
                    raise NotImplementedError("operator %d (DEPTHWISE_CONV_2D): depth multiplier 1 with filter depth %d on input "
                                              "depth %d" % (i, w.shape[3], cin[3]))
            if name == "MEAN" and op["axes"] is None:
                raise NotImplementedError("operator %d (MEAN): the axes are not a constant" % i)
            if name == "PAD" and op["paddings"] is None:
                raise NotImplementedError("operator %d (PAD): the paddings are not a constant" % i)


def resolve_slice(op, shape, what):
    """A STRIDED_SLICE / SLICE operator of a Graph on an input of `shape` ([N, H, W, C]; N may be unknown, < 1) ->
    [(start, stride, count)] per axis, with TensorFlow's rules: a masked begin / end is the axis' edge, a negative index
    counts from the end, both are clamped to [0, size]; SLICE's size -1 runs to the end.  shape None: only what does not
    depend on the shape is checked, and None returned.  Refused, by `what` (the operator's name and index): begin / end /
    strides / size that are not constants, an ellipsis, new-axis or shrink-axis mask, `offset`, a stride below 1, an empty
    result, anything but the full range on the batch and on the channel axis."""
    strided = op["name"] == "STRIDED_SLICE"
    keys = ("begin", "end", "strides") if strided else ("begin", "size")
    for key in keys:
        if op.get(key) is None:
            raise NotImplementedError("%s: %s is not a constant" % (what, key))
        if len(op[key]) != 4:
            raise NotImplementedError("%s: %s has %d elements, only slices of [N, H, W, C] tensors are run" % (what, key, len(op[key])))
    if strided:
        for key in ("ellipsis_mask", "new_axis_mask", "shrink_axis_mask"):
            if op.get(key, 0):
                raise NotImplementedError("%s: %s %d, only begin_mask and end_mask are run" % (what, key, op[key]))
        if op.get("offset", False):
            raise NotImplementedError("%s: offset (end counted from begin) is not run" % what)
        if min(op["strides"]) < 1:
            raise NotImplementedError("%s: strides %s, only strides of 1 and above are run" % (what, op["strides"]))
    if shape is None:
        return None
    out = []
    for ax in range(4):
        d = max(int(shape[ax]), 1) if ax == 0 else int(shape[ax])
        b = op["begin"][ax]
        if strided:
            s, e = op["strides"][ax], op["end"][ax]
            b = 0 if op["begin_mask"] >> ax & 1 else min(max(b + d if b < 0 else b, 0), d)
            e = d if op["end_mask"] >> ax & 1 else min(max(e + d if e < 0 else e, 0), d)
        else:
            s, z = 1, op["size"][ax]
            e = d if z == -1 else b + z
            if b < 0 or z < -1 or e > d:
                raise NotImplementedError("%s: begin %s, size %s reach beyond the input %s" % (what, op["begin"], op["size"], list(shape)))
        count = max(-(-(e - b) // s), 0)
        if count < 1:
            raise NotImplementedError("%s: the result is empty along axis %d" % (what, ax))
        if ax in (0, 3) and (b, s, count) != (0, 1, d):
            raise NotImplementedError("%s: only the full range is run on the %s axis, not %d:%d:%d of %d"
                                      % (what, "batch" if ax == 0 else "channel", b, e, s, d))
        out.append((b, s, count))
    return out


# ---- the walk: operators in order -> Keras-layout names -------------------------------------------------------
def identity_variance():
    """moving_variance v with float32(v + eps) == 1, so that gamma / sqrt(v + eps) == gamma."""
    v = np.float32(1) - BN_EPS
    for cand in (v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(2))):
        if np.float32(cand + BN_EPS) == np.float32(1):
            return np.float32(cand)
    raise AssertionError("no float32 variance gives 1 with eps")


def bn_params(scale, shift):
    c = scale.shape[0]
    return {"gamma": scale.astype(np.float32), "beta": shift.astype(np.float32),
            "moving_mean": np.zeros(c, np.float32), "moving_variance": np.full(c, identity_variance(), np.float32)}


def conv_kernel(g, op, groups=2, const=None):
    """TFLite OHWI [Cout, kh, kw, Cin/groups] -> Keras HWIO [kh, kw, Cin/groups, Cout]; bias.  const: how a constant is
    read (default g.const; g.dequantised multiplies an INT8 filter out)."""
    w = (const or g.const)(op["inputs"][1])
    b = g.const(op["inputs"][2]) if len(op["inputs"]) > 2 and op["inputs"][2] >= 0 else None
    if w is None:
        raise ValueError("CONV_2D without a constant filter")
    k = np.ascontiguousarray(np.transpose(w, (1, 2, 3, 0))).astype(np.float32)
    return k, (np.zeros(w.shape[0], np.float32) if b is None else b.astype(np.float32))


def convert(g, blocks=3, filters=(16, 64, 128, 256), quantised_math=None):
    """quantised_math: None refuses an INT8 filter by its tensor's name; "float" multiplies every INT8 filter out,
    float32(int8) * scale, and converts the float32 network the file stands for."""
    if quantised_math not in (None, "float"):
        raise ValueError("quantised_math %r: None or 'float'" % (quantised_math,))
    for op in g.ops:
        ten = g.quantised_filter(op)
        if ten is not None and quantised_math is None:
            raise NotImplementedError("tensor %r is an INT8 filter: a dynamic-range quantised WR-ResNet is not converted "
                                      "(the graph executor runs quantised files: LiteInterpreter, build_plan(..., "
                                      "grouped_convolutions=True); or multiply the filters out: convert(g, "
                                      "quantised_math=\"float\"), CPX_TFLITE_QUANT_MATH=float)" % ten["name"])
    const = g.dequantised if quantised_math == "float" else g.const
    ops = list(g.ops)
    pos = [0]

    def peek():
        return ops[pos[0]] if pos[0] < len(ops) else None

    def take(name):
        op = peek()
        if op is None or op["name"] != name:
            raise ValueError("operator %d: expected %s, found %s" % (pos[0], name, None if op is None else op["name"]))
        pos[0] += 1
        return op

    def affine(channels):
        """MUL const, ADD const (+ fused or separate RELU) -> (scale, shift)."""
        m = take("MUL")
        a = take("ADD")
        sc = next(g.const(i) for i in m["inputs"] if g.const(i) is not None).reshape(-1)
        sh = next(g.const(i) for i in a["inputs"] if g.const(i) is not None).reshape(-1)
        if sc.shape[0] != channels or sh.shape[0] != channels:
            raise ValueError("BatchNorm constants of %d / %d channels where %d were expected" % (sc.shape[0], sh.shape[0], channels))
        if a["act"] != 1:
            take("RELU")
        return sc, sh

    w = {}
    op = take("CONV_2D")
    w["conv1_1/kernel"], w["conv1_1/bias"] = conv_kernel(g, op, const=const)
    c_in = filters[0]
    for stage in (2, 3, 4):
        f = filters[stage - 1]
        for d in range(blocks):
            b = "%db%d" % (stage, d)
            shortcut = None
            nxt = peek()
            if d == 0 and nxt is not None and nxt["name"] == "CONV_2D" and g.const(nxt["inputs"][1]).shape[1] == 1:
                shortcut = take("CONV_2D")              # the shortcut reads the block's raw input: it may come first
            sc, sh = affine(c_in)                       # pre-activation BatchNorm + ReLU of the block's input
            for k, v in bn_params(sc, sh).items():
                w["bn%s_branch2a/%s" % (b, k)] = v
            nxt = peek()
            if d == 0 and shortcut is None:
                # the 1x1 shortcut convolution; the converter may put it before or after the main branch
                if nxt["name"] == "CONV_2D" and g.const(nxt["inputs"][1]).shape[1] == 1:
                    shortcut = take("CONV_2D")
            a = take("CONV_2D")                         # conv a with the following BatchNorm folded in, ReLU fused
            w["res%s_branch2a/kernel" % b], w["res%s_branch2a/bias" % b] = conv_kernel(g, a, const=const)
            if a["act"] != 1:
                take("RELU")
            for k, v in bn_params(np.ones(f, np.float32), np.zeros(f, np.float32)).items():
                w["bn%s_branch2b/%s" % (b, k)] = v
            cb = take("CONV_2D")
            w["res%s_branch2b/kernel" % b], w["res%s_branch2b/bias" % b] = conv_kernel(g, cb, const=const)
            if d == 0 and shortcut is None:
                shortcut = take("CONV_2D")
            if shortcut is not None:
                w["shortcut%d/kernel" % stage], w["shortcut%d/bias" % stage] = conv_kernel(g, shortcut, const=const)
            add = take("ADD")
            # (the ReLU behind the residual ADD, wr_resnet.py:96-97, is fused into it by the converter; the network the
            # weights go to applies it either way)
            if add["act"] not in (0, 1):
                raise ValueError("operator %d: the residual ADD carries the activation %d, neither none nor RELU"
                                 % (pos[0] - 1, add["act"]))
            c_in = f
    sc, sh = affine(c_in)
    for k, v in bn_params(sc, sh).items():
        w["final_bn/%s" % k] = v
    take("MEAN")
    n_hidden = 0
    while True:
        fc = take("FULLY_CONNECTED")
        wt = const(fc["inputs"][1])
        bias = g.const(fc["inputs"][2]) if len(fc["inputs"]) > 2 and fc["inputs"][2] >= 0 else np.zeros(wt.shape[0], np.float32)
        nxt = peek()
        last = nxt is None or nxt["name"] in ("LOGISTIC", "SOFTMAX")
        name = "prediction" if last else "dense_%d" % n_hidden
        w[name + "/kernel"] = np.ascontiguousarray(wt.T).astype(np.float32)   # TFLite [out, in] -> Keras [in, out]
        w[name + "/bias"] = bias.astype(np.float32)
        if last:
            w["prediction/activation"] = "softmax" if (nxt is not None and nxt["name"] == "SOFTMAX") else "sigmoid"
            break
        if fc["act"] != 1:
            take("RELU")
        n_hidden += 1
    return w


def load_tflite(path, quantised_math=None):
    """-> the weights dict of cpx.ml_tools.wrresnet (what load_weights returns for an .npz) of a .tflite model file;
    quantised_math: convert's."""
    with open(str(path), "rb") as fh:
        g = Graph(fh.read())
    return convert(g, quantised_math=quantised_math)


def has_quantised_filters(path):
    """A .tflite file holds at least one INT8 filter: it is dynamic-range quantised."""
    with open(str(path), "rb") as fh:
        g = Graph(fh.read())
    return any(g.quantised_filter(op) is not None for op in g.ops)
