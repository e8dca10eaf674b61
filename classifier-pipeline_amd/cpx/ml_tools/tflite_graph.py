"""A TFLite graph, float32 or dynamic-range quantised, (cpx/ml_tools/tflite_reader.py: Graph) turned into a plan the device executor runs
(cpx_graph_create / cpx_graph_forward, include/cpx.h) -- what the reference's LiteInterpreter hands to the TFLite runtime
(src/ml_tools/interpreter.py:520-560).  A Plan is the operators in launch order, the tensors with their place in one
per-sample arena and every operator's constants in its kernel's layout.  build_plan is host work, needs no GPU, and is
these passes over one _Build, in this order, each described where it stands:

  lower_ops            flatbuffer operators -> PlanOps: shapes, constants and activations folded into their producers
                       (_fold_into_producer), concatenations as channel slices, convolutions by filter (_lower_filter)
  resolve_views        every tensor's storage, channel offset and stride
  attach_input         the caller's sample: as it is, through the channel map, or through an input mode (INPUT_MODES)
  prune_to_output      the operators the output does not need are dropped
  fold_window_chains   fold_windows: 1 x 1 pools, chains of PAD / SLICE, a PAD into its VALID convolution
  fuse_preactivations  fuse_preactivation / fuse_preactivation_dw: an AFFINE with a RELU into the convolutions behind it
  check_used_tensors   the tensors of the plan; one view of the input and of the output
  place_arena          offsets by lifetime
  pack_weights         each kind's weight image

With integer_activations=True lower_ops hands every operator that touches an INT8 activation to tflite_graph_i8 (the int8
kinds; float32 stays at the graph's two ends), annotate_types marks the int8 tensors and place_arena counts them in bytes.

What an operator kind takes part in is one row of KINDS.  GraphDevice uploads a plan's constants to an engine's device and
runs it."""
import collections
import ctypes as C

import numpy as np

from .. import _lib
from . import tflite_graph_i8
from .tflite_reader import ACT_NONE, ACT_RELU, ACT_RELU6, FILTER_OPS, INTEGER_OPS, PADDING_SAME, SLICE_OPS, resolve_slice

ALIGN = 64   # floats: every tensor of the arena starts on a 256-byte boundary


def _set_fields(obj, kw):
    if not set(kw) <= set(vars(obj)):
        raise TypeError("%s has no field %s" % (type(obj).__name__, ", ".join(sorted(set(kw) - set(vars(obj))))))
    vars(obj).update(kw)


class PlanOp:
    def __init__(self, kind, name, in0, out, in1=-1, **kw):
        self.kind, self.name, self.in0, self.in1, self.out = kind, name, in0, in1, out
        self.kh = self.kw = self.stride_h = self.stride_w = 1
        self.pads = (0, 0, 0, 0)   # top, left, bottom, right
        self.act = ACT_NONE
        self.param = 0.0
        self.channel_map = None
        self.input_mode = None     # of an INPUT operator: the key of INPUT_MODES
        self.weights = self.scale = self.shift = None   # numpy float32 (or packed bytes), host
        self.filter = self.filter_scale = None   # the flatbuffer's filter; an INT8 filter's per-output-channel scales
        self.groups = 1
        self.pre_scale = self.pre_shift = self.pre_source = None   # CONV_PRE: the dropped AFFINE's constants and operator
        self.copy = False
        self.source = None   # index of the flatbuffer's operator
        _set_fields(self, kw)


class PlanTensor:
    def __init__(self, tid, H, W, C, **kw):
        self.id, self.H, self.W, self.C = tid, H, W, C
        self.root = tid       # the tensor whose storage this one lives in: one step (storage: the end of the chain)
        self.storage = None   # resolve_views
        self.c_offset = 0
        self.c_stride = C
        self.arena_offset = -1
        self.external = False   # the caller's buffer (the plan's input and output), not the arena
        self.alias = False      # a RESHAPE's view of its input
        self.src_shape = None   # of such a view: its input's (H, W, C)
        self.dtype = "float32"  # or "int8": an activation of a full-integer graph, with its scale and zero point
        self.scale = self.zero_point = None
        _set_fields(self, kw)


class Plan:
    """ops: [PlanOp] in launch order; tensors: {flatbuffer tensor id: PlanTensor}; input / output: tensor ids;
    arena_floats: per sample."""

    def __init__(self):
        self.ops, self.tensors = [], {}
        self.input = self.output = -1
        self.out_storage = None   # the tensor the output's storage is (the output itself, or what it is a view of)
        self.input_shape = self.graph_input_shape = self.output_shape = None   # the caller's sample; the graph's input
        self.arena_floats = 0
        self.lifetimes = {}   # root tensor id -> (first op, last op) of the plan

    @property
    def arena_bytes_per_sample(self):
        return 4 * self.arena_floats

    def copies(self):
        return [o for o in self.ops if o.copy]

    def census(self):
        out = {}
        for o in self.ops:
            out[o.name] = out.get(o.name, 0) + 1
        return out


def same_pads(size, k, s):
    """TensorFlow's SAME: the surplus padding goes bottom and right."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


def window(size, k, s, padding):
    if padding == PADDING_SAME:
        return same_pads(size, k, s)
    return (size - k) // s + 1, 0, 0


def slice_pads(H, W, ho, wo, sh, sw, pad_top, pad_left):
    """The four pads of a SLICE operator (include/cpx.h: CPX_GRAPH_SLICE) that makes ho x wo pixels of an H x W input
    with the signed pad_top / pad_left: pad_bottom / pad_right are what the output size implies, negative where input rows
    are left over."""
    return (pad_top, pad_left, (ho - 1) * sh + 1 - H - pad_top, (wo - 1) * sw + 1 - W - pad_left)


def _channel_const(g, tid, channels, what):
    c = g.const(tid)
    v = np.asarray(c, np.float32).reshape(-1)
    if v.size == 1:
        v = np.full(channels, v[0], np.float32)
    if v.size != channels or (c.ndim > 1 and c.shape[-1] != v.size and c.size != 1):
        raise NotImplementedError("%s: a constant of shape %s against %d channels" % (what, list(c.shape), channels))
    return v.astype(np.float32)


# What an operator kind is, once.  A kind without a row is Kind(): none of it.
#   hybrid    an INT8 filter on the int8 pipe: in1 is the QUANT_PARAMS tensor of the input view
#   grouped   GraphOp.n_map carries the number of groups (a convolution has no channel map)
#   params    the kind writes the 1 x 1 x 4 per-sample tensor of a view (_view_params)
#   folds     MUL / ADD / SUB / DIV by constants and a swish fold into it (_fold_into_producer)
#   logistic  a LOGISTIC folds into it.  Behind a FULLY_CONNECTED it stays a launch
#   table     a full-integer kind whose int8 result can go through a 256-entry table behind its header (the activation
#             LUT: integer_lut folds an INT8 LOGISTIC or swish into it, tflite_graph_i8._emit_table).  Not FC_I8
#   pad       a PAD in front of it, VALID, becomes its four explicit pads (fold_window_chains).  Not the grouped kinds
#   pre       the kind it becomes behind a dropped pre-activation (fuse_preactivations).  There is no grouped and no fp16x2
#             CONV_PRE: in front of those kinds the AFFINE stays a launch.  CONV_PRE and DWCONV_PRE are made behind every
#             other fold, so nothing folds into them
#   pack      PlanOp -> its weights in the kernel's layout (pack_weights)
#   scaled    the device multiplies by float32(filter scale x folded scale): pack_weights puts the product into `scale`
#             (the hybrid kinds: only an INT8 filter has scales)
Kind = collections.namedtuple("Kind", "hybrid grouped params folds logistic pad pre pack scaled table",
                              defaults=(False, False, False, False, False, False, None, None, False, False))
_CONV_EPILOGUE = dict(folds=True, logistic=True)
KINDS = {
    _lib.GRAPH_CONV: Kind(pad=True, pre=_lib.GRAPH_CONV_PRE, pack=lambda o: pack_conv_filter(o.filter), **_CONV_EPILOGUE),
    _lib.GRAPH_CONV_Q8: Kind(hybrid=True, pad=True, pack=lambda o: pack_conv_filter_q8(o.filter), scaled=True, **_CONV_EPILOGUE),
    _lib.GRAPH_CONV_F16X2: Kind(pad=True, pack=lambda o: pack_conv_filter_f16x2(o.filter), **_CONV_EPILOGUE),
    _lib.GRAPH_CONV_PRE: Kind(pack=lambda o: pack_conv_pre(o.filter, o.pre_scale, o.pre_shift)),
    _lib.GRAPH_DWCONV: Kind(pad=True, pre=_lib.GRAPH_DWCONV_PRE, pack=lambda o: pack_dw_filter(o.filter), **_CONV_EPILOGUE),
    _lib.GRAPH_DWCONV_Q8: Kind(hybrid=True, pad=True, pack=lambda o: pack_dw_filter_q8(o.filter), scaled=True, **_CONV_EPILOGUE),
    _lib.GRAPH_DWCONV_PRE: Kind(pack=lambda o: pack_dw_filter(o.filter)),
    _lib.GRAPH_CONV_GROUPED: Kind(grouped=True, pack=lambda o: pack_conv_filter_grouped(o.filter, o.groups), **_CONV_EPILOGUE),
    _lib.GRAPH_CONV_Q8_GROUPED: Kind(hybrid=True, grouped=True, pack=lambda o: pack_conv_filter_q8_grouped(o.filter, o.groups),
                                     scaled=True, **_CONV_EPILOGUE),
    _lib.GRAPH_AFFINE: Kind(folds=True),
    _lib.GRAPH_FC: Kind(pack=lambda o: np.ascontiguousarray(o.filter, np.float32)),
    _lib.GRAPH_FC_Q8: Kind(hybrid=True, pack=lambda o: pack_fc_filter_q8(o.filter), scaled=True),
    _lib.GRAPH_QUANT_PARAMS: Kind(params=True), _lib.GRAPH_RANGE: Kind(params=True),
    # the full-integer kinds (tflite_graph_i8): the hybrid kinds' filter images unchanged; their integers ride in `scale`
    # and `shift`, which the lowering has already made.  A same-parameter PAD folds into the two that take explicit pads
    _lib.GRAPH_CONV_I8: Kind(pad=True, pack=lambda o: pack_conv_filter_q8(o.filter), table=True),
    _lib.GRAPH_CONV_I8_GROUPED: Kind(grouped=True, pack=lambda o: pack_conv_filter_q8_grouped(o.filter, o.groups), table=True),
    _lib.GRAPH_DWCONV_I8: Kind(pad=True, pack=lambda o: pack_dw_filter_q8(o.filter), table=True),
    _lib.GRAPH_FC_I8: Kind(pack=lambda o: pack_fc_filter_q8(o.filter)),
}


def kind_of(kind):
    return KINDS.get(kind, Kind())


def _kinds(column):
    return tuple(k for k, row in KINDS.items() if getattr(row, column))


Q8_KINDS, GROUPED_KINDS, PARAM_KINDS = _kinds("hybrid"), _kinds("grouped"), _kinds("params")
I8_FILTER_KINDS = (_lib.GRAPH_CONV_I8, _lib.GRAPH_CONV_I8_GROUPED, _lib.GRAPH_DWCONV_I8, _lib.GRAPH_FC_I8)
FOLD_INTO, LOGISTIC_INTO, LUT_INTO = _kinds("folds"), _kinds("logistic"), _kinds("table")

QUANT_MATHS = ("hybrid", "float")
CONV_MATHS = ("f32", "fp16x2")
ACT_SWISH, ACT_LOGISTIC = _lib.GRAPH_ACT_SWISH, _lib.GRAPH_ACT_LOGISTIC

# the 'caffe' / 'torch' modes of keras.applications.imagenet_utils.preprocess_input as the INPUT operator's constants
# (include/cpx.h: CPX_GRAPH_INPUT): mode -> (param, shift per graph channel, scale or None, the graph reads BGR)
INPUT_MODES = {
    "caffe": (1.0, np.array([103.939, 116.779, 123.68], np.float32), None, True),
    "torch": (255.0, np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32), False),
}
PRE_ACTS = (ACT_RELU, ACT_RELU6)


class _Build:
    """The plan under construction and what the passes share: the graph, its input and the output asked for, and -- while
    the flatbuffer's operators are lowered -- who writes and who reads a tensor."""

    def __init__(self, g, gin, gout):
        self.g, self.gin, self.gout, self.plan = g, gin, gout, Plan()
        self.ops, self.T = self.plan.ops, self.plan.tensors   # the passes change the two in place
        self.producer = {}    # tensor id -> PlanOp that writes it
        self.consumers = {}   # activation tensor id -> the flatbuffer's operators (indices) that read it
        for i, op in enumerate(g.ops):
            for t in op["inputs"]:
                if t >= 0 and g.const(t) is None:
                    self.consumers.setdefault(t, []).append(i)

    def emit(self, o, src):
        o.source = src
        self.ops.append(o)
        self.producer[o.out] = o
        return o

    def own_tensor(self, tid):
        """tid is a tensor of its own: in no concatenation, no view of it read, neither the graph's input nor its output."""
        return self.T[tid].storage == tid and tid not in (self.plan.out_storage, self.gout, self.plan.input, self.gin) and \
            not any(t.storage == tid and k != tid for k, t in self.T.items())

    def readers_of(self, tid):
        return [r for r in self.ops if tid in (r.in0, r.in1)]


def build_plan(g, input_shape=None, output=None, channel_map=None, quantised_math="hybrid", fuse_activations=True,
               input_mode=None, fuse_preactivation=False, fold_windows=False, fuse_preactivation_dw=False, conv_math="f32",
               grouped_convolutions=False, integer_activations=False, integer_gate_mul=False, integer_lut=False):
    """g: tflite_reader.Graph.  input_shape: (H, W, C) of a sample, default: the flatbuffer's.  output: the tensor the
    forward hands out, default the graph's output; the operators it does not need are dropped.  channel_map: up to 4
    indices into the channels of the sample the CALLER brings ([N, H, W, max(map) + 1 or more]): the graph's input
    channel c is the caller's channel channel_map[c].  quantised_math: "hybrid" runs INT8 filters on the int8 operators,
    "float" multiplies them out on the host.  fuse_activations=False: LOGISTIC and the MUL of a swish stay launches.
    input_mode: "caffe" | "torch": the caller brings the unscaled 0..255 sample and the channel map becomes the INPUT
    operator, which also does that mode's arithmetic on exactly three graph channels; channel_map is what the graph
    reads, so the BGR reversal of 'caffe' is the caller's (LiteInterpreter.channel_map).  fuse_preactivation: an AFFINE with a RELU / RELU6 whose only readers are float32
    convolutions is dropped and those convolutions become CONV_PRE (the same float32 operations, bit for bit).
    fold_windows: 1 x 1 pools and chains of PAD / SLICE become one SLICE, a PAD folds into the VALID convolution behind it.
    fuse_preactivation_dw: a bare RELU / RELU6 is also dropped in front of float32 depthwise convolutions (DWCONV_PRE) and
    SLICEs; both keep every bit (fold_window_chains, fuse_preactivations).  conv_math: "f32" runs float32 convolutions on
    the exact float32 kernel, "fp16x2" as two fp16 planes on the fp16 matrix pipe behind one RANGE launch per input view; a
    pre-activation is then not folded into them (no CONV_PRE is planned: the AFFINE stays a launch).  grouped_convolutions:
    False refuses a grouped CONV_2D by name, True plans it as CONV_GROUPED / CONV_Q8_GROUPED (_lower_filter).
    integer_activations: False refuses a full-integer file (INT8 activations, QUANTIZE / DEQUANTIZE) as ever, True plans its
    interior on the int8 kinds (tflite_graph_i8: float32 stays at the two ends; a float32 operator behind a DEQUANTIZE is
    the existing kind).  integer_gate_mul (with integer_activations; default False refuses it as ever): an INT8 MUL of an
    [H, W, C] tensor by the [1, 1, C] gate of a squeeze-and-excite block, in either operand order, is MUL_I8 with the gate as
    in1.  integer_lut (with integer_activations; default False: DEQUANTIZE -> LOGISTIC -> QUANTIZE as ever): an interior INT8
    LOGISTIC is a 256-entry table, and so is a swish (LOGISTIC + MUL of the same x: both operands are functions of the one
    byte); the table is folded into x's producer where that is one of KINDS' table column under _fold_into_producer's rules,
    elsewhere it is ONE LUT_I8 launch.  An INT8 LOGISTIC that a DEQUANTIZE reads (the head) and SOFTMAX keep their three
    launches.  The arithmetic: include/cpx.h, "Tables"."""
    if quantised_math not in QUANT_MATHS:
        raise ValueError("quantised_math %r: one of %s" % (quantised_math, ", ".join(QUANT_MATHS)))
    if conv_math not in CONV_MATHS:
        raise ValueError("conv_math %r: one of %s" % (conv_math, ", ".join(CONV_MATHS)))
    if input_mode is not None and input_mode not in INPUT_MODES:
        raise ValueError("input_mode %r: one of %s" % (input_mode, ", ".join(sorted(INPUT_MODES))))
    g.check_executable(grouped=grouped_convolutions, integer=integer_activations)
    if len(g.inputs) != 1 or len(g.outputs) < 1:
        raise NotImplementedError("graphs with %d inputs" % len(g.inputs))
    gin = g.inputs[0]
    if input_shape is None:
        input_shape = tuple(g.tensors[gin]["shape"][1:])
    if len(input_shape) != 3 or min(input_shape) < 1:
        raise NotImplementedError("operator 0: the input has the dynamic shape %s: pass input_shape" % (list(input_shape),))
    s = _Build(g, gin, g.outputs[0] if output is None else int(output))
    s.T[gin] = PlanTensor(gin, *[int(v) for v in input_shape])
    lower_ops(s, quantised_math, fuse_activations, conv_math, grouped_convolutions, integer_activations, integer_gate_mul,
              integer_lut)
    if integer_activations:
        tflite_graph_i8.annotate_types(s)
    resolve_views(s)
    attach_input(s, channel_map, input_mode)
    prune_to_output(s)
    if fold_windows:
        fold_window_chains(s)
    if integer_activations:
        tflite_graph_i8.finish_pads(s)
    if fuse_preactivation or fuse_preactivation_dw:
        fuse_preactivations(s, fuse_preactivation, fuse_preactivation_dw)
    check_used_tensors(s)
    place_arena(s)
    pack_weights(s.ops)
    return s.plan


def _find_swishes(s):
    """A swish as the converter writes it: s = LOGISTIC(x); y = MUL(x, s) in either operand order, s read by nothing else.
    -> ({operator index of the LOGISTIC: of the MUL}, {of the MUL: x})."""
    g, swish_logistic, swish_mul = s.g, {}, {}
    for i, op in enumerate(g.ops):
        if op["name"] != "LOGISTIC":
            continue
        xt, st = op["inputs"][0], op["outputs"][0]
        readers = s.consumers.get(st, [])
        if len(readers) != 1 or st == s.gout or st in g.outputs or g.const(xt) is not None:
            continue
        mul = g.ops[readers[0]]
        if mul["name"] == "MUL" and mul.get("act", 0) == ACT_NONE and sorted(t for t in mul["inputs"] if t >= 0) == sorted((xt, st)) \
                and xt != st:
            swish_logistic[i] = readers[0]
            swish_mul[readers[0]] = xt
    return swish_logistic, swish_mul


def _fold_into_producer(s, x, y, into, suffix, act, scale=None, shift=None, readers=1, through_view=False):
    """The operator that makes y of x alone becomes part of x's producer p, where p is one of the kinds `into`, carries
    no activation and is no copy, and x is not the output and has exactly `readers` readers in the flatbuffer (a swish's x
    has two, its LOGISTIC and its MUL): p then writes y, with the activation `act` behind (v * s0 + h0) * scale + shift
    where constants are given, and x is gone.  -> whether it did; elsewhere the caller emits a launch.
    through_view: a RESHAPE hands its input's producer on to its view, so p may write another tensor than x (p.out != x.id).
    The swish and the LOGISTIC fold ask for x itself; the fold of constants never has, and takes the view too."""
    p = s.producer.get(x.id)
    if p is None or p.kind not in into or p.act != ACT_NONE or p.copy or (p.out != x.id and not through_view) \
            or len(s.consumers.get(x.id, [])) != readers or x.id == s.gout:
        return False
    if scale is not None:
        s0 = np.ones_like(scale) if p.scale is None else p.scale
        h0 = np.zeros_like(scale) if p.shift is None else p.shift
        p.scale, p.shift = (s0 * scale).astype(np.float32), (h0 * scale + shift).astype(np.float32)
    p.act, p.out, p.name = act, y, p.name + "+" + suffix   # the producer now writes this operator's output
    s.producer[y] = p
    del s.T[x.id]
    return True


def _view_params(s, kind, key, name, param, x, src):
    """The 1 x 1 x 4 per-sample tensor `key` of view x -- the QUANT_PARAMS (sx, inv, zp) of a hybrid operator, the RANGE
    (up, down) of a CONV_F16X2 -- which ONE operator per view writes and all its consumers share; the operator goes in
    front of the first consumer that asks, i.e. behind every producer of x (the flatbuffer's operators are in execution
    order)."""
    if key not in s.T:
        s.T[key] = PlanTensor(key, 1, 1, 4)
        o = PlanOp(kind, name, x.id, key, param=param)
        o.source = src
        s.ops.append(o)
    return key


def _quant_params(s, x, symmetric, src):
    return _view_params(s, _lib.GRAPH_QUANT_PARAMS, ("quant_params", x.id, bool(symmetric)), "QUANT_PARAMS",
                        1.0 if symmetric else 0.0, x, src)


def _filter_of(g, op, tid, quantised_math):
    """-> (filter, per-output-channel scales or None): INT8 with its scales in hybrid mode, float32 otherwise
    (quantised_math="float" multiplies the filter out, int8 x scale, and the float32 operators are planned)."""
    ten = g.quantised_filter(op)
    if ten is None:
        return g.const(tid), None
    if quantised_math == "float":
        return g.dequantised(tid), None
    sc = np.asarray(ten["quant"]["scale"], np.float32).reshape(-1)
    channels = ten["shape"][FILTER_OPS[op["name"]]]
    return ten["const"], (np.full(channels, sc[0], np.float32) if sc.size == 1 else sc)


def _overflow_check(what, k):
    if k * 127 * 255 >= 2 ** 31:
        raise NotImplementedError("%s: %d products of an 8-bit activation and an INT8 weight could overflow the int32 "
                                  "accumulator" % (what, k))


def _bias(g, ins, absent=None):
    """The bias of a filter operator, or `absent` where it has none."""
    bias = g.const(ins[2]) if len(ins) > 2 else None
    return absent if bias is None else np.asarray(bias, np.float32).reshape(-1)


def _lower_filter(s, i, op, what, x, y, ins, quantised_math, conv_math, grouped_convolutions):
    """CONV_2D (filter OHWI) or DEPTHWISE_CONV_2D (filter [1, kh, kw, C], depth multiplier 1: the MobileNetV2 family):
    * float32: CONV (pack_conv_filter) or DWCONV (pack_dw_filter); both take folded constants and write into a
      concatenation's slice;
    * an INT8 filter (dynamic-range quantisation: what the reference's converter writes, src/tfliteconverter.py:54-62;
      depthwise scales along dimension 3) with quantised_math="hybrid": CONV_Q8 / DWCONV_Q8 on the parameters of the input
      view (_view_params), the filter in the order the int8 MFMA's B fragment wants with the per-channel integer sums wsum
      behind it (pack_conv_filter_q8, pack_dw_filter_q8: int8 taps, then wsum).  The arithmetic: include/cpx.h;
    * conv_math="fp16x2" (default "f32": nothing changes): every operator that would have been a float32 CONV is
      CONV_F16X2: float32 in and out, every operand as two fp16 planes of 11 + 11 significand bits, three plane products on
      the fp16 matrix pipe with float32 accumulation (include/cpx.h fixes the arithmetic, tests/tflite_eval_h2.py restates
      it).  Its second input is the RANGE tensor of its input view, the exact power of two that brings the sample's largest
      magnitude below 2^15.  The filter is scaled per output channel by the power of two that puts its largest magnitude in
      [8, 16), split the same way and packed in the MFMA's fragment order (pack_conv_filter_f16x2).  Fused activations and
      folded MUL / ADD work unchanged: the epilogue is CONV's.  Depthwise, FULLY_CONNECTED and the hybrid kinds are
      untouched; quantised_math="float" composes (the multiplied-out filters are split like any others);
    * with grouped_convolutions=True (default False: a grouped CONV_2D is refused by name, as ever) a CONV_2D whose filter
      depth divides the input depth is a CONV_GROUPED of G = input depth / filter depth groups (Cout % G == 0; a
      WR-ResNet's convolutions are groups = 2, src/ml_tools/resnet/wr_resnet.py:12-20): ONE launch, the group a grid
      dimension, each group's outputs bit for bit what CONV computes from that group's channel slice
      (pack_conv_filter_grouped: G CONV images one after another).  With an INT8 filter (one scale or one per output
      channel) hybrid math plans CONV_Q8_GROUPED on the QUANT_PARAMS of the WHOLE input view -- the tensor is quantised once
      per sample, before the groups are walked, as the TFLite runtime's published hybrid kernels do (taken from their
      text; parity with the runtime is not pinned, as for every hybrid operator here) -- and the int32 overflow check counts
      kh * kw * (Cin / G) products; quantised_math="float" multiplies the filter out and plans CONV_GROUPED.  Strides 1 to 3
      on either axis (the network's last stage has stride 3).  The kinds have CONV's epilogue (KINDS); conv_math="fp16x2"
      leaves them on the float32 kernel.  Still refused, by operator name and index: a filter depth that does not divide the
      input depth, a Cout that G does not divide, dilation, a grouped DEPTHWISE_CONV_2D (a depth multiplier), strides above 3."""
    dw = op["name"] == "DEPTHWISE_CONV_2D"
    w, fscale = _filter_of(s.g, op, ins[1], quantised_math)
    kh, kw, depth = w.shape[1:]
    co = depth if dw else w.shape[0]
    groups = 1
    if depth != x.C:
        if dw or not grouped_convolutions:
            raise NotImplementedError(("%s: depth multiplier (filter depth %d, input depth %d), only 1 is run" if dw else
                                       "%s: grouped convolution (filter depth %d, input depth %d)") % (what, depth, x.C))
        if depth < 1 or x.C % depth != 0:
            raise NotImplementedError("%s: grouped convolution whose filter depth %d does not divide the input depth %d"
                                      % (what, depth, x.C))
        groups = x.C // depth
        if co % groups != 0:
            raise NotImplementedError("%s: grouped convolution of %d groups (filter depth %d, input depth %d) that do "
                                      "not divide its %d output channels" % (what, groups, depth, x.C, co))
    sh, sw = op.get("stride_h", 1), op.get("stride_w", 1)
    strides = (1, 2, 3) if groups > 1 else (1, 2)
    if not (1 <= kh <= 7 and 1 <= kw <= 7 and sh in strides and sw in strides):
        raise NotImplementedError("%s: %d x %d kernel with strides %d, %d" % (what, kh, kw, sh, sw))
    ho, pt, pb = window(x.H, kh, sh, op.get("padding", 0))
    wo, pl, pr = window(x.W, kw, sw, op.get("padding", 0))
    if ho < 1 or wo < 1:
        raise NotImplementedError("%s: the %d x %d input is smaller than the kernel" % (what, x.H, x.W))
    s.T[y] = PlanTensor(y, ho, wo, co)
    kind, in1 = _lib.GRAPH_DWCONV if dw else _lib.GRAPH_CONV, -1
    if fscale is not None:
        if not dw:   # (a depthwise output sums kh * kw <= 49 products)
            _overflow_check(what, kh * kw * depth)   # (depth: the channels of ONE group)
        kind, in1 = _lib.GRAPH_DWCONV_Q8 if dw else _lib.GRAPH_CONV_Q8, _quant_params(s, x, False, i)
        if groups > 1:
            kind = _lib.GRAPH_CONV_Q8_GROUPED   # the parameters are the whole view's, shared like any other reader's
    elif groups > 1:
        kind = _lib.GRAPH_CONV_GROUPED          # (also with conv_math="fp16x2": there is no grouped fp16x2 kernel)
    elif conv_math == "fp16x2" and not dw:
        kind, in1 = _lib.GRAPH_CONV_F16X2, _view_params(s, _lib.GRAPH_RANGE, ("range", x.id), "RANGE", 0.0, x, i)
    s.emit(PlanOp(kind, op["name"], x.id, y, in1=in1, kh=kh, kw=kw, stride_h=sh, stride_w=sw, pads=(pt, pl, pb, pr), groups=groups,
                  act=op.get("act", 0), filter=w, filter_scale=fscale, shift=_bias(s.g, ins, np.zeros(co, np.float32))), i)


def _affine_of(name, c, const_first, what):
    """x `name` c (c `name` x where const_first) per channel as x * scale + shift -> (scale, shift).  x / c is the scale
    float32(1 / float64(c)); c / x is refused."""
    one, zero = np.ones_like(c), np.zeros_like(c)
    if name == "DIV":
        if const_first:
            raise NotImplementedError("%s: a constant divided by an activation (c / x) is not run" % what)
        if np.any(c == 0):
            raise NotImplementedError("%s: division by a constant 0" % what)
        return (1.0 / c.astype(np.float64)).astype(np.float32), zero
    if name == "MUL":
        return c, zero
    if name == "ADD":
        return one, c
    return (-one, c) if const_first else (one, -c)   # c - x; x - c


def lower_ops(s, quantised_math, fuse_activations, conv_math, grouped_convolutions, integer_activations=False,
              integer_gate_mul=False, integer_lut=False):
    """Every operator of the flatbuffer, in its order, as PlanOps on tensors of inferred shape ([H, W, C] of one sample,
    TensorFlow's SAME / VALID arithmetic):
    * MUL / ADD / SUB / DIV by a per-channel constant behind one of FOLD_INTO (a convolution, or another such operator)
      that nothing else reads are folded into its scale and shift; elsewhere they are one element-wise AFFINE operator;
    * a swish (_find_swishes) is folded into x's producer as the activation SWISH (_lib.GRAPH_ACT_SWISH) where
      _fold_into_producer allows; elsewhere it is ONE AFFINE operator with that activation.  A LOGISTIC behind one of
      LOGISTIC_INTO (CONV_2D / DEPTHWISE_CONV_2D, float32 or hybrid) that nothing else reads is folded as the activation
      LOGISTIC (the gate of a squeeze-and-excite block); behind a FULLY_CONNECTED it stays a launch.
      fuse_activations=False keeps every LOGISTIC and MUL a launch: the same float32 operations, bit for bit;
    * any other MUL of two activations is a MUL operator: two tensors of one shape, or [H, W, C] by the [1, 1, C] gate of a
      squeeze-and-excite block in either operand order.  Every other broadcast is refused;
    * STRIDED_SLICE / SLICE over H and W (tflite_reader.resolve_slice: start, stride, count per axis) is one SLICE operator,
      a copy with a signed pad (negative: a crop), a stride and an optional RELU / RELU6 (include/cpx.h: CPX_GRAPH_SLICE);
    * MEAN over H and W, with or without keep_dims (and the RESHAPE to [1, 1, 1, C] older Keras versions put behind it, a
      view), is one operator with two summation orders (include/cpx.h: CPX_GRAPH_MEAN);
    * a CONCATENATION along the channels runs no kernel: every producer of one of its inputs writes straight into its
      channel slice of the concatenated tensor (channel offset + row stride).  Only an input that cannot be placed -- it
      feeds two concatenations, it is the graph's input, it is a view of another tensor -- is copied (a COPY entry: an
      AFFINE operator without constants);
    * CONV_2D / DEPTHWISE_CONV_2D: _lower_filter.  A FULLY_CONNECTED with an INT8 filter is the hybrid FC_Q8
      (pack_fc_filter_q8) on the symmetric or asymmetric QUANT_PARAMS of its input view, as the flatbuffer asks;
    * integer_activations: an operator on INT8 tensors is tflite_graph_i8's.  A swish of an INT8 x is no float32 activation:
      with integer_lut it is one table (lower_integer_swish), without it its LOGISTIC and its MUL are lowered as they stand."""
    g, T, gin, gout = s.g, s.T, s.gin, s.gout
    swish_logistic, swish_mul = _find_swishes(s) if fuse_activations or (integer_activations and integer_lut) else ({}, {})
    i8_logistic, i8_mul = {}, {}
    if integer_activations:
        i8_mul = {m: x for m, x in swish_mul.items() if tflite_graph_i8.is_int8(g, x)}
        i8_logistic = {lg: m for lg, m in swish_logistic.items() if m in i8_mul}
        swish_mul = {m: x for m, x in swish_mul.items() if m not in i8_mul} if fuse_activations else {}
        swish_logistic = {lg: m for lg, m in swish_logistic.items() if m in swish_mul}
        if not integer_lut:
            i8_logistic, i8_mul = {}, {}
    for i, op in enumerate(g.ops):
        name = op["name"]
        what = "operator %d (%s)" % (i, name)
        ins = [t for t in op["inputs"] if t >= 0]
        act_ins = [t for t in ins if g.const(t) is None]
        if i in swish_logistic or i in i8_logistic:
            continue   # (its MUL does the work)
        if i in i8_mul:
            if i8_mul[i] not in T:
                raise NotImplementedError("%s reads tensor %d, which no earlier operator wrote" % (what, i8_mul[i]))
            logistic = g.ops[next(lg for lg, m in i8_logistic.items() if m == i)]
            tflite_graph_i8.lower_integer_swish(s, i, op, logistic, T[i8_mul[i]], op["outputs"][0], what)
            continue
        if i in swish_mul:
            if swish_mul[i] not in T:
                raise NotImplementedError("%s reads tensor %d, which no earlier operator wrote" % (what, swish_mul[i]))
            x, y = T[swish_mul[i]], op["outputs"][0]
            T[y] = PlanTensor(y, x.H, x.W, x.C)
            if not _fold_into_producer(s, x, y, FOLD_INTO, "SWISH", ACT_SWISH, readers=2):
                s.emit(PlanOp(_lib.GRAPH_AFFINE, "SWISH", x.id, y, act=ACT_SWISH), i)
            continue
        for t in act_ins:
            if t not in T:
                raise NotImplementedError("%s reads tensor %d, which no earlier operator wrote" % (what, t))
        y = op["outputs"][0]
        x = T[act_ins[0]] if act_ins else None
        if op.get("act", 0) not in (ACT_NONE, ACT_RELU, ACT_RELU6):
            raise NotImplementedError("%s: fused activation %d" % (what, op["act"]))
        int8 = integer_activations and (name in INTEGER_OPS or any(tflite_graph_i8.is_int8(g, t) for t in act_ins + [y]))
        if int8 and tflite_graph_i8.lower_integer_op(s, i, op, what, x, y, ins, act_ins, grouped_convolutions, integer_gate_mul,
                                                     integer_lut):
            continue
        if name in ("CONV_2D", "DEPTHWISE_CONV_2D"):
            _lower_filter(s, i, op, what, x, y, ins, quantised_math, conv_math, grouped_convolutions)
        elif name in ("MAX_POOL_2D", "AVERAGE_POOL_2D"):
            kh, kw = op["filter_height"], op["filter_width"]
            sh, sw = op["stride_h"], op["stride_w"]
            if not (1 <= kh <= 7 and 1 <= kw <= 7 and 1 <= sh <= 7 and 1 <= sw <= 7):
                raise NotImplementedError("%s: %d x %d window with strides %d, %d" % (what, kh, kw, sh, sw))
            ho, pt, pb = window(x.H, kh, sh, op["padding"])
            wo, pl, pr = window(x.W, kw, sw, op["padding"])
            if ho < 1 or wo < 1:
                raise NotImplementedError("%s: the %d x %d input is smaller than the window" % (what, x.H, x.W))
            T[y] = PlanTensor(y, ho, wo, x.C)
            s.emit(PlanOp(_lib.GRAPH_MAX_POOL if name[0] == "M" else _lib.GRAPH_AVG_POOL, name, x.id, y, kh=kh, kw=kw,
                          stride_h=sh, stride_w=sw, pads=(pt, pl, pb, pr), act=op["act"]), i)
        elif name in ("ADD", "SUB", "MUL", "DIV"):
            if len(act_ins) == 2:
                b = T[act_ins[1]]
                same = (x.H, x.W, x.C) == (b.H, b.W, b.C)
                if name == "DIV":
                    raise NotImplementedError("%s of two activations: only a division by a constant is run" % what)
                if name == "MUL":
                    # [H, W, C] by the [1, 1, C] gate of its sample, in either order: the gate is in1
                    if not same and (b.H, b.W, b.C) != (1, 1, x.C):
                        x, b = b, x
                    if not same and (b.H, b.W, b.C) != (1, 1, x.C):
                        raise NotImplementedError("%s of two tensors of shapes %s, %s: only one shape, or [H, W, C] by [1, 1, C]"
                                                  % (what, (b.H, b.W, b.C), (x.H, x.W, x.C)))
                    T[y] = PlanTensor(y, x.H, x.W, x.C)
                    s.emit(PlanOp(_lib.GRAPH_MUL, name, x.id, y, in1=b.id, act=op["act"]), i)
                    continue
                if not same:
                    raise NotImplementedError("%s of two tensors of shapes %s, %s" % (what, (x.H, x.W, x.C), (b.H, b.W, b.C)))
                T[y] = PlanTensor(y, x.H, x.W, x.C)
                s.emit(PlanOp(_lib.GRAPH_ADD, name, x.id, y, in1=b.id, act=op["act"], param=1.0 if name == "ADD" else -1.0), i)
            else:
                cid = next(t for t in ins if g.const(t) is not None)
                sc, sf = _affine_of(name, _channel_const(g, cid, x.C, what), ins[0] == cid, what)
                T[y] = PlanTensor(y, x.H, x.W, x.C)
                if not _fold_into_producer(s, x, y, FOLD_INTO, name, op["act"], scale=sc, shift=sf, through_view=True):
                    s.emit(PlanOp(_lib.GRAPH_AFFINE, name, x.id, y, scale=sc, shift=sf, act=op["act"]), i)
        elif name in ("RELU", "RELU6"):
            T[y] = PlanTensor(y, x.H, x.W, x.C)
            s.emit(PlanOp(_lib.GRAPH_AFFINE, name, x.id, y, act=ACT_RELU if name == "RELU" else ACT_RELU6), i)
        elif name == "CONCATENATION":
            rank = len(g.tensors[act_ins[0]]["shape"]) or 4
            axis = op.get("axis", 0)
            if axis not in (-1, rank - 1) or len(act_ins) != len(ins):
                raise NotImplementedError("%s along axis %d: only the channel axis of activations is concatenated" % (what, axis))
            parts = [T[t] for t in act_ins]
            if any((p.H, p.W) != (x.H, x.W) for p in parts):
                raise NotImplementedError("%s of different spatial sizes" % what)
            T[y] = PlanTensor(y, x.H, x.W, sum(p.C for p in parts))
            off, seen = 0, set()
            for p in parts:
                must_copy = p.root != p.id or p.alias or p.id in seen or p.id == gin or p.id == gout or \
                    any(T[t].alias and T[t].root == p.id for t in T)
                if must_copy:
                    # a slice of the output that an AFFINE operator without constants fills
                    T[(y, off)] = PlanTensor((y, off), x.H, x.W, p.C, root=y, c_offset=off)
                    if int8:   # bytes: a SLICE that takes everything
                        s.emit(PlanOp(_lib.GRAPH_SLICE, "COPY", p.id, (y, off), copy=True,
                                      shift=tflite_graph_i8.header(z_in=tflite_graph_i8.qparams(g, y)[1])), i)
                    else:
                        s.emit(PlanOp(_lib.GRAPH_AFFINE, "COPY", p.id, (y, off), copy=True), i)
                    del s.producer[(y, off)]
                else:
                    p.root, p.c_offset = y, off
                seen.add(p.id)
                off += p.C
            if op.get("act", 0) != ACT_NONE:
                s.emit(PlanOp(_lib.GRAPH_AFFINE, "CONCATENATION_ACT", y, y, act=op["act"]), i)
        elif name == "MEAN":
            axes = sorted(a % 4 for a in op["axes"])
            if axes != [1, 2]:
                raise NotImplementedError("%s over axes %s: only H and W (global average pooling)" % (what, op["axes"]))
            T[y] = PlanTensor(y, 1, 1, x.C)
            s.emit(PlanOp(_lib.GRAPH_MEAN, name, x.id, y), i)
        elif name == "FULLY_CONNECTED":
            w, fscale = (None, None) if g.const(ins[1]) is None else _filter_of(g, op, ins[1], quantised_math)
            if w is None or x.H != 1 or x.W != 1 or w.shape[1] != x.C:
                raise NotImplementedError("%s: weights %s on a %d x %d x %d input" % (what, None if w is None else list(w.shape), x.H, x.W, x.C))
            T[y] = PlanTensor(y, 1, 1, w.shape[0])
            if fscale is not None:
                _overflow_check(what, w.shape[1])
                s.emit(PlanOp(_lib.GRAPH_FC_Q8, name, x.id, y, in1=_quant_params(s, x, not op.get("asymmetric_quantize_inputs", False), i),
                              act=op["act"], filter=w, filter_scale=fscale, shift=_bias(g, ins, np.zeros(w.shape[0], np.float32))), i)
            else:
                s.emit(PlanOp(_lib.GRAPH_FC, name, x.id, y, act=op["act"], filter=w, shift=_bias(g, ins)), i)
        elif name in ("LOGISTIC", "SOFTMAX"):
            T[y] = PlanTensor(y, x.H, x.W, x.C)
            if not (name == "LOGISTIC" and fuse_activations and _fold_into_producer(s, x, y, LOGISTIC_INTO, "LOGISTIC", ACT_LOGISTIC)):
                s.emit(PlanOp(_lib.GRAPH_LOGISTIC if name == "LOGISTIC" else _lib.GRAPH_SOFTMAX, name, x.id, y,
                              param=float(op.get("beta", 1.0))), i)
        elif name == "PAD":
            pd = op["paddings"]
            if len(pd) != 4 or pd[0] != [0, 0] or pd[3] != [0, 0] or min(min(p) for p in pd) < 0:
                raise NotImplementedError("%s with paddings %s: only H and W are padded" % (what, pd))
            T[y] = PlanTensor(y, x.H + pd[1][0] + pd[1][1], x.W + pd[2][0] + pd[2][1], x.C)
            s.emit(PlanOp(_lib.GRAPH_PAD, name, x.id, y, pads=(pd[1][0], pd[2][0], pd[1][1], pd[2][1])), i)
        elif name in SLICE_OPS:
            (_, (y0, sh, ho), (x0, sw, wo), _) = resolve_slice(op, (1, x.H, x.W, x.C), what)
            if sh > 7 or sw > 7:
                raise NotImplementedError("%s: strides %d, %d, only 1 to 7 are run" % (what, sh, sw))
            T[y] = PlanTensor(y, ho, wo, x.C)
            s.emit(PlanOp(_lib.GRAPH_SLICE, name, x.id, y, stride_h=sh, stride_w=sw,
                          pads=slice_pads(x.H, x.W, ho, wo, sh, sw, -y0, -x0)), i)
        elif name == "RESHAPE":
            shp = g.const(ins[1]) if len(ins) > 1 else None
            shp = [int(v) for v in (shp.reshape(-1) if shp is not None else (op.get("new_shape") or g.tensors[y]["shape"]))]
            dims = shp[1:]
            n_el = x.H * x.W * x.C
            if -1 in dims:
                known = int(np.prod([d for d in dims if d != -1])) if len(dims) > 1 else 1
                dims[dims.index(-1)] = n_el // max(known, 1)
            if len(dims) not in (1, 3) or int(np.prod(dims)) != n_el or min(dims) < 1:
                raise NotImplementedError("%s to shape %s from %d x %d x %d" % (what, shp, x.H, x.W, x.C))
            hwc = (1, 1, dims[0]) if len(dims) == 1 else tuple(dims)
            T[y] = PlanTensor(y, *hwc, root=x.id, alias=True, src_shape=(x.H, x.W, x.C))
            s.producer[y] = s.producer.get(x.id)
        else:
            raise NotImplementedError("%s is not run by the graph executor" % what)
    if gout not in T:
        raise NotImplementedError("tensor %d is not an activation of the graph" % gout)


def resolve_views(s):
    """Follows the chains of roots (a concatenation inside a concatenation; a reshape of a tensor) to the storage: every
    tensor gets its storage, its channel offset in it and the storage's row stride."""
    T = s.T

    def resolve(t):
        r, off = t, 0
        while r.root != r.id:
            if r.alias:
                # a view with another shape needs the storage to be dense in its own right
                parent = T[r.root]
                if parent.root != parent.id and not parent.alias:
                    raise NotImplementedError("RESHAPE of tensor %s, which lives inside a concatenation" % (parent.id,))
            off += r.c_offset
            r = T[r.root]
        return r, off

    for t in list(T.values()):
        r, off = resolve(t)
        t.storage = r.id
        if t.alias:
            if off != 0:
                raise NotImplementedError("RESHAPE of a channel slice")
            t.c_offset, t.c_stride = 0, t.C
        else:
            t.c_offset, t.c_stride = off, r.C
    for t in T.values():
        if t.alias and T[t.storage].H * T[t.storage].W * T[t.storage].C != t.H * t.W * t.C:
            raise NotImplementedError("RESHAPE changes the element count")


def attach_input(s, channel_map, input_mode):
    """The plan's two ends.  The input is the graph's own input tensor, as the caller brings it, or -- with a channel map --
    an external tensor "input" in front of a CHANNEL_MAP operator.  input_mode "caffe" / "torch" plans the INPUT operator
    where the channel map stands: the channel map plus the arithmetic of keras.applications' preprocess_input in those
    modes on the unscaled sample (INPUT_MODES)."""
    T, plan, gin, gout = s.T, s.plan, s.gin, s.gout
    if input_mode is not None and (channel_map is None or T[gin].C != 3):
        raise ValueError("input_mode %r subtracts the means of three colour channels: it needs a channel map and a graph of "
                         "exactly three input channels, not %s and %d" % (input_mode, channel_map, T[gin].C))
    plan.input = gin
    if channel_map is not None:
        cmap = [int(c) for c in channel_map]
        if len(cmap) != T[gin].C or not 1 <= len(cmap) <= 4 or min(cmap) < 0:
            raise ValueError("channel map %s for a graph of %d input channels" % (cmap, T[gin].C))
        plan.input = "input"
        T["input"] = PlanTensor("input", T[gin].H, T[gin].W, max(max(cmap) + 1, 2), storage="input")
        if input_mode is None:
            o = PlanOp(_lib.GRAPH_CHANNEL_MAP, "CHANNEL_MAP", "input", gin, channel_map=cmap)
        else:
            param, shift, scale, _ = INPUT_MODES[input_mode]
            o = PlanOp(_lib.GRAPH_INPUT, "INPUT", "input", gin, channel_map=cmap, param=param, shift=shift.copy(),
                       scale=None if scale is None else scale.copy(), input_mode=input_mode)
        o.source = -1
        s.ops.insert(0, o)
    plan.output = gout
    if T[gout].storage != gout and not T[gout].alias:
        raise NotImplementedError("the output tensor %d lives inside a concatenation" % gout)
    plan.out_storage = T[gout].storage
    if T[plan.input].storage != plan.input:
        raise NotImplementedError("the input tensor lives inside another tensor")
    plan.input_shape = (T[plan.input].H, T[plan.input].W, T[plan.input].C)
    plan.graph_input_shape = (T[gin].H, T[gin].W, T[gin].C)
    plan.output_shape = (T[gout].H, T[gout].W, T[gout].C)


def prune_to_output(s):
    """Drops what the output does not need."""
    T, needed, kept = s.T, {s.plan.out_storage}, []
    for o in reversed(s.ops):
        if T[o.out].storage in needed:
            kept.append(o)
            needed.add(T[o.in0].storage)
            if o.in1 != -1:
                needed.add(T[o.in1].storage)
    s.ops[:] = kept[::-1]


def fold_window_chains(s):
    """fold_windows=True (a NASNet's adjust block and stride-2 separable convolutions, MobileNetV2's stride-2 blocks):
    - a 1 x 1 AVERAGE_POOL_2D / MAX_POOL_2D without an activation is a SLICE: the mean or maximum of one element is it.
      The pool kernel's mean is (0 + e) / 1, which makes +0.0 of a -0.0: the SLICE of an average pool carries param 1 and
      adds 0.0f too (include/cpx.h), so that not even that bit moves;
    - a PAD, a SLICE or such a pool followed by a SLICE or such a pool that reads only inside its input (no positive pad
      of its own) is ONE SLICE, start and stride composed affinely: PAD((0,1),(0,1)) -> [:, 1:, 1:, :] -> 1 x 1 stride 2
      is pad_top = pad_left = -1, stride 2.  A crop followed by a PAD is not composed: its zeros lie inside the original;
    - a PAD whose only reader is a VALID convolution of a kind that takes one (KINDS' pad: CONV_2D / DEPTHWISE_CONV_2D,
      float32, fp16x2 or hybrid; not the grouped kinds), with every pad below the kernel side, is dropped and the reader
      takes its input with the four explicit pads.  Not into MAX_POOL ("padding never wins") nor into a wider AVERAGE_POOL
      ("divided by the in-bounds count"): different arithmetic.
    The dropped tensor must be one of its own (_Build.own_tensor) and read by the folding operator alone; the QUANT_PARAMS
    of a hybrid reader's view and the RANGE of an fp16x2 reader's move to the PAD's input (zeros do not change max |x|).
    Every fold yields the bits of the launches it replaces.  A SLICE moves values.  The depthwise sum is one chain from +0
    in raster order: a tap that the PAD launch made a stored 0 is fmaf(0, w, acc) = acc for finite w (acc is never -0: it
    starts at +0, and x + (+-0) = x, +0 + (+-0) = +0 when rounding to nearest), a tap the kernel masks is skipped -- the same
    acc; the implicit-GEMM patch holds 0 for a padded tap either way and its K walk (tap, chunk) does not change; a hybrid
    padded tap is q = zp, a real 0, whether read or masked, and QUANT_PARAMS already takes rmin = min(0, min x),
    rmax = max(0, max x), which zeros do not move."""
    ops, T = s.ops, s.T
    for o in ops:
        avg = o.kind == _lib.GRAPH_AVG_POOL
        if (avg or o.kind == _lib.GRAPH_MAX_POOL) and (o.kh, o.kw) == (1, 1) and o.act == ACT_NONE:
            a, y = T[o.in0], T[o.out]
            o.param = 1.0 if avg else 0.0
            o.kind, o.pads = _lib.GRAPH_SLICE, slice_pads(a.H, a.W, y.H, y.W, o.stride_h, o.stride_w, 0, 0)
    changed = True
    while changed:
        changed = False
        for b in ops:
            # b reads only inside its input: t[y * sb - pb], no pad of its own.  Behind a: t[y] = in[y * sa - pa] (0
            # outside in), b is in[y * sa * sb - (pb * sa + pa)], 0 outside in -- start and stride compose affinely
            if b.kind != _lib.GRAPH_SLICE or max(b.pads) > 0 or not s.own_tensor(b.in0) or s.readers_of(b.in0) != [b]:
                continue
            a = next((p for p in ops if p.out == b.in0), None)
            if a is None or (a.kind != _lib.GRAPH_PAD and a.kind != _lib.GRAPH_SLICE) or a.act != ACT_NONE or b.act != ACT_NONE \
                    or a.stride_h * b.stride_h > 7 or a.stride_w * b.stride_w > 7:
                continue
            src, y = T[a.in0], T[b.out]
            sh, sw = a.stride_h * b.stride_h, a.stride_w * b.stride_w
            b.pads = slice_pads(src.H, src.W, y.H, y.W, sh, sw, b.pads[0] * a.stride_h + a.pads[0],
                                b.pads[1] * a.stride_w + a.pads[1])
            b.in0, b.stride_h, b.stride_w, b.name = a.in0, sh, sw, a.name + ">" + b.name
            b.param = max(a.param, b.param)   # (+ 0.0f anywhere in a chain of copies is + 0.0f at its end)
            ops.remove(a)
            changed = True
            break
    for p in list(ops):
        if p.kind != _lib.GRAPH_PAD or not s.own_tensor(p.out):
            continue
        readers = s.readers_of(p.out)
        params = [r for r in readers if kind_of(r.kind).params]
        rest = [r for r in readers if not kind_of(r.kind).params]
        if len(rest) != 1:
            continue
        r = rest[0]
        if not kind_of(r.kind).pad or r.in0 != p.out or r.pads != (0, 0, 0, 0) or any(s.readers_of(q.out) != [r] for q in params):
            continue
        pt, pl, pb, pr = p.pads
        if max(pt, pb) >= r.kh or max(pl, pr) >= r.kw:
            continue
        r.in0, r.pads, r.name = p.in0, p.pads, "PAD>" + r.name
        for q in params:
            q.in0 = p.in0
            # the PAD's input may have a RANGE of its own (another fp16x2 reader): one per view, the earlier one
            twin = next((t for t in ops if t is not q and t.kind == _lib.GRAPH_RANGE == q.kind and t.in0 == q.in0), None)
            if twin is not None:
                first, second = (twin, q) if ops.index(twin) < ops.index(q) else (q, twin)
                for c in ops:
                    if c.in1 == second.out:
                        c.in1 = first.out
                ops.remove(second)
        ops.remove(p)


def fuse_preactivations(s, fuse_preactivation, fuse_preactivation_dw):
    """A pre-activation (DenseNet's and ResNetV2's BatchNorm + ReLU IN FRONT of a convolution: MUL + ADD by constants with a
    fused RELU on a tensor that has other readers -- the next concatenation, the shortcut -- so it could not fold into its
    producer and is one AFFINE) is, with fuse_preactivation=True, dropped where every reader of its output is a float32 CONV
    and that output is a tensor of its own (not the graph's output, in no concatenation, no view of it read): those
    convolutions become CONV_PRE (KINDS' pre), read the AFFINE's input -- a channel slice of a concatenated tensor included
    -- and apply the two float32 operations and the activation while they stage the patch, bit for bit what the launch
    did (pack_conv_pre: the constants ride behind the filter image).  A convolution that went fp16x2 or is grouped has no
    CONV_PRE form: its AFFINE stays a launch whatever fuse_preactivation says.
    With fuse_preactivation_dw=True the pass also drops a BARE RELU / RELU6 every reader of which reads it as in0 and is a
    float32 CONV (-> CONV_PRE, scale 1, shift 0), a float32 DWCONV (-> DWCONV_PRE) or a SLICE without an activation (which
    takes it): NASNet's Activation('relu') in front of every separable convolution and of the two paths of an adjust block.
    The hybrid DWCONV_Q8 quantises with the parameters of the STORED tensor and keeps the launch.  The pass runs behind the
    window folds: the PAD between the RELU and a stride-2 depthwise convolution has to be gone first.
    Both keywords yield the bits of the launches they replace: activate() is the one the AFFINE launch ran, and act(0) = 0,
    so it commutes with a SLICE's selection and with zero padding."""
    ops, T = s.ops, s.T
    for o in list(ops):
        if o.kind != _lib.GRAPH_AFFINE or o.copy or o.act not in PRE_ACTS or o.in0 == o.out or o.out == s.gout \
                or not s.own_tensor(o.out):
            continue
        readers = s.readers_of(o.out)
        if not readers or any(r.in0 != o.out or r.in1 == o.out for r in readers):
            continue
        bare = o.scale is None and o.shift is None
        if not (fuse_preactivation and all(r.kind == _lib.GRAPH_CONV for r in readers)) and not (
                fuse_preactivation_dw and bare and all(
                    kind_of(r.kind).pre is not None or (r.kind == _lib.GRAPH_SLICE and r.act == ACT_NONE) for r in readers)):
            continue
        cin = T[o.in0].C
        for r in readers:
            r.in0, conv, pre = o.in0, r.kind == _lib.GRAPH_CONV, kind_of(r.kind).pre
            if pre is None:
                r.act, r.name = o.act, o.name + ">" + r.name
                continue
            r.kind, r.param, r.name = pre, float(o.act), ("AFFINE" if conv else o.name) + ">" + r.name
            if conv:
                r.pre_scale = np.ones(cin, np.float32) if o.scale is None else o.scale
                r.pre_shift = np.zeros(cin, np.float32) if o.shift is None else o.shift
                r.pre_source = o.source
        ops.remove(o)


def check_used_tensors(s):
    """The plan keeps the tensors whose storage an operator touches.  The native graph knows ONE tensor as its input and
    one as its output: no second view of either."""
    plan, T = s.plan, s.T
    used = {t for o in s.ops for t in (o.in0, o.in1, o.out) if t != -1}
    if plan.input not in used:
        raise NotImplementedError("the output does not depend on the input")
    live = set(T[k].storage for k in used)
    for k in [k for k, t in T.items() if t.storage not in live]:
        del T[k]
    for k, t in T.items():
        if (t.storage == plan.input and k != plan.input) or (t.storage == plan.out_storage and k != s.gout):
            raise NotImplementedError("tensor %s is a view of the graph's input or output" % (k,))


def place_arena(s):
    """Tensors get offsets in one arena by the lifetime of their storage (first write to last read, in operator order),
    greedy by size; the offsets are per sample, the arena of a forward over N samples is N times as large.  The plan's
    input and output are the caller's buffers."""
    plan, T = s.plan, s.T
    life = {}
    for k, o in enumerate(s.ops):
        for tid in (o.in0, o.in1, o.out):
            if tid == -1:
                continue
            st = T[tid].storage
            a, b = life.get(st, (k, k))
            life[st] = (min(a, k), max(b, k))
    plan.lifetimes = life
    external = {plan.input, plan.out_storage}
    # (floats per sample; an int8 tensor: its bytes rounded up to floats)
    extent = {k: -(-(T[k].H * T[k].W * T[k].C) // 4) if T[k].dtype == "int8" else T[k].H * T[k].W * T[k].C for k in life}
    sizes = {k: -(-extent[k] // ALIGN) * ALIGN for k in life if k not in external}
    placed = []   # (offset, size, first, last)
    offsets = {}
    for k in sorted(sizes, key=lambda k: (-sizes[k], life[k][0])):
        a, b = life[k]
        busy = sorted((o, z) for o, z, fa, fb in placed if not (fb < a or b < fa))
        off = 0
        for o, z in busy:
            if off + sizes[k] <= o:
                break
            off = max(off, o + z)
        offsets[k] = off
        placed.append((off, sizes[k], a, b))
    plan.arena_floats = max([offsets[k] + extent[k] for k in offsets] or [0])   # (the last tensor unpadded)
    for t in plan.tensors.values():
        t.arena_offset = offsets.get(t.storage, 0)
        t.external = t.storage in external


def pack_weights(ops):
    """Every filter in its kernel's layout (KINDS' pack: CONV_2D filters from TFLite's OHWI to [tap][Cin][Cout], Cin padded
    to 16 and Cout to 32, and so on, each packer says its own); an INT8 filter's scales times what was folded into the
    operator are its `scale`."""
    for o in ops:
        row = kind_of(o.kind)
        if row.pack is not None:
            o.weights = row.pack(o)
            if row.scaled and o.filter_scale is not None:   # the device multiplies by float32(filter scale x folded scale)
                o.scale = o.filter_scale if o.scale is None else (o.filter_scale * o.scale).astype(np.float32)


def pack_conv_filter_q8(w_ohwi):
    """INT8 OHWI [Cout, kh, kw, Cin] -> bytes: [kh * kw][chunks of GRAPH_CONV_Q8_KC input channels][tiles of GRAPH_CONV_CO
    output channels][64 lanes][16], lane l = output channel l & 31 of the tile, input channels 16 * (l >> 5) + j of the
    chunk (the B fragment of v_mfma_i32_32x32x32_i8), zeros beyond Cin and Cout; behind them int32 wsum[Cout rounded up]."""
    w = np.asarray(w_ohwi)
    assert w.dtype == np.int8, w.dtype
    co, kh, kw, ci = w.shape
    KC, CO = _lib.GRAPH_CONV_Q8_KC, _lib.GRAPH_CONV_CO
    nch, nt = -(-ci // KC), -(-co // CO)
    full = np.zeros((nt * CO, kh * kw, nch * KC), np.int8)
    full[:co, :, :ci] = w.reshape(co, kh * kw, ci)
    # [tile, c, tap, chunk, half, j] -> [tap, chunk, tile, half, c, j]
    frag = full.reshape(nt, CO, kh * kw, nch, 2, 16).transpose(2, 3, 0, 4, 1, 5)
    wsum = np.zeros(nt * CO, np.int32)
    wsum[:co] = w.reshape(co, -1).astype(np.int64).sum(axis=1)
    return np.concatenate([np.ascontiguousarray(frag).reshape(-1).view(np.uint8), wsum.view(np.uint8)])


def unpack_conv_filter_q8(packed, shape):
    """The inverse of pack_conv_filter_q8 for a filter of `shape` (OHWI) -> (int8 filter, int32 wsum[Cout])."""
    co, kh, kw, ci = shape
    KC, CO = _lib.GRAPH_CONV_Q8_KC, _lib.GRAPH_CONV_CO
    nch, nt = -(-ci // KC), -(-co // CO)
    n = kh * kw * nch * nt * 64 * 16
    packed = np.asarray(packed, np.uint8)
    assert packed.size == n + 4 * nt * CO, (packed.size, n)
    frag = packed[:n].view(np.int8).reshape(kh * kw, nch, nt, 2, CO, 16)
    full = frag.transpose(2, 4, 0, 1, 3, 5).reshape(nt * CO, kh * kw, nch * KC)
    return np.ascontiguousarray(full[:co, :, :ci]).reshape(co, kh, kw, ci), packed[n:].view(np.int32)[:co].copy()


def _group_rows(w_ohwi, groups):
    w = np.asarray(w_ohwi)
    co = w.shape[0]
    if groups < 2 or co % groups != 0:
        raise ValueError("%d groups for a filter of %d output channels" % (groups, co))
    return [w[g * (co // groups):(g + 1) * (co // groups)] for g in range(groups)]


def pack_conv_filter_grouped(w_ohwi, groups):
    """float32 OHWI [Cout, kh, kw, Cin / groups] of a grouped CONV_2D -> float32, flat: `groups` pack_conv_filter images
    for Cin / groups -> Cout / groups one after another, image g of the filter rows [g * Cout / groups, (g + 1) * Cout /
    groups): byte for byte what pack_conv_filter makes of those rows (include/cpx.h: CPX_GRAPH_CONV_GROUPED)."""
    return np.concatenate([pack_conv_filter(r).reshape(-1) for r in _group_rows(w_ohwi, groups)])


def unpack_conv_filter_grouped(packed, shape, groups):
    """The inverse of pack_conv_filter_grouped for a filter of `shape` (OHWI, I = Cin / groups)."""
    co, kh, kw, ci = shape
    cog = co // groups
    cip = -(-ci // _lib.GRAPH_CONV_KC) * _lib.GRAPH_CONV_KC
    cop = -(-cog // _lib.GRAPH_CONV_CO) * _lib.GRAPH_CONV_CO
    img = np.asarray(packed, np.float32).reshape(groups, kh * kw, cip, cop)[:, :, :ci, :cog]
    # [g, tap, ci, co] -> [g, co, tap, ci]
    return np.ascontiguousarray(img.transpose(0, 3, 1, 2)).reshape(co, kh, kw, ci)


def pack_conv_filter_q8_grouped(w_ohwi, groups):
    """INT8 OHWI [Cout, kh, kw, Cin / groups] of a grouped CONV_2D -> bytes: `groups` fragment images of
    pack_conv_filter_q8 for Cin / groups -> Cout / groups one after another (image g of the filter rows of group g, byte
    for byte what pack_conv_filter_q8 makes of them), then int32 wsum[groups][Cout / groups rounded up to GRAPH_CONV_CO],
    each group's own rows summed (include/cpx.h: CPX_GRAPH_CONV_Q8_GROUPED)."""
    images, wsums = [], []
    for r in _group_rows(w_ohwi, groups):
        one = pack_conv_filter_q8(r)
        nws = 4 * (-(-r.shape[0] // _lib.GRAPH_CONV_CO) * _lib.GRAPH_CONV_CO)
        images.append(one[:-nws])
        wsums.append(one[-nws:])
    return np.concatenate(images + wsums)


def unpack_conv_filter_q8_grouped(packed, shape, groups):
    """The inverse of pack_conv_filter_q8_grouped for a filter of `shape` (OHWI, I = Cin / groups) -> (int8 filter, int32
    wsum[Cout])."""
    co, kh, kw, ci = shape
    cog = co // groups
    KC, CO = _lib.GRAPH_CONV_Q8_KC, _lib.GRAPH_CONV_CO
    n = kh * kw * (-(-ci // KC)) * (-(-cog // CO)) * 64 * 16
    nws = 4 * (-(-cog // CO) * CO)
    packed = np.asarray(packed, np.uint8)
    assert packed.size == groups * (n + nws), (packed.size, n, nws)
    parts = [unpack_conv_filter_q8(np.concatenate([packed[g * n:(g + 1) * n], packed[groups * n + g * nws:groups * n + (g + 1) * nws]]),
                                   (cog, kh, kw, ci)) for g in range(groups)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def split_filter_f16x2(w_ohwi):
    """float32 OHWI [Cout, kh, kw, Cin] -> (wh, wl, kw): kw[c] = clamp(4 - e, -100, 100) with max |w[c]| = f * 2^e, f in
    [0.5, 1), which puts max |w[c]| * 2^kw[c] in [8, 16) (an all-zero or non-finite filter: kw = 0); wh = fp16(w * 2^kw)
    rounded to nearest even, wl = fp16(w * 2^kw - wh), the difference exact in float32 (include/cpx.h: CONV_F16X2)."""
    w = np.ascontiguousarray(w_ohwi, np.float32)
    m = np.abs(w.reshape(w.shape[0], -1)).max(axis=1) if w.size else np.zeros(w.shape[0], np.float32)
    ok = (m > 0) & np.isfinite(m)
    e = np.frexp(np.where(ok, m, np.float32(8.0)))[1]   # (8 = 0.5 * 2^4: kw = 0)
    kw = np.clip(4 - e, -100, 100).astype(np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        ws = (w * np.ldexp(np.float32(1.0), kw).astype(np.float32)[:, None, None, None]).astype(np.float32)
        wh = ws.astype(np.float16)
        wl = (ws - wh.astype(np.float32)).astype(np.float16)
    return wh, wl, kw


def pack_conv_filter_f16x2(w_ohwi):
    """float32 OHWI [Cout, kh, kw, Cin] -> bytes: fp16 [kh * kw][chunks of GRAPH_CONV_H2_KC input channels][tiles of
    GRAPH_CONV_CO output channels][plane: wh, wl][k half m][64 lanes][8], lane l = output channel l & 31 of the tile, input
    channels 16 * m + 8 * (l >> 5) + j of the chunk (the B fragment of v_mfma_f32_32x32x16_f16), zeros beyond Cin and Cout;
    behind them float32 wdown[Cout rounded up] = 2^-kw (split_filter_f16x2; 1 beyond Cout)."""
    wh, wl, kwc = split_filter_f16x2(w_ohwi)
    co, kh, kw, ci = wh.shape
    KC, CO = _lib.GRAPH_CONV_H2_KC, _lib.GRAPH_CONV_CO
    nch, nt = -(-ci // KC), -(-co // CO)
    full = np.zeros((2, nt * CO, kh * kw, nch * KC), np.float16)
    full[0, :co, :, :ci] = wh.reshape(co, kh * kw, ci)
    full[1, :co, :, :ci] = wl.reshape(co, kh * kw, ci)
    # [plane, tile, c, tap, chunk, m, half, j] -> [tap, chunk, tile, plane, m, half, c, j]
    frag = full.reshape(2, nt, CO, kh * kw, nch, 2, 2, 8).transpose(3, 4, 1, 0, 5, 6, 2, 7)
    wdown = np.ones(nt * CO, np.float32)
    wdown[:co] = np.ldexp(np.float32(1.0), -kwc).astype(np.float32)
    return np.concatenate([np.ascontiguousarray(frag).reshape(-1).view(np.uint8), wdown.view(np.uint8)])


def unpack_conv_filter_f16x2(packed, shape):
    """The inverse of pack_conv_filter_f16x2 for a filter of `shape` (OHWI) -> (wh, wl, kw): the two fp16 planes and
    the int32 exponents of split_filter_f16x2."""
    co, kh, kw, ci = shape
    KC, CO = _lib.GRAPH_CONV_H2_KC, _lib.GRAPH_CONV_CO
    nch, nt = -(-ci // KC), -(-co // CO)
    n = 2 * kh * kw * nch * nt * 4 * 64 * 8
    packed = np.asarray(packed, np.uint8)
    assert packed.size == n + 4 * nt * CO, (packed.size, n)
    frag = packed[:n].view(np.float16).reshape(kh * kw, nch, nt, 2, 2, 2, CO, 8)
    full = frag.transpose(3, 2, 6, 0, 1, 4, 5, 7).reshape(2, nt * CO, kh * kw, nch * KC)
    planes = np.ascontiguousarray(full[:, :co, :, :ci]).reshape(2, co, kh, kw, ci)
    kwc = (-np.frexp(packed[n:].view(np.float32)[:co])[1] + 1).astype(np.int32)   # wdown = 0.5 * 2^(1 - kw)
    return planes[0], planes[1], kwc


def pack_fc_filter_q8(w):
    """INT8 [Cout][Cin] -> bytes: int8 [Cout][Cin rounded up to 4] (zeros beyond), then int32 wsum[Cout]."""
    w = np.asarray(w)
    assert w.dtype == np.int8, w.dtype
    co, ci = w.shape
    full = np.zeros((co, -(-ci // 4) * 4), np.int8)
    full[:, :ci] = w
    wsum = w.astype(np.int64).sum(axis=1).astype(np.int32)
    return np.concatenate([full.reshape(-1).view(np.uint8), wsum.view(np.uint8)])


def pack_dw_filter(w_1hwc):
    """A depthwise filter [1, kh, kw, C] -> float32 [kh * kw][C rounded up to 4], zeros beyond."""
    _, kh, kw, c = w_1hwc.shape
    out = np.zeros((kh * kw, -(-c // 4) * 4), np.float32)
    out[:, :c] = np.asarray(w_1hwc, np.float32).reshape(kh * kw, c)
    return out


def unpack_dw_filter(packed, shape):
    """The inverse of pack_dw_filter for a filter of `shape` ([1, kh, kw, C])."""
    _, kh, kw, c = shape
    return np.ascontiguousarray(np.asarray(packed, np.float32).reshape(kh * kw, -1)[:, :c]).reshape(1, kh, kw, c)


def pack_dw_filter_q8(w_1hwc):
    """An INT8 depthwise filter [1, kh, kw, C] -> bytes: int8 [kh * kw][C rounded up to 4] (zeros beyond), then int32
    wsum[C rounded up to 4], the filter summed over its taps."""
    w = np.asarray(w_1hwc)
    assert w.dtype == np.int8, w.dtype
    _, kh, kw, c = w.shape
    cp = -(-c // 4) * 4
    full = np.zeros((kh * kw, cp), np.int8)
    full[:, :c] = w.reshape(kh * kw, c)
    wsum = np.zeros(cp, np.int32)
    wsum[:c] = w.reshape(kh * kw, c).astype(np.int64).sum(axis=0)
    return np.concatenate([full.reshape(-1).view(np.uint8), wsum.view(np.uint8)])


def unpack_dw_filter_q8(packed, shape):
    """The inverse of pack_dw_filter_q8 for a filter of `shape` -> (int8 filter, int32 wsum[C])."""
    _, kh, kw, c = shape
    cp = -(-c // 4) * 4
    packed = np.asarray(packed, np.uint8)
    assert packed.size == kh * kw * cp + 4 * cp, packed.size
    full = packed[:kh * kw * cp].view(np.int8).reshape(kh * kw, cp)
    return np.ascontiguousarray(full[:, :c]).reshape(1, kh, kw, c), packed[kh * kw * cp:].view(np.int32)[:c].copy()


def pack_conv_filter(w_ohwi):
    """TFLite OHWI [Cout, kh, kw, Cin] -> [kh * kw][Cin rounded up to 16][Cout rounded up to 32], zeros beyond."""
    co, kh, kw, ci = w_ohwi.shape
    cip = -(-ci // _lib.GRAPH_CONV_KC) * _lib.GRAPH_CONV_KC
    cop = -(-co // _lib.GRAPH_CONV_CO) * _lib.GRAPH_CONV_CO
    out = np.zeros((kh * kw, cip, cop), np.float32)
    out[:, :ci, :co] = np.transpose(np.asarray(w_ohwi, np.float32), (1, 2, 3, 0)).reshape(kh * kw, ci, co)
    return out


def pack_conv_pre(w_ohwi, pre_scale, pre_shift):
    """The weights of a CONV_PRE, flat: the pack_conv_filter image, then pre_scale and pre_shift, each Cin rounded up to
    GRAPH_CONV_KC with zeros beyond."""
    ci = w_ohwi.shape[3]
    cip = -(-ci // _lib.GRAPH_CONV_KC) * _lib.GRAPH_CONV_KC
    consts = np.zeros((2, cip), np.float32)
    consts[0, :ci], consts[1, :ci] = pre_scale, pre_shift
    return np.concatenate([pack_conv_filter(w_ohwi).reshape(-1), consts.reshape(-1)])


def load_plan(path, **options):
    """-> (Graph, build_plan(Graph, **options)) of the flatbuffer at `path`."""
    from .tflite_reader import Graph

    with open(str(path), "rb") as fh:
        g = Graph(fh.read())
    return g, build_plan(g, **options)


class GraphDevice:
    """A plan resident on one engine's GPU: constants uploaded once, one native graph (cpx_graph_create) on the
    engine's handle; forward() is one cpx_graph_forward call = one launch per planned operator on the engine's stream."""

    def __init__(self, engine, plan, out_slice=None):
        """out_slice = (c_offset, c_stride): the output goes into that channel slice of the caller's [N, H, W, c_stride]
        buffer (forward's `out`), whose other channels are left alone."""
        self.eng, self.lib, self.torch, self.plan = engine, engine.lib, engine.torch, plan
        self.out_slice = out_slice
        t = self.torch
        self._const = []   # device tensors the native graph points into

        def up(a):
            if a is None:
                return None
            # (the packed int8 filters of the hybrid operators travel as bytes)
            d = t.from_numpy(np.array(a, dtype=np.uint8 if a.dtype == np.uint8 else np.float32, order="C")).to(engine.device)
            self._const.append(d)
            return d.data_ptr()

        ids = {tid: k for k, tid in enumerate(plan.tensors)}
        tens = (_lib.GraphTensor * len(ids))()
        for tid, k in ids.items():
            p = plan.tensors[tid]
            tens[k].H, tens[k].W, tens[k].C = p.H, p.W, p.C
            tens[k].c_offset, tens[k].c_stride, tens[k].arena_offset = p.c_offset, p.c_stride, p.arena_offset
            tens[k].type = _lib.GRAPH_TYPE_INT8 if p.dtype == "int8" else _lib.GRAPH_TYPE_FLOAT32
            if out_slice is not None and tid == plan.output:
                tens[k].c_offset, tens[k].c_stride = out_slice
        out_id = plan.output
        ops = (_lib.GraphOp * len(plan.ops))()
        for k, o in enumerate(plan.ops):
            n = ops[k]
            n.kind, n.in0, n.in1, n.out = o.kind, ids[o.in0], (ids[o.in1] if o.in1 != -1 else -1), ids[o.out]
            n.kh, n.kw, n.stride_h, n.stride_w = o.kh, o.kw, o.stride_h, o.stride_w
            n.pad_top, n.pad_left, n.pad_bottom, n.pad_right = o.pads
            n.activation = o.act
            n.out_c_offset, n.out_c_stride = tens[ids[o.out]].c_offset, tens[ids[o.out]].c_stride
            n.param = o.param
            if o.channel_map is not None:
                n.n_map = len(o.channel_map)
                for c, v in enumerate(o.channel_map):
                    n.channel_map[c] = v
            if kind_of(o.kind).grouped:
                n.n_map = o.groups   # (a convolution has no channel map: the field carries the number of groups)
            n.weights, n.scale, n.shift = up(o.weights), up(o.scale), up(o.shift)
        self._graph = None   # (what close() finds when the creation below refuses the plan)
        graph = C.c_void_p()
        engine.call("cpx_graph_create", ops, len(plan.ops), tens, len(ids), ids[plan.input], ids[out_id], C.byref(graph))
        self._graph = graph

    def arena_bytes(self, N):
        v = C.c_size_t()
        self.eng.call("cpx_graph_arena_bytes", int(N), C.byref(v), on=self._graph)
        return int(v.value)

    def arena_allocated(self):
        v = C.c_size_t()
        self.eng.status("cpx_graph_arena_allocated", C.byref(v))
        return int(v.value)

    def forward(self, x, out=None):
        """x: device float32 [N, H, W, C] of plan.input_shape -> device float32 [N, C_out] (or [N, H, W, C_out])."""
        t = self.torch
        H, W, Cin = self.plan.input_shape
        assert x.dtype == t.float32 and x.is_contiguous() and tuple(x.shape[1:]) == (H, W, Cin), (tuple(x.shape), self.plan.input_shape)
        N = int(x.shape[0])
        t.cuda.current_stream(self.eng.device).synchronize()
        oh, ow, oc = self.plan.output_shape
        if self.out_slice is not None:
            assert out is not None and out.is_contiguous() and tuple(out.shape) == (N, oh, ow, self.out_slice[1])
        if out is None:
            out = t.empty((N, oc) if (oh, ow) == (1, 1) else (N, oh, ow, oc), dtype=t.float32, device=self.eng.device)
        self._enqueue(x, N, out)
        self.eng.synchronize()
        return out

    def _enqueue(self, x, N, out):
        for attempt in range(2):
            rc = self.eng.status("cpx_graph_forward", x, N, out, on=self._graph)
            if rc == -6 and attempt == 0:   # CPX_ERR_NOMEM: the arena is a plain hipMalloc; torch's cache is invisible to it
                self.eng.synchronize()
                self.torch.cuda.empty_cache()
                continue
            break
        self.eng.check(rc)

    def forward_async(self, x, out):
        """forward() for a caller that orders its work by the engine's stream (the batched pipeline): the launches are
        enqueued behind what that stream holds, straight into the caller's `out` ([N, C_out], or a view of its rows);
        no host synchronisation before or after and no allocation -- unless the handle's arena has to grow."""
        H, W, Cin = self.plan.input_shape
        assert x.dtype == self.torch.float32 and x.is_contiguous() and tuple(x.shape[1:]) == (H, W, Cin), (tuple(x.shape), self.plan.input_shape)
        N = int(x.shape[0])
        assert self.out_slice is None and out.dtype == self.torch.float32 and out.is_contiguous() and \
            out.numel() == N * int(np.prod(self.plan.output_shape)), tuple(out.shape)
        self._enqueue(x, N, out)

    def close(self):
        if self._graph is not None:
            if self.eng.h:   # a closed engine has already freed its graphs
                self.lib.cpx_graph_destroy(self._graph)
            self._graph = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GraphNetwork:
    """A GraphDevice behind the batched pipeline's network protocol (WRResNetDevice's: `.eng` and
    forward_async(x, logits, probs) on the engine's stream).  A graph hands out one tensor -- the probabilities -- so
    there are no logits (has_logits: the pipeline allocates none and reports None)."""

    has_logits = False

    def __init__(self, dev):
        self.dev, self.eng = dev, dev.eng
        # a forward over N samples holds N times this much arena: the pipeline clamps its chunk to its memory budget
        self.arena_bytes_per_sample = dev.plan.arena_bytes_per_sample

    def forward_async(self, x, logits, probs):
        assert logits is None
        self.dev.forward_async(x, probs)
