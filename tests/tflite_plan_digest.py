"""Helper (not a test): the corpus of graphs and build_plan options whose plans tests/test_tflite_plan_digest_cpu.py pins,
and digest(plan): a SHA-256 over everything GraphDevice hands to the device -- the plan's own fields, every tensor and
every operator with the bytes of its weights, scale and shift, in the plan's order.  A plan that differs in one launch, one
weight byte or one arena offset has another digest; a combination the planner refuses is recorded as the exception's type
and text.  The golden (tests/golden/tflite_plan_digests.json) is written by tests/golden/make_golden_plan_digests.py."""
import hashlib

import numpy as np

import tflite_build as tb
import tflite_build_dw as td
import tflite_build_nas as tn
import tflite_build_preact as tp
import tflite_build_q8 as tq
import tflite_build_se as ts


def fc_reshape_add():
    """-> flatbuffer bytes: MEAN -> FULLY_CONNECTED -> RESHAPE to [1, 1, 1, C] -> ADD of a constant -> LOGISTIC: the
    constant's fold asks for the producer of a VIEW (the RESHAPE hands its input's producer on), and FULLY_CONNECTED takes
    neither constants nor a LOGISTIC."""
    rng = np.random.default_rng(11)
    m = tb.Model()
    x = m.tensor([1, 5, 5, 12], name="input")
    m.inputs = [x]
    y = m.dense(m.mean(x), rng.normal(0, 0.3, size=(10, 12)).astype(np.float32), rng.normal(0, 0.1, size=10).astype(np.float32))
    y = m.binary("ADD", m.reshape(y, [1, 1, 1, 10]), rng.normal(0, 0.1, size=10).astype(np.float32))
    m.outputs = [m.unary("LOGISTIC", y)]
    return m.finish()


def conv_reshape_add(shape=(1, 2, 2, 4)):
    """-> flatbuffer bytes: CONV_2D (1 x 1 on a 2 x 2 x 6 input, 4 channels) -> RESHAPE to `shape` -> ADD of a constant of
    shape[-1] values -> RELU.  The convolution IS a fold target and the tensor the ADD reads is a view of its output, not
    its output: the one case in which the constants' guard (no `p.out == x.id`) and the swish / LOGISTIC guards differ.
    (A shape of other channels, [1, 16], ends in NumPy's broadcast error, whose text is no fixture: not in the corpus.)"""
    rng = np.random.default_rng(12)
    m = tb.Model()
    x = m.tensor([1, 2, 2, 6], name="input")
    m.inputs = [x]
    y = m.conv(x, rng.normal(0, 0.3, size=(4, 1, 1, 6)).astype(np.float32), rng.normal(0, 0.1, size=4).astype(np.float32))
    y = m.binary("ADD", m.reshape(y, list(shape)), rng.normal(0, 0.1, size=shape[-1]).astype(np.float32))
    m.outputs = [m.unary("RELU", y)]
    return m.finish()


def _wr_weights():
    from cpx.ml_tools import wrresnet as wr

    return wr.random_weights(17, seed=5)


# name -> (builder of the flatbuffer's bytes, the graph reads three colour channels)
GRAPHS = {
    "inception_v3": (lambda: tb.inception_v3(6, (16,), seed=1, width=0.25), True),
    "mobilenet_v2": (lambda: td.mobilenet_v2(6, size=64, width=0.35), True),
    "efficientnet_b0": (lambda: ts.efficientnet_b0(6, size=64, width=0.5), True),
    "efficientnet_b0_div_reshape": (lambda: ts.efficientnet_b0(6, size=64, width=0.5, normalisation_div=True, se_reshape=True), True),
    "densenet": (lambda: tp.densenet(6, blocks=(2, 2), growth=8, seed=1), True),
    "resnet_v2": (lambda: tp.resnet_v2(6, seed=1), True),
    "nasnet": (lambda: tn.nasnet(6), True),
    "nasnet_as_slice": (lambda: tn.nasnet(17, as_slice=True), True),
    "nasnet_merge_relus": (lambda: tn.nasnet(6, merge_relus=True), True),
    "wrresnet": (lambda: tb.wrresnet(_wr_weights()), False),
    "inception_v3_q8": (lambda: tq.quantise(tb.inception_v3(6, (16,), seed=1, width=0.25)), True),
    "mobilenet_v2_q8": (lambda: td.quantise(td.mobilenet_v2(6, size=64, width=0.35)), True),
    "efficientnet_b0_q8": (lambda: td.quantise(ts.efficientnet_b0(6, size=64, width=0.5)), True),
    "wrresnet_q8": (lambda: tq.quantise(tb.wrresnet(_wr_weights())), False),
    "adjust_block": (lambda: tn.adjust_block(), False),
    "adjust_block_as_slice": (lambda: tn.adjust_block(as_slice=True), False),
    "inception_resnet_block": (lambda: tn.inception_resnet_block(), False),
    "pad_conv": (lambda: tn.pad_then("conv"), False),
    "pad_dw_stride2": (lambda: tn.pad_then("dw", pads=((0, 1), (0, 1)), stride=2), False),
    "pad_max_pool": (lambda: tn.pad_then("MAX_POOL_2D"), False),
    "pad_avg_pool": (lambda: tn.pad_then("AVERAGE_POOL_2D"), False),
    "pad_conv_extra_reader": (lambda: tn.pad_then("conv", extra_reader=True), False),
    "pad_conv_as_output": (lambda: tn.pad_then("conv", as_output=True), False),
    "pad_conv_hybrid": (lambda: tn.pad_then("conv", hybrid=True), False),
    "pad_dw_hybrid": (lambda: tn.pad_then("dw", hybrid=True, c=72), False),
    "fc_reshape_add": (fc_reshape_add, False),
    "conv_reshape_add": (conv_reshape_add, False),
}

FOLDS = dict(fuse_preactivation=True, fold_windows=True, fuse_preactivation_dw=True)
# every graph is planned with each of these (grouped_convolutions=True throughout); "caffe" wants three colour channels
OPTION_SETS = {
    "defaults": {},
    "no_fused_activations": dict(fuse_activations=False),
    "preact": dict(fuse_preactivation=True),
    "windows": dict(fold_windows=True),
    "folds": FOLDS,
    "fp16x2_folds": dict(FOLDS, conv_math="fp16x2"),
    "float_math": dict(quantised_math="float"),
    "caffe": dict(channel_map=[0, 1, 1], input_mode="caffe"),
}
# (graph, name of the entry, options): what the cross above leaves out.  The inner outputs are operator indices of the
# flatbuffer (the output of that operator), chosen by reading the graphs: a tensor of its own in the middle of the network
EXTRA = [
    ("wrresnet", "caffe", dict(channel_map=[0, 1, 1], input_mode="caffe", grouped_convolutions=True)),
    ("wrresnet_q8", "caffe", dict(channel_map=[0, 1, 1], input_mode="caffe", grouped_convolutions=True)),
    ("wrresnet", "ungrouped", dict(grouped_convolutions=False)),
    ("wrresnet_q8", "ungrouped", dict(grouped_convolutions=False)),
    ("wrresnet", "map", dict(channel_map=[1, 0], grouped_convolutions=True)),
    ("mobilenet_v2", "torch", dict(channel_map=[0, 1, 2], input_mode="torch", grouped_convolutions=True)),
    ("mobilenet_v2_q8", "torch_folds", dict(FOLDS, channel_map=[2, 1, 0], input_mode="torch", grouped_convolutions=True)),
    ("mobilenet_v2", "map", dict(channel_map=[1, 0, 0], grouped_convolutions=True)),
    ("inception_v3", "map4", dict(channel_map=[3, 0, 2], grouped_convolutions=True)),
    ("mobilenet_v2", "input_shape", dict(input_shape=(48, 80, 3), grouped_convolutions=True)),
    ("nasnet", "input_shape_folds", dict(FOLDS, input_shape=(96, 64, 3), grouped_convolutions=True)),
    ("inception_v3", "inner_output", dict(output_of=40, grouped_convolutions=True)),
    ("densenet", "inner_output_folds", dict(FOLDS, output_of=12, grouped_convolutions=True)),
    ("efficientnet_b0_q8", "inner_output", dict(output_of=47, grouped_convolutions=True)),
    ("inception_v3", "output_concatenation", dict(output_of=39, grouped_convolutions=True)),
]


def entries():
    """-> [(key, graph name, build_plan options)] in a fixed order."""
    out = []
    for name, (_, rgb) in GRAPHS.items():
        for oname, options in OPTION_SETS.items():
            if rgb or oname != "caffe":
                out.append(("%s|%s" % (name, oname), name, dict(options, grouped_convolutions=True)))
    return out + [("%s|%s" % (name, oname), name, dict(options)) for name, oname, options in EXTRA]


def _canon(v):
    """ids and shapes as plain Python values, so that an int and a NumPy int are one key."""
    if isinstance(v, (tuple, list)):
        return type(v)(_canon(e) for e in v)
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    return v


def digest(plan):
    h = hashlib.sha256()

    def put(*values):
        for v in values:
            h.update(repr(_canon(v)).encode() + b"\n")

    def put_array(a):
        if a is None:
            put(None)
        else:
            a = np.asarray(a)
            put(str(a.dtype), a.shape)
            h.update(np.ascontiguousarray(a).tobytes() + b"\n")

    put(plan.input, plan.output, plan.input_shape, plan.graph_input_shape, plan.output_shape, plan.arena_floats,
        plan.out_storage, sorted(plan.lifetimes.items(), key=repr))
    put(len(plan.tensors))
    for key, t in plan.tensors.items():
        put(key, t.H, t.W, t.C, t.storage, t.c_offset, t.c_stride, t.arena_offset, t.alias, t.external)
    put(len(plan.ops))
    for o in plan.ops:
        put(o.kind, o.name, o.in0, o.in1, o.out, o.kh, o.kw, (o.stride_h, o.stride_w), tuple(o.pads), o.act, o.param,
            None if o.channel_map is None else list(o.channel_map), o.copy, o.source, getattr(o, "groups", 1))
        for a in (o.weights, o.scale, o.shift):
            put_array(a)
    return h.hexdigest()


def compute():
    """-> {key: {"digest": hex} | {"refused": "ExceptionType: text"}} for every entry, in entries()' order."""
    from cpx.ml_tools.tflite_graph import build_plan
    from cpx.ml_tools.tflite_reader import Graph

    blobs, out = {}, {}
    for key, name, options in entries():
        if name not in blobs:
            blobs[name] = GRAPHS[name][0]()
        g = Graph(blobs[name])   # (a fresh one per plan: no entry sees what another left in a graph's caches)
        if "output_of" in options:
            options["output"] = g.ops[options.pop("output_of")]["outputs"][0]
        try:
            out[key] = {"digest": digest(build_plan(g, **options))}
        except (NotImplementedError, ValueError) as e:
            out[key] = {"refused": "%s: %s" % (type(e).__name__, e)}
    return out
