#!/usr/bin/env python3
"""A released TFLite WR-ResNet model (.tflite) -> the <out_base>.npz the cpx kernels read -- in pure Python: the
flatbuffer is parsed here, TensorFlow is not needed (only NumPy).

    python tools/tflite_to_npz.py model.tflite /tmp/wr [--sidecar model.json]
    python tools/tflite_to_npz.py --describe model.tflite
    python tools/tflite_to_npz.py --dequantise quantised.tflite /tmp/wr

--dequantise writes the .npz of a dynamic-range quantised WR-ResNet (what the reference's converter writes,
src/tfliteconverter.py:54-62): every INT8 filter multiplied out, float32(int8) * scale -- the float32 network the file
stands for, which the fused kernels run (CPX_TFLITE_QUANT_MATH=float does the same on load).  Without it such a file is
refused by the name of its first INT8 tensor.  --describe plans a grouped CONV_2D as LiteInterpreter does
(grouped_convolutions=True) and prints each grouped convolution's G, the hybrid ones marked and counted in the census.  A
full-integer file (INT8 activations, QUANTIZE / DEQUANTIZE) is planned as LiteInterpreter plans it too
(integer_activations=True, integer_gate_mul=True, integer_lut=True): the tensor types and the smaller per-sample arena are
printed, the 256-entry tables an INT8 LOGISTIC or swish became -- folded into the convolution in front (CONV_2D+SWISH,
CONV_2D+LOGISTIC in the census) or a LUT_I8 launch of their own (SWISH, LOGISTIC) -- or the refusal.

--describe converts nothing: it prints the operator census, the input and output shapes, the arena bytes per sample and,
for a dynamic-range quantised file, the number of hybrid operators with the int8 against the float32 weight bytes of ANY graph the device executor runs (cpx/ml_tools/tflite_graph.py: an Inception-v3, a MobileNetV2 or an EfficientNet, say; the launches carry what was folded into them: CONV_2D+SWISH, CONV_2D+LOGISTIC, CONV_2D+MUL+ADD, AFFINE>CONV_2D for a folded pre-activation; a second line gives the launches with the window folds on, as LiteInterpreter runs the file: PAD>DEPTHWISE_CONV_2D, RELU>DEPTHWISE_CONV_2D, PAD>STRIDED_SLICE>AVERAGE_POOL_2D), or the refusal -- the
operator and its index -- of one it does not.  With a sidecar JSON beside the file (or --sidecar) it also prints the
family's input mode.

The reference loads this artefact with LiteInterpreter (/root/reference/src/ml_tools/interpreter.py:520-560); its CI
downloads it (.github/workflows/release.yml:46) and tests/clips/possum.txt's prediction came from one.  Anyone holding
the released file can therefore pin row a20 (CNN logits) of SURVEY section 8 without a TensorFlow installation:
convert, then run tests/test_tf_parity_gpu.py against outputs recorded with the TFLite runtime.

What is read: the float32 graph of WR-ResNet-22-4 (src/ml_tools/resnet/wr_resnet.py:5-98) as the TFLite converter
writes it -- CONV_2D (filter OHWI, bias, fused ReLU: a convolution with the BatchNorm that follows it folded in), MUL +
ADD by per-channel constants (a BatchNorm that follows a residual ADD cannot be folded: scale and shift), RELU, ADD of
two activations (the residual), MEAN (global average pooling), FULLY_CONNECTED, LOGISTIC / SOFTMAX.  The walk follows
the operators in order and fills the Keras-layout names of cpx/ml_tools/wrresnet.py; a folded or affine-only BatchNorm
becomes gamma = scale, beta = shift, moving_mean = 0, moving_variance = 1 - eps (so that the loader's
gamma / sqrt(var + eps) gives the scale back exactly).  Anything else (quantised tensors, another topology) is refused
with the operator that stopped the walk."""
import argparse
import os
import shutil
import sys

import numpy as np

# the reader lives in the package (cpx.ml_tools.tflite_reader: get_interpreter converts a .tflite on load with it)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "classifier-pipeline_amd"))
from cpx.ml_tools.tflite_reader import (BN_EPS, OPS, Graph, Table, bn_params, conv_kernel, convert,  # noqa: E402,F401
                                        identity_variance)


def input_mode_of(sidecar):
    """-> (model_name, 'caffe' | 'torch' | 'tf' | None) of a sidecar JSON, as LiteInterpreter reads it."""
    import json

    from cpx.ml_tools.hyperparams import HyperParams
    from cpx.ml_tools.interpreter import Interpreter, LiteInterpreter

    hp = HyperParams()
    with open(sidecar, "r") as fh:
        hp.update(json.load(fh).get("hyperparams", {}))
    name = hp.model_name
    return name, LiteInterpreter.INPUT_MODE_OF.get(name, "tf" if name in Interpreter.TF_SCALED_MODELS else None)


def describe(g, sidecar=None, conv_math="f32"):
    from cpx.ml_tools.tflite_graph import build_plan

    I8 = dict(integer_activations=True, integer_gate_mul=True, integer_lut=True)   # a full-integer file, as LiteInterpreter plans it
    census = {}
    for op in g.ops:
        census[op["name"]] = census.get(op["name"], 0) + 1
    print("operators: " + ", ".join("%s: %d" % kv for kv in sorted(census.items())))
    try:
        # every PAD, 1 x 1 pool and slice a launch (CPX_TFLITE_FOLD_WINDOWS=0), and what LiteInterpreter runs
        unfolded = build_plan(g, fuse_preactivation=True, grouped_convolutions=True, **I8)
        plan = build_plan(g, fuse_preactivation=True, fuse_preactivation_dw=True, fold_windows=True, grouped_convolutions=True, **I8)
    except NotImplementedError as e:
        print("refused: %s" % e)
        return 1
    print("input shape %s, output shape %s" % (list(plan.input_shape), list(plan.output_shape)))
    print("launches: " + ", ".join("%s: %d" % kv for kv in sorted(unfolded.census().items())))
    print("folded launches (%d of %d): " % (len(plan.ops), len(unfolded.ops)) + ", ".join("%s: %d" % kv for kv in sorted(plan.census().items())))
    print("arena bytes per sample: %d (unfolded: %d)" % (plan.arena_bytes_per_sample, unfolded.arena_bytes_per_sample))
    from cpx.ml_tools.tflite_graph import GROUPED_KINDS, I8_FILTER_KINDS, Q8_KINDS

    n8 = sum(t.dtype == "int8" for t in plan.tensors.values())
    if n8:
        # a full-integer file: int8 activations between QUANTIZE and DEQUANTIZE, an arena counted in bytes
        full = [o for o in plan.ops if o.kind in I8_FILTER_KINDS]
        print("tensor types: %d int8, %d float32; full-integer filter operators (int8 in, int8 out): %d, int8 weight bytes: %d"
              % (n8, len(plan.tensors) - n8, len(full), sum(int(np.prod(o.filter.shape)) for o in full)))
        from cpx import _lib

        print("tables (an INT8 LOGISTIC or swish as 256 entries): %d folded into their convolutions, %d LUT_I8 launches; gate MUL_I8: %d"
              % (sum(o.act == _lib.GRAPH_ACT_LUT for o in plan.ops), sum(o.kind == _lib.GRAPH_LUT_I8 for o in plan.ops),
                 sum(o.kind == _lib.GRAPH_MUL_I8 and o.in1 != -1 and plan.tensors[o.in1].H * plan.tensors[o.in1].W == 1
                     < plan.tensors[o.out].H * plan.tensors[o.out].W for o in plan.ops)))
    grouped = [o for o in plan.ops if o.kind in GROUPED_KINDS]
    if grouped:
        print("grouped convolutions: %d (%d hybrid): " % (len(grouped), sum(o.kind in Q8_KINDS for o in grouped))
              + ", ".join("operator %d: G = %d%s" % (o.source, o.groups, " (hybrid)" if o.kind in Q8_KINDS else "") for o in grouped))
    hybrid = [o for o in plan.ops if o.kind in Q8_KINDS]
    q8 = sum(int(np.prod(o.filter.shape)) for o in hybrid)
    f32 = sum(4 * int(np.prod((o.filter if getattr(o, "filter", None) is not None else o.weights).shape)) for o in plan.ops
              if o.kind not in Q8_KINDS and o.kind not in I8_FILTER_KINDS and o.weights is not None and o.weights.dtype != np.uint8)
    print("hybrid operators (int8 filter, activations quantised per sample): %d; int8 weight bytes: %d, float32 weight bytes: %d"
          % (len(hybrid), q8, f32))
    if conv_math != "f32":
        # what CPX_TFLITE_CONV_MATH=fp16x2 makes of the file, with LiteInterpreter's default folds
        from cpx import _lib

        base = build_plan(g, fuse_preactivation=True, fold_windows=True, grouped_convolutions=True, **I8)
        h2 = build_plan(g, fuse_preactivation=True, fold_windows=True, conv_math=conv_math, grouped_convolutions=True, **I8)
        n_h2 = sum(o.kind == _lib.GRAPH_CONV_F16X2 for o in h2.ops)
        n_range = sum(o.kind == _lib.GRAPH_RANGE for o in h2.ops)
        n_pre = sum(o.kind == _lib.GRAPH_CONV_PRE for o in base.ops)
        print("conv_math %s: %d convolutions go fp16x2 behind %d RANGE launches; %d pre-activations stay AFFINE launches; "
              "%d launches instead of %d" % (conv_math, n_h2, n_range,
                                            sum(o.kind == _lib.GRAPH_AFFINE for o in h2.ops) - sum(o.kind == _lib.GRAPH_AFFINE for o in base.ops),
                                            len(h2.ops), len(base.ops)))
        if n_pre:
            print("conv_math %s: %d CONV_PRE of the float32 plan run as CONV_F16X2 behind their AFFINE" % (conv_math, n_pre))
    if sidecar is not None and os.path.exists(sidecar):
        name, mode = input_mode_of(sidecar)
        how = {"caffe": "BGR, the ImageNet means subtracted from the unscaled sample by the graph's INPUT operator",
               "torch": "x / 255, ImageNet means and deviations, by the graph's INPUT operator",
               "tf": "x / 127.5 - 1, by the crop kernel", None: "the unscaled sample"}[mode]
        print("input mode: %s (model_name %s: %s)" % (mode or "none", name, how))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("model", help="the .tflite file")
    ap.add_argument("out_base", nargs="?", help="writes <out_base>.npz (and copies the sidecar to <out_base>.json)")
    ap.add_argument("--describe", action="store_true", help="print what the graph executor makes of the file; writes nothing")
    ap.add_argument("--sidecar", default=None, help="the model's JSON sidecar (default: <model>.json next to it)")
    ap.add_argument("--conv-math", default="f32", choices=("f32", "fp16x2"),
                    help="with --describe: also print how many convolutions go fp16x2 and how many RANGE launches that adds")
    ap.add_argument("--dequantise", action="store_true",
                    help="convert a dynamic-range quantised WR-ResNet: the INT8 filters multiplied out by their scales")
    args = ap.parse_args()
    with open(args.model, "rb") as fh:
        g = Graph(fh.read())
    if args.describe:
        return describe(g, args.sidecar or os.path.splitext(args.model)[0] + ".json", conv_math=args.conv_math)
    if args.out_base is None:
        ap.error("out_base is required unless --describe is given")
    weights = convert(g, quantised_math="float" if args.dequantise else None)
    np.savez(args.out_base + ".npz", **weights)
    sidecar = args.sidecar or os.path.splitext(args.model)[0] + ".json"
    if os.path.exists(sidecar):
        shutil.copy(sidecar, args.out_base + ".json")
    else:
        print("no sidecar JSON found (%s): write %s.json with labels / hyperparams yourself" % (sidecar, args.out_base))
    print("wrote %s.npz: %d arrays, output %s" % (args.out_base, len(weights), weights["prediction/activation"]))


if __name__ == "__main__":
    sys.exit(main())
