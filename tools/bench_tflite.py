#!/usr/bin/env python3
"""Times the TFLite graph executor (cpx_graph_forward) on a width-1.0 Inception-v3 at 160 x 160 x 3 (the synthetic
flatbuffer of tests/tflite_build.py: the converter's layout, seeded weights) with HIP events after warm-up, for a few
batch sizes, and -- the yardstick, on the same card in the same run -- PyTorch-ROCm evaluating the same graph in float32
with its reduced-precision convolution paths disabled.  Prints one JSON line.

    python tools/bench_tflite.py [--batches 1,8,32,128] [--steps 10] [--warmup 3]

The per-kernel-kind split of the time comes from the device's own timestamps: run the script (one batch size, --skip-torch)
under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_tflite.py ...`, then hand the trace back:

    python tools/bench_tflite.py --kernel-trace DIR/.../*_kernel_trace.csv --batches 128

which needs no GPU: it maps the last forward's launches, in order, onto the plan's operators and prints the time per kind,
the GPU-busy share of the forward and, for the convolution shape that takes the most time, its algorithmic TFLOP/s and
the share of the float32 matrix-pipe peak (157.3 TFLOP/s) that is.

    python tools/bench_tflite.py --quantised [--batches 32,128]

runs the same Inception-v3 three ways -- the float32 file, its dynamic-range quantised twin (tests/tflite_build_q8.py:
INT8 filters) on the hybrid operators, and the twin with the filters multiplied out (quantised_math="float") -- and prints
ms per forward for each, with the hybrid convolutions' algorithmic TOP/s against the int8 matrix-pipe roof (twice the
BF16 rate: ~5000 TOP/s dense).

    python tools/bench_tflite.py --mobilenet [--quantised] [--batches 1,8,32,128]

times a width-1.0 MobileNetV2 (tests/tflite_build_dw.py) the same way against PyTorch-ROCm float32 and, for the largest
batch, every depthwise launch alone (a one-operator graph of the same shape, HIP events): the bytes it must move -- input
and output once, the weights -- over its time, against the HBM peak (8.0 TB/s; a float4 copy reaches 6.29).  With
--quantised the hybrid twin (INT8 filters) is timed beside it.  --kernel-trace with --mobilenet splits a rocprofv3 trace
of such a run by kind and gives the depthwise launches' bytes per second inside the forward.

    python tools/bench_tflite.py --efficientnet [--batches 1,128]

times an EfficientNet-B0 (tests/tflite_build_se.py; 160 x 160 x 3, the size a frame_size of 32 gives) with the swish and
the sigmoid fused into their producers and with fuse_activations=False (LOGISTIC and MUL as launches), against
PyTorch-ROCm float32 on the same graph.  --kernel-trace with --efficientnet (add --unfused for the other plan) splits a
rocprofv3 trace of such a run by kind and gives, for the MUL, the wide MEAN and the depthwise launches, the bytes they
must move over their time inside the forward against the HBM peak.

    python tools/bench_tflite.py --densenet [--batches 1,8,32,128]

times a DenseNet121 (tests/tflite_build_preact.py; 160 x 160 x 3) with its 61 pre-activations folded into the 1 x 1
convolutions that read them (fuse_preactivation=True: what LiteInterpreter runs) and as AFFINE launches, the same bits,
against PyTorch-ROCm float32 on the same graph.

    python tools/bench_tflite.py --nasnet [--batches 1,8,128]

times a NASNet-layout graph (tests/tflite_build_nas.py, a structural stand-in: 160 x 160 x 3, penultimate 1056 as
NASNetMobile's) with the window folds and the depthwise pre-activation on (fold_windows, fuse_preactivation_dw: what
LiteInterpreter runs) and with every PAD, 1 x 1 pool, STRIDED_SLICE and RELU a launch, the same bits, against PyTorch-ROCm
float32 on the same graph; and, for the largest batch, every SLICE launch of the folded plan alone (a one-operator graph,
HIP events): the bytes it must move -- what it reads of its input and its output once -- over its time, against the HBM
peak and the float4-copy rate.  --mobilenet times the folded plan beside the plain one too; --folded chooses it for a run
under a profiler and for its --kernel-trace (--nasnet: --unfused chooses the other plan).

    python tools/bench_tflite.py --conv-math fp16x2 [--mobilenet | --efficientnet | --densenet] [--batches 1,8,32,128]

times the chosen network (default: the Inception-v3) as LiteInterpreter plans it with conv_math="f32" (the exact float32
convolution: the yardstick) and with conv_math="fp16x2" (two fp16 planes per operand behind one RANGE launch per input
view), both in the same process on the same input, in --rounds alternating rounds: the median over the rounds and their
scatter.  With --skip-torch the fp16x2 plan alone runs (a run under a profiler); --kernel-trace with --conv-math fp16x2
splits such a trace by kind, RANGE and the new kernel included, and gives the fp16x2 convolutions' float32-equivalent
TFLOP/s against the 16 / 3 x 157.3 roof and RANGE's bytes per second against the HBM peak.

    python tools/bench_tflite.py --wrresnet [--batches 1,8,128]

times the WR-ResNet-22-4 (tests/tflite_build.py: wrresnet, every convolution groups = 2; 160 x 160 x 2) four ways on one
card in one process: its dynamic-range quantised file on the graph executor (CONV_Q8_GROUPED: TFLite's hybrid arithmetic,
what get_interpreter runs by default), the float32 file on the graph executor (CONV_GROUPED), the fused kernels in their
default math (WRResNetDevice: what CPX_TFLITE_QUANT_MATH=float and a float32 file run) and PyTorch-ROCm float32
(conv2d(groups=2), reduced-precision paths off).  Prints launches per forward and ms per forward (HIP events, median) for
each; the launches of the last two are counted by torch.profiler over one forward (null where it cannot).

    python tools/bench_tflite.py --int8 [--batches 1,8,128] [--rounds 3]

times the WR-ResNet-22-4 and a width-1.0 MobileNetV2 as full-integer files (tests/tflite_build_i8.py: quantise_full from a
calibration batch; INT8 activations between QUANTIZE and DEQUANTIZE) on the int8 kinds, and beside them, in the same
process on the same card in alternating rounds, the same network's hybrid plan and float32 plan: the median over the
rounds and their scatter, the launches by kind, the arena bytes per sample.  --int8 --skip-torch runs the full-integer
plans alone at the last batch size (a run under `rocprofv3 --kernel-trace --stats`, whose per-kernel times give CONV_I8's
share and the DWCONV_I8 / SLICE bytes per second: the bytes are printed as dwconv_i8_bytes / slice_bytes; --int8-net wr |
mobilenet keeps one network's kernels in the trace).

    python tools/bench_tflite.py --int8 --int8-net efficientnet [--batches 1,8,128] [--rounds 3]

is the same for a width-1.0 EfficientNet-B0 (tests/tflite_build_se.py through quantise_full), with FOUR legs interleaved:
the full-integer plan with its tables (`int8`: integer_gate_mul and integer_lut, every swish and gate sigmoid folded into
its convolution), the full-integer plan with integer_lut=False (`int8_no_lut`: the gate MUL_I8 only, every LOGISTIC as
DEQUANTIZE -> LOGISTIC -> QUANTIZE), the hybrid plan and the float32 plan.  With --skip-torch the tabled plan runs alone,
followed by one forward of a probe graph whose only int8 launch is a LUT_I8 (the EfficientNet's own plan has none: every
table folds) -- under `rocprofv3 --kernel-trace --stats` graph_i8_lut_kernel's time against lut_i8_probe_bytes and
graph_i8_ew_kernel<16, 4>'s against gate_mul_i8_bytes_per_sample x N are the two launches' bytes per second."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "classifier-pipeline_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

KIND_NAMES = {24: "conv_grouped", 25: "conv_q8_grouped", 1: "conv", 2: "max_pool", 3: "avg_pool", 4: "add", 5: "affine", 6: "mean", 7: "fc", 8: "logistic", 9: "softmax",
              10: "pad", 11: "channel_map", 12: "conv_q8", 13: "fc_q8", 14: "quant_params", 15: "dwconv", 16: "dwconv_q8", 17: "mul", 18: "input", 19: "conv_pre",
              20: "slice", 21: "dwconv_pre", 22: "range", 23: "conv_f16x2", 26: "quantize", 27: "dequantize", 28: "conv_i8",
              29: "conv_i8_grouped", 30: "dwconv_i8", 31: "fc_i8", 32: "add_i8", 33: "mul_i8", 34: "max_pool_i8", 35: "avg_pool_i8",
              36: "mean_i8", 37: "lut_i8"}
CONV_KINDS = (1, 12, 19, 23)
DW_KINDS = (15, 16, 21)
FOLDS = dict(fold_windows=True, fuse_preactivation_dw=True, fuse_preactivation=True)
HBM_PEAK_TBS = 8.0          # MI355X HBM3E, specification
HBM_COPY_TBS = 6.29         # what a float4 copy kernel reaches


def torch_model(g, device):
    """The graph as PyTorch modules' functional calls, float32, weights on the device."""
    import torch
    import torch.nn.functional as F

    from tflite_eval import _act, _pads

    const = {i: torch.from_numpy(np.array(t["const"])).to(device) for i, t in enumerate(g.tensors)
             if t["const"] is not None and t["type"] == 0}
    wts = {i: c.permute(0, 3, 1, 2).contiguous() for i, c in const.items() if c.ndim == 4}
    dw_wts = {op["inputs"][1]: const[op["inputs"][1]].permute(3, 0, 1, 2).contiguous() for op in g.ops
              if op["name"] == "DEPTHWISE_CONV_2D"}   # [1, kh, kw, C] -> [C, 1, kh, kw]

    def forward(x_nchw):
        val = {g.inputs[0]: x_nchw}
        for op in g.ops:
            name, ins = op["name"], op["inputs"]
            a = val.get(ins[0])
            if name == "CONV_2D":
                kh, kw = wts[ins[1]].shape[2:]
                pt, pb = _pads(a.shape[2], kh, op["stride_h"], op["padding"])
                pl, pr = _pads(a.shape[3], kw, op["stride_w"], op["padding"])
                if pt or pb or pl or pr:
                    a = F.pad(a, (pl, pr, pt, pb))
                bias = const[ins[2]] if len(ins) > 2 and ins[2] >= 0 else None
                r = _act(F.conv2d(a, wts[ins[1]], bias, stride=(op["stride_h"], op["stride_w"]),
                                  groups=a.shape[1] // wts[ins[1]].shape[1]), op["act"])
            elif name == "DEPTHWISE_CONV_2D":
                w = dw_wts[ins[1]]
                pt, pb = _pads(a.shape[2], w.shape[2], op["stride_h"], op["padding"])
                pl, pr = _pads(a.shape[3], w.shape[3], op["stride_w"], op["padding"])
                if pt or pb or pl or pr:
                    a = F.pad(a, (pl, pr, pt, pb))
                r = _act(F.conv2d(a, w, const[ins[2]], stride=(op["stride_h"], op["stride_w"]), groups=w.shape[0]), op["act"])
            elif name == "PAD":
                (_, _), (t0, t1), (l0, l1), (_, _) = op["paddings"]
                r = F.pad(a, (l0, l1, t0, t1))
            elif name in ("STRIDED_SLICE", "SLICE"):
                from cpx.ml_tools.tflite_reader import resolve_slice

                (_, (y0, sy, ny), (x0, sx, nx), _) = resolve_slice(op, [1, a.shape[2], a.shape[3], a.shape[1]], name)
                r = a[:, :, y0:y0 + sy * (ny - 1) + 1:sy, x0:x0 + sx * (nx - 1) + 1:sx]
            elif name == "RELU":
                r = torch.relu(a)
            elif name in ("ADD", "SUB", "MUL", "DIV"):
                p, q = (val[t] if t in val else const[t].reshape(1, -1, 1, 1) for t in ins[:2])
                r = _act(p + q if name == "ADD" else p - q if name == "SUB" else p * q if name == "MUL" else p / q, op["act"])
            elif name in ("MAX_POOL_2D", "AVERAGE_POOL_2D"):
                k, st = (op["filter_height"], op["filter_width"]), (op["stride_h"], op["stride_w"])
                pt, pb = _pads(a.shape[2], k[0], st[0], op["padding"])
                pl, pr = _pads(a.shape[3], k[1], st[1], op["padding"])
                assert pt == pb and pl == pr and op["act"] == 0, "the yardstick takes symmetric pool padding only"
                if name == "MAX_POOL_2D":
                    r = F.max_pool2d(a, k, st, (pt, pl))
                else:
                    r = F.avg_pool2d(a, k, st, (pt, pl), count_include_pad=False)
            elif name == "CONCATENATION":
                r = torch.cat([val[t] for t in ins], dim=1)
            elif name == "MEAN":
                r = a.mean(dim=(2, 3), keepdim=op["keep_dims"])
            elif name == "FULLY_CONNECTED":
                r = _act(F.linear(a, const[ins[1]], const[ins[2]]), op["act"])
            elif name == "LOGISTIC":
                r = torch.sigmoid(a)
            else:
                raise NotImplementedError(name)
            val[op["outputs"][0]] = r
        return val[g.outputs[0]]

    return forward


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(steps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


F32_MFMA_PEAK_TFLOPS = 157.3
# three fp16 plane products per float32 product on a pipe 16 times as fast as v_mfma_f32_32x32x2_f32
F16X2_ROOF_TFLOPS = F32_MFMA_PEAK_TFLOPS * 16.0 / 3.0
I8_MFMA_PEAK_TOPS = 5000.0   # 2 x the ~2.5 PFLOP/s dense BF16 peak: the i8 forms have twice the K in the same cycles


def count_launches(torch, fn):
    """Kernels one call of fn launches, by torch.profiler's device events; None where the profiler sees none."""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:   # (a profiler that cannot start is no reason to lose the timings)
        return None


def wrresnet_leg(args):
    """The WR-ResNet-22-4 four ways: hybrid and float32 on the graph executor, the fused kernels, PyTorch-ROCm float32."""
    import ctypes as C

    import tflite_build as tb
    import tflite_build_q8 as tq
    import torch
    from cpx import _lib
    from cpx.engine import TrackEngine
    from cpx.ml_tools import wrresnet as wr
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    eng = TrackEngine(model="lepton3", device=0)
    # BatchNorm statistics fitted to the kind of input that is timed: activations of ordinary size, nothing leaves fp16's range
    xcal = torch.from_numpy(np.random.default_rng(1).uniform(0, 255, size=(2, 160, 160, 2)).astype(np.float32)).to(eng.device)
    w = wr.calibrate_bn_device(eng, wr.random_weights(17, seed=3), xcal)
    blob = tb.wrresnet(w)
    g = Graph(blob)
    plans = {"hybrid_graph": build_plan(Graph(tq.quantise(blob)), grouped_convolutions=True, **FOLDS),
             "float32_graph": build_plan(g, grouped_convolutions=True, **FOLDS)}
    stream = torch.cuda.ExternalStream(eng.lib.cpx_stream(eng.h), device=eng.device)
    net = wr.WRResNetDevice(eng, w, 17)
    ref = torch_model(g, eng.device)
    out = {"model": "wr-resnet-22-4 groups 2 160x160x2", "batches": [],
           "launches": {k: len(p.ops) for k, p in plans.items()},
           "launches_by_kind": {k: {KIND_NAMES[kind]: sum(o.kind == kind for o in p.ops) for kind in sorted(set(o.kind for o in p.ops))}
                                for k, p in plans.items()}}
    assert sum(o.kind == _lib.GRAPH_CONV_Q8_GROUPED for o in plans["hybrid_graph"].ops) == 20
    rng = np.random.default_rng(0)
    for n in [int(v) for v in args.batches.split(",")]:
        x = torch.from_numpy(rng.uniform(0, 255, size=(n, 160, 160, 2)).astype(np.float32)).to(eng.device)
        y = torch.empty((n, 17), dtype=torch.float32, device=eng.device)
        logits, probs = torch.empty_like(y), torch.empty_like(y)
        x_nchw = x.permute(0, 3, 1, 2).contiguous()
        rec = {"N": n}
        for name, plan in plans.items():
            dev = GraphDevice(eng, plan)

            def forward():
                rc = eng.lib.cpx_graph_forward(dev._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(y.data_ptr()))
                assert rc == 0, eng._err()

            with torch.cuda.stream(stream):
                rec[name + "_ms"] = timed(torch, forward, args.steps, args.warmup)
            dev.close()
        with torch.cuda.stream(stream):
            rec["fused_ms"] = timed(torch, lambda: net.forward_async(x, logits, probs), args.steps, args.warmup)
            if "fused" not in out["launches"]:
                out["launches"]["fused"] = count_launches(torch, lambda: net.forward_async(x, logits, probs))
        with torch.no_grad():
            rec["torch_ms"] = timed(torch, lambda: ref(x_nchw), args.steps, args.warmup)
            if "torch" not in out["launches"]:
                out["launches"]["torch"] = count_launches(torch, lambda: ref(x_nchw))
        out["batches"].append(rec)
    net.close()
    eng.close()
    print(json.dumps(out))


def int8_leg(args):
    """The WR-ResNet-22-4, a MobileNetV2 and (where it is named) an EfficientNet-B0 as full-integer files against their hybrid
    and float32 plans, interleaved."""
    import ctypes as C

    import tflite_build as tb
    import tflite_build_dw as td
    import tflite_build_i8 as ti
    import tflite_build_q8 as tq
    import tflite_build_se as ts
    import torch
    from cpx import _lib
    from cpx.engine import TrackEngine
    from cpx.ml_tools import wrresnet as wr
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    eng = TrackEngine(model="lepton3", device=0)
    stream = torch.cuda.ExternalStream(eng.lib.cpx_stream(eng.h), device=eng.device)
    rng = np.random.default_rng(0)
    nets = {}
    if args.int8_net in ("all", "wr"):
        xcal = torch.from_numpy(np.random.default_rng(1).uniform(0, 255, size=(2, 160, 160, 2)).astype(np.float32)).to(eng.device)
        w = wr.calibrate_bn_device(eng, wr.random_weights(17, seed=3), xcal)
        nets["wr-resnet-22-4 groups 2 160x160x2"] = (tb.wrresnet(w), tq.quantise, (160, 160, 2), (0.0, 255.0))
    if args.int8_net in ("all", "mobilenet"):
        nets["mobilenet_v2 width 1.00 160x160x3"] = (td.mobilenet_v2(17, width=1.0, seed=7), td.quantise, (160, 160, 3), (-1.0, 1.0))
    if args.int8_net == "efficientnet":   # (the model rescales and normalises its 0 .. 255 input itself)
        nets["efficientnet_b0 width 1.00 160x160x3"] = (ts.efficientnet_b0(17, (), seed=7, width=1.0, size=160), td.quantise,
                                                        (160, 160, 3), (0.0, 255.0))
    out = {"networks": []}
    batches = [int(v) for v in args.batches.split(",")]
    for model, (blob, hybrid_of, shape, (lo, hi)) in nets.items():
        full = ti.quantise_full(blob, np.random.default_rng(2).uniform(lo, hi, size=(1,) + shape))
        opts = dict(grouped_convolutions=True, **FOLDS)
        if model.startswith("efficientnet"):
            plans = {"int8": build_plan(Graph(full), integer_activations=True, integer_gate_mul=True, integer_lut=True, **opts)}
            if not args.skip_torch:
                plans["int8_no_lut"] = build_plan(Graph(full), integer_activations=True, integer_gate_mul=True, **opts)
        else:
            plans = {"int8": build_plan(Graph(full), integer_activations=True, **opts)}
        if not args.skip_torch:
            plans.update(hybrid=build_plan(Graph(hybrid_of(blob)), **opts), float32=build_plan(Graph(blob), **opts))
        p8 = plans["int8"]
        rec = {"model": model, "launches": {k: len(p.ops) for k, p in plans.items()},
               "arena_bytes_per_sample": {k: p.arena_bytes_per_sample for k, p in plans.items()},
               "launches_by_kind": {k: {KIND_NAMES[kind]: sum(o.kind == kind for o in p.ops) for kind in sorted(set(o.kind for o in p.ops))}
                                    for k, p in plans.items()},
               # what the HBM-bound int8 launches must move per sample: input and output once (bytes), the weights apart
               "dwconv_i8_bytes_per_sample": sum(p8.tensors[o.in0].H * p8.tensors[o.in0].W * p8.tensors[o.in0].C +
                                                 p8.tensors[o.out].H * p8.tensors[o.out].W * p8.tensors[o.out].C
                                                 for o in p8.ops if o.kind == _lib.GRAPH_DWCONV_I8),
               "slice_bytes_per_sample": sum(2 * p8.tensors[o.out].H * p8.tensors[o.out].W * p8.tensors[o.out].C
                                             for o in p8.ops if o.kind == _lib.GRAPH_SLICE),
               # (a gate MUL_I8 reads and writes the map once; the gate itself is C bytes)
               "gate_mul_i8_bytes_per_sample": sum(2 * p8.tensors[o.out].H * p8.tensors[o.out].W * p8.tensors[o.out].C + p8.tensors[o.in1].C
                                                   for o in p8.ops if o.kind == _lib.GRAPH_MUL_I8 and o.in1 != -1 and
                                                   p8.tensors[o.in1].H * p8.tensors[o.in1].W == 1 < p8.tensors[o.out].H * p8.tensors[o.out].W),
               "lut_i8_bytes_per_sample": sum(2 * p8.tensors[o.out].H * p8.tensors[o.out].W * p8.tensors[o.out].C
                                              for o in p8.ops if o.kind == _lib.GRAPH_LUT_I8),
               "folded_tables": sum(o.act == _lib.GRAPH_ACT_LUT for o in p8.ops),
               "conv_i8_gop_per_sample": sum(2.0 * p8.tensors[o.out].H * p8.tensors[o.out].W * p8.tensors[o.out].C * o.kh * o.kw *
                                             p8.tensors[o.in0].C / o.groups for o in p8.ops
                                             if o.kind in (_lib.GRAPH_CONV_I8, _lib.GRAPH_CONV_I8_GROUPED)) / 1e9,
               "batches": []}
        for n in (batches[-1:] if args.skip_torch else batches):
            x = torch.from_numpy(rng.uniform(lo, hi, size=(n,) + shape).astype(np.float32)).to(eng.device)
            y = torch.empty((n, 17), dtype=torch.float32, device=eng.device)
            devs = {k: GraphDevice(eng, p) for k, p in plans.items()}
            times = {k: [] for k in plans}
            for _ in range(args.rounds):   # alternating: a drift of the card or the host lands on every plan alike
                for k, dev in devs.items():
                    def forward(dev=dev):
                        rc = eng.lib.cpx_graph_forward(dev._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(y.data_ptr()))
                        assert rc == 0, eng._err()

                    with torch.cuda.stream(stream):
                        times[k].append(timed(torch, forward, args.steps, args.warmup))
            for dev in devs.values():
                dev.close()
            b = {"N": n}
            for k, v in times.items():
                b[k + "_ms"] = float(np.median(v))
                b[k + "_runs_ms"] = [round(t, 4) for t in v]
            if "hybrid_ms" in b:
                b["hybrid_over_int8"], b["float32_over_int8"] = b["hybrid_ms"] / b["int8_ms"], b["float32_ms"] / b["int8_ms"]
            if "int8_no_lut_ms" in b:
                b["no_lut_over_int8"] = b["int8_no_lut_ms"] / b["int8_ms"]
            rec["batches"].append(b)
        if args.skip_torch and model.startswith("efficientnet"):
            rec["lut_i8_probe_bytes"] = lut_i8_probe(eng, stream, batches[-1])
        out["networks"].append(rec)
    eng.close()
    print(json.dumps(out))


def lut_i8_probe(eng, stream, n):
    """One forward of QUANTIZE -> swish -> DEQUANTIZE on [n, 80, 80, 96] (the EfficientNet-B0's widest expanded map): the
    swish has nothing to fold into, so it is ONE LUT_I8 launch, the only graph_i8_lut_kernel of a trace.  -> the bytes that
    launch moves (in and out once)."""
    import ctypes as C

    import tflite_build_i8_se as tis
    import torch
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    shape = (80, 80, 96)
    m, q = tis.start([1] + list(shape), (np.float32(0.05), 7))
    plan = build_plan(Graph(tis.finish(m, m.swish_i8(q, (np.float32(0.026), -117)))), integer_activations=True, integer_lut=True)
    assert [KIND_NAMES[o.kind] for o in plan.ops] == ["quantize", "lut_i8", "dequantize"]
    x = torch.from_numpy(np.random.default_rng(3).uniform(-6, 6, size=(n,) + shape).astype(np.float32)).to(eng.device)
    y = torch.empty((n,) + shape, dtype=torch.float32, device=eng.device)
    dev = GraphDevice(eng, plan)
    with torch.cuda.stream(stream):
        for _ in range(3):
            rc = eng.lib.cpx_graph_forward(dev._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(y.data_ptr()))
            assert rc == 0, eng._err()
    torch.cuda.synchronize()
    dev.close()
    return 2 * n * int(np.prod(shape))


def quantised_leg(args):
    """float32 / hybrid / float-math forwards of one Inception-v3, ms per forward by batch size."""
    import ctypes as C

    import tflite_build as tb
    import tflite_build_q8 as tq
    import torch
    from cpx import _lib
    from cpx.engine import TrackEngine
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    blob = tb.inception_v3(17, (), seed=7, width=args.width)
    gq = Graph(tq.quantise(blob))
    plans = {"float32": build_plan(Graph(blob)), "hybrid": build_plan(gq), "quantised_float_math": build_plan(gq, quantised_math="float")}
    ops8 = 0.0   # algorithmic int8 multiply-adds x 2 of the hybrid convolutions, per sample
    for o in plans["hybrid"].ops:
        if o.kind == _lib.GRAPH_CONV_Q8:
            t, i = plans["hybrid"].tensors[o.out], plans["hybrid"].tensors[o.in0]
            ops8 += 2.0 * t.H * t.W * t.C * o.kh * o.kw * i.C
    eng = TrackEngine(model="lepton3", device=0)
    stream = torch.cuda.ExternalStream(eng.lib.cpx_stream(eng.h), device=eng.device)
    out = {"model": "inception_v3 width %.2f 160x160x3" % args.width, "hybrid_conv_gop_per_sample": ops8 / 1e9,
           "hybrid_operators": sum(o.kind in (_lib.GRAPH_CONV_Q8, _lib.GRAPH_FC_Q8) for o in plans["hybrid"].ops),
           "quant_params_launches": sum(o.kind == _lib.GRAPH_QUANT_PARAMS for o in plans["hybrid"].ops), "batches": []}
    rng = np.random.default_rng(0)
    for n in [int(v) for v in args.batches.split(",")]:
        x = torch.from_numpy(rng.uniform(-1, 1, size=(n, 160, 160, 3)).astype(np.float32)).to(eng.device)
        y = torch.empty((n, 17), dtype=torch.float32, device=eng.device)
        rec = {"N": n}
        for name, plan in plans.items():
            dev = GraphDevice(eng, plan)

            def forward():
                rc = eng.lib.cpx_graph_forward(dev._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(y.data_ptr()))
                assert rc == 0, eng._err()

            with torch.cuda.stream(stream):
                rec[name + "_ms"] = timed(torch, forward, args.steps, args.warmup)
            dev.close()
        rec["hybrid_over_float32"] = rec["float32_ms"] / rec["hybrid_ms"]
        # the whole forward's time against the hybrid convolutions' work: a lower bound of what they reach while running
        rec["hybrid_tops_over_whole_forward"] = ops8 * n / rec["hybrid_ms"] / 1e9
        rec["i8_roof_share"] = rec["hybrid_tops_over_whole_forward"] / I8_MFMA_PEAK_TOPS
        out["batches"].append(rec)
    eng.close()
    print(json.dumps(out))


def dw_bytes(plan, o, n):
    """What a depthwise launch must move for n samples: its input and its output once, its weights."""
    t, i = plan.tensors[o.out], plan.tensors[o.in0]
    return 4.0 * n * (i.H * i.W * i.C + t.H * t.W * t.C) + o.weights.nbytes


def dw_shape(plan, o):
    t, i = plan.tensors[o.out], plan.tensors[o.in0]
    return "%dx%d s%d C%d %dx%d->%dx%d%s" % (o.kh, o.kw, o.stride_h, t.C, i.H, i.W, t.H, t.W, " q8" if o.kind == 16 else "")


def mobilenet_leg(args):
    """ms per forward of a MobileNetV2 by batch size against PyTorch-ROCm float32; the depthwise launches alone."""
    import ctypes as C

    import tflite_build as tb
    import tflite_build_dw as td
    import torch
    from cpx.engine import TrackEngine
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    blob = td.mobilenet_v2(17, (), seed=7, width=args.width)
    g = Graph(blob)
    plans = {"float32": build_plan(g), "folded": build_plan(g, **FOLDS)}
    if args.quantised:
        plans["hybrid"] = build_plan(Graph(td.quantise(blob)))
        plans["hybrid_folded"] = build_plan(Graph(td.quantise(blob)), **FOLDS)
    if args.folded and args.skip_torch:
        plans = {"folded": plans["folded"]}   # (a run under a profiler ends with forwards of ONE plan)
    batches = [int(v) for v in args.batches.split(",")]
    if args.kernel_trace:
        name = "folded" if args.folded else "hybrid" if args.quantised else "float32"
        print(json.dumps(dict(split_from_trace(args.kernel_trace, plans[name], batches[-1]), plan=name)))
        return
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    eng = TrackEngine(model="lepton3", device=0)
    stream = torch.cuda.ExternalStream(eng.lib.cpx_stream(eng.h), device=eng.device)
    ref = torch_model(g, eng.device)
    first = next(iter(plans))
    out = {"model": "mobilenet_v2 width %.2f 160x160x3" % args.width, "arena_bytes_per_sample": plans[first].arena_bytes_per_sample,
           "launches": {k: len(v.ops) for k, v in plans.items()}, "launches_by_kind": {}, "batches": []}
    for o in plans[first].ops:
        out["launches_by_kind"][KIND_NAMES[o.kind]] = out["launches_by_kind"].get(KIND_NAMES[o.kind], 0) + 1
    rng = np.random.default_rng(0)

    def forward_of(dev, x, y, n):
        def forward():
            rc = eng.lib.cpx_graph_forward(dev._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(y.data_ptr()))
            assert rc == 0, eng._err()
        return forward

    for n in batches:
        x = torch.from_numpy(rng.uniform(-1, 1, size=(n, 160, 160, 3)).astype(np.float32)).to(eng.device)
        y = torch.empty((n, 17), dtype=torch.float32, device=eng.device)
        rec = {"N": n}
        for name, plan in plans.items():
            dev = GraphDevice(eng, plan)
            with torch.cuda.stream(stream):
                rec[name + "_ms"] = timed(torch, forward_of(dev, x, y, n), args.steps, args.warmup)
            if name == "float32" and not args.skip_torch:
                x_nchw = x.permute(0, 3, 1, 2).contiguous()
                with torch.no_grad():
                    rec["torch_ms"] = timed(torch, lambda: ref(x_nchw), args.steps, args.warmup)
                    forward_of(dev, x, y, n)()
                    torch.cuda.synchronize()
                    rec["max_abs_diff_vs_torch"] = float((ref(x_nchw) - y).abs().max())
                rec["ratio_vs_torch"] = rec["torch_ms"] / rec["float32_ms"]
            dev.close()
        out["batches"].append(rec)
    # every depthwise launch of the largest batch alone: a one-operator graph of its shape
    n = batches[-1]
    for name, plan in ({} if args.skip_alone else plans).items():
        if "folded" in name:
            continue   # (the same depthwise shapes with explicit pads)
        rows, total_b, total_ms = [], 0.0, 0.0
        for o in plan.ops:
            if o.kind not in DW_KINDS:
                continue
            i = plan.tensors[o.in0]
            m = td.ModelDW()
            xin = m.tensor([1, i.H, i.W, i.C], name="input")
            m.inputs = [xin]
            pad = tb.VALID if o.pads == (0, 0, 0, 0) else tb.SAME
            m.outputs = [m.depthwise(xin, rng.normal(0, 0.5, size=(1, o.kh, o.kw, i.C)).astype(np.float32),
                                     np.zeros(i.C, np.float32), (o.stride_h, o.stride_w), pad, o.act)]
            one = build_plan(Graph(td.quantise(m.finish(), min_elements=0) if o.kind == 16 else m.finish()))
            k = [p for p in one.ops if p.kind in DW_KINDS][0]
            assert (k.kind, k.pads, one.output_shape) == (o.kind, o.pads, (plan.tensors[o.out].H, plan.tensors[o.out].W, i.C))
            # (the hybrid one-operator graph also launches its QUANT_PARAMS, which reads the input once more: launches_timed = 2)
            x = torch.from_numpy(rng.uniform(-1, 1, size=(n, i.H, i.W, i.C)).astype(np.float32)).to(eng.device)
            y = torch.empty((n,) + one.output_shape, dtype=torch.float32, device=eng.device)
            dev = GraphDevice(eng, one)
            with torch.cuda.stream(stream):
                ms = timed(torch, forward_of(dev, x, y, n), args.steps, args.warmup)
            dev.close()
            b = dw_bytes(one, k, n)
            rows.append({"shape": dw_shape(one, k), "ms": ms, "mbytes": b / 1e6, "tb_per_s": b / ms / 1e9,
                         "launches_timed": len(one.ops)})
            total_b += b
            total_ms += ms
        out["depthwise_alone_" + name] = {"N": n, "launches": rows, "ms_sum": total_ms, "tb_per_s": total_b / total_ms / 1e9,
                                          "share_of_hbm_peak": total_b / total_ms / 1e9 / HBM_PEAK_TBS,
                                          "share_of_copy_rate": total_b / total_ms / 1e9 / HBM_COPY_TBS}
    eng.close()
    print(json.dumps(out))


def efficientnet_leg(args):
    """ms per forward of an EfficientNet-B0, fused and unfused, by batch size, against PyTorch-ROCm float32."""
    import ctypes as C

    import tflite_build_se as ts
    import torch
    from cpx.engine import TrackEngine
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    size = 160
    g = Graph(ts.efficientnet_b0(17, (), seed=7, width=args.width, size=size))
    plans = {"fused": build_plan(g), "unfused": build_plan(g, fuse_activations=False)}
    batches = [int(v) for v in args.batches.split(",")]
    if args.kernel_trace:
        name = "unfused" if args.unfused else "fused"
        print(json.dumps(dict(split_from_trace(args.kernel_trace, plans[name], batches[-1]), plan=name)))
        return
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    eng = TrackEngine(model="lepton3", device=0)
    stream = torch.cuda.ExternalStream(eng.lib.cpx_stream(eng.h), device=eng.device)
    ref = torch_model(g, eng.device)
    out = {"model": "efficientnet_b0 width %.2f %dx%dx3" % (args.width, size, size), "batches": []}
    for name, plan in plans.items():
        kinds = {}
        for o in plan.ops:
            kinds[KIND_NAMES[o.kind]] = kinds.get(KIND_NAMES[o.kind], 0) + 1
        out[name] = {"launches": len(plan.ops), "launches_by_kind": kinds, "arena_bytes_per_sample": plan.arena_bytes_per_sample}
    rng = np.random.default_rng(0)
    for n in batches:
        x = torch.from_numpy(rng.uniform(0, 255, size=(n, size, size, 3)).astype(np.float32)).to(eng.device)
        rec, ys = {"N": n}, {}
        for name, plan in plans.items():
            if args.unfused and name == "fused" or args.skip_torch and not args.unfused and name == "unfused":
                continue   # (a run under a profiler ends with forwards of ONE plan)
            dev = GraphDevice(eng, plan)
            y = ys[name] = torch.empty((n, 17), dtype=torch.float32, device=eng.device)

            def forward():
                rc = eng.lib.cpx_graph_forward(dev._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(y.data_ptr()))
                assert rc == 0, eng._err()

            with torch.cuda.stream(stream):
                rec[name + "_ms"] = timed(torch, forward, args.steps, args.warmup)
            dev.close()
        if len(ys) == 2:
            rec["fused_equals_unfused"] = bool(torch.equal(ys["fused"], ys["unfused"]))
            rec["unfused_over_fused"] = rec["unfused_ms"] / rec["fused_ms"]
        if not args.skip_torch:
            x_nchw = x.permute(0, 3, 1, 2).contiguous()
            with torch.no_grad():
                rec["torch_ms"] = timed(torch, lambda: ref(x_nchw), args.steps, args.warmup)
                rec["max_abs_diff_vs_torch"] = float((ref(x_nchw) - next(iter(ys.values()))).abs().max())
            for name in ys:
                rec["ratio_vs_torch_" + name] = rec["torch_ms"] / rec[name + "_ms"]
        out["batches"].append(rec)
    eng.close()
    print(json.dumps(out))


def densenet_leg(args):
    """ms per forward of a DenseNet121, pre-activations folded and as launches, by batch size, against PyTorch-ROCm float32."""
    import ctypes as C

    import tflite_build_preact as tp
    import torch
    from cpx.engine import TrackEngine
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    size = 160
    g = Graph(tp.densenet121(17, size=size, seed=7))
    plans = {"fused": build_plan(g, fuse_preactivation=True), "unfused": build_plan(g)}
    batches = [int(v) for v in args.batches.split(",")]
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    eng = TrackEngine(model="lepton3", device=0)
    stream = torch.cuda.ExternalStream(eng.lib.cpx_stream(eng.h), device=eng.device)
    ref = torch_model(g, eng.device)
    out = {"model": "densenet121 %dx%dx3" % (size, size), "batches": []}
    for name, plan in plans.items():
        kinds = {}
        for o in plan.ops:
            kinds[KIND_NAMES[o.kind]] = kinds.get(KIND_NAMES[o.kind], 0) + 1
        out[name] = {"launches": len(plan.ops), "launches_by_kind": kinds, "arena_bytes_per_sample": plan.arena_bytes_per_sample}
    rng = np.random.default_rng(0)
    for n in batches:
        # (the sample as the 'torch' input mode leaves it: a few units either side of 0)
        x = torch.from_numpy(rng.uniform(-2.2, 2.6, size=(n, size, size, 3)).astype(np.float32)).to(eng.device)
        rec, ys = {"N": n}, {}
        for name, plan in plans.items():
            dev = GraphDevice(eng, plan)
            y = ys[name] = torch.empty((n, 17), dtype=torch.float32, device=eng.device)

            def forward():
                rc = eng.lib.cpx_graph_forward(dev._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(y.data_ptr()))
                assert rc == 0, eng._err()

            with torch.cuda.stream(stream):
                rec[name + "_ms"] = timed(torch, forward, args.steps, args.warmup)
            dev.close()
        rec["fused_equals_unfused"] = bool(torch.equal(ys["fused"], ys["unfused"]))
        rec["unfused_over_fused"] = rec["unfused_ms"] / rec["fused_ms"]
        if not args.skip_torch:
            x_nchw = x.permute(0, 3, 1, 2).contiguous()
            with torch.no_grad():
                rec["torch_ms"] = timed(torch, lambda: ref(x_nchw), args.steps, args.warmup)
                rec["max_abs_diff_vs_torch"] = float((ref(x_nchw) - ys["fused"]).abs().max())
            for name in ys:
                rec["ratio_vs_torch_" + name] = rec["torch_ms"] / rec[name + "_ms"]
        out["batches"].append(rec)
    eng.close()
    print(json.dumps(out))


def slice_bytes(plan, o, n):
    """What a SLICE launch must move for n samples: the input elements it reads (one per output element that lies inside
    the input) and its output once."""
    t, i = plan.tensors[o.out], plan.tensors[o.in0]
    rows = sum(0 <= y * o.stride_h - o.pads[0] < i.H for y in range(t.H))
    cols = sum(0 <= x * o.stride_w - o.pads[1] < i.W for x in range(t.W))
    return 4.0 * n * t.C * (rows * cols + t.H * t.W)


def nasnet_leg(args):
    """ms per forward of a NASNet-layout graph, folds on and off, by batch size, against PyTorch-ROCm float32; the SLICE
    launches alone."""
    import ctypes as C

    import tflite_build_nas as tn
    import torch
    from cpx import _lib
    from cpx.engine import TrackEngine
    from cpx.ml_tools.tflite_graph import GraphDevice, PlanOp, Plan, PlanTensor, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    size = 160
    g = Graph(tn.nasnet(17, size=size, penultimate=int(1056 * args.width) // 24 * 24, num_blocks=args.nasnet_blocks,
                        stem_filters=32, seed=7))
    # windows_only: fold_windows alone; conv_pre_only: fuse_preactivation alone (RELU into the 1 x 1 convolutions, no fold)
    plans = {"folded": build_plan(g, **FOLDS), "unfolded": build_plan(g), "windows_only": build_plan(g, fold_windows=True),
             "conv_pre_only": build_plan(g, fuse_preactivation=True)}
    batches = [int(v) for v in args.batches.split(",")]
    if args.kernel_trace:
        name = "unfolded" if args.unfused else "folded"
        print(json.dumps(dict(split_from_trace(args.kernel_trace, plans[name], batches[-1]), plan=name)))
        return
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    eng = TrackEngine(model="lepton3", device=0)
    stream = torch.cuda.ExternalStream(eng.lib.cpx_stream(eng.h), device=eng.device)
    ref = torch_model(g, eng.device)
    out = {"model": "nasnet stand-in, %d blocks, penultimate %d, %dx%dx3" % (args.nasnet_blocks, int(1056 * args.width) // 24 * 24, size, size),
           "batches": []}
    for name, plan in plans.items():
        kinds = {}
        for o in plan.ops:
            kinds[KIND_NAMES[o.kind]] = kinds.get(KIND_NAMES[o.kind], 0) + 1
        out[name] = {"launches": len(plan.ops), "launches_by_kind": kinds, "arena_bytes_per_sample": plan.arena_bytes_per_sample}
    rng = np.random.default_rng(0)

    def forward_of(dev, x, y, n):
        def forward():
            rc = eng.lib.cpx_graph_forward(dev._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(y.data_ptr()))
            assert rc == 0, eng._err()
        return forward

    for n in batches:
        x = torch.from_numpy(rng.uniform(-1, 1, size=(n, size, size, 3)).astype(np.float32)).to(eng.device)
        rec, ys = {"N": n}, {}
        for name, plan in plans.items():
            if args.skip_torch and name != ("unfolded" if args.unfused else "folded"):
                continue   # (a run under a profiler ends with forwards of ONE plan)
            dev = GraphDevice(eng, plan)
            y = ys[name] = torch.empty((n, 17), dtype=torch.float32, device=eng.device)
            with torch.cuda.stream(stream):
                rec[name + "_ms"] = timed(torch, forward_of(dev, x, y, n), args.steps, args.warmup)
            dev.close()
        if len(ys) > 1:
            rec["folded_equals_unfolded"] = all(bool(torch.equal(ys["folded"], v)) for v in ys.values())
            rec["unfolded_over_folded"] = rec["unfolded_ms"] / rec["folded_ms"]
        if not args.skip_torch:
            x_nchw = x.permute(0, 3, 1, 2).contiguous()
            with torch.no_grad():
                rec["torch_ms"] = timed(torch, lambda: ref(x_nchw), args.steps, args.warmup)
                rec["max_abs_diff_vs_torch"] = float((ref(x_nchw) - next(iter(ys.values()))).abs().max())
            for name in ("folded", "unfolded"):
                rec["ratio_vs_torch_" + name] = rec["torch_ms"] / rec[name + "_ms"]
        out["batches"].append(rec)
    # every SLICE launch of the folded plan alone, at the largest batch: a one-operator plan of its shape
    n = batches[-1]
    rows, total_b, total_ms = [], 0.0, 0.0
    seen = set()
    for o in ([] if args.skip_alone else plans["folded"].ops):
        i, t = plans["folded"].tensors[o.in0], plans["folded"].tensors[o.out]
        key = (o.kind, i.H, i.W, i.C, o.pads, o.stride_h, o.act)
        if o.kind != _lib.GRAPH_SLICE or key in seen:
            continue
        seen.add(key)
        one = Plan()
        one.tensors = {0: PlanTensor(0, i.H, i.W, i.C), 1: PlanTensor(1, t.H, t.W, t.C)}
        for v in one.tensors.values():
            v.arena_offset, v.storage = 0, v.id
        one.ops = [PlanOp(_lib.GRAPH_SLICE, o.name, 0, 1, stride_h=o.stride_h, stride_w=o.stride_w, pads=o.pads, act=o.act, param=o.param)]
        one.input, one.output, one.input_shape, one.output_shape = 0, 1, (i.H, i.W, i.C), (t.H, t.W, t.C)
        x = torch.from_numpy(rng.uniform(-1, 1, size=(n, i.H, i.W, i.C)).astype(np.float32)).to(eng.device)
        y = torch.empty((n, t.H, t.W, t.C), dtype=torch.float32, device=eng.device)
        dev = GraphDevice(eng, one)
        with torch.cuda.stream(stream):
            ms = timed(torch, forward_of(dev, x, y, n), args.steps, args.warmup)
        dev.close()
        b = slice_bytes(one, one.ops[0], n)
        rows.append({"shape": "%s %dx%dx%d -> %dx%d pads %s stride %d" % (o.name, i.H, i.W, i.C, t.H, t.W, list(o.pads), o.stride_h),
                     "ms": ms, "mbytes": b / 1e6, "tb_per_s": b / ms / 1e9})
        total_b += b
        total_ms += ms
    if rows:
        out["slice_alone"] = {"N": n, "launches": rows, "ms_sum": total_ms, "tb_per_s": total_b / total_ms / 1e9,
                              "share_of_hbm_peak": total_b / total_ms / 1e9 / HBM_PEAK_TBS,
                              "share_of_copy_rate": total_b / total_ms / 1e9 / HBM_COPY_TBS}
    eng.close()
    print(json.dumps(out))


def hbm_group(plan, o, n):
    """-> (group, bytes the launch must move for n samples) of the HBM-bound kinds beside the depthwise ones: MUL (in0 and the
    output once, in1 once: C floats per sample where it is the gate) and the wide MEAN (its input once)."""
    from cpx import _lib

    t, i = plan.tensors[o.out], plan.tensors[o.in0]
    if o.kind == _lib.GRAPH_MUL:
        b = plan.tensors[o.in1]
        return "mul", 4.0 * n * (2 * t.H * t.W * t.C + b.H * b.W * b.C)
    if o.kind == _lib.GRAPH_SLICE:
        return "slice", slice_bytes(plan, o, n)
    if o.kind == _lib.GRAPH_MEAN and i.H * i.W >= _lib.GRAPH_MEAN_WIDE_PIXELS:
        return "mean_wide", 4.0 * n * (i.H * i.W * i.C + i.C)
    return None, 0.0


def split_from_trace(path, plan, n):
    """The last forward of a rocprofv3 kernel trace: its launches are the plan's operators in order."""
    import csv

    with open(path) as fh:
        rows = [r for r in csv.DictReader(fh) if "graph_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[-len(plan.ops):]
    assert len(rows) == len(plan.ops), "the trace holds no whole forward"
    by_kind, shapes, dws, hbm = {}, {}, {}, {}
    for r, o in zip(rows, plan.ops):
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        assert ("conv" in r["Kernel_Name"]) == (o.kind in CONV_KINDS) and ("graph_dw" in r["Kernel_Name"]) == (o.kind in DW_KINDS), \
            (r["Kernel_Name"], o.name)
        k = by_kind.setdefault(KIND_NAMES[o.kind], {"launches": 0, "ms": 0.0})
        k["launches"] += 1
        k["ms"] += ns / 1e6
        grp, nbytes = hbm_group(plan, o, n)
        if grp:
            h = hbm.setdefault(grp, {"launches": 0, "ms": 0.0, "mbytes": 0.0})
            h["launches"] += 1
            h["ms"] += ns / 1e6
            h["mbytes"] += nbytes / 1e6
        if o.kind in DW_KINDS:
            d = dws.setdefault(dw_shape(plan, o), {"launches": 0, "ms": 0.0, "mbytes": 0.0})
            d["launches"] += 1
            d["ms"] += ns / 1e6
            d["mbytes"] += dw_bytes(plan, o, n) / 1e6
        if o.kind == 22:   # RANGE reads its view once
            i = plan.tensors[o.in0]
            h = hbm.setdefault("range", {"launches": 0, "ms": 0.0, "mbytes": 0.0})
            h["launches"] += 1
            h["ms"] += ns / 1e6
            h["mbytes"] += 4.0 * n * i.H * i.W * i.C / 1e6
        if o.kind in CONV_KINDS:
            t, i = plan.tensors[o.out], plan.tensors[o.in0]
            key = "%dx%d s%d %d->%d at %dx%d" % (o.kh, o.kw, o.stride_h, i.C, t.C, t.H, t.W)
            s = shapes.setdefault(key, {"launches": 0, "ms": 0.0, "gflop": 0.0})
            s["launches"] += 1
            s["ms"] += ns / 1e6
            s["gflop"] += 2.0 * n * t.H * t.W * t.C * o.kh * o.kw * i.C / 1e9
    wall = (int(rows[-1]["End_Timestamp"]) - int(rows[0]["Start_Timestamp"])) / 1e6
    busy = sum(k["ms"] for k in by_kind.values())
    top = max(shapes, key=lambda k: shapes[k]["ms"])
    conv = {"ms": sum(by_kind[k]["ms"] for k in ("conv", "conv_q8", "conv_pre", "conv_f16x2") if k in by_kind)}
    conv_gflop = sum(s["gflop"] for s in shapes.values())
    tf = shapes[top]["gflop"] / shapes[top]["ms"]
    dw = {}
    if dws:
        for d in dws.values():
            d["tb_per_s"] = d["mbytes"] / d["ms"] / 1e3
        dw_mb, dw_ms = sum(d["mbytes"] for d in dws.values()), sum(d["ms"] for d in dws.values())
        dw = {"depthwise": {"launches": dws, "ms": dw_ms, "tb_per_s": dw_mb / dw_ms / 1e3,
                            "share_of_hbm_peak": dw_mb / dw_ms / 1e3 / HBM_PEAK_TBS, "share_of_copy_rate": dw_mb / dw_ms / 1e3 / HBM_COPY_TBS}}
    for h in hbm.values():
        h["tb_per_s"] = h["mbytes"] / h["ms"] / 1e3
        h["share_of_hbm_peak"] = h["tb_per_s"] / HBM_PEAK_TBS
    if hbm:
        dw["hbm_bound"] = hbm
    return {**dw, "N": n, "forward_ms_first_start_to_last_end": wall, "kernel_ms_sum": busy, "gpu_busy_share": busy / wall,
            "ms_by_kind": by_kind, "conv_tflops_while_running": conv_gflop / conv["ms"],
            "conv_matrix_pipe_share": conv_gflop / conv["ms"] / F32_MFMA_PEAK_TFLOPS,
            "dominant_conv": dict(shapes[top], shape=top, tflops=tf, matrix_pipe_share=tf / F32_MFMA_PEAK_TFLOPS),
            **({"conv_f16x2_roof_tflops": F16X2_ROOF_TFLOPS, "conv_share_of_f16x2_roof": conv_gflop / conv["ms"] / F16X2_ROOF_TFLOPS}
               if "conv_f16x2" in by_kind else {})}


def conv_math_leg(args):
    """The chosen network as LiteInterpreter plans it, conv_math f32 and fp16x2, same process, same input, alternating rounds."""
    import ctypes as C

    import torch
    from cpx import _lib
    from cpx.engine import TrackEngine
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    if args.mobilenet:
        import tflite_build_dw as td
        name, blob = "mobilenet_v2", td.mobilenet_v2(17, (), seed=7, width=args.width)
    elif args.efficientnet:
        import tflite_build_se as ts
        name, blob = "efficientnet_b0", ts.efficientnet_b0(17, (), seed=7, width=args.width, size=160)
    elif args.densenet:
        import tflite_build_preact as tp
        name, blob = "densenet121", tp.densenet121(17, size=160, seed=7)
    else:
        import tflite_build as tb
        name, blob = "inception_v3", tb.inception_v3(17, (), seed=7, width=args.width)
    g = Graph(blob)
    folds = dict(fuse_preactivation=True, fold_windows=True)   # LiteInterpreter's defaults
    plans = {m: build_plan(g, conv_math=m, **folds) for m in ("f32", "fp16x2")}
    batches = [int(v) for v in args.batches.split(",")]
    if args.kernel_trace:
        print(json.dumps(dict(split_from_trace(args.kernel_trace, plans["fp16x2"], batches[-1]), plan="fp16x2", model=name)))
        return
    census = {m: {KIND_NAMES[k]: sum(o.kind == k for o in p.ops) for k in sorted(set(o.kind for o in p.ops))} for m, p in plans.items()}
    flops = sum(2.0 * plans["f32"].tensors[o.out].H * plans["f32"].tensors[o.out].W * plans["f32"].tensors[o.out].C * o.kh * o.kw
                * plans["f32"].tensors[o.in0].C for o in plans["f32"].ops if o.kind in (_lib.GRAPH_CONV, _lib.GRAPH_CONV_PRE))
    eng = TrackEngine(model="lepton3", device=0)
    stream = torch.cuda.ExternalStream(eng.lib.cpx_stream(eng.h), device=eng.device)
    maths = ("fp16x2",) if args.skip_torch else ("f32", "fp16x2")
    devs = {m: GraphDevice(eng, plans[m]) for m in maths}
    out = {"model": "%s 160x160x3" % name, "conv_gflop_per_sample": flops / 1e9, "launches_by_kind": census, "rounds": args.rounds,
           "batches": []}
    rng = np.random.default_rng(0)
    for n in batches:
        x = torch.from_numpy(rng.uniform(-1, 1, size=(n, 160, 160, 3)).astype(np.float32)).to(eng.device)
        ys = {m: torch.empty((n, 17), dtype=torch.float32, device=eng.device) for m in maths}
        torch.cuda.synchronize()
        ms = {m: [] for m in maths}
        for _ in range(args.rounds):
            for m in maths:
                def fwd(m=m):
                    rc = eng.lib.cpx_graph_forward(devs[m]._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(ys[m].data_ptr()))
                    assert rc == 0, eng._err()

                with torch.cuda.stream(stream):
                    ms[m].append(timed(torch, fwd, args.steps, args.warmup))
        rec = {"N": n}
        for m in maths:
            rec[m] = {"ms": float(np.median(ms[m])), "ms_min": min(ms[m]), "ms_max": max(ms[m]),
                      "conv_tflops_if_all_time_were_conv": flops * n / float(np.median(ms[m])) / 1e9}
        if len(maths) == 2:
            rec["speedup"] = rec["f32"]["ms"] / rec["fp16x2"]["ms"]
            rec["max_abs_diff"] = float((ys["f32"] - ys["fp16x2"]).abs().max())
        out["batches"].append(rec)
    for d in devs.values():
        d.close()
    eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", default="1,8,32,128")
    ap.add_argument("--skip-torch", action="store_true", help="time the executor only (for a run under a profiler)")
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 kernel trace CSV of a run of this script: print the split")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=float, default=1.0)
    ap.add_argument("--quantised", action="store_true",
                    help="time the float32 file, its dynamic-range quantised twin (hybrid operators) and the twin in float math")
    ap.add_argument("--mobilenet", action="store_true",
                    help="time a MobileNetV2 (DEPTHWISE_CONV_2D) instead of the Inception-v3, and its depthwise launches alone")
    ap.add_argument("--skip-alone", action="store_true",
                    help="with --mobilenet: do not time the depthwise launches alone (for a run under a profiler: the trace ends with a forward)")
    ap.add_argument("--efficientnet", action="store_true",
                    help="time an EfficientNet-B0 (swish, squeeze-and-excite) with its activations fused and unfused")
    ap.add_argument("--unfused", action="store_true",
                    help="with --efficientnet: the fuse_activations=False plan alone (a run under a profiler, and its --kernel-trace)")
    ap.add_argument("--densenet", action="store_true",
                    help="a DenseNet121 with the pre-activations folded into their convolutions and as launches, against PyTorch-ROCm")
    ap.add_argument("--nasnet", action="store_true",
                    help="a NASNet-layout graph with the window folds and the depthwise pre-activation on and off, against PyTorch-ROCm")
    ap.add_argument("--nasnet-blocks", type=int, default=2, help="with --nasnet: normal cells per stage (NASNetMobile: 4, NASNetLarge: 6)")
    ap.add_argument("--folded", action="store_true",
                    help="with --mobilenet: the fold_windows plan alone (a run under a profiler, and its --kernel-trace)")
    ap.add_argument("--conv-math", default="f32", choices=("f32", "fp16x2"),
                    help="fp16x2: time the network (default Inception-v3; --mobilenet, --efficientnet, --densenet) with both "
                         "convolution maths in the same process; with --kernel-trace: split a trace of the fp16x2 plan")
    ap.add_argument("--wrresnet", action="store_true",
                    help="the WR-ResNet-22-4 (grouped convolutions): hybrid and float32 on the graph executor, the fused kernels, PyTorch-ROCm")
    ap.add_argument("--rounds", type=int, default=3, help="with --conv-math fp16x2: alternating rounds per batch size (median, scatter)")
    ap.add_argument("--int8", action="store_true",
                    help="the WR-ResNet-22-4 and a MobileNetV2 as full-integer files beside their hybrid and float32 plans, interleaved")
    ap.add_argument("--int8-net", default="all", choices=("all", "wr", "mobilenet", "efficientnet"),
                    help="with --int8: one network alone (a run under a profiler: the kernels of one network in the trace).  all: the "
                         "WR-ResNet and the MobileNetV2; efficientnet: an EfficientNet-B0, with and without its tables, when named")
    args = ap.parse_args()
    if args.int8:
        if args.batches == "1,8,32,128":
            args.batches = "1,8,128"
        return int8_leg(args)
    if args.wrresnet:
        if args.batches == "1,8,32,128":
            args.batches = "1,8,128"
        return wrresnet_leg(args)
    if args.conv_math == "fp16x2":
        if (args.mobilenet or args.efficientnet or args.densenet) and args.batches == "1,8,32,128":
            args.batches = "1,128"
        return conv_math_leg(args)
    if args.nasnet:
        if args.batches == "1,8,32,128":
            args.batches = "1,8,128"
        return nasnet_leg(args)
    if args.densenet:
        return densenet_leg(args)
    if args.efficientnet:
        if args.batches == "1,8,32,128":
            args.batches = "1,128"
        return efficientnet_leg(args)
    if args.mobilenet:
        return mobilenet_leg(args)
    if args.quantised:
        return quantised_leg(args)
    import ctypes as C

    import tflite_build as tb
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph
    g = Graph(tb.inception_v3(17, (), seed=7, width=args.width))
    plan = build_plan(g)
    if args.kernel_trace:
        print(json.dumps(split_from_trace(args.kernel_trace, plan, int(args.batches.split(",")[-1]))))
        return
    flops = 0.0   # algorithmic, per sample
    for o in plan.ops:
        if o.kind == 1:
            t, i = plan.tensors[o.out], plan.tensors[o.in0]
            flops += 2.0 * t.H * t.W * t.C * o.kh * o.kw * i.C
    import torch

    from cpx.engine import TrackEngine

    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    eng = TrackEngine(model="lepton3", device=0)
    dev = GraphDevice(eng, plan)
    ref = torch_model(g, eng.device)
    stream = torch.cuda.ExternalStream(eng.lib.cpx_stream(eng.h), device=eng.device)
    out = {"model": "inception_v3 width %.2f 160x160x3" % args.width, "gflop_per_sample": flops / 1e9,
           "arena_bytes_per_sample": plan.arena_bytes_per_sample, "batches": []}
    rng = np.random.default_rng(0)
    for n in [int(v) for v in args.batches.split(",")]:
        x = torch.from_numpy(rng.uniform(-1, 1, size=(n, 160, 160, 3)).astype(np.float32)).to(eng.device)
        y = torch.empty((n, 17), dtype=torch.float32, device=eng.device)
        x_nchw = x.permute(0, 3, 1, 2).contiguous()
        torch.cuda.synchronize()

        def ours():
            rc = eng.lib.cpx_graph_forward(dev._graph, C.c_void_p(x.data_ptr()), n, C.c_void_p(y.data_ptr()))
            assert rc == 0, eng._err()

        with torch.cuda.stream(stream):
            ms = timed(torch, ours, args.steps, args.warmup)
        rec = {"N": n, "ms": ms, "samples_per_s": n / ms * 1e3, "tflops": flops * n / ms / 1e9}
        if not args.skip_torch:
            with torch.no_grad():
                ms_ref = timed(torch, lambda: ref(x_nchw), args.steps, args.warmup)
                err = float((ref(x_nchw) - y).abs().max())
            rec.update({"torch_ms": ms_ref, "torch_samples_per_s": n / ms_ref * 1e3, "ratio_vs_torch": ms_ref / ms,
                        "max_abs_diff_vs_torch": err})
        out["batches"].append(rec)
    # (the per-kernel-kind split of the TIME: --kernel-trace, from a run under rocprofv3)
    kinds = {}
    for o in plan.ops:
        kinds[KIND_NAMES[o.kind]] = kinds.get(KIND_NAMES[o.kind], 0) + 1
    out["launches_by_kind"] = kinds
    dev.close()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
