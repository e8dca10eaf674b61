"""Helper (not a test): the hybrid arithmetic of a GROUPED dynamic-range quantised CONV_2D (include/cpx.h,
CPX_GRAPH_CONV_Q8_GROUPED) restated in NumPy / PyTorch-CPU on tflite_eval_q8's quant_params, quantise_input and _finish,
and a whole-graph evaluate_hybrid that accepts grouped filters.  It reads the tflite_reader.Graph only.  The input tensor
is quantised ONCE per sample, over all its channels, before the groups are walked (per_group=False); per_group=True gives
every group parameters of its own channels -- the arithmetic the device must NOT compute, for tests that show their
inputs tell the two apart.  The float64 yardstick of a grouped float32 graph is tflite_eval.evaluate, which handles
groups already."""
import numpy as np
import torch
import torch.nn.functional as F

import tflite_eval as te
import tflite_eval_q8 as tq8


def hybrid_conv_grouped(op, x, ten, bias, per_group=False):
    """-> (float32 value, float64 magnitude); the groups follow from the filter's depth: G = x C / filter I."""
    w = ten["const"]                       # int8 OHWI, I = Cin / G
    x = np.asarray(x, np.float32)
    G = x.shape[3] // w.shape[3]
    assert G * w.shape[3] == x.shape[3] and w.shape[0] % G == 0, (x.shape, w.shape)
    if per_group and G > 1:
        cg, cog = w.shape[3], w.shape[0] // G
        sc = tq8._scales(ten)
        shift = np.zeros(w.shape[0], np.float32) if bias is None else np.asarray(bias, np.float32).reshape(-1)
        parts = []
        for k in range(G):
            sub = dict(ten, const=w[k * cog:(k + 1) * cog], shape=[cog] + list(w.shape[1:]),
                       quant=dict(ten["quant"], scale=sc[k * cog:(k + 1) * cog]))
            parts.append(hybrid_conv_grouped(op, x[..., k * cg:(k + 1) * cg], sub, shift[k * cog:(k + 1) * cog]))
        return np.concatenate([p[0] for p in parts], axis=3), np.concatenate([p[1] for p in parts], axis=3)
    sx, inv, zp = tq8.quant_params(x)      # the whole tensor, all groups
    qz = tq8.quantise_input(x, inv, zp) - zp.reshape(-1, 1, 1, 1).astype(np.float64)
    kh, kw = w.shape[1], w.shape[2]
    sh, sw = op.get("stride_h", 1), op.get("stride_w", 1)
    pt, pb = te._pads(x.shape[1], kh, sh, op.get("padding", 0))
    pl, pr = te._pads(x.shape[2], kw, sw, op.get("padding", 0))
    xin = F.pad(torch.from_numpy(qz).permute(0, 3, 1, 2), (pl, pr, pt, pb))
    acc_z = F.conv2d(xin, torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2), stride=(sh, sw), groups=G)
    acc_z = acc_z.permute(0, 2, 3, 1).numpy()
    shift = np.zeros(w.shape[0], np.float32) if bias is None else np.asarray(bias, np.float32).reshape(-1)
    return tq8._finish(acc_z, sx, tq8._scales(ten), shift, op.get("act", 0))


def evaluate_hybrid(g, x_nhwc, per_group=False):
    """tflite_eval_q8.evaluate_hybrid with grouped filters -> ({tensor id: float32 array}, {tensor id of a hybrid output:
    float64 magnitude})."""
    val = {g.inputs[0]: np.asarray(x_nhwc, np.float32)}
    mag = {}
    for op in g.ops:
        ins = [t for t in op["inputs"] if t >= 0]
        ten = g.quantised_filter(op)
        y = op["outputs"][0]
        if ten is not None:
            bias = g.const(ins[2]) if len(ins) > 2 else None
            if op["name"] == "CONV_2D":
                val[y], mag[y] = hybrid_conv_grouped(op, val[ins[0]], ten, bias, per_group=per_group)
            else:
                val[y], mag[y] = tq8.hybrid_fc(op, val[ins[0]], ten, bias)
        else:
            shim = tq8._OneOp(g, op, val)
            val[y] = te.evaluate(shim, val[shim.inputs[0]], dtype=torch.float32)[y]
    return val, mag
