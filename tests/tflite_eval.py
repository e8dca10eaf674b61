"""Helper (not a test): a straight operator-by-operator evaluation of a tflite_reader.Graph on PyTorch-CPU, float64 by
default.  It reads the Graph only -- nothing of cpx/ml_tools/tflite_graph.py -- so that a mistake of the planner (shapes,
padding, folding, placement) cannot cancel out against it."""
import numpy as np
import torch
import torch.nn.functional as F


def _pads(size, k, s, padding):
    """TensorFlow: SAME gives ceil(size / s) outputs, the surplus padding bottom / right; VALID none."""
    if padding == 1:
        return 0, 0
    out = (size + s - 1) // s
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def _act(x, code):
    if code == 1:
        return torch.relu(x)
    if code == 3:
        return torch.clamp(x, 0.0, 6.0)
    assert code == 0, code
    return x


def evaluate(g, x_nhwc, dtype=torch.float64, magnitudes=False):
    """-> {tensor id: numpy array in TFLite's layout (NHWC / [N, C])} of every activation.  magnitudes=True: also
    {tensor id of a CONV_2D / FULLY_CONNECTED output: sum |x| |w| + |b|}, the scale of its rounding error."""
    val = {g.inputs[0]: torch.as_tensor(np.asarray(x_nhwc), dtype=dtype)}
    mag = {}

    def get(t):
        if t in val:
            return val[t]
        return torch.as_tensor(np.array(g.const(t)), dtype=dtype if g.tensors[t]["type"] == 0 else torch.int64)

    for op in g.ops:
        name, ins = op["name"], [t for t in op["inputs"] if t >= 0]
        a = get(ins[0])
        if name == "CONV_2D":
            w = get(ins[1])                      # OHWI
            b = get(ins[2]) if len(ins) > 2 else None
            kh, kw = w.shape[1], w.shape[2]
            sh, sw = op.get("stride_h", 1), op.get("stride_w", 1)
            pt, pb = _pads(a.shape[1], kh, sh, op.get("padding", 0))
            pl, pr = _pads(a.shape[2], kw, sw, op.get("padding", 0))
            xin = F.pad(a.permute(0, 3, 1, 2), (pl, pr, pt, pb))
            groups = a.shape[3] // w.shape[3]
            y = F.conv2d(xin, w.permute(0, 3, 1, 2), b, stride=(sh, sw), groups=groups)
            if magnitudes:
                mag[op["outputs"][0]] = F.conv2d(xin.abs(), w.permute(0, 3, 1, 2).abs(), None if b is None else b.abs(),
                                                 stride=(sh, sw), groups=groups).permute(0, 2, 3, 1).numpy()
            r = _act(y, op.get("act", 0)).permute(0, 2, 3, 1)
        elif name in ("MAX_POOL_2D", "AVERAGE_POOL_2D"):
            kh, kw, sh, sw = op["filter_height"], op["filter_width"], op["stride_h"], op["stride_w"]
            pt, pb = _pads(a.shape[1], kh, sh, op["padding"])
            pl, pr = _pads(a.shape[2], kw, sw, op["padding"])
            xin = a.permute(0, 3, 1, 2)
            if name == "MAX_POOL_2D":
                y = F.max_pool2d(F.pad(xin, (pl, pr, pt, pb), value=float("-inf")), (kh, kw), (sh, sw))
            else:
                ones = torch.ones((1, 1, kh, kw), dtype=dtype)
                c = xin.shape[1]
                s = F.conv2d(F.pad(xin, (pl, pr, pt, pb)), ones.expand(c, 1, kh, kw), stride=(sh, sw), groups=c)
                cnt = F.conv2d(F.pad(torch.ones_like(xin[:1, :1]), (pl, pr, pt, pb)), ones, stride=(sh, sw))
                y = s / cnt                     # the divisor counts the in-bounds elements only
            r = _act(y, op.get("act", 0)).permute(0, 2, 3, 1)
        elif name in ("ADD", "SUB", "MUL"):
            b = get(ins[1])
            r = _act(a + b if name == "ADD" else a - b if name == "SUB" else a * b, op.get("act", 0))
        elif name == "RELU":
            r = torch.relu(a)
        elif name == "RELU6":
            r = torch.clamp(a, 0.0, 6.0)
        elif name == "CONCATENATION":
            r = _act(torch.cat([get(t) for t in ins], dim=op.get("axis", 0)), op.get("act", 0))
        elif name == "MEAN":
            r = a.mean(dim=tuple(int(v) for v in op["axes"]), keepdim=op["keep_dims"])
        elif name == "FULLY_CONNECTED":
            w = get(ins[1])
            b = get(ins[2]) if len(ins) > 2 else None
            flat = a.reshape(a.shape[0], -1)
            r = _act(F.linear(flat, w, b), op.get("act", 0))
            if magnitudes:
                mag[op["outputs"][0]] = F.linear(flat.abs(), w.abs(), None if b is None else b.abs()).numpy()
        elif name == "LOGISTIC":
            r = torch.sigmoid(a)
        elif name == "SOFTMAX":
            r = torch.softmax(op.get("beta", 1.0) * a, dim=-1)
        elif name == "RESHAPE":
            shp = [int(v) for v in (get(ins[1]) if len(ins) > 1 else op["new_shape"])]
            r = a.reshape([a.shape[0]] + shp[1:])
        elif name == "PAD":
            (_, _), (t0, t1), (l0, l1), (_, _) = op["paddings"]
            r = F.pad(a.permute(0, 3, 1, 2), (l0, l1, t0, t1)).permute(0, 2, 3, 1)
        else:
            raise NotImplementedError(name)
        val[op["outputs"][0]] = r.contiguous()
    out = {k: v.numpy() for k, v in val.items()}
    return (out, mag) if magnitudes else out
